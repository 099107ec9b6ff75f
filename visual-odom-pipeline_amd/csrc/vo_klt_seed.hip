// Pyramidal LK with a caller-supplied start per point: OpenCV's OPTFLOW_USE_INITIAL_FLOW (video/lkpyramid.cpp).  The reference only calls
// cv2.calcOpticalFlowPyrLK(..., flags = 0) (src/extractor/extractor.py:44,65): the top pyramid level starts at the point's previous position.
// Here it starts at a guess g,
//   level == top:  nextPt = g * (float)(1.0 / (1 << top))      (top = the highest level actually used)
// and everything else is the unseeded tracker: template at p0 / 2^level, propagation, skips, exits, status, err, iters.  A guess with a
// component that is not finite starts from p0 (OpenCV leaves that undefined); g == p0 gives k_klt_track's bits.
//   k_klt_seeded      k_klt_track with the guess
//   k_klt_seeded_fb   k_klt_track_fb with the guess for the FORWARD pass; the backward pass LK(cur, prev, p1) starts at p1 as before
// Both are one wave per keypoint around klt_lk_point<true> (vo_klt_lk.h), with k_klt_track's XCD remap and dead-slot rules.  In a translation
// unit of their own: co-compiled kernels perturb each other's register allocation, and k_klt_track / k_klt_track_fb are pinned.
//
// The guesses of the resident paths come from two small predictor kernels (vo_tracks.hip: k_trk_predict, vo_pipeline.hip: k_pipe_predict),
// constant velocity from the track's own history: g = uv + (uv - prev), or uv without a finite prev.  They write c->guess
// [batch][max_pts][2] f32 in the tracker's point order on the tracker's stream, right before the launch here.
#include "vo_klt_lk.h"

#include <math.h>

// the guess of point pt as two wave-uniform floats; not finite -> p0
__device__ __forceinline__ void klt_guess(const float* __restrict__ guess, int pt, float p0x, float p0y, float& gx, float& gy) {
  gx = uniform_f(guess[2 * pt]); gy = uniform_f(guess[2 * pt + 1]);
  if (!(fabsf(gx) < __builtin_inff()) || !(fabsf(gy) < __builtin_inff())) { gx = p0x; gy = p0y; }
}

// WAVES = minimum waves per SIMD the register allocation must allow: one instantiation each, 5 (84 / 90 VGPRs, no scratch).  At 6 the
// allocator's 80 registers leave 12 bytes per lane in scratch: the guess keeps the top level's start apart from the template position
template <int WAVES>
__global__ void __launch_bounds__(64, WAVES) k_klt_seeded(klt_args A, const float* __restrict__ p0, const float* __restrict__ guess, size_t guess_seq,
                                                   float* __restrict__ p1, uint8_t* __restrict__ status, float* __restrict__ err,
                                                   int32_t* __restrict__ iters, const int32_t* __restrict__ counts) {
  int pt = blockIdx.x, bseq = blockIdx.y;
  if (A.xcd_remap) {             // one sequence per XCD (k_klt_track)
    const unsigned id = blockIdx.y * gridDim.x + blockIdx.x;
    const unsigned q = id >> 3;
    bseq = (int)(id & 7u) + 8 * (int)(q / (unsigned)A.n);
    pt = (int)(q % (unsigned)A.n);
  }
  if (pt >= A.n) return;
  const int lane = threadIdx.x;
  if (iters) iters += (size_t)bseq * A.iters_seq;
  const bool dead = counts && pt >= counts[bseq];    // track table: this sequence has fewer live points
  if (iters && lane < A.iters_stride && (dead || lane > A.top)) iters[pt * A.iters_stride + lane] = -1;
  if (dead) return;
  p0 = vo_seq(p0, A.slab_seq, bseq); p1 = vo_seq(p1, A.slab_seq, bseq);
  status = vo_seq(status, A.slab_seq, bseq); err = vo_seq(err, A.slab_seq, bseq);
  guess = vo_seq(guess, guess_seq, bseq);
  const float p0x = uniform_f(p0[2 * pt]), p0y = uniform_f(p0[2 * pt + 1]);
  float gx, gy;
  klt_guess(guess, pt, p0x, p0y, gx, gy);
  float outx, outy, errv;
  int st;
  klt_lk_point<true>(A, A.lv, bseq, pt, lane, p0x, p0y, iters, nullptr, outx, outy, st, errv, gx, gy);
  if (lane == 0) {
    p1[2 * pt] = outx; p1[2 * pt + 1] = outy;
    status[pt] = (uint8_t)st;
    err[pt] = st ? errv : 0.f;
  }
}

template <int WAVES>
__global__ void __launch_bounds__(64, WAVES) k_klt_seeded_fb(klt_args A, klt_fb_args F, const float* __restrict__ p0, const float* __restrict__ guess,
                                                      size_t guess_seq, float* __restrict__ p1, uint8_t* __restrict__ status,
                                                      float* __restrict__ err, int32_t* __restrict__ iters, const int32_t* __restrict__ counts,
                                                      uint8_t* __restrict__ fb) {
  int pt = blockIdx.x, bseq = blockIdx.y;
  if (A.xcd_remap) {             // one sequence per XCD (k_klt_track)
    const unsigned id = blockIdx.y * gridDim.x + blockIdx.x;
    const unsigned q = id >> 3;
    bseq = (int)(id & 7u) + 8 * (int)(q / (unsigned)A.n);
    pt = (int)(q % (unsigned)A.n);
  }
  if (pt >= A.n) return;
  const int lane = threadIdx.x;
  if (iters) iters += (size_t)bseq * A.iters_seq;
  fb += (size_t)bseq * F.fb_seq;
  float* const p0r = reinterpret_cast<float*>(fb);
  float* const fb_err = reinterpret_cast<float*>(fb + F.off_err);
  uint8_t* const ok = fb + F.off_ok;
  const bool dead = counts && pt >= counts[bseq];
  if (iters && lane < A.iters_stride && (dead || lane > A.top)) iters[pt * A.iters_stride + lane] = -1;
  if (dead) {                                        // a dead slot is never good (its check reads as NaN)
    if (lane == 0) { p0r[2 * pt] = p0r[2 * pt + 1] = fb_err[pt] = __builtin_nanf(""); ok[pt] = 0; }
    return;
  }
  p0 = vo_seq(p0, A.slab_seq, bseq); p1 = vo_seq(p1, A.slab_seq, bseq);
  status = vo_seq(status, A.slab_seq, bseq); err = vo_seq(err, A.slab_seq, bseq);
  guess = vo_seq(guess, guess_seq, bseq);
  const float p0x = uniform_f(p0[2 * pt]), p0y = uniform_f(p0[2 * pt + 1]);
  float gx, gy;
  klt_guess(guess, pt, p0x, p0y, gx, gy);
  float outx, outy, errv;
  int st;
  klt_lk_point<true>(A, A.lv, bseq, pt, lane, p0x, p0y, iters, nullptr, outx, outy, st, errv, gx, gy);
  if (lane == 0) {
    p1[2 * pt] = outx; p1[2 * pt + 1] = outy;
    status[pt] = (uint8_t)st;
    err[pt] = st ? errv : 0.f;
  }
  // backward from the tracked position whatever its status, unseeded (k_klt_track_fb)
  float rx, ry, rerr;
  int rst;
  klt_lk_point(A, F.bw, bseq, pt, lane, outx, outy, nullptr, nullptr, rx, ry, rst, rerr);
  if (lane == 0) {
    const float ex = fabsf(p0x - rx), ey = fabsf(p0y - ry);
    const float e = (ex != ex || ey != ey) ? __builtin_nanf("") : (ex >= ey ? ex : ey);     // numpy's max: NaN propagates
    p0r[2 * pt] = rx; p0r[2 * pt + 1] = ry;
    fb_err[pt] = e;
    ok[pt] = (e < F.max_err) ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
// the guesses are the rows of c->guess
void vo_klt_launch_seeded(vo_ctx* c, const klt_launch_rows& L, const klt_args& A, const klt_fb_args* F) {
  const float* const g = vo_side_col<const float>(c->guess, 0);
  if (F) hipLaunchKernelGGL(k_klt_seeded_fb<5>, dim3(L.n, c->batch), dim3(64), 0, L.q, A, *F, L.p0, g, c->guess.seq, L.p1, L.status, L.err,
                            c->d_iters, L.counts, c->fb.d);
  else hipLaunchKernelGGL(k_klt_seeded<5>, dim3(L.n, c->batch), dim3(64), 0, L.q, A, L.p0, g, c->guess.seq, L.p1, L.status, L.err, c->d_iters, L.counts);
}

extern "C" int32_t vo_set_klt_predict(vo_ctx* c, int32_t mode) {
  if (!c) return VO_E_INVALID;
  VO_CHECK(c, mode == VO_KLT_PREDICT_OFF || mode == VO_KLT_PREDICT_CONST_VELOCITY, VO_E_INVALID, "unknown prediction mode");
  if (mode != VO_KLT_PREDICT_OFF) {           // the guess rows exist before the first enqueue that needs them
    const int32_t r = vo_side_reserve_on_device(c, vo_guess_reserve);
    if (r != VO_OK) return r;
  }
  c->klt_predict = mode;
  return VO_OK;
}

extern "C" int32_t vo_get_klt_predict(vo_ctx* c, int32_t* mode) {
  if (!c || !mode) return VO_E_INVALID;
  *mode = c->klt_predict;
  return VO_OK;
}

extern "C" int32_t vo_klt_guess_read(vo_ctx* c, float* guess, int32_t n) {
  if (!c) return VO_E_INVALID;
  return vo_side_read(c, __func__, c->guess, "the last track did not predict", "n exceeds the points of the last track", n, {{guess, 0}}, true);
}
