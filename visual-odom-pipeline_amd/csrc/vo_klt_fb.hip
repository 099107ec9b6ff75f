// Forward-backward consistency check of the pyramidal LK tracker (the standard outlier filter of KLT front ends, and what the reference's
// max_bidir_error promises: src/extractor/extractor.py:44-47,65-68 of the reference, with the image order of the second call fixed, as in
// the OpenCV sample it copies, notebooks/tracking.py:39-42):
//   p1, st, err = LK(prev, cur, p0)      bit for bit what k_klt_track returns
//   p0r         = LK(cur, prev, p1)      template = the CURRENT frame (image + Scharr derivatives, both already in the frame store)
//   fb_err      = max(|p0 - p0r|) over x, y (float32; NaN propagates)      ok = fb_err < max_err (NaN fails)
// k_klt_track_fb runs both passes in ONE launch, one wave per keypoint as k_klt_track: the backward pass starts from the wave's own p1, so
// nothing goes back to memory in between.  Both passes are the same per-level LK body, bound by vector-instruction issue like k_klt_track
// (DESIGN.md 4): the launch costs about two tracker launches.
//
// k_klt_track lives in its own translation unit: co-compiled kernels perturb each other's register allocation.  Both kernels call the one
// per-point LK body, klt_lk_point (vo_klt_lk.h), a function of the level images, so that this kernel can run it twice.
#include "vo_klt_lk.h"

#include <math.h>

// WAVES = minimum waves per SIMD the register allocation must allow: ONE instantiation, 6 (k_klt_track's default; 80 VGPRs, no scratch)
template <int WAVES>
__global__ void __launch_bounds__(64, WAVES) k_klt_track_fb(klt_args A, klt_fb_args F, const float* __restrict__ p0, float* __restrict__ p1,
                                                     uint8_t* __restrict__ status, float* __restrict__ err, int32_t* __restrict__ iters,
                                                     const int32_t* __restrict__ counts, uint8_t* __restrict__ fb) {
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
  const bool dead = counts && pt >= counts[bseq];    // track table: this sequence has fewer live points
  if (iters && lane < A.iters_stride && (dead || lane > A.top)) iters[pt * A.iters_stride + lane] = -1;
  if (dead) {                                        // a dead slot is never good (its check reads as NaN)
    if (lane == 0) { p0r[2 * pt] = p0r[2 * pt + 1] = fb_err[pt] = __builtin_nanf(""); ok[pt] = 0; }
    return;
  }
  p0 = vo_seq(p0, A.slab_seq, bseq); p1 = vo_seq(p1, A.slab_seq, bseq);
  status = vo_seq(status, A.slab_seq, bseq); err = vo_seq(err, A.slab_seq, bseq);

  const float p0x = uniform_f(p0[2 * pt]), p0y = uniform_f(p0[2 * pt + 1]);
  float outx, outy, errv;
  int st;
  klt_lk_point(A, A.lv, bseq, pt, lane, p0x, p0y, iters, nullptr, outx, outy, st, errv);
  if (lane == 0) {
    p1[2 * pt] = outx; p1[2 * pt + 1] = outy;
    status[pt] = (uint8_t)st;
    err[pt] = st ? errv : 0.f;
  }
  // backward from the tracked position whatever its status (the reference hands every p1 to the second call)
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
// the backward pass's argument block for the forward block A (the check's rows must exist: vo_fb_reserve)
void vo_klt_fb_make_args(const vo_ctx* c, const klt_args& A, klt_fb_args& F) {
  const vo_frame& P = c->fr[c->cur ^ 1];
  const vo_frame& C = c->fr[c->cur];
  for (int l = 0; l <= A.top; l++) {
    F.bw[l] = A.lv[l];
    F.bw[l].imgI = C.img[l]; F.bw[l].derI = reinterpret_cast<const uint32_t*>(C.der[l]); F.bw[l].imgJ = P.img[l];
  }
  F.fb_seq = c->fb.seq; F.off_err = c->fb.off[VO_FB_ERR]; F.off_ok = c->fb.off[VO_FB_OK];
  F.max_err = c->fb_max_err;
}

void vo_klt_launch_fb(vo_ctx* c, const klt_launch_rows& L, const klt_args& A, const klt_fb_args& F) {
  hipLaunchKernelGGL(k_klt_track_fb<6>, dim3(L.n, c->batch), dim3(64), 0, L.q, A, F, L.p0, L.p1, L.status, L.err, c->d_iters, L.counts, c->fb.d);
}

extern "C" int32_t vo_set_fb_check(vo_ctx* c, float max_err) {
  if (!c) return VO_E_INVALID;
  VO_CHECK(c, max_err == max_err, VO_E_INVALID, "NaN threshold (+inf turns the check off)");
  if (!(max_err == __builtin_inff())) {       // the rows of the check exist before the first enqueue that needs them
    const int32_t r = vo_side_reserve_on_device(c, vo_fb_reserve);
    if (r != VO_OK) return r;
  }
  c->fb_max_err = max_err;
  return VO_OK;
}

extern "C" int32_t vo_get_fb_check(vo_ctx* c, float* max_err) {
  if (!c || !max_err) return VO_E_INVALID;
  *max_err = c->fb_max_err;
  return VO_OK;
}

extern "C" int32_t vo_fb_read(vo_ctx* c, uint8_t* ok, float* fb_err, int32_t n) {
  if (!c) return VO_E_INVALID;
  return vo_side_read(c, __func__, c->fb, "the last track ran without the forward-backward check", "n exceeds the points of the last track", n,
                      {{ok, VO_FB_OK}, {fb_err, VO_FB_ERR}});
}
