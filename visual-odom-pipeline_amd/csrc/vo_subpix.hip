// Sub-pixel corner refinement: cv2.cornerSubPix (OpenCV 4.4 imgproc/cornersubpix.cpp with getRectSubPix 8u -> 32f), the call that follows
// cv2.goodFeaturesToTrack in OpenCV's own pipeline.  The reference keeps the detector's integer corners (src/extractor/extractor.py:111); with
// vo_set_subpix the resident detections refine them on the device before they become tracks.  tests/subpix_model.py is the definition, and
// the kernel follows it operation by operation (-ffp-contract=off: no product is fused into a sum):
//   mask [wh][ww] f32 (host): (f32)exp((f64)(-y*y)) * (f32)exp((f64)(-x*x)), y = (f32)(i - wy) / (f32)wy; optional zero zone in the middle
//   per corner, cT = input, cI = cT; repeat
//     S = (wh + 2) x (ww + 2) bilinear samples (f32) of level 0 around cI, pixel coordinates clamped to the image (replicate border: the frame
//         store's reflect-101 pad is never read)
//     per window pixel k = i*ww + j: tgx, tgy = central differences of S (f32) as f64, m = mask[k];
//         gxx = tgx*tgx*m, gxy = tgx*tgy*m, gyy = tgy*tgy*m; terms gxx, gxy, gyy, gxx*px + gxy*py, gxy*px + gyy*py   (px = j - wx, py = i - wy)
//     a, b, c, bb1, bb2 = the terms' sums: lane l adds k = l, l + 64, l + 128, l + 192 to 0.0 in that order, then v += shfl_xor(v, 32 .. 1)
//     det = a*c - b*b; |det| <= DBL_EPSILON^2: stop (flag 1)
//     cI2 = (f32)(cI + (c*bb1 - b*bb2, -b*bb1 + a*bb2) * (1 / det)); err = |cI2 - cI|^2 (f32); cI = cI2
//     cI not inside [0, W) x [0, H): stop (flag 2), not counted;  else iters++, go on while iters < max_count && err > eps^2
//   cI further than win from cT on an axis (or not a number): the result is cT (flag 3).  Input not finite or outside the image: unchanged, flag 4.
// One wave per corner, four corners per 256-thread workgroup; the patch (17 x 17 f32, sized for win = 7) lives in the wave's own LDS rows and
// no workgroup barrier is needed.  After the butterfly every lane holds the same five sums, so every exit is taken by the whole wave.
#include "vo_internal.h"

#include <float.h>
#include <math.h>

#define SUBPIX_MAX_WIN 7
#define SUBPIX_PW (2 * SUBPIX_MAX_WIN + 3)                    // patch pitch = its largest width
#define SUBPIX_MAX_PIX ((2 * SUBPIX_MAX_WIN + 1) * (2 * SUBPIX_MAX_WIN + 1))

struct subpix_args {
  const uint8_t* img;          // level 0 of the chosen frame, sequence 0 (padded: interior at (VO_PAD, VO_PAD))
  size_t img_seq;              // pixels per sequence
  int pitch, W, H;
  int wx, wy, max_count;
  float eps2;
  int cap;                     // corner slots per sequence this launch covers
  int xcd_remap;
  float mask[SUBPIX_MAX_PIX];  // [wh][ww], dense
};

__device__ __forceinline__ float subpix_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// orders this wave's LDS writes before its LDS reads (and the reverse): the wave waits for its own LDS traffic, nothing else
__device__ __forceinline__ void subpix_lds_wait() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__device__ __forceinline__ double subpix_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = v + __shfl_xor(v, off);
  return v;
}

// corners / out: sequence-0 rows [n][2] f32, `rows_seq` bytes apart (they may be the same rows: a wave reads its corner before it writes it);
// raw [cap][2] f32, iters [cap] i32, flags [cap] u8: sequence-0 rows `info_seq` bytes apart; counts: per-sequence corner count as the selection
// kernel left it (word 2 of the sequence's st_scalars, 0xFFFFFFFF = none), `counts_seq` bytes apart, or null = all `cap` slots
__global__ void __launch_bounds__(256) k_corner_subpix(subpix_args A, const float* corners, float* out, size_t rows_seq, float* __restrict__ raw,
                                                       int32_t* __restrict__ iters, uint8_t* __restrict__ flags, size_t info_seq,
                                                       const uint32_t* __restrict__ counts, size_t counts_seq) {
  __shared__ float patch[4][SUBPIX_PW * SUBPIX_PW];
  int blk, bseq;
  vo_xcd_assign(blockIdx.y * gridDim.x + blockIdx.x, gridDim.x, A.xcd_remap, blk, bseq);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int pt = blk * 4 + wave;
  int n = A.cap;
  if (counts) {
    const uint32_t nd = vo_seq(counts, counts_seq, bseq)[2];
    n = (nd == 0xFFFFFFFFu) ? 0 : (int)min(nd, (uint32_t)A.cap);
  }
  if (pt >= n) {                 // a slot the detection did not fill: marked in the info rows (vo_subpix_read), its corner row is left alone
    if (counts && pt < A.cap && lane == 0) {
      reinterpret_cast<float2*>(vo_seq(raw, info_seq, bseq))[pt] = make_float2(__builtin_nanf(""), __builtin_nanf(""));
      vo_seq(iters, info_seq, bseq)[pt] = 0; vo_seq(flags, info_seq, bseq)[pt] = 4;
    }
    return;
  }
  const float2 cT = reinterpret_cast<const float2*>(vo_seq(corners, rows_seq, bseq))[pt];
  const float tx = subpix_uniform(cT.x), ty = subpix_uniform(cT.y);
  const float Wf = (float)A.W, Hf = (float)A.H;
  float2* const o_out = reinterpret_cast<float2*>(vo_seq(out, rows_seq, bseq)) + pt;
  float2* const o_raw = reinterpret_cast<float2*>(vo_seq(raw, info_seq, bseq)) + pt;
  int32_t* const o_it = vo_seq(iters, info_seq, bseq) + pt;
  uint8_t* const o_fl = vo_seq(flags, info_seq, bseq) + pt;
  if (!(fabsf(tx) < __builtin_inff() && fabsf(ty) < __builtin_inff() && tx >= 0.f && tx < Wf && ty >= 0.f && ty < Hf)) {
    if (lane == 0) { *o_raw = cT; *o_out = cT; *o_it = 0; *o_fl = 4; }
    return;
  }
  const int ww = 2 * A.wx + 1, wh = 2 * A.wy + 1, npix = ww * wh, pw = ww + 2, nsamp = pw * (wh + 2);
  // this lane's window pixels: k = lane + 64 t
  int cidx[4];
  double mk[4], pxk[4], pyk[4];
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const int k = lane + 64 * t;
    const int i = k / ww, j = k - i * ww;
    cidx[t] = (i + 1) * SUBPIX_PW + (j + 1);
    mk[t] = (k < npix) ? (double)A.mask[min(k, SUBPIX_MAX_PIX - 1)] : 0.0;
    pxk[t] = (double)(j - A.wx); pyk[t] = (double)(i - A.wy);
  }
  const uint8_t* const img = A.img + (size_t)bseq * A.img_seq + (size_t)VO_PAD * A.pitch + VO_PAD;
  float* const S = patch[wave];
  float cx = tx, cy = ty;
  int it = 0, flag = 0;
  for (;;) {
    // ---- the patch around (cx, cy) ----
    const float x0 = cx - (float)((ww + 1) * 0.5), y0 = cy - (float)((wh + 1) * 0.5);
    const float fx = floorf(x0), fy = floorf(y0);
    const int ix = (int)fx, iy = (int)fy;
    const float fa = x0 - fx, fb = y0 - fy;
    const float a11 = (1.f - fa) * (1.f - fb), a12 = fa * (1.f - fb), a21 = (1.f - fa) * fb, a22 = fa * fb;
#pragma unroll
    for (int t = 0; t < 5; t++) {
      const int s = lane + 64 * t;
      if (s < nsamp) {
        const int r = s / pw, q = s - r * pw;
        const int xa = min(max(ix + q, 0), A.W - 1), xb = min(max(ix + q + 1, 0), A.W - 1);
        const int ya = min(max(iy + r, 0), A.H - 1), yb = min(max(iy + r + 1, 0), A.H - 1);
        const uint8_t* const r0 = img + (size_t)ya * A.pitch;
        const uint8_t* const r1 = img + (size_t)yb * A.pitch;
        const float p00 = (float)r0[xa], p01 = (float)r0[xb], p10 = (float)r1[xa], p11 = (float)r1[xb];
        S[r * SUBPIX_PW + q] = ((p00 * a11 + p01 * a12) + p10 * a21) + p11 * a22;
      }
    }
    subpix_lds_wait();
    // ---- the five window sums ----
    double a = 0.0, b = 0.0, c = 0.0, bb1 = 0.0, bb2 = 0.0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
      if (lane + 64 * t < npix) {
        const float* const p = S + cidx[t];
        const double tgx = (double)(p[1] - p[-1]), tgy = (double)(p[SUBPIX_PW] - p[-SUBPIX_PW]);
        const double gxx = tgx * tgx * mk[t], gxy = tgx * tgy * mk[t], gyy = tgy * tgy * mk[t];
        a = a + gxx; b = b + gxy; c = c + gyy;
        bb1 = bb1 + (gxx * pxk[t] + gxy * pyk[t]);
        bb2 = bb2 + (gxy * pxk[t] + gyy * pyk[t]);
      }
    }
    subpix_lds_wait();           // the next fill overwrites what was just read
    a = subpix_wave_sum(a); b = subpix_wave_sum(b); c = subpix_wave_sum(c); bb1 = subpix_wave_sum(bb1); bb2 = subpix_wave_sum(bb2);
    // ---- solve and step: every lane holds the same sums ----
    const double det = a * c - b * b;
    int stop;
    float nx = cx, ny = cy;
    if (fabs(det) <= DBL_EPSILON * DBL_EPSILON) { flag = 1; stop = 1; }
    else {
      const double scale = 1.0 / det;
      nx = (float)((double)cx + c * scale * bb1 - b * scale * bb2);
      ny = (float)((double)cy - b * scale * bb1 + a * scale * bb2);
      const float dx = nx - cx, dy = ny - cy;
      const float err = dx * dx + dy * dy;
      if (!(nx >= 0.f && nx < Wf && ny >= 0.f && ny < Hf)) { flag = 2; stop = 1; }
      else { it++; stop = (it < A.max_count && err > A.eps2) ? 0 : 1; }
    }
    cx = subpix_uniform(nx); cy = subpix_uniform(ny);
    if (__builtin_amdgcn_readfirstlane(stop)) break;
  }
  if (!(fabsf(cx - tx) <= (float)A.wx && fabsf(cy - ty) <= (float)A.wy)) { cx = tx; cy = ty; flag = 3; }
  if (lane == 0) { *o_raw = cT; *o_out = make_float2(cx, cy); *o_it = it; *o_fl = (uint8_t)flag; }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
extern "C" int32_t vo_subpix_default_params(vo_subpix_params* p) {
  if (!p) return VO_E_INVALID;
  p->win_x = p->win_y = 5; p->zero_x = p->zero_y = -1; p->max_count = 40; p->_pad = 0; p->epsilon = 0.001;
  return VO_OK;
}

// every rule that refuses a parameter set on this context; nothing is enqueued
static int32_t subpix_check(vo_ctx* c, const vo_subpix_params* p) {
  VO_CHECK(c, p->win_x >= 1 && p->win_x <= SUBPIX_MAX_WIN && p->win_y >= 1 && p->win_y <= SUBPIX_MAX_WIN, VO_E_INVALID, "win must be 1..7");
  VO_CHECK(c, c->width >= 2 * p->win_x + 5 && c->height >= 2 * p->win_y + 5, VO_E_INVALID, "the image is smaller than 2 * win + 5");
  VO_CHECK(c, p->epsilon == p->epsilon, VO_E_INVALID, "epsilon is not a number");
  return VO_OK;
}

static void subpix_make_args(const vo_ctx* c, const vo_frame& F, const vo_subpix_params* p, int cap, subpix_args& A) {
  A.img = F.img[0]; A.img_seq = c->lvl_px[0]; A.pitch = c->lv[0].pitch; A.W = c->width; A.H = c->height;
  A.wx = p->win_x; A.wy = p->win_y;
  A.max_count = p->max_count < 1 ? 1 : (p->max_count > 100 ? 100 : p->max_count);
  const float e = (float)(p->epsilon > 0.0 ? p->epsilon : 0.0);
  A.eps2 = e * e;
  A.cap = cap;
  A.xcd_remap = (!c->tune.xcd_remap_off && c->batch % 8 == 0) ? 1 : 0;
  const int ww = 2 * A.wx + 1, wh = 2 * A.wy + 1;
  for (int i = 0; i < wh; i++) {
    const float y = (float)(i - A.wy) / (float)A.wy;
    const float vy = (float)exp((double)(-y * y));
    for (int j = 0; j < ww; j++) {
      const float x = (float)(j - A.wx) / (float)A.wx;
      const float vx = (float)exp((double)(-x * x));
      A.mask[i * ww + j] = vy * vx;
    }
  }
  for (int k = ww * wh; k < SUBPIX_MAX_PIX; k++) A.mask[k] = 0.f;
  const int zx = p->zero_x, zy = p->zero_y;
  if (zx >= 0 && zy >= 0 && 2 * zx + 1 < ww && 2 * zy + 1 < wh)
    for (int i = A.wy - zy; i <= A.wy + zy; i++)
      for (int j = A.wx - zx; j <= A.wx + zx; j++) A.mask[i * ww + j] = 0.f;
}

// the kernel over the corner rows `rows` (refined in place); its notes go to c->subpix
static int32_t subpix_launch(vo_ctx* c, hipStream_t q, const subpix_args& A, float* rows, size_t rows_seq, const uint32_t* counts, size_t counts_seq) {
  const vo_side_rows& s = c->subpix;
  hipLaunchKernelGGL(k_corner_subpix, dim3(vo_div_up(A.cap, 4), c->batch), dim3(256), 0, q, A, rows, rows, rows_seq, vo_side_col<float>(s, VO_SUBPIX_RAW),
                     vo_side_col<int32_t>(s, VO_SUBPIX_ITERS), vo_side_col<uint8_t>(s, VO_SUBPIX_FLAGS), s.seq, counts, counts_seq);
  VO_HIP(c, hipGetLastError());
  return VO_OK;
}

extern "C" int32_t vo_corner_subpix(vo_ctx* c, int32_t which, const float* corners, int32_t n, const vo_subpix_params* prm, float* out,
                                    int32_t* iters, uint8_t* flags) {
  if (!c) return VO_E_INVALID;
  vo_subpix_params def;
  if (!prm) { vo_subpix_default_params(&def); prm = &def; }
  return vo_corner_sync(c, __func__, &c->subpix, vo_subpix_reserve, VO_SUBPIX_OUT, which, corners, n, [&] { return subpix_check(c, prm); },
                        [&](const vo_frame& F) {
                          subpix_args A;
                          subpix_make_args(c, F, prm, n, A);
                          return subpix_launch(c, c->stream, A, vo_side_col<float>(c->subpix, VO_SUBPIX_OUT), c->subpix.seq, nullptr, 0);
                        },
                        {{out, VO_SUBPIX_OUT}, {iters, VO_SUBPIX_ITERS}, {flags, VO_SUBPIX_FLAGS}});
}

extern "C" int32_t vo_set_subpix(vo_ctx* c, const vo_subpix_params* prm) {
  if (!c) return VO_E_INVALID;
  if (!prm) { c->subpix_on = false; return VO_OK; }
  { const int32_t r = subpix_check(c, prm); if (r != VO_OK) return r; }
  { const int32_t rr = vo_side_reserve_on_device(c, vo_subpix_reserve); if (rr != VO_OK) return rr; }
  c->subpix_prm = *prm; c->subpix_prm._pad = 0;
  c->subpix_on = true;
  return VO_OK;
}

extern "C" int32_t vo_get_subpix(vo_ctx* c, int32_t* on, vo_subpix_params* prm) {
  return vo_corner_get(c, &vo_ctx::subpix_on, &vo_ctx::subpix_prm, vo_subpix_default_params, on, prm);
}

// (vo_corners_detected) the corners the selection kernel has just left in st_out on q, refined in place against the current frame
int32_t vo_subpix_launch_detected(vo_ctx* c, hipStream_t q, int cap) {
  subpix_args A;
  subpix_make_args(c, c->fr[c->cur], &c->subpix_prm, cap, A);
  return subpix_launch(c, q, A, vo_slab<float>(c, c->off_st_out), c->slab_seq, vo_slab<const uint32_t>(c, c->off_st_scalars), c->slab_seq);
}

extern "C" int32_t vo_subpix_read(vo_ctx* c, float* raw, int32_t* iters, uint8_t* flags, int32_t n) {
  if (!c) return VO_E_INVALID;
  return vo_side_read(c, __func__, c->subpix, "the last detection did not refine", "n exceeds the corners of the last detection", n,
                      {{raw, VO_SUBPIX_RAW}, {iters, VO_SUBPIX_ITERS}, {flags, VO_SUBPIX_FLAGS}});
}
