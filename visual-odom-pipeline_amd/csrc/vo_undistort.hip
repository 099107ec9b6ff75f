// Lens undistortion of every frame that enters the frame store: cv2.undistort(src, K, dist, None, newK) of OpenCV 4.4
// (imgproc/undistort.cpp initUndistortRectifyMap to a fixed-point map, then imgproc/imgwarp.cpp remap INTER_LINEAR, BORDER_CONSTANT 0).
//
// The definition is tests/undistort_model.py.  One float64 map evaluation per output pixel on the HOST (this unit is built contract-off and
// the map uses + - x / and rint only, so it equals numpy bit for bit), quantised to 1/32 pixel; everything behind it is integer:
//   table entry (8 bytes per output pixel, shared by every sequence of the batch):
//     int16 sx, int16 sy     top-left tap, clamped to [-2, w] x [-2, h]
//     uint16 frac            fy5 * 32 + fx5, the two 5-bit fractions
//     uint16 outside         1: the output pixel is 0 (map not finite, or the tap origin beyond the clamp range)
//   sample: the four taps (sx, sy), (sx + 1, sy), (sx, sy + 1), (sx + 1, sy + 1), a tap outside the image reads 0, weights
//     (32 - fx5)(32 - fy5) * 32 ... fx5 fy5 * 32 (sum 32768), dst = (sum + 16384) >> 15.
// k_undistort writes a tight [batch][h][w] staging image that the UNCHANGED level-0 kernels (vo_frame.hip) then read as their raw frame, so
// undistortion precedes the bilateral pre-filter, as a loader would order the two.
#include "vo_internal.h"

#include <math.h>

#include <vector>

// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t und_sample(const uint8_t* __restrict__ raw, int w, int h, uint2 e) {
  if (e.y >> 16) return 0u;                                             // outside: BORDER_CONSTANT 0
  const int sx = (int)(short)(e.x & 0xffffu), sy = (int)(short)(e.x >> 16);
  const uint32_t fx = e.y & 31u, fy = (e.y >> 5) & 31u;
  const bool x0 = sx >= 0 && sx < w, x1 = sx + 1 >= 0 && sx + 1 < w;
  const bool y0 = sy >= 0 && sy < h, y1 = sy + 1 >= 0 && sy + 1 < h;
  const ptrdiff_t o = (ptrdiff_t)sy * w + sx;
  const uint32_t t00 = (x0 && y0) ? raw[o] : 0u, t01 = (x1 && y0) ? raw[o + 1] : 0u;
  const uint32_t t10 = (x0 && y1) ? raw[o + w] : 0u, t11 = (x1 && y1) ? raw[o + w + 1] : 0u;
  const uint32_t s = (32u - fx) * (32u - fy) * t00 + fx * (32u - fy) * t01 + (32u - fx) * fy * t10 + fx * fy * t11;
  return (s * 32u + 16384u) >> 15;                                      // <= 255
}

// `raw`, raw_seq_stride, frame_idx: exactly k_pad_level0's triple (the frame index may come from device memory, so that a captured step
// replays for any frame).  A thread makes 4 consecutive pixels of one output row: 32 bytes of table (the wave reads 2 KB in a row), 16
// byte gathers, one 32-bit store; the threads run over (row, 4-pixel group) pairs in one flat index.  No LDS, no barrier.
__global__ void __launch_bounds__(256) k_undistort(const uint8_t* __restrict__ raw, size_t raw_seq_stride, const int32_t* __restrict__ frame_idx,
                                                   int w, int h, const uint2* __restrict__ tab, uint8_t* __restrict__ dst, int remap) {
  int blk, bseq;
  vo_xcd_assign(blockIdx.z * gridDim.x + blockIdx.x, gridDim.x, remap, blk, bseq);
  const int gpr = (w + 3) / 4;                                          // 4-pixel groups per row
  const unsigned gid = (unsigned)blk * blockDim.x + threadIdx.x;
  const int y = (int)(gid / (unsigned)gpr);
  const int x0 = (int)(gid - (unsigned)y * (unsigned)gpr) * 4;
  if (y >= h) return;
  raw += (size_t)bseq * raw_seq_stride;
  if (frame_idx) raw += (size_t)(*frame_idx) * w * h;
  const size_t o = (size_t)y * w + x0;
  uint8_t* out = dst + (size_t)bseq * w * h + o;
  const uint2* t = tab + o;
  if (x0 + 3 < w) {
    const uint2 e0 = t[0], e1 = t[1], e2 = t[2], e3 = t[3];
    const uint32_t v = und_sample(raw, w, h, e0) | (und_sample(raw, w, h, e1) << 8) | (und_sample(raw, w, h, e2) << 16) |
                       (und_sample(raw, w, h, e3) << 24);
    __builtin_memcpy(out, &v, 4);                                       // one dword store (rows of a width that is no multiple of 4: unaligned)
  } else {
    for (int k = 0; x0 + k < w; k++) out[k] = (uint8_t)und_sample(raw, w, h, t[k]);
  }
}

// ------------------------------------------------------------------------------------------------
// host: the table
// ------------------------------------------------------------------------------------------------
// one axis of the quantisation: q = rint(32 u) (half to even); not finite: outside, stored (-2, 0).  Else q is clamped to +-2^30 (far beyond
// any image), s = q >> 5, f = q & 31, outside when s is not in [-2, len], s stored clamped to that range.
static inline bool und_quant(double u, int len, int& s, int& f) {
  const double q = rint(u * 32.0);
  if (!isfinite(q)) { s = -2; f = 0; return true; }
  const double lim = 1073741824.0;
  const int iq = (int)(q < -lim ? -lim : (q > lim ? lim : q));
  s = iq >> 5; f = iq & 31;
  const bool out = s < -2 || s > len;
  s = s < -2 ? -2 : (s > len ? len : s);
  return out;
}

static void und_build_table(int w, int h, const double* K, const double* d, const double* nK, std::vector<uint64_t>& tab) {
  const double fx = K[0], fy = K[1], cx = K[2], cy = K[3];
  const double k1 = d[0], k2 = d[1], p1 = d[2], p2 = d[3], k3 = d[4], k4 = d[5], k5 = d[6], k6 = d[7];
  tab.resize((size_t)w * h);
  for (int i = 0; i < h; i++)
    for (int j = 0; j < w; j++) {
      const double x = ((double)j - nK[2]) / nK[0], y = ((double)i - nK[3]) / nK[1];
      const double x2 = x * x, y2 = y * y, r2 = x2 + y2, _2xy = 2.0 * x * y;
      const double kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2);
      const double u = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2.0 * x2)) + cx;
      const double v = fy * (y * kr + p1 * (r2 + 2.0 * y2) + p2 * _2xy) + cy;
      int sx, sy, fx5, fy5;
      const bool ox = und_quant(u, w, sx, fx5), oy = und_quant(v, h, sy, fy5);
      tab[(size_t)i * w + j] = (uint64_t)(uint16_t)(int16_t)sx | ((uint64_t)(uint16_t)(int16_t)sy << 16) | ((uint64_t)(fy5 * 32 + fx5) << 32) |
                               ((uint64_t)((ox || oy) ? 1 : 0) << 48);
    }
}

// the stage's enqueue (vo_build_pyramid's chain, vo_ingest_run): the raw frames -> c->d_und on q
void vo_undistort_enqueue(vo_ctx* c, hipStream_t q, const uint8_t* d_raw_img, size_t raw_seq_stride, const int32_t* d_frame_idx, int remap) {
  const int w = c->width, h = c->height;
  hipLaunchKernelGGL(k_undistort, dim3(vo_div_up(vo_div_up(w, 4) * h, 256), 1, c->batch), dim3(256), 0, q, d_raw_img, raw_seq_stride, d_frame_idx,
                     w, h, reinterpret_cast<const uint2*>(c->d_und_tab.get()), c->d_und, remap);
}

extern "C" int32_t vo_set_undistort(vo_ctx* c, const double* K, const double* dist, int32_t n_dist, const double* newK) {
  if (!c) return VO_E_INVALID;
  VO_CHECK(c, K != nullptr, VO_E_INVALID, "K is NULL");
  VO_CHECK(c, n_dist == 0 || n_dist == 4 || n_dist == 5 || n_dist == 8, VO_E_INVALID, "n_dist must be 0, 4, 5 or 8");
  VO_CHECK(c, n_dist == 0 || dist != nullptr, VO_E_INVALID, "dist is NULL");
  const double* nK = newK ? newK : K;
  double d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k = 0; k < n_dist; k++) d[k] = dist[k];
  for (int k = 0; k < 4; k++) VO_CHECK(c, isfinite(K[k]) && isfinite(nK[k]), VO_E_INVALID, "camera matrix entry is not finite");
  for (int k = 0; k < 8; k++) VO_CHECK(c, isfinite(d[k]), VO_E_INVALID, "distortion coefficient is not finite");
  VO_CHECK(c, K[0] > 0 && K[1] > 0 && nK[0] > 0 && nK[1] > 0, VO_E_INVALID, "focal lengths must be positive");
  VO_CHECK(c, c->width <= 32766 && c->height <= 32766, VO_E_CAPACITY, "the map's tap origins are int16");
  VO_HIP(c, hipSetDevice(c->device));
  std::vector<uint64_t> tab;
  und_build_table(c->width, c->height, K, d, nK, tab);
  const size_t px = (size_t)c->width * c->height;
  VO_HIP(c, c->d_und_tab.reserve(px));
  int32_t r = vo_ingest_reserve(c, &c->d_und);
  if (r == VO_OK) r = vo_sync_streams(c);                               // no build in flight reads the table that is replaced
  if (r != VO_OK) return r;
  VO_HIP(c, hipMemcpyAsync(c->d_und_tab, tab.data(), px * sizeof(uint64_t), hipMemcpyHostToDevice, c->stream));
  r = vo_ingest_commit(c, &c->und_on);
  if (r != VO_OK) return r;
  for (int k = 0; k < 4; k++) { c->und_K[k] = K[k]; c->und_newK[k] = nK[k]; }
  for (int k = 0; k < 8; k++) c->und_dist[k] = d[k];
  return VO_OK;
}

extern "C" int32_t vo_clear_undistort(vo_ctx* c) {
  if (!c) return VO_E_INVALID;
  c->und_on = false;                 // enqueued builds have their launches; the buffers stay for the next vo_set_undistort
  c->ingest_gen++;
  return VO_OK;
}

extern "C" int32_t vo_get_undistort(vo_ctx* c, int32_t* on, double* K, double* dist, double* newK) {
  if (!c || !on) return VO_E_INVALID;
  *on = c->und_on ? 1 : 0;
  for (int k = 0; k < 4; k++) { if (K) K[k] = c->und_on ? c->und_K[k] : 0.0; if (newK) newK[k] = c->und_on ? c->und_newK[k] : 0.0; }
  for (int k = 0; k < 8; k++) if (dist) dist[k] = c->und_on ? c->und_dist[k] : 0.0;
  return VO_OK;
}

extern "C" int32_t vo_undistort(vo_ctx* c, const uint8_t* img, int32_t stride, uint8_t* out) {
  if (!c) return VO_E_INVALID;
  return vo_ingest_run(c, {c->und_on, vo_undistort_enqueue, c->d_und}, "no undistortion set (vo_set_undistort)", img, stride, out);
}

extern "C" int32_t vo_undistort_map_read(vo_ctx* c, int16_t* sxy, uint16_t* frac, uint8_t* outside) {
  if (!c) return VO_E_INVALID;
  VO_CHECK(c, c->und_on, VO_E_STATE, "no undistortion set (vo_set_undistort)");
  VO_HIP(c, hipSetDevice(c->device));
  const size_t px = (size_t)c->width * c->height;
  std::vector<uint64_t> tab(px);
  VO_HIP(c, hipStreamSynchronize(c->stream));
  VO_HIP(c, hipMemcpy(tab.data(), c->d_und_tab, px * sizeof(uint64_t), hipMemcpyDeviceToHost));    // what the kernel reads
  for (size_t i = 0; i < px; i++) {
    const uint64_t e = tab[i];
    if (sxy) { sxy[2 * i] = (int16_t)(uint16_t)(e & 0xffffu); sxy[2 * i + 1] = (int16_t)(uint16_t)((e >> 16) & 0xffffu); }
    if (frac) frac[i] = (uint16_t)((e >> 32) & 0xffffu);
    if (outside) outside[i] = (uint8_t)((e >> 48) & 1u);
  }
  return VO_OK;
}
