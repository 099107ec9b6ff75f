// CLAHE contrast equalisation of every frame that enters the frame store: cv2.createCLAHE(clipLimit, tileGridSize).apply(img) of OpenCV 4.4
// (imgproc/clahe.cpp, 8-bit path, histSize 256).
//
// The definition is tests/clahe_model.py (a restatement: no OpenCV source or binary was at hand, parity is with the model).  In short:
//   extension   tiles cut the image when both sides divide; otherwise BOTH sides grow, by tiles_x - w % tiles_x columns and tiles_y - h % tiles_y
//               rows (an axis that divides still grows by a whole tiles_*), BORDER_REFLECT_101; tw = ext_w / tiles_x, th = ext_h / tiles_y
//   clip        clip_limit > 0: max((int)(clip_limit * area / 256), 1); clip_limit == 0: none
//   per tile    hist[256]; excess above clip summed, cut, redistributed (clipped / 256 to every bin, the residual one each to bins k * step);
//               lut[i] = clamp(rint((float)prefix[i] * lut_scale), 0, 255), lut_scale = 255.0f / (float)area
//   per pixel   txf = (float)x * inv_tw - 0.5f, tx1 = floor, xa = txf - tx1, xa1 = 1 - xa, then the clamps; the same in y; four LUT values of
//               the pixel's grey level blended in float32, every operation on its own; rint, clamp
// The three float32 divisions (inv_tw, inv_th, lut_scale) are made on the HOST and passed as kernel arguments; the unit is built
// contract-off like the others, so no multiply-add is fused on either side.
//
// Two kernels.  k_clahe_lut: one workgroup per (tile, sequence) -> d_clahe_lut [batch][tiles_y][tiles_x][256] u8.  k_clahe_apply: a thread makes
// 4 pixels of a row -> the tight [batch][h][w] staging image c->d_clahe that the UNCHANGED level-0 kernels (vo_frame.hip) then read as their
// raw frame.  The order of the chain is undistort -> CLAHE -> bilateral pre-filter or plain level 0 -> pyramid.
#include "vo_internal.h"

#include <math.h>

#define CL_MAX_TILES 16
#define CL_COPIES 16           // private histograms per workgroup
#define CL_STRIDE 257          // words between two copies: copy k's bin v lies on bank (k + v) % 32

// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t cl_lut_value(int prefix, float lut_scale) {
  const float r = rintf((float)prefix * lut_scale);
  return (uint32_t)(int)fminf(fmaxf(r, 0.0f), 255.0f);
}

// `raw`, raw_seq_stride, frame_idx: k_pad_level0's triple, as k_undistort takes it.  Workgroup = one tile of one sequence, 256 threads.
// Histogram: LDS atomics into CL_COPIES private copies, copy = thread & 15, CL_STRIDE words apart.  A flat tile (every pixel one grey level --
// the contention worst case and the case where clipping matters) then sends a wave to 16 addresses on 16 different banks, 4 lanes each,
// instead of 64 lanes to one word; thread t afterwards sums bin t over the copies (consecutive lanes, consecutive banks).  The extended image
// is never made: a coordinate beyond the image is reflected (2 n - 2 - x; the host has checked that the extension is smaller than the side).
// Then: excess above the clip (wave sums by shuffle, one LDS add per wave), cut, redistribution in closed form, and wave 0 scans the 256 bins
// four per lane and stores four table bytes per lane.
__global__ void __launch_bounds__(256) k_clahe_lut(const uint8_t* __restrict__ raw, size_t raw_seq_stride, const int32_t* __restrict__ frame_idx,
                                                   int w, int h, int tiles_x, int tw, int th, int clip, float lut_scale,
                                                   uint8_t* __restrict__ lut, int remap) {
  __shared__ int s_hist[CL_COPIES * CL_STRIDE];
  __shared__ __attribute__((aligned(16))) int s_fin[256];
  __shared__ int s_clipped;
  int blk, bseq;
  vo_xcd_assign(blockIdx.z * gridDim.x + blockIdx.x, gridDim.x, remap, blk, bseq);
  const int tid = threadIdx.x;
  for (int i = tid; i < CL_COPIES * CL_STRIDE; i += 256) s_hist[i] = 0;
  if (tid == 0) s_clipped = 0;
  __syncthreads();
  raw += (size_t)bseq * raw_seq_stride;
  if (frame_idx) raw += (size_t)(*frame_idx) * w * h;
  const int ty = blk / tiles_x, tx = blk - ty * tiles_x;
  const int x0 = tx * tw, y0 = ty * th, area = tw * th;
  int* mine = s_hist + (tid & (CL_COPIES - 1)) * CL_STRIDE;
  // the tile's pixels in one flat index, 256 apart per thread: (r, cx) advance without a division
  const int dr = 256 / tw, dc = 256 - dr * tw;
  int r = tid / tw, cx = tid - r * tw;
  for (int i = tid; i < area; i += 256) {
    int x = x0 + cx, y = y0 + r;
    if (x >= w) x = 2 * w - 2 - x;
    if (y >= h) y = 2 * h - 2 - y;
    atomicAdd(&mine[raw[(size_t)y * w + x]], 1);
    cx += dc; r += dr;
    if (cx >= tw) { cx -= tw; r++; }
  }
  __syncthreads();
  int hv = 0;
#pragma unroll
  for (int k = 0; k < CL_COPIES; k++) hv += s_hist[k * CL_STRIDE + tid];
  if (clip > 0) {                                                        // uniform over the workgroup
    int over = max(hv - clip, 0);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) over += __shfl_xor(over, d);
    if ((tid & 63) == 0 && over) atomicAdd(&s_clipped, over);
    __syncthreads();
    const int clipped = s_clipped;
    const int batch = clipped / 256, residual = clipped - 256 * batch;
    hv = min(hv, clip) + batch;
    if (residual != 0) {
      const int step = max(256 / residual, 1);
      const int k = tid / step;
      if (tid - k * step == 0 && k < residual) hv++;
    }
  }
  s_fin[tid] = hv;
  __syncthreads();
  if (tid < 64) {
    const int4 v = reinterpret_cast<const int4*>(s_fin)[tid];            // bins 4 tid .. 4 tid + 3
    const int s = v.x + v.y + v.z + v.w;
    int incl = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int t = __shfl_up(incl, d);
      if (tid >= d) incl += t;
    }
    const int c0 = incl - s + v.x, c1 = c0 + v.y, c2 = c1 + v.z, c3 = c2 + v.w;
    const uint32_t out = cl_lut_value(c0, lut_scale) | (cl_lut_value(c1, lut_scale) << 8) | (cl_lut_value(c2, lut_scale) << 16) |
                         (cl_lut_value(c3, lut_scale) << 24);
    uint8_t* dst = lut + (((size_t)bseq * gridDim.x + blk) << 8);
    reinterpret_cast<uint32_t*>(dst)[tid] = out;                         // a table is 256-byte aligned
  }
}

// one axis of the interpolation: the two tile indices and the two weights, the weights taken before the clamps
__device__ __forceinline__ void cl_axis(int i, float inv, int tiles, int& i1, int& i2, float& a, float& a1) {
  const float f = (float)i * inv - 0.5f;
  const float fl = floorf(f);
  a = f - fl;
  a1 = 1.0f - a;
  const int t = (int)fl;
  i2 = min(t + 1, tiles - 1);
  i1 = max(t, 0);
}

__device__ __forceinline__ uint32_t cl_pixel(const uint8_t* __restrict__ row1, const uint8_t* __restrict__ row2, int x, float inv_tw, int tiles_x,
                                             uint32_t v, float ya, float ya1) {
  int x1, x2; float xa, xa1;
  cl_axis(x, inv_tw, tiles_x, x1, x2, xa, xa1);
  const float p11 = (float)row1[(x1 << 8) + v], p12 = (float)row1[(x2 << 8) + v];
  const float p21 = (float)row2[(x1 << 8) + v], p22 = (float)row2[(x2 << 8) + v];
  const float res = (p11 * xa1 + p12 * xa) * ya1 + (p21 * xa1 + p22 * xa) * ya;
  return (uint32_t)(int)fminf(fmaxf(rintf(res), 0.0f), 255.0f);
}

// A thread makes 4 consecutive pixels of one output row, the threads run over (row, 4-pixel group) pairs in one flat index (k_undistort's
// shape): one 32-bit load of the raw pixels, 16 byte gathers out of the sequence's tables (16 KB at 8 x 8 tiles: they stay in the L1 / L2
// of the XCD the sequence is on, see vo_xcd_assign), one 32-bit store.  No LDS, no barrier.
__global__ void __launch_bounds__(256) k_clahe_apply(const uint8_t* __restrict__ raw, size_t raw_seq_stride, const int32_t* __restrict__ frame_idx,
                                                     int w, int h, int tiles_x, int tiles_y, float inv_tw, float inv_th,
                                                     const uint8_t* __restrict__ lut, uint8_t* __restrict__ dst, int remap) {
  int blk, bseq;
  vo_xcd_assign(blockIdx.z * gridDim.x + blockIdx.x, gridDim.x, remap, blk, bseq);
  const int gpr = (w + 3) / 4;                                          // 4-pixel groups per row
  const unsigned gid = (unsigned)blk * blockDim.x + threadIdx.x;
  const int y = (int)(gid / (unsigned)gpr);
  const int x0 = (int)(gid - (unsigned)y * (unsigned)gpr) * 4;
  if (y >= h) return;
  raw += (size_t)bseq * raw_seq_stride;
  if (frame_idx) raw += (size_t)(*frame_idx) * w * h;
  int y1, y2; float ya, ya1;
  cl_axis(y, inv_th, tiles_y, y1, y2, ya, ya1);
  const uint8_t* seq_lut = lut + (((size_t)bseq * tiles_y * tiles_x) << 8);
  const uint8_t* row1 = seq_lut + (((size_t)y1 * tiles_x) << 8);
  const uint8_t* row2 = seq_lut + (((size_t)y2 * tiles_x) << 8);
  const size_t o = (size_t)y * w + x0;
  uint8_t* out = dst + (size_t)bseq * w * h + o;
  if (x0 + 3 < w) {
    uint32_t p;
    __builtin_memcpy(&p, raw + o, 4);                                   // one dword load (rows of a width that is no multiple of 4: unaligned)
    const uint32_t v = cl_pixel(row1, row2, x0, inv_tw, tiles_x, p & 255u, ya, ya1) |
                       (cl_pixel(row1, row2, x0 + 1, inv_tw, tiles_x, (p >> 8) & 255u, ya, ya1) << 8) |
                       (cl_pixel(row1, row2, x0 + 2, inv_tw, tiles_x, (p >> 16) & 255u, ya, ya1) << 16) |
                       (cl_pixel(row1, row2, x0 + 3, inv_tw, tiles_x, p >> 24, ya, ya1) << 24);
    __builtin_memcpy(out, &v, 4);
  } else {
    for (int k = 0; x0 + k < w; k++) out[k] = (uint8_t)cl_pixel(row1, row2, x0 + k, inv_tw, tiles_x, raw[o + k], ya, ya1);
  }
}

// ------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------
struct cl_geom {
  int tw, th, clip;                 // clip 0: no clipping
  float inv_tw, inv_th, lut_scale;
};

// the geometry of a setting on a w x h image; false: an extension that reflect-101 cannot serve (not smaller than the side)
static bool cl_geometry(int w, int h, double clip_limit, int tiles_x, int tiles_y, cl_geom& g) {
  int ew = w, eh = h;
  if (w % tiles_x != 0 || h % tiles_y != 0) { ew = w + (tiles_x - w % tiles_x); eh = h + (tiles_y - h % tiles_y); }   // both, as OpenCV does
  if (ew - w >= w || eh - h >= h) return false;
  g.tw = ew / tiles_x; g.th = eh / tiles_y;
  const int area = g.tw * g.th;
  g.clip = 0;
  if (clip_limit > 0.0) {
    const double v = clip_limit * area / 256;
    g.clip = v >= (double)area ? area : (int)v;                         // no bin exceeds area: the cap changes nothing and the cast cannot overflow
    if (g.clip < 1) g.clip = 1;
  }
  g.inv_tw = 1.0f / (float)g.tw;
  g.inv_th = 1.0f / (float)g.th;
  g.lut_scale = (float)255 / (float)area;
  return true;
}

// the stage's enqueue (vo_build_pyramid's chain, vo_ingest_run): the raw (or undistorted) frames -> c->d_clahe on q
void vo_clahe_enqueue(vo_ctx* c, hipStream_t q, const uint8_t* d_raw_img, size_t raw_seq_stride, const int32_t* d_frame_idx, int remap) {
  const int w = c->width, h = c->height;
  cl_geom g;
  (void)cl_geometry(w, h, c->cl_clip, c->cl_tx, c->cl_ty, g);            // vo_set_clahe has accepted the setting
  {
    vo_prof_scope prof(c, q, VO_PROF_CLAHE_LUT);
    hipLaunchKernelGGL(k_clahe_lut, dim3(c->cl_tx * c->cl_ty, 1, c->batch), dim3(256), 0, q, d_raw_img, raw_seq_stride, d_frame_idx, w, h, c->cl_tx,
                       g.tw, g.th, g.clip, g.lut_scale, c->d_clahe_lut, remap);
  }
  {
    vo_prof_scope prof(c, q, VO_PROF_CLAHE_APPLY);
    hipLaunchKernelGGL(k_clahe_apply, dim3(vo_div_up(vo_div_up(w, 4) * h, 256), 1, c->batch), dim3(256), 0, q, d_raw_img, raw_seq_stride, d_frame_idx,
                       w, h, c->cl_tx, c->cl_ty, g.inv_tw, g.inv_th, c->d_clahe_lut, c->d_clahe, remap);
  }
}

extern "C" int32_t vo_set_clahe(vo_ctx* c, double clip_limit, int32_t tiles_x, int32_t tiles_y) {
  if (!c) return VO_E_INVALID;
  VO_CHECK(c, isfinite(clip_limit) && clip_limit >= 0.0, VO_E_INVALID, "clip_limit must be finite and >= 0");
  VO_CHECK(c, tiles_x >= 1 && tiles_x <= CL_MAX_TILES && tiles_y >= 1 && tiles_y <= CL_MAX_TILES, VO_E_INVALID, "tiles must be 1 .. 16");
  cl_geom g;
  VO_CHECK(c, cl_geometry(c->width, c->height, clip_limit, tiles_x, tiles_y, g), VO_E_INVALID,
           "the reflect-101 extension to whole tiles is not smaller than the image");
  VO_HIP(c, hipSetDevice(c->device));
  const size_t lut_bytes = (size_t)c->batch * CL_MAX_TILES * CL_MAX_TILES * 256;      // room for every accepted grid
  int32_t r = vo_ingest_reserve(c, &c->d_clahe);
  if (r != VO_OK) return r;
  VO_HIP(c, c->d_clahe_lut.reserve(lut_bytes));
  r = vo_sync_streams(c);                                                // no build in flight runs with the setting that is replaced
  if (r != VO_OK) return r;
  VO_HIP(c, hipMemsetAsync(c->d_clahe_lut, 0, lut_bytes, c->stream));    // vo_clahe_lut_read before the first launch of a setting: zeros
  r = vo_ingest_commit(c, &c->cl_on);
  if (r != VO_OK) return r;
  c->cl_clip = clip_limit; c->cl_tx = tiles_x; c->cl_ty = tiles_y;
  return VO_OK;
}

extern "C" int32_t vo_clear_clahe(vo_ctx* c) {
  if (!c) return VO_E_INVALID;
  c->cl_on = false;                  // enqueued builds have their launches; the buffers stay for the next vo_set_clahe
  c->ingest_gen++;
  return VO_OK;
}

extern "C" int32_t vo_get_clahe(vo_ctx* c, int32_t* on, double* clip_limit, int32_t* tiles_x, int32_t* tiles_y) {
  if (!c || !on) return VO_E_INVALID;
  *on = c->cl_on ? 1 : 0;
  if (clip_limit) *clip_limit = c->cl_on ? c->cl_clip : 0.0;
  if (tiles_x) *tiles_x = c->cl_on ? c->cl_tx : 0;
  if (tiles_y) *tiles_y = c->cl_on ? c->cl_ty : 0;
  return VO_OK;
}

// CLAHE alone: not the undistortion in front of it
extern "C" int32_t vo_clahe(vo_ctx* c, const uint8_t* img, int32_t stride, uint8_t* out) {
  if (!c) return VO_E_INVALID;
  return vo_ingest_run(c, {c->cl_on, vo_clahe_enqueue, c->d_clahe}, "no CLAHE set (vo_set_clahe)", img, stride, out);
}

// lut: [batch][tiles_y][tiles_x][256] of the current setting, as the last launch wrote it
extern "C" int32_t vo_clahe_lut_read(vo_ctx* c, uint8_t* lut) {
  if (!c) return VO_E_INVALID;
  VO_CHECK(c, c->cl_on, VO_E_STATE, "no CLAHE set (vo_set_clahe)");
  VO_CHECK(c, lut != nullptr, VO_E_INVALID, "lut is NULL");
  VO_HIP(c, hipSetDevice(c->device));
  { const int32_t rq = vo_quiesce_side(c); if (rq != VO_OK) return rq; }
  VO_HIP(c, hipStreamSynchronize(c->stream));
  VO_HIP(c, hipMemcpy(lut, c->d_clahe_lut, (size_t)c->batch * c->cl_ty * c->cl_tx * 256, hipMemcpyDeviceToHost));
  return VO_OK;
}
