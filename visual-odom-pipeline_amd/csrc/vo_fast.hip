// FAST-9/16 corner response: the score cv2.FastFeatureDetector (TYPE_9_16) reports, as a response map for the selection stages of
// vo_shi_tomasi.hip (vo_st_params.fast_threshold > 0).
//
// Definition (tests/fast_model.py): ring offsets (dx, dy), k = 0 .. 15, on the radius-3 Bresenham circle
//     (0,3) (1,3) (2,2) (3,1) (3,0) (3,-1) (2,-2) (1,-3) (0,-3) (-1,-3) (-2,-2) (-3,-1) (-3,0) (-3,1) (-2,2) (-1,3)
// d_k = I(x + dx_k, y + dy_k) - I(x, y);  m = max over the 16 cyclic arcs of 9 consecutive k of max(min_arc d, min_arc -d).
// A pixel with 3 <= x < W - 3, 3 <= y < H - 3 is a corner iff m > t; its score is m - 1, the largest threshold at which it still
// passes the 9-of-16 segment test.  Every other pixel scores 0.  Integer arithmetic throughout; R = (float)score is exact.
//
// One launch, one pass over the image, no LDS beyond the block-maximum exchange:
//   * a thread owns FAST_PX = 4 consecutive pixels of a row and walks FAST_ROWS rows; the 7 image rows of a pixel row arrive as
//     unaligned dwords (level 0 of the frame store carries a VO_PAD border, so no load leaves the allocation);
//   * any arc of 9 holds at least two of the four cardinal ring pixels (k = 0, 4, 8, 12), so a pixel with fewer than two of them
//     brighter than I + t and fewer than two darker than I - t cannot pass: the cardinals come out of 3 of the 7 rows, and where no
//     lane of the wave has such a pixel (flat image regions) the other 4 rows are not loaded and nothing else is computed;
//   * the arc minima / maxima (sliding windows of 2, 4, 8, 9 by doubling) are formed only by lanes whose pixel passed that test, on a
//     ring held in registers: every ring index is a compile-time constant;
//   * R is stored for EVERY pixel, zeros included (k_st_nms reads neighbours and nothing clears the map); the exclusion mask enters
//     only the per-workgroup masked maximum.
#include "vo_internal.h"

#define FAST_PX 4                         // consecutive pixels per thread
#define FAST_ROWS 4                       // rows per thread (a wave owns FAST_ROWS consecutive rows of 256 columns)
#define FAST_COLS (64 * FAST_PX)          // columns per workgroup
#define FAST_TILE_ROWS (4 * FAST_ROWS)    // rows per workgroup (4 waves)

__device__ __forceinline__ uint32_t fast_ld_u32_any(const uint8_t* p) {     // unaligned dword load (one global_load_dword)
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

// byte `o` (compile-time constant after unrolling) of a row window held as consecutive dwords
__device__ __forceinline__ int fast_byte(const uint32_t* w, int o) { return (int)((w[o >> 2] >> ((o & 3) * 8)) & 0xFFu); }

// m of pixel P of the thread's run.  Windows: w0 = row y, u1 / m1 = rows y + 1 / y - 1 (all three start at column x0 - 3), u2 / m2 = rows
// y + 2 / y - 2 (start x0 - 2), u3 / m3 = rows y + 3 / y - 3 (start x0 - 1)
template <int P>
__device__ __forceinline__ int fast_arc_max(const uint32_t (&w0)[3], const uint32_t (&u1)[3], const uint32_t (&m1)[3], const uint32_t (&u2)[2],
                                            const uint32_t (&m2)[2], const uint32_t (&u3)[2], const uint32_t (&m3)[2]) {
  const int c = fast_byte(w0, P + 3);
  int d[16];
  d[0] = fast_byte(u3, P + 1) - c;  d[1] = fast_byte(u3, P + 2) - c;  d[2] = fast_byte(u2, P + 4) - c;  d[3] = fast_byte(u1, P + 6) - c;
  d[4] = fast_byte(w0, P + 6) - c;  d[5] = fast_byte(m1, P + 6) - c;  d[6] = fast_byte(m2, P + 4) - c;  d[7] = fast_byte(m3, P + 2) - c;
  d[8] = fast_byte(m3, P + 1) - c;  d[9] = fast_byte(m3, P + 0) - c;  d[10] = fast_byte(m2, P + 0) - c; d[11] = fast_byte(m1, P + 0) - c;
  d[12] = fast_byte(w0, P + 0) - c; d[13] = fast_byte(u1, P + 0) - c; d[14] = fast_byte(u2, P + 0) - c; d[15] = fast_byte(u3, P + 0) - c;
  // sliding minima and maxima over 2, 4, 8 and 9 consecutive ring pixels; max_arcs min(-d) = -min_arcs max(d)
  int lo2[16], hi2[16], lo4[16], hi4[16];
#pragma unroll
  for (int k = 0; k < 16; k++) { lo2[k] = min(d[k], d[(k + 1) & 15]); hi2[k] = max(d[k], d[(k + 1) & 15]); }
#pragma unroll
  for (int k = 0; k < 16; k++) { lo4[k] = min(lo2[k], lo2[(k + 2) & 15]); hi4[k] = max(hi2[k], hi2[(k + 2) & 15]); }
  int best_lo = -255, best_hi = 255;        // max over arcs of the arc minimum, min over arcs of the arc maximum
#pragma unroll
  for (int k = 0; k < 16; k++) {
    const int lo9 = min(min(lo4[k], lo4[(k + 4) & 15]), d[(k + 8) & 15]);
    const int hi9 = max(max(hi4[k], hi4[(k + 4) & 15]), d[(k + 8) & 15]);
    best_lo = max(best_lo, lo9); best_hi = min(best_hi, hi9);
  }
  return max(best_lo, -best_hi);
}

// grid (column blocks of FAST_COLS, row blocks of FAST_TILE_ROWS, batch); R and mask [batch][H][W]; blockmax [batch][gridDim.x * gridDim.y]
__global__ void __launch_bounds__(256) k_fast_score(const uint8_t* __restrict__ img, size_t img_seq_px, int pitch, int W, int H, int t,
                                                    const uint8_t* __restrict__ mask, float* __restrict__ R, float* __restrict__ blockmax) {
  __shared__ int s_m[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = ((int)blockIdx.x * 64 + lane) * FAST_PX;
  const int bseq = blockIdx.z;
  const size_t np = (size_t)W * H;
  img += (size_t)bseq * img_seq_px; mask += (size_t)bseq * np; R += (size_t)bseq * np;
  const int xc = x0 < W ? x0 : 0;            // lanes past the row's end load from a valid column and keep nothing
  int lmax = 0;
#pragma unroll 1
  for (int k = 0; k < FAST_ROWS; k++) {
    const int y = (int)blockIdx.y * FAST_TILE_ROWS + wave * FAST_ROWS + k;      // (wave-uniform)
    if (y >= H) break;
    int sc[FAST_PX];
#pragma unroll
    for (int p = 0; p < FAST_PX; p++) sc[p] = 0;
    if (y >= 3 && y < H - 3) {
      const uint8_t* const c0 = img + (size_t)(y + VO_PAD) * pitch + (xc + VO_PAD);
      uint32_t w0[3], u3[2], m3[2];
      w0[0] = fast_ld_u32_any(c0 - 3); w0[1] = fast_ld_u32_any(c0 + 1); w0[2] = fast_ld_u32_any(c0 + 5);
      u3[0] = fast_ld_u32_any(c0 + 3 * pitch - 1); u3[1] = fast_ld_u32_any(c0 + 3 * pitch + 3);
      m3[0] = fast_ld_u32_any(c0 - 3 * pitch - 1); m3[1] = fast_ld_u32_any(c0 - 3 * pitch + 3);
      unsigned cm = 0;                       // bit p: pixel p may pass the segment test
#pragma unroll
      for (int p = 0; p < FAST_PX; p++) {
        const int c = fast_byte(w0, p + 3);
        const int d0 = fast_byte(u3, p + 1) - c, d4 = fast_byte(w0, p + 6) - c, d8 = fast_byte(m3, p + 1) - c, d12 = fast_byte(w0, p) - c;
        const int nb = (d0 > t) + (d4 > t) + (d8 > t) + (d12 > t), nd = (d0 < -t) + (d4 < -t) + (d8 < -t) + (d12 < -t);
        const bool inside = (x0 + p >= 3) && (x0 + p < W - 3);
        cm |= (inside && (nb >= 2 || nd >= 2)) ? (1u << p) : 0u;
      }
      if (__ballot(cm != 0)) {               // (wave-uniform) some lane holds a possible corner: the other four rows
        uint32_t u1[3], m1[3], u2[2], m2[2];
        u1[0] = fast_ld_u32_any(c0 + pitch - 3); u1[1] = fast_ld_u32_any(c0 + pitch + 1); u1[2] = fast_ld_u32_any(c0 + pitch + 5);
        m1[0] = fast_ld_u32_any(c0 - pitch - 3); m1[1] = fast_ld_u32_any(c0 - pitch + 1); m1[2] = fast_ld_u32_any(c0 - pitch + 5);
        u2[0] = fast_ld_u32_any(c0 + 2 * pitch - 2); u2[1] = fast_ld_u32_any(c0 + 2 * pitch + 2);
        m2[0] = fast_ld_u32_any(c0 - 2 * pitch - 2); m2[1] = fast_ld_u32_any(c0 - 2 * pitch + 2);
        int m;
        if (cm & 1u) { m = fast_arc_max<0>(w0, u1, m1, u2, m2, u3, m3); sc[0] = m > t ? m - 1 : 0; }
        if (cm & 2u) { m = fast_arc_max<1>(w0, u1, m1, u2, m2, u3, m3); sc[1] = m > t ? m - 1 : 0; }
        if (cm & 4u) { m = fast_arc_max<2>(w0, u1, m1, u2, m2, u3, m3); sc[2] = m > t ? m - 1 : 0; }
        if (cm & 8u) { m = fast_arc_max<3>(w0, u1, m1, u2, m2, u3, m3); sc[3] = m > t ? m - 1 : 0; }
      }
    }
    if (x0 < W) {
      const size_t o = (size_t)y * W + x0;
      if (x0 + FAST_PX <= W) {
        const float v[FAST_PX] = {(float)sc[0], (float)sc[1], (float)sc[2], (float)sc[3]};
        __builtin_memcpy(R + o, v, sizeof(v));
        const uint32_t mk = fast_ld_u32_any(mask + o);
#pragma unroll
        for (int p = 0; p < FAST_PX; p++) if ((mk >> (8 * p)) & 0xFFu) lmax = max(lmax, sc[p]);
      } else {
#pragma unroll
        for (int p = 0; p < FAST_PX; p++)
          if (x0 + p < W) { R[o + p] = (float)sc[p]; if (mask[o + p]) lmax = max(lmax, sc[p]); }
      }
    }
  }
  // block max -> one float per workgroup (k_st_nms / k_st_select reduce them; max is order independent)
  for (int o = 32; o > 0; o >>= 1) lmax = max(lmax, __shfl_xor(lmax, o));
  if (lane == 0) s_m[wave] = lmax;
  __syncthreads();
  if (threadIdx.x == 0)
    blockmax[(size_t)bseq * gridDim.x * gridDim.y + blockIdx.y * gridDim.x + blockIdx.x] = (float)max(max(s_m[0], s_m[1]), max(s_m[2], s_m[3]));
}

int vo_fast_n_blockmax(int W, int H) { return vo_div_up(W, FAST_COLS) * vo_div_up(H, FAST_TILE_ROWS); }

void vo_fast_enqueue(vo_ctx* c, hipStream_t q, int t, const uint8_t* d_mask, float* d_R, float* d_blockmax) {
  const int W = c->width, H = c->height;
  hipLaunchKernelGGL(k_fast_score, dim3(vo_div_up(W, FAST_COLS), vo_div_up(H, FAST_TILE_ROWS), c->batch), dim3(256), 0, q, c->fr[c->cur].img[0],
                     c->lvl_px[0], c->lv[0].pitch, W, H, t, d_mask, d_R, d_blockmax);
}
