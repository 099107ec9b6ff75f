// FAST-9/16 corner response: the score cv2.FastFeatureDetector (TYPE_9_16) reports, as a response map for the selection stages of
// vo_shi_tomasi.hip (vo_st_params.fast_threshold > 0).
//
// Definition (tests/fast_model.py): ring offsets (dx, dy), k = 0 .. 15, on the radius-3 Bresenham circle
//     (0,3) (1,3) (2,2) (3,1) (3,0) (3,-1) (2,-2) (1,-3) (0,-3) (-1,-3) (-2,-2) (-3,-1) (-3,0) (-3,1) (-2,2) (-1,3)
// d_k = I(x + dx_k, y + dy_k) - I(x, y);  m = max over the 16 cyclic arcs of 9 consecutive k of max(min_arc d, min_arc -d).
// A pixel with 3 <= x < W - 3, 3 <= y < H - 3 is a corner iff m > t; its score is m - 1, the largest threshold at which it still
// passes the 9-of-16 segment test.  Every other pixel scores 0.  Integer arithmetic throughout; R = (float)score is exact.
//
// One launch, one pass over the image, no LDS beyond the block-maximum exchange (the row body, fast_score_px4, lives in vo_fast_dev.h: k_orb_score
// of vo_orb.hip runs it on the levels of its pyramid):
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
#include "vo_fast_dev.h"

#define FAST_ROWS 4                       // rows per thread (a wave owns FAST_ROWS consecutive rows of 256 columns)
#define FAST_COLS (64 * FAST_PX)          // columns per workgroup
#define FAST_TILE_ROWS (4 * FAST_ROWS)    // rows per workgroup (4 waves)

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
    if (y >= 3 && y < H - 3) fast_score_px4(img + (size_t)(y + VO_PAD) * pitch + (xc + VO_PAD), pitch, x0, W, t, sc);
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
