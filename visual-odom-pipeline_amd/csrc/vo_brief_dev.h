// Device code of the oriented BRIEF descriptor (definition: vo_brief.hip, tests/brief_model.py) shared by its two kernels: k_brief_describe
// (vo_brief.hip, corners of the frame store) and k_orb_describe (vo_orb.hip, keypoints on the levels of the ORB pyramid).
#pragma once
#include "vo_internal.h"

#define BRIEF_M 24                      // margin: 21 + 3
#define BRIEF_TW (2 * BRIEF_M + 1)      // 49: raw tile
#define BRIEF_R 21                      // furthest rotated sample: rint(15 * sqrt(2))
#define BRIEF_SW (2 * BRIEF_R + 1)      // 43: blurred tile

__device__ __constant__ static const unsigned char brief_umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};

__device__ __forceinline__ int brief_wave_sum(int v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// The per-corner body, one wave (64 lanes, all of them call): orientation, blur and the 256 steered tests of the integer pixel (x, y)
// (wave-uniform) of the image whose pixel (0, 0) is at img0, rows `pitch` bytes apart, W x H pixels.  pat: the sampling table [256][4] (read by
// lane); raw [BRIEF_TW * BRIEF_TW + 3] u8, hs [BRIEF_TW * BRIEF_SW + 1] u16, S [BRIEF_SW * BRIEF_SW + 3] u8: the workgroup's LDS.  Returns, in lane t < 4,
// word t of the descriptor, and the angle in `ang`.  A pixel within BRIEF_M of a border reads nothing: word 0, angle 0 (the callers' own margin
// rules never send one).
__device__ __forceinline__ unsigned long long brief_describe_px(const uint8_t* __restrict__ img0, int pitch, int W, int H, int x, int y,
                                                                const int8_t* __restrict__ pat, int lane, uint8_t* raw, uint16_t* hs, uint8_t* S,
                                                                float& ang) {
  ang = 0.f;
  if (x < BRIEF_M || x > W - 1 - BRIEF_M || y < BRIEF_M || y > H - 1 - BRIEF_M) return 0ull;
  // ---- the raw tile: rows y-24 .. y+24, columns x-24 .. x+24, all inside the image ----
  const uint8_t* const img = img0 + (size_t)(y - BRIEF_M) * pitch + (x - BRIEF_M);
  for (int k = lane; k < BRIEF_TW * BRIEF_TW; k += 64) {
    const int r = k / BRIEF_TW, q = k - r * BRIEF_TW;
    raw[k] = img[(size_t)r * pitch + q];
  }
  __syncthreads();
  // ---- orientation: the intensity centroid of the disc of radius 15 ----
  int m10 = 0, m01 = 0;
  for (int k = lane; k < 31 * 31; k += 64) {
    const int r = k / 31, q = k - r * 31;
    const int v = r - 15, u = q - 15;
    if (abs(u) <= (int)brief_umax[abs(v)]) {
      const int I = raw[(v + BRIEF_M) * BRIEF_TW + (u + BRIEF_M)];
      m10 += u * I; m01 += v * I;
    }
  }
  m10 = brief_wave_sum(m10); m01 = brief_wave_sum(m01);
  float c = 1.f, s = 0.f;
  ang = 0.f;
  if (m10 != 0 || m01 != 0) {
    const double dx = (double)m10, dy = (double)m01;
    const double r = sqrt(dx * dx + dy * dy);
    c = (float)(dx / r); s = (float)(dy / r);
    double a = atan2(dy, dx) * (180.0 / 3.14159265358979323846);
    if (a < 0.0) a = a + 360.0;
    ang = (float)a;
    if (ang >= 360.f) ang = 0.f;
  }
  // ---- blur: horizontal sums of the 49 rows over the 43 middle columns, then the vertical pass ----
  for (int k = lane; k < BRIEF_TW * BRIEF_SW; k += 64) {
    const int r = k / BRIEF_SW, q = k - r * BRIEF_SW;
    const uint8_t* const p = raw + r * BRIEF_TW + q;            // tile column q .. q + 6 = centre q + 3
    hs[k] = (uint16_t)(18 * (p[0] + p[6]) + 33 * (p[1] + p[5]) + 49 * (p[2] + p[4]) + 56 * p[3]);
  }
  __syncthreads();
  for (int k = lane; k < BRIEF_SW * BRIEF_SW; k += 64) {
    const int r = k / BRIEF_SW, q = k - r * BRIEF_SW;
    const uint16_t* const p = hs + r * BRIEF_SW + q;            // rows r .. r + 6 = centre r + 3
    const int v = 18 * ((int)p[0] + (int)p[6 * BRIEF_SW]) + 33 * ((int)p[BRIEF_SW] + (int)p[5 * BRIEF_SW]) +
                  49 * ((int)p[2 * BRIEF_SW] + (int)p[4 * BRIEF_SW]) + 56 * (int)p[3 * BRIEF_SW];
    S[k] = (uint8_t)((v + 32768) >> 16);
  }
  __syncthreads();
  // ---- the tests: lane l runs tests l, l + 64, l + 128, l + 192; ballot t is descriptor word t ----
  unsigned long long word = 0ull;
#pragma unroll
  for (int t = 0; t < 4; t++) {
    const char4 p = reinterpret_cast<const char4*>(pat)[t * 64 + lane];
    const float x1 = (float)p.x, y1 = (float)p.y, x2 = (float)p.z, y2 = (float)p.w;
    const int ix1 = (int)rintf(__fsub_rn(__fmul_rn(x1, c), __fmul_rn(y1, s))), iy1 = (int)rintf(__fadd_rn(__fmul_rn(x1, s), __fmul_rn(y1, c)));
    const int ix2 = (int)rintf(__fsub_rn(__fmul_rn(x2, c), __fmul_rn(y2, s))), iy2 = (int)rintf(__fadd_rn(__fmul_rn(x2, s), __fmul_rn(y2, c)));
    // (|ix|, |iy| <= 21 for coordinates in +-15, which the host checked; the clamp keeps a table it did not see inside the tile)
    const int a0 = (min(max(iy1, -BRIEF_R), BRIEF_R) + BRIEF_R) * BRIEF_SW + (min(max(ix1, -BRIEF_R), BRIEF_R) + BRIEF_R);
    const int a1 = (min(max(iy2, -BRIEF_R), BRIEF_R) + BRIEF_R) * BRIEF_SW + (min(max(ix2, -BRIEF_R), BRIEF_R) + BRIEF_R);
    const unsigned long long b = __ballot(S[a0] < S[a1]);
    if (lane == t) word = b;
  }
  return word;
}
