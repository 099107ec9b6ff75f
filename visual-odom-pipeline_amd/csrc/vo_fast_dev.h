// Device code of the FAST-9/16 score (definition: vo_fast.hip, tests/fast_model.py) shared by its two kernels: k_fast_score (vo_fast.hip, the
// response map of one frame) and k_orb_score (vo_orb.hip, the levels of the ORB pyramid).
#pragma once
#include "vo_internal.h"

#define FAST_PX 4                         // consecutive pixels per thread

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

// The scores of the FAST_PX pixels x0 .. x0 + FAST_PX - 1 of one image row y, 3 <= y < H - 3 (the caller's check), into sc (zero where the
// caller left it zero: a pixel that is no corner, or outside 3 <= x < W - 3, is not written).  c0: the address of pixel (xc, y), xc = x0 or, for
// a lane past the row's end, any valid column; rows are `pitch` bytes apart and columns xc - 3 .. xc + 8 of rows y - 3 .. y + 3 are readable (a
// VO_PAD border).  Holds a ballot: every lane of the wave must call it (the row is wave-uniform).
__device__ __forceinline__ void fast_score_px4(const uint8_t* const c0, int pitch, int x0, int W, int t, int (&sc)[FAST_PX]) {
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
