// Oriented BRIEF descriptor at detected corners: the descriptor half of ORB.  The reference's Extractor names it -- cv2.ORB_create() and the
// describe=True branch of extract (src/extractor/extractor.py:30-31, 119-122) -- and its detector half is the FAST response of vo_fast.hip.
// OpenCV's learned sampling table is not part of this project, so parity with cv2.ORB is not pinned: tests/brief_model.py is the definition,
// all-integer or fixed-order IEEE arithmetic, and the kernel equals it bit for bit.  A caller who has OpenCV uploads ORB's own table.
//   corner    (x, y) = (rint(cx), rint(cy)) (half to even) on level 0 of the named frame -- what undistortion, CLAHE and the pre-filter left.
//             M = 24 (21 for the furthest rotated sample + 3 for the blur): described iff M <= x <= w-1-M and M <= y <= h-1-M; else flags = 1,
//             32 zero bytes, angle 0.  A row that is not finite: flags = 2, the same zeros.  No border pixel is ever extrapolated.
//   angle     ORB's IC_Angle on the raw image: m10 = sum u I(x+u, y+v), m01 = sum v I(x+u, y+v) over |v| <= 15, |u| <= umax[|v|],
//             umax = {15,15,15,15,14,14,14,13,13,12,11,10,9,8,6,3}, exact in int32.  Both 0: c = 1, s = 0, angle = 0.  Else in float64
//             r = sqrt(m10*m10 + m01*m01), c = (f32)(m10 / r), s = (f32)(m01 / r); angle = atan2(m01, m10) in degrees in [0, 360) as f32,
//             reported only: it never enters the descriptor (ORB goes through fastAtan2 and cos / sin; this keeps the bits exact).
//   blur      separable 7-tap integer Gaussian g = {18,33,49,56,49,33,18} (sum 256, sigma ~ 2): the horizontal sums fit u16, the vertical
//             pass runs over them, S = (v + 32768) >> 16.  ORB's GaussianBlur(7 x 7, 2) in spirit, not bit for bit.
//   tests     pattern rows (x1, y1, x2, y2) int8 in [-15, 15]; per point in float32 without contraction fx = x1*c - y1*s, fy = x1*s + y1*c
//             (two rounded products, one rounded sum), ix = rint(fx), iy = rint(fy) half to even; bit i = S(x+ix1, y+iy1) < S(x+ix2, y+iy2),
//             stored in byte i / 8 at bit i % 8.
// One wave per corner (a 64-thread workgroup), grid (corners, batch).  The 49 x 49 raw tile goes to LDS once, the blur runs in LDS over the
// 43 x 43 pixels a rotated sample can reach, the moments are a wave butterfly, and the 256 tests are four per lane: four ballots are the
// four 64-bit words of the descriptor.  A per-corner tile instead of a blurred image: a corner is described once in its life and a
// steady-state detection spawns few of them.  The per-corner body, brief_describe_px, lives in vo_brief_dev.h: k_orb_describe of vo_orb.hip runs it on
// the levels of its pyramid.
#include "vo_internal.h"
#include "vo_brief_pattern.h"
#include "vo_brief_dev.h"

#include <math.h>
#include <string.h>

struct brief_args {
  const uint8_t* img;          // level 0 of the chosen frame, sequence 0 (padded: interior at (VO_PAD, VO_PAD))
  size_t img_seq;              // pixels per sequence
  int pitch, W, H;
  int cap;                     // corner slots per sequence this launch covers
  int8_t pat[1024];            // [256][4]
};

// corners: sequence-0 rows [n][2] f32, `rows_seq` bytes apart; desc [cap][32] u8, angle [cap] f32, flags [cap] u8: sequence-0 rows `out_seq`
// bytes apart; counts: per-sequence corner count as the selection kernel left it (word 2 of the sequence's st_scalars, 0xFFFFFFFF = none),
// `counts_seq` bytes apart, or null = all `cap` slots
__global__ void __launch_bounds__(64) k_brief_describe(brief_args A, const float* __restrict__ corners, size_t rows_seq, uint8_t* __restrict__ desc,
                                                       float* __restrict__ angle, uint8_t* __restrict__ flags, size_t out_seq,
                                                       const uint32_t* __restrict__ counts, size_t counts_seq) {
  __shared__ uint8_t raw[BRIEF_TW * BRIEF_TW + 3];
  __shared__ uint16_t hs[BRIEF_TW * BRIEF_SW + 1];
  __shared__ uint8_t S[BRIEF_SW * BRIEF_SW + 3];
  const int pt = blockIdx.x, bseq = blockIdx.y, lane = threadIdx.x;
  if (pt >= A.cap) return;
  int n = A.cap;
  if (counts) {
    const uint32_t nd = vo_seq(counts, counts_seq, bseq)[2];
    n = (nd == 0xFFFFFFFFu) ? 0 : (int)min(nd, (uint32_t)A.cap);
  }
  unsigned long long* const o_desc = reinterpret_cast<unsigned long long*>(vo_seq(desc, out_seq, bseq)) + (size_t)pt * 4;
  float* const o_ang = vo_seq(angle, out_seq, bseq) + pt;
  uint8_t* const o_fl = vo_seq(flags, out_seq, bseq) + pt;
  int flag = 0, x = 0, y = 0;
  if (pt >= n) flag = 2;         // a slot the detection did not fill
  else {
    const float2 cT = reinterpret_cast<const float2*>(vo_seq(corners, rows_seq, bseq))[pt];
    if (!(fabsf(cT.x) < __builtin_inff() && fabsf(cT.y) < __builtin_inff())) flag = 2;
    else {
      const float xr = rintf(cT.x), yr = rintf(cT.y);
      if (!(xr >= (float)BRIEF_M && xr <= (float)(A.W - 1 - BRIEF_M) && yr >= (float)BRIEF_M && yr <= (float)(A.H - 1 - BRIEF_M))) flag = 1;
      else { x = (int)xr; y = (int)yr; }
    }
  }
  flag = __builtin_amdgcn_readfirstlane(flag);
  if (flag) {
    if (lane < 4) o_desc[lane] = 0ull;
    if (lane == 0) { *o_ang = 0.f; *o_fl = (uint8_t)flag; }
    return;
  }
  x = __builtin_amdgcn_readfirstlane(x); y = __builtin_amdgcn_readfirstlane(y);
  float ang;
  const unsigned long long word = brief_describe_px(A.img + (size_t)bseq * A.img_seq + (size_t)VO_PAD * A.pitch + VO_PAD, A.pitch, A.W, A.H, x, y, A.pat,
                                                    lane, raw, hs, S, ang);
  if (lane < 4) o_desc[lane] = word;
  if (lane == 0) { *o_ang = ang; *o_fl = 0; }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
extern "C" int32_t vo_brief_default_pattern(int8_t* out) {
  if (!out) return VO_E_INVALID;
  memcpy(out, VO_BRIEF_DEFAULT_PATTERN, 1024);
  return VO_OK;
}

extern "C" int32_t vo_brief_default_params(vo_brief_params* p) {
  if (!p) return VO_E_INVALID;
  memset(p, 0, sizeof(*p));
  p->n_bits = 256;
  return VO_OK;
}

// every rule that refuses a parameter set or a pattern; nothing is enqueued
static int32_t brief_check(vo_ctx* c, const vo_brief_params* p, const int8_t* pattern) {
  VO_CHECK(c, p->n_bits == 256, VO_E_INVALID, "n_bits must be 256");
  return vo_brief_check_pattern(c, pattern);
}

// (shared with vo_orb_detect_compute) null = the default table
int32_t vo_brief_check_pattern(vo_ctx* c, const int8_t* pattern) {
  if (pattern)
    for (int i = 0; i < 256; i++) {
      const int8_t* r = pattern + 4 * i;
      VO_CHECK(c, r[0] >= -15 && r[0] <= 15 && r[1] >= -15 && r[1] <= 15 && r[2] >= -15 && r[2] <= 15 && r[3] >= -15 && r[3] <= 15, VO_E_INVALID,
               "a pattern coordinate lies outside [-15, 15]");
      VO_CHECK(c, r[0] != r[2] || r[1] != r[3], VO_E_INVALID, "a pattern row's two points are equal");
    }
  return VO_OK;
}

// the kernel over the corner rows `rows`; what it writes goes to c->brief
static int32_t brief_launch(vo_ctx* c, hipStream_t q, const vo_frame& F, const int8_t* pattern, int cap, const float* rows, size_t rows_seq,
                            const uint32_t* counts, size_t counts_seq) {
  const vo_side_rows& s = c->brief;
  brief_args A;
  A.img = F.img[0]; A.img_seq = c->lvl_px[0]; A.pitch = c->lv[0].pitch; A.W = c->width; A.H = c->height; A.cap = cap;
  memcpy(A.pat, pattern ? pattern : VO_BRIEF_DEFAULT_PATTERN, 1024);
  hipLaunchKernelGGL(k_brief_describe, dim3(cap, c->batch), dim3(64), 0, q, A, rows, rows_seq, vo_side_col<uint8_t>(s, VO_BRIEF_DESC),
                     vo_side_col<float>(s, VO_BRIEF_ANGLE), vo_side_col<uint8_t>(s, VO_BRIEF_FLAGS), s.seq, counts, counts_seq);
  VO_HIP(c, hipGetLastError());
  return VO_OK;
}

extern "C" int32_t vo_brief_compute(vo_ctx* c, int32_t which, const float* corners, int32_t n, const vo_brief_params* prm, const int8_t* pattern,
                                    uint8_t* desc, float* angle, uint8_t* flags) {
  if (!c) return VO_E_INVALID;
  vo_brief_params def;
  if (!prm) { vo_brief_default_params(&def); prm = &def; }
  return vo_corner_sync(c, __func__, &c->brief, vo_brief_reserve, VO_BRIEF_IN, which, corners, n, [&] { return brief_check(c, prm, pattern); },
                        [&](const vo_frame& F) {
                          return brief_launch(c, c->stream, F, pattern, n, vo_side_col<const float>(c->brief, VO_BRIEF_IN), c->brief.seq, nullptr, 0);
                        },
                        {{desc, VO_BRIEF_DESC}, {angle, VO_BRIEF_ANGLE}, {flags, VO_BRIEF_FLAGS}});
}

extern "C" int32_t vo_set_brief(vo_ctx* c, const vo_brief_params* prm, const int8_t* pattern) {
  if (!c) return VO_E_INVALID;
  if (!prm) { c->brief_on = false; return VO_OK; }
  { const int32_t r = brief_check(c, prm, pattern); if (r != VO_OK) return r; }
  { const int32_t rr = vo_side_reserve_on_device(c, vo_brief_reserve); if (rr != VO_OK) return rr; }
  vo_brief_default_params(&c->brief_prm);
  c->brief_prm.n_bits = prm->n_bits;
  memcpy(c->brief_pat, pattern ? pattern : VO_BRIEF_DEFAULT_PATTERN, 1024);  // a launch takes the table by value: steps in flight keep theirs
  c->brief_on = true;
  return VO_OK;
}

extern "C" int32_t vo_get_brief(vo_ctx* c, int32_t* on, vo_brief_params* prm) {
  return vo_corner_get(c, &vo_ctx::brief_on, &vo_ctx::brief_prm, vo_brief_default_params, on, prm);
}

extern "C" int32_t vo_brief_pattern_read(vo_ctx* c, int8_t* out) {
  if (!c || !out) return VO_E_INVALID;
  memcpy(out, c->brief_on ? c->brief_pat : VO_BRIEF_DEFAULT_PATTERN, 1024);
  return VO_OK;
}

// (vo_corners_detected) the corners the selection kernel has just left in st_out on q, described against the current frame
int32_t vo_brief_launch_detected(vo_ctx* c, hipStream_t q, int cap) {
  return brief_launch(c, q, c->fr[c->cur], c->brief_pat, cap, vo_slab<const float>(c, c->off_st_out), c->slab_seq,
                      vo_slab<const uint32_t>(c, c->off_st_scalars), c->slab_seq);
}

extern "C" int32_t vo_brief_read(vo_ctx* c, uint8_t* desc, float* angle, uint8_t* flags, int32_t n) {
  if (!c) return VO_E_INVALID;
  return vo_side_read(c, __func__, c->brief, "the last detection did not describe", "n exceeds the corners of the last detection", n,
                      {{desc, VO_BRIEF_DESC}, {angle, VO_BRIEF_ANGLE}, {flags, VO_BRIEF_FLAGS}});
}
