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

#define BRIEF_CAP 4096                  // corners a Shi-Tomasi launch can put out (ST_OUT_CAP)

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
// c->d_brief, per sequence: desc [cap][32] u8 | in [cap][2] f32 (the synchronous form's corners) | angle [cap] f32 | flags [cap] u8
static inline int brief_cap(const vo_ctx* c) { return c->max_pts > BRIEF_CAP ? c->max_pts : BRIEF_CAP; }
static inline size_t brief_off_in(const vo_ctx* c) { return 32 * (size_t)brief_cap(c); }
static inline size_t brief_off_angle(const vo_ctx* c) { return brief_off_in(c) + sizeof(float) * 2 * (size_t)brief_cap(c); }
static inline size_t brief_off_flags(const vo_ctx* c) { return brief_off_angle(c) + sizeof(float) * (size_t)brief_cap(c); }
static inline size_t brief_seq(const vo_ctx* c) { return (brief_off_flags(c) + (size_t)brief_cap(c) + 15) & ~(size_t)15; }
static inline uint8_t* brief_rows(const vo_ctx* c, size_t off) { return c->d_brief + off; }

static int32_t brief_reserve(vo_ctx* c) {
  if (c->d_brief) return VO_OK;
  VO_HIP(c, hipMalloc((void**)&c->d_brief, brief_seq(c) * (size_t)c->batch));
  return VO_OK;
}

void vo_brief_destroy(vo_ctx* c) {
  if (c->d_brief) (void)hipFree(c->d_brief);
  c->d_brief = nullptr;
}

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

static int32_t brief_launch(vo_ctx* c, hipStream_t q, const vo_frame& F, const int8_t* pattern, int cap, const float* rows, size_t rows_seq,
                            const uint32_t* counts, size_t counts_seq) {
  brief_args A;
  A.img = F.img[0]; A.img_seq = c->lvl_px[0]; A.pitch = c->lv[0].pitch; A.W = c->width; A.H = c->height; A.cap = cap;
  memcpy(A.pat, pattern ? pattern : VO_BRIEF_DEFAULT_PATTERN, 1024);
  hipLaunchKernelGGL(k_brief_describe, dim3(cap, c->batch), dim3(64), 0, q, A, rows, rows_seq, brief_rows(c, 0),
                     reinterpret_cast<float*>(brief_rows(c, brief_off_angle(c))), brief_rows(c, brief_off_flags(c)), brief_seq(c), counts, counts_seq);
  VO_HIP(c, hipGetLastError());
  return VO_OK;
}

static hipError_t brief_d2h(vo_ctx* c, void* h, size_t off, size_t row_bytes) {
  return hipMemcpy2DAsync(h, row_bytes, brief_rows(c, off), brief_seq(c), row_bytes, c->batch, hipMemcpyDeviceToHost, c->stream);
}

extern "C" int32_t vo_brief_compute(vo_ctx* c, int32_t which, const float* corners, int32_t n, const vo_brief_params* prm, const int8_t* pattern,
                                    uint8_t* desc, float* angle, uint8_t* flags) {
  if (!c) return VO_E_INVALID;
  vo_brief_params def;
  if (!prm) { vo_brief_default_params(&def); prm = &def; }
  VO_CHECK(c, which == 0 || which == 1, VO_E_INVALID, "which must be 0 (previous frame) or 1 (current frame)");
  VO_CHECK(c, n >= 0 && n <= c->max_pts, VO_E_INVALID, "n exceeds max_pts");
  { const int32_t r = brief_check(c, prm, pattern); if (r != VO_OK) return r; }
  VO_CHECK(c, c->n_pushed >= (which == 0 ? 2 : 1), VO_E_STATE, "frame not pushed yet");
  if (n == 0) return VO_OK;
  VO_CHECK(c, corners && desc, VO_E_INVALID, "null buffer");
  VO_HIP(c, hipSetDevice(c->device));
  { const int32_t rq = vo_quiesce_side(c); if (rq != VO_OK) return rq; }
  { const int32_t rr = brief_reserve(c); if (rr != VO_OK) return rr; }
  c->brief_n = -1;                        // the rows no longer describe a detection
  const size_t row = sizeof(float) * 2 * (size_t)n;
  VO_HIP(c, hipMemcpy2DAsync(brief_rows(c, brief_off_in(c)), brief_seq(c), corners, row, row, c->batch, hipMemcpyHostToDevice, c->stream));
  { const int32_t r = brief_launch(c, c->stream, c->fr[which == 1 ? c->cur : (c->cur ^ 1)], pattern, n,
                                   reinterpret_cast<const float*>(brief_rows(c, brief_off_in(c))), brief_seq(c), nullptr, 0);
    if (r != VO_OK) return r; }
  VO_HIP(c, brief_d2h(c, desc, 0, 32 * (size_t)n));
  if (angle) VO_HIP(c, brief_d2h(c, angle, brief_off_angle(c), sizeof(float) * (size_t)n));
  if (flags) VO_HIP(c, brief_d2h(c, flags, brief_off_flags(c), (size_t)n));
  VO_HIP(c, hipStreamSynchronize(c->stream));
  return VO_OK;
}

extern "C" int32_t vo_set_brief(vo_ctx* c, const vo_brief_params* prm, const int8_t* pattern) {
  if (!c) return VO_E_INVALID;
  if (!prm) { c->brief_on = false; return VO_OK; }
  { const int32_t r = brief_check(c, prm, pattern); if (r != VO_OK) return r; }
  VO_HIP(c, hipSetDevice(c->device));
  { const int32_t rr = brief_reserve(c); if (rr != VO_OK) return rr; }       // the rows exist before the first enqueue that needs them
  vo_brief_default_params(&c->brief_prm);
  c->brief_prm.n_bits = prm->n_bits;
  memcpy(c->brief_pat, pattern ? pattern : VO_BRIEF_DEFAULT_PATTERN, 1024);  // a launch takes the table by value: steps in flight keep theirs
  c->brief_on = true;
  return VO_OK;
}

extern "C" int32_t vo_get_brief(vo_ctx* c, int32_t* on, vo_brief_params* prm) {
  if (!c || !on) return VO_E_INVALID;
  *on = c->brief_on ? 1 : 0;
  if (prm) { if (c->brief_on) *prm = c->brief_prm; else vo_brief_default_params(prm); }
  return VO_OK;
}

extern "C" int32_t vo_brief_pattern_read(vo_ctx* c, int8_t* out) {
  if (!c || !out) return VO_E_INVALID;
  memcpy(out, c->brief_on ? c->brief_pat : VO_BRIEF_DEFAULT_PATTERN, 1024);
  return VO_OK;
}

// the resident detections' hook: describe the corners the selection kernel has just left in st_out on q, against the current frame
int32_t vo_brief_describe_detected(vo_ctx* c, hipStream_t q, int max_corners) {
  c->brief_n = -1;
  if (!c->brief_on) return VO_OK;
  { const int32_t rr = brief_reserve(c); if (rr != VO_OK) return rr; }
  const int cap = (max_corners > 0 && max_corners < BRIEF_CAP) ? max_corners : BRIEF_CAP;
  const int32_t r = brief_launch(c, q, c->fr[c->cur], c->brief_pat, cap, vo_slab<const float>(c, c->off_st_out), c->slab_seq,
                                 vo_slab<const uint32_t>(c, c->off_st_scalars), c->slab_seq);
  if (r != VO_OK) return r;
  c->brief_n = cap;
  return VO_OK;
}

extern "C" int32_t vo_brief_read(vo_ctx* c, uint8_t* desc, float* angle, uint8_t* flags, int32_t n) {
  if (!c) return VO_E_INVALID;
  VO_CHECK(c, !vo_pipe_busy(c) && c->steps_enq == c->steps_fetched, VO_E_STATE, "steps in flight: fetch them first");
  VO_CHECK(c, c->brief_n >= 0, VO_E_STATE, "the last detection did not describe");
  VO_CHECK(c, n >= 0 && n <= c->brief_n, VO_E_INVALID, "n exceeds the corners of the last detection");
  VO_HIP(c, hipSetDevice(c->device));
  { const int32_t rq = vo_quiesce_side(c); if (rq != VO_OK) return rq; }
  if (n > 0) {
    if (desc) VO_HIP(c, brief_d2h(c, desc, 0, 32 * (size_t)n));
    if (angle) VO_HIP(c, brief_d2h(c, angle, brief_off_angle(c), sizeof(float) * (size_t)n));
    if (flags) VO_HIP(c, brief_d2h(c, flags, brief_off_flags(c), (size_t)n));
  }
  VO_HIP(c, hipStreamSynchronize(c->stream));
  return VO_OK;
}
