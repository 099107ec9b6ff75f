// Lucas-Kanade pieces shared by the tracker kernels: the argument blocks, the cross-lane sums and the packed bilinear / derivative taps
// (vo_klt.hip: k_klt_track; vo_klt_fb.hip: k_klt_track_fb; vo_klt_seed.hip: their seeded forms; vo_klt_reuse.hip: k_klt_track_r) and, built from them, the per-point LK body
// klt_lk_point that all of them call.
// All of it is inlined into the kernels.  At the end, the host side the three units share: the one launch path and the row copies.
#pragma once
#include "vo_internal.h"

#include <limits.h>

#define W_BITS 14

struct klt_level_args {
  const uint8_t* imgI;    // sequence 0; sequence b at + b * seq_px pixels
  const uint32_t* derI;   // (4 Ix | 4 Iy << 16) per pixel
  const uint8_t* imgJ;
  size_t seq_px;
  int w, h, pitch;
};

struct klt_args {
  klt_level_args lv[VO_MAX_LEVELS];
  size_t slab_seq;        // byte stride between the sequences' point / status / err arrays
  size_t iters_seq;       // int32 stride between the sequences' iteration tables
  int top, win, max_count, n, iters_stride;
  int xcd_remap;             // batch % 8 == 0: keep every sequence on ONE XCD (see k_klt_track)
  float min_eig_num;         // minEig < threshold  <=>  numerator < min_eig_num  (klt_min_eig_numerator: no division per level)
  float eps_lo, eps_hi;      // |delta|^2 in float below / above these decides the convergence test; in between: float64
  double eps2;
};

// the backward pass's levels of the forward-backward kernels: template image + derivatives of the current frame, target = the previous frame
struct klt_fb_args {
  klt_level_args bw[VO_MAX_LEVELS];
  size_t fb_seq;                 // byte stride between the sequences' rows of the check
  size_t off_err, off_ok;        // fb_err and ok rows (p0r at 0)
  float max_err;
};

// Window loads go through buffer instructions: address = descriptor base (the level's image: scalar registers) + ONE per-lane
// offset that is fixed for the level (vector register) + the wave-uniform window origin advanced per row (scalar register).
// With global_load the compiler kept the row advance in vector registers: one v_add per image load and a 64-bit
// v_lshl_add_u64 more per derivative load -- 8 / 24 vector instructions per LK iteration / template in a kernel that is bound
// by vector-instruction issue (tools/vmem_probe.hip).  Unaligned dwords are fine (same rules as global_load).
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t klt_rsrc(const void* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, -1, 0x00020000);   // raw, 4 GB range, no swizzle
}

// every lane receives the value of the lane 16 further up (the same column pair of the next row group; lanes 48..63 wrap
// around to rows that only masked pixels use): ds_bpermute_b32, the LDS crossbar -- no vector-ALU or memory-pipe slot
__device__ __forceinline__ uint32_t row_next(uint32_t v, int lane) {
  return (uint32_t)__builtin_amdgcn_ds_bpermute(((lane + 16) & 63) << 2, (int)v);
}

// exact wave-wide sum of an int32 per lane whose total fits in int32; result uniform
__device__ __forceinline__ int wave_sum_i32(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111 /* row_shr:1 */, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112 /* row_shr:2 */, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114 /* row_shr:4 */, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118 /* row_shr:8 */, 0xf, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142 /* row_bcast:15 */, 0xa, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143 /* row_bcast:31 */, 0xc, 0xf, false);
  return __builtin_amdgcn_readlane(v, 63);
}

// exact wave-wide sum of arbitrary int32 per lane (the total needs up to 36 bits), returned as the float nearest
// to the exact integer: the two 16-bit-split partial sums are combined in float64 (exact, < 2^53) and rounded ONCE,
// which is bit-identical to converting the 64-bit integer sum to float (what the CPU oracle does) and far cheaper
// than the software int64 -> float conversion.
__device__ __forceinline__ float wave_sum_exact_f32(int v) {
  const int lo = wave_sum_i32(v & 0xFFFF);
  const int hi = wave_sum_i32(v >> 16);
  return (float)((double)hi * 65536.0 + (double)lo);
}

// Four (two) wave-wide int32 sums at once as a reduce-scatter: after two quad exchanges lane l holds the quad sum of value
// number l & 3, the remaining steps (row rotations, row swaps) are multiples of 4 lanes and keep that assignment -- 15 + 4
// instructions instead of 4 x 7.  Totals must fit int32 (callers pass 16-bit halves).
template <int CTRL>
__device__ __forceinline__ int klt_dpp(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }

__device__ __forceinline__ int klt_rows_sum(int z) {            // sum over the 16 quads, class (lane & 3) preserved
  z += klt_dpp<0x124>(z);                                       // row_ror:4
  z += klt_dpp<0x128>(z);                                       // row_ror:8
  {
    const auto r = __builtin_amdgcn_permlane16_swap((unsigned)z, (unsigned)z, false, false);
    z = (int)r[0] + (int)r[1];
  }
  {
    const auto r = __builtin_amdgcn_permlane32_swap((unsigned)z, (unsigned)z, false, false);
    z = (int)r[0] + (int)r[1];
  }
  return z;
}

__device__ __forceinline__ void wave_sum4_i32(int a, int b, int c, int d, int lane, int& sa, int& sb, int& sc, int& sd) {
  const bool odd = lane & 1, up = lane & 2;
  const int x = (odd ? b : a) + klt_dpp<0xB1>(odd ? a : b);     // quad_perm [1,0,3,2]: even lanes sum a, odd lanes sum b (pairs)
  const int y = (odd ? d : c) + klt_dpp<0xB1>(odd ? c : d);     //                      even lanes sum c, odd lanes sum d
  int z = (up ? y : x) + klt_dpp<0x4E>(up ? x : y);             // quad_perm [2,3,0,1]: lane & 3 = 0, 1, 2, 3 <-> a, b, c, d (quads)
  z = klt_rows_sum(z);
  sa = __builtin_amdgcn_readlane(z, 0); sb = __builtin_amdgcn_readlane(z, 1);
  sc = __builtin_amdgcn_readlane(z, 2); sd = __builtin_amdgcn_readlane(z, 3);
}

__device__ __forceinline__ void wave_sum2_i32(int a, int b, int lane, int& sa, int& sb) {
  const bool odd = lane & 1;
  int z = (odd ? b : a) + klt_dpp<0xB1>(odd ? a : b);           // even lanes sum a, odd lanes sum b (pairs)
  z += klt_dpp<0x4E>(z);                                        // quads
  z = klt_rows_sum(z);
  sa = __builtin_amdgcn_readlane(z, 0); sb = __builtin_amdgcn_readlane(z, 1);
}

// Two / three wave-wide sums whose QUAD partial sums still fit int32 (callers guarantee |per-lane value| < 2^29): the first
// two butterfly stages run on the full 32-bit values as a reduce-scatter (lane & 1 selects the value), and only the 16 quad
// sums are split into 16-bit halves -- the spare lane class of every quad carries the high halves, so ONE row reduction
// delivers low and high totals of both values (15 vector instructions instead of 21 for the four pre-split halves).
__device__ __forceinline__ void wave_sum2_wide(int a, int b, int lane, int& la, int& ha, int& lb, int& hb) {
  const bool odd = lane & 1, up = lane & 2;
  int z = (odd ? b : a) + klt_dpp<0xB1>(odd ? a : b);           // pairs: even lanes a, odd lanes b
  z += klt_dpp<0x4E>(z);                                        // quads: lanes 0, 2 hold a's quad sum, lanes 1, 3 b's
  int w = up ? (z >> 16) : (z & 0xFFFF);                        // lane & 3 = 0: lo a, 1: lo b, 2: hi a, 3: hi b
  w = klt_rows_sum(w);
  la = __builtin_amdgcn_readlane(w, 0); lb = __builtin_amdgcn_readlane(w, 1);
  ha = __builtin_amdgcn_readlane(w, 2); hb = __builtin_amdgcn_readlane(w, 3);
}

__device__ __forceinline__ void wave_sum3_wide(int a, int b, int c, int lane, int& la, int& ha, int& lb, int& hb, int& lc, int& hc) {
  const bool odd = lane & 1, up = lane & 2;
  const int x = (odd ? b : a) + klt_dpp<0xB1>(odd ? a : b);     // pairs: even lanes a, odd lanes b
  const int y = c + klt_dpp<0xB1>(c);                           // pairs of c in every lane
  const int z = (up ? y : x) + klt_dpp<0x4E>(up ? x : y);       // quads: lane & 3 = 0: a, 1: b, 2 and 3: c
  const int w0 = klt_rows_sum(((lane & 3) == 3) ? (z >> 16) : (z & 0xFFFF));   // lo a, lo b, lo c, hi c
  const int w1 = klt_rows_sum(z >> 16);                                        // hi a, hi b
  la = __builtin_amdgcn_readlane(w0, 0); lb = __builtin_amdgcn_readlane(w0, 1);
  lc = __builtin_amdgcn_readlane(w0, 2); hc = __builtin_amdgcn_readlane(w0, 3);
  ha = __builtin_amdgcn_readlane(w1, 0); hb = __builtin_amdgcn_readlane(w1, 1);
}

// float nearest to the exact integer hi * 2^16 + lo (lo < 2^20).  It fits int32 whenever |hi| < 2^14 -- always, except for
// gross mismatches -- and then ONE v_cvt_f32_i32 rounds it exactly like the float64 route (5 quarter-rate instructions).
__device__ __forceinline__ float klt_combine(int hi, int lo) {
  if ((unsigned)(hi + 16384) < 32768u) return (float)(hi * 65536 + lo);
  return (float)((double)hi * 65536.0 + (double)lo);
}

// cvRound(x) for 0 <= x <= 2^14: adding 1.5 * 2^23 leaves round-to-nearest-even(x) in the low mantissa bits (one float add and one
// integer subtract at full rate instead of v_rndne_f32 + v_cvt_i32_f32 at quarter rate)
__device__ __forceinline__ int klt_round(float x) { return __float_as_int(x + 12582912.f) - 0x4B400000; }

// the four bilinear weights as packed 16-bit pairs wt = iw00 | iw01 << 16, wb = iw10 | iw11 << 16.  The rounded values sit in
// the low 16 bits of the magic-number sums (weights <= 2^14), so the byte gathers take them from there directly
__device__ __forceinline__ void lk_weights(float a, float b, uint32_t& wt, uint32_t& wb) {
  const uint32_t r00 = (uint32_t)__float_as_int((1.f - a) * (1.f - b) * (float)(1 << W_BITS) + 12582912.f);
  const uint32_t r01 = (uint32_t)__float_as_int(a * (1.f - b) * (float)(1 << W_BITS) + 12582912.f);
  const uint32_t r10 = (uint32_t)__float_as_int((1.f - a) * b * (float)(1 << W_BITS) + 12582912.f);
  const uint32_t iw11 = (uint32_t)(1 << W_BITS) + 3u * 0x4B400000u - (r00 + r01 + r10);
  wt = __builtin_amdgcn_perm(r01, r00, 0x05040100u);
  wb = __builtin_amdgcn_perm(iw11, r10, 0x05040100u);
}

__device__ __forceinline__ float uniform_f(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}

typedef short s16x2 __attribute__((ext_vector_type(2)));

// D = a.lo * b.lo + a.hi * b.hi + c  (signed 16-bit halves) -> v_dot2c_i32_i16
__device__ __forceinline__ int dot2(uint32_t a, uint32_t b, int c) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b), c, false);
}
// The same product with the accumulator taken from a THIRD operand (VOP3P v_dot2_i32_i16): hipcc selects the two-address
// v_dot2c form for the plain builtin and then needs a v_mov to preload every rounding constant / zero (16 per LK iteration);
// the clamp bit exists only in the three-address encoding, so asking for it selects that form.  No sum here comes near
// the int32 range (|taps| <= 255 * 2^14), so the saturation never acts and the value is the plain dot product.
__device__ __forceinline__ int dot2k(uint32_t a, uint32_t b, int c) {
  return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b), c, true);
}
// (lo16(a) | lo16(b) << 16) -> one v_perm_b32
__device__ __forceinline__ uint32_t pack_lo(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x05040100u); }
__device__ __forceinline__ uint32_t pack_hi(uint32_t a, uint32_t b) { return __builtin_amdgcn_perm(b, a, 0x07060302u); }
// bytes (k, k+1) of a dword widened to two 16-bit halves
__device__ __forceinline__ uint32_t bytes01(uint32_t t) { return __builtin_amdgcn_perm(0u, t, 0x0c010c00u); }
__device__ __forceinline__ uint32_t bytes12(uint32_t t) { return __builtin_amdgcn_perm(0u, t, 0x0c020c01u); }
__device__ __forceinline__ uint32_t pk_sub(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_bit_cast(s16x2, a) - __builtin_bit_cast(s16x2, b));
}
__device__ __forceinline__ uint32_t pk_abs(uint32_t a) {
  const s16x2 v = __builtin_bit_cast(s16x2, a);
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(v, -v));
}

// bilinear samples (5 fractional bits) of the two pixels a lane owns in one step, packed (v0 | v1 << 16).
// T/B: top / bottom row dwords (3 useful bytes each); wt = iw00 | iw01 << 16, wb = iw10 | iw11 << 16.
__device__ __forceinline__ uint32_t sample2(uint32_t T, uint32_t B, uint32_t wt, uint32_t wb) {
  const int s0 = dot2(bytes01(B), wb, dot2k(bytes01(T), wt, 1 << (W_BITS - 5 - 1)));
  const int s1 = dot2(bytes12(B), wb, dot2k(bytes12(T), wt, 1 << (W_BITS - 5 - 1)));
  // (s >> 9) of both sums packed: bytes 1..2 of each sum are s >> 8 (0 <= s < 2^24), one packed 16-bit shift finishes --
  // two instructions instead of two shifts and a pack
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  const u16x2 h = __builtin_bit_cast(u16x2, __builtin_amdgcn_perm((uint32_t)s1, (uint32_t)s0, 0x06050201u));
  return __builtin_bit_cast(uint32_t, h >> (unsigned short)(W_BITS - 5 - 8));
}
// sample2 in two parts, sample2(T, B, ..) == sample2_combine(sample2_gather(T), sample2_gather(B), ..): the gather widens a row dword to its two
// byte pairs (it depends on the row alone), the combine weighs the pairs of the top and the bottom row.  klt_lk_point<.., REUSE = true> keeps the
// gathered rows while the window stays in one pixel cell.  sample2 itself is not written as that call: the order of the four gathers in the
// source decides the instruction order of the pinned kernels (tests/test_klt_fb_build.py), and their device code is to stay what it is.
__device__ __forceinline__ uint2 sample2_gather(uint32_t T) { return make_uint2(bytes01(T), bytes12(T)); }
__device__ __forceinline__ uint32_t sample2_combine(uint2 t, uint2 b, uint32_t wt, uint32_t wb) {
  const int s0 = dot2(b.x, wb, dot2k(t.x, wt, 1 << (W_BITS - 5 - 1)));
  const int s1 = dot2(b.y, wb, dot2k(t.y, wt, 1 << (W_BITS - 5 - 1)));
  typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
  const u16x2 h = __builtin_bit_cast(u16x2, __builtin_amdgcn_perm((uint32_t)s1, (uint32_t)s0, 0x06050201u));
  return __builtin_bit_cast(uint32_t, h >> (unsigned short)(W_BITS - 5 - 8));
}

// ---- REUSE: the gathered rows of the target window, parked in LDS for as long as the window origin stays in one pixel cell ----
// Row k (0..8: the eight rows a lane loads and the one it takes from the lane 16 further up) of lane l is the pair (bytes01, bytes12) at
// rows[k * 64 + l]: one ds_write_b64 / ds_read_b64 per row at an immediate offset from ONE per-lane address, consecutive lanes on consecutive
// bank pairs.  4608 bytes per one-wave workgroup; a lane reads only what it wrote itself, so there is no barrier.
__device__ __forceinline__ char* klt_rows_lds() {
  __shared__ uint2 rows[9 * 64];
  return reinterpret_cast<char*>(rows);
}
__device__ __forceinline__ uint2 klt_row_read(const char* rows, uint32_t ab, int k) {
  return *reinterpret_cast<const uint2*>(rows + ab + (uint32_t)k * 512u);
}
// what every sampling of klt_lk_point did: eight dword loads, the ninth row from the neighbour lane, the byte gathers -- here into LDS.
// uo: the window origin's pixel offset (wave-uniform)
__device__ __forceinline__ void klt_rows_fetch(char* rows, uint32_t ab, __amdgpu_buffer_rsrc_t rJ, uint32_t lane_off, uint32_t uo, uint32_t pitch, int lane) {
  uint32_t Tj[8];
#pragma unroll
  for (int s = 0; s < 8; s++) Tj[s] = __builtin_amdgcn_raw_buffer_load_b32(rJ, (int)lane_off, (int)(uo + (uint32_t)s * pitch), 0);
  const uint32_t Tj8 = row_next(Tj[0], lane);
#pragma unroll
  for (int k = 0; k < 9; k++) {
    *reinterpret_cast<uint2*>(rows + ab + (uint32_t)k * 512u) = sample2_gather(k < 8 ? Tj[k & 7] : Tj8);
  }
}
// The step loops of a REUSE sampling walk the parked rows two reads ahead of the step that needs them: rows s and s + 1 in registers, row s + 2
// in flight.  Left to itself the compiler issues all nine reads at the head of the loop and the 18 registers they occupy push the 6-wave
// instance into scratch; the empty asm ties the address of the next read to a sum of the step before it (vo_ba_wave.h pins an order the same way).
#define KLT_ROWS_PIN(ab, acc) asm volatile("" : "+v"(ab), "+v"(acc))
// after a fetch the reads go through an address the compiler cannot match with the writes: forwarding the fetched registers past the branch
// splits the 64-bit reads and adds a branch and copies to every sampling
#define KLT_ROWS_OPAQUE(v) asm volatile("" : "+v"(v))

// interpolated derivative of one pixel, times 2^16: top pair / bottom pair already gathered as (left | right << 16).  The
// derivative image holds 4 x Scharr (vo_frame.hip), so the sum is 4 (s + 2^13) and the value OpenCV keeps, (s + 2^13) >> 14, is its
// UPPER HALF: the byte gather that packs two pixels reads it from there (and zeroes masked pixels): one instruction per pixel pair
// instead of two shifts, a pack and a mask
__device__ __forceinline__ uint32_t deriv1(uint32_t top, uint32_t bot, uint32_t wt, uint32_t wb) {
  return (uint32_t)dot2(bot, wb, dot2k(top, wt, 1 << (W_BITS + 1)));
}

// ------------------------------------------------------------------------------------------------
// The per-point LK body of both tracker kernels: ONE WAVE (64 lanes) PER KEYPOINT, template in registers, exact integer arithmetic.
//
// Lane <-> window mapping (window <= 31x31, read footprint 32 rows x 34 bytes):
//   lane = r*16 + cp,  cp = 0..15 (column pair), r = 0..3;  step s = 0..7 covers window row 8r + s,
//   columns 2cp and 2cp+1.  One unaligned dword load per lane per step fetches the 3 bytes the two
//   bilinear footprints need from the top row; the bottom row of step s is the SAME lane's top row of
//   step s + 1 (already in a register, its byte gathers are shared), only step 7 takes it from the
//   lane 16 further up (row group r + 1, step 0: one ds_bpermute per iteration).  => 8 dword loads per
//   lane per LK iteration for a 1 KB window, served by L1/L2 (a pyramid level is <= 0.6 MB; HBM sees it once).
//   The 16 lanes of a row group read 34 CONSECUTIVE bytes, so a load instruction touches 4 rows = 4-8 cache lines and each
//   quad of lanes one line.  (With lane = cp*4 + r -- a quad = four different rows, chosen in round 1 for a one-instruction
//   DPP neighbour exchange -- the texture addresser issued 28 cache accesses per load instruction and was busy 91 % of the
//   kernel: the kernel was bound by it, not by the vector ALUs; profiles/r02_pmc_klt_*.txt.)
//   The template (I, Ix, Iy at 16 pixels per lane) lives in 24 VGPRs across all iterations.
//
// Pyramidal LK of the keypoint (p0x, p0y) (wave-uniform) through levels A.top .. 0 with template lv[l].imgI / derI and target lv[l].imgJ.
// Results are wave-uniform: outx, outy = nextPts, st = status, errv = the error before the status mask.  iters (this sequence's table)
// gets the iterations per level, or null.  dbgk: where the six diagnostic stamps of one wave go (k_klt_track), or null; a literal nullptr folds them away.
// SEEDED (OpenCV's OPTFLOW_USE_INITIAL_FLOW; vo_klt_seed.hip): the top level starts at the guess (gx, gy) (wave-uniform, finite: the callers
// replace a non-finite guess by p0) scaled like p0 instead of at p0 itself; nothing else changes, so (gx, gy) = (p0x, p0y) gives the unseeded
// bits.  The unseeded instantiation does not see the two values.
// REUSE (vo_klt_reuse.hip): inside one level -- its LK loop and, on level 0, the error pass behind it -- the gathered rows of the target window
// stay in LDS together with the integer cell (inx, iny) they were fetched for.  The first sampling of a level fetches; a later one fetches only
// if its cell differs (wave-uniform, compared on the scalar unit), else only the four weights are new.  Nothing carries over to the next level.
// The same bytes go through the same integer sums: the bits of REUSE = false, whose code is textually what it was.
// ------------------------------------------------------------------------------------------------
template <bool SEEDED = false, bool REUSE = false>
__device__ __forceinline__ void klt_lk_point(const klt_args& A, const klt_level_args (&lv)[VO_MAX_LEVELS], int bseq, int pt, int lane,
                                             float p0x, float p0y, int32_t* iters, unsigned long long* dbgk,
                                             float& outx, float& outy, int& st, float& errv, float gx = 0.f, float gy = 0.f) {
  VO_STAMP(dbgk, 0);
  const int cp = lane & 15, r = lane >> 4;
  const int win = A.win;
  const float half = (float)(win - 1) * 0.5f;
  const float FLT_SCALE = 1.f / (float)(1 << 20);

  outx = 0.f; outy = 0.f;   // nextPts[pt]
  st = 1;
  errv = 0.f;

  // validity of the lane's two columns as 16-bit masks (lo = column 2cp, hi = column 2cp + 1)
  const uint32_t colmask = ((2 * cp < win) ? 0x0000FFFFu : 0u) | ((2 * cp + 1 < win) ? 0xFFFF0000u : 0u);
  const uint32_t colones = colmask & 0x00010001u;
  // v_perm selector "upper halves of (a, b)" with the constant-zero code 0x0c for the columns outside the window
  const uint32_t colsel = (0x07060302u & colmask) | (0x0c0c0c0cu & ~colmask);
  char* rows = nullptr;             // REUSE: the parked rows and the lane's byte address in them
  uint32_t rows_ab = 0;
  if constexpr (REUSE) { rows = klt_rows_lds(); rows_ab = (uint32_t)lane * 8u; }

  for (int level = A.top; level >= 0; level--) {
    klt_level_args L = lv[level];
    L.imgI += (size_t)bseq * L.seq_px; L.derI += (size_t)bseq * L.seq_px; L.imgJ += (size_t)bseq * L.seq_px;
    const float scale = __int_as_float((127 - level) << 23);       // 2^-level, exactly what 1.f / (float)(1 << level) gives (no division)
    float prevx = p0x * scale, prevy = p0y * scale;
    float nextx, nexty;
    if (level == A.top) {
      if (SEEDED) { nextx = gx * scale; nexty = gy * scale; }
      else { nextx = prevx; nexty = prevy; }
    }
    else { nextx = outx * 2.f; nexty = outy * 2.f; }
    outx = nextx; outy = nexty;
    int n_it = -1;

    prevx -= half; prevy -= half;
    const float fpx = floorf(prevx), fpy = floorf(prevy);        // (float)(int)floorf(x) == floorf(x): the fraction needs no int -> float convert
    const int ipx = (int)fpx, ipy = (int)fpy;
    if (ipx < -win || ipx >= L.w || ipy < -win || ipy >= L.h) {
      if (level == 0) { st = 0; errv = 0.f; }
      if (iters && lane == 0) iters[pt * A.iters_stride + level] = n_it;
      continue;
    }
    const uint32_t lane_off = (uint32_t)(8 * r * L.pitch + 2 * cp);    // the lane's corner of the 32 x 34 footprint
    uint32_t wt, wb;
    lk_weights(prevx - fpx, prevy - fpy, wt, wb);

    // ---- template: packed pairs of I (5 frac bits), Ix, Iy for the lane's 16 pixels; exact A11, A12, A22 ----
    uint32_t tI[8], tX[8], tY[8];
    {
      uint32_t T[8], D0[8], D1[8], D2[8];
      // addresses = level base (scalar registers) + a 32-bit offset: the wave-uniform window origin, advanced per row on the
      // scalar unit, plus ONE per-lane offset that is fixed for the level (it was a chain of 64-bit vector adds per row)
      const uint32_t uo = (uint32_t)(ipy + VO_PAD) * (uint32_t)L.pitch + (uint32_t)(ipx + VO_PAD);
      const __amdgpu_buffer_rsrc_t rI = klt_rsrc(L.imgI), rD = klt_rsrc(L.derI);
#pragma unroll
      for (int s = 0; s < 8; s++) {
        const uint32_t o = uo + (uint32_t)s * (uint32_t)L.pitch;          // wave-uniform
        T[s] = __builtin_amdgcn_raw_buffer_load_b32(rI, (int)lane_off, (int)o, 0);
        // three consecutive pixels: one 12-byte load.  (8 bytes + the neighbour lane's first pixel through a DPP row shift was
        // measured: the same kernel time -- the data path is not priced per byte.)
        const u32x3 d3 = __builtin_amdgcn_raw_buffer_load_b96(rD, (int)(lane_off * 4u), (int)(o * 4u), 0);
        D0[s] = d3[0]; D1[s] = d3[1]; D2[s] = d3[2];
      }
      // row 8r + 8 = step 0 of row group r + 1 (lanes of r == 3 receive a row that only masked pixels use)
      const uint32_t T8 = row_next(T[0], lane), D08 = row_next(D0[0], lane), D18 = row_next(D1[0], lane), D28 = row_next(D2[0], lane);
      int a11 = 0, a12 = 0, a22 = 0;
#pragma unroll
      for (int s = 0; s < 8; s++) {
        const uint32_t B = (s < 7) ? T[(s + 1) & 7] : T8;
        const uint32_t E0 = (s < 7) ? D0[(s + 1) & 7] : D08;
        const uint32_t E1 = (s < 7) ? D1[(s + 1) & 7] : D18;
        const uint32_t E2 = (s < 7) ? D2[(s + 1) & 7] : D28;
        tI[s] = sample2(T[s], B, wt, wb);
        const uint32_t x0 = deriv1(pack_lo(D0[s], D1[s]), pack_lo(E0, E1), wt, wb);
        const uint32_t y0 = deriv1(pack_hi(D0[s], D1[s]), pack_hi(E0, E1), wt, wb);
        const uint32_t x1 = deriv1(pack_lo(D1[s], D2[s]), pack_lo(E1, E2), wt, wb);
        const uint32_t y1 = deriv1(pack_hi(D1[s], D2[s]), pack_hi(E1, E2), wt, wb);
        const uint32_t sel = (8 * r + s < win) ? colsel : 0x0c0c0c0cu;    // rows / columns outside the window contribute nothing
        const uint32_t xp = __builtin_amdgcn_perm(x1, x0, sel), yp = __builtin_amdgcn_perm(y1, y0, sel);
        tX[s] = xp; tY[s] = yp;
        // the first step starts the three sums from an inline zero (three-address form: no preload)
        a11 = s ? dot2(xp, xp, a11) : dot2k(xp, xp, 0);
        a12 = s ? dot2(xp, yp, a12) : dot2k(xp, yp, 0);
        a22 = s ? dot2(yp, yp, a22) : dot2k(yp, yp, 0);
      }
      float A11, A12, A22;
      {
        // per lane 16 products of two int16 derivatives (|Scharr| <= 4080): < 2^28.01, a quad's sum < 2^30.01
        int l11, h11, l12, h12, l22, h22;
        wave_sum3_wide(a11, a12, a22, lane, l11, h11, l12, h12, l22, h22);
        A11 = klt_combine(h11, l11) * FLT_SCALE; A12 = klt_combine(h12, l12) * FLT_SCALE; A22 = klt_combine(h22, l22) * FLT_SCALE;
      }
      if (level == A.top) VO_STAMP(dbgk, 1);   // first template
      float D = A11 * A22 - A12 * A12;
      // minEig = num / (2 win^2) < minEigThreshold, decided on the numerator (threshold pre-divided exactly on the host)
      const float num = A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12);
      if (num < A.min_eig_num || D < 1.1920929e-07f) {
        if (level == 0) st = 0;
        if (iters && lane == 0) iters[pt * A.iters_stride + level] = n_it;
        continue;
      }
      D = 1.f / D;

      nextx -= half; nexty -= half;
      const __amdgpu_buffer_rsrc_t rJ = klt_rsrc(L.imgJ);
      float pdx = 0.f, pdy = 0.f;
      // REUSE: the cell the parked rows were fetched for.  Nothing is parked when a level starts (no window origin is INT_MIN), so the first
      // sampling of a level always fetches: cell numbers can coincide across levels while the images differ
      int cellx = INT_MIN, celly = INT_MIN;
      int j = 0;
      for (; j < A.max_count; j++) {
        const float fnx = floorf(nextx), fny = floorf(nexty);
        const int inx = (int)fnx, iny = (int)fny;
        if (inx < -win || inx >= L.w || iny < -win || iny >= L.h) {
          if (level == 0) st = 0;
          break;
        }
        uint32_t jt, jb;
        lk_weights(nextx - fnx, nexty - fny, jt, jb);
        int b1 = 0, b2 = 0;
        if constexpr (REUSE) {
          // the cell is wave-uniform: compared on the scalar unit, a branch without exec masking
          const int ux = __builtin_amdgcn_readfirstlane(inx), uy = __builtin_amdgcn_readfirstlane(iny);
          if (ux != cellx || uy != celly) {
            klt_rows_fetch(rows, rows_ab, rJ, lane_off, (uint32_t)(uy + VO_PAD) * (uint32_t)L.pitch + (uint32_t)(ux + VO_PAD), (uint32_t)L.pitch, lane);
            cellx = ux; celly = uy;
          }
          KLT_ROWS_OPAQUE(rows_ab);
          uint2 r0 = klt_row_read(rows, rows_ab, 0), r1 = klt_row_read(rows, rows_ab, 1);
#pragma unroll
          for (int s = 0; s < 8; s++) {
            uint2 r2 = r1;
            if (s < 7) r2 = klt_row_read(rows, rows_ab, s + 2);
            const uint32_t d = pk_sub(sample2_combine(r0, r1, jt, jb), tI[s]);
            b1 = s ? dot2(d, tX[s], b1) : dot2k(d, tX[0], 0);
            b2 = s ? dot2(d, tY[s], b2) : dot2k(d, tY[0], 0);
            if (s < 6) KLT_ROWS_PIN(rows_ab, b1);
            r0 = r1; r1 = r2;
          }
        } else {
          uint32_t Tj[8];
          const uint32_t uj = (uint32_t)(iny + VO_PAD) * (uint32_t)L.pitch + (uint32_t)(inx + VO_PAD);
#pragma unroll
          for (int s = 0; s < 8; s++) Tj[s] = __builtin_amdgcn_raw_buffer_load_b32(rJ, (int)lane_off, (int)(uj + (uint32_t)s * (uint32_t)L.pitch), 0);
          const uint32_t Tj8 = row_next(Tj[0], lane);
#pragma unroll
          for (int s = 0; s < 8; s++) {
            const uint32_t B = (s < 7) ? Tj[(s + 1) & 7] : Tj8;
            const uint32_t d = pk_sub(sample2(Tj[s], B, jt, jb), tI[s]);   // (diff0 | diff1 << 16), |diff| <= 8160
            b1 = s ? dot2(d, tX[s], b1) : dot2k(d, tX[0], 0);
            b2 = s ? dot2(d, tY[s], b2) : dot2k(d, tY[0], 0);
          }
        }
        // per lane 16 products |diff| <= 8160 (255 << 5) times |derivative| <= 4080: < 2^28.99, a quad's sum < 2^30.99
        int l1, h1, l2, h2;
        wave_sum2_wide(b1, b2, lane, l1, h1, l2, h2);
        const float fb1 = klt_combine(h1, l1) * FLT_SCALE;
        const float fb2 = klt_combine(h2, l2) * FLT_SCALE;
        const float dx = (A12 * fb2 - A22 * fb1) * D;
        const float dy = (A12 * fb1 - A11 * fb2) * D;
        nextx += dx; nexty += dy;
        outx = nextx + half; outy = nexty + half;
        // |delta|^2 <= eps^2 is OpenCV's float64 test; its float32 value is within 2^-22 of it, so only a value between the
        // two guard constants needs the float64 evaluation
        const float d2 = dx * dx + dy * dy;
        bool conv;
        if (d2 < A.eps_lo) conv = true;
        else if (d2 > A.eps_hi) conv = false;
        else conv = (double)dx * (double)dx + (double)dy * (double)dy <= A.eps2;
        if (conv) { j++; break; }
        // fabs((double)x) < 0.01 for a float x  <=>  fabsf(x) <= (float)0.01: 0.01 lies strictly between that float and the next
        if (j > 0 && fabsf(dx + pdx) <= 0.01f && fabsf(dy + pdy) <= 0.01f) {
          outx -= dx * 0.5f; outy -= dy * 0.5f;
          j++;
          break;
        }
        pdx = dx; pdy = dy;
        if (level == A.top && j == 0) VO_STAMP(dbgk, 2);   // first LK iteration
      }
      n_it = j;
      if (level == A.top) VO_STAMP(dbgk, 3);   // top level done
      if (level == 1) VO_STAMP(dbgk, 4);       // levels top-1 .. 1 done
      if (iters && lane == 0) iters[pt * A.iters_stride + level] = n_it;

      if (st && level == 0) {
        const float nx = outx - half, ny = outy - half;
        const float fnx = floorf(nx), fny = floorf(ny);
        const int inx = (int)fnx, iny = (int)fny;
        if (inx < -win || inx >= L.w || iny < -win || iny >= L.h) {
          st = 0;
        } else {
          uint32_t jt, jb;
          lk_weights(nx - fnx, ny - fny, jt, jb);
          int e = 0;
          if constexpr (REUSE) {
            // the rows of the last iteration serve when the result lies in its cell; with max_count == 0 nothing is parked and this fetches
            const int ux = __builtin_amdgcn_readfirstlane(inx), uy = __builtin_amdgcn_readfirstlane(iny);
            if (ux != cellx || uy != celly)
              klt_rows_fetch(rows, rows_ab, rJ, lane_off, (uint32_t)(uy + VO_PAD) * (uint32_t)L.pitch + (uint32_t)(ux + VO_PAD), (uint32_t)L.pitch, lane);
            KLT_ROWS_OPAQUE(rows_ab);
            // the row masks are made here, once per keypoint: as eight loop invariants of the level loop they cost the 6-wave instance three
            // registers it does not have
            uint32_t cones = colones;
            KLT_ROWS_OPAQUE(cones);
            uint2 r0 = klt_row_read(rows, rows_ab, 0), r1 = klt_row_read(rows, rows_ab, 1);
#pragma unroll
            for (int s = 0; s < 8; s++) {
              uint2 r2 = r1;
              if (s < 7) r2 = klt_row_read(rows, rows_ab, s + 2);
              const uint32_t d = pk_abs(pk_sub(sample2_combine(r0, r1, jt, jb), tI[s]));
              const uint32_t ones = (8 * r + s < win) ? cones : 0u;
              e = s ? dot2(d, ones, e) : dot2k(d, ones, 0);
              if (s < 6) KLT_ROWS_PIN(rows_ab, e);
              r0 = r1; r1 = r2;
            }
          } else {
            uint32_t Tj[8];
            const uint32_t uj = (uint32_t)(iny + VO_PAD) * (uint32_t)L.pitch + (uint32_t)(inx + VO_PAD);
#pragma unroll
            for (int s = 0; s < 8; s++) Tj[s] = __builtin_amdgcn_raw_buffer_load_b32(rJ, (int)lane_off, (int)(uj + (uint32_t)s * (uint32_t)L.pitch), 0);
            const uint32_t Tj8 = row_next(Tj[0], lane);
#pragma unroll
            for (int s = 0; s < 8; s++) {
              const uint32_t B = (s < 7) ? Tj[(s + 1) & 7] : Tj8;
              const uint32_t d = pk_abs(pk_sub(sample2(Tj[s], B, jt, jb), tI[s]));
              const uint32_t ones = (8 * r + s < win) ? colones : 0u;
              e = s ? dot2(d, ones, e) : dot2k(d, ones, 0);
            }
          }
          const int ierr = wave_sum_i32(e);
          errv = (float)ierr * 1.f / (float)(32 * win * win);
        }
      }
    }
  }
  VO_STAMP(dbgk, 5);
}

// ------------------------------------------------------------------------------------------------
// host side: one launch path for the four forms (vo_internal.h: KLT_FORM_FB, KLT_FORM_SEEDED)
// ------------------------------------------------------------------------------------------------
// One tracker launch on q from the slab rows at off_in to those at off_out (vo_klt.hip): resets fb.n / guess.n, checks and fills the argument
// block (vo_klt_make_args; n == 0 ends there, fb.n = 0 for a form with the check), reserves the check's rows or asks for the guesses in
// c->guess as the form needs them, launches the form's kernel inside ONE VO_PROF_KLT bracket, and sets fb.n.  d_counts: see vo_internal.h
int32_t vo_klt_enqueue(vo_ctx* c, hipStream_t q, int n, const vo_klt_params* prm, size_t off_in, size_t off_out, const int32_t* d_counts, unsigned form);
// the argument checks and block of a tracker launch (vo_klt.hip); nothing is filled for n = 0
int32_t vo_klt_make_args(vo_ctx* c, int n, const vo_klt_params* prm, klt_args& A);
// the backward pass's argument block (vo_klt_fb.hip)
void vo_klt_fb_make_args(const vo_ctx* c, const klt_args& A, klt_fb_args& F);

// what vo_klt_enqueue hands a unit's launcher: the stream and the resolved rows (sequence 0).  A launcher is the hipLaunchKernelGGL of the
// unit's own kernels and nothing else: dim3(n, batch) waves of 64 on q (the kernels stay one translation unit each, see vo_klt_fb.hip)
struct klt_launch_rows {
  hipStream_t q;
  int n;
  const float* p0; float* p1; uint8_t* status; float* err;
  const int32_t* counts;
};
void vo_klt_launch_fb(vo_ctx* c, const klt_launch_rows& L, const klt_args& A, const klt_fb_args& F);            // vo_klt_fb.hip: k_klt_track_fb
void vo_klt_launch_seeded(vo_ctx* c, const klt_launch_rows& L, const klt_args& A, const klt_fb_args* F);        // vo_klt_seed.hip: F null = k_klt_seeded, else k_klt_seeded_fb
void vo_klt_launch_reuse(vo_ctx* c, const klt_launch_rows& L, const klt_args& A);                               // vo_klt_reuse.hip: k_klt_track_r

// the iteration table of the last launch: n points x `levels` entries per sequence
inline hipError_t iters_d2h(vo_ctx* c, int32_t* h, int n, int levels) {
  return rows_d2h(c, h, c->d_iters, sizeof(int32_t) * (size_t)c->max_pts * VO_MAX_LEVELS, sizeof(int32_t) * (size_t)n * levels);
}
