// Multi-scale ORB: FAST-9/16 corners on a scale pyramid, Harris re-ranking with per-level quotas, orientation and steered BRIEF -- the
// reference Extractor's 'orb' feature method (cv2.ORB_create(), src/extractor/extractor.py:30-31, 114-122).  OpenCV and its learned table are not
// part of this project, so parity with cv2.ORB is not pinned: tests/orb_model.py is the definition (stated in include/vo_mi355x.h, section
// "multi-scale ORB features"), integer arithmetic or single IEEE operations in a fixed order, and these kernels equal it bit for bit.
//
// Launches of one vo_orb_detect_compute, all sequences at once:
//   k_orb_level0    the uploaded frames into level 0 of the padded pyramid (one contiguous upload instead of a pitched copy per sequence)
//   k_orb_resize    one per level above 0 (level l reads level l-1): fixed-point bilinear, the (taps, weight) tables come from the host
//   k_orb_score     FAST score of every pixel of every level, u8 (vo_fast_dev.h: the code of k_fast_score)         } one grid over the tiles of
//   k_orb_nms       strict 3 x 3 maxima inside the 31-pixel edge, mask -> candidate lists + a 256-bin score histogram } all levels (tile0[])
//   k_orb_cut       per (sequence, level): the FAST score below which retainBest(2 * quota) drops a candidate, read off the histogram
//   k_orb_harris    a thread per candidate: the survivors' Harris response -> rows (response, position)
//   k_orb_rank      all pairs of a (sequence, level): keep = fewer than quota rows have a strictly greater response; output position = the
//                   number of rows that precede under (response descending, ly, lx) -- for a kept row every such row is kept too.  No sort.
//   k_orb_describe  one wave per kept row (vo_brief_dev.h: the code of k_brief_describe) -> vo_orb_kp + 32 bytes at its output position
// The lists are filled through atomic counters, so their order varies from run to run; everything read from them is a count or a set, so the
// output does not.  Every write is bounded by the capacity of its buffer; a count beyond one is VO_E_CAPACITY on the host, nothing is truncated.
#include "vo_internal.h"
#include "vo_brief_pattern.h"
#include "vo_brief_dev.h"
#include "vo_fast_dev.h"

#include <math.h>
#include <string.h>
#include <algorithm>
#include <vector>

#define ORB_EDGE 31                       // edge_threshold: a keypoint keeps this distance from the borders of its level
#define ORB_LEVELS 8
#define ORB_CAND_CAP 65536                // strict maxima per (sequence, level)
#define ORB_KEEP_CAP 8192                 // rows behind the FAST cut per (sequence, level)
#define ORB_TILE_W (64 * FAST_PX)         // 256 columns x 16 rows per workgroup of the two tiled kernels
#define ORB_TILE_H 16
#define ORB_QUOTA_MAX (1 << 29)           // (a quota above every capacity; keeps 2 * quota in int32)
// per (sequence, level) counters, int32 [batch][ORB_LEVELS][ORB_META]
enum { ORB_N_CAND = 0, ORB_THR = 1, ORB_N_CUT = 2, ORB_N_ROWS = 3, ORB_N_KEPT = 4, ORB_META = 8 };

struct orb_geom {
  int nlevels, W, H;                      // W x H: level 0
  int w[ORB_LEVELS], h[ORB_LEVELS], pitch[ORB_LEVELS];
  int tile0[ORB_LEVELS + 1], tiles_x[ORB_LEVELS];     // tiles tile0[l] .. tile0[l + 1] - 1 of the tiled grids belong to level l
  int quota[ORB_LEVELS];
  int cand_off[ORB_LEVELS], cand_cap[ORB_LEVELS];     // candidate slots of level l within a sequence
  float scale[ORB_LEVELS];
  float sc4;
  size_t img_off[ORB_LEVELS];             // bytes from a sequence's pyramid to the padded level (its interior starts at (VO_PAD, VO_PAD))
  size_t score_off[ORB_LEVELS];           // bytes from a sequence's score maps to the level's [h][w] u8
  size_t pyr_seq, score_seq, cand_seq;    // per-sequence strides: bytes, bytes, slots
};

__device__ __forceinline__ const uint8_t* orb_level(const orb_geom& G, const uint8_t* pyr, int bseq, int l) {      // pixel (0, 0) of a level
  return pyr + (size_t)bseq * G.pyr_seq + G.img_off[l] + (size_t)VO_PAD * G.pitch[l] + VO_PAD;
}

__device__ __forceinline__ int orb_tile_level(const orb_geom& G, int tile) {
  int l = 0;
  while (l + 1 < G.nlevels && tile >= G.tile0[l + 1]) l++;
  return l;
}

// level 0: the tight upload [batch][h][w] into the padded pyramid.  grid (w / 256, h, batch)
__global__ void __launch_bounds__(256) k_orb_level0(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int dst_pitch, size_t pyr_seq, int w) {
  const int x = (int)blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= w) return;
  dst[(size_t)blockIdx.z * pyr_seq + (size_t)y * dst_pitch + x] = src[((size_t)blockIdx.z * gridDim.y + y) * w + x];
}

// xtab [dw], ytab [dh]: x = tap 0 | tap 1 << 16 (both clamped by the host), y = the weight of tap 1 in 1/2048.  grid (dw / 256, dh, batch)
__global__ void __launch_bounds__(256) k_orb_resize(const uint8_t* __restrict__ src, int src_pitch, uint8_t* __restrict__ dst, int dst_pitch, size_t pyr_seq,
                                                    int dw, const uint2* __restrict__ xtab, const uint2* __restrict__ ytab) {
  const int x = (int)blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= dw) return;
  const uint2 tx = xtab[x], ty = ytab[y];
  const uint8_t* const s = src + (size_t)blockIdx.z * pyr_seq;
  const uint8_t* const r0 = s + (size_t)(ty.x & 0xFFFFu) * src_pitch;
  const uint8_t* const r1 = s + (size_t)(ty.x >> 16) * src_pitch;
  const uint32_t x0 = tx.x & 0xFFFFu, x1 = tx.x >> 16, ax = tx.y, ay = ty.y;
  const uint32_t top = (2048u - ax) * r0[x0] + ax * r0[x1];
  const uint32_t bot = (2048u - ax) * r1[x0] + ax * r1[x1];
  const uint32_t v = (2048u - ay) * top + ay * bot;                  // <= 2048 * 2048 * 255
  dst[(size_t)blockIdx.z * pyr_seq + (size_t)y * dst_pitch + x] = (uint8_t)((v + (1u << 21)) >> 22);
}

// grid (tiles of all levels, batch).  score: [h_l][w_l] u8 per level (a FAST score is at most 254), every pixel written
__global__ void __launch_bounds__(256) k_orb_score(orb_geom G, const uint8_t* __restrict__ pyr, int t, uint8_t* __restrict__ score) {
  const int bseq = blockIdx.y;
  const int l = orb_tile_level(G, blockIdx.x);
  const int local = (int)blockIdx.x - G.tile0[l], ty = local / G.tiles_x[l], tx = local - ty * G.tiles_x[l];
  const int W = G.w[l], H = G.h[l], pitch = G.pitch[l];
  const uint8_t* const img = orb_level(G, pyr, bseq, l);
  uint8_t* const S = score + (size_t)bseq * G.score_seq + G.score_off[l];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int x0 = (tx * 64 + lane) * FAST_PX;
  const int xc = x0 < W ? x0 : 0;            // lanes past the row's end load from a valid column and keep nothing
#pragma unroll 1
  for (int k = 0; k < ORB_TILE_H / 4; k++) {
    const int y = ty * ORB_TILE_H + wave * (ORB_TILE_H / 4) + k;      // (wave-uniform)
    if (y >= H) break;
    int sc[FAST_PX];
#pragma unroll
    for (int p = 0; p < FAST_PX; p++) sc[p] = 0;
    if (y >= 3 && y < H - 3) fast_score_px4(img + (size_t)y * pitch + xc, pitch, x0, W, t, sc);
    if (x0 < W) {
      uint8_t* const o = S + (size_t)y * W + x0;
      if (x0 + FAST_PX <= W) {
        const uint32_t v = (uint32_t)sc[0] | ((uint32_t)sc[1] << 8) | ((uint32_t)sc[2] << 16) | ((uint32_t)sc[3] << 24);
        __builtin_memcpy(o, &v, 4);
      } else {
#pragma unroll
        for (int p = 0; p < FAST_PX; p++) if (x0 + p < W) o[p] = (uint8_t)sc[p];
      }
    }
  }
}

// grid (tiles of all levels, batch); a thread owns one column of its tile.  mask: [batch][H][W] of level 0 or null.  cand: x = lx | ly << 16, y = score
__global__ void __launch_bounds__(256) k_orb_nms(orb_geom G, const uint8_t* __restrict__ score, const uint8_t* __restrict__ mask, uint2* __restrict__ cand,
                                                 int32_t* __restrict__ meta, uint32_t* __restrict__ hist) {
  __shared__ uint32_t s_hist[256];
  const int bseq = blockIdx.y;
  const int l = orb_tile_level(G, blockIdx.x);
  const int local = (int)blockIdx.x - G.tile0[l], ty = local / G.tiles_x[l], tx = local - ty * G.tiles_x[l];
  const int W = G.w[l], H = G.h[l];
  const uint8_t* const S = score + (size_t)bseq * G.score_seq + G.score_off[l];
  const float s = G.scale[l];
  int32_t* const m = meta + ((size_t)bseq * ORB_LEVELS + l) * ORB_META;
  uint2* const out = cand + (size_t)bseq * G.cand_seq + G.cand_off[l];
  const int cap = G.cand_cap[l];
  s_hist[threadIdx.x] = 0;
  __syncthreads();
  const int x = tx * ORB_TILE_W + (int)threadIdx.x;
  if (x >= ORB_EDGE && x < W - ORB_EDGE) {
    const int y_lo = max(ty * ORB_TILE_H, ORB_EDGE), y_hi = min(ty * ORB_TILE_H + ORB_TILE_H, H - ORB_EDGE);
    for (int y = y_lo; y < y_hi; y++) {
      const uint8_t* const p = S + (size_t)y * W + x;
      const int c = p[0];
      if (c == 0) continue;
      if (!(c > p[-1] && c > p[1] && c > p[-W - 1] && c > p[-W] && c > p[-W + 1] && c > p[W - 1] && c > p[W] && c > p[W + 1])) continue;
      if (mask) {
        const int mx = min(G.W - 1, (int)rintf(__fmul_rn((float)x, s))), my = min(G.H - 1, (int)rintf(__fmul_rn((float)y, s)));
        if (mask[((size_t)bseq * G.H + my) * G.W + mx] == 0) continue;
      }
      atomicAdd(&s_hist[c], 1u);
      const int slot = atomicAdd(&m[ORB_N_CAND], 1);
      if (slot < cap) out[slot] = make_uint2((uint32_t)x | ((uint32_t)y << 16), (uint32_t)c);
    }
  }
  __syncthreads();
  const uint32_t n = s_hist[threadIdx.x];
  if (n) atomicAdd(&hist[((size_t)bseq * ORB_LEVELS + l) * 256 + threadIdx.x], n);
}

// grid (levels, batch), 256 threads = the 256 scores.  retainBest(2 * quota) keeps score v iff fewer than 2 * quota candidates score more than v:
// the scores >= THR.  N_CUT = how many those are (the rows k_orb_harris will write)
__global__ void __launch_bounds__(256) k_orb_cut(orb_geom G, const uint32_t* __restrict__ hist, int32_t* __restrict__ meta) {
  __shared__ uint32_t s_suf[256];
  __shared__ int s_thr;
  const int l = blockIdx.x, bseq = blockIdx.y, v = threadIdx.x;
  const uint32_t own = hist[((size_t)bseq * ORB_LEVELS + l) * 256 + v];
  s_suf[v] = own;
  if (v == 0) s_thr = 256;
  __syncthreads();
  for (int off = 1; off < 256; off <<= 1) {           // inclusive suffix sums
    const uint32_t add = v + off < 256 ? s_suf[v + off] : 0u;
    __syncthreads();
    s_suf[v] += add;
    __syncthreads();
  }
  const uint32_t greater = s_suf[v] - own;
  if (v >= 1 && greater < 2u * (uint32_t)G.quota[l]) atomicMin(&s_thr, v);
  __syncthreads();
  if (v == 0) {
    int32_t* const m = meta + ((size_t)bseq * ORB_LEVELS + l) * ORB_META;
    m[ORB_THR] = s_thr;
    m[ORB_N_CUT] = s_thr < 256 ? (int32_t)s_suf[s_thr] : 0;
  }
}

// The Harris response of the 7 x 7 block centred on p (rows `pitch` apart; columns -4 .. +7 of rows -4 .. +4 are read): int32 sums, then float32
// with every operation rounded on its own
__device__ __forceinline__ float orb_harris(const uint8_t* p, int pitch, float sc4) {
  uint32_t r0[3], r1[3], r2[3];
  const uint8_t* q = p - 4 * (size_t)pitch - 4;
  r0[0] = fast_ld_u32_any(q); r0[1] = fast_ld_u32_any(q + 4); r0[2] = fast_ld_u32_any(q + 8);
  q += pitch;
  r1[0] = fast_ld_u32_any(q); r1[1] = fast_ld_u32_any(q + 4); r1[2] = fast_ld_u32_any(q + 8);
  int a = 0, b = 0, c = 0;
#pragma unroll
  for (int k = 0; k < 7; k++) {              // block row k: r0, r1, r2 = the image rows above it, of it, below it; byte j + 1 = block column j
    q += pitch;
    r2[0] = fast_ld_u32_any(q); r2[1] = fast_ld_u32_any(q + 4); r2[2] = fast_ld_u32_any(q + 8);
#pragma unroll
    for (int j = 0; j < 7; j++) {
      const int ix = 2 * (fast_byte(r1, j + 2) - fast_byte(r1, j)) + (fast_byte(r0, j + 2) - fast_byte(r0, j)) + (fast_byte(r2, j + 2) - fast_byte(r2, j));
      const int iy = 2 * (fast_byte(r2, j + 1) - fast_byte(r0, j + 1)) + (fast_byte(r2, j) - fast_byte(r0, j)) + (fast_byte(r2, j + 2) - fast_byte(r0, j + 2));
      a += ix * ix; b += iy * iy; c += ix * iy;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) { r0[i] = r1[i]; r1[i] = r2[i]; }
  }
  const float fa = (float)a, fb = (float)b, fc = (float)c;
  const float det = __fsub_rn(__fmul_rn(fa, fb), __fmul_rn(fc, fc));
  const float tr = __fadd_rn(fa, fb);
  return __fmul_rn(__fsub_rn(det, __fmul_rn(__fmul_rn(0.04f, tr), tr)), sc4);
}

// grid (candidates / 256, levels, batch).  rows [batch][ORB_LEVELS][ORB_KEEP_CAP]: response f32, position lx | ly << 16
__global__ void __launch_bounds__(256) k_orb_harris(orb_geom G, const uint8_t* __restrict__ pyr, const uint2* __restrict__ cand, int32_t* __restrict__ meta,
                                                    float* __restrict__ row_resp, uint32_t* __restrict__ row_xy) {
  const int l = blockIdx.y, bseq = blockIdx.z;
  int32_t* const m = meta + ((size_t)bseq * ORB_LEVELS + l) * ORB_META;
  const int n = min(m[ORB_N_CAND], G.cand_cap[l]);
  const int i = (int)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint2 cd = cand[(size_t)bseq * G.cand_seq + G.cand_off[l] + i];
  if ((int)cd.y < m[ORB_THR]) return;
  const int x = (int)(cd.x & 0xFFFFu), y = (int)(cd.x >> 16);
  const float r = orb_harris(orb_level(G, pyr, bseq, l) + (size_t)y * G.pitch[l] + x, G.pitch[l], G.sc4);
  const int slot = atomicAdd(&m[ORB_N_ROWS], 1);
  if (slot < ORB_KEEP_CAP) {
    const size_t o = ((size_t)bseq * ORB_LEVELS + l) * ORB_KEEP_CAP + slot;
    row_resp[o] = r; row_xy[o] = cd.x;
  }
}

// grid (rows / 256, levels, batch).  row_pos: the row's place among its level's output, -1 = not kept; N_KEPT: the kept rows of the level
__global__ void __launch_bounds__(256) k_orb_rank(orb_geom G, int32_t* __restrict__ meta, const float* __restrict__ row_resp, const uint32_t* __restrict__ row_xy,
                                                  int32_t* __restrict__ row_pos) {
  __shared__ float s_r[256];
  __shared__ uint32_t s_xy[256];
  const int l = blockIdx.y, bseq = blockIdx.z;
  int32_t* const m = meta + ((size_t)bseq * ORB_LEVELS + l) * ORB_META;
  const int n = min(m[ORB_N_ROWS], ORB_KEEP_CAP);
  if ((int)blockIdx.x * 256 >= n) return;             // (the whole workgroup)
  const size_t base = ((size_t)bseq * ORB_LEVELS + l) * ORB_KEEP_CAP;
  const int i = (int)blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n;
  const float r = live ? row_resp[base + i] : 0.f;
  const uint32_t xy = live ? row_xy[base + i] : 0u;
  int greater = 0, before = 0;
  for (int j0 = 0; j0 < n; j0 += 256) {
    __syncthreads();
    if (j0 + (int)threadIdx.x < n) { s_r[threadIdx.x] = row_resp[base + j0 + threadIdx.x]; s_xy[threadIdx.x] = row_xy[base + j0 + threadIdx.x]; }
    __syncthreads();
    const int cnt = min(256, n - j0);
    for (int j = 0; j < cnt; j++) {
      const float rj = s_r[j];
      const uint32_t xyj = s_xy[j];
      greater += rj > r ? 1 : 0;
      before += (rj > r || (rj == r && xyj < xy)) ? 1 : 0;
    }
  }
  const bool keep = live && greater < G.quota[l];
  if (live) row_pos[base + i] = keep ? before : -1;
  const unsigned long long b = __ballot(keep);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&m[ORB_N_KEPT], (int32_t)__popcll(b));
}

struct orb_desc_args {
  orb_geom G;
  int max_out;
  int8_t pat[1024];            // [256][4]
};

// grid (rows, levels, batch), one wave per row.  kps [batch][max_out], desc [batch][max_out][32]: a row beyond max_out is not written (the
// host answers VO_E_CAPACITY from the counts)
__global__ void __launch_bounds__(64) k_orb_describe(orb_desc_args A, const uint8_t* __restrict__ pyr, const int32_t* __restrict__ meta,
                                                     const float* __restrict__ row_resp, const uint32_t* __restrict__ row_xy, const int32_t* __restrict__ row_pos,
                                                     vo_orb_kp* __restrict__ kps, uint8_t* __restrict__ desc) {
  __shared__ uint8_t raw[BRIEF_TW * BRIEF_TW + 3];
  __shared__ uint16_t hs[BRIEF_TW * BRIEF_SW + 1];
  __shared__ uint8_t S[BRIEF_SW * BRIEF_SW + 3];
  const int i = blockIdx.x, l = blockIdx.y, bseq = blockIdx.z, lane = threadIdx.x;
  const int32_t* const m0 = meta + (size_t)bseq * ORB_LEVELS * ORB_META;
  if (i >= min(m0[l * ORB_META + ORB_N_ROWS], ORB_KEEP_CAP)) return;
  const size_t o = ((size_t)bseq * ORB_LEVELS + l) * ORB_KEEP_CAP + i;
  const int pos = __builtin_amdgcn_readfirstlane(row_pos[o]);
  if (pos < 0) return;
  int dst = pos;
  for (int k = 0; k < l; k++) dst += m0[k * ORB_META + ORB_N_KEPT];
  dst = __builtin_amdgcn_readfirstlane(dst);
  if (dst >= A.max_out) return;
  const uint32_t xy = __builtin_amdgcn_readfirstlane(row_xy[o]);
  const int x = (int)(xy & 0xFFFFu), y = (int)(xy >> 16);
  float ang;
  const unsigned long long word = brief_describe_px(orb_level(A.G, pyr, bseq, l), A.G.pitch[l], A.G.w[l], A.G.h[l], x, y, A.pat, lane, raw, hs, S, ang);
  const size_t row = (size_t)bseq * A.max_out + dst;
  if (lane < 4) reinterpret_cast<unsigned long long*>(desc)[row * 4 + lane] = word;
  if (lane == 0) {
    const float s = A.G.scale[l];
    vo_orb_kp k;
    k.x = __fmul_rn((float)x, s); k.y = __fmul_rn((float)y, s); k.size = __fmul_rn(31.0f, s); k.angle = ang; k.response = row_resp[o];
    k.octave = l; k.lx = x; k.ly = y;
    kps[row] = k;
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
struct vo_orb_ws {
  // every buffer only grows, each on its own: after a refused allocation it is empty and the next call reserves it again
  vo_dev<uint8_t> d_pyr;                                  // [batch][pyr_seq]: the padded levels
  vo_dev<uint8_t> d_score;                                // [batch][score_seq]
  vo_dev<uint2> d_cand;                                   // [batch][cand_seq]
  vo_dev<uint2> d_tab;                                    // the resize tables of the levels above 0: x then y
  vo_dev<uint8_t> d_in;                                   // [batch][H][W]: the frames as uploaded
  vo_dev<uint8_t> d_mask;                                 // [batch][H][W]
  vo_dev<int32_t> d_meta;                                 // [batch][ORB_LEVELS][ORB_META] i32, then the histograms [batch][ORB_LEVELS][256] u32
  vo_dev<float> d_resp; vo_dev<uint32_t> d_xy; vo_dev<int32_t> d_pos;            // rows [batch][ORB_LEVELS][ORB_KEEP_CAP]
  vo_dev<vo_orb_kp> d_kps; vo_dev<uint8_t> d_desc;        // [batch][max_out] of the largest max_out asked for
  orb_geom G = {};
  bool have = false;                                      // G and n_l describe a call that succeeded
  std::vector<int32_t> n_l;                               // [batch][ORB_LEVELS]
  std::vector<uint2> h_tab;
  std::vector<uint8_t> h_out;                             // host side of the output read-back
};

void vo_orb_destroy(vo_ctx* c) {
  delete c->orb;
  c->orb = nullptr;
}

extern "C" int32_t vo_orb_default_params(vo_orb_params* p) {
  if (!p) return VO_E_INVALID;
  memset(p, 0, sizeof(*p));
  p->nfeatures = 500; p->nlevels = 8; p->scale_factor = 1.2; p->fast_threshold = 20; p->edge_threshold = ORB_EDGE; p->harris_k = 0.04f;
  return VO_OK;
}

// the (taps, weight) table of one axis: destination d samples the source at (d + 0.5) * (src / dst) - 0.5
static void orb_axis_table(int src, int dst, uint2* out) {
  const double ratio = (double)src / (double)dst;
  for (int d = 0; d < dst; d++) {
    const double fx = ((double)d + 0.5) * ratio - 0.5;
    const double f0 = floor(fx);
    const long i0 = (long)f0;
    const uint32_t a = (uint32_t)rint((fx - f0) * 2048.0);
    const uint32_t t0 = (uint32_t)std::min<long>(std::max<long>(i0, 0), src - 1), t1 = (uint32_t)std::min<long>(std::max<long>(i0 + 1, 0), src - 1);
    out[d] = make_uint2(t0 | (t1 << 16), a);
  }
}

// level sizes, quotas, the tile table and the layout of the per-sequence buffers for one parameter set
static void orb_geometry(const vo_ctx* c, const vo_orb_params* p, orb_geom& G) {
  memset(&G, 0, sizeof(G));
  G.nlevels = p->nlevels; G.W = c->width; G.H = c->height;
  G.sc4 = (float)pow(1.0 / (4 * 7 * 255), 4.0);
  size_t img = 0, sco = 0, cand = 0;
  int tiles = 0;
  for (int l = 0; l < G.nlevels; l++) {
    const double s = pow(p->scale_factor, (double)l);
    int w = (int)rint((double)c->width / s), h = (int)rint((double)c->height / s);
    if (w < 1 || h < 1 || (l > 0 && G.w[l - 1] == 0)) w = h = 0;
    G.w[l] = w; G.h[l] = h; G.scale[l] = (float)s;
    G.pitch[l] = (w + 2 * VO_PAD + 63) & ~63;
    G.img_off[l] = img; G.score_off[l] = sco; G.cand_off[l] = (int)cand;
    G.tile0[l] = tiles;
    if (w > 0) { img += (size_t)G.pitch[l] * (h + 2 * VO_PAD); sco += ((size_t)w * h + 15) & ~(size_t)15; }
    if (std::min(w, h) >= 2 * ORB_EDGE + 1) {              // a smaller level has no pixel inside the edge: no tiles, no candidates
      G.tiles_x[l] = vo_div_up(w, ORB_TILE_W);
      tiles += G.tiles_x[l] * vo_div_up(h, ORB_TILE_H);
      // strict 3 x 3 maxima are never neighbours: at most one per 2 x 2 cell of the eligible region
      const size_t most = (size_t)((w - 2 * ORB_EDGE + 1) / 2) * (size_t)((h - 2 * ORB_EDGE + 1) / 2);
      G.cand_cap[l] = (int)std::min<size_t>(most, ORB_CAND_CAP);
      cand += (size_t)G.cand_cap[l];
    } else G.tiles_x[l] = 1;
  }
  for (int l = G.nlevels; l <= ORB_LEVELS; l++) G.tile0[l] = tiles;
  G.pyr_seq = img; G.score_seq = sco; G.cand_seq = cand;
  // OpenCV's quotas
  if (G.nlevels == 1) G.quota[0] = std::min(p->nfeatures, ORB_QUOTA_MAX);
  else {
    const double f = 1.0 / p->scale_factor;
    double nd = (double)p->nfeatures * (1.0 - f) / (1.0 - pow(f, (double)G.nlevels));
    long sum = 0;
    for (int l = 0; l < G.nlevels - 1; l++) {
      const long q = (long)rint(nd);
      G.quota[l] = (int)std::min<long>(q, ORB_QUOTA_MAX);
      sum += q; nd *= f;
    }
    G.quota[G.nlevels - 1] = (int)std::min<long>(std::max<long>((long)p->nfeatures - sum, 0), ORB_QUOTA_MAX);
  }
}

static int32_t orb_reserve(vo_ctx* c, const orb_geom& G, bool with_mask, int max_out) {
  if (!c->orb) c->orb = new vo_orb_ws();
  vo_orb_ws* w = c->orb;
  const size_t B = c->batch;
  VO_HIP(c, w->d_pyr.reserve(B * G.pyr_seq));
  if (w->d_pyr.grew()) VO_HIP(c, hipMemsetAsync(w->d_pyr, 0, w->d_pyr.bytes(), c->stream));   // the borders: read by tile loads, never part of a result
  VO_HIP(c, w->d_score.reserve(B * G.score_seq));
  VO_HIP(c, w->d_cand.reserve(B * G.cand_seq));
  size_t tab = 0;
  for (int l = 1; l < G.nlevels; l++) tab += (size_t)G.w[l] + G.h[l];
  VO_HIP(c, w->d_tab.reserve(tab));
  VO_HIP(c, w->d_in.reserve(B * (size_t)c->width * c->height));
  if (with_mask) VO_HIP(c, w->d_mask.reserve(B * (size_t)c->width * c->height));
  const size_t rows = B * ORB_LEVELS * ORB_KEEP_CAP;
  VO_HIP(c, w->d_meta.reserve(B * ORB_LEVELS * (ORB_META + 256)));
  VO_HIP(c, w->d_resp.reserve(rows));
  VO_HIP(c, w->d_xy.reserve(rows));
  VO_HIP(c, w->d_pos.reserve(rows));
  VO_HIP(c, w->d_kps.reserve(B * (size_t)max_out));
  VO_HIP(c, w->d_desc.reserve((size_t)32 * B * max_out));
  return VO_OK;
}

// `rows` rows of w bytes, `stride` apart on the host, to a tight device image: one linear copy where the host rows are tight too (a pitched copy
// from pageable memory goes row by row: 2.6 ms for one 1241 x 376 frame against 0.1 ms)
static hipError_t orb_upload(uint8_t* dst, const uint8_t* src, int stride, int w, size_t rows, hipStream_t q) {
  if (stride == w) return hipMemcpyAsync(dst, src, (size_t)w * rows, hipMemcpyHostToDevice, q);
  return hipMemcpy2DAsync(dst, w, src, stride, w, rows, hipMemcpyHostToDevice, q);
}

extern "C" int32_t vo_orb_detect_compute(vo_ctx* c, const uint8_t* img, int32_t stride, const uint8_t* mask, const vo_orb_params* prm,
                                         const int8_t* pattern, int32_t max_out, vo_orb_kp* kps, uint8_t* desc, int32_t* n_out) {
  if (!c) return VO_E_INVALID;
  vo_orb_params def;
  if (!prm) { vo_orb_default_params(&def); prm = &def; }
  VO_CHECK(c, img && kps && desc && n_out, VO_E_INVALID, "null buffer");
  VO_CHECK(c, stride >= c->width && max_out >= 1, VO_E_INVALID, "bad stride / max_out");
  VO_CHECK(c, prm->nfeatures >= 1, VO_E_INVALID, "nfeatures must be >= 1");
  VO_CHECK(c, prm->scale_factor > 1.0 && prm->scale_factor <= 2.0, VO_E_INVALID, "scale_factor must lie in (1, 2]");
  VO_CHECK(c, prm->nlevels >= 1 && prm->nlevels <= ORB_LEVELS, VO_E_INVALID, "nlevels must lie in 1..8");
  VO_CHECK(c, prm->fast_threshold >= 1 && prm->fast_threshold <= 254, VO_E_INVALID, "fast_threshold must lie in 1..254");
  VO_CHECK(c, prm->edge_threshold == ORB_EDGE, VO_E_INVALID, "edge_threshold must be 31");
  VO_CHECK(c, prm->harris_k == 0.04f, VO_E_INVALID, "harris_k must be 0.04f");
  VO_CHECK(c, c->width <= 32767 && c->height <= 32767, VO_E_INVALID, "an image side above 32767");
  { const int32_t r = vo_brief_check_pattern(c, pattern); if (r != VO_OK) return r; }
  VO_HIP(c, hipSetDevice(c->device));
  { const int32_t rq = vo_quiesce_side(c); if (rq != VO_OK) return rq; }
  orb_desc_args A;
  orb_geom& G = A.G;
  orb_geometry(c, prm, G);
  A.max_out = max_out;
  memcpy(A.pat, pattern ? pattern : VO_BRIEF_DEFAULT_PATTERN, 1024);
  { const int32_t r = orb_reserve(c, G, mask != nullptr, max_out); if (r != VO_OK) return r; }
  vo_orb_ws* w = c->orb;
  w->have = false;
  const size_t B = c->batch;
  const int W = c->width, H = c->height;
  hipStream_t q = c->stream;
  uint32_t* const d_hist = reinterpret_cast<uint32_t*>(w->d_meta + B * ORB_LEVELS * ORB_META);
  VO_HIP(c, hipMemsetAsync(w->d_meta, 0, sizeof(int32_t) * B * ORB_LEVELS * (ORB_META + 256), q));
  // ---- level 0 and the mask from the host, the tables, the levels above ----
  uint8_t* const lvl0 = w->d_pyr + G.img_off[0] + (size_t)VO_PAD * G.pitch[0] + VO_PAD;
  VO_HIP(c, orb_upload(w->d_in, img, stride, W, (size_t)H * B, q));
  hipLaunchKernelGGL(k_orb_level0, dim3(vo_div_up(W, 256), H, (unsigned)B), dim3(256), 0, q, w->d_in, lvl0, G.pitch[0], G.pyr_seq, W);
  if (mask) VO_HIP(c, orb_upload(w->d_mask, mask, stride, W, (size_t)H * B, q));
  w->h_tab.clear();
  for (int l = 1; l < G.nlevels && G.w[l] > 0; l++) {
    const size_t at = w->h_tab.size();
    w->h_tab.resize(at + G.w[l] + G.h[l]);
    orb_axis_table(G.w[l - 1], G.w[l], w->h_tab.data() + at);
    orb_axis_table(G.h[l - 1], G.h[l], w->h_tab.data() + at + G.w[l]);
  }
  if (!w->h_tab.empty()) VO_HIP(c, hipMemcpyAsync(w->d_tab, w->h_tab.data(), sizeof(uint2) * w->h_tab.size(), hipMemcpyHostToDevice, q));
  {
    vo_prof_scope prof(c, q, VO_PROF_ORB_PYRAMID);
    size_t at = 0;
    for (int l = 1; l < G.nlevels && G.w[l] > 0; l++) {
      hipLaunchKernelGGL(k_orb_resize, dim3(vo_div_up(G.w[l], 256), G.h[l], (unsigned)B), dim3(256), 0, q,
                         w->d_pyr + G.img_off[l - 1] + (size_t)VO_PAD * G.pitch[l - 1] + VO_PAD, G.pitch[l - 1],
                         w->d_pyr + G.img_off[l] + (size_t)VO_PAD * G.pitch[l] + VO_PAD, G.pitch[l], G.pyr_seq, G.w[l], w->d_tab + at, w->d_tab + at + G.w[l]);
      at += (size_t)G.w[l] + G.h[l];
    }
  }
  // ---- candidates and the FAST cut ----
  const int tiles = G.tile0[ORB_LEVELS];
  if (tiles > 0) {
    vo_prof_scope prof(c, q, VO_PROF_ORB_CANDIDATES);
    hipLaunchKernelGGL(k_orb_score, dim3(tiles, (unsigned)B), dim3(256), 0, q, G, w->d_pyr, prm->fast_threshold, w->d_score);
    hipLaunchKernelGGL(k_orb_nms, dim3(tiles, (unsigned)B), dim3(256), 0, q, G, w->d_score, mask ? w->d_mask : nullptr, w->d_cand, w->d_meta, d_hist);
    hipLaunchKernelGGL(k_orb_cut, dim3(G.nlevels, (unsigned)B), dim3(256), 0, q, G, d_hist, w->d_meta);
  }
  VO_HIP(c, hipGetLastError());
  std::vector<int32_t> meta(B * ORB_LEVELS * ORB_META);
  VO_HIP(c, hipMemcpyAsync(meta.data(), w->d_meta, sizeof(int32_t) * meta.size(), hipMemcpyDeviceToHost, q));
  VO_HIP(c, hipStreamSynchronize(q));
  int max_cand = 0, max_rows = 0;
  for (size_t b = 0; b < B; b++)
    for (int l = 0; l < G.nlevels; l++) {
      const int32_t* m = meta.data() + (b * ORB_LEVELS + l) * ORB_META;
      VO_CHECK(c, m[ORB_N_CAND] <= G.cand_cap[l], VO_E_CAPACITY, "more than 65536 FAST maxima on one level of one sequence");
      VO_CHECK(c, m[ORB_N_CUT] <= ORB_KEEP_CAP, VO_E_CAPACITY, "more than 8192 keypoints of one level of one sequence pass the FAST cut (nfeatures too large for this image)");
      max_cand = std::max(max_cand, m[ORB_N_CAND]); max_rows = std::max(max_rows, m[ORB_N_CUT]);
    }
  // ---- Harris, retention, description ----
  if (max_rows > 0) {
    {
      vo_prof_scope prof(c, q, VO_PROF_ORB_RETAIN);
      hipLaunchKernelGGL(k_orb_harris, dim3(vo_div_up(max_cand, 256), G.nlevels, (unsigned)B), dim3(256), 0, q, G, w->d_pyr, w->d_cand, w->d_meta, w->d_resp,
                         w->d_xy);
      hipLaunchKernelGGL(k_orb_rank, dim3(vo_div_up(max_rows, 256), G.nlevels, (unsigned)B), dim3(256), 0, q, G, w->d_meta, w->d_resp, w->d_xy, w->d_pos);
    }
    {
      vo_prof_scope prof(c, q, VO_PROF_ORB_DESCRIBE);
      hipLaunchKernelGGL(k_orb_describe, dim3(max_rows, G.nlevels, (unsigned)B), dim3(64), 0, q, A, w->d_pyr, w->d_meta, w->d_resp, w->d_xy, w->d_pos, w->d_kps,
                         w->d_desc);
    }
    VO_HIP(c, hipGetLastError());
    VO_HIP(c, hipMemcpyAsync(meta.data(), w->d_meta, sizeof(int32_t) * meta.size(), hipMemcpyDeviceToHost, q));
    VO_HIP(c, hipStreamSynchronize(q));
  }
  std::vector<int32_t> total(B, 0);
  w->n_l.assign(B * ORB_LEVELS, 0);
  for (size_t b = 0; b < B; b++) {
    for (int l = 0; l < G.nlevels; l++) {
      const int32_t* m = meta.data() + (b * ORB_LEVELS + l) * ORB_META;
      VO_CHECK(c, m[ORB_N_ROWS] == m[ORB_N_CUT], VO_E_HIP, "the rows behind the FAST cut do not add up to the histogram's count");
      w->n_l[b * ORB_LEVELS + l] = m[ORB_N_KEPT];
      total[b] += m[ORB_N_KEPT];
    }
    VO_CHECK(c, total[b] <= max_out, VO_E_CAPACITY, "more keypoints than max_out");
  }
  // the rows: two read-backs of the whole [batch][max_out] buffers where those are small, else two per sequence
  const size_t rows_all = B * (size_t)max_out;
  const bool whole = rows_all * (sizeof(vo_orb_kp) + 32) <= ((size_t)4 << 20);
  if (whole) {
    w->h_out.resize(rows_all * (sizeof(vo_orb_kp) + 32));
    VO_HIP(c, hipMemcpyAsync(w->h_out.data(), w->d_kps, rows_all * sizeof(vo_orb_kp), hipMemcpyDeviceToHost, q));
    VO_HIP(c, hipMemcpyAsync(w->h_out.data() + rows_all * sizeof(vo_orb_kp), w->d_desc, rows_all * 32, hipMemcpyDeviceToHost, q));
  } else
    for (size_t b = 0; b < B; b++)
      if (total[b] > 0) {
        VO_HIP(c, hipMemcpyAsync(kps + b * (size_t)max_out, w->d_kps + b * (size_t)max_out, sizeof(vo_orb_kp) * total[b], hipMemcpyDeviceToHost, q));
        VO_HIP(c, hipMemcpyAsync(desc + b * (size_t)max_out * 32, w->d_desc + b * (size_t)max_out * 32, (size_t)32 * total[b], hipMemcpyDeviceToHost, q));
      }
  VO_HIP(c, hipStreamSynchronize(q));
  for (size_t b = 0; b < B; b++) {
    n_out[b] = total[b];
    if (whole && total[b] > 0) {
      memcpy(kps + b * (size_t)max_out, w->h_out.data() + b * (size_t)max_out * sizeof(vo_orb_kp), sizeof(vo_orb_kp) * total[b]);
      memcpy(desc + b * (size_t)max_out * 32, w->h_out.data() + rows_all * sizeof(vo_orb_kp) + b * (size_t)max_out * 32, (size_t)32 * total[b]);
    }
  }
  w->G = G;
  w->have = true;
  return VO_OK;
}

extern "C" int32_t vo_orb_levels_read(vo_ctx* c, int32_t* w_l, int32_t* h_l, float* scale_l, int32_t* quota_l, int32_t* n_l) {
  if (!c) return VO_E_INVALID;
  VO_CHECK(c, c->orb && c->orb->have, VO_E_STATE, "no vo_orb_detect_compute has succeeded on this context");
  const vo_orb_ws* w = c->orb;
  for (int l = 0; l < ORB_LEVELS; l++) {
    const bool in = l < w->G.nlevels;
    if (w_l) w_l[l] = in ? w->G.w[l] : 0;
    if (h_l) h_l[l] = in ? w->G.h[l] : 0;
    if (scale_l) scale_l[l] = in ? w->G.scale[l] : 0.f;
    if (quota_l) quota_l[l] = in ? w->G.quota[l] : 0;
  }
  if (n_l) memcpy(n_l, w->n_l.data(), sizeof(int32_t) * w->n_l.size());
  return VO_OK;
}

extern "C" int32_t vo_orb_level_image_read(vo_ctx* c, int32_t seq, int32_t level, uint8_t* out) {
  if (!c) return VO_E_INVALID;
  VO_CHECK(c, c->orb && c->orb->have, VO_E_STATE, "no vo_orb_detect_compute has succeeded on this context");
  const vo_orb_ws* w = c->orb;
  VO_CHECK(c, seq >= 0 && seq < c->batch && level >= 0 && level < w->G.nlevels, VO_E_INVALID, "no such sequence / level");
  const orb_geom& G = w->G;
  if (G.w[level] == 0) return VO_OK;
  VO_CHECK(c, out != nullptr, VO_E_INVALID, "null buffer");
  VO_HIP(c, hipSetDevice(c->device));
  VO_HIP(c, hipMemcpy2DAsync(out, G.w[level], w->d_pyr + (size_t)seq * G.pyr_seq + G.img_off[level] + (size_t)VO_PAD * G.pitch[level] + VO_PAD, G.pitch[level],
                             G.w[level], G.h[level], hipMemcpyDeviceToHost, c->stream));
  VO_HIP(c, hipStreamSynchronize(c->stream));
  return VO_OK;
}
