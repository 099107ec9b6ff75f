// Brute-force 2-nearest-neighbour descriptor matching, plain and guided: one scan per distance kind behind four entry points.
//
// Plain (SURVEY.md 8f "next" row 4, the matching part of the bootstrap): vo_match_knn2 replaces  self._matcher.knnMatch(desc_1, desc_2, k=2)
// with cv2.BFMatcher() (NORM_L2, no cross check) in Extractor.match, the reference's extractor.py:134-145 (the ratio test on the two distances
// stays in the Python adapter, as in the reference); vo_match_hamming_knn2 is cv2.BFMatcher(NORM_HAMMING).knnMatch(k = 2) over binary
// descriptors (the oriented BRIEF of vo_brief.hip).  L2 distance = sqrt of the sum of squared float32 differences (accumulated in float64,
// rounded to float32 once: independent of the summation order; OpenCV accumulates in float32 SIMD lanes -- unpinned at that level),
// neighbours ordered by (distance, train index), as OpenCV's batchDistance keeps the first of equals.
// Guided (vo_match_guided_l2 / vo_match_guided_hamming; definition: include/vo_mi355x.h, section "guided descriptor matching"; numpy model:
// tests/gmatch_model.py, which the kernels equal bit for bit): the same two scans with a per-pair gate in front of the distance, and the
// accept rule (distance ceiling, Lowe's ratio, cross-check) on the device.  The plain calls are the forward scan at gate 0 and nothing else.
//
// The gate decides per (query, train row) pair whether the distance is computed at all:
//   window    (dx dx + dy dy) <= radius^2 in float64 between the train position and the query's centre;
//   epipolar  f7_inlier of vo_epi_dev.h, the consensus test of the fundamental-matrix search, at epi_dist^2.
// GPU mapping: a wave per query, four queries per 256-thread workgroup, grid y = batch; the train rows are scanned 64 at a time, every lane
// keeps its two best and the 64 lane results are merged by shuffles under the same (distance, index) order.  The train positions of a tile
// are staged in LDS as float2 (twice where the window and the epipolar gate read different arrays: the reverse pass with centres); what belongs
// to the query (its centre, its epipolar line) does not depend on the lane and is hoisted out of the scan by the compiler.
//   Hamming  the train set is staged in LDS in tiles of MATCH_TILE_WORDS words (1024 descriptors of 32 bytes at once), every row on a pitch
//            of nw + 1 words: lane l reads row l and an odd pitch spreads the 64 rows over the banks.  The four queries of a workgroup sit in
//            LDS too (every lane of a wave reads the same word: a broadcast).  A rejected row's popcounts are skipped.  Gate 0 has an instance
//            of its own without the position tiles, whose tile is as long as the descriptor words allow.
//   L2       rows are read from memory with 16-byte loads (n1 x n2 x dim x 4 B through L2, 0.5 GB at 1000 x 1000 x 128), the query through a
//            wave-uniform pointer (scalar loads).  A rejected row's 4 dim bytes are never loaded: the lanes ballot the predicate, append the
//            admitted row indices to a ring of 128 in LDS that the wave owns, and whenever it holds 64 every lane takes one and computes its
//            whole row.  The order in which rows reach knn_insert does not matter: (distance, index) is a total order over the rows that can
//            enter (a NaN distance never does).
// The cross-check's reverse pass is the same kernel with the sets swapped: the window's dx changes sign, which its square does not see, and
// the host passes F^T, under which f7_inlier evaluates the same two squared distances in the other order.  k_match_accept applies the rule.
// Rows at or beyond counts[b] do not exist: as queries they get the empty result, as train rows they are never scanned.
#include "vo_internal.h"
#include "vo_epi_dev.h"

#include <math.h>
#include <string.h>

#define MATCH_MAX_WORDS 16
#define MATCH_TILE_WORDS 9216             // the Hamming descriptor tile
#define MATCH_POS_ROWS 1024               // train positions staged at once; a gated Hamming tile holds min(MATCH_POS_ROWS, MATCH_TILE_WORDS / (nw + 1)) rows
#define MATCH_RING 128                    // admitted row indices a wave holds (L2): under 64 left over + 64 appended

// Every buffer is laid out for the call at hand ([batch][n][width] packed), sized in bytes, and only ever grows; the four entry points share
// them.  Beside the two descriptor sets a guided call moves two slabs: every gate input in one upload from a pinned mirror, every output in
// one read-back into a pinned mirror (a copy per array from and to the caller's pageable memory costs more than the kernels at these sizes).
struct vo_match_ws {
  // every buffer counts bytes and only grows; the calls are synchronous, so nothing is in flight when one is replaced
  vo_dev<char> a, b;                      // descriptors
  vo_dev<char> in, out, rev;              // gate inputs; match | idx | dist | n_admitted | rbest; the reverse pass's idx | dist
  vo_pinned<char> h_in, h_out;            // pinned mirrors of in and out
};

struct gm_gate {
  int gate;                               // bit 0 window, bit 1 epipolar
  double r2, e2;                          // radius^2, epi_dist^2
  const double* F;                        // [batch][2][9]
  int f_off;                              // 0: F (forward), 9: F^T (reverse)
  const float2* qw; const float2* qe;     // query side: window centre / epipolar point, [batch][nq]
  const float2* tw; const float2* te;     // train side, [batch][nt]
};

// the pair predicate; qw, tw are read under bit 0 and qe, te under bit 1 only
__device__ __forceinline__ bool gm_admit(int gate, double r2, double e2, const double* F, float2 qw, float2 qe, float2 tw, float2 te) {
  bool ok = true;
  if (gate & 1) {
    const double dx = (double)tw.x - (double)qw.x, dy = (double)tw.y - (double)qw.y;
    ok = (dx * dx + dy * dy) <= r2;
  }
  if (gate & 2) {
    double err;
    ok = f7_inlier(F, (double)qe.x, (double)qe.y, (double)te.x, (double)te.y, e2, err) && ok;
  }
  return ok;
}

// the two best of a scan under (distance, train index); D = float (L2) or int (Hamming).  An empty slot holds (far, 0x7fffffff).
template <class D> struct knn2 { D d0, d1; int i0, i1; };

template <class D> __device__ __forceinline__ knn2<D> knn_empty(D far) { return {far, far, 0x7fffffff, 0x7fffffff}; }

template <class D> __device__ __forceinline__ bool knn_less(D da, int ia, D db, int ib) { return da < db || (da == db && ia < ib); }

template <class D> __device__ __forceinline__ void knn_insert(knn2<D>& s, D d, int i) {
  if (knn_less(d, i, s.d0, s.i0)) { s.d1 = s.d0; s.i1 = s.i0; s.d0 = d; s.i0 = i; }
  else if (knn_less(d, i, s.d1, s.i1)) { s.d1 = d; s.i1 = i; }
}

// the 64 lane records of a wave -> the wave's record, in every lane
template <class D> __device__ __forceinline__ void knn_merge(knn2<D>& s) {
  for (int o = 32; o > 0; o >>= 1) {
    const D od0 = __shfl_xor(s.d0, o), od1 = __shfl_xor(s.d1, o);
    const int oi0 = __shfl_xor(s.i0, o), oi1 = __shfl_xor(s.i1, o);
    knn_insert(s, od0, oi0);
    knn_insert(s, od1, oi1);
  }
}

// row o of idx, dist [..][2]: an empty slot's index is -1
template <class D> __device__ __forceinline__ void knn_store(const knn2<D>& s, size_t o, int32_t* __restrict__ idx, D* __restrict__ dist) {
  idx[o * 2] = (s.i0 == 0x7fffffff) ? -1 : s.i0; idx[o * 2 + 1] = (s.i1 == 0x7fffffff) ? -1 : s.i1;
  dist[o * 2] = s.d0; dist[o * 2 + 1] = s.d1;
}

// bit distance of two rows of nw words: __popcll over word pairs, __popc over an odd last word
__device__ __forceinline__ int match_hamming(const uint32_t* q, const uint32_t* r, int nw) {
  int d = 0, k = 0;
  for (; k + 1 < nw; k += 2) d += __popcll(((unsigned long long)(q[k + 1] ^ r[k + 1]) << 32) | (unsigned long long)(q[k] ^ r[k]));
  if (k < nw) d += __popc(q[k] ^ r[k]);
  return d;
}

// float64 sum of the squared float32 differences in ascending k, rounded to float32 once, sqrtf
__device__ __forceinline__ float match_l2(const float* __restrict__ q, const float* __restrict__ r, int dim) {
  double acc = 0.0;
  int k = 0;
  if ((dim & 3) == 0) {
    for (; k < dim; k += 4) {
      const float4 x = *reinterpret_cast<const float4*>(r + k);
      const float4 y = *reinterpret_cast<const float4*>(q + k);
      const double e0 = (double)y.x - (double)x.x, e1 = (double)y.y - (double)x.y, e2 = (double)y.z - (double)x.z, e3 = (double)y.w - (double)x.w;
      acc += e0 * e0; acc += e1 * e1; acc += e2 * e2; acc += e3 * e3;
    }
  }
  for (; k < dim; k++) { const double e = (double)q[k] - (double)r[k]; acc += e * e; }
  return sqrtf((float)acc);
}

// A [batch][nq][nw], Bm [batch][nt][nw] words; idx, dist [batch][nq][2]; nadm [batch][nq] or null.  grid (ceil(nq / 4), batch), 256 threads.
// GATED = false is the instance of gate 0 and of vo_match_hamming_knn2: no position tiles in LDS (so a tile is not cut at MATCH_POS_ROWS),
// no gate state in registers and no count of admitted rows -- every row below the train count is admitted
template <bool GATED>
__global__ void __launch_bounds__(256) k_match_hamming(const uint32_t* __restrict__ A, const uint32_t* __restrict__ Bm, int nq, int nt, int nw,
                                                       const int32_t* __restrict__ cntq, const int32_t* __restrict__ cntt,
                                                       int32_t* __restrict__ idx, int32_t* __restrict__ dist, int32_t* __restrict__ nadm, gm_gate g) {
  __shared__ uint32_t tile[MATCH_TILE_WORDS];
  __shared__ uint32_t qs[4][MATCH_MAX_WORDS];
  __shared__ float2 posw[GATED ? MATCH_POS_ROWS : 1], pose[GATED ? MATCH_POS_ROWS : 1];
  const int gate = GATED ? g.gate : 0;
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qi = blockIdx.x * 4 + wave;
  const int nq_b = cntq ? cntq[b] : nq, nt_b = cntt ? cntt[b] : nt;
  const bool live = qi < nq;                       // the wave has an output row
  const bool active = qi < nq_b;                   // ... and a query (a wave without one still loads tiles and meets the barriers)
  if (active && lane < nw) qs[wave][lane] = A[((size_t)b * nq + qi) * nw + lane];
  const float2 zero = make_float2(0.f, 0.f);
  float2 qw = zero, qe = zero;
  if (active && (gate & 1)) qw = g.qw[(size_t)b * nq + qi];
  if (active && (gate & 2)) qe = g.qe[(size_t)b * nq + qi];
  double F[9];
#pragma unroll
  for (int k = 0; k < 9; k++) F[k] = (gate & 2) ? g.F[(size_t)b * 18 + g.f_off + k] : 0.0;
  const uint32_t* const T = Bm + (size_t)b * nt * nw;
  const int pitch = nw + 1, rows_tile = GATED ? min(MATCH_TILE_WORDS / pitch, MATCH_POS_ROWS) : MATCH_TILE_WORDS / pitch;
  knn2<int> s = knn_empty(0x7fffffff);
  int na = 0;
  for (int j0 = 0; j0 < nt_b; j0 += rows_tile) {
    const int rows = min(rows_tile, nt_b - j0);
    __syncthreads();                               // the previous tile has been read (first pass: the queries are written)
    for (int k = threadIdx.x; k < rows * nw; k += 256) {
      const int r = k / nw, q = k - r * nw;
      tile[r * pitch + q] = T[(size_t)j0 * nw + k];
    }
    for (int r = threadIdx.x; r < rows; r += 256) {
      if (gate & 1) posw[r] = g.tw[(size_t)b * nt + j0 + r];
      if (gate & 2) pose[r] = g.te[(size_t)b * nt + j0 + r];
    }
    __syncthreads();
    if (active)
      for (int j = lane; j < rows; j += 64) {
        float2 tw = zero, te = zero;
        if (gate & 1) tw = posw[j];
        if (gate & 2) te = pose[j];
        if (gm_admit(gate, g.r2, g.e2, F, qw, qe, tw, te)) {
          if (GATED) na++;
          knn_insert(s, match_hamming(qs[wave], tile + j * pitch, nw), j0 + j);
        }
      }
  }
  knn_merge(s);
  if (GATED) { for (int o = 32; o > 0; o >>= 1) na += __shfl_xor(na, o); }
  else na = active ? nt_b : 0;
  if (live && lane == 0) {
    const size_t o = (size_t)b * nq + qi;
    knn_store(s, o, idx, dist);
    if (nadm) nadm[o] = na;
  }
}

// A [batch][nq][dim], Bm [batch][nt][dim] f32; idx, dist [batch][nq][2]; nadm [batch][nq] or null.  grid (ceil(nq / 4), batch), 256 threads
__global__ void __launch_bounds__(256) k_match_l2(const float* __restrict__ A, const float* __restrict__ Bm, int nq, int nt, int dim,
                                                  const int32_t* __restrict__ cntq, const int32_t* __restrict__ cntt,
                                                  int32_t* __restrict__ idx, float* __restrict__ dist, int32_t* __restrict__ nadm, gm_gate g) {
  __shared__ float2 posw[MATCH_POS_ROWS], pose[MATCH_POS_ROWS];
  __shared__ int ring[4][MATCH_RING];
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);     // uniform: the query's row is read by scalar loads
  const int qi = blockIdx.x * 4 + wave;
  const int nq_b = cntq ? cntq[b] : nq, nt_b = cntt ? cntt[b] : nt;
  const bool live = qi < nq, active = qi < nq_b;
  const float* const q = A + ((size_t)b * nq + (active ? qi : 0)) * dim;
  const float* const T = Bm + (size_t)b * nt * dim;
  const float2 zero = make_float2(0.f, 0.f);
  float2 qw = zero, qe = zero;
  if (active && (g.gate & 1)) qw = g.qw[(size_t)b * nq + qi];
  if (active && (g.gate & 2)) qe = g.qe[(size_t)b * nq + qi];
  double F[9];
#pragma unroll
  for (int k = 0; k < 9; k++) F[k] = (g.gate & 2) ? g.F[(size_t)b * 18 + g.f_off + k] : 0.0;
  volatile int* const rg = ring[wave];
  knn2<float> s = knn_empty(__builtin_inff());
  int head = 0, tail = 0;                          // wave-uniform; tail - head entries wait in the ring
  for (int j0 = 0; j0 < nt_b; j0 += MATCH_POS_ROWS) {
    const int rows = min(MATCH_POS_ROWS, nt_b - j0);
    __syncthreads();                               // the previous tile's positions have been read
    for (int r = threadIdx.x; r < rows; r += 256) {
      if (g.gate & 1) posw[r] = g.tw[(size_t)b * nt + j0 + r];
      if (g.gate & 2) pose[r] = g.te[(size_t)b * nt + j0 + r];
    }
    __syncthreads();
    if (active)
      for (int c0 = 0; c0 < rows; c0 += 64) {
        const int r = c0 + lane;
        bool adm = r < rows;
        if (adm) {
          float2 tw = zero, te = zero;
          if (g.gate & 1) tw = posw[r];
          if (g.gate & 2) te = pose[r];
          adm = gm_admit(g.gate, g.r2, g.e2, F, qw, qe, tw, te);
        }
        const unsigned long long m = __ballot(adm);
        if (adm) rg[(tail + __popcll(m & ((1ull << lane) - 1ull))) & (MATCH_RING - 1)] = j0 + r;
        tail += __popcll(m);
        __builtin_amdgcn_wave_barrier();
        if (tail - head >= 64) {
          const int j = rg[(head + lane) & (MATCH_RING - 1)];
          head += 64;
          knn_insert(s, match_l2(q, T + (size_t)j * dim, dim), j);
          __builtin_amdgcn_wave_barrier();
        }
      }
  }
  if (lane < tail - head) {
    const int j = rg[(head + lane) & (MATCH_RING - 1)];
    knn_insert(s, match_l2(q, T + (size_t)j * dim, dim), j);
  }
  knn_merge(s);
  if (live && lane == 0) {
    const size_t o = (size_t)b * nq + qi;
    knn_store(s, o, idx, dist);
    if (nadm) nadm[o] = tail;
  }
}

// the accept rule, a thread per query, and rbest = column 0 of the reverse pass, a thread per train row.  grid (ceil(max(n1, n2) / 256), batch)
template <class D>
__global__ void __launch_bounds__(256) k_match_accept(const int32_t* __restrict__ idx, const D* __restrict__ dist, const int32_t* __restrict__ ridx,
                                                      int n1, int n2, int cross, double ratio, double max_dist, int32_t* __restrict__ match,
                                                      int32_t* __restrict__ rbest) {
  const int b = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (t < n1) {
    const size_t o = (size_t)b * n1 + t;
    const int i0 = idx[o * 2], i1 = idx[o * 2 + 1];
    bool ok = i0 >= 0;
    if (ok) {
      const double d0 = (double)dist[o * 2], d1 = (double)dist[o * 2 + 1];
      ok = d0 <= max_dist;
      ok = ok && (ratio == 1.0 || i1 < 0 || d0 < ratio * d1);
      ok = ok && (!cross || ridx[((size_t)b * n2 + i0) * 2] == t);
    }
    match[o] = ok ? i0 : -1;
  }
  if (t < n2) rbest[(size_t)b * n2 + t] = cross ? ridx[((size_t)b * n2 + t) * 2] : -1;
}

void vo_match_destroy(vo_ctx* c) {
  delete c->match;
  c->match = nullptr;
}

extern "C" int32_t vo_gmatch_default_params(vo_gmatch_params* p) {
  if (!p) return VO_E_INVALID;
  p->gate = 0; p->cross_check = 0; p->radius = 0.0; p->epi_dist = 0.0; p->ratio = 1.0; p->max_dist = (double)INFINITY;
  return VO_OK;
}

// one scan on the context's stream, queries A against train rows Bm
template <bool HAM, class DT>
static void gm_scan(vo_ctx* c, const void* A, const void* Bm, int nq, int nt, int width, const int32_t* cntq, const int32_t* cntt, const gm_gate& g,
                    int32_t* idx, DT* dist, int32_t* nadm) {
  const dim3 grid(vo_div_up(nq, 4), (unsigned)c->batch);
  if constexpr (HAM)
    hipLaunchKernelGGL(g.gate ? k_match_hamming<true> : k_match_hamming<false>, grid, dim3(256), 0, c->stream, (const uint32_t*)A, (const uint32_t*)Bm,
                       nq, nt, width, cntq, cntt, idx, dist, nadm, g);
  else
    hipLaunchKernelGGL(k_match_l2, grid, dim3(256), 0, c->stream, (const float*)A, (const float*)Bm, nq, nt, width, cntq, cntt, idx, dist, nadm, g);
}

// The four entry points behind their own argument checks (this function's name is part of its own checks' messages).  width: words per row
// (Hamming) or floats per row (L2); DT: the distance type.
// match = null is a plain call: gate 0 without counts, the forward scan alone (no gate slab, reverse pass, accept launch or profile region),
// idx and dist read back.
template <bool HAM, class DT>
static int32_t gm_run(vo_ctx* c, const void* desc1, int32_t n1, const void* desc2, int32_t n2, int32_t width, const float* pts1, const float* pts2,
                      const float* centers, const double* F, const int32_t* counts1, const int32_t* counts2, const vo_gmatch_params* prm,
                      int32_t* match, int32_t* idx, DT* dist, int32_t* n_admitted, int32_t* rbest) {
  vo_gmatch_params P;
  vo_gmatch_default_params(&P);
  if (prm) P = *prm;
  VO_CHECK(c, P.gate >= 0 && P.gate <= 3, VO_E_INVALID, "gate must be in 0..3");
  VO_CHECK(c, P.cross_check == 0 || P.cross_check == 1, VO_E_INVALID, "cross_check must be 0 or 1");
  VO_CHECK(c, !(P.gate & 1) || (P.radius > 0 && std::isfinite(P.radius)), VO_E_INVALID, "the window gate needs a finite radius > 0");
  VO_CHECK(c, !(P.gate & 2) || (P.epi_dist > 0 && std::isfinite(P.epi_dist)), VO_E_INVALID, "the epipolar gate needs a finite epi_dist > 0");
  VO_CHECK(c, P.gate == 0 || (pts1 && pts2), VO_E_INVALID, "a gate needs pts1 and pts2");
  VO_CHECK(c, !(P.gate & 2) || F, VO_E_INVALID, "the epipolar gate needs F");
  VO_CHECK(c, P.ratio > 0 && P.ratio <= 1, VO_E_INVALID, "ratio must be in (0, 1]");
  VO_CHECK(c, P.max_dist >= 0, VO_E_INVALID, "max_dist must be >= 0 (inf = off)");
  const size_t B = c->batch;
  for (size_t b = 0; b < B; b++) {
    VO_CHECK(c, !counts1 || (counts1[b] >= 0 && counts1[b] <= n1), VO_E_INVALID, "counts1 outside 0..n1");
    VO_CHECK(c, !counts2 || (counts2[b] >= 0 && counts2[b] <= n2), VO_E_INVALID, "counts2 outside 0..n2");
  }
  VO_HIP(c, hipSetDevice(c->device));
  if (!c->match) c->match = new vo_match_ws();
  vo_match_ws* w = c->match;
  const size_t N1 = (size_t)n1 * B, N2 = (size_t)n2 * B, row = 4 * (size_t)width;
  const int cross = P.cross_check;
  // the input slab: F and F^T [batch][2][9] f64 | pts1 | pts2 | centers (float2 each) | counts1 | counts2
  const size_t o_p1 = B * 18 * sizeof(double), o_p2 = o_p1 + N1 * sizeof(float2), o_ce = o_p2 + N2 * sizeof(float2),
               o_c1 = o_ce + N1 * sizeof(float2), o_c2 = o_c1 + B * sizeof(int32_t), in_bytes = o_c2 + B * sizeof(int32_t);
  // the output slab: match | idx | dist | n_admitted | rbest
  const size_t o_idx = N1 * sizeof(int32_t), o_dist = o_idx + N1 * 2 * sizeof(int32_t), o_nadm = o_dist + N1 * 2 * sizeof(DT),
               o_rbest = o_nadm + N1 * sizeof(int32_t), out_bytes = o_rbest + N2 * sizeof(int32_t);
  VO_HIP(c, w->a.reserve(N1 * row));
  VO_HIP(c, w->b.reserve(N2 * row));
  VO_HIP(c, w->in.reserve(in_bytes));
  VO_HIP(c, w->out.reserve(out_bytes));
  if (cross) VO_HIP(c, w->rev.reserve(N2 * 2 * (sizeof(int32_t) + sizeof(DT))));
  // the 2-D form: the runtime stages the rows and copies them on the device; after the 1-D form (a host-to-device transfer from the caller's
  // pageable memory) the Hamming scan took 0.3 - 0.5 us longer in a kernel trace and the call 3 - 20 us longer (EXPERIMENTS.md)
  VO_HIP(c, hipMemcpy2DAsync(w->a.get(), n1 * row, desc1, n1 * row, n1 * row, B, hipMemcpyHostToDevice, c->stream));
  VO_HIP(c, hipMemcpy2DAsync(w->b.get(), n2 * row, desc2, n2 * row, n2 * row, B, hipMemcpyHostToDevice, c->stream));
  const bool use_ce = (P.gate & 1) && centers;
  if (P.gate || counts1 || counts2) {
    VO_HIP(c, w->h_in.reserve(in_bytes));
    char* const h = (char*)w->h_in.get();
    if (P.gate & 2) {
      double* hF = (double*)h;
      for (size_t b = 0; b < B; b++)
        for (int i = 0; i < 3; i++)
          for (int j = 0; j < 3; j++) {
            hF[b * 18 + i * 3 + j] = F[b * 9 + i * 3 + j];
            hF[b * 18 + 9 + i * 3 + j] = F[b * 9 + j * 3 + i];
          }
    }
    if (P.gate) { memcpy(h + o_p1, pts1, N1 * sizeof(float2)); memcpy(h + o_p2, pts2, N2 * sizeof(float2)); }
    if (use_ce) memcpy(h + o_ce, centers, N1 * sizeof(float2));
    if (counts1) memcpy(h + o_c1, counts1, B * sizeof(int32_t));
    if (counts2) memcpy(h + o_c2, counts2, B * sizeof(int32_t));
    VO_HIP(c, hipMemcpyAsync(w->in.get(), h, in_bytes, hipMemcpyHostToDevice, c->stream));
  }
  char* const din = (char*)w->in.get(); char* const dout = (char*)w->out.get();
  const float2* const dp1 = (const float2*)(din + o_p1); const float2* const dp2 = (const float2*)(din + o_p2);
  const float2* const dc = use_ce ? (const float2*)(din + o_ce) : dp1;
  const int32_t* const dc1 = counts1 ? (const int32_t*)(din + o_c1) : nullptr; const int32_t* const dc2 = counts2 ? (const int32_t*)(din + o_c2) : nullptr;
  int32_t* const d_match = (int32_t*)dout; int32_t* const d_idx = (int32_t*)(dout + o_idx); DT* const d_dist = (DT*)(dout + o_dist);
  int32_t* const d_nadm = (int32_t*)(dout + o_nadm); int32_t* const d_rbest = (int32_t*)(dout + o_rbest);
  int32_t* const d_ridx = (int32_t*)w->rev.get(); DT* const d_rdist = (DT*)((char*)w->rev.get() + N2 * 2 * sizeof(int32_t));
  gm_gate g;
  g.gate = P.gate; g.r2 = P.radius * P.radius; g.e2 = P.epi_dist * P.epi_dist; g.F = (const double*)din;
  g.f_off = 0; g.qw = dc; g.qe = dp1; g.tw = dp2; g.te = dp2;
  if (!match) {                                    // a plain call: the scan, and idx and dist straight into the caller's arrays (no pinned mirror:
                                                   // through it the call is 14 us shorter, the Hamming scan 0.4 - 0.9 us longer in a kernel trace)
    gm_scan<HAM>(c, w->a.get(), w->b.get(), n1, n2, width, dc1, dc2, g, d_idx, d_dist, (int32_t*)nullptr);
    VO_HIP(c, hipGetLastError());
    const size_t ri = (size_t)n1 * 2 * sizeof(int32_t), rd = (size_t)n1 * 2 * sizeof(DT);
    VO_HIP(c, hipMemcpy2DAsync(idx, ri, d_idx, ri, ri, B, hipMemcpyDeviceToHost, c->stream));
    VO_HIP(c, hipMemcpy2DAsync(dist, rd, d_dist, rd, rd, B, hipMemcpyDeviceToHost, c->stream));
    VO_HIP(c, hipStreamSynchronize(c->stream));
    return VO_OK;
  }
  {
    vo_prof_scope prof(c, c->stream, VO_PROF_GMATCH_FORWARD);
    gm_scan<HAM>(c, w->a.get(), w->b.get(), n1, n2, width, dc1, dc2, g, d_idx, d_dist, d_nadm);
  }
  VO_HIP(c, hipGetLastError());
  if (cross) {                                     // the reverse pass: the train rows ask, the queries answer
    gm_gate gr = g;
    gr.f_off = 9; gr.qw = dp2; gr.qe = dp2; gr.tw = dc; gr.te = dp1;
    vo_prof_scope prof(c, c->stream, VO_PROF_GMATCH_REVERSE);
    gm_scan<HAM>(c, w->b.get(), w->a.get(), n2, n1, width, dc2, dc1, gr, d_ridx, d_rdist, (int32_t*)nullptr);
  }
  VO_HIP(c, hipGetLastError());
  {
    vo_prof_scope prof(c, c->stream, VO_PROF_GMATCH_ACCEPT);
    hipLaunchKernelGGL(k_match_accept<DT>, dim3(vo_div_up(n1 > n2 ? n1 : n2, 256), (unsigned)B), dim3(256), 0, c->stream, (const int32_t*)d_idx,
                       (const DT*)d_dist, (const int32_t*)d_ridx, n1, n2, cross, P.ratio, P.max_dist, d_match, d_rbest);
  }
  VO_HIP(c, hipGetLastError());
  VO_HIP(c, w->h_out.reserve(out_bytes));
  const char* const ho = (const char*)w->h_out.get();
  VO_HIP(c, hipMemcpyAsync(w->h_out.get(), dout, out_bytes, hipMemcpyDeviceToHost, c->stream));
  VO_HIP(c, hipStreamSynchronize(c->stream));
  memcpy(match, ho, N1 * sizeof(int32_t));
  if (idx) memcpy(idx, ho + o_idx, N1 * 2 * sizeof(int32_t));
  if (dist) memcpy(dist, ho + o_dist, N1 * 2 * sizeof(DT));
  if (n_admitted) memcpy(n_admitted, ho + o_nadm, N1 * sizeof(int32_t));
  if (rbest) memcpy(rbest, ho + o_rbest, N2 * sizeof(int32_t));
  return VO_OK;
}

// what every entry point checks of its sets, under its own name in the message
#define MATCH_CHECK_SETS(outputs, width_ok)                                                      \
  if (!c) return VO_E_INVALID;                                                                   \
  VO_CHECK(c, desc1 && desc2 && (outputs), VO_E_INVALID, "null buffer");                         \
  VO_CHECK(c, n1 >= 1 && n2 >= 1 && (width_ok), VO_E_INVALID, "empty descriptor set")
#define MATCH_CHECK_NBYTES() \
  VO_CHECK(c, nbytes >= 4 && nbytes <= 4 * MATCH_MAX_WORDS && nbytes % 4 == 0, VO_E_INVALID, "nbytes must be a multiple of 4 in 4..64")

// desc1 [batch][n1][dim], desc2 [batch][n2][dim] f32 -> idx [batch][n1][2] (train index of the nearest / second nearest,
// -1 if n2 < 2 leaves the slot empty), dist [batch][n1][2] f32 (inf for an empty slot).  A NaN anywhere in a train
// descriptor makes its distance NaN, which never beats a finite one.
extern "C" int32_t vo_match_knn2(vo_ctx* c, const float* desc1, int32_t n1, const float* desc2, int32_t n2, int32_t dim,
                                 int32_t* idx, float* dist) {
  MATCH_CHECK_SETS(idx && dist, dim >= 1);
  return gm_run<false, float>(c, desc1, n1, desc2, n2, dim, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, idx, dist, nullptr, nullptr);
}

// desc1 [batch][n1][nbytes], desc2 [batch][n2][nbytes] u8 -> idx [batch][n1][2] (train index of the nearest / second nearest under the bit
// distance, ordered by (distance, train index); -1 where n2 < 2 leaves the slot empty), dist [batch][n1][2] i32 (INT32_MAX for an empty slot)
extern "C" int32_t vo_match_hamming_knn2(vo_ctx* c, const uint8_t* desc1, int32_t n1, const uint8_t* desc2, int32_t n2, int32_t nbytes,
                                         int32_t* idx, int32_t* dist) {
  MATCH_CHECK_SETS(idx && dist, true);
  MATCH_CHECK_NBYTES();
  return gm_run<true, int32_t>(c, desc1, n1, desc2, n2, nbytes / 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, idx, dist, nullptr, nullptr);
}

extern "C" int32_t vo_match_guided_hamming(vo_ctx* c, const uint8_t* desc1, int32_t n1, const uint8_t* desc2, int32_t n2, int32_t nbytes,
                                           const float* pts1, const float* pts2, const float* centers, const double* F, const int32_t* counts1,
                                           const int32_t* counts2, const vo_gmatch_params* prm, int32_t* match, int32_t* idx, int32_t* dist,
                                           int32_t* n_admitted, int32_t* rbest) {
  MATCH_CHECK_SETS(match, true);
  MATCH_CHECK_NBYTES();
  return gm_run<true, int32_t>(c, desc1, n1, desc2, n2, nbytes / 4, pts1, pts2, centers, F, counts1, counts2, prm, match, idx, dist, n_admitted, rbest);
}

extern "C" int32_t vo_match_guided_l2(vo_ctx* c, const float* desc1, int32_t n1, const float* desc2, int32_t n2, int32_t dim, const float* pts1,
                                      const float* pts2, const float* centers, const double* F, const int32_t* counts1, const int32_t* counts2,
                                      const vo_gmatch_params* prm, int32_t* match, int32_t* idx, float* dist, int32_t* n_admitted, int32_t* rbest) {
  MATCH_CHECK_SETS(match, dim >= 1);
  return gm_run<false, float>(c, desc1, n1, desc2, n2, dim, pts1, pts2, centers, F, counts1, counts2, prm, match, idx, dist, n_admitted, rbest);
}
