// Brute-force 2-nearest-neighbour descriptor matching (SURVEY.md 8f "next" row 4, the matching part of the bootstrap).
//
// Replaces  self._matcher.knnMatch(desc_1, desc_2, k=2)  with cv2.BFMatcher() (NORM_L2, no cross check) in
// Extractor.match, /root/reference/src/extractor/extractor.py:134-145 (the ratio test on the two distances stays in the
// Python adapter, as in the reference); called once per sequence through match_lists by Pipeline._get_init_state,
// pipeline.py:52.  Distance = sqrt of the sum of squared float32 differences (accumulated in float64, rounded to
// float32 once: independent of the summation order; OpenCV accumulates in float32 SIMD lanes -- unpinned at that
// level), neighbours ordered by (distance, train index), as OpenCV's batchDistance keeps the first of equals.
//
// GPU mapping: a wave per query descriptor; lane l scans train rows l, l + 64, ... with 16-byte loads (the query is
// wave-uniform -> scalar loads), keeps its two best, the 64 lane pairs are merged by shuffles.  HBM/L2 traffic is
// n1 x n2 x dim x 4 B (0.5 GB at 1000 x 1000 x 128): a one-off per sequence, not tiled further.
#include "vo_internal.h"

#include <math.h>

struct vo_match_ws {
  size_t cap1 = 0, cap2 = 0;       // floats per sequence
  int cap_q = 0;
  float* d_a = nullptr; float* d_b = nullptr;
  int32_t* d_idx = nullptr; float* d_dist = nullptr;
  // the Hamming matcher's own buffers (vo_match_hamming_knn2): 32-bit words per sequence
  size_t hcap1 = 0, hcap2 = 0;
  int hcap_q = 0;
  uint32_t* d_ha = nullptr; uint32_t* d_hb = nullptr;
  int32_t* d_hidx = nullptr; int32_t* d_hdist = nullptr;
};

struct knn2 { float d0, d1; int i0, i1; };

__device__ __forceinline__ bool knn_less(float da, int ia, float db, int ib) { return da < db || (da == db && ia < ib); }

__device__ __forceinline__ void knn_insert(knn2& s, float d, int i) {
  if (knn_less(d, i, s.d0, s.i0)) { s.d1 = s.d0; s.i1 = s.i0; s.d0 = d; s.i0 = i; }
  else if (knn_less(d, i, s.d1, s.i1)) { s.d1 = d; s.i1 = i; }
}

// grid (ceil(n1 / 4), batch), 256 threads = 4 queries
__global__ void __launch_bounds__(256) k_match_knn2(const float* __restrict__ A, const float* __restrict__ Bm, int n1, int n2, int dim,
                                                    size_t seq_a, size_t seq_b, int32_t* __restrict__ idx, float* __restrict__ dist, int cap_q) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int qi = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (qi >= n1) return;
  const float* q = A + (size_t)b * seq_a + (size_t)qi * dim;
  const float* T = Bm + (size_t)b * seq_b;
  knn2 s;
  s.d0 = s.d1 = __builtin_inff(); s.i0 = s.i1 = 0x7fffffff;
  for (int j = lane; j < n2; j += 64) {
    const float* r = T + (size_t)j * dim;
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
    knn_insert(s, sqrtf((float)acc), j);
  }
  for (int o = 32; o > 0; o >>= 1) {
    const float od0 = __shfl_xor(s.d0, o), od1 = __shfl_xor(s.d1, o);
    const int oi0 = __shfl_xor(s.i0, o), oi1 = __shfl_xor(s.i1, o);
    knn_insert(s, od0, oi0);
    knn_insert(s, od1, oi1);
  }
  if (lane == 0) {
    int32_t* io = idx + ((size_t)b * cap_q + qi) * 2;
    float* dd = dist + ((size_t)b * cap_q + qi) * 2;
    io[0] = (s.i0 == 0x7fffffff) ? -1 : s.i0; io[1] = (s.i1 == 0x7fffffff) ? -1 : s.i1;
    dd[0] = s.d0; dd[1] = s.d1;
  }
}

// ---- Hamming 2-NN over binary descriptors (the oriented BRIEF of vo_brief.hip): cv2.BFMatcher(NORM_HAMMING).knnMatch(k = 2) ----
// The same wave-per-query mapping and shuffle merge as k_match_knn2, on integer bit distances.  The train set is staged in LDS in tiles of
// HAM_TILE_WORDS words (1024 descriptors of 32 bytes at once), every row on a pitch of nw + 1 words: lane l reads row l and an odd pitch
// spreads the 64 rows over the banks.  The four queries of a workgroup sit in LDS too (every lane of a wave reads the same word: a broadcast).
#define HAM_MAX_WORDS 16
#define HAM_TILE_WORDS 9216

struct knn2i { int d0, d1; int i0, i1; };

__device__ __forceinline__ bool knn_less(int da, int ia, int db, int ib) { return da < db || (da == db && ia < ib); }

__device__ __forceinline__ void knn_insert(knn2i& s, int d, int i) {
  if (knn_less(d, i, s.d0, s.i0)) { s.d1 = s.d0; s.i1 = s.i0; s.d0 = d; s.i0 = i; }
  else if (knn_less(d, i, s.d1, s.i1)) { s.d1 = d; s.i1 = i; }
}

// grid (ceil(n1 / 4), batch), 256 threads = 4 queries; A [batch][seq_a words], Bm [batch][seq_b words], rows of nw words
__global__ void __launch_bounds__(256) k_match_hamming_knn2(const uint32_t* __restrict__ A, const uint32_t* __restrict__ Bm, int n1, int n2, int nw,
                                                            size_t seq_a, size_t seq_b, int32_t* __restrict__ idx, int32_t* __restrict__ dist, int cap_q) {
  __shared__ uint32_t tile[HAM_TILE_WORDS];
  __shared__ uint32_t qs[4][HAM_MAX_WORDS];
  const int b = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qi = blockIdx.x * 4 + wave;
  const bool live = qi < n1;                       // (a wave without a query still loads tiles and meets the barriers)
  if (live && lane < nw) qs[wave][lane] = A[(size_t)b * seq_a + (size_t)qi * nw + lane];
  const uint32_t* const T = Bm + (size_t)b * seq_b;
  const int pitch = nw + 1, rows_tile = HAM_TILE_WORDS / pitch;
  knn2i s;
  s.d0 = s.d1 = 0x7fffffff; s.i0 = s.i1 = 0x7fffffff;
  for (int j0 = 0; j0 < n2; j0 += rows_tile) {
    const int rows = min(rows_tile, n2 - j0);
    __syncthreads();                               // the previous tile has been read (first pass: the queries are written)
    for (int k = threadIdx.x; k < rows * nw; k += 256) {
      const int r = k / nw, q = k - r * nw;
      tile[r * pitch + q] = T[(size_t)j0 * nw + k];
    }
    __syncthreads();
    if (live)
      for (int j = lane; j < rows; j += 64) {
        const uint32_t* const r = tile + j * pitch;
        const uint32_t* const q = qs[wave];
        int d = 0, k = 0;
        for (; k + 1 < nw; k += 2) d += __popcll(((unsigned long long)(q[k + 1] ^ r[k + 1]) << 32) | (unsigned long long)(q[k] ^ r[k]));
        if (k < nw) d += __popc(q[k] ^ r[k]);
        knn_insert(s, d, j0 + j);
      }
  }
  for (int o = 32; o > 0; o >>= 1) {
    const int od0 = __shfl_xor(s.d0, o), od1 = __shfl_xor(s.d1, o);
    const int oi0 = __shfl_xor(s.i0, o), oi1 = __shfl_xor(s.i1, o);
    knn_insert(s, od0, oi0);
    knn_insert(s, od1, oi1);
  }
  if (live && lane == 0) {
    int32_t* io = idx + ((size_t)b * cap_q + qi) * 2;
    int32_t* dd = dist + ((size_t)b * cap_q + qi) * 2;
    io[0] = (s.i0 == 0x7fffffff) ? -1 : s.i0; io[1] = (s.i1 == 0x7fffffff) ? -1 : s.i1;
    dd[0] = s.d0; dd[1] = s.d1;
  }
}

void vo_match_destroy(vo_ctx* c) {
  if (!c->match) return;
  vo_match_ws* w = c->match;
  void* bufs[] = {w->d_a, w->d_b, w->d_idx, w->d_dist, w->d_ha, w->d_hb, w->d_hidx, w->d_hdist};
  for (void* p : bufs) if (p) (void)hipFree(p);
  delete w;
  c->match = nullptr;
}

// desc1 [batch][n1][dim], desc2 [batch][n2][dim] f32 -> idx [batch][n1][2] (train index of the nearest / second nearest,
// -1 if n2 < 2 leaves the slot empty), dist [batch][n1][2] f32 (inf for an empty slot).  A NaN anywhere in a train
// descriptor makes its distance NaN, which never beats a finite one.
extern "C" int32_t vo_match_knn2(vo_ctx* c, const float* desc1, int32_t n1, const float* desc2, int32_t n2, int32_t dim,
                                 int32_t* idx, float* dist) {
  if (!c) return VO_E_INVALID;
  VO_CHECK(c, desc1 && desc2 && idx && dist, VO_E_INVALID, "null buffer");
  VO_CHECK(c, n1 >= 1 && n2 >= 1 && dim >= 1, VO_E_INVALID, "empty descriptor set");
  VO_HIP(c, hipSetDevice(c->device));
  const size_t B = c->batch;
  const size_t na = (size_t)n1 * dim, nb = (size_t)n2 * dim;
  if (c->match && (c->match->cap1 < na || c->match->cap2 < nb || c->match->cap_q < n1)) vo_match_destroy(c);
  if (!c->match) {
    vo_match_ws* w = new vo_match_ws();
    c->match = w;
    w->cap1 = na; w->cap2 = nb; w->cap_q = n1;
    VO_HIP(c, hipMalloc((void**)&w->d_a, sizeof(float) * na * B));
    VO_HIP(c, hipMalloc((void**)&w->d_b, sizeof(float) * nb * B));
    VO_HIP(c, hipMalloc((void**)&w->d_idx, sizeof(int32_t) * 2 * (size_t)n1 * B));
    VO_HIP(c, hipMalloc((void**)&w->d_dist, sizeof(float) * 2 * (size_t)n1 * B));
  }
  vo_match_ws* w = c->match;
  VO_HIP(c, hipMemcpy2DAsync(w->d_a, sizeof(float) * w->cap1, desc1, sizeof(float) * na, sizeof(float) * na, B, hipMemcpyHostToDevice, c->stream));
  VO_HIP(c, hipMemcpy2DAsync(w->d_b, sizeof(float) * w->cap2, desc2, sizeof(float) * nb, sizeof(float) * nb, B, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_match_knn2, dim3(vo_div_up(n1, 4), (unsigned)B), dim3(256), 0, c->stream, w->d_a, w->d_b, n1, n2, dim, w->cap1, w->cap2,
                     w->d_idx, w->d_dist, w->cap_q);
  VO_HIP(c, hipGetLastError());
  VO_HIP(c, hipMemcpy2DAsync(idx, sizeof(int32_t) * 2 * n1, w->d_idx, sizeof(int32_t) * 2 * w->cap_q, sizeof(int32_t) * 2 * n1, B, hipMemcpyDeviceToHost, c->stream));
  VO_HIP(c, hipMemcpy2DAsync(dist, sizeof(float) * 2 * n1, w->d_dist, sizeof(float) * 2 * w->cap_q, sizeof(float) * 2 * n1, B, hipMemcpyDeviceToHost, c->stream));
  VO_HIP(c, hipStreamSynchronize(c->stream));
  return VO_OK;
}

// desc1 [batch][n1][nbytes], desc2 [batch][n2][nbytes] u8 -> idx [batch][n1][2] (train index of the nearest / second nearest under the bit
// distance, ordered by (distance, train index); -1 where n2 < 2 leaves the slot empty), dist [batch][n1][2] i32 (INT32_MAX for an empty slot)
extern "C" int32_t vo_match_hamming_knn2(vo_ctx* c, const uint8_t* desc1, int32_t n1, const uint8_t* desc2, int32_t n2, int32_t nbytes,
                                         int32_t* idx, int32_t* dist) {
  if (!c) return VO_E_INVALID;
  VO_CHECK(c, desc1 && desc2 && idx && dist, VO_E_INVALID, "null buffer");
  VO_CHECK(c, n1 >= 1 && n2 >= 1, VO_E_INVALID, "empty descriptor set");
  VO_CHECK(c, nbytes >= 4 && nbytes <= 4 * HAM_MAX_WORDS && nbytes % 4 == 0, VO_E_INVALID, "nbytes must be a multiple of 4 in 4..64");
  VO_HIP(c, hipSetDevice(c->device));
  const size_t B = c->batch;
  const int nw = nbytes / 4;
  const size_t na = (size_t)n1 * nw, nb = (size_t)n2 * nw;
  if (!c->match) c->match = new vo_match_ws();
  vo_match_ws* w = c->match;
  if (w->hcap1 < na || w->hcap2 < nb || w->hcap_q < n1) {
    VO_HIP(c, hipStreamSynchronize(c->stream));
    void* old[] = {w->d_ha, w->d_hb, w->d_hidx, w->d_hdist};
    for (void* p : old) if (p) (void)hipFree(p);
    w->d_ha = w->d_hb = nullptr; w->d_hidx = w->d_hdist = nullptr;
    w->hcap1 = w->hcap2 = 0; w->hcap_q = 0;
    VO_HIP(c, hipMalloc((void**)&w->d_ha, 4 * na * B));
    VO_HIP(c, hipMalloc((void**)&w->d_hb, 4 * nb * B));
    VO_HIP(c, hipMalloc((void**)&w->d_hidx, sizeof(int32_t) * 2 * (size_t)n1 * B));
    VO_HIP(c, hipMalloc((void**)&w->d_hdist, sizeof(int32_t) * 2 * (size_t)n1 * B));
    w->hcap1 = na; w->hcap2 = nb; w->hcap_q = n1;
  }
  VO_HIP(c, hipMemcpy2DAsync(w->d_ha, 4 * w->hcap1, desc1, 4 * na, 4 * na, B, hipMemcpyHostToDevice, c->stream));
  VO_HIP(c, hipMemcpy2DAsync(w->d_hb, 4 * w->hcap2, desc2, 4 * nb, 4 * nb, B, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_match_hamming_knn2, dim3(vo_div_up(n1, 4), (unsigned)B), dim3(256), 0, c->stream, w->d_ha, w->d_hb, n1, n2, nw, w->hcap1, w->hcap2,
                     w->d_hidx, w->d_hdist, w->hcap_q);
  VO_HIP(c, hipGetLastError());
  VO_HIP(c, hipMemcpy2DAsync(idx, sizeof(int32_t) * 2 * n1, w->d_hidx, sizeof(int32_t) * 2 * w->hcap_q, sizeof(int32_t) * 2 * n1, B, hipMemcpyDeviceToHost, c->stream));
  VO_HIP(c, hipMemcpy2DAsync(dist, sizeof(int32_t) * 2 * n1, w->d_hdist, sizeof(int32_t) * 2 * w->hcap_q, sizeof(int32_t) * 2 * n1, B, hipMemcpyDeviceToHost, c->stream));
  VO_HIP(c, hipStreamSynchronize(c->stream));
  return VO_OK;
}
