// What the four two-view units (vo_essential.hip, vo_homography.hip, vo_fundamental.hip, vo_hpose.hip) have in common beyond the sampling
// side of vo_ransac.h, in one place; the 3D-3D unit (vo_sim3.hip) takes the host side and the reduction with points of three coordinates:
//   host    the workspace -- the two views [B][2][cap][dim] f32 (dim = 2), the mask, the result rows and their pinned copy; a search adds its hypotheses
//           and control blocks -- with its allocate-or-regrow and free, the upload of the two views and the read-back of result and mask
//   device  a sequence's pointers into those buffers, the no-winner exit of a finish kernel, and what k_h4_finish and k_f7_finish do alike:
//           the 256-thread reduction of VO_NSUM sums, the winner's mask with count and centroids, the Hartley scales, the Gram matrix of the
//           normalised inliers' rows, its unpacking, the 9 x 9 eigenvector, and the right factor of the two denormalisations
// Samplers, minimal solvers, left factors and sign rules are each model's own and stay in its unit.
#pragma once
#include "vo_buf.h"
#include "vo_ransac.h"

// ================================================================================================
// host
// ================================================================================================
struct vo_tv_ws {
  static constexpr bool search = false;
  static constexpr int dim = 2;        // coordinates per point; a workspace of 3-D point sets (vo_sim3.hip) says 3
  int cap = 0;
  vo_dev<float> d_p;           // [B][2][cap][dim] pixel coordinates of the two views
  vo_dev<uint8_t> d_mask;      // [B][cap]
  vo_dev<double> d_out;        // [B][n_out]
  vo_pinned<double> h_out;
};

template <class Hyp, class Ctrl, int Batch>
struct vo_tv_search_ws : vo_tv_ws {
  static constexpr bool search = true;
  static constexpr int batch = Batch;
  vo_dev<Hyp> d_hyp;           // [B][Batch]
  vo_dev<Ctrl> d_ctrl;         // [B]
  vo_pinned<Ctrl> h_ctrl;
};

// a unit's destroy hook: the workspace goes with every buffer it owns
template <class W>
inline void vo_tv_free(W*& slot) {
  delete slot;
  slot = nullptr;
}

// *slot for n correspondences: a workspace of cap < n goes (by the unit's destroy), a new one has cap = max(n, max_pts, min_cap) and
// n_out (+ h_extra in the pinned copy) doubles per sequence.  `extra` allocates the unit's own buffers behind the shared ones.  The
// workspace is attached once all of it is built (vo_ws_replace): a failed allocation leaves the slot null and the next call builds afresh
inline int32_t vo_tv_no_extra(vo_tv_ws&) { return VO_OK; }
template <class W, class Extra = int32_t (*)(vo_tv_ws&)>
inline int32_t vo_tv_alloc(vo_ctx* c, W*& slot, void (*destroy)(vo_ctx*), int n, int n_out, int h_extra = 0, int min_cap = 0,
                           Extra extra = vo_tv_no_extra) {
  const size_t B = c->batch;
  if (slot && slot->cap < n) destroy(c);
  if (slot) return VO_OK;
  return vo_ws_replace(slot, [&](W& w) -> int32_t {
    w.cap = n > c->max_pts ? n : c->max_pts;
    if (w.cap < min_cap) w.cap = min_cap;
    VO_HIP(c, w.d_p.reserve(2 * W::dim * B * w.cap));
    if constexpr (W::search) {
      VO_HIP(c, w.d_hyp.reserve(B * W::batch));
      VO_HIP(c, w.d_ctrl.reserve(B));
    }
    VO_HIP(c, w.d_mask.reserve(B * w.cap));
    VO_HIP(c, w.d_out.reserve(n_out * B));
    if constexpr (W::search) VO_HIP(c, w.h_ctrl.reserve(B));
    VO_HIP(c, w.h_out.reserve((n_out + h_extra) * B));
    return extra(w);
  });
}

// pts1 / pts2 [B][n][dim] f32 of the host -> the two views of every sequence, on q
inline int32_t vo_tv_upload(vo_ctx* c, hipStream_t q, const vo_tv_ws* w, const float* pts1, const float* pts2, int n, int dim = 2) {
  const size_t row = sizeof(float) * dim * n, pitch = sizeof(float) * 2 * dim * (size_t)w->cap;
  VO_HIP(c, hipMemcpy2DAsync(w->d_p, pitch, pts1, row, row, c->batch, hipMemcpyHostToDevice, q));
  VO_HIP(c, hipMemcpy2DAsync(w->d_p + (size_t)w->cap * dim, pitch, pts2, row, row, c->batch, hipMemcpyHostToDevice, q));
  return VO_OK;
}

// the result rows -> h_out, the mask -> inlier_mask [B][n] (if asked for), and the end of everything enqueued on q
inline int32_t vo_tv_readback(vo_ctx* c, hipStream_t q, const vo_tv_ws* w, int n_out, uint8_t* inlier_mask, int n) {
  VO_HIP(c, hipMemcpyAsync(w->h_out, w->d_out, sizeof(double) * n_out * c->batch, hipMemcpyDeviceToHost, q));
  if (inlier_mask) VO_HIP(c, hipMemcpy2DAsync(inlier_mask, n, w->d_mask, w->cap, n, c->batch, hipMemcpyDeviceToHost, q));
  VO_HIP(c, hipStreamSynchronize(q));
  return VO_OK;
}

// ================================================================================================
// device
// ================================================================================================
// Sequence b's two views in p [B][2][cap][2] of scalars S (float: pixels, double: the essential search's normalised coordinates), as
// elements T: S itself or a pair of them (float2)
template <class T> struct vo_tv_views { const T *pa, *pb; };
template <class T, class S>
__device__ __forceinline__ vo_tv_views<T> vo_tv_seq_views(const S* p, int cap, int b) {
  const S* pa = p + ((size_t)b * 2) * cap * 2;
  return {(const T*)pa, (const T*)(pa + (size_t)cap * 2)};
}

// ... with the sequence's mask row and result row of n_out doubles: what a finish kernel works on
template <class T> struct vo_tv_seq { const T *pa, *pb; uint8_t* mask; double* out; };
template <class T, class S>
__device__ __forceinline__ vo_tv_seq<T> vo_tv_seq_rows(const S* p, int cap, int b, uint8_t* mask_all, double* out_all, int n_out) {
  const vo_tv_views<T> v = vo_tv_seq_views<T>(p, cap, b);
  return {v.pa, v.pb, mask_all + (size_t)b * cap, out_all + n_out * b};
}

// a finish kernel's exit for a sequence without a winner: an empty mask, the first n_nan of the n_out results NaN, the rest 0
__device__ __forceinline__ void vo_tv_no_winner(uint8_t* mask, int n, double* out, int n_out, int n_nan) {
  const int tid = threadIdx.x;
  for (int i = tid; i < n; i += 256) mask[i] = 0;
  if (tid < n_out) out[tid] = (tid < n_nan) ? __builtin_nan("") : 0.0;
}

// a 256-thread reduction of VO_NSUM running sums (the 45 distinct entries of a 9 x 9 normal matrix)
#define VO_NSUM 45

// sum of every acc[k] over the 256 threads -> s_tot[k], the same order every time (wave shuffles, then the four waves in order)
__device__ inline void vo_block_sum(double (&acc)[VO_NSUM], double (*s_part)[VO_NSUM], double* s_tot) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  __syncthreads();                                       // the previous totals have been read
#pragma unroll
  for (int k = 0; k < VO_NSUM; k++) {
    double v = acc[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) s_part[wave][k] = v;
  }
  __syncthreads();
  if (tid < VO_NSUM) s_tot[tid] = (s_part[0][tid] + s_part[1][tid]) + (s_part[2][tid] + s_part[3][tid]);
  __syncthreads();
}

// The passes of a finish kernel over the n points of its sequence, 256 threads; acc, s_part and s_tot are the kernel's reduction buffers.
// The winner's mask (each thread re-reads in the later passes what it wrote itself) -> the inliers' count m and the centroids of the two
// views; inlier(x, y, u, v) is the model's consensus test
struct vo_tv_centroids { double m, c1x, c1y, c2x, c2y; };
template <class In>
__device__ __forceinline__ vo_tv_centroids vo_tv_mask_pass(const float2* pa, const float2* pb, uint8_t* mask, int n, In inlier,
                                                           double (&acc)[VO_NSUM], double (*s_part)[VO_NSUM], double* s_tot) {
#pragma unroll
  for (int k = 0; k < VO_NSUM; k++) acc[k] = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float2 a = pa[i], c = pb[i];
    const bool in = inlier((double)a.x, (double)a.y, (double)c.x, (double)c.y);
    mask[i] = in ? 1 : 0;
    if (in) { acc[0] += 1.0; acc[1] += (double)a.x; acc[2] += (double)a.y; acc[3] += (double)c.x; acc[4] += (double)c.y; }
  }
  vo_block_sum(acc, s_part, s_tot);
  const double m = s_tot[0];
  return {m, s_tot[1] / m, s_tot[2] / m, s_tot[3] / m, s_tot[4] / m};
}

// Hartley scales of the inliers about their centroids: mean distance sqrt 2
struct vo_tv_scales { double s1, s2; };
__device__ __forceinline__ vo_tv_scales vo_tv_scale_pass(const float2* pa, const float2* pb, const uint8_t* mask, int n, const vo_tv_centroids& g,
                                                         double (&acc)[VO_NSUM], double (*s_part)[VO_NSUM], double* s_tot) {
#pragma unroll
  for (int k = 0; k < VO_NSUM; k++) acc[k] = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    if (!mask[i]) continue;
    const float2 a = pa[i], c = pb[i];
    const double dx1 = (double)a.x - g.c1x, dy1 = (double)a.y - g.c1y, dx2 = (double)c.x - g.c2x, dy2 = (double)c.y - g.c2y;
    acc[0] += sqrt(dx1 * dx1 + dy1 * dy1); acc[1] += sqrt(dx2 * dx2 + dy2 * dy2);
  }
  vo_block_sum(acc, s_part, s_tot);
  return {1.4142135623730951 / (s_tot[0] / g.m), 1.4142135623730951 / (s_tot[1] / g.m)};
}

// Gram matrix (its 45 distinct entries -> s_tot) of the one or two rows that rows(x, y, u, v) gives for each normalised inlier
template <int NR> struct vo_tv_rows { double r[NR][9]; };
template <class Rows>
__device__ __forceinline__ void vo_tv_gram_pass(const float2* pa, const float2* pb, const uint8_t* mask, int n, const vo_tv_centroids& g,
                                                double s1, double s2, Rows rows, double (&acc)[VO_NSUM], double (*s_part)[VO_NSUM], double* s_tot) {
#pragma unroll
  for (int k = 0; k < VO_NSUM; k++) acc[k] = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    if (!mask[i]) continue;
    const float2 a = pa[i], c = pb[i];
    const double x = ((double)a.x - g.c1x) * s1, y = ((double)a.y - g.c1y) * s1, u = ((double)c.x - g.c2x) * s2, v = ((double)c.y - g.c2y) * s2;
    const auto q = rows(x, y, u, v);
    constexpr int NR = sizeof(q.r) / sizeof(q.r[0]);
    static_assert(NR == 1 || NR == 2, "one or two rows per point");
    int k = 0;
#pragma unroll
    for (int ia = 0; ia < 9; ia++)
#pragma unroll
      for (int ib = ia; ib < 9; ib++, k++) {
        if constexpr (NR == 2) acc[k] += q.r[0][ia] * q.r[0][ib] + q.r[1][ia] * q.r[1][ib];
        else acc[k] += q.r[0][ia] * q.r[0][ib];
      }
  }
  vo_block_sum(acc, s_part, s_tot);
}

// the 45 sums -> the symmetric 9 x 9
__device__ __forceinline__ void vo_tv_unpack_sym9(const double* s_tot, double (*M)[9]) {
  for (int ia = 0, k = 0; ia < 9; ia++)
    for (int ib = ia; ib < 9; ib++, k++) { M[ia][ib] = s_tot[k]; M[ib][ia] = s_tot[k]; }
}

// eigenvector of the smallest eigenvalue of the symmetric 9 x 9 M (destroyed) by cyclic Jacobi rotations; one thread, arrays in LDS
__device__ inline void vo_smallest_eigenvector9(double (*M)[9], double (*V)[9], double* out) {
  for (int i = 0; i < 9; i++) for (int j = 0; j < 9; j++) V[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; sweep++) {
    bool changed = false;
    for (int p = 0; p < 8; p++)
      for (int q = p + 1; q < 9; q++) {
        const double apq = M[p][q];
        if (!(apq * apq > 4.930380657631324e-32 * fabs(M[p][p] * M[q][q]))) continue;      // |a_pq| <= 2^-52 sqrt(a_pp a_qq): converged
        changed = true;
        const double zeta = (M[q][q] - M[p][p]) / (2.0 * apq);
        const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
        for (int k = 0; k < 9; k++) { const double a = M[k][p], bq = M[k][q]; M[k][p] = c * a - s * bq; M[k][q] = s * a + c * bq; }
        for (int k = 0; k < 9; k++) { const double a = M[p][k], bq = M[q][k]; M[p][k] = c * a - s * bq; M[q][k] = s * a + c * bq; }
        for (int k = 0; k < 9; k++) { const double a = V[k][p], bq = V[k][q]; V[k][p] = c * a - s * bq; V[k][q] = s * a + c * bq; }
      }
    if (!changed) break;
  }
  int j = 0;
  for (int k = 1; k < 9; k++) if (M[k][k] < M[j][j]) j = k;
  for (int k = 0; k < 9; k++) out[k] = V[k][j];
}

// The right factor of a denormalisation: M = Xn T1 with T1 = [[s1 0 -s1 c1x] [0 s1 -s1 c1y] [0 0 1]].  The left factor (T2^-1 for a
// homography, T2^T for a fundamental matrix) and the sign rule are the model's
__device__ __forceinline__ void vo_tv_right_factor(const double* Xn, double c1x, double c1y, double s1, double* M) {
#pragma unroll
  for (int r = 0; r < 3; r++) {
    M[3 * r] = Xn[3 * r] * s1; M[3 * r + 1] = Xn[3 * r + 1] * s1;
    M[3 * r + 2] = Xn[3 * r + 2] - (M[3 * r] * c1x + M[3 * r + 1] * c1y);
  }
}
