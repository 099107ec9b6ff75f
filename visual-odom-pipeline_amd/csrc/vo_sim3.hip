// Sim(3) / rigid 3D-3D alignment RANSAC: the transform dst ~ s R src + t between two sets of corresponding 3-D points that differ by a rotation,
// a translation and a scale -- two maps of the same landmarks after a re-bootstrap, an estimated trajectory against its ground truth (the
// scale-aligned absolute trajectory error), a loop closure.  The one member of the family of searches that relates 3-D to 3-D.
//
// This is Umeyama 1991 ("Least-squares estimation of transformation parameters between two point patterns") / Horn 1987 inside the RANSAC of
// cv2.estimateAffine3D(src, dst, ransacThreshold = 3.0, confidence = 0.99) (later OpenCV: force_rotation = True) and of ORB-SLAM's ComputeSim3.
// The algorithm is defined by tests/sim3_model.py and compared with it hypothesis by hypothesis:
//   sample     hypothesis h draws sample3(seed, h, n) = vo_ransac_sample<3>: three distinct indices.  A sample with a coordinate that is not
//              finite, or whose three points are collinear or coincident in either set (|(b - a) x (c - a)|^2 <= 1e-10 |b - a|^2 |c - a|^2), has
//              no model and still counts
//   solve      one lane per sample, float64: centroids, Sigma = 1/3 sum (y_i - yc)(x_i - xc)^T, its singular values and vectors by one-sided
//              Jacobi rotations on the columns in registers (vo_svd3.h); R = u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T, which is U diag(1, 1, det U det V) V^T
//              (a three-point Sigma has rank 2: the determinant rule decides every sample, and R is a proper rotation also where dst mirrors
//              src); s = (s1 + s2 + d3) / var_x with d3 = (u1 x u2)^T Sigma (v1 x v2) the signed third singular value, or s = 1 (with_scale = 0);
//              t = yc - s R xc.  With scale, s <= 0 or not finite has no model
//   score      one wave per hypothesis: |y - (s R x + t)|^2 <= threshold^2, in dst's units; the 13 model scalars stay in registers
//   select     most inliers, ties to the smallest h; at least 3; iteration bound RANSACUpdateNumIters with 3 model points
//   finish     one workgroup per sequence: mask of the winner (not recomputed afterwards); refit = 1: Umeyama over the consensus set in two
//              passes (centroids, then the central moments about them; 256 threads in a fixed order), unless the set is degenerate (the second
//              eigenvalue of either set's 3 x 3 scatter matrix <= 1e-10 of the first: the squared singular values of the centred set) or the
//              re-fit is not finite -- then, and with refit = 0, the winner's model is returned; cost = sum of squared errors over the mask
//              at the returned model
// Measured (tests/sim3_model.py, tests/test_sim3_model.py): the float64 model lies within 3.00 x 2^-52 x kappa (a sample) and 7.93 x 2^-52 x kappa
// (a set) of a 40-digit truth, kappa = s1 / (s2 + d3); the kernels are held to 4 x that against the model: SOLVE_FACTOR = 13, REFIT_FACTOR = 32.
// vo_sim3_fit is the finish kernel on a given mask without a search: the plain least-squares alignment.  vo_sim3_ransac returns, bit for bit,
// what vo_sim3_fit returns on the mask it reports (when stats.refit = 1).
// Stated deviations from cv2.estimateAffine3D: the sample sequence is this library's (parity is statistical); the model is a similarity
// (7 parameters, or 6 with with_scale = 0), not a 12-parameter affine map; the error is evaluated in float64.
// The points are rows of three floats, 12 bytes and not 16-byte aligned: a lane reads its row with one 12-byte load (global_load_dwordx3, which
// asks only for dword alignment); consecutive lanes read consecutive rows, so a wave's load covers 768 contiguous bytes.  No padded copy is made.
// Rounds of 256 hypotheses, a control block per sequence, [batch] everywhere: vo_ransac.h; workspace, upload, read-back and the 256-thread
// reduction: vo_twoview.h (with three coordinates per point).
#include "vo_internal.h"
#include "vo_twoview.h"
#include "vo_svd3.h"

#include <math.h>
#include <string.h>

#define S3_BATCH 256
#define S3_NM 13                       // a model: s, R (9, row-major), t (3)
#define S3_OUT 32                      // doubles per sequence: model (13), model0 (13), cost, n_inliers, refit, status, 2 spare
#define S3_DEGENERATE 1e-10            // squared sine of a sample's triangle / eigenvalue ratio of a set's scatter matrix at or under this: no model

struct s3_pt { float x, y, z; };
static_assert(sizeof(s3_pt) == 12 && alignof(s3_pt) == 4, "s3_pt layout");

struct s3_hyp { double m[S3_NM]; int count, h, ok, pad; };
struct s3_ctrl { vo_ransac_state s; int best_h, best_count, degenerate; double m[S3_NM]; };
static_assert(sizeof(s3_ctrl) == 128 && offsetof(s3_ctrl, best_h) == 12 && offsetof(s3_ctrl, m) == 24, "s3_ctrl layout");

struct vo_sim3_ws : vo_tv_search_ws<s3_hyp, s3_ctrl, S3_BATCH> {
  static constexpr int dim = 3;
};

// sequence b's two point sets in p [B][2][cap][3]
struct s3_views { const s3_pt *pa, *pb; };
__device__ __forceinline__ s3_views s3_seq_views(const float* p, int cap, int b) {
  const float* pa = p + ((size_t)b * 2) * cap * 3;
  return {(const s3_pt*)pa, (const s3_pt*)(pa + (size_t)cap * 3)};
}

__device__ __forceinline__ bool s3_finite(double x) { return fabs(x) < __builtin_inf(); }

__device__ __forceinline__ void s3_cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

// squared error of a pair under the model m: |y - (s R x + t)|^2
__device__ __forceinline__ double s3_err(const double* m, double x0, double x1, double x2, double y0, double y1, double y2) {
  const double d0 = y0 - (m[0] * ((m[1] * x0 + m[2] * x1) + m[3] * x2) + m[10]);
  const double d1 = y1 - (m[0] * ((m[4] * x0 + m[5] * x1) + m[6] * x2) + m[11]);
  const double d2 = y2 - (m[0] * ((m[7] * x0 + m[8] * x1) + m[9] * x2) + m[12]);
  return (d0 * d0 + d1 * d1) + d2 * d2;
}

// ------------------------------------------------------------------------------------------------
// Umeyama's closed form
// ------------------------------------------------------------------------------------------------
// Sg (3 x 3 row-major) = 1/m sum (y - cy)(x - cx)^T, varx = 1/m sum |x - cx|^2 -> the model (s, R, t); false if an entry is not finite or,
// with scale, s <= 0.  One-sided Jacobi on the columns of Sg (vo_jacobi3_cols of vo_svd3.h, which vo_hpose.hip runs too: the condition of Sg is
// never squared, and no array is indexed by a run-time value)
__device__ inline bool s3_umeyama(const double* Sg, double varx, const double* cx, const double* cy, int with_scale, double* m) {
  double A[3][3], V[3][3], nn[3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) A[i][j] = Sg[3 * i + j];
  vo_jacobi3_cols(A, V, nn);
  const double s1 = sqrt(nn[0]), s2 = sqrt(nn[1]);
  double u1[3], u2[3], u3[3], v1[3], v2[3], v3[3], sv[3];
#pragma unroll
  for (int k = 0; k < 3; k++) { u1[k] = A[k][0] / s1; u2[k] = A[k][1] / s2; v1[k] = V[k][0]; v2[k] = V[k][1]; }
  s3_cross(u1, u2, u3);
  s3_cross(v1, v2, v3);
#pragma unroll
  for (int i = 0; i < 3; i++) sv[i] = (Sg[3 * i] * v3[0] + Sg[3 * i + 1] * v3[1]) + Sg[3 * i + 2] * v3[2];
  const double d3 = (u3[0] * sv[0] + u3[1] * sv[1]) + u3[2] * sv[2];
  const double s = with_scale ? ((s1 + s2) + d3) / varx : 1.0;
  m[0] = s;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) m[1 + 3 * i + j] = (u1[i] * v1[j] + u2[i] * v2[j]) + u3[i] * v3[j];
#pragma unroll
  for (int i = 0; i < 3; i++) m[10 + i] = cy[i] - s * ((m[1 + 3 * i] * cx[0] + m[2 + 3 * i] * cx[1]) + m[3 + 3 * i] * cx[2]);
  bool ok = s > 0.0;
#pragma unroll
  for (int k = 0; k < S3_NM; k++) ok = ok && s3_finite(m[k]);
  return ok;
}

// is the triangle (a, b, c) collinear or coincident (or not finite)
__device__ __forceinline__ bool s3_collinear(const double (&a)[3], const double (&b)[3], const double (&c)[3]) {
  const double u[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, v[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  double w[3];
  s3_cross(u, v, w);
  const double ww = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], uu = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2], vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
  return !(ww > S3_DEGENERATE * (uu * vv));
}

// the three-point solve -> has a model
__device__ inline bool s3_solve3(const double (&x)[3][3], const double (&y)[3][3], int with_scale, double* m) {
  bool fin = true;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) fin = fin && s3_finite(x[i][k]) && s3_finite(y[i][k]);
  if (!fin || s3_collinear(x[0], x[1], x[2]) || s3_collinear(y[0], y[1], y[2])) return false;
  double cx[3], cy[3], xc[3][3], yc[3][3], Sg[9], varx = 0.0;
#pragma unroll
  for (int k = 0; k < 3; k++) { cx[k] = ((x[0][k] + x[1][k]) + x[2][k]) / 3.0; cy[k] = ((y[0][k] + y[1][k]) + y[2][k]) / 3.0; }
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int k = 0; k < 3; k++) { xc[i][k] = x[i][k] - cx[k]; yc[i][k] = y[i][k] - cy[k]; }
#pragma unroll
  for (int j = 0; j < 3; j++)
#pragma unroll
    for (int k = 0; k < 3; k++) Sg[3 * j + k] = ((yc[0][j] * xc[0][k] + yc[1][j] * xc[1][k]) + yc[2][j] * xc[2][k]) / 3.0;
#pragma unroll
  for (int i = 0; i < 3; i++) varx += (xc[i][0] * xc[i][0] + xc[i][1] * xc[i][1]) + xc[i][2] * xc[i][2];
  varx = varx / 3.0;
  return s3_umeyama(Sg, varx, cx, cy, with_scale, m);
}

// the second largest eigenvalue of the symmetric 3 x 3 (a00 a01 a02 a11 a12 a22) over the largest, by cyclic Jacobi rotations in registers;
// NaN if the largest is not positive
__device__ inline double s3_eig_ratio(double a00, double a01, double a02, double a11, double a12, double a22) {
  double M[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}}, V[3][3];
  vo_jacobi3_sym(M, V);
  const double e0 = M[0][0], e1 = M[1][1], e2 = M[2][2];
  const double hi = fmax(fmax(e0, e1), e2), mid = fmax(fmin(e0, e1), fmin(fmax(e0, e1), e2));
  return hi > 0.0 ? mid / hi : __builtin_nan("");
}

// ------------------------------------------------------------------------------------------------
// kernels of the search
// ------------------------------------------------------------------------------------------------
__global__ void k_s3_init(s3_ctrl* ctrl, int max_iters) {
  s3_ctrl* c = ctrl + blockIdx.x;
  vo_ransac_reset(&c->s, max_iters);
  c->best_h = -1; c->best_count = 2; c->degenerate = 0;
  for (int i = 0; i < S3_NM; i++) c->m[i] = 0;
}

// grid (S3_BATCH / 64, batch), a lane per hypothesis
__global__ void __launch_bounds__(64) k_s3_solve(const float* __restrict__ p, int cap, int n, unsigned seed, int with_scale, s3_hyp* __restrict__ hyps,
                                                 const s3_ctrl* __restrict__ ctrl) {
  const int b = blockIdx.y, slot = blockIdx.x * 64 + threadIdx.x;
  const s3_ctrl* cs = ctrl + b;
  s3_hyp* out = hyps + (size_t)b * S3_BATCH + slot;
  const int h = cs->s.h_done + slot;
  out->h = h; out->ok = 0; out->count = 0; out->pad = 0;
  if (cs->s.done) return;
  const auto [pa, pb] = s3_seq_views(p, cap, b);
  int idx[3];
  vo_ransac_sample<3>(seed, (unsigned)h, n, idx);
  double x[3][3], y[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const s3_pt a = pa[idx[i]], c = pb[idx[i]];
    x[i][0] = (double)a.x; x[i][1] = (double)a.y; x[i][2] = (double)a.z; y[i][0] = (double)c.x; y[i][1] = (double)c.y; y[i][2] = (double)c.z;
  }
  double m[S3_NM];
  const bool ok = s3_solve3(x, y, with_scale, m);
  if (ok) {
#pragma unroll
    for (int k = 0; k < S3_NM; k++) out->m[k] = m[k];
    out->ok = 1;
  }
}

// grid (S3_BATCH / 4, batch), 4 waves: a wave counts the consensus of one hypothesis; the points are read once per wave, a 12-byte row per lane
__global__ void __launch_bounds__(256) k_s3_score(const float* __restrict__ p, int cap, int n, double thr2, s3_hyp* __restrict__ hyps) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  s3_hyp* hp = hyps + (size_t)b * S3_BATCH + blockIdx.x * 4 + (threadIdx.x >> 6);
  if (!hp->ok) return;                                   // count stays 0 (k_s3_solve)
  const auto [pa, pb] = s3_seq_views(p, cap, b);
  const double m0 = hp->m[0], m1 = hp->m[1], m2 = hp->m[2], m3 = hp->m[3], m4 = hp->m[4], m5 = hp->m[5], m6 = hp->m[6], m7 = hp->m[7], m8 = hp->m[8],
               m9 = hp->m[9], m10 = hp->m[10], m11 = hp->m[11], m12 = hp->m[12];
  const double m[S3_NM] = {m0, m1, m2, m3, m4, m5, m6, m7, m8, m9, m10, m11, m12};
  int cnt = 0;
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)    // left alone: two rows at a time and 19 times unrolled, 256 VGPRs
  for (int i = lane; i < n; i += 64) {
    const s3_pt a = pa[i], c = pb[i];
    cnt += (s3_err(m, (double)a.x, (double)a.y, (double)a.z, (double)c.x, (double)c.y, (double)c.z) <= thr2) ? 1 : 0;
  }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0) hp->count = cnt;
}

// grid (batch): running best (most inliers; ties to the smallest h), the samples without a model, and the iteration bound
__global__ void __launch_bounds__(S3_BATCH) k_s3_select(const s3_hyp* __restrict__ hyps, s3_ctrl* __restrict__ ctrl, int n, double conf, int max_iters) {
  __shared__ int s_cnt[S3_BATCH];
  const int b = blockIdx.x, tid = threadIdx.x;
  s3_ctrl* c = ctrl + b;
  if (c->s.done) return;
  const s3_hyp* H = hyps + (size_t)b * S3_BATCH;
  s_cnt[tid] = H[tid].ok ? H[tid].count : -1;
  __syncthreads();
  if (tid == 0) {
    const int bi = vo_ransac_best_slot(s_cnt, S3_BATCH, c->best_count);
    if (bi >= 0) {
      c->best_count = s_cnt[bi]; c->best_h = H[bi].h;
      for (int i = 0; i < S3_NM; i++) c->m[i] = H[bi].m[i];
    }
    int deg = 0;
    for (int i = 0; i < S3_BATCH; i++) deg += (s_cnt[i] < 0) ? 1 : 0;
    c->degenerate += deg;
    vo_ransac_advance(&c->s, S3_BATCH, n, c->best_count, c->best_h >= 0, conf, 3, max_iters);
  }
}

// ------------------------------------------------------------------------------------------------
// finish: mask, Umeyama over the consensus set, cost
// ------------------------------------------------------------------------------------------------
// grid (batch), 256 threads.  ctrl != NULL: the search's finish -- the mask is the winner's.  ctrl == NULL: the fit alone -- the mask is the
// caller's (have_mask) or every row, and in either case only rows whose six coordinates are finite stay in it
__global__ void __launch_bounds__(256) k_s3_finish(const float* __restrict__ p, int cap, int n, double thr2, int with_scale, int refit, int have_mask,
                                                   const s3_ctrl* __restrict__ ctrl, uint8_t* __restrict__ mask_all, double* __restrict__ out_all) {
  __shared__ double s_part[4][VO_NSUM], s_tot[VO_NSUM];
  __shared__ double s_m[S3_NM];
  __shared__ int s_refit;
  const int b = blockIdx.x, tid = threadIdx.x;
  const auto [pa, pb] = s3_seq_views(p, cap, b);
  uint8_t* mask = mask_all + (size_t)b * cap;
  double* out = out_all + S3_OUT * b;
  const bool search = ctrl != nullptr;
  double m0[S3_NM];
  if (search) {
    const s3_ctrl* cs = ctrl + b;
    if (cs->best_h < 0) { vo_tv_no_winner(mask, n, out, S3_OUT, 27); return; }
    for (int k = 0; k < S3_NM; k++) m0[k] = cs->m[k];
  } else {
    for (int k = 0; k < S3_NM; k++) m0[k] = __builtin_nan("");
  }
  // ---- the mask (each thread re-reads in the later passes what it wrote itself), the count and the sums of the coordinates
  double acc[VO_NSUM];
#pragma unroll
  for (int k = 0; k < VO_NSUM; k++) acc[k] = 0.0;
  for (int i = tid; i < n; i += 256) {
    const s3_pt a = pa[i], c = pb[i];
    const double x0 = (double)a.x, x1 = (double)a.y, x2 = (double)a.z, y0 = (double)c.x, y1 = (double)c.y, y2 = (double)c.z;
    bool in;
    if (search) in = s3_err(m0, x0, x1, x2, y0, y1, y2) <= thr2;
    else in = (have_mask ? mask[i] != 0 : true) && s3_finite(x0) && s3_finite(x1) && s3_finite(x2) && s3_finite(y0) && s3_finite(y1) && s3_finite(y2);
    mask[i] = in ? 1 : 0;
    if (in) { acc[0] += 1.0; acc[1] += x0; acc[2] += x1; acc[3] += x2; acc[4] += y0; acc[5] += y1; acc[6] += y2; }
  }
  vo_block_sum(acc, s_part, s_tot);
  const double cnt = s_tot[0];
  const double cx[3] = {s_tot[1] / cnt, s_tot[2] / cnt, s_tot[3] / cnt}, cy[3] = {s_tot[4] / cnt, s_tot[5] / cnt, s_tot[6] / cnt};
  if (tid == 0) {
    for (int k = 0; k < S3_NM; k++) s_m[k] = m0[k];
    s_refit = 0;
  }
  if ((refit || !search) && cnt >= 3.0) {
    // ---- the central moments about the centroids: sum yc xc^T (9), sum xc xc^T (6), sum yc yc^T (6)
#pragma unroll
    for (int k = 0; k < VO_NSUM; k++) acc[k] = 0.0;
    for (int i = tid; i < n; i += 256) {
      if (!mask[i]) continue;
      const s3_pt a = pa[i], c = pb[i];
      const double x[3] = {(double)a.x - cx[0], (double)a.y - cx[1], (double)a.z - cx[2]}, y[3] = {(double)c.x - cy[0], (double)c.y - cy[1], (double)c.z - cy[2]};
#pragma unroll
      for (int j = 0; j < 3; j++)
#pragma unroll
        for (int k = 0; k < 3; k++) acc[3 * j + k] += y[j] * x[k];
      acc[9] += x[0] * x[0]; acc[10] += x[0] * x[1]; acc[11] += x[0] * x[2]; acc[12] += x[1] * x[1]; acc[13] += x[1] * x[2]; acc[14] += x[2] * x[2];
      acc[15] += y[0] * y[0]; acc[16] += y[0] * y[1]; acc[17] += y[0] * y[2]; acc[18] += y[1] * y[1]; acc[19] += y[1] * y[2]; acc[20] += y[2] * y[2];
    }
    vo_block_sum(acc, s_part, s_tot);
    if (tid == 0) {
      const double rx = s3_eig_ratio(s_tot[9], s_tot[10], s_tot[11], s_tot[12], s_tot[13], s_tot[14]);
      const double ry = s3_eig_ratio(s_tot[15], s_tot[16], s_tot[17], s_tot[18], s_tot[19], s_tot[20]);
      if (rx > S3_DEGENERATE && ry > S3_DEGENERATE) {
        double Sg[9], mf[S3_NM];
        for (int k = 0; k < 9; k++) Sg[k] = s_tot[k] / cnt;
        const double varx = ((s_tot[9] + s_tot[12]) + s_tot[14]) / cnt;
        if (s3_umeyama(Sg, varx, cx, cy, with_scale, mf)) {
          for (int k = 0; k < S3_NM; k++) s_m[k] = mf[k];
          s_refit = 1;
        }
      }
    }
  }
  __syncthreads();
  // ---- cost: the sum of squared errors over the mask at the returned model
  double m[S3_NM];
  for (int k = 0; k < S3_NM; k++) m[k] = s_m[k];
  const int did = s_refit;
#pragma unroll
  for (int k = 0; k < VO_NSUM; k++) acc[k] = 0.0;
  for (int i = tid; i < n; i += 256) {
    if (!mask[i]) continue;
    const s3_pt a = pa[i], c = pb[i];
    acc[0] += s3_err(m, (double)a.x, (double)a.y, (double)a.z, (double)c.x, (double)c.y, (double)c.z);
  }
  vo_block_sum(acc, s_part, s_tot);
  if (tid == 0) {
    const bool none = !search && !did;                     // the fit alone without a fit: no model
    for (int k = 0; k < S3_NM; k++) { out[k] = m[k]; out[S3_NM + k] = m0[k]; }
    out[26] = none ? __builtin_nan("") : s_tot[0]; out[27] = cnt; out[28] = (double)did; out[29] = none ? (double)VO_E_NUMERIC : 0.0;
    for (int k = 30; k < S3_OUT; k++) out[k] = 0.0;
  }
  if (!search && !did) for (int i = tid; i < n; i += 256) mask[i] = 0;
}

// ================================================================================================
// host
// ================================================================================================
void vo_sim3_destroy(vo_ctx* c) { vo_tv_free(c->sim3); }

extern "C" int32_t vo_sim3_default_params(vo_sim3_params* p) {
  if (!p) return VO_E_INVALID;
  p->threshold = 3.0; p->confidence = 0.99; p->max_iters = 1000; p->seed = 0; p->with_scale = 1; p->refit = 1;
  return VO_OK;
}

// the pinned read-back -> the caller's arrays (each may be NULL)
static void sim3_unpack(const vo_ctx* c, double* scale, double* R, double* t, double* model0) {
  for (size_t b = 0; b < (size_t)c->batch; b++) {
    const double* o = c->sim3->h_out + S3_OUT * b;
    if (scale) scale[b] = o[0];
    if (R) memcpy(R + 9 * b, o + 1, sizeof(double) * 9);
    if (t) memcpy(t + 3 * b, o + 10, sizeof(double) * 3);
    if (model0) memcpy(model0 + S3_NM * b, o + S3_NM, sizeof(double) * S3_NM);
  }
}

// src / dst [batch][n][3] f32 with dst ~ s R src + t -> scale [batch], R [batch][9] row-major, t [batch][3] (the winner's, or Umeyama over its
// consensus set), model0 [batch][13] = (s, R, t) of the winning sample, inlier_mask [batch][n] u8 (of model0), stats [batch]
extern "C" int32_t vo_sim3_ransac(vo_ctx* c, const float* src, const float* dst, int32_t n, const vo_sim3_params* prm, double* scale, double* R,
                                  double* t, double* model0, uint8_t* inlier_mask, vo_sim3_stats* stats) {
  if (!c) return VO_E_INVALID;
  vo_sim3_params def;
  if (!prm) { vo_sim3_default_params(&def); prm = &def; }
  VO_CHECK(c, src && dst, VO_E_INVALID, "null buffer");
  VO_CHECK(c, n >= 3, VO_E_INVALID, "at least 3 correspondences");
  VO_CHECK(c, prm->threshold > 0 && prm->threshold < __builtin_inf() && prm->confidence > 0 && prm->confidence < 1 && prm->max_iters >= 1 &&
           prm->with_scale >= 0 && prm->with_scale <= 1 && prm->refit >= 0 && prm->refit <= 1, VO_E_INVALID, "bad parameters");
  VO_HIP(c, hipSetDevice(c->device));
  int32_t r = vo_tv_alloc(c, c->sim3, vo_sim3_destroy, n, S3_OUT);
  if (r != VO_OK) return r;
  vo_sim3_ws* w = c->sim3;
  hipStream_t q = c->stream;
  const size_t B = c->batch;
  const int cap = w->cap;
  const double thr2 = prm->threshold * prm->threshold;
  r = vo_tv_upload(c, q, w, src, dst, n, 3);
  if (r != VO_OK) return r;
  hipLaunchKernelGGL(k_s3_init, dim3((unsigned)B), dim3(1), 0, q, w->d_ctrl, prm->max_iters);
  r = vo_ransac_rounds(c, q, w->d_ctrl.get(), w->h_ctrl.get(), B, (prm->max_iters + S3_BATCH - 1) / S3_BATCH, [&](int) {
    {
      vo_prof_scope prof(c, q, VO_PROF_SIM3_SOLVE);
      hipLaunchKernelGGL(k_s3_solve, dim3(S3_BATCH / 64, (unsigned)B), dim3(64), 0, q, w->d_p, cap, n, (unsigned)prm->seed, prm->with_scale, w->d_hyp, w->d_ctrl);
    }
    {
      vo_prof_scope prof(c, q, VO_PROF_SIM3_SCORE);
      hipLaunchKernelGGL(k_s3_score, dim3(S3_BATCH / 4, (unsigned)B), dim3(256), 0, q, w->d_p, cap, n, thr2, w->d_hyp);
    }
    {
      vo_prof_scope prof(c, q, VO_PROF_SIM3_SELECT);
      hipLaunchKernelGGL(k_s3_select, dim3((unsigned)B), dim3(S3_BATCH), 0, q, w->d_hyp, w->d_ctrl, n, prm->confidence, prm->max_iters);
    }
  });
  if (r != VO_OK) return r;
  {
    vo_prof_scope prof(c, q, VO_PROF_SIM3_FINISH);
    hipLaunchKernelGGL(k_s3_finish, dim3((unsigned)B), dim3(256), 0, q, w->d_p, cap, n, thr2, prm->with_scale, prm->refit, 0, w->d_ctrl, w->d_mask, w->d_out);
  }
  VO_HIP(c, hipGetLastError());
  r = vo_tv_readback(c, q, w, S3_OUT, inlier_mask, n);
  if (r != VO_OK) return r;
  sim3_unpack(c, scale, R, t, model0);
  if (stats) {
    for (size_t b = 0; b < B; b++) {
      const double* o = w->h_out + S3_OUT * b;
      const s3_ctrl& hc = w->h_ctrl[b];
      const bool none = hc.best_h < 0;
      stats[b].cost = o[26];
      stats[b].n_inliers = none ? 0 : (int32_t)o[27]; stats[b].hypotheses = hc.s.h_done; stats[b].best = hc.best_h;
      stats[b].status = none ? VO_E_NUMERIC : 0; stats[b].degenerate = hc.degenerate; stats[b].refit = none ? 0 : (int32_t)o[28];
    }
  }
  return VO_OK;
}

// the finish pass alone: Umeyama over the rows of mask [batch][n] u8 (NULL: every row) with finite coordinates
extern "C" int32_t vo_sim3_fit(vo_ctx* c, const float* src, const float* dst, const uint8_t* mask, int32_t n, int32_t with_scale, double* scale,
                               double* R, double* t, vo_sim3_stats* stats) {
  if (!c) return VO_E_INVALID;
  VO_CHECK(c, src && dst, VO_E_INVALID, "null buffer");
  VO_CHECK(c, n >= 3, VO_E_INVALID, "at least 3 correspondences");
  VO_CHECK(c, with_scale >= 0 && with_scale <= 1, VO_E_INVALID, "bad parameters");
  VO_HIP(c, hipSetDevice(c->device));
  int32_t r = vo_tv_alloc(c, c->sim3, vo_sim3_destroy, n, S3_OUT);
  if (r != VO_OK) return r;
  vo_sim3_ws* w = c->sim3;
  hipStream_t q = c->stream;
  const size_t B = c->batch;
  r = vo_tv_upload(c, q, w, src, dst, n, 3);
  if (r != VO_OK) return r;
  if (mask) VO_HIP(c, hipMemcpy2DAsync(w->d_mask, w->cap, mask, n, n, B, hipMemcpyHostToDevice, q));
  {
    vo_prof_scope prof(c, q, VO_PROF_SIM3_FINISH);
    hipLaunchKernelGGL(k_s3_finish, dim3((unsigned)B), dim3(256), 0, q, w->d_p, w->cap, n, 0.0, with_scale, 1, mask ? 1 : 0, (const s3_ctrl*)nullptr, w->d_mask,
                       w->d_out);
  }
  VO_HIP(c, hipGetLastError());
  r = vo_tv_readback(c, q, w, S3_OUT, nullptr, n);
  if (r != VO_OK) return r;
  sim3_unpack(c, scale, R, t, nullptr);
  if (stats) {
    for (size_t b = 0; b < B; b++) {
      const double* o = w->h_out + S3_OUT * b;
      const bool none = o[29] != 0.0;
      stats[b].cost = o[26];
      stats[b].n_inliers = none ? 0 : (int32_t)o[27]; stats[b].hypotheses = 0; stats[b].best = -1;
      stats[b].status = none ? VO_E_NUMERIC : 0; stats[b].degenerate = 0; stats[b].refit = none ? 0 : 1;
    }
  }
  return VO_OK;
}
