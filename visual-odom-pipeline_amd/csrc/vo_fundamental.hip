// Fundamental-matrix RANSAC: the two-view model that needs no intrinsics, for the epipolar verification of matches when K is unknown,
// guessed or not yet trusted (the reference's notebooks/estimateFundamentalMat.py carries the model's name).
//
// This is  F, mask = cv2.findFundamentalMat(p1, p2, cv2.FM_RANSAC, 3.0, 0.99)  of OpenCV 4.4 (modules/calib3d/src/fundam.cpp, ptsetreg.cpp).
// OpenCV's sample draws cannot be reproduced; the algorithm is defined by tests/fundamental_model.py and compared with it hypothesis by
// hypothesis:
//   sample     hypothesis h draws sample7(seed, h, n) = vo_ransac_sample<7>: seven distinct indices.  FMEstimatorCallback has no subset check,
//              so there is none: a degenerate sample yields poor models and still counts
//   solve      one lane per sample, float64: Hartley normalisation of the seven points of each view, the two-dimensional null space of the
//              7 x 9 epipolar system by elimination with complete pivoting in registers, an orthonormal basis of it, the cubic
//              det(P + t Q) = 0 in the chart whose point at infinity Q has the largest determinant of four fixed directions (so the roots do
//              not depend on the basis the elimination happened to give), every real root (1 or 3; a double root that rounding split into a
//              complex pair is kept twice) polished by Newton steps on the cubic, denormalised, unit Frobenius norm, largest entry positive.
//              A system whose null space has more than two dimensions (a repeated point, a sample on a line) has no model and still counts
//   score      one wave per (hypothesis, root): err = max(d1^2 s1, d2^2 s2), the larger squared distance of a point to its epipolar line
//              (OpenCV's FMEstimatorCallback::computeError), err <= threshold^2, and the sum of err over the consensus set
//   select     most inliers, ties to the smallest h, between the models of one sample to the smaller sum of err; at least 7; iteration
//              bound RANSACUpdateNumIters with 7 model points
//   finish     one workgroup per sequence: mask of the winner F0 (not recomputed afterwards); refit = 1 and at least 8 inliers: the normalised
//              eight-point algorithm on the consensus set (smallest eigenvector of the 9 x 9 Gram matrix by Jacobi, the smallest singular
//              value of the 3 x 3 set to zero), denormalised; cost = sum of err over the mask at the returned F
// Stated deviations from cv2: err is evaluated in float64 (OpenCV: float32); for 7 < n < 15 cv2 silently switches to LMedS, this search runs
// RANSAC for every n >= 8; for n = 7 cv2 returns all roots stacked as 9 x 3, this search evaluates the one possible sample and returns the
// winner by the tie rule above; cv2 scales F to f33 = 1, the C ABI returns unit norm (the Python layer divides by f33).
// Rounds of 256 hypotheses, a control block per sequence, [batch] everywhere.  What the searches share on the sampling side is vo_ransac.h;
// what the two-view units share beyond it (workspace, upload and read-back, a sequence's pointers, the mask, Hartley and Gram passes of the
// finish kernel, which the homography's finish kernel runs too) is vo_twoview.h.
#include "vo_internal.h"
#include "vo_twoview.h"
#include "vo_epi_dev.h"
#include "vo_svd3.h"

#include <math.h>
#include <string.h>

#define F7_BATCH 256
#define F7_ROOTS 3
#define F7_OUT 24                      // doubles per sequence: F (9), F0 (9), cost, n_inliers, 4 spare
#define F7_RANK_TOL 1e-12              // last pivot against the first: under it the null space has more than two dimensions
#define F7_IMAG_REAL 1e-8              // a complex pair whose imaginary part is under this (relative to max(1, |re|)) is a double root
#define F7_NEWTON_STEPS 4

struct f7_hyp { double F[F7_ROOTS][9]; double sum[F7_ROOTS]; int count[F7_ROOTS]; int nroots, h, pad; };
struct f7_ctrl { vo_ransac_state s; int best_h, best_count, n_roots, models, pad; double best_sum; double F[9]; };
static_assert(sizeof(f7_ctrl) == 112 && offsetof(f7_ctrl, best_h) == 12 && offsetof(f7_ctrl, best_sum) == 32 && offsetof(f7_ctrl, F) == 40, "f7_ctrl layout");

struct vo_fund_ws : vo_tv_search_ws<f7_hyp, f7_ctrl, F7_BATCH> {};

// ------------------------------------------------------------------------------------------------
// the minimal problem
// ------------------------------------------------------------------------------------------------
// Hartley normalisation of seven points in place: -> centroid and scale, x <- (x - c) s with mean distance sqrt 2
__device__ inline void f7_normalise7(double (&x)[7], double (&y)[7], double& cx, double& cy, double& s) {
  double sx = 0.0, sy = 0.0, d = 0.0;
#pragma unroll
  for (int i = 0; i < 7; i++) { sx += x[i]; sy += y[i]; }
  cx = sx / 7.0; cy = sy / 7.0;
#pragma unroll
  for (int i = 0; i < 7; i++) { x[i] = x[i] - cx; y[i] = y[i] - cy; d += sqrt(x[i] * x[i] + y[i] * y[i]); }
  s = 1.4142135623730951 / (d / 7.0);
#pragma unroll
  for (int i = 0; i < 7; i++) { x[i] = x[i] * s; y[i] = y[i] * s; }
}

// Fn (normalised frame) -> T2^T Fn T1 with T = [[s 0 -s cx] [0 s -s cy] [0 0 1]], scaled to unit Frobenius norm, the entry of the largest
// magnitude positive.  -> false if an entry is not finite or the norm is 0
__device__ inline bool f7_denormalise(const double* Fn, double c1x, double c1y, double s1, double c2x, double c2y, double s2, double* F) {
  double M[9], nn = 0.0, big = 0.0, sgn = 1.0;
  vo_tv_right_factor(Fn, c1x, c1y, s1, M);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    F[k] = M[k] * s2; F[3 + k] = M[3 + k] * s2;
    F[6 + k] = M[6 + k] - (F[k] * c2x + F[3 + k] * c2y);
  }
#pragma unroll
  for (int k = 0; k < 9; k++) {
    nn += F[k] * F[k];
    if (fabs(F[k]) > big) { big = fabs(F[k]); sgn = F[k] < 0 ? -1.0 : 1.0; }
  }
  nn = sqrt(nn);
  if (!(nn > 0) || !(nn < __builtin_inf())) return false;
  const double sc = sgn / nn;
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 9; k++) { F[k] = F[k] * sc; ok = ok && (fabs(F[k]) < __builtin_inf()); }
  return ok;
}

__device__ __forceinline__ double f7_det3(const double* m) {
  return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}

// sum_ij cof(A)_ij B_ij: the coefficient of t in det(A + t B)
__device__ inline double f7_cof_dot(const double* a, const double* b) {
  return ((a[4] * a[8] - a[5] * a[7]) * b[0] - (a[3] * a[8] - a[5] * a[6]) * b[1] + (a[3] * a[7] - a[4] * a[6]) * b[2]) +
         (-(a[1] * a[8] - a[2] * a[7]) * b[3] + (a[0] * a[8] - a[2] * a[6]) * b[4] - (a[0] * a[7] - a[1] * a[6]) * b[5]) +
         ((a[1] * a[5] - a[2] * a[4]) * b[6] - (a[0] * a[5] - a[2] * a[3]) * b[7] + (a[0] * a[4] - a[1] * a[3]) * b[8]);
}

// Orthonormal basis (G1, G2) of the null space of the 7 x 9 system of seven normalised correspondences, rows (u x, u y, u, v x, v y, v, x, y, 1)
// for x2^T F x1 = 0: Gaussian elimination with complete pivoting.  Every loop has constant bounds; the pivot comes up by conditional row
// and column swaps and the column order is undone by selects, so that after unrolling nothing is indexed by a run-time value and the 63
// entries live in registers.  -> false if the last pivot is under F7_RANK_TOL of the first (more than two null dimensions) or not finite
__device__ inline bool f7_null_space(const double (&x)[7], const double (&y)[7], const double (&u)[7], const double (&v)[7], double* G1, double* G2) {
  double A[7][9];
  int perm[9];
#pragma unroll
  for (int i = 0; i < 7; i++) {
    A[i][0] = u[i] * x[i]; A[i][1] = u[i] * y[i]; A[i][2] = u[i]; A[i][3] = v[i] * x[i]; A[i][4] = v[i] * y[i]; A[i][5] = v[i];
    A[i][6] = x[i]; A[i][7] = y[i]; A[i][8] = 1.0;
  }
#pragma unroll
  for (int k = 0; k < 9; k++) perm[k] = k;
  double first = 0.0, last = 0.0;
#pragma unroll
  for (int c = 0; c < 7; c++) {
    double rmax[7];
#pragma unroll
    for (int r = c; r < 7; r++) {
      double m = 0.0;
#pragma unroll
      for (int k = c; k < 9; k++) m = fabs(A[r][k]) > m ? fabs(A[r][k]) : m;
      rmax[r] = m;
    }
#pragma unroll
    for (int r = c + 1; r < 7; r++) {                    // the row that holds the largest entry comes up ...
      const bool sw = rmax[r] > rmax[c];
      const double ma = rmax[c], mb = rmax[r];
      rmax[c] = sw ? mb : ma; rmax[r] = sw ? ma : mb;
#pragma unroll
      for (int k = c; k < 9; k++) {
        const double a = A[c][k], b = A[r][k];
        A[c][k] = sw ? b : a; A[r][k] = sw ? a : b;
      }
    }
#pragma unroll
    for (int k = c + 1; k < 9; k++) {                    // ... and its column comes forward
      const bool sw = fabs(A[c][k]) > fabs(A[c][c]);
      const int pa = perm[c], pb = perm[k];
      perm[c] = sw ? pb : pa; perm[k] = sw ? pa : pb;
#pragma unroll
      for (int r = 0; r < 7; r++) {
        const double a = A[r][c], b = A[r][k];
        A[r][c] = sw ? b : a; A[r][k] = sw ? a : b;
      }
    }
    if (c == 0) first = fabs(A[0][0]);
    if (c == 6) last = fabs(A[6][6]);
    const double inv = 1.0 / A[c][c];                    // a zero pivot makes every later entry non-finite: no model
#pragma unroll
    for (int r = c + 1; r < 7; r++) {
      const double f = A[r][c] * inv;
#pragma unroll
      for (int k = c + 1; k < 9; k++) A[r][k] = A[r][k] - f * A[c][k];
    }
  }
  if (!(last > F7_RANK_TOL * first) || !(first < __builtin_inf())) return false;
  // two null vectors in the permuted order: free entries (1, 0) and (0, 1)
  double v1[9], v2[9];
  v1[7] = 1.0; v1[8] = 0.0; v2[7] = 0.0; v2[8] = 1.0;
#pragma unroll
  for (int c = 6; c >= 0; c--) {
    double a = A[c][7], b = A[c][8];
#pragma unroll
    for (int k = c + 1; k < 7; k++) { a = a + A[c][k] * v1[k]; b = b + A[c][k] * v2[k]; }
    v1[c] = -a / A[c][c]; v2[c] = -b / A[c][c];
  }
#pragma unroll
  for (int k = 0; k < 9; k++) { G1[k] = 0.0; G2[k] = 0.0; }
#pragma unroll
  for (int j = 0; j < 9; j++)
#pragma unroll
    for (int k = 0; k < 9; k++) { G1[k] = (perm[j] == k) ? v1[j] : G1[k]; G2[k] = (perm[j] == k) ? v2[j] : G2[k]; }
  // Gram-Schmidt
  double n1 = 0.0, d12 = 0.0, n2 = 0.0;
#pragma unroll
  for (int k = 0; k < 9; k++) n1 += G1[k] * G1[k];
  n1 = 1.0 / sqrt(n1);
#pragma unroll
  for (int k = 0; k < 9; k++) { G1[k] = G1[k] * n1; d12 += G1[k] * G2[k]; }
#pragma unroll
  for (int k = 0; k < 9; k++) { G2[k] = G2[k] - d12 * G1[k]; n2 += G2[k] * G2[k]; }
  n2 = 1.0 / sqrt(n2);
#pragma unroll
  for (int k = 0; k < 9; k++) G2[k] = G2[k] * n2;
  return (n1 < __builtin_inf()) && (n2 < __builtin_inf());
}

// real roots of c0 + c1 t + c2 t^2 + c3 t^3 (c3 != 0), each polished by Newton steps on the cubic -> their number (1 or 3)
__device__ inline int f7_cubic_roots(double c0, double c1, double c2, double c3, double* t) {
  const double b = c2 / c3, c = c1 / c3, d = c0 / c3;
  const double p = c - b * b / 3.0, q = (2.0 * b * b * b / 27.0 - b * c / 3.0) + d;
  const double disc = q * q / 4.0 + p * p * p / 27.0;
  int nr;
  if (disc > 0) {
    const double sq = sqrt(disc);
    const double w = cbrt(q < 0 ? -q / 2.0 + sq : -q / 2.0 - sq);      // the larger of the two cube roots; the other is -p / (3 w)
    const double z = (w != 0.0) ? -p / (3.0 * w) : 0.0;
    t[0] = (w + z) - b / 3.0;
    const double re = -(w + z) / 2.0 - b / 3.0, im = 0.8660254037844386 * fabs(w - z);
    nr = 1;
    if (im <= F7_IMAG_REAL * fmax(1.0, fabs(re))) { t[1] = re; t[2] = re; nr = 3; }
  } else if (p < 0) {
    const double r = 2.0 * sqrt(-p / 3.0);
    const double arg = fmin(fmax((3.0 * q) / (p * r), -1.0), 1.0);
    const double phi = acos(arg) / 3.0;
    t[0] = r * cos(phi) - b / 3.0;
    t[1] = r * cos(phi - 2.0943951023931953) - b / 3.0;
    t[2] = r * cos(phi - 4.1887902047863905) - b / 3.0;
    nr = 3;
  } else {                                               // p = q = 0: a triple root
    t[0] = -b / 3.0; t[1] = t[0]; t[2] = t[0];
    nr = 3;
  }
#pragma unroll
  for (int k = 0; k < F7_ROOTS; k++) {
    if (k < nr) {
      double x = t[k];
      for (int it = 0; it < F7_NEWTON_STEPS; it++) {
        const double f = ((c3 * x + c2) * x + c1) * x + c0, g = (3.0 * c3 * x + 2.0 * c2) * x + c1;
        const double xn = x - f / g;
        if ((g != 0.0) && (fabs(xn) < __builtin_inf())) x = xn;
      }
      t[k] = x;
    }
  }
  return nr;
}

// the seven-point solve -> number of models (0, 1 or 3) in F[.][9]
__device__ inline int f7_solve(double (&x1)[7], double (&y1)[7], double (&x2)[7], double (&y2)[7], double (*F)[9]) {
  double c1x, c1y, s1, c2x, c2y, s2, G1[9], G2[9];
  f7_normalise7(x1, y1, c1x, c1y, s1);
  f7_normalise7(x2, y2, c2x, c2y, s2);
  if (!f7_null_space(x1, y1, x2, y2, G1, G2)) return 0;
  // the chart: of the directions G1, G2, (G1 + G2) / sqrt 2, (G1 - G2) / sqrt 2 the one with the largest |det| is the point at infinity Q
  // (a binary cubic cannot be small at four directions unless it is small everywhere), P is the direction orthogonal to it
  const double rh = 0.7071067811865476;
  double P[9], Q[9], S[9], D[9];
#pragma unroll
  for (int k = 0; k < 9; k++) { S[k] = rh * (G1[k] + G2[k]); D[k] = rh * (G1[k] - G2[k]); }
  const double d1 = fabs(f7_det3(G1)), d2 = fabs(f7_det3(G2)), d3 = fabs(f7_det3(S)), d4 = fabs(f7_det3(D));
  const double dm = fmax(fmax(d1, d2), fmax(d3, d4));
  const int pick = (d1 == dm) ? 0 : (d2 == dm) ? 1 : (d3 == dm) ? 2 : 3;
#pragma unroll
  for (int k = 0; k < 9; k++) {
    Q[k] = pick == 0 ? G1[k] : pick == 1 ? G2[k] : pick == 2 ? S[k] : D[k];
    P[k] = pick == 0 ? G2[k] : pick == 1 ? -G1[k] : pick == 2 ? D[k] : -S[k];
  }
  const double c0 = f7_det3(P), c1 = f7_cof_dot(P, Q), c2 = f7_cof_dot(Q, P), c3 = f7_det3(Q);
  if (!(fabs(c3) > 0) || !(fabs(c3) < __builtin_inf()) || !(fabs(c0) < __builtin_inf()) || !(fabs(c1) < __builtin_inf()) || !(fabs(c2) < __builtin_inf())) return 0;
  double t[F7_ROOTS];
  const int nr = f7_cubic_roots(c0, c1, c2, c3, t);
  bool ok = true;
#pragma unroll
  for (int k = 0; k < F7_ROOTS; k++) {
    if (k < nr) {
      double Fn[9];
#pragma unroll
      for (int i = 0; i < 9; i++) Fn[i] = P[i] + t[k] * Q[i];
      ok = f7_denormalise(Fn, c1x, c1y, s1, c2x, c2y, s2, F[k]) && ok;
    }
  }
  return ok ? nr : 0;
}

// the consensus test f7_inlier (OpenCV's FMEstimatorCallback::computeError in float64) lives in vo_epi_dev.h: the guided matcher's epipolar
// gate is the same function

// ------------------------------------------------------------------------------------------------
// kernels of the search
// ------------------------------------------------------------------------------------------------
__global__ void k_f7_init(f7_ctrl* ctrl, int max_iters) {
  f7_ctrl* c = ctrl + blockIdx.x;
  vo_ransac_reset(&c->s, max_iters);
  c->best_h = -1; c->best_count = 6; c->n_roots = 0; c->models = 0; c->pad = 0; c->best_sum = 0.0;
  for (int i = 0; i < 9; i++) c->F[i] = 0;
}

// grid (F7_BATCH / 64, batch), a lane per hypothesis
__global__ void __launch_bounds__(64) k_f7_solve(const float* __restrict__ p, int cap, int n, unsigned seed, f7_hyp* __restrict__ hyps,
                                                 const f7_ctrl* __restrict__ ctrl) {
  const int b = blockIdx.y, slot = blockIdx.x * 64 + threadIdx.x;
  const f7_ctrl* cs = ctrl + b;
  f7_hyp* out = hyps + (size_t)b * F7_BATCH + slot;
  const int h = cs->s.h_done + slot;
  out->h = h; out->nroots = 0; out->pad = 0;
#pragma unroll
  for (int k = 0; k < F7_ROOTS; k++) { out->count[k] = 0; out->sum[k] = 0.0; }
  if (cs->s.done) return;
  const auto [pa, pb] = vo_tv_seq_views<float>(p, cap, b);
  int idx[7];
  vo_ransac_sample<7>(seed, (unsigned)h, n, idx);
  double x1[7], y1[7], x2[7], y2[7];
#pragma unroll
  for (int i = 0; i < 7; i++) {
    const int j = idx[i];
    x1[i] = (double)pa[2 * j]; y1[i] = (double)pa[2 * j + 1]; x2[i] = (double)pb[2 * j]; y2[i] = (double)pb[2 * j + 1];
  }
  double F[F7_ROOTS][9];
  const int nr = f7_solve(x1, y1, x2, y2, F);
#pragma unroll
  for (int k = 0; k < F7_ROOTS; k++)
    if (k < nr)
#pragma unroll
      for (int i = 0; i < 9; i++) out->F[k][i] = F[k][i];
  out->nroots = nr;
}

// grid (F7_BATCH * F7_ROOTS / 4, batch), 4 waves: a wave counts the consensus of one model (hypothesis, root); the points are read once per wave
__global__ void __launch_bounds__(256) k_f7_score(const float* __restrict__ p, int cap, int n, double thr2, f7_hyp* __restrict__ hyps) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int model = blockIdx.x * 4 + (threadIdx.x >> 6), slot = model / F7_ROOTS, root = model - slot * F7_ROOTS;
  f7_hyp* hp = hyps + (size_t)b * F7_BATCH + slot;
  if (root >= hp->nroots) return;                        // count and sum stay 0 (k_f7_solve)
  const auto [pa, pb] = vo_tv_seq_views<float2>(p, cap, b);
  const double* Fp = hp->F[root];
  const double F0 = Fp[0], F1 = Fp[1], F2 = Fp[2], F3 = Fp[3], F4 = Fp[4], F5 = Fp[5], F6 = Fp[6], F7 = Fp[7], F8 = Fp[8];
  const double F[9] = {F0, F1, F2, F3, F4, F5, F6, F7, F8};
  int cnt = 0;
  double sum = 0.0;
  for (int i = lane; i < n; i += 64) {
    const float2 a = pa[i], c = pb[i];
    double err;
    const bool in = f7_inlier(F, (double)a.x, (double)a.y, (double)c.x, (double)c.y, thr2, err);
    cnt += in ? 1 : 0;
    sum += in ? err : 0.0;
  }
  for (int o = 32; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o); sum += __shfl_xor(sum, o); }
  if (lane == 0) { hp->count[root] = cnt; hp->sum[root] = sum; }
}

// grid (batch): the better model of each sample (more inliers, then the smaller sum of err), the running best (most inliers; ties to the
// smallest h) and the iteration bound
__global__ void __launch_bounds__(F7_BATCH) k_f7_select(const f7_hyp* __restrict__ hyps, f7_ctrl* __restrict__ ctrl, int n, double conf, int max_iters) {
  __shared__ int s_cnt[F7_BATCH], s_root[F7_BATCH], s_models;
  const int b = blockIdx.x, tid = threadIdx.x;
  f7_ctrl* c = ctrl + b;
  if (c->s.done) return;
  const f7_hyp* H = hyps + (size_t)b * F7_BATCH;
  if (tid == 0) s_models = 0;
  __syncthreads();
  const int nr = H[tid].nroots;
  int bc = -1, br = 0;
  double bs = 0.0;
#pragma unroll
  for (int k = 0; k < F7_ROOTS; k++) {
    if (k < nr) {
      const int cnt = H[tid].count[k];
      const double sum = H[tid].sum[k];
      if (cnt > bc || (cnt == bc && sum < bs)) { bc = cnt; bs = sum; br = k; }
    }
  }
  s_cnt[tid] = bc; s_root[tid] = br;
  if (nr > 0) atomicAdd(&s_models, nr);
  __syncthreads();
  if (tid == 0) {
    const int bi = vo_ransac_best_slot(s_cnt, F7_BATCH, c->best_count);
    if (bi >= 0) {
      const int r = s_root[bi];
      c->best_count = s_cnt[bi]; c->best_h = H[bi].h; c->n_roots = H[bi].nroots; c->best_sum = H[bi].sum[r];
      for (int i = 0; i < 9; i++) c->F[i] = H[bi].F[r][i];
    }
    c->models += s_models;
    vo_ransac_advance(&c->s, F7_BATCH, n, c->best_count, c->best_h >= 0, conf, 7, max_iters);
  }
}

// ------------------------------------------------------------------------------------------------
// finish: mask, eight-point re-fit
// ------------------------------------------------------------------------------------------------
// unit eigenvector of the smallest eigenvalue of the symmetric 3 x 3 (a00 a01 a02 a11 a12 a22) by cyclic Jacobi rotations, in registers
__device__ inline void f7_smallest_eigenvector3(double a00, double a01, double a02, double a11, double a12, double a22, double* out) {
  double M[3][3] = {{a00, a01, a02}, {a01, a11, a12}, {a02, a12, a22}}, V[3][3];
  vo_jacobi3_sym(M, V);
  const bool m1 = M[1][1] < M[0][0];
  const double e01 = m1 ? M[1][1] : M[0][0];
  const bool m2 = M[2][2] < e01;
#pragma unroll
  for (int k = 0; k < 3; k++) out[k] = m2 ? V[k][2] : (m1 ? V[k][1] : V[k][0]);
}

// grid (batch), 256 threads
__global__ void __launch_bounds__(256) k_f7_finish(const float* __restrict__ p, int cap, int n, double thr2, int refit, const f7_ctrl* __restrict__ ctrl,
                                                   uint8_t* __restrict__ mask_all, double* __restrict__ out_all) {
  __shared__ double s_part[4][VO_NSUM], s_tot[VO_NSUM];
  __shared__ double s_M[9][9], s_V[9][9];
  __shared__ double s_F[9];
  const int b = blockIdx.x, tid = threadIdx.x;
  const auto [pa, pb, mask, out] = vo_tv_seq_rows<float2>(p, cap, b, mask_all, out_all, F7_OUT);
  const f7_ctrl* cs = ctrl + b;
  if (cs->best_h < 0) { vo_tv_no_winner(mask, n, out, F7_OUT, 19); return; }
  double F0[9];
  for (int k = 0; k < 9; k++) F0[k] = cs->F[k];
  double acc[VO_NSUM];
  // ---- the winner's mask, the inliers' count and centroids
  const vo_tv_centroids g = vo_tv_mask_pass(pa, pb, mask, n, [&](double x, double y, double u, double v) { double err; return f7_inlier(F0, x, y, u, v, thr2, err); },
                                            acc, s_part, s_tot);
  const double m = g.m, c1x = g.c1x, c1y = g.c1y, c2x = g.c2x, c2y = g.c2y;
  if (tid == 0) for (int k = 0; k < 9; k++) s_F[k] = F0[k];
  if (refit && m >= 8.0) {
    // ---- Hartley scales of the inliers, then the Gram matrix of the epipolar rows (u x, u y, u, v x, v y, v, x, y, 1)
    const auto [s1, s2] = vo_tv_scale_pass(pa, pb, mask, n, g, acc, s_part, s_tot);
    vo_tv_gram_pass(pa, pb, mask, n, g, s1, s2, [](double x, double y, double u, double v) {
      return vo_tv_rows<1>{{{u * x, u * y, u, v * x, v * y, v, x, y, 1.0}}};
    }, acc, s_part, s_tot);
    if (tid == 0) {
      vo_tv_unpack_sym9(s_tot, s_M);
      double fn[9], Fd[9], w[3];
      vo_smallest_eigenvector9(s_M, s_V, fn);
      // rank 2: the right singular vector w of the smallest singular value is the smallest eigenvector of Fn^T Fn; Fn <- Fn - (Fn w) w^T
      f7_smallest_eigenvector3((fn[0] * fn[0] + fn[3] * fn[3]) + fn[6] * fn[6], (fn[0] * fn[1] + fn[3] * fn[4]) + fn[6] * fn[7],
                               (fn[0] * fn[2] + fn[3] * fn[5]) + fn[6] * fn[8], (fn[1] * fn[1] + fn[4] * fn[4]) + fn[7] * fn[7],
                               (fn[1] * fn[2] + fn[4] * fn[5]) + fn[7] * fn[8], (fn[2] * fn[2] + fn[5] * fn[5]) + fn[8] * fn[8], w);
#pragma unroll
      for (int r = 0; r < 3; r++) {
        const double fw = (fn[3 * r] * w[0] + fn[3 * r + 1] * w[1]) + fn[3 * r + 2] * w[2];
        fn[3 * r] = fn[3 * r] - fw * w[0]; fn[3 * r + 1] = fn[3 * r + 1] - fw * w[1]; fn[3 * r + 2] = fn[3 * r + 2] - fw * w[2];
      }
      const bool ok = (fabs(s1) < __builtin_inf()) && (fabs(s2) < __builtin_inf()) && f7_denormalise(fn, c1x, c1y, s1, c2x, c2y, s2, Fd);
      if (ok) for (int k = 0; k < 9; k++) s_F[k] = Fd[k];    // without a finite re-fit the winner itself is returned
    }
  }
  __syncthreads();
  // ---- cost: the sum of err over the mask at the returned F
  double F[9];
  for (int k = 0; k < 9; k++) F[k] = s_F[k];
#pragma unroll
  for (int k = 0; k < VO_NSUM; k++) acc[k] = 0.0;
  for (int i = tid; i < n; i += 256) {
    if (!mask[i]) continue;
    const float2 a = pa[i], c = pb[i];
    double err;
    (void)f7_inlier(F, (double)a.x, (double)a.y, (double)c.x, (double)c.y, thr2, err);
    acc[0] += err;
  }
  vo_block_sum(acc, s_part, s_tot);
  if (tid == 0) {
    for (int k = 0; k < 9; k++) { out[k] = F[k]; out[9 + k] = F0[k]; }
    out[18] = s_tot[0]; out[19] = m;
    for (int k = 20; k < F7_OUT; k++) out[k] = 0.0;
  }
}

// ================================================================================================
// host
// ================================================================================================
void vo_fund_destroy(vo_ctx* c) { vo_tv_free(c->fund); }

extern "C" int32_t vo_fundamental_default_params(vo_fund_params* p) {
  if (!p) return VO_E_INVALID;
  p->threshold = 3.0; p->confidence = 0.99; p->max_iters = 1000; p->seed = 0; p->refit = 0; p->_pad = 0;
  return VO_OK;
}

// the whole search on stream q: upload, rounds, finish, read-back
static int32_t fund_search(vo_ctx* c, hipStream_t q, const float* pts1, const float* pts2, int n, const vo_fund_params* prm, uint8_t* inlier_mask) {
  vo_fund_ws* w = c->fund;
  const size_t B = c->batch;
  const int cap = w->cap;
  const double thr2 = prm->threshold * prm->threshold;
  int32_t r = vo_tv_upload(c, q, w, pts1, pts2, n);
  if (r != VO_OK) return r;
  hipLaunchKernelGGL(k_f7_init, dim3((unsigned)B), dim3(1), 0, q, w->d_ctrl, prm->max_iters);
  r = vo_ransac_rounds(c, q, w->d_ctrl.get(), w->h_ctrl.get(), B, (prm->max_iters + F7_BATCH - 1) / F7_BATCH, [&](int) {
    {
      vo_prof_scope prof(c, q, VO_PROF_FUND_SOLVE);
      hipLaunchKernelGGL(k_f7_solve, dim3(F7_BATCH / 64, (unsigned)B), dim3(64), 0, q, w->d_p, cap, n, (unsigned)prm->seed, w->d_hyp, w->d_ctrl);
    }
    {
      vo_prof_scope prof(c, q, VO_PROF_FUND_SCORE);
      hipLaunchKernelGGL(k_f7_score, dim3(F7_BATCH * F7_ROOTS / 4, (unsigned)B), dim3(256), 0, q, w->d_p, cap, n, thr2, w->d_hyp);
    }
    {
      vo_prof_scope prof(c, q, VO_PROF_FUND_SELECT);
      hipLaunchKernelGGL(k_f7_select, dim3((unsigned)B), dim3(F7_BATCH), 0, q, w->d_hyp, w->d_ctrl, n, prm->confidence, prm->max_iters);
    }
  });
  if (r != VO_OK) return r;
  {
    vo_prof_scope prof(c, q, VO_PROF_FUND_FINISH);
    hipLaunchKernelGGL(k_f7_finish, dim3((unsigned)B), dim3(256), 0, q, w->d_p, cap, n, thr2, prm->refit, w->d_ctrl, w->d_mask, w->d_out);
  }
  VO_HIP(c, hipGetLastError());
  return vo_tv_readback(c, q, w, F7_OUT, inlier_mask, n);
}

// pts1 / pts2 [batch][n][2] f32 (pixels, view 1 / view 2) -> F [batch][9] (the winner's, or the eight-point re-fit), F0 [batch][9] (the
// winning sample's), both of unit Frobenius norm with the largest entry positive and x2^T F x1 = 0; inlier_mask [batch][n] u8 (of F0),
// stats [batch].
extern "C" int32_t vo_fundamental_ransac(vo_ctx* c, const float* pts1, const float* pts2, int32_t n, const vo_fund_params* prm, double* F, double* F0,
                                         uint8_t* inlier_mask, vo_fund_stats* stats) {
  if (!c) return VO_E_INVALID;
  vo_fund_params def;
  if (!prm) { vo_fundamental_default_params(&def); prm = &def; }
  VO_CHECK(c, pts1 && pts2 && F, VO_E_INVALID, "null buffer");
  VO_CHECK(c, n >= 7, VO_E_INVALID, "at least 7 correspondences");
  VO_CHECK(c, prm->threshold > 0 && prm->threshold < __builtin_inf() && prm->confidence > 0 && prm->confidence < 1 && prm->max_iters >= 1 &&
           prm->refit >= 0 && prm->refit <= 1, VO_E_INVALID, "bad parameters");
  VO_HIP(c, hipSetDevice(c->device));
  int32_t r = vo_tv_alloc(c, c->fund, vo_fund_destroy, n, F7_OUT);
  if (r != VO_OK) return r;
  r = fund_search(c, c->stream, pts1, pts2, n, prm, inlier_mask);
  if (r != VO_OK) return r;
  const vo_fund_ws* w = c->fund;
  for (size_t b = 0; b < (size_t)c->batch; b++) {
    const double* o = w->h_out + F7_OUT * b;
    const f7_ctrl& hc = w->h_ctrl[b];
    const bool none = hc.best_h < 0;
    for (int k = 0; k < 9; k++) F[9 * b + k] = o[k];
    if (F0) for (int k = 0; k < 9; k++) F0[9 * b + k] = o[9 + k];
    if (stats) {
      stats[b].cost = o[18];
      stats[b].n_inliers = none ? 0 : (int32_t)o[19]; stats[b].hypotheses = hc.s.h_done; stats[b].best = hc.best_h;
      stats[b].status = none ? VO_E_NUMERIC : 0;
      stats[b].n_roots = none ? 0 : hc.n_roots; stats[b].models = hc.models;
    }
  }
  return VO_OK;
}
