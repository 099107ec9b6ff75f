// Homography RANSAC for the 2D-2D bootstrap: the planar / rotational model that is fitted next to the essential matrix to tell a degenerate
// frame pair (no baseline, or a planar scene) from one the five-point pose can be trusted on.
//
// The reference's bootstrap names the step in a comment only (src/pipeline/pipeline.py:66, "Estimate homography") and goes on with
// findEssentialMat alone; this is  H, mask = cv2.findHomography(p1, p2, cv2.RANSAC, 3.0, maxIters=2000, confidence=0.995)  of OpenCV 4.4
// (modules/calib3d/src/fundam.cpp, ptsetreg.cpp).  OpenCV's sample draws cannot be reproduced and its float32 error is not kept; the algorithm
// is defined by tests/homography_model.py and compared with it hypothesis by hypothesis:
//   sample     hypothesis h draws sample4(seed, h, n) = vo_ransac_sample<4>: four distinct indices, no redraw
//   checkSubset  no three of the four points collinear in either view (haveCollinearPoints' test on all four triples), and the orientation
//              of the four triples either kept or reversed together by the map (HomographyEstimatorCallback::checkSubset); a rejected sample
//              has no model and still counts as one hypothesis
//   solve      one lane per sample, float64: Hartley normalisation of the four points of each view (centroid, mean distance sqrt 2), the
//              8 x 8 system with h33 = 1 in that frame by Gaussian elimination with partial pivoting, denormalised, unit Frobenius norm
//   consensus  one wave per hypothesis: |x2 - proj(H x1)|^2 <= threshold^2 in float64
//   select     most inliers, ties to the smallest h, at least 4; iteration bound RANSACUpdateNumIters with 4 model points
//   finish     one workgroup per sequence: mask of the winner H0 (not recomputed afterwards, as in OpenCV); with n > 4 the normalised DLT on
//              the inliers (smallest eigenvector of the 9 x 9 normal matrix by Jacobi) and up to refine_iters Levenberg-Marquardt steps on
//              the forward transfer error in the 8 parameters of the normalised frame (its scale is isotropic, so the minimiser is the
//              pixel error's); cost = sum of squared pixel errors over the mask at the returned H
// Rounds of 256 hypotheses, a control block per sequence, [batch] everywhere, everything on ctx->stream.  What the searches share on the
// sampling side (generator, bound, control head, select tail, the host's round loop) is vo_ransac.h; what the two-view units share beyond
// it (workspace, upload and read-back, a sequence's pointers, the mask, Hartley and Gram passes of the finish kernel) is vo_twoview.h.
// This library is built with -ffp-contract=off: the sign tests of checkSubset evaluate exactly as the model's float64 expressions do.
#include "vo_internal.h"
#include "vo_twoview.h"

#include <math.h>
#include <string.h>

#define H4_BATCH 256
#define H4_OUT 24              // doubles per sequence: H (9), H0 (9), cost, n_inliers, lm_iters, 3 spare
#define H4_NSUM VO_NSUM        // sums of one reduction pass: the 45 distinct entries of a 9 x 9 normal matrix, or 36 + 8 + 1 of an LM step

struct h4_hyp { double H[9]; int count; int ok; int h; int pad; };
struct h4_ctrl { vo_ransac_state s; int best_h, best_count, pad; double H[9]; };
static_assert(sizeof(h4_ctrl) == 96 && offsetof(h4_ctrl, best_h) == 12 && offsetof(h4_ctrl, best_count) == 16 && offsetof(h4_ctrl, pad) == 20 &&
              offsetof(h4_ctrl, H) == 24, "h4_ctrl layout");

struct vo_hom_ws : vo_tv_search_ws<h4_hyp, h4_ctrl, H4_BATCH> {};

// ------------------------------------------------------------------------------------------------
// the minimal problem
// ------------------------------------------------------------------------------------------------
// OpenCV's haveCollinearPoints test of the triple (a, b, pivot): the pivot is the triple's last point
__device__ __forceinline__ bool h4_collinear(double ax, double ay, double bx, double by, double px, double py) {
  const double dx1 = bx - px, dy1 = by - py, dx2 = ax - px, dy2 = ay - py;
  return fabs(dx2 * dy1 - dy2 * dx1) <= 1.1920928955078125e-07 * (((fabs(dx1) + fabs(dy1)) + fabs(dx2)) + fabs(dy2));
}

// determinant of [[x0 y0 1] [x1 y1 1] [x2 y2 1]] in the order of cv::determinant(Matx33d)
__device__ __forceinline__ double h4_det3(double x0, double y0, double x1, double y1, double x2, double y2) {
  return (x0 * (y1 - y2) - y0 * (x1 - x2)) + (x1 * y2 - y1 * x2);
}

__device__ inline bool h4_check_subset(const double (&x1)[4], const double (&y1)[4], const double (&x2)[4], const double (&y2)[4]) {
  bool col = false;
  col = col || h4_collinear(x1[0], y1[0], x1[1], y1[1], x1[2], y1[2]) || h4_collinear(x2[0], y2[0], x2[1], y2[1], x2[2], y2[2]);
  col = col || h4_collinear(x1[0], y1[0], x1[1], y1[1], x1[3], y1[3]) || h4_collinear(x2[0], y2[0], x2[1], y2[1], x2[3], y2[3]);
  col = col || h4_collinear(x1[0], y1[0], x1[2], y1[2], x1[3], y1[3]) || h4_collinear(x2[0], y2[0], x2[2], y2[2], x2[3], y2[3]);
  col = col || h4_collinear(x1[1], y1[1], x1[2], y1[2], x1[3], y1[3]) || h4_collinear(x2[1], y2[1], x2[2], y2[2], x2[3], y2[3]);
  if (col) return false;
  int negative = 0;
  negative += (h4_det3(x1[0], y1[0], x1[1], y1[1], x1[2], y1[2]) * h4_det3(x2[0], y2[0], x2[1], y2[1], x2[2], y2[2]) < 0) ? 1 : 0;
  negative += (h4_det3(x1[1], y1[1], x1[2], y1[2], x1[3], y1[3]) * h4_det3(x2[1], y2[1], x2[2], y2[2], x2[3], y2[3]) < 0) ? 1 : 0;
  negative += (h4_det3(x1[0], y1[0], x1[2], y1[2], x1[3], y1[3]) * h4_det3(x2[0], y2[0], x2[2], y2[2], x2[3], y2[3]) < 0) ? 1 : 0;
  negative += (h4_det3(x1[0], y1[0], x1[1], y1[1], x1[3], y1[3]) * h4_det3(x2[0], y2[0], x2[1], y2[1], x2[3], y2[3]) < 0) ? 1 : 0;
  return negative == 0 || negative == 4;
}

// Hartley normalisation of four points in place: -> centroid and scale, x <- (x - c) s with mean distance sqrt 2
__device__ inline void h4_normalise4(double (&x)[4], double (&y)[4], double& cx, double& cy, double& s) {
  cx = 0.25 * ((x[0] + x[1]) + (x[2] + x[3]));
  cy = 0.25 * ((y[0] + y[1]) + (y[2] + y[3]));
  double d = 0.0;
#pragma unroll
  for (int i = 0; i < 4; i++) { x[i] = x[i] - cx; y[i] = y[i] - cy; d += sqrt(x[i] * x[i] + y[i] * y[i]); }
  s = 1.4142135623730951 / (0.25 * d);
#pragma unroll
  for (int i = 0; i < 4; i++) { x[i] = x[i] * s; y[i] = y[i] * s; }
}

// Hn (normalised frame) -> T2^-1 Hn T1 with T = [[s 0 -s cx] [0 s -s cy] [0 0 1]], scaled to unit Frobenius norm with h33 >= 0.
// -> false if an entry is not finite or the norm is 0
__device__ inline bool h4_denormalise(const double* Hn, double c1x, double c1y, double s1, double c2x, double c2y, double s2, double* H) {
  double M[9], nn = 0.0;
  vo_tv_right_factor(Hn, c1x, c1y, s1, M);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    H[k] = M[k] / s2 + c2x * M[6 + k];
    H[3 + k] = M[3 + k] / s2 + c2y * M[6 + k];
    H[6 + k] = M[6 + k];
  }
#pragma unroll
  for (int k = 0; k < 9; k++) nn += H[k] * H[k];
  nn = sqrt(nn);
  if (!(nn > 0) || !(nn < __builtin_inf())) return false;
  const double sc = (H[8] < 0 ? -1.0 : 1.0) / nn;
#pragma unroll
  for (int k = 0; k < 9; k++) H[k] = H[k] * sc;
  return true;
}

// the 8 x 8 system of four normalised correspondences with h33 = 1: Gaussian elimination with partial pivoting.  Every loop has constant
// bounds and the pivot row is brought up by conditional row swaps, so that after unrolling no array is indexed by a run-time value and the
// 72 entries live in registers
__device__ inline void h4_solve8(const double (&x)[4], const double (&y)[4], const double (&u)[4], const double (&v)[4], double* Hn) {
  double A[8][9];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    A[2 * i][0] = x[i]; A[2 * i][1] = y[i]; A[2 * i][2] = 1.0; A[2 * i][3] = 0.0; A[2 * i][4] = 0.0; A[2 * i][5] = 0.0;
    A[2 * i][6] = -(x[i] * u[i]); A[2 * i][7] = -(y[i] * u[i]); A[2 * i][8] = u[i];
    A[2 * i + 1][0] = 0.0; A[2 * i + 1][1] = 0.0; A[2 * i + 1][2] = 0.0; A[2 * i + 1][3] = x[i]; A[2 * i + 1][4] = y[i]; A[2 * i + 1][5] = 1.0;
    A[2 * i + 1][6] = -(x[i] * v[i]); A[2 * i + 1][7] = -(y[i] * v[i]); A[2 * i + 1][8] = v[i];
  }
#pragma unroll
  for (int c = 0; c < 8; c++) {
#pragma unroll
    for (int r = c + 1; r < 8; r++) {
      const bool sw = fabs(A[r][c]) > fabs(A[c][c]);
#pragma unroll
      for (int k = c; k < 9; k++) {
        const double a = A[c][k], b = A[r][k];
        A[c][k] = sw ? b : a; A[r][k] = sw ? a : b;
      }
    }
    const double inv = 1.0 / A[c][c];                  // a zero pivot makes every later entry non-finite: no model
#pragma unroll
    for (int r = c + 1; r < 8; r++) {
      const double f = A[r][c] * inv;
#pragma unroll
      for (int k = c + 1; k < 9; k++) A[r][k] = A[r][k] - f * A[c][k];
    }
  }
#pragma unroll
  for (int c = 7; c >= 0; c--) {
    double s = A[c][8];
#pragma unroll
    for (int k = c + 1; k < 8; k++) s = s - A[c][k] * Hn[k];
    Hn[c] = s / A[c][c];
  }
  Hn[8] = 1.0;
}

// x2 ~ H x1 within the squared pixel threshold; a NaN coordinate or a projective w that is 0 or not finite is never an inlier
__device__ __forceinline__ bool h4_inlier(const double* H, double x, double y, double u, double v, double thr2) {
  const double w = (H[6] * x + H[7] * y) + H[8];
  const double iw = 1.0 / w;
  const double dx = u - ((H[0] * x + H[1] * y) + H[2]) * iw, dy = v - ((H[3] * x + H[4] * y) + H[5]) * iw;
  return (w != 0.0) && (fabs(w) < __builtin_inf()) && (dx * dx + dy * dy <= thr2);
}

// ------------------------------------------------------------------------------------------------
// kernels of the search
// ------------------------------------------------------------------------------------------------
__global__ void k_h4_init(h4_ctrl* ctrl, int max_iters) {
  h4_ctrl* c = ctrl + blockIdx.x;
  vo_ransac_reset(&c->s, max_iters);
  c->best_h = -1; c->best_count = 3; c->pad = 0;
  for (int i = 0; i < 9; i++) c->H[i] = 0;
}

// grid (H4_BATCH / 64, batch), a lane per hypothesis
__global__ void __launch_bounds__(64) k_h4_solve(const float* __restrict__ p, int cap, int n, unsigned seed, h4_hyp* __restrict__ hyps,
                                                 const h4_ctrl* __restrict__ ctrl) {
  const int b = blockIdx.y, slot = blockIdx.x * 64 + threadIdx.x;
  const h4_ctrl* cs = ctrl + b;
  h4_hyp* out = hyps + (size_t)b * H4_BATCH + slot;
  const int h = cs->s.h_done + slot;
  out->h = h; out->count = 0; out->ok = 0;
  if (cs->s.done) return;
  const auto [pa, pb] = vo_tv_seq_views<float>(p, cap, b);
  int idx[4];
  vo_ransac_sample<4>(seed, (unsigned)h, n, idx);
  const int i0 = idx[0], i1 = idx[1], i2 = idx[2], i3 = idx[3];
  double x1[4] = {(double)pa[2 * i0], (double)pa[2 * i1], (double)pa[2 * i2], (double)pa[2 * i3]};
  double y1[4] = {(double)pa[2 * i0 + 1], (double)pa[2 * i1 + 1], (double)pa[2 * i2 + 1], (double)pa[2 * i3 + 1]};
  double x2[4] = {(double)pb[2 * i0], (double)pb[2 * i1], (double)pb[2 * i2], (double)pb[2 * i3]};
  double y2[4] = {(double)pb[2 * i0 + 1], (double)pb[2 * i1 + 1], (double)pb[2 * i2 + 1], (double)pb[2 * i3 + 1]};
  if (!h4_check_subset(x1, y1, x2, y2)) return;          // NaN coordinates pass every comparison above and end as a non-finite H below
  double c1x, c1y, s1, c2x, c2y, s2, Hn[9], H[9];
  h4_normalise4(x1, y1, c1x, c1y, s1);
  h4_normalise4(x2, y2, c2x, c2y, s2);
  h4_solve8(x1, y1, x2, y2, Hn);
  bool ok = h4_denormalise(Hn, c1x, c1y, s1, c2x, c2y, s2, H);
#pragma unroll
  for (int k = 0; k < 9; k++) ok = ok && (fabs(H[k]) < __builtin_inf());
  if (!ok) return;
#pragma unroll
  for (int k = 0; k < 9; k++) out->H[k] = H[k];
  out->ok = 1;
}

// grid (H4_BATCH / 4, batch), 4 waves: a wave counts the consensus of one hypothesis; the points are read once per wave
__global__ void __launch_bounds__(256) k_h4_score(const float* __restrict__ p, int cap, int n, double thr2, h4_hyp* __restrict__ hyps) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  h4_hyp* hp = hyps + (size_t)b * H4_BATCH + blockIdx.x * 4 + (threadIdx.x >> 6);
  if (!hp->ok) return;                                   // count stays 0 (k_h4_solve)
  const auto [pa, pb] = vo_tv_seq_views<float2>(p, cap, b);
  const double H0 = hp->H[0], H1 = hp->H[1], H2 = hp->H[2], H3 = hp->H[3], H4 = hp->H[4], H5 = hp->H[5], H6 = hp->H[6], H7 = hp->H[7], H8 = hp->H[8];
  const double H[9] = {H0, H1, H2, H3, H4, H5, H6, H7, H8};
  int cnt = 0;
  for (int i = lane; i < n; i += 64) {
    const float2 a = pa[i], c = pb[i];
    cnt += h4_inlier(H, (double)a.x, (double)a.y, (double)c.x, (double)c.y, thr2) ? 1 : 0;
  }
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
  if (lane == 0) hp->count = cnt;
}

// grid (batch): running best (most inliers; ties to the smallest h) and the iteration bound
__global__ void __launch_bounds__(H4_BATCH) k_h4_select(const h4_hyp* __restrict__ hyps, h4_ctrl* __restrict__ ctrl, int n, double conf, int max_iters) {
  __shared__ int s_cnt[H4_BATCH];
  const int b = blockIdx.x, tid = threadIdx.x;
  h4_ctrl* c = ctrl + b;
  if (c->s.done) return;
  const h4_hyp* H = hyps + (size_t)b * H4_BATCH;
  s_cnt[tid] = H[tid].ok ? H[tid].count : -1;
  __syncthreads();
  if (tid == 0) {
    const int bi = vo_ransac_best_slot(s_cnt, H4_BATCH, c->best_count);
    if (bi >= 0) {
      c->best_count = s_cnt[bi]; c->best_h = H[bi].h;
      for (int i = 0; i < 9; i++) c->H[i] = H[bi].H[i];
    }
    vo_ransac_advance(&c->s, H4_BATCH, n, c->best_count, c->best_h >= 0, conf, 4, max_iters);
  }
}

// ------------------------------------------------------------------------------------------------
// finish: mask, DLT re-fit, Levenberg-Marquardt
// ------------------------------------------------------------------------------------------------
// (A + lam diag A) d = -g for the 8 x 8 normal matrix packed in s (upper triangle, row by row, then g): Cholesky.  -> false on a
// non-positive pivot
__device__ inline bool h4_lm_step(const double* s, double lam, double* d) {
  double L[8][8];
  for (int a = 0, k = 0; a < 8; a++)
    for (int b = a; b < 8; b++, k++) L[b][a] = (a == b) ? s[k] + lam * s[k] : s[k];
  for (int a = 0; a < 8; a++)
    for (int b = 0; b <= a; b++) {
      double v = L[a][b];
      for (int k = 0; k < b; k++) v -= L[a][k] * L[b][k];
      if (a == b) {
        if (!(v > 0)) return false;
        L[a][a] = sqrt(v);
      } else {
        L[a][b] = v / L[b][b];
      }
    }
  for (int a = 0; a < 8; a++) {
    double v = -s[36 + a];
    for (int k = 0; k < a; k++) v -= L[a][k] * d[k];
    d[a] = v / L[a][a];
  }
  for (int a = 7; a >= 0; a--) {
    double v = d[a];
    for (int k = a + 1; k < 8; k++) v -= L[k][a] * d[k];
    d[a] = v / L[a][a];
  }
  return true;
}

#define H4_LM_LAMBDA0 1e-3
#define H4_LM_SLACK 9.313225746154785e-10      // 2^-30: a step is kept unless the cost rises by more than the rounding of its sum could explain
#define H4_LM_XTOL 3.552713678800501e-15       // 2^-48: a kept step this small (relative to max(1, |p|)) ends the refinement

// grid (batch), 256 threads
__global__ void __launch_bounds__(256) k_h4_finish(const float* __restrict__ p, int cap, int n, double thr2, int refine_iters,
                                                   const h4_ctrl* __restrict__ ctrl, uint8_t* __restrict__ mask_all, double* __restrict__ out_all) {
  __shared__ double s_part[4][H4_NSUM], s_tot[H4_NSUM], s_keep[H4_NSUM];
  __shared__ double s_M[9][9], s_V[9][9];
  __shared__ double s_nrm[6];                            // c1x c1y s1 c2x c2y s2
  __shared__ double s_p[8], s_try[8], s_H[9];
  __shared__ int s_flag, s_lm;
  const int b = blockIdx.x, tid = threadIdx.x;
  const auto [pa, pb, mask, out] = vo_tv_seq_rows<float2>(p, cap, b, mask_all, out_all, H4_OUT);
  const h4_ctrl* cs = ctrl + b;
  if (cs->best_h < 0) { vo_tv_no_winner(mask, n, out, H4_OUT, 19); return; }
  double H0[9];
  for (int k = 0; k < 9; k++) H0[k] = cs->H[k];
  double acc[H4_NSUM];
  // ---- the winner's mask, the inliers' count and centroids
  const vo_tv_centroids g = vo_tv_mask_pass(pa, pb, mask, n, [&](double x, double y, double u, double v) { return h4_inlier(H0, x, y, u, v, thr2); },
                                            acc, s_part, s_tot);
  const double m = g.m, c1x = g.c1x, c1y = g.c1y, c2x = g.c2x, c2y = g.c2y;
  if (tid == 0) { for (int k = 0; k < 9; k++) s_H[k] = H0[k]; s_lm = 0; s_flag = 0; }
  if (n > 4) {
    // ---- Hartley scales of the inliers, then the normal matrix of the DLT rows (-x -y -1 0 0 0 ux uy u), (0 0 0 -x -y -1 vx vy v)
    const auto [s1, s2] = vo_tv_scale_pass(pa, pb, mask, n, g, acc, s_part, s_tot);
    vo_tv_gram_pass(pa, pb, mask, n, g, s1, s2, [](double x, double y, double u, double v) {
      return vo_tv_rows<2>{{{-x, -y, -1.0, 0.0, 0.0, 0.0, u * x, u * y, u}, {0.0, 0.0, 0.0, -x, -y, -1.0, v * x, v * y, v}}};
    }, acc, s_part, s_tot);
    if (tid == 0) {
      vo_tv_unpack_sym9(s_tot, s_M);
      double hn[9];
      vo_smallest_eigenvector9(s_M, s_V, hn);
      bool ok = true;
      for (int k = 0; k < 9; k++) ok = ok && (fabs(hn[k]) < __builtin_inf());
      for (int k = 0; k < 8; k++) { s_p[k] = hn[k] / hn[8]; ok = ok && (fabs(s_p[k]) < __builtin_inf()); }
      double Hd[9];
      ok = ok && (fabs(s1) < __builtin_inf()) && (fabs(s2) < __builtin_inf()) && h4_denormalise(hn, c1x, c1y, s1, c2x, c2y, s2, Hd);
      for (int k = 0; k < 9; k++) ok = ok && (fabs(Hd[k]) < __builtin_inf());
      if (ok) for (int k = 0; k < 9; k++) s_H[k] = Hd[k];      // the DLT re-fit; without one the winner itself is returned
      s_flag = (ok && refine_iters > 0) ? 1 : 0;
      s_nrm[0] = c1x; s_nrm[1] = c1y; s_nrm[2] = s1; s_nrm[3] = c2x; s_nrm[4] = c2y; s_nrm[5] = s2;
    }
    __syncthreads();
    if (s_flag) {
      // ---- Levenberg-Marquardt on the forward transfer error, 8 parameters (h33 = 1) of the normalised frame.  Pass `it` evaluates the
      // trial point of step `it` (pass 0: the DLT start) -- cost, J^T J (36), J^T r (8) -- and thread 0 keeps or drops it and sets the next
      double lam = H4_LM_LAMBDA0, cost = 0.0;
      int steps = 0;
      if (tid == 0) for (int k = 0; k < 8; k++) s_try[k] = s_p[k];
      __syncthreads();
      for (int it = 0; it <= refine_iters; it++) {
        double q[8];
#pragma unroll
        for (int k = 0; k < 8; k++) q[k] = s_try[k];
#pragma unroll
        for (int k = 0; k < H4_NSUM; k++) acc[k] = 0.0;
        for (int i = tid; i < n; i += 256) {
          if (!mask[i]) continue;
          const float2 a = pa[i], c = pb[i];
          const double x = ((double)a.x - c1x) * s1, y = ((double)a.y - c1y) * s1, u = ((double)c.x - c2x) * s2, v = ((double)c.y - c2y) * s2;
          const double iw = 1.0 / ((q[6] * x + q[7] * y) + 1.0);
          const double X = ((q[0] * x + q[1] * y) + q[2]) * iw, Y = ((q[3] * x + q[4] * y) + q[5]) * iw;
          const double rx = X - u, ry = Y - v;
          const double jx[8] = {x * iw, y * iw, iw, 0.0, 0.0, 0.0, -(x * iw) * X, -(y * iw) * X};
          const double jy[8] = {0.0, 0.0, 0.0, x * iw, y * iw, iw, -(x * iw) * Y, -(y * iw) * Y};
          int k = 0;
#pragma unroll
          for (int ia = 0; ia < 8; ia++)
#pragma unroll
            for (int ib = ia; ib < 8; ib++, k++) acc[k] += jx[ia] * jx[ib] + jy[ia] * jy[ib];
#pragma unroll
          for (int ia = 0; ia < 8; ia++) acc[36 + ia] += jx[ia] * rx + jy[ia] * ry;
          acc[44] += rx * rx + ry * ry;
        }
        vo_block_sum(acc, s_part, s_tot);
        if (tid == 0) {
          bool stop = false;
          const double cnew = s_tot[44];
          if (it == 0) {
            if (!(cnew < __builtin_inf())) stop = true;                          // the DLT start has no finite cost: it is returned as it is
            else { cost = cnew; for (int k = 0; k < H4_NSUM; k++) s_keep[k] = s_tot[k]; }
          } else if (cnew <= cost + H4_LM_SLACK * cost) {                        // kept (NaN fails the comparison)
            double big = 1.0, dmax = 0.0;
            for (int k = 0; k < 8; k++) { big = fmax(big, fabs(s_try[k])); dmax = fmax(dmax, fabs(s_try[k] - s_p[k])); }
            for (int k = 0; k < 8; k++) s_p[k] = s_try[k];
            for (int k = 0; k < H4_NSUM; k++) s_keep[k] = s_tot[k];
            cost = cnew; lam = fmax(lam * 0.1, 1e-12);
            if (dmax <= H4_LM_XTOL * big) stop = true;
          } else {
            lam = lam * 10.0;
          }
          if (!stop && it < refine_iters) {
            double d[8];
            if (h4_lm_step(s_keep, lam, d)) { for (int k = 0; k < 8; k++) s_try[k] = s_p[k] + d[k]; steps++; }
            else stop = true;
          } else {
            stop = true;
          }
          s_flag = stop ? 0 : 1;
        }
        __syncthreads();
        if (!s_flag) break;
      }
      if (tid == 0) {
        s_lm = steps;
        if (steps > 0) {
          double hn[9], Hd[9];
          for (int k = 0; k < 8; k++) hn[k] = s_p[k];
          hn[8] = 1.0;
          bool ok = h4_denormalise(hn, s_nrm[0], s_nrm[1], s_nrm[2], s_nrm[3], s_nrm[4], s_nrm[5], Hd);
          for (int k = 0; k < 9; k++) ok = ok && (fabs(Hd[k]) < __builtin_inf());
          if (ok) for (int k = 0; k < 9; k++) s_H[k] = Hd[k];
        }
      }
    }
  }
  __syncthreads();
  // ---- cost in pixels over the mask at the returned H
  double H[9];
  for (int k = 0; k < 9; k++) H[k] = s_H[k];
#pragma unroll
  for (int k = 0; k < H4_NSUM; k++) acc[k] = 0.0;
  for (int i = tid; i < n; i += 256) {
    if (!mask[i]) continue;
    const float2 a = pa[i], c = pb[i];
    const double x = (double)a.x, y = (double)a.y;
    const double w = (H[6] * x + H[7] * y) + H[8];
    const double dx = (double)c.x - ((H[0] * x + H[1] * y) + H[2]) / w, dy = (double)c.y - ((H[3] * x + H[4] * y) + H[5]) / w;
    acc[0] += dx * dx + dy * dy;
  }
  vo_block_sum(acc, s_part, s_tot);
  if (tid == 0) {
    for (int k = 0; k < 9; k++) { out[k] = H[k]; out[9 + k] = H0[k]; }
    out[18] = s_tot[0]; out[19] = m; out[20] = (double)s_lm; out[21] = 0.0; out[22] = 0.0; out[23] = 0.0;
  }
}

// ================================================================================================
// host
// ================================================================================================
void vo_hom_destroy(vo_ctx* c) { vo_tv_free(c->hom); }

extern "C" int32_t vo_homography_default_params(vo_hom_params* p) {
  if (!p) return VO_E_INVALID;
  p->threshold = 3.0; p->confidence = 0.995; p->max_iters = 2000; p->seed = 0; p->refine_iters = 10; p->_pad = 0;
  return VO_OK;
}

// pts1 / pts2 [batch][n][2] f32 (pixels, view 1 / view 2) -> H [batch][9] (refined), H0 [batch][9] (the winning sample's), both of unit
// Frobenius norm with h33 >= 0 and x2 ~ H x1; inlier_mask [batch][n] u8 (of H0), stats [batch].
extern "C" int32_t vo_homography_ransac(vo_ctx* c, const float* pts1, const float* pts2, int32_t n, const vo_hom_params* prm, double* H, double* H0,
                                        uint8_t* inlier_mask, vo_hom_stats* stats) {
  return vo_hom_ransac_tail(c, pts1, pts2, n, prm, H, H0, inlier_mask, stats, nullptr);
}

int32_t vo_hom_ransac_tail(vo_ctx* c, const float* pts1, const float* pts2, int32_t n, const vo_hom_params* prm, double* H, double* H0,
                           uint8_t* inlier_mask, vo_hom_stats* stats, const vo_hom_tail* tail) {
  if (!c) return VO_E_INVALID;
  vo_hom_params def;
  if (!prm) { vo_homography_default_params(&def); prm = &def; }
  VO_CHECK(c, pts1 && pts2 && H, VO_E_INVALID, "null buffer");
  VO_CHECK(c, n >= 4, VO_E_INVALID, "at least 4 correspondences");
  VO_CHECK(c, prm->threshold > 0 && prm->confidence > 0 && prm->confidence < 1 && prm->max_iters >= 1 && prm->refine_iters >= 0 && prm->refine_iters <= 100,
           VO_E_INVALID, "bad parameters");
  VO_HIP(c, hipSetDevice(c->device));
  int32_t r = vo_tv_alloc(c, c->hom, vo_hom_destroy, n, H4_OUT);
  if (r != VO_OK) return r;
  vo_hom_ws* w = c->hom;
  const size_t B = c->batch;
  const int cap = w->cap;
  const double thr2 = prm->threshold * prm->threshold;
  r = vo_tv_upload(c, c->stream, w, pts1, pts2, n);
  if (r != VO_OK) return r;
  hipLaunchKernelGGL(k_h4_init, dim3((unsigned)B), dim3(1), 0, c->stream, w->d_ctrl, prm->max_iters);
  r = vo_ransac_rounds(c, c->stream, w->d_ctrl.get(), w->h_ctrl.get(), B, (prm->max_iters + H4_BATCH - 1) / H4_BATCH, [&](int) {
    {
      vo_prof_scope prof(c, c->stream, VO_PROF_HOM_SOLVE);
      hipLaunchKernelGGL(k_h4_solve, dim3(H4_BATCH / 64, (unsigned)B), dim3(64), 0, c->stream, w->d_p, cap, n, (unsigned)prm->seed, w->d_hyp, w->d_ctrl);
    }
    {
      vo_prof_scope prof(c, c->stream, VO_PROF_HOM_SCORE);
      hipLaunchKernelGGL(k_h4_score, dim3(H4_BATCH / 4, (unsigned)B), dim3(256), 0, c->stream, w->d_p, cap, n, thr2, w->d_hyp);
    }
    {
      vo_prof_scope prof(c, c->stream, VO_PROF_HOM_SELECT);
      hipLaunchKernelGGL(k_h4_select, dim3((unsigned)B), dim3(H4_BATCH), 0, c->stream, w->d_hyp, w->d_ctrl, n, prm->confidence, prm->max_iters);
    }
  });
  if (r != VO_OK) return r;
  {
    vo_prof_scope prof(c, c->stream, VO_PROF_HOM_FINISH);
    hipLaunchKernelGGL(k_h4_finish, dim3((unsigned)B), dim3(256), 0, c->stream, w->d_p, cap, n, thr2, prm->refine_iters, w->d_ctrl, w->d_mask, w->d_out);
  }
  VO_HIP(c, hipGetLastError());
  if (tail) {
    r = tail->enqueue(c, c->stream, w->d_p, cap, n, w->d_out, H4_OUT, w->d_mask, tail->user);
    if (r != VO_OK) return r;
  }
  r = vo_tv_readback(c, c->stream, w, H4_OUT, inlier_mask, n);
  if (r != VO_OK) return r;
  for (size_t b = 0; b < B; b++) {
    const double* o = w->h_out + H4_OUT * b;
    const bool none = w->h_ctrl[b].best_h < 0;
    for (int k = 0; k < 9; k++) H[9 * b + k] = o[k];
    if (H0) for (int k = 0; k < 9; k++) H0[9 * b + k] = o[9 + k];
    if (stats) {
      stats[b].cost = o[18];
      stats[b].n_inliers = none ? 0 : (int32_t)o[19]; stats[b].hypotheses = w->h_ctrl[b].s.h_done; stats[b].best = w->h_ctrl[b].best_h;
      stats[b].status = none ? VO_E_NUMERIC : 0;
      stats[b].lm_iters = none ? 0 : (int32_t)o[20]; stats[b]._pad = 0;
    }
  }
  return VO_OK;
}
