// The two 3 x 3 Jacobi iterations that several units run on one lane, in registers: every loop has constant bounds and nothing is indexed
// by a run-time value, so the nine or eighteen entries never leave the register file.
//   vo_jacobi3_cols   one-sided (Hestenes) rotations on the columns of a general matrix -- its singular values and vectors without squaring
//                     its condition: vo_hpose.hip (G = K^-1 H K) and vo_sim3.hip (Umeyama's Sigma)
//   vo_jacobi3_sym    cyclic two-sided rotations on a symmetric matrix -- its eigenvalues and vectors: vo_fundamental.hip (the rank-2 step
//                     of the eight-point re-fit) and vo_sim3.hip (the scatter matrices of a consensus set)
// Both stop when every off-diagonal term is under 2^-52 of the geometric mean of its two diagonal terms (the test of vo_smallest_eigenvector9).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

// U (overwritten by U diag(sigma): its columns become orthogonal, their squared norms -> nn) and V (the accumulated rotations, V^T V = I),
// the columns ordered by descending norm; a tie keeps the column order: (0,1), (1,2), (0,1)
__device__ inline void vo_jacobi3_cols(double (&U)[3][3], double (&V)[3][3], double (&nn)[3]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) V[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 60; sweep++) {
    bool changed = false;
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
      for (int q = p + 1; q < 3; q++) {
        double al = 0, be = 0, ga = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) { al += U[k][p] * U[k][p]; be += U[k][q] * U[k][q]; ga += U[k][p] * U[k][q]; }
        if (ga * ga > 4.930380657631324e-32 * (al * be)) {
          changed = true;
          const double zeta = (be - al) / (2.0 * ga);
          const double tt = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double cs = 1.0 / sqrt(1.0 + tt * tt), sn = cs * tt;
#pragma unroll
          for (int k = 0; k < 3; k++) {
            const double up = U[k][p], uq = U[k][q];
            U[k][p] = cs * up - sn * uq; U[k][q] = sn * up + cs * uq;
            const double vp = V[k][p], vq = V[k][q];
            V[k][p] = cs * vp - sn * vq; V[k][q] = sn * vp + cs * vq;
          }
        }
      }
    if (!changed) break;
  }
#pragma unroll
  for (int j = 0; j < 3; j++) nn[j] = (U[0][j] * U[0][j] + U[1][j] * U[1][j]) + U[2][j] * U[2][j];
#pragma unroll
  for (int pass = 0; pass < 3; pass++) {
    const int j = (pass == 1) ? 1 : 0;
    const bool sw = nn[j] < nn[j + 1];
    { const double a = nn[j], b = nn[j + 1]; nn[j] = sw ? b : a; nn[j + 1] = sw ? a : b; }
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double a = U[k][j], b = U[k][j + 1]; U[k][j] = sw ? b : a; U[k][j + 1] = sw ? a : b;
      const double e = V[k][j], f = V[k][j + 1]; V[k][j] = sw ? f : e; V[k][j + 1] = sw ? e : f;
    }
  }
}

// the symmetric M -> its eigenvalues on the diagonal of M (in no order) and the eigenvectors in the columns of V
__device__ inline void vo_jacobi3_sym(double (&M)[3][3], double (&V)[3][3]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) V[i][j] = (i == j) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < 30; sweep++) {
    bool changed = false;
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
      for (int q = p + 1; q < 3; q++) {
        const double apq = M[p][q];
        if (apq * apq > 4.930380657631324e-32 * fabs(M[p][p] * M[q][q])) {       // as vo_smallest_eigenvector9
          changed = true;
          const double zeta = (M[q][q] - M[p][p]) / (2.0 * apq);
          const double t = (zeta >= 0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
          const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
          for (int k = 0; k < 3; k++) { const double a = M[k][p], bq = M[k][q]; M[k][p] = c * a - s * bq; M[k][q] = s * a + c * bq; }
#pragma unroll
          for (int k = 0; k < 3; k++) { const double a = M[p][k], bq = M[q][k]; M[p][k] = c * a - s * bq; M[q][k] = s * a + c * bq; }
#pragma unroll
          for (int k = 0; k < 3; k++) { const double a = V[k][p], bq = V[k][q]; V[k][p] = c * a - s * bq; V[k][q] = s * a + c * bq; }
        }
      }
    if (!changed) break;
  }
}
