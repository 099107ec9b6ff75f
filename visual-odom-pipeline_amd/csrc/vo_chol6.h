// The 6 x 6 Cholesky solve of the two pose refinements that iterate inside one workgroup: the PnP Gauss-Newton (k_pnp_refine, vo_pnp.hip) and
// the sparse image alignment (k_align_level, vo_align.hip).  One lane, float64, everything in registers.
#pragma once
#include <hip/hip_runtime.h>

// 1 / sqrt(x) from v_rsq_f64 + two Newton steps
__device__ __forceinline__ double vo_rsqrt_nr(double x) {
  double y = __builtin_amdgcn_rsq(x);
  double e = fma(-x * y, y, 1.0);
  y = fma(0.5 * y, e, y);
  e = fma(-x * y, y, 1.0);
  return fma(0.5 * y, e, y);
}

// H d = g for the symmetric H whose upper triangle lies row by row in s[0 .. 20]; -> false if a pivot is not positive (d is then
// meaningless).  Every loop is unrolled over compile-time bounds (no early exit: a bad pivot only clears the flag), so the factor lives in
// registers -- indexed by run-time loop counters it sat in scratch memory (480 bytes per thread) and every access of this one-lane chain
// was a memory round trip
__device__ __forceinline__ bool vo_chol6_solve(const double* s, const double (&g)[6], double (&d)[6]) {
  double Hm[6][6];
  {
    int q = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
      for (int c = a; c < 6; c++) { Hm[a][c] = s[q]; Hm[c][a] = s[q]; q++; }
  }
  bool okc = true;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    double sdiag = Hm[j][j];
#pragma unroll
    for (int k = 0; k < j; k++) sdiag -= Hm[j][k] * Hm[j][k];
    if (!(sdiag > 0)) { okc = false; sdiag = 1.0; }
    const double rs = vo_rsqrt_nr(sdiag);         // 1 / L_jj
    Hm[j][j] = rs;                                // the diagonal holds the INVERSE pivot
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      double sv = Hm[i][j];
#pragma unroll
      for (int k = 0; k < j; k++) sv -= Hm[i][k] * Hm[j][k];
      Hm[i][j] = sv * rs;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double sv = g[i];
#pragma unroll
    for (int k = 0; k < i; k++) sv -= Hm[i][k] * d[k];
    d[i] = sv * Hm[i][i];
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    double sv = d[i];
#pragma unroll
    for (int k = i + 1; k < 6; k++) sv -= Hm[k][i] * d[k];
    d[i] = sv * Hm[i][i];
  }
  return okc;
}
