// The RANSAC searches' counter-based sample generator and OpenCV's iteration bound, for translation units that include it
// (vo_homography.hip; vo_pnp.hip and vo_essential.hip carry the same arithmetic as private copies from before this header existed).
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ unsigned long long vo_splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  unsigned long long z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// M distinct indices in [0, n), n >= M, of hypothesis h: draw k is splitmix64(seed, h, k) mod n, a draw that repeats an index is skipped
// (M = 5: e5_sample5, M = 4: pnp_sample4 and sample4(seed, h, n) of tests/homography_model.py)
template <int M>
__device__ inline void vo_ransac_sample(unsigned seed, unsigned h, int n, int* idx) {
  int cnt = 0;
  unsigned k = 0;
  while (cnt < M) {
    const unsigned long long r = (k < 256) ? vo_splitmix64(((unsigned long long)(seed & 0xFFFFFFu) << 40) ^ ((unsigned long long)h << 8) ^ (unsigned long long)(k & 0xFFu))
                                           : vo_splitmix64((unsigned long long)k);
    const int i = (int)((r >> 11) % (unsigned long long)n);
    k++;
    bool dup = false;
    for (int j = 0; j < cnt; j++) dup = dup || (idx[j] == i);
    if (!dup) idx[cnt++] = i;
  }
}

__device__ inline int vo_ransac_update_iters(double p, double ep, int model_points, int max_iters) {   // OpenCV RANSACUpdateNumIters
  p = fmin(fmax(p, 0.0), 1.0); ep = fmin(fmax(ep, 0.0), 1.0);
  double num = fmax(1.0 - p, 2.2250738585072014e-308);
  double denom = 1.0 - pow(1.0 - ep, (double)model_points);
  if (denom < 2.2250738585072014e-308) return 0;
  num = log(num); denom = log(denom);
  return (denom >= 0 || -num >= max_iters * (-denom)) ? max_iters : (int)rint(num / denom);
}
