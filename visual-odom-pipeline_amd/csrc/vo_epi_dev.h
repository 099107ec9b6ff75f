// The symmetric epipolar error shared by the fundamental-matrix search (vo_fundamental.hip: the consensus of a model) and the guided
// matcher (vo_match.hip: the epipolar gate of a pair), so that a pair the gate admits at epi_dist = t is a pair the search counts as
// an inlier at threshold t.  The numpy restatement is tests/fundamental_model.py (err_parts).
// And the squared Sampson distance shared by the essential-matrix search (vo_essential.hip: consensus and mask) and the pose from a
// homography (vo_hpose.hip: the vote of the points off the plane); oracle/essential_oracle.py and tests/hpose_model.py restate it.
#pragma once
#include "vo_internal.h"

// OpenCV's FMEstimatorCallback::computeError in float64: the larger of the two squared distances of a point to its epipolar line.
// -> true (and err) if both are within thr2; a NaN coordinate, or an epipolar line with a^2 + b^2 = 0 or a value that is not finite, is never an inlier
__device__ __forceinline__ bool f7_inlier(const double* F, double x, double y, double u, double v, double thr2, double& err) {
  const double a2 = (F[0] * x + F[1] * y) + F[2], b2 = (F[3] * x + F[4] * y) + F[5], c2 = (F[6] * x + F[7] * y) + F[8];
  const double s2 = 1.0 / (a2 * a2 + b2 * b2), d2 = (u * a2 + v * b2) + c2;
  const double a1 = (F[0] * u + F[3] * v) + F[6], b1 = (F[1] * u + F[4] * v) + F[7], c1 = (F[2] * u + F[5] * v) + F[8];
  const double s1 = 1.0 / (a1 * a1 + b1 * b1), d1 = (x * a1 + y * b1) + c1;
  const double e1 = (d1 * d1) * s1, e2 = (d2 * d2) * s2;
  err = e1 > e2 ? e1 : e2;
  return (e1 <= thr2) && (e2 <= thr2);
}

// squared Sampson distance of the normalised correspondence (x1, y1) <-> (x2, y2) to E
__device__ __forceinline__ double vo_sampson(const double* E, double x1, double y1, double x2, double y2) {
  const double a0 = E[0] * x1 + E[1] * y1 + E[2], a1 = E[3] * x1 + E[4] * y1 + E[5], a2 = E[6] * x1 + E[7] * y1 + E[8];   // E x1
  const double b0 = E[0] * x2 + E[3] * y2 + E[6], b1 = E[1] * x2 + E[4] * y2 + E[7];                                       // E^T x2
  const double num = x2 * a0 + y2 * a1 + a2;
  return num * num / (a0 * a0 + a1 * a1 + b0 * b0 + b1 * b1);
}
