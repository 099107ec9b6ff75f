// Bundle adjustment: what the translation units of the solver share -- vo_ba.hip (lane-per-observation and wave-private kernels, solve, host side)
// and vo_ba_factored.hip (the factored wave-private build / update).  Sizes, the pointer block of a launch, the workspace, the camera and loss
// helpers, the cross-lane sums on doubles and the LM decision; every function is inline, so a unit compiles exactly what it uses.
#pragma once
#include "vo_internal.h"

#include <math.h>
#include <type_traits>
#include <stdlib.h>
#include <string.h>

// (float64 against tolerances: a*b+c may fuse, see vo_ba.hip)
#pragma clang fp contract(fast)

#define BA_SOLVE_THREADS 1024
#define BA_AUX 18            // per landmark: Hll(6) gl(3) Cinv(6) z(3)
#define BA_POSE_VALS 28      // Hpp upper (21) + gp (6) + cost (1)
#define BA_MAX_SLOTS 20
#define BA_EVAL_VALS 4
#define BA_PITCH_PAD 8       // panel row pitch = RP + 8 doubles.  A pitch of RP + 16 keeps the 16-lane row groups of the MFMA operand reads on
                             // disjoint LDS banks, but its 30.7 KB panel lets only 4 workgroups share a CU; measured (vo_tuning.ba_pitch_pad): pads 0..12
                             // 54 us per launch, pad 16 57 us -- the bank conflicts cost nothing here, the fifth workgroup is worth 5 %
#define BA_CAM 21            // per-slot camera data staged in LDS: R(9) t(3) Jr(9)

typedef double d4 __attribute__((ext_vector_type(4)));

struct ba_info {            // written by k_ba_solve for the iteration
  double cost_cur, pred_pose, step2_pose, x2_pose, ginf;
  int chol_fail, pad;
};

struct ba_params_dev {
  double ftol, xtol, gtol, lambda0, lambda_min, delta;   // delta: scipy's f_scale C, for every loss
  int max_iters;
  int loss;                   // VO_LOSS_HUBER / _SOFT_L1 / _CAUCHY / _ARCTAN; selects the kernel set (ba_launch_iter).  VO_LOSS_LINEAR never reaches
                              // the device: it runs the Huber kernels with an unreachable knee (ba_dev_params)
};

struct ba_ptrs {
  const double* K; const double* obs; const double* x0;
  double* xa; double* xb;             // x[0] / x[1] (two named members: a dynamically indexed array would push the struct into scratch)
  double* aux; double* posepart; double* gmax; double* tiles; double* dp; double* evalpart;
  double* tilesum; double* posesum;   // k_ba_reduce outputs: n_tiles*256, W*28 + 1 (last = max |g_l|); ONE allocation per problem:
                                      // [tilesum | posesum | max|g_l| slot per rank] = the all-reduced packet of a sharded solve
  double* xstat;                      // sharded solve: [4] step statistics summed over all shards (every entry holds the total)
  double* cams;                       // [2][W][21]: R, t, Jr of the poses in x[0] / x[1] (written by k_ba_solve)
  ba_state* state; ba_info* info;
  unsigned long long* dbg;
  // per-problem strides (elements) of the batched buffers
  size_t s_obs, s_x, s_aux, s_posepart, s_gmax, s_tiles, s_dp, s_evalpart, s_tilesum, s_posesum, s_cams;
  int W, N, LPP, PPB, nblk, RP, RT, n_tiles, pitch;
  int nset;                           // partial sets (= workgroups of k_ba_build): nblk, or fewer when a workgroup walks several landmark chunks
  int cam_off;                        // k_ba_build: offset (doubles) of the staged cameras inside the dynamic LDS
  int sharded, rank, n_ranks, batch;  // sharded: the batch entries (x the ranks) are landmark shards of one problem
  int fold;                           // the solve sums the partial sets itself, no k_ba_reduce launch (small windows, unsharded: ba_make_ptrs)
  int n_eval;                         // entries of evalpart (= workgroups of k_ba_update)
  int* gdyn;                          // wave-private kernels: [2][batch] partial sets / statistics entries of a problem in iteration it & 1 (null: nset, n_eval)
  const int32_t* n_live; int s_nlive; // optional (closed loop): landmark slots [0, *n_live) of the problem are in use, the workgroups of the rest only zero
                                      // their partial sums (the tables of vo_pipeline.hip are sized for max_pts landmarks, a scene fills a part of them)
};

__device__ __forceinline__ double* ba_x(const ba_ptrs& P, int k) { return k ? P.xb : P.xa; }

// pointers of problem b of the batch
__device__ __forceinline__ ba_ptrs ba_select(ba_ptrs P, int b) {
  const size_t sb = (size_t)b;
  P.K += sb * 9; P.obs += sb * P.s_obs; P.x0 += sb * P.s_x; P.xa += sb * P.s_x; P.xb += sb * P.s_x;
  P.aux += sb * P.s_aux; P.posepart += sb * P.s_posepart; P.gmax += sb * P.s_gmax; P.tiles += sb * P.s_tiles;
  P.dp += sb * P.s_dp; P.evalpart += sb * P.s_evalpart; P.tilesum += sb * P.s_tilesum; P.posesum += sb * P.s_posesum; P.cams += sb * P.s_cams;
  P.xstat += sb * BA_EVAL_VALS;
  P.state += 2 * sb; P.info += sb;
  if (P.n_live) P.n_live += sb * P.s_nlive;
  if (b != 0) P.dbg = nullptr;
  return P;
}

struct vo_ba_ws {
  int W = 0, N = 0, LPP = 0, PPB = 0, nblk = 0, RP = 0, RT = 0, n_tiles = 0, pitch = 0, tpb = 0;
  int cap_W = 0, cap_N = 0;
  int cap_nblk = 0;             // partial sets the nblk-sized buffers (posepart, gmax, tiles, evalpart) were allocated for
  size_t build_lds = 0, solve_lds = 0;
  int cam_off = 0;
  vo_dev<double> d_K;           // 9
  double* d_obs = nullptr;      // W*N*2   } the problem a solve reads: d_obs_own / d_x0_own, or the selected problem of the bank
  double* d_x0 = nullptr;       // W*6 + N*3 } (d_bank_obs / d_bank_x0)
  vo_dev<double> d_obs_own, d_x0_own;
  vo_dev<double> d_x[2];
  vo_dev<double> d_aux;         // N * BA_AUX
  vo_dev<double> d_posepart;    // nblk * W * 28
  vo_dev<double> d_gmax;        // nblk
  vo_dev<double> d_tiles;       // nblk * n_tiles * 256
  vo_dev<double> d_dp;          // 6W
  vo_dev<double> d_evalpart;    // nblk * 4
  vo_dev<double> d_tilesum;     // n_tiles * 256                  } one allocation, red_stride doubles per problem:
  double* d_posesum = nullptr;  // W * 28 + 1 (+ 16 rank slots)    } d_posesum = d_tilesum + n_tiles * 256
  size_t red_stride = 0;
  vo_dev<double> d_xstat;       // [batch][4] sharded solve: summed step statistics
  vo_dev<double> d_gather;      // vo_ba_gather_points: send [batch][N][3] | recv [n_ranks][batch][N][3]; made and grown there
  vo_pinned<double> h_gather;   // pinned mirror of recv
  vo_dev<double> d_cams;        // 2 * W * 21
  vo_dev<double> d_S;           // probe: (6W)^2 + 6W
  vo_dev<double> d_Hpp;         // W*28 reduced pose values (probe)
  vo_dev<double> d_res;         // probe residual W*N
  vo_dev<double> d_dl;          // probe d_points 3N
  double* d_xout = nullptr;     // published solution 6W + 3N (points into d_pub)
  vo_dev<uint8_t> d_pub;        // [ba_state (64 B) | x]: what a fetch copies back in one go
  vo_pinned<uint8_t> h_pub;     // pinned mirror
  size_t pub_bytes = 0;
  vo_dev<ba_state> d_state;     // [2]
  vo_dev<ba_info> d_info;
  vo_pinned<ba_state> h_state;
  bool uploaded = false;
  // bank of resident problems (vo_ba_upload_bank): d_x0 / d_obs point at the selected one
  vo_dev<double> d_bank_x0, d_bank_obs;
  int bank_n = 0, bank_sel = 0;
  // wave-private kernels (vo_ba_wave.h): windows of <= 10 slots; v2 = 2: their factored form (vo_ba_factored.hip) where the loss allows it
  int v2 = 0, v2_rt = 0, v2_spl = 0, v2_lpp = 8;
  size_t v2_lds = 0;
  int v2_g0 = 1, v2_gcap = 1;       // workgroups per problem of a launch; the most a running problem is given once others have finished
  vo_dev<int> d_gdyn;               // [2][batch]
};

// ------------------------------------------------------------------------------------------------
// small device helpers
// ------------------------------------------------------------------------------------------------
// R (Rodrigues), t and the right Jacobian of SO(3) (R(r + dr) ~ R(r) Exp(Jr dr)) of one pose: 21 doubles, ONE sincos -- the trial
// cameras are on k_ba_solve's critical path, computed by W lanes
__device__ __forceinline__ void d_camera(const double* p, double* cam) {
  const double x = p[0], y = p[1], z = p[2];
  const double th2 = x * x + y * y + z * z;
  const double th = sqrt(th2);
  double sn, cs;
  sincos(th, &sn, &cs);
  double* R = cam;
  if (th < 2.220446049250313e-16) {
    R[0] = 1; R[1] = 0; R[2] = 0; R[3] = 0; R[4] = 1; R[5] = 0; R[6] = 0; R[7] = 0; R[8] = 1;
  } else {
    const double kx = x / th, ky = y / th, kz = z / th, c1 = 1.0 - cs;
    R[0] = cs + c1 * kx * kx;      R[1] = c1 * kx * ky - sn * kz; R[2] = c1 * kx * kz + sn * ky;
    R[3] = c1 * ky * kx + sn * kz; R[4] = cs + c1 * ky * ky;      R[5] = c1 * ky * kz - sn * kx;
    R[6] = c1 * kz * kx - sn * ky; R[7] = c1 * kz * ky + sn * kx; R[8] = cs + c1 * kz * kz;
  }
  cam[9] = p[3]; cam[10] = p[4]; cam[11] = p[5];
  double a, b;
  if (th2 < 1e-8) { a = 0.5 - th2 / 24.0; b = 1.0 / 6.0 - th2 / 120.0; }
  else { a = (1.0 - cs) / th2; b = (th - sn) / (th2 * th); }
  double* J = cam + 12;
  J[0] = 1.0 + b * (x * x - th2); J[1] = a * z + b * x * y;       J[2] = -a * y + b * x * z;
  J[3] = -a * z + b * y * x;      J[4] = 1.0 + b * (y * y - th2); J[5] = a * x + b * y * z;
  J[6] = a * y + b * z * x;       J[7] = -a * x + b * z * y;      J[8] = 1.0 + b * (z * z - th2);
}

__device__ __forceinline__ void stage_cameras(const double* poses, int W, double* cam, int tid, int nthreads) {
  for (int i = tid; i < W; i += nthreads) {
    const double* p = poses + 6 * i;
    double* c = cam + BA_CAM * i;
    d_camera(p, c);
  }
}

struct ba_obs_lin {
  double e0, e1, w, rho;
  double Jl[2][3];
  double Jp[2][6];
};

template <int LOSS>
__device__ __forceinline__ void ba_loss(double s, double delta, double d2, double id2, double& w, double& rho);

// residual + Jacobian blocks of one observation.  returns false if unobserved.
// Aout (optional, with WANT_JP = false): the 2 x 3 projection Jacobian d(u, v) / d(camera-frame point) -- with it the caller forms
// Jp d for a given step d without the 2 x 6 block (k_ba_update)
template <bool WANT_JP, int LOSS = VO_LOSS_HUBER>
__device__ __forceinline__ bool ba_linearize_obs(const double* __restrict__ K, const double* __restrict__ cam,
                                                 const double X[3], double uo, double vo, double delta, ba_obs_lin& o,
                                                 double (*Aout)[3] = nullptr) {
  if (uo != uo) return false;
  const double* R = cam; const double* t = cam + 9; const double* Jr = cam + 12;
  const double xc = R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0];
  const double yc = R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1];
  const double zc = R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2];
  const double p0 = K[0] * xc + K[1] * yc + K[2] * zc;
  const double p1 = K[3] * xc + K[4] * yc + K[5] * zc;
  const double p2 = K[6] * xc + K[7] * yc + K[8] * zc;
  const double ip2 = 1.0 / p2;
  const double u = p0 * ip2, v = p1 * ip2;
  o.e0 = u - uo; o.e1 = v - vo;
  const double s = o.e0 * o.e0 + o.e1 * o.e1;
  const double d2 = delta * delta;
  if constexpr (LOSS == VO_LOSS_HUBER) {
    if (s <= d2) { o.w = 1.0; o.rho = s; }
    else { const double rs = sqrt(s); o.w = delta / rs; o.rho = 2.0 * delta * rs - d2; }
  } else {
    ba_loss<LOSS>(s, delta, d2, 1.0 / d2, o.w, o.rho);
  }
  double A[2][3];
#pragma unroll
  for (int c = 0; c < 3; c++) { A[0][c] = (K[c] - u * K[6 + c]) * ip2; A[1][c] = (K[3 + c] - v * K[6 + c]) * ip2; }
  if (Aout) {
#pragma unroll
    for (int c = 0; c < 3; c++) { Aout[0][c] = A[0][c]; Aout[1][c] = A[1][c]; }
  }
#pragma unroll
  for (int k = 0; k < 2; k++)
#pragma unroll
    for (int c = 0; c < 3; c++) o.Jl[k][c] = A[k][0] * R[c] + A[k][1] * R[3 + c] + A[k][2] * R[6 + c];
  if (WANT_JP) {
    // M3 = [X]x Jr  (column c = X x Jr[:,c]);  Jp_rot = -Jl M3 ;  Jp_trans = A
    double M3[3][3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double a0 = Jr[c], a1 = Jr[3 + c], a2 = Jr[6 + c];
      M3[0][c] = X[1] * a2 - X[2] * a1;
      M3[1][c] = X[2] * a0 - X[0] * a2;
      M3[2][c] = X[0] * a1 - X[1] * a0;
    }
#pragma unroll
    for (int k = 0; k < 2; k++) {
#pragma unroll
      for (int c = 0; c < 3; c++)
        o.Jp[k][c] = -(o.Jl[k][0] * M3[0][c] + o.Jl[k][1] * M3[1][c] + o.Jl[k][2] * M3[2][c]);
#pragma unroll
      for (int c = 0; c < 3; c++) o.Jp[k][3 + c] = A[k][c];
    }
  }
  return true;
}

// ---- cross-lane helpers on doubles ----
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}

// v[l] + v[l ^ 16] in every lane: v_permlane16_swap (VALU, no LDS traffic).  swap(a, b) with a = b = v leaves
// a' = {row0, row0, row2, row2}, b' = {row1, row1, row3, row3}, so a' + b' is the pair sum everywhere.
__device__ __forceinline__ double xor16_sum(double v) {
  const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
  const auto l2 = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
  const auto h2 = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
  return __hiloint2double((int)h2[0], (int)l2[0]) + __hiloint2double((int)h2[1], (int)l2[1]);
}
// v[l] + v[l ^ 32] in every lane: v_permlane32_swap
__device__ __forceinline__ double xor32_sum(double v) {
  const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
  const auto l2 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto h2 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  return __hiloint2double((int)h2[0], (int)l2[0]) + __hiloint2double((int)h2[1], (int)l2[1]);
}

// Reduce-scatter forms of the two swaps: x and y are summed over lane pairs at once, half of the lanes keep x's sum, the other
// half y's -- 3 instructions for two values instead of 3 per value (the all-reduce forms above duplicate every sum).
//   rs16(x, y): rows 0 and 2 of the wave receive x[row] + x[row + 1], rows 1 and 3 receive y[row - 1] + y[row]
//   rs32(x, y): lanes 0..31 receive x[l] + x[l + 32], lanes 32..63 receive y[l - 32] + y[l]
__device__ __forceinline__ double rs16_sum(double x, double y) {
  const auto l2 = __builtin_amdgcn_permlane16_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
  const auto h2 = __builtin_amdgcn_permlane16_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
  return __hiloint2double((int)h2[0], (int)l2[0]) + __hiloint2double((int)h2[1], (int)l2[1]);
}
__device__ __forceinline__ double rs32_sum(double x, double y) {
  const auto l2 = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(x), (unsigned)__double2loint(y), false, false);
  const auto h2 = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(x), (unsigned)__double2hiint(y), false, false);
  return __hiloint2double((int)h2[0], (int)l2[0]) + __hiloint2double((int)h2[1], (int)l2[1]);
}

// sum over the LPP (16 or 32) lanes of a landmark group; every lane of the group gets the total
__device__ __forceinline__ double group_allreduce(double v, int lpp) {
  v += dpp_f64<0x128>(v);   // row_ror:8
  v += dpp_f64<0x124>(v);   // row_ror:4
  v += dpp_f64<0x122>(v);   // row_ror:2
  v += dpp_f64<0x121>(v);   // row_ror:1
  if (lpp == 32) v = xor16_sum(v);
  return v;
}

// the same over a group of 8 lanes (windows of <= 8 slots: twice the landmarks per wave): x[l] + x[7 - l] by row_half_mirror, then the two
// quad exchanges -- lanes 0..3 and 4..7 of the group hold the same four pair sums (mirrored), so both quads finish with the total
__device__ __forceinline__ double group8_allreduce(double v) {
  v += dpp_f64<0x141>(v);   // row_half_mirror
  v += dpp_f64<0xB1>(v);    // quad_perm [1, 0, 3, 2]
  v += dpp_f64<0x4E>(v);    // quad_perm [2, 3, 0, 1]
  return v;
}
template <int LPPC>
__device__ __forceinline__ double group_allreduce_t(double v, int lpp) { return LPPC == 8 ? group8_allreduce(v) : group_allreduce(v, lpp); }

//   rs8(x, y): lanes with bit 3 clear receive x[l] + x[l ^ 8], lanes with bit 3 set receive y[l ^ 8] + y[l]  (row_ror:8 = lane ^ 8 in a row)
__device__ __forceinline__ double rs8_sum(double x, double y, int lane) {
  const bool hi = (lane & 8) != 0;
  const double keep = hi ? y : x, send = hi ? x : y;
  return keep + dpp_f64<0x128>(send);
}

// sum over the 64 lanes of a wave, result in every lane
__device__ __forceinline__ double wave_allreduce(double v) {
  v += dpp_f64<0x128>(v);
  v += dpp_f64<0x124>(v);
  v += dpp_f64<0x122>(v);
  v += dpp_f64<0x121>(v);
  return xor32_sum(xor16_sum(v));
}

__device__ __forceinline__ double readlane_f64(double v, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}

// 1/sqrt(x) to double precision: v_rsq_f64 seed + two Newton steps
__device__ __forceinline__ double rsqrt_nr(double x) {
  double y = __builtin_amdgcn_rsq(x);
  double e = fma(-x * y, y, 1.0);
  y = fma(0.5 * y, e, y);
  e = fma(-x * y, y, 1.0);
  y = fma(0.5 * y, e, y);
  return y;
}

// reciprocal to double precision without the division's scaling / fix-up sequence (the operand is a depth times the focal scale, or 1 + z
// of a robust loss: far from the denormals and from overflow)
__device__ __forceinline__ double rcp_nr(double x) {
  double y = __builtin_amdgcn_rcp(x);
  double e = fma(-x, y, 1.0);
  y = fma(y, e, y);
  e = fma(-x, y, 1.0);
  y = fma(y, e, y);
  return y;
}

// log1p(z) and atan(z) for z >= 0, to a few units in the last place in a handful of registers: the math library's forms spill the
// accumulators of the build kernels (k_ba_build_w<4, 2, 5, cauchy> 56 B, <.., arctan> 140 B of scratch per lane).
//   log1p: 1 + z = 2^k m, m in [sqrt(1/2), sqrt(2)); log m = 2 atanh(f), f = (m - 1) / (m + 1), |f| <= 0.1716: the odd series to f^23
//          (the first term left out, (f^2)^12 / 25, is below 1e-19); the rounding of 1 + z is put back to first order, c = (z - (u - 1)) / u
//   atan:  z > 1 -> pi/2 - atan(1 / z); t > tan(pi/12) -> pi/6 + atan((sqrt(3) t - 1) / (t + sqrt(3))); |t| <= 0.268: the series to t^29
__device__ __forceinline__ double ba_log1p(double z) {
  const double u = 1.0 + z;
  const double c = (z - (u - 1.0)) * rcp_nr(u);
  int k;
  double m = frexp(u, &k);                               // u = m 2^k, m in [1/2, 1)
  const bool lo = m < 0.70710678118654752;
  m = lo ? 2.0 * m : m; k = lo ? k - 1 : k;
  const double f = (m - 1.0) * rcp_nr(m + 1.0), f2 = f * f;
  double p = 1.0 / 23.0;
  p = fma(p, f2, 1.0 / 21.0); p = fma(p, f2, 1.0 / 19.0); p = fma(p, f2, 1.0 / 17.0); p = fma(p, f2, 1.0 / 15.0); p = fma(p, f2, 1.0 / 13.0);
  p = fma(p, f2, 1.0 / 11.0); p = fma(p, f2, 1.0 / 9.0); p = fma(p, f2, 1.0 / 7.0); p = fma(p, f2, 1.0 / 5.0); p = fma(p, f2, 1.0 / 3.0);
  const double lm = fma(2.0 * f * f2, p, 2.0 * f);
  const double kd = (double)k;
  return fma(kd, 6.93147180369123816490e-01, lm + fma(kd, 1.90821492927058770002e-10, c));    // ln 2 = hi (exact times k) + lo
}
__device__ __forceinline__ double ba_atan(double z) {
  const bool inv = z > 1.0;
  double t = inv ? rcp_nr(z) : z;
  const bool red = t > 0.26794919243112270647;
  t = red ? (fma(t, 1.73205080756887729353, -1.0)) * rcp_nr(t + 1.73205080756887729353) : t;
  const double t2 = t * t;
  double p = -1.0 / 29.0;
  p = fma(p, t2, 1.0 / 27.0); p = fma(p, t2, -1.0 / 25.0); p = fma(p, t2, 1.0 / 23.0); p = fma(p, t2, -1.0 / 21.0); p = fma(p, t2, 1.0 / 19.0);
  p = fma(p, t2, -1.0 / 17.0); p = fma(p, t2, 1.0 / 15.0); p = fma(p, t2, -1.0 / 13.0); p = fma(p, t2, 1.0 / 11.0); p = fma(p, t2, -1.0 / 9.0);
  p = fma(p, t2, 1.0 / 7.0); p = fma(p, t2, -1.0 / 5.0); p = fma(p, t2, 1.0 / 3.0);
  double r = fma(-t * t2, p, t);
  r = red ? 0.52359877559829887308 + r : r;
  return inv ? 1.57079632679489661923 - r : r;
}

// IRLS weight w = rho'(z) and cost term C^2 rho(z) of one observation, scipy's losses with C = f_scale = delta, s = |e|^2, z = s / C^2
// (d2 = C^2, id2 = 1 / C^2); the cost is 1/2 sum C^2 rho(z).  s = 0 (an unobserved slot) gives w = 1, rho = 0 for every loss.
//   huber    z <= 1: z, w = 1;  else 2 sqrt(z) - 1, w = 1 / sqrt(z)     (the expressions the Huber kernels have always used)
//   soft_l1  2 (sqrt(1 + z) - 1) = 2 z / (sqrt(1 + z) + 1),  w = 1 / sqrt(1 + z)
//   cauchy   log1p(z),  w = 1 / (1 + z)
//   arctan   atan(z),   w = 1 / (1 + z^2)
// The weights come from v_rsq / v_rcp + Newton steps like the rest of the solver; log1p and atan (ba_log1p, ba_atan) feed the cost sums only.
// vo_ba_check_params keeps C in [VO_BA_F_SCALE_MIN, VO_BA_F_SCALE_MAX] for these losses (C^2 and 1 / C^2 finite and normal); z is still
// unbounded (a point close to a camera plane), so it is capped below inf (rsqrt_nr / rcp_nr of inf are NaN), and arctan's weight takes
// z <= ~2^511: every weight finite and >= 0, every cost term finite.
// The caps clamp the high word of z >= 0 as an unsigned integer: one v_min_u32 with a literal, where an f64 constant for v_min_f64 would
// take two scalar registers in every robust build / update kernel.
__device__ __forceinline__ double ba_cap_hi(double x, unsigned hi_max) {
  const unsigned hi = min((unsigned)__double2hiint(x), hi_max);
  return __hiloint2double((int)hi, __double2loint(x));
}
template <int LOSS>
__device__ __forceinline__ void ba_loss(double s, double delta, double d2, double id2, double& w, double& rho) {
  if constexpr (LOSS == VO_LOSS_HUBER) {
    const bool inl = s <= d2;
    const double irs = rsqrt_nr(inl ? 1.0 : s);          // 1 / |e| (outliers only)
    w = inl ? 1.0 : delta * irs;
    rho = inl ? s : 2.0 * delta * (s * irs) - d2;
  } else {
    const double z = ba_cap_hi(s * id2, 0x7FEFFFFFu), opz = 1.0 + z;     // (a residual far beyond f_scale: z ~ 1.8e308, not inf)
    if constexpr (LOSS == VO_LOSS_SOFT_L1) {
      w = rsqrt_nr(opz);
      rho = 2.0 * s * rcp_nr(fma(opz, w, 1.0));          // opz w = sqrt(1 + z)
    } else if constexpr (LOSS == VO_LOSS_CAUCHY) {
      w = rcp_nr(opz);
      rho = d2 * ba_log1p(z);
    } else {
      static_assert(LOSS == VO_LOSS_ARCTAN, "a robust loss");
      const double zw = ba_cap_hi(z, 0x5FE00000u);          // (z <= ~2^511, z^2 finite: w ~ 2^-1022 where 1 / (1 + z^2) is below it)
      w = rcp_nr(fma(zw, zw, 1.0));
      rho = d2 * ba_atan(z);
    }
  }
}

// ------------------------------------------------------------------------------------------------
// LM decision (inputs are identical in every workgroup, so every workgroup derives the same state)
// ------------------------------------------------------------------------------------------------
// fixed-order block reduction of the per-workgroup step statistics written by k_ba_update (4 values per workgroup): wave k sums
// statistic k -- lane l the workgroups l, l + 64, ... in order, then the fixed cross-lane tree of wave_allreduce -- so every caller
// derives bit-identical sums without staging anything in LDS (one barrier instead of three).  Call from all threads (TPB >= 256).
template <int TPB>
__device__ __forceinline__ void ba_reduce_evalpart(const double* __restrict__ evalpart, int n_eblk, double* s_sum /* 4 */) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (wave < BA_EVAL_VALS) {
    double s = 0;
    for (int b = lane; b < n_eblk; b += 64) s += evalpart[b * BA_EVAL_VALS + wave];
    s = wave_allreduce(s);
    if (lane == 0) s_sum[wave] = s;
  }
  __syncthreads();
}

__device__ inline void ba_decide(const ba_state& in, const ba_info& info, const double* __restrict__ sums,
                                 const ba_params_dev& prm, ba_state& out) {
  out = in;
  if (in.done) return;
  const double F = info.cost_cur;
  if (in.iter == 0) out.cost0 = F;
  out.cost = F;
  // a non-finite cost takes none of the convergence exits (the maxima behind ginf drop NaN: with every gradient entry NaN it arrives as 0);
  // its steps are rejected until the damping overflows (status 4)
  const bool fin = F - F == 0.0;
  if (fin && info.ginf < prm.gtol) { out.done = 1; out.status = 1; return; }
  const double Ft = sums[0], predp = sums[1], step2 = sums[2], x2 = sums[3];
  const double pred = 0.5 * (predp + info.pred_pose);
  const double step = sqrt(step2 + info.step2_pose), xn = sqrt(x2 + info.x2_pose);
  const bool ok = !info.chol_fail;
  const double rho = (ok && pred > 0) ? (F - Ft) / pred : -1.0;
  out.iter = in.iter + 1;
  if (ok && Ft < F && rho > 0) {
    out.cur = in.cur ^ 1;
    out.cost = Ft;
    out.accepted = in.accepted + 1;
    const double q = 2.0 * rho - 1.0;
    double f = 1.0 - q * q * q;
    if (f < 1.0 / 3.0) f = 1.0 / 3.0;
    double lam = in.lambda * f;
    if (lam < prm.lambda_min) lam = prm.lambda_min;
    out.lambda = lam; out.nu = 2.0;
    if ((F - Ft) < prm.ftol * Ft) { out.done = 1; out.status = 2; }
    else if (fin && step < prm.xtol * (prm.xtol + xn)) { out.done = 1; out.status = 3; }
  } else {
    if (ok && fin && step < prm.xtol * (prm.xtol + xn)) { out.done = 1; out.status = 3; }
    else {
      out.lambda = in.lambda * in.nu; out.nu = in.nu * 2.0;
      if (out.lambda > 1e12) { out.done = 1; out.status = 4; }
    }
  }
  if (!out.done && out.iter >= prm.max_iters) { out.done = 1; out.status = 0; }
}

__device__ inline ba_state ba_init_state(const ba_params_dev& prm) {
  ba_state s;
  s.lambda = prm.lambda0; s.nu = 2.0; s.cost = 0; s.cost0 = 0;
  s.cur = 0; s.iter = 0; s.accepted = 0; s.status = 0; s.done = 0; s.n_obs = 0;
  return s;
}
