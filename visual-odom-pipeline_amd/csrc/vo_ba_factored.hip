// Bundle adjustment, windows of 9 and 10 slots: the FACTORED form of the wave-private build / update kernels of vo_ba_wave.h.
//
// Same reference lines and algorithm as k_ba_build_w / k_ba_update_w, and for the build the SAME TEXT around pass 2: the geometry, the chunk
// prefetch, the camera staging, the observation, the landmark factor with its aux record and gmax, the Gram phase and the fold of the four waves
// are the shared phases of vo_ba_wave.h ("The phases of the wave walk"), called from both forms -- lane maps, partial-set layout and summation
// orders agree because they are defined once.  This file's own: the head (the text of k_ba_build_w's), pass 2 of the build, its rotation
// epilogue, and the update (k_ba_update_w's text with another Jp d_pose; its observations and its trial cost go through ba2_observe too).  What changes is where the per-CAMERA constants of the camera block
// are applied.  With
// Jl_k = a_k K R (row k of the landmark block) the camera block of an observation of slot s is
//     Jp_k = j_k^T T_s,   j_k = [X x Jl_k ; Jl_k],   T_s = blockdiag(Jr_s, R_s^T)
// -- the wave-private kernels multiply by Jr_s and form a_k K = Jl_k R_s^T once per OBSERVATION (5.12 M per launch at 256 x 2 000 x 10).
// Everything the build sums is a product of Jp, so it is summed here in the basis of j_k, from the observation's landmark block
//     P = w sum_k Jl_k Jl_k^T,   gamma = w sum_k Jl_k e_k      (pass 1 forms both anyway: their sums over the slots are H_ll and g_l)
// alone -- no Jacobian is formed a second time:
//     H^_s = sum_l [[ [X]x P [X]x^T, [X]x P ], [ P [X]x^T, P ]],   g^_s = sum_l [X x gamma ; gamma],
//     panel rows Y^ = [ [X]x Q ; Q ],  Q = P Cinv^T           (column 6 W, y = Cinv g_l, has no camera index)
// and T is applied ONCE per partial set, after the four waves' tiles and camera sums are added in LDS:
//     H_pp,s = T_s^T H^_s T_s,   g_p,s = T_s^T g^_s,   sum Y Y^T = TT^T (sum Y^ Y^^T) TT,  TT = blockdiag(T_1 .. T_W, 1).
// P.tiles and P.posepart then hold what k_ba_build_w stores (to float64 rounding), and k_ba_solve, k_ba_reduce and the probes read them as before.
// The update needs Jp_s d_pose_s only: it is Jl z with z = R_s^T d_trans + (Jr_s d_rot) x X, the two camera vectors formed once per camera
// while the cameras are staged.
//
// Huber / linear loss, the <4, 2, 5> geometry (5 lanes per landmark, two slots per lane); every other shape and loss keeps vo_ba_wave.h.
#include "vo_ba_factored.h"

#pragma clang fp contract(fast)

#include "vo_ba_wave.h"      // lane maps, group sums and the shared phases of the wave walk

#define BA3_CAM 18           // update: per window slot in LDS: K R (9), K t (3), R^T d_trans (3), Jr d_rot (3)

// X x v
__device__ __forceinline__ void ba3_cross(const double X[3], double v0, double v1, double v2, double& o0, double& o1, double& o2) {
  o0 = X[1] * v2 - X[2] * v1; o1 = X[2] * v0 - X[0] * v2; o2 = X[0] * v1 - X[1] * v0;
}

// out = Ti^T g Tj for 3 x 3 blocks, T row-major (T[b][a] = T[3 b + a])
__device__ __forceinline__ void ba3_rot3(const double* __restrict__ Ti, const double* __restrict__ Tj, const double g[3][3], double out[3][3]) {
  double tmp[3][3];
#pragma unroll
  for (int b = 0; b < 3; b++)
#pragma unroll
    for (int a = 0; a < 3; a++) tmp[b][a] = g[b][0] * Tj[a] + g[b][1] * Tj[3 + a] + g[b][2] * Tj[6 + a];
#pragma unroll
  for (int a = 0; a < 3; a++)
#pragma unroll
    for (int c = 0; c < 3; c++) out[a][c] = Ti[a] * tmp[0][c] + Ti[3 + a] * tmp[1][c] + Ti[6 + a] * tmp[2][c];
}

// element (a, b), a / 16 <= b / 16, of the symmetric 16 RT x 16 RT matrix kept as upper 16 x 16 tiles in the accumulator layout of
// v_mfma_f64_16x16x4 (col = lane & 15, row = (lane >> 4) + 4 reg): the index k_ba_solve reads
template <int RT>
__device__ __forceinline__ int ba3_tile_index(int a, int b) {
  const int ta = a >> 4, tb = b >> 4, ii = a & 15, jj = b & 15;
  return (ta * RT - (ta * (ta - 1)) / 2 + (tb - ta)) * 256 + ((ii & 3) * 16 + jj) * 4 + (ii >> 2);
}

// ------------------------------------------------------------------------------------------------
// k_ba_build_f
// ------------------------------------------------------------------------------------------------
// template arguments (ba2_geom), grid and partial sets as k_ba_build_w
template <int RT, int SPL, int LPP, int LOSS>
__global__ void __launch_bounds__(256, 2) k_ba_build_f(ba_ptrs Pall, ba_params_dev prm, int it, double probe_lambda, int G0, int Gcap) {
  using GEO = ba2_geom<RT, SPL, LPP>;
  constexpr int LPC = GEO::LPC, LEAD = GEO::LEAD, PITCH = GEO::PITCH, NT = GEO::NT, REGION = GEO::REGION, WMAX = GEO::WMAX, CAMV = GEO::CAMV, TPR = GEO::TPR;
  ba2_work wk = ba2_select_work<true>(Pall, it, G0, Gcap);
  wk.prob = ba2_uniform(wk.prob); wk.part = ba2_uniform(wk.part); wk.G = ba2_uniform(wk.G);
  if (wk.prob < 0) return;                   // (uniform) more workgroups than the running problems can use
  const ba_ptrs P = ba_select(Pall, wk.prob);
  const int part = wk.part, G = wk.G;
  extern __shared__ double dyn[];            // [4 waves][ROWS][PITCH] panels | [W][21] cameras
  double* const s_cam = dyn + 4 * REGION;
  __shared__ double s_gmax[4];
  __shared__ ba_state s_st;
  __shared__ double s_esum[4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int n_live = ba2_uniform(Pall.n_live ? *P.n_live : P.N);
  ba_state prev;
  ba_info inf;
  if (it > 0) {
    if (tid == 0) { prev = P.state[(it - 1) & 1]; inf = *P.info; }
    ba_reduce_evalpart<256>(P.sharded ? P.xstat : P.evalpart, P.sharded ? 1 : Pall.gdyn[((it - 1) & 1) * Pall.batch + wk.prob], s_esum);
  }
  if (tid == 0) {
    ba_state st;
    if (it == 0) st = ba_init_state(prm);
    else ba_decide(prev, inf, s_esum, prm, st);
    if (probe_lambda >= 0) st.lambda = probe_lambda;
    s_st = st;
    if (part == 0) { P.state[it & 1] = st; Pall.gdyn[(it & 1) * Pall.batch + wk.prob] = G; }
  }
  __syncthreads();
  ba_state st = s_st;
  st.done = ba2_uniform(st.done); st.cur = ba2_uniform(st.cur); st.lambda = ba2_uniform(st.lambda);
  if (st.done) return;
  unsigned long long* dbgb = (blockIdx.x == 0 && P.dbg) ? P.dbg + 16 : nullptr;
  VO_STAMP(dbgb, 0);
  const int W = P.W, N = P.N;
  const double* poses = (it == 0) ? P.x0 : ba_x(P, st.cur);
  const double* pts = poses + 6 * W;
  const ba2_map<LPP> mp(lane);
  const int pl = mp.pl, q = mp.q;
  const int lead4 = 4 * (lane - q + LEAD);        // (LPP = 5) ds_bpermute source: the leader of this lane's group
  const int nchunk = (N + LPC - 1) / LPC;
  const int nchunk_live = min(nchunk, (n_live + LPC - 1) / LPC);
  const bool seed_x = it == 0;
  double* const pan = dyn + wave * REGION;
  d4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) acc[t] = d4{0.0, 0.0, 0.0, 0.0};
  double camacc[7 * SPL];
#pragma unroll
  for (int t = 0; t < 7 * SPL; t++) camacc[t] = 0.0;
  double gm = 0.0;
  const double lam = st.lambda;
  const ba2_scale sc = ba2_loss_scale<LOSS>(prm.delta);
  double Xn[3], uon[SPL], von[SPL];
  const ba2_fetch<SPL, LPP> fetch{P, pts, mp, pl, q, W, N, nchunk, nchunk_live, Xn, uon, von};     // (references, in the order of ba2_fetch's members)
  fetch(part * 4 + wave);
  ba2_stage_build<GEO>(P, st, it, part, poses, dyn);      // (Jr waits in LDS for the epilogue)
  __syncthreads();
  int nwalk = 0;
#pragma unroll 1
  for (int chunk = part * 4 + wave; chunk < nchunk; chunk += 4 * G) {
    const int j = chunk * LPC + pl;
    const bool inr = j < N && !mp.idle;
    if (nwalk == 2) VO_STAMP(dbgb, 1);   // (diagnostic stamps 1..4: the third chunk of the walk, steady state)
    const double X[3] = {Xn[0], Xn[1], Xn[2]};
    double uo[SPL], vo[SPL];
#pragma unroll
    for (int i = 0; i < SPL; i++) { uo[i] = uon[i]; vo[i] = von[i]; }
    if (seed_x && q == LEAD && inr) { double* dst = P.xa + 6 * W + 3 * j; dst[0] = X[0]; dst[1] = X[1]; dst[2] = X[2]; }
    if (chunk >= nchunk_live) { fetch(chunk + 4 * G); continue; }      // (wave-uniform) an unused part of the table: only x[0] is seeded
    // ---- pass 1: residual, weight and landmark block of this lane's observations; landmark sums over its slots.  Pass 2 needs the slot's own
    //      landmark block and nothing else: P (6), gamma (3) and rho are kept per slot ----
    double kP[SPL][6], kg[SPL][3], krho[SPL];
    double h[6] = {0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0};
#pragma unroll
    for (int i = 0; i < SPL; i++) {
      const int s = min(q + LPP * i, W - 1);      // (a lane without an i-th slot computes zeros on a valid camera)
      ba2_obs o;
      ba2_observe<LOSS>(s_cam + BA2_CAM * s, X, uo[i], vo[i], sc, o);
      krho[i] = o.rho;
      const double* l0 = o.Jl[0];
      const double* l1 = o.Jl[1];
      const double wl0[3] = {o.w * l0[0], o.w * l0[1], o.w * l0[2]};
      const double wl1[3] = {o.w * l1[0], o.w * l1[1], o.w * l1[2]};
      kP[i][0] = wl0[0] * l0[0] + wl1[0] * l1[0];
      kP[i][1] = wl0[1] * l0[0] + wl1[1] * l1[0];
      kP[i][2] = wl0[1] * l0[1] + wl1[1] * l1[1];
      kP[i][3] = wl0[2] * l0[0] + wl1[2] * l1[0];
      kP[i][4] = wl0[2] * l0[1] + wl1[2] * l1[1];
      kP[i][5] = wl0[2] * l0[2] + wl1[2] * l1[2];
      kg[i][0] = wl0[0] * o.e0 + wl1[0] * o.e1;
      kg[i][1] = wl0[1] * o.e0 + wl1[1] * o.e1;
      kg[i][2] = wl0[2] * o.e0 + wl1[2] * o.e1;
#pragma unroll
      for (int k = 0; k < 6; k++) h[k] += kP[i][k];
#pragma unroll
      for (int k = 0; k < 3; k++) g[k] += kg[i][k];
    }
    double ci[6], y[3];
    gm = ba2_factor_landmark<LPP>(h, g, lam, P.aux, j, inr, q == LEAD, lead4, dbgb, nwalk, gm, ci, y);
    const double i00 = ci[0], i10 = ci[1], i11 = ci[2], i20 = ci[3], i21 = ci[4], i22 = ci[5];
    // ---- pass 2, slot by slot, in the basis of j_k = [X x Jl_k ; Jl_k]: the slot's camera sums from M = [X]x P, M [X]x^T, P, X x gamma, gamma;
    //      the landmark's panel rows [X]x Q, Q with Q = P Cinv^T;  column 6 W = y ----
    double* const rw0 = pan + (3 * pl) * PITCH;
    double* const rw1 = rw0 + PITCH;
    double* const rw2 = rw1 + PITCH;
#pragma unroll
    for (int i = 0; i < SPL; i++) {
      const int sr = q + LPP * i;
      const double Ps[3][3] = {{kP[i][0], kP[i][1], kP[i][3]}, {kP[i][1], kP[i][2], kP[i][4]}, {kP[i][3], kP[i][4], kP[i][5]}};
      double M[3][3];      // [X]x P: column b = X x P[:, b]
#pragma unroll
      for (int b = 0; b < 3; b++) ba3_cross(X, Ps[0][b], Ps[1][b], Ps[2][b], M[0][b], M[1][b], M[2][b]);
      // M [X]x^T: row i = X x M[i, :]  (symmetric: the upper six)
      const double rr00 = X[1] * M[0][2] - X[2] * M[0][1], rr01 = X[2] * M[0][0] - X[0] * M[0][2], rr02 = X[0] * M[0][1] - X[1] * M[0][0];
      const double rr11 = X[2] * M[1][0] - X[0] * M[1][2], rr12 = X[0] * M[1][1] - X[1] * M[1][0];
      const double rr22 = X[0] * M[2][1] - X[1] * M[2][0];
      double xg[3];
      ba3_cross(X, kg[i][0], kg[i][1], kg[i][2], xg[0], xg[1], xg[2]);
      // camera sums of the slot: 28 values (21 of the upper H^, 6 of g^, the cost) four at a time through two reduce-scatter stages over
      // the landmark bits 5 and 4 of the lane index, as in k_ba_build_w
      const double term[28] = {rr00, rr01, rr02, M[0][0], M[0][1], M[0][2], rr11, rr12, M[1][0], M[1][1], M[1][2], rr22, M[2][0], M[2][1], M[2][2],
                               Ps[0][0], Ps[0][1], Ps[0][2], Ps[1][1], Ps[1][2], Ps[2][2], xg[0], xg[1], xg[2], kg[i][0], kg[i][1], kg[i][2],
                               LOSS == VO_LOSS_HUBER ? 0.5 * krho[i] : 0.0};
#pragma unroll
      for (int n = 0; n < 7; n++) {
        camacc[7 * i + n] += rs16_sum(rs32_sum(term[4 * n], term[4 * n + 1]), rs32_sum(term[4 * n + 2], term[4 * n + 3]));
        asm volatile("" : "+v"(camacc[7 * i + n]));      // (the sum is taken here, not carried through the Gram phase: see k_ba_build_w)
      }
      if (sr < W && !mp.idle) {
        double Q[3][3], XQ[3][3];
#pragma unroll
        for (int b = 0; b < 3; b++) {
          Q[b][0] = Ps[b][0] * i00;
          Q[b][1] = Ps[b][0] * i10 + Ps[b][1] * i11;
          Q[b][2] = Ps[b][0] * i20 + Ps[b][1] * i21 + Ps[b][2] * i22;
        }
#pragma unroll
        for (int c = 0; c < 3; c++) ba3_cross(X, Q[0][c], Q[1][c], Q[2][c], XQ[0][c], XQ[1][c], XQ[2][c]);
        double* const rw[3] = {rw0, rw1, rw2};
#pragma unroll
        for (int c = 0; c < 3; c++) {
          *reinterpret_cast<double2*>(rw[c] + 6 * sr) = make_double2(XQ[0][c], XQ[1][c]);
          *reinterpret_cast<double2*>(rw[c] + 6 * sr + 2) = make_double2(XQ[2][c], Q[0][c]);
          *reinterpret_cast<double2*>(rw[c] + 6 * sr + 4) = make_double2(Q[1][c], Q[2][c]);
        }
      }
    }
    if (q == LEAD && !mp.idle) { rw0[6 * W] = inr ? y[0] : 0.0; rw1[6 * W] = inr ? y[1] : 0.0; rw2[6 * W] = inr ? y[2] : 0.0; }
    __builtin_amdgcn_wave_barrier();
    if (nwalk == 2) VO_STAMP(dbgb, 3);   // first chunk: pass 2, panel written
    fetch(chunk + 4 * G);
    ba2_gram<GEO, RT>(pan, lane, acc);
    __builtin_amdgcn_wave_barrier();
    if (nwalk == 2) VO_STAMP(dbgb, 4);
    nwalk++;   // first chunk: Gram
  }
  VO_STAMP(dbgb, 5);   // walk
  // R of this lane's camera for the rotation at the end (only K R was staged): requested here, in flight while the waves fold their sums
  double Rc[9];
  if (tid < W) {
    if (it == 0) {
      double c[BA_CAM];
      d_camera(poses + 6 * tid, c);      // (iteration 0 only: cams[0] is being written by part 0 and may not be read here)
#pragma unroll
      for (int k = 0; k < 9; k++) Rc[k] = c[k];
    } else {
      const double* cg = P.cams + ((size_t)st.cur * W + tid) * BA_CAM;
#pragma unroll
      for (int k = 0; k < 9; k++) Rc[k] = cg[k];
    }
  }
  // ---- after the walk: the landmark bits the chunk stages left, then the four waves' sums through LDS in wave order ----
  ba2_finish_walk<GEO, SPL, LPP>(camacc, gm, mp, W, lane, pan, s_gmax + wave);
  constexpr int NCS = (CAMV + 255) / 256;                    // camera sums a lane folds
  // the folded set stays in registers (a lane: element tid of every tile, camera sums tid and tid + 256) until every round has been read
  double fsum[NT], csum[NCS];
#pragma unroll
  for (int t0 = 0; t0 < NT; t0 += TPR) {
    ba2_tiles_to_lds<GEO>(acc, pan, lane, t0);
#pragma unroll
    for (int t = t0; t < NT && t < t0 + TPR; t++) fsum[t] = ba2_fold4<GEO>(dyn, (t - t0) * 256 + tid);
    if (t0 == 0) {
#pragma unroll
      for (int k = 0; k < NCS; k++) csum[k] = ba2_fold4<GEO>(dyn, TPR * 256 + min(tid + 256 * k, CAMV - 1));
    }
  }
  __syncthreads();                                          // the last round has been read: the panels' LDS is free
  // ---- back to the pose basis, once per partial set: [NT tiles | W x 28 camera sums | 2 W blocks of T] in LDS ----
  double* const f_cam = dyn + NT * 256;
  double* const f_T = f_cam + CAMV;                         // block 2 s: Jr_s, block 2 s + 1: R_s^T, row-major
  static_assert(NT * 256 + CAMV + 18 * WMAX <= 4 * REGION, "the folded set and the rotations fit the panels' LDS");
#pragma unroll
  for (int t = 0; t < NT; t++) dyn[t * 256 + tid] = fsum[t];
#pragma unroll
  for (int k = 0; k < NCS; k++) if (tid + 256 * k < W * BA_POSE_VALS) f_cam[tid + 256 * k] = csum[k];
  if (tid < W) {
#pragma unroll
    for (int b = 0; b < 3; b++)
#pragma unroll
      for (int a = 0; a < 3; a++) {
        f_T[18 * tid + 3 * b + a] = s_cam[BA2_CAM * tid + 12 + 3 * b + a];
        f_T[18 * tid + 9 + 3 * b + a] = Rc[3 * a + b];
      }
  }
  __syncthreads();
  const int n6 = 6 * W, nb = 2 * W, npair = nb * (nb + 1) / 2;
  double* const out = P.tiles + (size_t)part * NT * 256;
  // what carries no camera index: the padding rows and columns (zeros) and y^T y
  {
    const int r = (tid >> 6) + 4 * (tid & 3), cc = (tid >> 2) & 15;
    int t = 0;
#pragma unroll
    for (int ta = 0; ta < RT; ta++)
#pragma unroll
      for (int tb = ta; tb < RT; tb++, t++) {
        const int gr = 16 * ta + r, gc = 16 * tb + cc;
        if (gr > n6 || gc > n6 || (gr == n6 && gc == n6)) out[t * 256 + tid] = fsum[t];
      }
  }
  // element (ga, gb), ga <= gb, and its mirror inside a diagonal tile
  auto put = [&](int ga, int gb, double v) {
    out[ba3_tile_index<RT>(ga, gb)] = v;
    if ((ga >> 4) == (gb >> 4) && ga != gb) out[ba3_tile_index<RT>(gb, ga)] = v;
  };
  if (tid < npair) {                                        // 3 x 3 block (I, J), I <= J, of the camera columns: T_I^T G T_J
    int I = 0, r = tid;
    while (r >= nb - I) { r -= nb - I; I++; }
    const int J = I + r;
    double g[3][3], o[3][3];
#pragma unroll
    for (int b = 0; b < 3; b++)
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const int ga = 3 * I + b, gb = 3 * J + a;
        g[b][a] = dyn[ba3_tile_index<RT>(min(ga, gb), max(ga, gb))];
      }
    ba3_rot3(f_T + 9 * I, f_T + 9 * J, g, o);
#pragma unroll
    for (int b = 0; b < 3; b++)
#pragma unroll
      for (int a = 0; a < 3; a++)
        if (I != J || b <= a) put(3 * I + b, 3 * J + a, o[b][a]);
  } else if (tid < npair + nb) {                            // column 6 W (r = sum Y y): T_I^T of its three entries
    const int I = tid - npair;
    const double* T = f_T + 9 * I;
    const double v0 = dyn[ba3_tile_index<RT>(3 * I, n6)], v1 = dyn[ba3_tile_index<RT>(3 * I + 1, n6)], v2 = dyn[ba3_tile_index<RT>(3 * I + 2, n6)];
#pragma unroll
    for (int a = 0; a < 3; a++) put(3 * I + a, n6, T[a] * v0 + T[3 + a] * v1 + T[6 + a] * v2);
  } else if (tid < npair + nb + W) {                        // camera sums of slot s: T_s^T H^_s T_s (upper-packed), T_s^T g^_s, the cost
    const int s = tid - npair - nb;
    const double* h = f_cam + s * BA_POSE_VALS;
    double* po = P.posepart + (size_t)part * W * BA_POSE_VALS + s * BA_POSE_VALS;
    constexpr int UP[6][6] = {{0, 1, 2, 3, 4, 5}, {1, 6, 7, 8, 9, 10}, {2, 7, 11, 12, 13, 14}, {3, 8, 12, 15, 16, 17}, {4, 9, 13, 16, 18, 19}, {5, 10, 14, 17, 19, 20}};
#pragma unroll
    for (int bi = 0; bi < 2; bi++)
#pragma unroll
      for (int bj = bi; bj < 2; bj++) {
        double g[3][3], o[3][3];
#pragma unroll
        for (int b = 0; b < 3; b++)
#pragma unroll
          for (int a = 0; a < 3; a++) g[b][a] = h[UP[3 * bi + b][3 * bj + a]];
        ba3_rot3(f_T + 18 * s + 9 * bi, f_T + 18 * s + 9 * bj, g, o);
#pragma unroll
        for (int b = 0; b < 3; b++)
#pragma unroll
          for (int a = 0; a < 3; a++)
            if (bi != bj || b <= a) po[UP[3 * bi + b][3 * bj + a]] = o[b][a];
      }
#pragma unroll
    for (int bi = 0; bi < 2; bi++) {
      const double* T = f_T + 18 * s + 9 * bi;
      const double v0 = h[21 + 3 * bi], v1 = h[22 + 3 * bi], v2 = h[23 + 3 * bi];
#pragma unroll
      for (int a = 0; a < 3; a++) po[21 + 3 * bi + a] = T[a] * v0 + T[3 + a] * v1 + T[6 + a] * v2;
    }
    po[27] = h[27];
  }
  if (tid == 0) P.gmax[part] = fmax(fmax(s_gmax[0], s_gmax[1]), fmax(s_gmax[2], s_gmax[3]));
  VO_STAMP(dbgb, 6);
}

// ------------------------------------------------------------------------------------------------
// k_ba_update_f : k_ba_update_w with Jp d_pose = Jl z, z = R^T d_trans + (Jr d_rot) x X
// ------------------------------------------------------------------------------------------------
// grid (G0 * batch), 256 lanes, the same assignment as k_ba_build_f of the iteration; step statistics: one entry of evalpart per part
template <int SPL, int LPP, int LOSS>
__global__ void __launch_bounds__(256, 2) k_ba_update_f(ba_ptrs Pall, ba_params_dev prm, int it, double* __restrict__ probe_dl, int G0, int Gcap) {
  constexpr int LPC = ba2_map<LPP>::LPC, LEAD = ba2_map<LPP>::LEAD;
  ba2_work wk = ba2_select_work<false>(Pall, it, G0, Gcap);
  wk.prob = ba2_uniform(wk.prob); wk.part = ba2_uniform(wk.part); wk.G = ba2_uniform(wk.G);
  if (wk.prob < 0) return;
  const ba_ptrs P = ba_select(Pall, wk.prob);
  const int part = wk.part, G = wk.G;
  if (wk.prob != 0) probe_dl = nullptr;
  __shared__ double s_cam[BA3_CAM * 10];            // current poses: K R, K t, R^T d_trans, Jr d_rot (windows of <= 10 slots)
  __shared__ double s_camt[12 * 10];                // trial poses: K R, K t
  __shared__ double s_red[4 * BA_EVAL_VALS];
  const ba_state st = P.state[it & 1];       // (a scalar load: P is uniform now)
  if (st.done) return;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, W = P.W, N = P.N;
  const double* poses = ba_x(P, st.cur);
  const double* pts = poses + 6 * W;
  double* tposes = ba_x(P, st.cur ^ 1);
  double* tpts = tposes + 6 * W;
  if (tid < W) {
    const double* cc = P.cams + ((size_t)st.cur * W + tid) * BA_CAM;          // current poses (k_ba_build it == 0 / k_ba_solve)
    const double* ct = P.cams + ((size_t)(st.cur ^ 1) * W + tid) * BA_CAM;    // trial poses (k_ba_solve of this iteration)
    double c[BA_CAM], t[BA2_CAM], d[6];
#pragma unroll
    for (int k = 0; k < BA_CAM; k++) c[k] = cc[k];
#pragma unroll
    for (int k = 0; k < 6; k++) d[k] = P.dp[6 * tid + k];
    ba2_stage_camera(P.K, c, t);
    double* dst = s_cam + BA3_CAM * tid;
#pragma unroll
    for (int k = 0; k < 12; k++) dst[k] = t[k];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      dst[12 + k] = c[k] * d[3] + c[3 + k] * d[4] + c[6 + k] * d[5];                  // R^T d_trans
      dst[15 + k] = c[12 + 3 * k] * d[0] + c[13 + 3 * k] * d[1] + c[14 + 3 * k] * d[2];   // Jr d_rot
    }
#pragma unroll
    for (int k = 0; k < 12; k++) c[k] = ct[k];
    ba2_stage_camera(P.K, c, t);
#pragma unroll
    for (int k = 0; k < 12; k++) s_camt[12 * tid + k] = t[k];
  }
  if (part == 0) for (int a = tid; a < 6 * W; a += 256) tposes[a] = poses[a] + P.dp[a];
  __syncthreads();
  const ba2_map<LPP> mp(lane);
  const int pl = mp.pl, q = mp.q;
  const int lead4 = 4 * (lane - q + LEAD);
  const int nchunk = (N + LPC - 1) / LPC;
  const int n_live = ba2_uniform(P.n_live ? *P.n_live : N);
  const int nchunk_live = min(nchunk, (n_live + LPC - 1) / LPC);
  const double lam = st.lambda, delta = prm.delta, d2 = delta * delta;
  const double id2 = LOSS == VO_LOSS_HUBER ? 0.0 : 1.0 / d2;
  const ba2_scale sc{delta, d2, id2};
  double e0 = 0, e1 = 0, e2 = 0, e3 = 0;
#pragma unroll 1
  for (int chunk = part * 4 + wave; chunk < nchunk_live; chunk += 4 * G) {
    const int j = chunk * LPC + pl;
    const bool inr = j < N && !mp.idle;
    double X[3] = {0.0, 0.0, 0.0};
    if (inr) { X[0] = pts[3 * j]; X[1] = pts[3 * j + 1]; X[2] = pts[3 * j + 2]; }
    double uo[SPL], vo[SPL];
#pragma unroll
    for (int i = 0; i < SPL; i++) {
      const int s = q + LPP * i;
      uo[i] = __builtin_nan(""); vo[i] = 0.0;
      if (s < W && inr) { const double2 ob = *reinterpret_cast<const double2*>(P.obs + ((size_t)s * N + j) * 2); uo[i] = ob.x; vo[i] = ob.y; }
    }
    double ax[15];
    if (inr) {
      const double* axp = P.aux + (size_t)j * BA_AUX;
#pragma unroll
      for (int k = 0; k < 15; k++) ax[k] = axp[k];
    } else {
#pragma unroll
      for (int k = 0; k < 15; k++) ax[k] = 0.0;
    }
    // B^T d_pose = sum over the slots of w Jl^T (Jl z)
    double v0 = 0, v1 = 0, v2 = 0;
#pragma unroll
    for (int i = 0; i < SPL; i++) {
      const int s = min(q + LPP * i, W - 1);
      const double* cam = s_cam + BA3_CAM * s;
      ba2_obs o;
      ba2_observe<LOSS>(cam, X, uo[i], vo[i], sc, o);
      const double w = o.w;
      const double* l0 = o.Jl[0];
      const double* l1 = o.Jl[1];
      const double z0 = cam[12] + (cam[16] * X[2] - cam[17] * X[1]);
      const double z1 = cam[13] + (cam[17] * X[0] - cam[15] * X[2]);
      const double z2 = cam[14] + (cam[15] * X[1] - cam[16] * X[0]);
      const double q0 = w * (l0[0] * z0 + l0[1] * z1 + l0[2] * z2), q1 = w * (l1[0] * z0 + l1[1] * z1 + l1[2] * z2);
      v0 += l0[0] * q0 + l1[0] * q1;
      v1 += l0[1] * q0 + l1[1] * q1;
      v2 += l0[2] * q0 + l1[2] * q1;
    }
    v0 = ba2_from_leader<LPP>(ba2_group_sum<LPP>(v0), lead4); v1 = ba2_from_leader<LPP>(ba2_group_sum<LPP>(v1), lead4);
    v2 = ba2_from_leader<LPP>(ba2_group_sum<LPP>(v2), lead4);
    const double w0 = ax[6] + v0, w1 = ax[7] + v1, w2 = ax[8] + v2;
    const double i00 = ax[9], i10 = ax[10], i11 = ax[11], i20 = ax[12], i21 = ax[13], i22 = ax[14];
    const double t0 = i00 * w0, t1 = i10 * w0 + i11 * w1, t2 = i20 * w0 + i21 * w1 + i22 * w2;   // Cinv u
    const double dl0 = -(i00 * t0 + i10 * t1 + i20 * t2), dl1 = -(i11 * t1 + i21 * t2), dl2 = -(i22 * t2);
    const double Xt[3] = {X[0] + dl0, X[1] + dl1, X[2] + dl2};
#pragma unroll
    for (int i = 0; i < SPL; i++) {
      const int s = min(q + LPP * i, W - 1);
      ba2_obs o;      // (only rho is used: the trial cost)
      ba2_observe<LOSS>(s_camt + 12 * s, Xt, uo[i], vo[i], sc, o);
      e0 += 0.5 * o.rho;
    }
    if (q == LEAD && inr) {
      tpts[3 * j] = Xt[0]; tpts[3 * j + 1] = Xt[1]; tpts[3 * j + 2] = Xt[2];
      if (probe_dl) { probe_dl[3 * j] = dl0; probe_dl[3 * j + 1] = dl1; probe_dl[3 * j + 2] = dl2; }
      e1 += lam * (fmax(ax[0], 1e-12) * dl0 * dl0 + fmax(ax[2], 1e-12) * dl1 * dl1 + fmax(ax[5], 1e-12) * dl2 * dl2)
            - (ax[6] * dl0 + ax[7] * dl1 + ax[8] * dl2);
      e2 += dl0 * dl0 + dl1 * dl1 + dl2 * dl2;
      e3 += X[0] * X[0] + X[1] * X[1] + X[2] * X[2];
    }
  }
  // four wave-wide sums as a reduce-scatter (k_ba_update_w)
  {
    double u = rs16_sum(rs32_sum(e0, e1), rs32_sum(e2, e3));
    u += dpp_f64<0x128>(u); u += dpp_f64<0x124>(u); u += dpp_f64<0x122>(u); u += dpp_f64<0x121>(u);   // row_ror 8, 4, 2, 1
    if ((lane & 15) == 0) {
      const int r = lane >> 4;
      s_red[wave * 4 + ((r & 1) ? (r == 1 ? 2 : 3) : (r == 0 ? 0 : 1))] = u;
    }
  }
  __syncthreads();
  if (tid < BA_EVAL_VALS) P.evalpart[part * BA_EVAL_VALS + tid] = (s_red[tid] + s_red[4 + tid]) + (s_red[8 + tid] + s_red[12 + tid]);
}

// ---- launchers ----
void vo_ba_f_launch_build(dim3 grid, size_t lds, hipStream_t q, const ba_ptrs& P, const ba_params_dev& prm, int it, double probe_lambda, int G0, int Gcap) {
  hipLaunchKernelGGL((k_ba_build_f<4, 2, 5, VO_LOSS_HUBER>), grid, dim3(256), lds, q, P, prm, it, probe_lambda, G0, Gcap);
}
void vo_ba_f_launch_update(dim3 grid, hipStream_t q, const ba_ptrs& P, const ba_params_dev& prm, int it, double* probe_dl, int G0, int Gcap) {
  hipLaunchKernelGGL((k_ba_update_f<2, 5, VO_LOSS_HUBER>), grid, dim3(256), 0, q, P, prm, it, probe_dl, G0, Gcap);
}
hipError_t vo_ba_f_set_lds_limits() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(k_ba_build_f<4, 2, 5, VO_LOSS_HUBER>), hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
}
