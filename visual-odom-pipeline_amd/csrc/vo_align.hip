// Sparse direct image alignment: the 6-DoF pose of the current frame of the store against the previous one, straight from the two pyramids
// and n 3-D points given in the previous camera's coordinates -- before any feature is tracked.  The first stage of semi-direct VO (Forster,
// Pizzoli, Scaramuzza: SVO, ICRA 2014, IV-A): 4 x 4 patches around the projected points, photometric error, inverse-compositional
// Gauss-Newton with Huber weights, coarse to fine.  The algorithm is defined by tests/align_model.py and stated in include/vo_mi355x.h.
//
// k_align_level: one workgroup of 256 threads per sequence runs a whole level in one launch, the iteration loop inside the kernel (as
// k_ba_solve and k_pnp_refine do); the host launches it once per level, coarse to fine, and the pose travels in the sequence's al_state.
//   lanes      sixteen lanes serve one point, one lane per patch pixel: a wave holds four points, the workgroup sixteen per round
//   per pixel  float32: the bilinear samples, the central-difference gradient, the residual, the Huber weight and the six products
//              w gx gx, w gx gy, w gy gy, w gx r, w gy r, w r r
//   per point  the sixteen-lane sums of those six by DPP row rotations (a DPP row is sixteen lanes; 8, 4, 2, 1: a fixed order, no LDS);
//              the row's first lane turns them into the point's share of the 21 + 6 + 3 sums in float64:
//              H += J_p^T G J_p, b += J_p^T e, sum w r^2, the count, sum of depths
//   per pass   vo_block_sum (vo_twoview.h) over the 256 threads in float64, a fixed order; every thread reads the totals and takes the
//              same decisions; thread 0 solves H xi = b (vo_chol6.h) and moves the pose
// The reference patch and its gradients do not fit in registers at max_pts points.  Two forms, the same bits: AL_FORM_WS keeps them in a
// workspace [batch][cap][16][3] f32 that the level's set-up pass writes (each thread re-reads what it wrote itself: no barrier), and
// AL_FORM_RECOMPUTE samples the previous level again in every pass.  The rule and its measurement: EXPERIMENTS.md.
// Reads of the padded store need no border branches: a point is used only where its whole footprint (patch, gradient stencil and the
// bilinear neighbour: 3 pixels to the left and above, 3 to the right and below of floor(u)) lies inside the level, and a point that is not
// used samples at (8, 8), which the 32-pixel border keeps inside the allocation at any level size.
#include "vo_internal.h"
#include "vo_twoview.h"
#include "vo_chol6.h"

#include <math.h>
#include <string.h>

enum { AL_FORM_WS = 1, AL_FORM_RECOMPUTE = 2 };
#define AL_FORM_RULE AL_FORM_WS
#define AL_SAFE 8.0                    // where a point that is not used samples

// per sequence: intrinsics, the pose that travels from level to level, what the finest level that ran left
struct al_state {
  double fx, fy, cx, cy;               // level 0
  double R[9], t[3];
  double chi, zbar;
  int32_t n_used, levels_run, flags, pad;
  int32_t iters[VO_MAX_LEVELS];
};
static_assert(sizeof(al_state) == 192, "al_state layout");

struct al_level { const uint8_t* prev; const uint8_t* cur; size_t seq_px; int w, h, pitch, level; };

struct vo_align_ws {
  int cap = 0;
  vo_dev<float> d_X;                   // [B][cap][3]
  vo_dev<float> d_ref;                 // [B][cap][16][3]: I, gx, gy of the reference patch (AL_FORM_WS; allocated when first used)
  vo_dev<uint8_t> d_mask;              // [B][cap]
  vo_dev<uint8_t> d_mask_tmp;          // [B][2][cap]: the masks of the last two passes
  vo_dev<al_state> d_state;            // [B]
  vo_pinned<al_state> h_state;
};

void vo_align_destroy(vo_ctx* c) {
  delete c->align;
  c->align = nullptr;
}

// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float al_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// the sum over the sixteen lanes of a DPP row, in every lane of it: row rotations by 8, 4, 2, 1
__device__ __forceinline__ float al_row_sum(float v) {
  v = v + al_dpp<0x128>(v);
  v = v + al_dpp<0x124>(v);
  v = v + al_dpp<0x122>(v);
  v = v + al_dpp<0x121>(v);
  return v;
}

// bilinear sample at (x, y) of a level whose interior starts at img: top = I00 + a (I01 - I00), bot likewise, top + b (bot - top)
__device__ __forceinline__ float al_sample(const uint8_t* img, int pitch, double x, double y) {
  const double x0 = floor(x), y0 = floor(y);
  const float a = (float)(x - x0), b = (float)(y - y0);
  const uint8_t* p = img + (ptrdiff_t)(int)y0 * pitch + (int)x0;
  const float i00 = (float)p[0], i01 = (float)p[1], i10 = (float)p[pitch], i11 = (float)p[pitch + 1];
  const float top = i00 + a * (i01 - i00), bot = i10 + a * (i11 - i10);
  return top + b * (bot - top);
}

__device__ __forceinline__ bool al_interior(double x, double y, int w, int h) {
  return x >= 4.0 && x < (double)w - 5.0 && y >= 4.0 && y < (double)h - 5.0;
}

__host__ __device__ inline void al_rodrigues(const double* r, double* R) {
  const double th = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
  double a, bq;
  if (th < 1e-12) { a = 1.0; bq = 0.0; }
  else { a = sin(th) / th; bq = (1.0 - cos(th)) / (th * th); }
  const double K0[9] = {0, -r[2], r[1], r[2], 0, -r[0], -r[1], r[0], 0};
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double kk = 0;
      for (int k = 0; k < 3; k++) kk += K0[3 * i + k] * K0[3 * k + j];
      R[3 * i + j] = (i == j ? 1.0 : 0.0) + a * K0[3 * i + j] + bq * kk;
    }
}

// the reference side of one patch pixel: I, gx, gy at (x, y) of the previous level
struct al_ref { float I, gx, gy; };
__device__ __forceinline__ al_ref al_reference(const uint8_t* img, int pitch, double x, double y) {
  al_ref r;
  r.I = al_sample(img, pitch, x, y);
  r.gx = 0.5f * (al_sample(img, pitch, x + 1.0, y) - al_sample(img, pitch, x - 1.0, y));
  r.gy = 0.5f * (al_sample(img, pitch, x, y + 1.0) - al_sample(img, pitch, x, y - 1.0));
  return r;
}

// grid (batch), 256 threads
template <bool WS>
__global__ void __launch_bounds__(256) k_align_level(al_level L, const float* __restrict__ X_all, int cap, int n, int max_iters, int min_points,
                                                     float huber, double eps, al_state* __restrict__ st_all, uint8_t* __restrict__ mask_all,
                                                     uint8_t* __restrict__ tmp_all, float* __restrict__ ref_all) {
  __shared__ double s_part[4][VO_NSUM], s_tot[VO_NSUM];
  __shared__ double s_pose[12], s_prev[12], s_xi[6];
  __shared__ int s_flag;
  const int b = blockIdx.x, tid = threadIdx.x, px = tid & 15, grp = tid >> 4;
  const double ox = (double)((px & 3) - 2), oy = (double)((px >> 2) - 2);
  al_state* st = st_all + b;
  const float* X = X_all + (size_t)b * cap * 3;
  uint8_t* mask = mask_all + (size_t)b * cap;
  uint8_t* tmp = tmp_all + (size_t)b * 2 * cap;
  float* ref = WS ? ref_all + (size_t)b * cap * 48 : nullptr;
  const uint8_t* prev = L.prev + (size_t)b * L.seq_px + (size_t)VO_PAD * L.pitch + VO_PAD;
  const uint8_t* cur = L.cur + (size_t)b * L.seq_px + (size_t)VO_PAD * L.pitch + VO_PAD;
  const double sc = 1.0 / (double)(1 << L.level);
  const double fx = st->fx * sc, fy = st->fy * sc, cx = st->cx * sc, cy = st->cy * sc;
  if (tid < 9) s_pose[tid] = st->R[tid];
  else if (tid < 12) s_pose[tid] = st->t[tid - 9];

  // a point's row, whether it is usable, where it projects in the previous level (AL_SAFE if not usable) and the row the Jacobian is taken at
  struct al_pt { double x, y, z, ux, uy; bool ok; };
  auto point = [&](int i) {
    al_pt p;
    const int ic = i < n ? i : 0;
    p.x = (double)X[3 * ic]; p.y = (double)X[3 * ic + 1]; p.z = (double)X[3 * ic + 2];
    const bool fin = i < n && fabs(p.x) < __builtin_inf() && fabs(p.y) < __builtin_inf() && p.z > 0.0 && p.z < __builtin_inf();
    if (!fin) { p.x = 1.0; p.y = 1.0; p.z = 1.0; }
    p.ux = fx * p.x / p.z + cx; p.uy = fy * p.y / p.z + cy;
    p.ok = fin && al_interior(p.ux, p.uy, L.w, L.h);
    if (!p.ok) { p.x = 1.0; p.y = 1.0; p.z = 1.0; p.ux = AL_SAFE; p.uy = AL_SAFE; }
    return p;
  };

  if (WS) {
    for (int base = 0; base < n; base += 16) {
      const int i = base + grp;
      const al_pt p = point(i);
      if (i < n) {
        const al_ref r = al_reference(prev, L.pitch, p.ux + ox, p.uy + oy);
        float* o = ref + ((size_t)i * 16 + px) * 3;
        o[0] = r.I; o[1] = r.gx; o[2] = r.gy;
      }
    }
  }

  double chi_prev = __builtin_inf(), zbar = 1.0, chi_last = 0.0;
  int iters = 0, last = -1, n_last = 0, reason = VO_ALIGN_END_MAX_ITERS;
  for (int it = 0; it < max_iters; it++) {
    __syncthreads();                                   // the pose of this pass is in s_pose
    double Rm[9], tv[3];
#pragma unroll
    for (int k = 0; k < 9; k++) Rm[k] = s_pose[k];
#pragma unroll
    for (int k = 0; k < 3; k++) tv[k] = s_pose[9 + k];
    double acc[VO_NSUM];
#pragma unroll
    for (int k = 0; k < VO_NSUM; k++) acc[k] = 0.0;
    uint8_t* tm = tmp + (size_t)(it & 1) * cap;
    for (int base = 0; base < n; base += 16) {
      const int i = base + grp;
      const al_pt p = point(i);
      al_ref r;
      if (WS) {
        const float* o = ref + ((size_t)(i < n ? i : 0) * 16 + px) * 3;
        r.I = o[0]; r.gx = o[1]; r.gy = o[2];
      } else {
        r = al_reference(prev, L.pitch, p.ux + ox, p.uy + oy);
      }
      const double Yx = (Rm[0] * p.x + Rm[1] * p.y) + Rm[2] * p.z + tv[0];
      const double Yy = (Rm[3] * p.x + Rm[4] * p.y) + Rm[5] * p.z + tv[1];
      const double Yz = (Rm[6] * p.x + Rm[7] * p.y) + Rm[8] * p.z + tv[2];
      const bool front = Yz > 0.0 && Yz < __builtin_inf();
      const double zs = front ? Yz : 1.0;
      double vx = fx * Yx / zs + cx, vy = fy * Yy / zs + cy;
      const bool used = p.ok && front && al_interior(vx, vy, L.w, L.h);
      if (!used) { vx = AL_SAFE; vy = AL_SAFE; }
      const float res = al_sample(cur, L.pitch, vx + ox, vy + oy) - r.I;
      const float ar = fabsf(res);
      const float wt = (huber > 0.0f && ar > huber) ? huber / ar : 1.0f;
      const float wgx = wt * r.gx, wgy = wt * r.gy;
      const float gxx = al_row_sum(wgx * r.gx), gxy = al_row_sum(wgx * r.gy), gyy = al_row_sum(wgy * r.gy);
      const float ex = al_row_sum(wgx * res), ey = al_row_sum(wgy * res), qq = al_row_sum((wt * res) * res);
      if (px == 0 && i < n) tm[i] = used ? 1 : 0;
      if (px == 0 && used) {
        // J_p = dpi_l/dX [I | -[X]x] at the reference point
        const double iz = 1.0 / p.z;
        const double a00 = fx * iz, a02 = -(fx * p.x * iz) * iz, a11 = fy * iz, a12 = -(fy * p.y * iz) * iz;
        const double J0[6] = {a00, 0.0, a02, a02 * p.y, a00 * p.z - a02 * p.x, -(a00 * p.y)};
        const double J1[6] = {0.0, a11, a12, a12 * p.y - a11 * p.z, -(a12 * p.x), a11 * p.x};
        const double Gxx = (double)gxx, Gxy = (double)gxy, Gyy = (double)gyy, Ex = (double)ex, Ey = (double)ey;
        double M0[6], M1[6];
#pragma unroll
        for (int k = 0; k < 6; k++) { M0[k] = Gxx * J0[k] + Gxy * J1[k]; M1[k] = Gxy * J0[k] + Gyy * J1[k]; }
        int q = 0;
#pragma unroll
        for (int a = 0; a < 6; a++)
#pragma unroll
          for (int c = a; c < 6; c++) acc[q++] += J0[a] * M0[c] + J1[a] * M1[c];
#pragma unroll
        for (int a = 0; a < 6; a++) acc[21 + a] += J0[a] * Ex + J1[a] * Ey;
        acc[27] += (double)qq; acc[28] += 1.0; acc[29] += Yz;
      }
    }
    vo_block_sum(acc, s_part, s_tot);
    const int n_used = (int)s_tot[28];
    if (it == 0) {
      if (n_used < min_points) { iters = -1; break; }
      zbar = s_tot[29] / (double)n_used;
    }
    iters = it + 1;
    const double chi = n_used > 0 ? s_tot[27] / (16.0 * (double)n_used) : __builtin_inf();
    if (n_used < min_points || chi > chi_prev) {       // the step is not kept
      __syncthreads();
      if (tid < 12) s_pose[tid] = s_prev[tid];
      reason = n_used < min_points ? VO_ALIGN_END_POINTS : VO_ALIGN_END_CHI;
      break;
    }
    last = it & 1; n_last = n_used; chi_last = chi;
    if (tid == 0) {
      double g[6], d[6];
#pragma unroll
      for (int a = 0; a < 6; a++) g[a] = s_tot[21 + a];
      const bool okc = vo_chol6_solve(s_tot, g, d);
      s_flag = okc ? 1 : 0;
      if (okc) {
        // T <- T E(xi)^-1: R <- R Rodrigues(omega)^T, t <- t - R v
        double E[9], Rn[9];
        const double w[3] = {d[3], d[4], d[5]};
        al_rodrigues(w, E);
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
          for (int j = 0; j < 3; j++) Rn[3 * i + j] = (Rm[3 * i] * E[3 * j] + Rm[3 * i + 1] * E[3 * j + 1]) + Rm[3 * i + 2] * E[3 * j + 2];
#pragma unroll
        for (int k = 0; k < 9; k++) { s_prev[k] = Rm[k]; s_pose[k] = Rn[k]; }
#pragma unroll
        for (int i = 0; i < 3; i++) {
          s_prev[9 + i] = tv[i];
          s_pose[9 + i] = tv[i] - ((Rn[3 * i] * d[0] + Rn[3 * i + 1] * d[1]) + Rn[3 * i + 2] * d[2]);
        }
#pragma unroll
        for (int k = 0; k < 6; k++) s_xi[k] = d[k];
      }
    }
    __syncthreads();
    if (!s_flag) { reason = VO_ALIGN_END_PIVOT; break; }
    chi_prev = chi;
    const double step = fmax(fmax(fmax(fabs(s_xi[3]), fabs(s_xi[4])), fabs(s_xi[5])),
                             fmax(fmax(fabs(s_xi[0]), fabs(s_xi[1])), fabs(s_xi[2])) / zbar);
    if (step < eps) { reason = VO_ALIGN_END_EPS; break; }
  }
  __syncthreads();
  if (iters > 0) {
    const uint8_t* tm = tmp + (size_t)last * cap;
    for (int i = tid; i < n; i += 256) mask[i] = tm[i];
    if (tid < 9) st->R[tid] = s_pose[tid];
    else if (tid < 12) st->t[tid - 9] = s_pose[tid];
  }
  if (tid == 0) {
    st->iters[L.level] = iters;
    if (iters > 0) { st->chi = chi_last; st->zbar = zbar; st->n_used = n_last; st->levels_run += 1; st->flags = reason; }
  }
}

// ================================================================================================
// host
// ================================================================================================
extern "C" int32_t vo_align_default_params(vo_align_params* p) {
  if (!p) return VO_E_INVALID;
  p->max_level = -1; p->min_level = 0; p->max_iters = 10; p->min_points = 10; p->huber = 10.0f; p->eps = 1e-5f; p->form = 0; p->reserved = 0;
  return VO_OK;
}

static void al_log_so3(const double* R, double* r) {
  double c = (R[0] + R[4] + R[8] - 1.0) / 2.0;
  c = fmin(1.0, fmax(-1.0, c));
  const double th = acos(c);
  const double w[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
  const double k = th < 1e-10 ? 0.5 : th / (2.0 * sin(th));
  r[0] = k * w[0]; r[1] = k * w[1]; r[2] = k * w[2];
}

static int32_t align_alloc(vo_ctx* c, bool want_ref) {
  const size_t B = c->batch;
  if (!c->align) {
    const int32_t r = vo_ws_replace(c->align, [&](vo_align_ws& w) -> int32_t {
      w.cap = c->max_pts > 0 ? c->max_pts : 1;
      VO_HIP(c, w.d_X.reserve(B * w.cap * 3));
      VO_HIP(c, w.d_mask.reserve(B * w.cap));
      VO_HIP(c, w.d_mask_tmp.reserve(B * 2 * w.cap));
      VO_HIP(c, w.d_state.reserve(B));
      VO_HIP(c, w.h_state.reserve(B));
      return VO_OK;
    });
    if (r != VO_OK) return r;
  }
  if (want_ref) VO_HIP(c, c->align->d_ref.reserve(B * c->align->cap * 48));
  return VO_OK;
}

extern "C" int32_t vo_sparse_align(vo_ctx* c, const double* K, const float* pts3d, int32_t n, const double* rvec0, const double* tvec0,
                                   const vo_align_params* prm, double* rvec, double* tvec, uint8_t* used_mask, vo_align_stats* stats) {
  if (!c) return VO_E_INVALID;
  vo_align_params def;
  if (!prm) { vo_align_default_params(&def); prm = &def; }
  VO_CHECK(c, c->n_pushed >= 2, VO_E_STATE, "two frames must have been pushed");
  VO_CHECK(c, !vo_pipe_busy(c) && c->steps_enq == c->steps_fetched, VO_E_STATE, "steps in flight: fetch them first");
  VO_CHECK(c, n >= 0 && K && (pts3d || n == 0), VO_E_INVALID, "null buffer or negative n");
  VO_CHECK(c, n <= c->max_pts, VO_E_CAPACITY, "n exceeds max_pts");
  const int max_level = prm->max_level == -1 ? c->top : prm->max_level;
  VO_CHECK(c, prm->min_level >= 0 && max_level <= c->top && prm->min_level <= max_level, VO_E_INVALID, "levels outside the store, or min_level > max_level");
  VO_CHECK(c, prm->max_iters >= 1 && prm->min_points >= 1, VO_E_INVALID, "max_iters and min_points must be at least 1");
  VO_CHECK(c, prm->huber >= 0.0f && prm->huber < __builtin_inff() && prm->eps >= 0.0f && prm->eps < __builtin_inff(), VO_E_INVALID,
           "huber and eps must be finite and not negative");
  VO_CHECK(c, prm->form >= 0 && prm->form <= 2, VO_E_INVALID, "form must be 0, 1 or 2");
  VO_CHECK(c, (rvec0 == nullptr) == (tvec0 == nullptr), VO_E_INVALID, "rvec0 and tvec0 go together");
  VO_HIP(c, hipSetDevice(c->device));
  { const int32_t rq = vo_quiesce_side(c); if (rq != VO_OK) return rq; }
  const int form = prm->form ? prm->form : AL_FORM_RULE;
  { const int32_t r = align_alloc(c, form == AL_FORM_WS); if (r != VO_OK) return r; }
  vo_align_ws* w = c->align;
  hipStream_t q = c->stream;
  const size_t B = c->batch;
  for (size_t b = 0; b < B; b++) {
    al_state& s = w->h_state[b];
    memset(&s, 0, sizeof(s));
    const double* Kb = K + 9 * b;
    s.fx = Kb[0]; s.fy = Kb[4]; s.cx = Kb[2]; s.cy = Kb[5];
    const double zero[3] = {0.0, 0.0, 0.0};
    al_rodrigues(rvec0 ? rvec0 + 3 * b : zero, s.R);
    memcpy(s.t, tvec0 ? tvec0 + 3 * b : zero, sizeof(s.t));
  }
  VO_HIP(c, hipMemcpyAsync(w->d_state, w->h_state, sizeof(al_state) * B, hipMemcpyHostToDevice, q));
  if (n > 0) {
    const size_t row = sizeof(float) * 3 * n;
    VO_HIP(c, hipMemcpy2DAsync(w->d_X, sizeof(float) * 3 * w->cap, pts3d, row, row, B, hipMemcpyHostToDevice, q));
  }
  VO_HIP(c, hipMemsetAsync(w->d_mask, 0, B * w->cap, q));
  const vo_frame& P = c->fr[c->cur ^ 1];
  const vo_frame& C = c->fr[c->cur];
  for (int l = max_level; l >= prm->min_level; l--) {
    const al_level L = {P.img[l], C.img[l], c->lvl_px[l], c->lv[l].w, c->lv[l].h, c->lv[l].pitch, l};
    vo_prof_scope prof(c, q, VO_PROF_ALIGN);
    if (form == AL_FORM_WS)
      hipLaunchKernelGGL(k_align_level<true>, dim3((unsigned)B), dim3(256), 0, q, L, w->d_X, w->cap, n, prm->max_iters, prm->min_points, prm->huber,
                         (double)prm->eps, w->d_state, w->d_mask, w->d_mask_tmp, w->d_ref);
    else
      hipLaunchKernelGGL(k_align_level<false>, dim3((unsigned)B), dim3(256), 0, q, L, w->d_X, w->cap, n, prm->max_iters, prm->min_points, prm->huber,
                         (double)prm->eps, w->d_state, w->d_mask, w->d_mask_tmp, (float*)nullptr);
  }
  VO_HIP(c, hipGetLastError());
  VO_HIP(c, hipMemcpyAsync(w->h_state, w->d_state, sizeof(al_state) * B, hipMemcpyDeviceToHost, q));
  if (used_mask && n > 0) VO_HIP(c, hipMemcpy2DAsync(used_mask, n, w->d_mask, w->cap, n, B, hipMemcpyDeviceToHost, q));
  VO_HIP(c, hipStreamSynchronize(q));
  for (size_t b = 0; b < B; b++) {
    const al_state& s = w->h_state[b];
    if (rvec) {
      if (s.levels_run > 0) al_log_so3(s.R, rvec + 3 * b);
      else for (int k = 0; k < 3; k++) rvec[3 * b + k] = rvec0 ? rvec0[3 * b + k] : 0.0;      // the initial pose as it was given
    }
    if (tvec) memcpy(tvec + 3 * b, s.t, sizeof(s.t));
    if (stats) {
      vo_align_stats& o = stats[b];
      o.status = s.levels_run > 0 ? 0 : VO_E_NUMERIC; o.n_used = s.n_used; o.levels_run = s.levels_run; o.flags = s.flags;
      for (int l = 0; l < VO_MAX_LEVELS; l++) o.iters[l] = s.iters[l];
      o.chi2 = (float)s.chi; o.zbar = (float)s.zbar;
    }
  }
  return VO_OK;
}
