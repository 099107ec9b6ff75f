// Recursive depth filter for track candidates: every candidate corner of a reference frame (a seed) holds a Gaussian over the inverse
// distance along its bearing and a Beta over its inlier ratio (Vogiatzis and Hernandez 2011); every later frame with a known pose gives one
// measurement, found by a patch search along the piece of the epipolar line the current uncertainty bounds (Forster et al., SVO, ICRA 2014,
// V; the dense form: Pizzoli et al., REMODE, ICRA 2014).  The algorithm is defined by tests/depth_model.py and stated in include/vo_mi355x.h.
//
// k_depth_update: one wave per seed, four seeds per workgroup, grid (ceil(n / 4), batch).
//   geometry   steps 1-4 and 7-10 of the model in float64, the same in every lane (most of the kernel's 1 493 float64 instructions; no lane holds an array)
//   search     one lane per candidate, 64 candidates per pass: the lane reads its eight rows as three aligned dwords each and shifts the
//              eight bytes out (v_alignbyte), then sum q, sum q^2 and sum p q by v_dot4_u32_u8 against the reference rows, which are the
//              same in every lane and sit in SGPRs; S is exact in int32; the arg-min over (S, k) is one wave reduction of the 64-bit key
//              after the last pass -- no cross-lane traffic per candidate
//   alignment  one lane per patch pixel; the 64-pixel sums in float32 by DPP row rotations (8, 4, 2, 1) and two butterflies (16, 32): the
//              order the model's tree_sum states
// Every index that addresses the store comes from a comparison in float64 that a NaN fails: a candidate that cannot be scored reads at
// (5, 5), an alignment that leaves the image ends before it samples.  The seed's own pixel never addresses the store here.
// k_depth_seed_init: one thread per patch row copies ten bytes of the current level 0.
#include "vo_internal.h"

#include <math.h>
#include <string.h>

#define DP_WAVES 4
#define DP_POSE 13                     // R (9), t (3), usable
#define DP_POSE_MAX 1e15
#define DP_INF __builtin_inf()

struct dp_args {
  const uint8_t* img; size_t seq_px; int w, h, pitch;
  const double* K4;                    // [B][4] fx, fy, cx, cy
  const double* poses;                 // [B][n_ref][DP_POSE]
  int n_ref, cap, n;
  vo_depth_seed* seeds;                // [B][cap]
  const uint8_t* patches;              // [B][cap][100]
  uint8_t* result;                     // [B][cap]
  float* match;                        // [B][cap][2]
  double* z;                           // [B][cap]
  int32_t* stats;                      // [B][10]
  int max_steps, max_iters, max_score;
  double eps_align, px_noise, conv_ratio, min_inlier;
};

struct vo_depth_ws {
  int cap = 0, n_ref_cap = 0;
  vo_dev<vo_depth_seed> d_seeds;       // [B][cap]
  vo_dev<uint8_t> d_patch;             // [B][cap][100]
  vo_dev<uint8_t> d_result;            // [B][cap]
  vo_dev<float> d_match;               // [B][cap][2]; the seed pixels on the way in (vo_depth_seed_init)
  vo_dev<double> d_z;                  // [B][cap]
  vo_dev<int32_t> d_stats;             // [B][10]
  vo_dev<double> d_head;               // [B][4] K, then [B][n_ref_cap][DP_POSE]
  vo_pinned<double> h_head;
  vo_pinned<int32_t> h_stats;
};

void vo_depth_destroy(vo_ctx* c) {
  delete c->depth;
  c->depth = nullptr;
}

// ------------------------------------------------------------------------------------------------
// device
// ------------------------------------------------------------------------------------------------
template <int CTRL>
__device__ __forceinline__ float dp_dpp(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
// the sum over the wave's 64 lanes, in every lane: DPP row rotations by 8, 4, 2, 1, then lanes l ^ 16 and l ^ 32
__device__ __forceinline__ float dp_wave_sum(float v) {
  v = v + dp_dpp<0x128>(v);
  v = v + dp_dpp<0x124>(v);
  v = v + dp_dpp<0x122>(v);
  v = v + dp_dpp<0x121>(v);
  v = v + __shfl_xor(v, 16);
  v = v + __shfl_xor(v, 32);
  return v;
}

__device__ __forceinline__ bool dp_finite(double x) { return fabs(x) < DP_INF; }
__device__ __forceinline__ bool dp_scorable(double x, double y, int w, int h) {
  return x >= 5.0 && x <= (double)(w - 5) && y >= 5.0 && y <= (double)(h - 5);
}

// bilinear sample in the aligner's form; img is the interior's origin
__device__ __forceinline__ float dp_sample(const uint8_t* img, int pitch, double x, double y) {
  const double x0 = floor(x), y0 = floor(y);
  const float a = (float)(x - x0), b = (float)(y - y0);
  const uint8_t* p = img + (ptrdiff_t)(int)y0 * pitch + (int)x0;
  const float i00 = (float)p[0], i01 = (float)p[1], i10 = (float)p[pitch], i11 = (float)p[pitch + 1];
  const float top = i00 + a * (i01 - i00), bot = i10 + a * (i11 - i10);
  return top + b * (bot - top);
}

__device__ __forceinline__ double dp_dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

struct dp_out { int code; double mx, my, z, mu, sg2, a, b; };

// one update of one seed by one wave; P: the seed's 10 x 10 patch in LDS; img: the interior's origin of the sequence's current level 0
__device__ __forceinline__ dp_out dp_seed(const dp_args& A, const vo_depth_seed& sd, const uint8_t* P, const uint8_t* img, const double* K4,
                                          const double* poses, int lane) {
  const double NaN = __builtin_nan("");
  dp_out o = {VO_DEPTH_SKIP_INACTIVE, NaN, NaN, NaN, sd.mu, sd.sigma2, sd.a, sd.b};
  const int w = A.w, h = A.h, pitch = A.pitch;
  const double mu = sd.mu, sg2 = sd.sigma2, sa = sd.a, sb = sd.b, zr = sd.z_range;
  const double u = (double)sd.u, v = (double)sd.v;
  const double fx = K4[0], fy = K4[1], cx = K4[2], cy = K4[3];
  // 1
  const bool rid_ok = sd.ref_id >= 0 && sd.ref_id < A.n_ref;
  const double* Q = poses + (size_t)(rid_ok ? sd.ref_id : 0) * DP_POSE;
  const bool fin = dp_finite(mu) && dp_finite(sg2) && dp_finite(sa) && dp_finite(sb) && dp_finite(zr);
  const bool uv_ok = u >= 0.0 && u < (double)w && v >= 0.0 && v < (double)h;
  if (!(fin && sg2 > 0.0 && mu > 0.0 && (sd.flags & 3) == 0 && uv_ok && rid_ok && Q[12] != 0.0)) return o;
  const double t0 = Q[9], t1 = Q[10], t2 = Q[11];
  const double bx = (u - cx) / fx, by = (v - cy) / fy;
  const double bn = sqrt((bx * bx + by * by) + 1.0);
  const double f0 = bx / bn, f1 = by / bn, f2 = 1.0 / bn;
  // 2
  const double s = sqrt(sg2);
  const double d_near = 1.0 / (mu + s), d_far = 1.0 / fmax(mu - s, 1e-8), d_mid = 1.0 / mu;
  const double r0 = dp_dot3(Q[0], Q[1], Q[2], f0, f1, f2), r1 = dp_dot3(Q[3], Q[4], Q[5], f0, f1, f2), r2 = dp_dot3(Q[6], Q[7], Q[8], f0, f1, f2);
  const double az = r2 * d_near + t2, bz = r2 * d_far + t2, cz = r2 * d_mid + t2;
  o.code = VO_DEPTH_SKIP_INVISIBLE;
  if (!(az > 0.0 && bz > 0.0 && cz > 0.0)) return o;
  const double Ax = (fx * (r0 * d_near + t0)) / az + cx, Ay = (fy * (r1 * d_near + t1)) / az + cy;
  const double Bx = (fx * (r0 * d_far + t0)) / bz + cx, By = (fy * (r1 * d_far + t1)) / bz + cy;
  const double Xc = r0 * d_mid + t0, Yc = r1 * d_mid + t1;
  const double Cx = (fx * Xc) / cz + cx, Cy = (fy * Yc) / cz + cy;
  // 3
  const double Dx = Bx - Ax, Dy = By - Ay;
  const double nsf = ceil(fmax(fabs(Dx), fabs(Dy)));
  o.code = VO_DEPTH_SKIP_LONG;
  if (!(Dx == Dx && Dy == Dy && nsf <= (double)A.max_steps)) return o;
  const int n_steps = (int)nsf;
  const double offx = u - floor(u + 0.5), offy = v - floor(v + 0.5);
  double sx, sy, dx, dy;                 // where the alignment starts, and along what
  if (n_steps < 2) {
    // 4
    const double c0 = floor(Cx + 0.5), c1 = floor(Cy + 0.5);
    o.code = VO_DEPTH_SKIP_INVISIBLE;
    if (!dp_scorable(c0, c1, w, h)) return o;
    const double gx = fx * (r0 * cz - Xc * r2) / (cz * cz), gy = fy * (r1 * cz - Yc * r2) / (cz * cz);
    const double gl = sqrt(gx * gx + gy * gy);
    o.code = VO_DEPTH_SKIP_DEGENERATE;
    if (!(gl > 0.0 && gl < DP_INF)) return o;
    sx = c0; sy = c1; dx = gx / gl; dy = gy / gl;
  } else {
    // 5: the reference rows (wave-uniform) and their sums
    uint32_t pr[16];
    uint32_t Sp = 0, Sp2 = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
      const uint8_t* r = P + (j + 1) * 10 + 1;
      const uint32_t lo = (uint32_t)r[0] | ((uint32_t)r[1] << 8) | ((uint32_t)r[2] << 16) | ((uint32_t)r[3] << 24);
      const uint32_t hi = (uint32_t)r[4] | ((uint32_t)r[5] << 8) | ((uint32_t)r[6] << 16) | ((uint32_t)r[7] << 24);
      pr[2 * j] = __builtin_amdgcn_readfirstlane(lo); pr[2 * j + 1] = __builtin_amdgcn_readfirstlane(hi);
      Sp = __builtin_amdgcn_udot4(pr[2 * j], 0x01010101u, Sp, false); Sp = __builtin_amdgcn_udot4(pr[2 * j + 1], 0x01010101u, Sp, false);
      Sp2 = __builtin_amdgcn_udot4(pr[2 * j], pr[2 * j], Sp2, false); Sp2 = __builtin_amdgcn_udot4(pr[2 * j + 1], pr[2 * j + 1], Sp2, false);
    }
    const double stx = Dx / (double)n_steps, sty = Dy / (double)n_steps;
    unsigned long long best = ~0ull;
    for (int base = 0; base <= n_steps; base += 64) {
      const int k = base + lane;
      const double c0 = floor((Ax + (double)k * stx) + 0.5), c1 = floor((Ay + (double)k * sty) + 0.5);
      const bool can = k <= n_steps && dp_scorable(c0, c1, w, h);
      const int px = can ? (int)c0 : 5, py = can ? (int)c1 : 5;
      // rows py - 4 .. py + 3, bytes px - 4 .. px + 3: the interior starts 4-byte aligned (VO_PAD and the pitch are multiples of 4)
      const int sh = (px - 4) & 3;
      const uint8_t* row = img + (ptrdiff_t)(py - 4) * pitch + ((px - 4) - sh);
      uint32_t Sq = 0, Sq2 = 0, Spq = 0;
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const uint32_t* r32 = reinterpret_cast<const uint32_t*>(row + (ptrdiff_t)j * pitch);
        const uint32_t w0 = r32[0], w1 = r32[1], w2 = r32[2];
        const uint32_t lo = __builtin_amdgcn_alignbyte(w1, w0, sh), hi = __builtin_amdgcn_alignbyte(w2, w1, sh);
        Sq = __builtin_amdgcn_udot4(lo, 0x01010101u, Sq, false); Sq = __builtin_amdgcn_udot4(hi, 0x01010101u, Sq, false);
        Sq2 = __builtin_amdgcn_udot4(lo, lo, Sq2, false); Sq2 = __builtin_amdgcn_udot4(hi, hi, Sq2, false);
        Spq = __builtin_amdgcn_udot4(lo, pr[2 * j], Spq, false); Spq = __builtin_amdgcn_udot4(hi, pr[2 * j + 1], Spq, false);
      }
      const int dS = (int)Sp - (int)Sq;
      const uint32_t S = 64u * (Sp2 + Sq2 - 2u * Spq) - (uint32_t)(dS * dS);
      const unsigned long long key = can ? (((unsigned long long)S << 32) | (unsigned)k) : ~0ull;
      best = key < best ? key : best;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const uint32_t olo = (uint32_t)__shfl_xor((int)(uint32_t)best, m), ohi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), m);
      const unsigned long long other = ((unsigned long long)ohi << 32) | olo;
      best = other < best ? other : best;
    }
    o.code = VO_DEPTH_SKIP_INVISIBLE;
    if (best == ~0ull) return o;
    const int kb = (int)(uint32_t)best;
    sx = floor((Ax + (double)kb * stx) + 0.5); sy = floor((Ay + (double)kb * sty) + 0.5);
    if ((long long)(best >> 32) > 64ll * A.max_score) {
      o.code = VO_DEPTH_OUTLIER_NOMATCH; o.mx = sx + offx; o.my = sy + offy; o.b = sb + 1.0;
      return o;
    }
    const double Dl = sqrt(Dx * Dx + Dy * Dy);
    dx = Dx / Dl; dy = Dy / Dl;
  }
  // 6: one lane per pixel of the inner 8 x 8
  const int pi = lane & 7, pj = lane >> 3;
  const uint8_t* pp = P + (pj + 1) * 10 + (pi + 1);
  const float T = (float)pp[0];
  const float gx = 0.5f * ((float)pp[1] - (float)pp[-1]), gy = 0.5f * ((float)pp[10] - (float)pp[-10]);
  const float g = (float)dx * gx + (float)dy * gy;
  const double H00 = (double)dp_wave_sum(g * g), H01 = (double)dp_wave_sum(g);
  const double det = H00 * 64.0 - H01 * H01;
  o.code = VO_DEPTH_OUTLIER_ALIGN; o.b = sb + 1.0;
  if (!(det > 0.0)) return o;
  const double ox = (double)(pi - 4), oy = (double)(pj - 4);
  double hh = 0.0, mm = 0.0;
  bool conv = false;
  for (int it = 0; it < A.max_iters; it++) {
    const double qx = sx + hh * dx, qy = sy + hh * dy;
    if (!(qx >= 4.0 && qx < (double)w - 4.0 && qy >= 4.0 && qy < (double)h - 4.0)) { o.mx = qx + offx; o.my = qy + offy; return o; }
    const float r = (dp_sample(img, pitch, qx + ox, qy + oy) - T) - (float)mm;
    const double b0 = (double)dp_wave_sum(g * r), b1 = (double)dp_wave_sum(r);
    const double dh = (64.0 * b0 - H01 * b1) / det, dm = (H00 * b1 - H01 * b0) / det;
    hh = hh - dh; mm = mm + dm;
    if (fabs(dh) < A.eps_align) { conv = true; break; }
  }
  const double px = (sx + hh * dx) + offx, py = (sy + hh * dy) + offy;
  o.mx = px; o.my = py;
  if (!conv) return o;
  // 7
  o.code = VO_DEPTH_SKIP_DEGENERATE; o.b = sb;
  const double ex = (px - cx) / fx, ey = (py - cy) / fy;
  const double en = sqrt((ex * ex + ey * ey) + 1.0);
  const double e0 = ex / en, e1 = ey / en, e2 = 1.0 / en;
  const double aa = dp_dot3(r0, r1, r2, r0, r1, r2), cc = dp_dot3(e0, e1, e2, e0, e1, e2), ac = dp_dot3(r0, r1, r2, e0, e1, e2);
  const double at = dp_dot3(r0, r1, r2, t0, t1, t2), ct = dp_dot3(e0, e1, e2, t0, t1, t2);
  const double tdet = aa * cc - ac * ac, tt = dp_dot3(t0, t1, t2, t0, t1, t2);
  const double z = (ac * ct - cc * at) / tdet;
  if (!(tdet >= 1e-6 * tt && z > 0.0)) return o;
  o.z = z;
  // 8
  const double q0 = -((Q[0] * t0 + Q[3] * t1) + Q[6] * t2), q1 = -((Q[1] * t0 + Q[4] * t1) + Q[7] * t2), q2 = -((Q[2] * t0 + Q[5] * t1) + Q[8] * t2);
  const double tn = sqrt(dp_dot3(q0, q1, q2, q0, q1, q2));
  const double a0 = f0 * z - q0, a1 = f1 * z - q1, a2 = f2 * z - q2;
  const double an = sqrt(dp_dot3(a0, a1, a2, a0, a1, a2));
  const double alpha = acos(fmin(fmax(dp_dot3(f0, f1, f2, q0, q1, q2) / tn, -1.0), 1.0));
  const double beta = acos(fmin(fmax(-dp_dot3(a0, a1, a2, q0, q1, q2) / (an * tn), -1.0), 1.0));
  const double beta_p = beta + 2.0 * atan(A.px_noise / (2.0 * fx));
  const double gamma = (M_PI - alpha) - beta_p;
  const double z_p = tn * sin(beta_p) / sin(gamma);
  const double tau = z_p - z;
  const double tau_inv = 0.5 * (1.0 / fmax(1e-7, z - tau) - 1.0 / (z + tau));
  // 9
  const double x = 1.0 / z, tau2 = tau_inv * tau_inv;
  const double ns = sqrt(sg2 + tau2);
  const double s2 = 1.0 / (1.0 / sg2 + 1.0 / tau2);
  const double m = s2 * (mu / sg2 + x / tau2);
  const double d = x - mu;
  const double pdf = exp(-(d * d) / (2.0 * (ns * ns))) / (ns * sqrt(2.0 * M_PI));
  double C1 = sa / (sa + sb) * pdf, C2 = sb / (sa + sb) * (1.0 / zr);
  const double nrm = C1 + C2;
  C1 = C1 / nrm; C2 = C2 / nrm;
  const double fm = C1 * (sa + 1.0) / (sa + sb + 1.0) + C2 * sa / (sa + sb + 1.0);
  const double em = C1 * (sa + 1.0) * (sa + 2.0) / ((sa + sb + 1.0) * (sa + sb + 2.0)) + C2 * sa * (sa + 1.0) / ((sa + sb + 1.0) * (sa + sb + 2.0));
  const double mu2 = C1 * m + C2 * mu;
  const double sgn = C1 * (s2 + m * m) + C2 * (sg2 + mu * mu) - mu2 * mu2;
  const double a2n = (em - fm) / (fm - em / fm);
  const double b2n = a2n * (1.0 - fm) / fm;
  if (!(dp_finite(mu2) && dp_finite(sgn) && dp_finite(a2n) && dp_finite(b2n) && sgn > 0.0)) return o;
  o.code = VO_DEPTH_UPDATED; o.mu = mu2; o.sg2 = sgn; o.a = a2n; o.b = b2n;
  return o;
}

// grid (ceil(n / DP_WAVES), batch), 64 * DP_WAVES threads
__global__ void __launch_bounds__(64 * DP_WAVES) k_depth_update(dp_args A) {
  __shared__ alignas(4) uint8_t s_patch[DP_WAVES][112];
  const int b = blockIdx.y, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int i = blockIdx.x * DP_WAVES + wave;
  const bool have = i < A.n;
  const size_t row = (size_t)b * A.cap + (have ? i : 0);
  if (lane < 25) reinterpret_cast<uint32_t*>(s_patch[wave])[lane] = reinterpret_cast<const uint32_t*>(A.patches + row * 100)[lane];
  __syncthreads();
  if (!have) return;
  vo_depth_seed* sp = A.seeds + row;
  const vo_depth_seed sd = *sp;
  const uint8_t* img = A.img + (size_t)b * A.seq_px + (size_t)VO_PAD * A.pitch + VO_PAD;
  const dp_out o = dp_seed(A, sd, s_patch[wave], img, A.K4 + 4 * b, A.poses + (size_t)b * A.n_ref * DP_POSE, lane);
  if (lane != 0) return;
  int flags = sd.flags;
  if (o.code <= VO_DEPTH_OUTLIER_ALIGN) {
    // 10
    flags += 1 << VO_DEPTH_OBS_SHIFT;
    if (sqrt(o.sg2) < sd.z_range / A.conv_ratio) flags |= VO_DEPTH_CONVERGED;
    if (o.a / (o.a + o.b) < A.min_inlier) flags |= VO_DEPTH_DIVERGED;
    sp->mu = o.mu; sp->sigma2 = o.sg2; sp->a = o.a; sp->b = o.b; sp->flags = flags;
  }
  if (A.result) A.result[row] = (uint8_t)o.code;
  if (A.match) { A.match[2 * row] = (float)o.mx; A.match[2 * row + 1] = (float)o.my; }
  if (A.z) A.z[row] = o.z;
  int32_t* st = A.stats + 10 * b;
  atomicAdd(st + o.code, 1);
  if (flags & VO_DEPTH_CONVERGED) atomicAdd(st + 7, 1);
  if (flags & VO_DEPTH_DIVERGED) atomicAdd(st + 8, 1);
}

// grid (ceil(10 n / 256), batch), 256 threads: thread = (seed, patch row)
__global__ void __launch_bounds__(256) k_depth_seed_init(const uint8_t* __restrict__ img_all, size_t seq_px, int w, int h, int pitch,
                                                         const float* __restrict__ uv_all, const double* __restrict__ depth, int cap, int n,
                                                         int ref_id, vo_depth_seed* __restrict__ seeds, uint8_t* __restrict__ patches,
                                                         uint8_t* __restrict__ ok_all) {
  const int b = blockIdx.y, tid = blockIdx.x * 256 + threadIdx.x;
  const int i = tid / 10, j = tid - 10 * i;
  if (i >= n) return;
  const size_t row = (size_t)b * cap + i;
  const float uf = uv_all[2 * row], vf = uv_all[2 * row + 1];
  const double c0 = floor((double)uf + 0.5), c1 = floor((double)vf + 0.5);
  const bool ok = dp_scorable(c0, c1, w, h);                       // (a NaN is not)
  const int px = ok ? (int)c0 : 5, py = ok ? (int)c1 : 5;
  const uint8_t* src = img_all + (size_t)b * seq_px + (size_t)(VO_PAD + py - 5 + j) * pitch + VO_PAD + px - 5;
  uint8_t* dst = patches + row * 100 + 10 * j;
#pragma unroll
  for (int k = 0; k < 10; k++) dst[k] = ok ? src[k] : (uint8_t)0;
  if (j == 0) {
    const double z_range = 1.0 / depth[2 * b + 1];
    vo_depth_seed s;
    s.mu = 1.0 / depth[2 * b]; s.sigma2 = z_range * z_range / 36.0; s.a = 10.0; s.b = 10.0; s.z_range = z_range;
    s.u = uf; s.v = vf; s.ref_id = ref_id; s.flags = ok ? 0 : VO_DEPTH_DIVERGED;
    seeds[row] = s;
    ok_all[row] = ok ? 1 : 0;
  }
}

// ================================================================================================
// host
// ================================================================================================
extern "C" int32_t vo_depth_default_params(vo_depth_params* p) {
  if (!p) return VO_E_INVALID;
  p->max_steps = 128; p->max_iters = 10; p->max_score = 300 * 64; p->eps_align = 0.03f; p->px_noise = 1.0f; p->conv_ratio = 200.0f;
  p->min_inlier = 0.1f; p->reserved = 0;
  return VO_OK;
}

static void dp_rodrigues(const double* r, double* R) {
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

static int32_t depth_alloc(vo_ctx* c, int n_ref) {
  const size_t B = c->batch;
  if (!c->depth) {
    const int32_t r = vo_ws_replace(c->depth, [&](vo_depth_ws& w) -> int32_t {
      w.cap = c->max_pts > 0 ? c->max_pts : 1;
      VO_HIP(c, w.d_seeds.reserve(B * w.cap));
      VO_HIP(c, w.d_patch.reserve(B * w.cap * 100 + 16));
      VO_HIP(c, w.d_result.reserve(B * w.cap));
      VO_HIP(c, w.d_match.reserve(B * w.cap * 2));
      VO_HIP(c, w.d_z.reserve(B * w.cap));
      VO_HIP(c, w.d_stats.reserve(B * 10));
      VO_HIP(c, w.h_stats.reserve(B * 10));
      return VO_OK;
    });
    if (r != VO_OK) return r;
  }
  vo_depth_ws* w = c->depth;
  if (n_ref > w->n_ref_cap) {
    const size_t len = B * 4 + B * (size_t)n_ref * DP_POSE;
    VO_HIP(c, w->d_head.reserve(len));
    VO_HIP(c, w->h_head.reserve(len));
    w->n_ref_cap = n_ref;
  }
  return VO_OK;
}

static bool dp_ok_float(float x) { return x >= 0.0f && x < __builtin_inff(); }

extern "C" int32_t vo_depth_seed_init(vo_ctx* c, const float* uv, int32_t n, const double* depth_mean, const double* depth_min, int32_t ref_id,
                                      vo_depth_seed* seeds, uint8_t* patches, uint8_t* ok_mask) {
  if (!c) return VO_E_INVALID;
  VO_CHECK(c, c->n_pushed >= 1, VO_E_STATE, "no frame pushed yet");
  VO_CHECK(c, !vo_pipe_busy(c) && c->steps_enq == c->steps_fetched, VO_E_STATE, "steps in flight: fetch them first");
  VO_CHECK(c, n >= 0 && depth_mean && depth_min && (n == 0 || (uv && seeds && patches)), VO_E_INVALID, "null buffer or negative n");
  VO_CHECK(c, n <= c->max_pts, VO_E_CAPACITY, "n exceeds max_pts");
  const size_t B = c->batch;
  for (size_t b = 0; b < B; b++)
    VO_CHECK(c, depth_mean[b] > 0.0 && depth_mean[b] < DP_INF && depth_min[b] > 0.0 && depth_min[b] < DP_INF, VO_E_INVALID,
             "depth_mean and depth_min must be finite and positive");
  if (n == 0) return VO_OK;
  VO_HIP(c, hipSetDevice(c->device));
  { const int32_t rq = vo_quiesce_side(c); if (rq != VO_OK) return rq; }
  { const int32_t r = depth_alloc(c, 1); if (r != VO_OK) return r; }
  vo_depth_ws* w = c->depth;
  hipStream_t q = c->stream;
  for (size_t b = 0; b < B; b++) { w->h_head[2 * b] = depth_mean[b]; w->h_head[2 * b + 1] = depth_min[b]; }
  VO_HIP(c, hipMemcpyAsync(w->d_head, w->h_head, sizeof(double) * 2 * B, hipMemcpyHostToDevice, q));
  const size_t urow = sizeof(float) * 2 * n;
  VO_HIP(c, hipMemcpy2DAsync(w->d_match, sizeof(float) * 2 * w->cap, uv, urow, urow, B, hipMemcpyHostToDevice, q));
  const vo_frame& F = c->fr[c->cur];
  hipLaunchKernelGGL(k_depth_seed_init, dim3((unsigned)vo_div_up(10 * n, 256), (unsigned)B), dim3(256), 0, q, F.img[0], c->lvl_px[0], c->lv[0].w,
                     c->lv[0].h, c->lv[0].pitch, w->d_match, w->d_head, w->cap, n, ref_id, w->d_seeds, w->d_patch, w->d_result);
  VO_HIP(c, hipGetLastError());
  const size_t srow = sizeof(vo_depth_seed) * n;
  VO_HIP(c, hipMemcpy2DAsync(seeds, srow, w->d_seeds, sizeof(vo_depth_seed) * w->cap, srow, B, hipMemcpyDeviceToHost, q));
  VO_HIP(c, hipMemcpy2DAsync(patches, 100 * (size_t)n, w->d_patch, 100 * (size_t)w->cap, 100 * (size_t)n, B, hipMemcpyDeviceToHost, q));
  if (ok_mask) VO_HIP(c, hipMemcpy2DAsync(ok_mask, n, w->d_result, w->cap, n, B, hipMemcpyDeviceToHost, q));
  VO_HIP(c, hipStreamSynchronize(q));
  return VO_OK;
}

extern "C" int32_t vo_depth_update(vo_ctx* c, const double* K, const double* poses, int32_t n_ref, vo_depth_seed* seeds, const uint8_t* patches,
                                   int32_t n, const vo_depth_params* prm, uint8_t* result, float* match_uv, double* z, vo_depth_stats* stats) {
  if (!c) return VO_E_INVALID;
  vo_depth_params def;
  if (!prm) { vo_depth_default_params(&def); prm = &def; }
  VO_CHECK(c, c->n_pushed >= 1, VO_E_STATE, "no frame pushed yet");
  VO_CHECK(c, !vo_pipe_busy(c) && c->steps_enq == c->steps_fetched, VO_E_STATE, "steps in flight: fetch them first");
  VO_CHECK(c, n >= 0 && K && poses && (n == 0 || (seeds && patches)), VO_E_INVALID, "null buffer or negative n");
  VO_CHECK(c, n_ref >= 1, VO_E_INVALID, "n_ref must be at least 1");
  VO_CHECK(c, n <= c->max_pts, VO_E_CAPACITY, "n exceeds max_pts");
  VO_CHECK(c, prm->max_steps >= 1 && prm->max_steps <= 128 && prm->max_iters >= 1, VO_E_INVALID, "max_steps outside 1..128, or max_iters < 1");
  VO_CHECK(c, prm->max_score >= 0 && prm->max_score <= 4161600, VO_E_INVALID, "max_score outside 0..4161600");
  VO_CHECK(c, dp_ok_float(prm->eps_align) && dp_ok_float(prm->px_noise) && dp_ok_float(prm->conv_ratio) && dp_ok_float(prm->min_inlier), VO_E_INVALID,
           "eps_align, px_noise, conv_ratio and min_inlier must be finite and not negative");
  VO_CHECK(c, prm->conv_ratio > 0.0f, VO_E_INVALID, "conv_ratio must be positive (z_range / 0 would call every seed converged)");
  const size_t B = c->batch;
  if (n == 0) {
    if (stats) memset(stats, 0, sizeof(vo_depth_stats) * B);
    return VO_OK;
  }
  VO_HIP(c, hipSetDevice(c->device));
  { const int32_t rq = vo_quiesce_side(c); if (rq != VO_OK) return rq; }
  { const int32_t r = depth_alloc(c, n_ref); if (r != VO_OK) return r; }
  vo_depth_ws* w = c->depth;
  hipStream_t q = c->stream;
  double* hp = w->h_head + 4 * B;
  for (size_t b = 0; b < B; b++) {
    const double* Kb = K + 9 * b;
    w->h_head[4 * b] = Kb[0]; w->h_head[4 * b + 1] = Kb[4]; w->h_head[4 * b + 2] = Kb[2]; w->h_head[4 * b + 3] = Kb[5];
    for (int r = 0; r < n_ref; r++) {
      const double* p = poses + (b * n_ref + r) * 6;
      double* o = hp + (b * n_ref + r) * DP_POSE;
      bool ok = true;
      for (int k = 0; k < 6; k++) ok = ok && fabs(p[k]) <= DP_POSE_MAX;          // (a NaN is not)
      const double zero[3] = {0.0, 0.0, 0.0};
      dp_rodrigues(ok ? p : zero, o);
      for (int k = 0; k < 3; k++) o[9 + k] = ok ? p[3 + k] : 0.0;
      o[12] = ok ? 1.0 : 0.0;
    }
  }
  const size_t head = 4 * B + B * (size_t)n_ref * DP_POSE;
  VO_HIP(c, hipMemcpyAsync(w->d_head, w->h_head, sizeof(double) * head, hipMemcpyHostToDevice, q));
  const size_t srow = sizeof(vo_depth_seed) * n, prow = 100 * (size_t)n;
  VO_HIP(c, hipMemcpy2DAsync(w->d_seeds, sizeof(vo_depth_seed) * w->cap, seeds, srow, srow, B, hipMemcpyHostToDevice, q));
  VO_HIP(c, hipMemcpy2DAsync(w->d_patch, 100 * (size_t)w->cap, patches, prow, prow, B, hipMemcpyHostToDevice, q));
  VO_HIP(c, hipMemsetAsync(w->d_stats, 0, sizeof(int32_t) * 10 * B, q));
  dp_args A;
  A.img = c->fr[c->cur].img[0]; A.seq_px = c->lvl_px[0]; A.w = c->lv[0].w; A.h = c->lv[0].h; A.pitch = c->lv[0].pitch;
  A.K4 = w->d_head; A.poses = w->d_head + 4 * B; A.n_ref = n_ref; A.cap = w->cap; A.n = n;
  A.seeds = w->d_seeds; A.patches = w->d_patch; A.result = w->d_result; A.match = w->d_match; A.z = w->d_z; A.stats = w->d_stats;
  A.max_steps = prm->max_steps; A.max_iters = prm->max_iters; A.max_score = prm->max_score;
  A.eps_align = (double)prm->eps_align; A.px_noise = (double)prm->px_noise; A.conv_ratio = (double)prm->conv_ratio; A.min_inlier = (double)prm->min_inlier;
  {
    vo_prof_scope prof(c, q, VO_PROF_DEPTH);
    hipLaunchKernelGGL(k_depth_update, dim3((unsigned)vo_div_up(n, DP_WAVES), (unsigned)B), dim3(64 * DP_WAVES), 0, q, A);
  }
  VO_HIP(c, hipGetLastError());
  VO_HIP(c, hipMemcpy2DAsync(seeds, srow, w->d_seeds, sizeof(vo_depth_seed) * w->cap, srow, B, hipMemcpyDeviceToHost, q));
  if (result) VO_HIP(c, hipMemcpy2DAsync(result, n, w->d_result, w->cap, n, B, hipMemcpyDeviceToHost, q));
  if (match_uv) VO_HIP(c, hipMemcpy2DAsync(match_uv, sizeof(float) * 2 * n, w->d_match, sizeof(float) * 2 * w->cap, sizeof(float) * 2 * n, B, hipMemcpyDeviceToHost, q));
  if (z) VO_HIP(c, hipMemcpy2DAsync(z, sizeof(double) * n, w->d_z, sizeof(double) * w->cap, sizeof(double) * n, B, hipMemcpyDeviceToHost, q));
  VO_HIP(c, hipMemcpyAsync(w->h_stats, w->d_stats, sizeof(int32_t) * 10 * B, hipMemcpyDeviceToHost, q));
  VO_HIP(c, hipStreamSynchronize(q));
  if (stats)
    for (size_t b = 0; b < B; b++) {
      const int32_t* s = w->h_stats + 10 * b;
      for (int k = 0; k < 7; k++) stats[b].counts[k] = s[k];
      stats[b].converged = s[7]; stats[b].diverged = s[8]; stats[b].reserved = 0;
    }
  return VO_OK;
}
