// Pose from a homography: what the 2D-2D bootstrap does with the H it has just fitted when the degeneracy check fires (a planar scene, or
// no baseline), where the five-point t means nothing.
//
// cv2.decomposeHomographyMat(H, K) followed by cv2.filterHomographyDecompByVisibleRefpoints, with OpenCV's two visibility tests counted per
// candidate instead of all-or-nothing, so that an outlier does not veto a candidate (ORB-SLAM's ReconstructH and COLMAP rank the same way).
// The algorithm is defined by tests/hpose_model.py and compared with it candidate by candidate and count by count:
//   decompose  one lane, float64: G = K^-1 H K of the H scaled by its largest entry, negated if det G < 0; one-sided Jacobi on the columns
//              of G (vo_jacobi3_cols of vo_svd3.h, the sweeps of e5_decompose: the condition of G is never squared), singular values over the middle one; the two pairs
//              {(R, t, n), (R, -t, -n)} in closed form, s^2 - 1 entering as (s - 1)(s + 1); s1 - s3 <= 2^-26 is a rotation (one solution,
//              t = n = 0); det = 0, a zero focal length or an entry that is not finite has no solution
//   vote       256 threads stride over the points: n_good = mask points with n . m1 > 0 and (R n) . m2 > 0, n_off = points outside the mask
//              within the Sampson threshold of E = [t / |t|]x R (vo_sampson of vo_epi_dev.h, the essential search's), m = ((p - c) / f, 1)
//              in float64
//   reduce     __shfl_xor across the wave, the four waves through LDS in a fixed order: no atomics, no scratch
//   rank       one lane: viable first, n_off, the hint, n_good, then trace R and the normal's entries; the ambiguity verdict
// One kernel, grid (batch); vo_homography_pose enqueues it behind k_h4_finish on the search's stream (vo_hom_ransac_tail).  The workspace,
// the upload of the two views and a sequence's pointers are the two-view units' own: vo_twoview.h.
// This library is built with -ffp-contract=off: each vote expression rounds as the model's does.
#include "vo_twoview.h"
#include "vo_epi_dev.h"
#include "vo_svd3.h"

#include <math.h>
#include <string.h>

#define HP_OUT 80              // doubles per sequence: R (36), t (12), n (12), sigma (3), then n_solutions, n_distinct, ambiguous, status,
                               // n_mask, n_good (4), n_off (4) as doubles, 4 spare
#define HP_ROT_CUT 1.4901161193847656e-08      // 2^-26
#define HP_MERGE_TOL 9.5367431640625e-07       // 2^-20
#define HP_NCNT 9              // n_good (4), n_off (4), n_mask

struct vo_hpose_ws : vo_tv_ws {
  vo_dev<double> d_K;          // [B][9] K, then [B][9] H
};

// the candidates of one sequence as the one lane leaves them for the vote, in the order of the formulas
struct hp_cand { double R[4][9], t[4][3], n[4][3], rn[4][3], E[4][9], sigma[3]; int ns; };

__device__ __forceinline__ bool hp_finite(double x) { return fabs(x) < __builtin_inf(); }

__device__ __forceinline__ void hp_cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

// K (fx, fy, cx, cy of the 3 x 3), H -> the candidates in LDS; c->ns = 0 without a solution.  Every loop has constant bounds and the
// singular values are ordered by conditional column swaps, so no private array is indexed by a run-time value
__device__ inline void hp_decompose(const double* K, const double* Hin, hp_cand* c) {
  c->ns = 0;
  const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
  double H[9], big = 0.0;
  bool ok = hp_finite(fx) && hp_finite(fy) && hp_finite(cx) && hp_finite(cy) && fx != 0.0 && fy != 0.0;
#pragma unroll
  for (int k = 0; k < 9; k++) { H[k] = Hin[k]; ok = ok && hp_finite(H[k]); big = fmax(big, fabs(H[k])); }
  if (!ok || big == 0.0) return;
  double M[3][3], U[3][3], V[3][3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const double h0 = H[3 * r] / big, h1 = H[3 * r + 1] / big, h2 = H[3 * r + 2] / big;
    M[r][0] = h0 * fx; M[r][1] = h1 * fy; M[r][2] = (h0 * cx + h1 * cy) + h2;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) { U[0][k] = (M[0][k] - cx * M[2][k]) / fx; U[1][k] = (M[1][k] - cy * M[2][k]) / fy; U[2][k] = M[2][k]; }
  const double det = (U[0][0] * (U[1][1] * U[2][2] - U[1][2] * U[2][1]) - U[0][1] * (U[1][0] * U[2][2] - U[1][2] * U[2][0])) +
                     U[0][2] * (U[1][0] * U[2][1] - U[1][1] * U[2][0]);
  if (!(fabs(det) > 0.0) || !hp_finite(det)) return;
  const double sg = (det < 0) ? -1.0 : 1.0;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) U[i][j] = sg * U[i][j];
  double nn[3];
  vo_jacobi3_cols(U, V, nn);
  const double s1 = sqrt(nn[0]), s2 = sqrt(nn[1]), s3 = sqrt(nn[2]);
  double u1[3], u2[3], u3[3], v1[3], v2[3], v3[3];
#pragma unroll
  for (int k = 0; k < 3; k++) { u1[k] = U[k][0] / s1; u2[k] = U[k][1] / s2; v1[k] = V[k][0]; v2[k] = V[k][1]; }
  hp_cross(u1, u2, u3);
  hp_cross(v1, v2, v3);
  const double a = (s1 - s2) / s2, b = (s2 - s3) / s2, w = (s1 - s3) / s2, r1 = s1 / s2, r3 = s3 / s2;
  int ns;
  if (w <= HP_ROT_CUT) {
    ns = 1;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) c->R[0][3 * i + j] = (u1[i] * v1[j] + u2[i] * v2[j]) + u3[i] * v3[j];
#pragma unroll
    for (int k = 0; k < 3; k++) { c->t[0][k] = 0.0; c->n[0][k] = 0.0; c->rn[0][k] = 0.0; }
#pragma unroll
    for (int k = 0; k < 9; k++) c->E[0][k] = 0.0;
  } else {
    ns = 4;
    const double den = w * (r1 + r3);
    const double x1 = sqrt(a * (r1 + 1) / den), x3 = sqrt(b * (1 + r3) / den);
    const double sn = sqrt(a * (r1 + 1) * b * (1 + r3)) / (r1 + r3), cs = (1 + r1 * r3) / (r1 + r3);
#pragma unroll
    for (int pair = 0; pair < 2; pair++) {
      const double e = pair ? -1.0 : 1.0;
      double R[9], t[3], n[3], tu[3], rn[3], E[9];
#pragma unroll
      for (int k = 0; k < 3; k++) { n[k] = x1 * v1[k] + (e * x3) * v3[k]; t[k] = w * (x1 * u1[k] - (e * x3) * u3[k]); }
#pragma unroll
      for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
          R[3 * i + j] = (cs * (u1[i] * v1[j] + u3[i] * v3[j]) + u2[i] * v2[j]) + (e * sn) * (u3[i] * v1[j] - u1[i] * v3[j]);
      const double tn = sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
#pragma unroll
      for (int k = 0; k < 3; k++) { tu[k] = t[k] / tn; rn[k] = (R[3 * k] * n[0] + R[3 * k + 1] * n[1]) + R[3 * k + 2] * n[2]; }
#pragma unroll
      for (int j = 0; j < 3; j++) {
        E[j] = tu[1] * R[6 + j] - tu[2] * R[3 + j]; E[3 + j] = tu[2] * R[j] - tu[0] * R[6 + j]; E[6 + j] = tu[0] * R[3 + j] - tu[1] * R[j];
      }
      // the twin (R, -t, -n): the same R, and an E of the other sign with the same Sampson distance
#pragma unroll
      for (int tw = 0; tw < 2; tw++) {
        const int k = 2 * pair + tw;
        const double f = tw ? -1.0 : 1.0;
#pragma unroll
        for (int i = 0; i < 9; i++) { c->R[k][i] = R[i]; c->E[k][i] = f * E[i]; }
#pragma unroll
        for (int i = 0; i < 3; i++) { c->t[k][i] = f * t[i]; c->n[k][i] = f * n[i]; c->rn[k][i] = f * rn[i]; }
      }
    }
  }
  bool fin = true;
  for (int k = 0; k < ns; k++) {
    for (int i = 0; i < 9; i++) fin = fin && hp_finite(c->R[k][i]);
    for (int i = 0; i < 3; i++) fin = fin && hp_finite(c->t[k][i]) && hp_finite(c->n[k][i]);
  }
  if (!fin) return;
  c->sigma[0] = r1; c->sigma[1] = 1.0; c->sigma[2] = r3;
  c->ns = ns;
}

__device__ inline bool hp_same(const hp_cand* c, int i, int j) {
  double dR = 0.0, dt = 0.0, dn = 0.0;
  for (int k = 0; k < 9; k++) dR = fmax(dR, fabs(c->R[i][k] - c->R[j][k]));
  for (int k = 0; k < 3; k++) { dt = fmax(dt, fabs(c->t[i][k] - c->t[j][k])); dn = fmax(dn, fabs(c->n[i][k] - c->n[j][k])); }
  return dR < HP_MERGE_TOL && dt < HP_MERGE_TOL && dn < HP_MERGE_TOL;
}

// lexicographic: is key a strictly above key b
__device__ inline bool hp_above(const double* a, const double* b) {
  for (int k = 0; k < 8; k++) {
    if (a[k] > b[k]) return true;
    if (a[k] < b[k]) return false;
  }
  return false;
}

// grid (batch), 256 threads.  H of sequence b at H + b * h_stride; p [batch][2][cap][2]; mask [batch][cap] or NULL (every point);
// out [batch][HP_OUT]
__global__ void __launch_bounds__(256) k_hpose(const double* __restrict__ Kall, const double* __restrict__ Hall, int h_stride,
                                               const float* __restrict__ p, int cap, const uint8_t* __restrict__ mask_all, int n,
                                               vo_hpose_params prm, double* __restrict__ out_all) {
  __shared__ hp_cand s_c;
  __shared__ int s_cnt[4][HP_NCNT];
  __shared__ double s_key[4][8];
  __shared__ int s_ord[4], s_rep[4], s_g[HP_NCNT];           // what the ranking lane indexes by a run-time value lives in LDS
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double* K = Kall + 9 * b;
  double* out = out_all + (size_t)HP_OUT * b;
  if (tid == 0) hp_decompose(K, Hall + (size_t)b * h_stride, &s_c);
  __syncthreads();
  const int ns = s_c.ns;
  if (ns == 0) {
    if (tid < HP_OUT) out[tid] = (tid < 63) ? __builtin_nan("") : ((tid == 66) ? (double)VO_E_NUMERIC : 0.0);
    return;
  }
  int cnt[HP_NCNT];
#pragma unroll
  for (int k = 0; k < HP_NCNT; k++) cnt[k] = 0;
  if (n > 0) {
    const auto [pa, pb] = vo_tv_seq_views<float2>(p, cap, b);
    const uint8_t* mask = mask_all ? mask_all + (size_t)b * cap : nullptr;
    const double fx = K[0], fy = K[4], cx = K[2], cy = K[5];
    const double tn = prm.threshold / ((fx + fy) / 2.0);
    const double thr2 = tn * tn;
    for (int i = tid; i < n; i += 256) {
      const float2 a = pa[i], c = pb[i];
      const double x1 = ((double)a.x - cx) / fx, y1 = ((double)a.y - cy) / fy, x2 = ((double)c.x - cx) / fx, y2 = ((double)c.y - cy) / fy;
      if (!(hp_finite(x1) && hp_finite(y1) && hp_finite(x2) && hp_finite(y2))) continue;
      const bool in = mask ? (mask[i] != 0) : true;
      cnt[8] += in ? 1 : 0;
      if (ns != 4) continue;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (in) {
          const double d1 = (s_c.n[k][0] * x1 + s_c.n[k][1] * y1) + s_c.n[k][2];
          const double d2 = (s_c.rn[k][0] * x2 + s_c.rn[k][1] * y2) + s_c.rn[k][2];
          cnt[k] += (d1 > 0 && d2 > 0) ? 1 : 0;
        } else {
          cnt[4 + k] += (vo_sampson(s_c.E[k], x1, y1, x2, y2) <= thr2) ? 1 : 0;
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < HP_NCNT; k++) {
    int v = cnt[k];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if (lane == 0) s_cnt[wave][k] = v;
  }
  __syncthreads();
  if (tid != 0) return;
  int* g = s_g;
  for (int k = 0; k < HP_NCNT; k++) g[k] = (s_cnt[0][k] + s_cnt[1][k]) + (s_cnt[2][k] + s_cnt[3][k]);
  int amb = 0, nd = 1;
  for (int k = 0; k < 4; k++) s_ord[k] = k;
  if (ns == 4) {
    int best = g[0];
    for (int k = 1; k < 4; k++) best = g[k] > best ? g[k] : best;
    for (int k = 0; k < 4; k++) {
      s_key[k][0] = ((double)g[k] >= prm.ratio * (double)best) ? 1.0 : 0.0;
      s_key[k][1] = (double)g[4 + k];
      s_key[k][2] = prm.use_hint ? (s_c.n[k][0] * prm.hint[0] + s_c.n[k][1] * prm.hint[1]) + s_c.n[k][2] * prm.hint[2] : 0.0;
      s_key[k][3] = (double)g[k];
      s_key[k][4] = (s_c.R[k][0] + s_c.R[k][4]) + s_c.R[k][8];
      s_key[k][5] = s_c.n[k][2]; s_key[k][6] = s_c.n[k][1]; s_key[k][7] = s_c.n[k][0];
    }
    for (int i = 1; i < 4; i++)                             // insertion sort: an entry moves up only past a strictly smaller key
      for (int j = i; j > 0 && hp_above(s_key[s_ord[j]], s_key[s_ord[j - 1]]); j--) { const int q = s_ord[j]; s_ord[j] = s_ord[j - 1]; s_ord[j - 1] = q; }
    // classes of entries in the order of the formulas: an entry that equals no earlier representative is a new one
    nd = 0;
    for (int i = 0; i < 4; i++) {
      bool dup = false;
      for (int j = 0; j < nd; j++) dup = dup || hp_same(&s_c, i, s_rep[j]);
      if (!dup) { s_rep[nd] = i; nd++; }
    }
    const int k0 = s_ord[0];
    if (!prm.use_hint && s_key[k0][0] > 0.0)
      for (int i = 1; i < 4; i++) {
        const int k = s_ord[i];
        if (s_key[k][0] > 0.0 && !hp_same(&s_c, k0, k)) { amb = (g[4 + k0] - g[4 + k] < prm.min_off) ? 1 : 0; break; }
      }
  }
  const double nan = __builtin_nan("");
  for (int i = 0; i < 4; i++) {
    const int k = s_ord[i];
    const bool have = i < ns;
    for (int j = 0; j < 9; j++) out[9 * i + j] = have ? s_c.R[k][j] : nan;
    for (int j = 0; j < 3; j++) { out[36 + 3 * i + j] = have ? s_c.t[k][j] : nan; out[48 + 3 * i + j] = have ? s_c.n[k][j] : nan; }
    out[68 + i] = (have && ns == 4) ? (double)g[k] : 0.0;
    out[72 + i] = (have && ns == 4) ? (double)g[4 + k] : 0.0;
  }
  for (int j = 0; j < 3; j++) out[60 + j] = s_c.sigma[j];
  out[63] = (double)ns; out[64] = (double)nd; out[65] = (double)amb; out[66] = 0.0; out[67] = (double)g[8];
  for (int j = 76; j < HP_OUT; j++) out[j] = 0.0;
}

// ================================================================================================
// host
// ================================================================================================
void vo_hpose_destroy(vo_ctx* c) { vo_tv_free(c->hpose); }

extern "C" int32_t vo_homography_pose_default_params(vo_hpose_params* p) {
  if (!p) return VO_E_INVALID;
  p->ratio = 0.75; p->threshold = 1.0; p->hint[0] = 0.0; p->hint[1] = 0.0; p->hint[2] = 0.0; p->min_off = 8; p->use_hint = 0;
  return VO_OK;
}

static inline bool hp_hfinite(double x) { return fabs(x) < __builtin_inf(); }

static int32_t hpose_check(vo_ctx* c, const vo_hpose_params* prm) {
  VO_CHECK(c, prm->ratio > 0 && prm->ratio <= 1, VO_E_INVALID, "ratio outside (0, 1]");
  VO_CHECK(c, prm->threshold > 0 && hp_hfinite(prm->threshold), VO_E_INVALID, "threshold must be positive and finite");
  VO_CHECK(c, prm->min_off >= 0, VO_E_INVALID, "min_off < 0");
  if (prm->use_hint) {
    const double* h = prm->hint;
    VO_CHECK(c, hp_hfinite(h[0]) && hp_hfinite(h[1]) && hp_hfinite(h[2]) && (h[0] != 0 || h[1] != 0 || h[2] != 0), VO_E_INVALID,
             "the normal hint is zero or not finite");
  }
  return VO_OK;
}

static int32_t hpose_alloc(vo_ctx* c, int n) {
  return vo_tv_alloc(c, c->hpose, vo_hpose_destroy, n, HP_OUT, 0, 1, [c](vo_hpose_ws& w) -> int32_t {
    VO_HIP(c, w.d_K.reserve((size_t)18 * c->batch));
    return VO_OK;
  });
}

// the pinned read-back -> the caller's arrays
static void hpose_unpack(const vo_ctx* c, double* R, double* t, double* nrm, vo_hpose_stats* stats) {
  const size_t B = c->batch;
  for (size_t b = 0; b < B; b++) {
    const double* o = c->hpose->h_out + HP_OUT * b;
    if (R) memcpy(R + 36 * b, o, sizeof(double) * 36);
    if (t) memcpy(t + 12 * b, o + 36, sizeof(double) * 12);
    if (nrm) memcpy(nrm + 12 * b, o + 48, sizeof(double) * 12);
    if (stats) {
      vo_hpose_stats* s = stats + b;
      for (int k = 0; k < 3; k++) s->sigma[k] = o[60 + k];
      s->n_solutions = (int32_t)o[63]; s->n_distinct = (int32_t)o[64]; s->ambiguous = (int32_t)o[65]; s->status = (int32_t)o[66];
      s->n_mask = (int32_t)o[67];
      for (int k = 0; k < 4; k++) { s->n_good[k] = (int32_t)o[68 + k]; s->n_off[k] = (int32_t)o[72 + k]; }
      s->_pad = 0;
    }
  }
}

static void hpose_launch(vo_ctx* c, hipStream_t q, const double* d_H, int h_stride, const float* d_p, int cap, const uint8_t* d_mask, int n,
                         const vo_hpose_params* prm) {
  vo_hpose_ws* w = c->hpose;
  vo_prof_scope prof(c, q, VO_PROF_HPOSE);
  hipLaunchKernelGGL(k_hpose, dim3((unsigned)c->batch), dim3(256), 0, q, w->d_K, d_H, h_stride, d_p, cap, d_mask, n, *prm, w->d_out);
}

extern "C" int32_t vo_homography_decompose(vo_ctx* c, const double* K, const double* H, const float* pts1, const float* pts2, const uint8_t* mask,
                                           int32_t n, const vo_hpose_params* prm, double* R, double* t, double* nrm, vo_hpose_stats* stats) {
  if (!c) return VO_E_INVALID;
  vo_hpose_params def;
  if (!prm) { vo_homography_pose_default_params(&def); prm = &def; }
  VO_CHECK(c, K && H, VO_E_INVALID, "null buffer");
  VO_CHECK(c, n >= 0, VO_E_INVALID, "n < 0");
  VO_CHECK(c, n == 0 || (pts1 && pts2), VO_E_INVALID, "n > 0 with null points");
  int32_t r = hpose_check(c, prm);
  if (r != VO_OK) return r;
  VO_HIP(c, hipSetDevice(c->device));
  r = hpose_alloc(c, n);
  if (r != VO_OK) return r;
  vo_hpose_ws* w = c->hpose;
  const size_t B = c->batch;
  const int cap = w->cap;
  VO_HIP(c, hipMemcpyAsync(w->d_K, K, sizeof(double) * 9 * B, hipMemcpyHostToDevice, c->stream));
  VO_HIP(c, hipMemcpyAsync(w->d_K + 9 * B, H, sizeof(double) * 9 * B, hipMemcpyHostToDevice, c->stream));
  if (n > 0) {
    r = vo_tv_upload(c, c->stream, w, pts1, pts2, n);
    if (r != VO_OK) return r;
    if (mask) VO_HIP(c, hipMemcpy2DAsync(w->d_mask, cap, mask, n, n, B, hipMemcpyHostToDevice, c->stream));
  }
  hpose_launch(c, c->stream, w->d_K + 9 * B, 9, w->d_p, cap, (n > 0 && mask) ? w->d_mask : nullptr, n, prm);
  VO_HIP(c, hipGetLastError());
  VO_HIP(c, hipMemcpyAsync(w->h_out, w->d_out, sizeof(double) * HP_OUT * B, hipMemcpyDeviceToHost, c->stream));
  VO_HIP(c, hipStreamSynchronize(c->stream));
  hpose_unpack(c, R, t, nrm, stats);
  return VO_OK;
}

struct hpose_tail_args { const double* K; const vo_hpose_params* prm; };

// behind k_h4_finish on the search's stream: K up, the kernel on the search's own points, refined H and mask, the result into pinned memory
static int32_t hpose_tail(vo_ctx* c, hipStream_t q, const float* d_p, int cap, int n, const double* d_H, int h_stride, const uint8_t* d_mask, void* user) {
  const hpose_tail_args* a = (const hpose_tail_args*)user;
  vo_hpose_ws* w = c->hpose;
  VO_HIP(c, hipMemcpyAsync(w->d_K, a->K, sizeof(double) * 9 * c->batch, hipMemcpyHostToDevice, q));
  hpose_launch(c, q, d_H, h_stride, d_p, cap, d_mask, n, a->prm);
  VO_HIP(c, hipGetLastError());
  VO_HIP(c, hipMemcpyAsync(w->h_out, w->d_out, sizeof(double) * HP_OUT * c->batch, hipMemcpyDeviceToHost, q));
  return VO_OK;
}

extern "C" int32_t vo_homography_pose(vo_ctx* c, const double* K, const float* pts1, const float* pts2, int32_t n, const vo_hom_params* hom_prm,
                                      const vo_hpose_params* pose_prm, double* H, uint8_t* inlier_mask, double* R, double* t, double* nrm,
                                      vo_hom_stats* hom_stats, vo_hpose_stats* pose_stats) {
  if (!c) return VO_E_INVALID;
  vo_hpose_params def;
  if (!pose_prm) { vo_homography_pose_default_params(&def); pose_prm = &def; }
  VO_CHECK(c, K, VO_E_INVALID, "null buffer");
  VO_CHECK(c, n >= 0, VO_E_INVALID, "n < 0");
  int32_t r = hpose_check(c, pose_prm);
  if (r != VO_OK) return r;
  VO_HIP(c, hipSetDevice(c->device));
  r = hpose_alloc(c, 1);                                   // K and the result only: the points, H and the mask are the search's
  if (r != VO_OK) return r;
  hpose_tail_args args = {K, pose_prm};
  vo_hom_tail tail = {hpose_tail, &args};
  r = vo_hom_ransac_tail(c, pts1, pts2, n, hom_prm, H, nullptr, inlier_mask, hom_stats, &tail);
  if (r != VO_OK) return r;
  hpose_unpack(c, R, t, nrm, pose_stats);
  return VO_OK;
}
