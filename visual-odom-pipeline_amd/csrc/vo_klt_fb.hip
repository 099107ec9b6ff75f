// Forward-backward consistency check of the pyramidal LK tracker (the standard outlier filter of KLT front ends, and what the reference's
// max_bidir_error promises: src/extractor/extractor.py:44-47,65-68 of the reference, with the image order of the second call fixed, as in
// the OpenCV sample it copies, notebooks/tracking.py:39-42):
//   p1, st, err = LK(prev, cur, p0)      bit for bit what k_klt_track returns
//   p0r         = LK(cur, prev, p1)      template = the CURRENT frame (image + Scharr derivatives, both already in the frame store)
//   fb_err      = max(|p0 - p0r|) over x, y (float32; NaN propagates)      ok = fb_err < max_err (NaN fails)
// k_klt_track_fb runs both passes in ONE launch, one wave per keypoint as k_klt_track: the backward pass starts from the wave's own p1, so
// nothing goes back to memory in between.  Both passes are the same per-level LK body, bound by vector-instruction issue like k_klt_track
// (DESIGN.md 4): the launch costs about two tracker launches.
//
// k_klt_track lives in its own translation unit and is not touched: co-compiled kernels perturb each other's register allocation.  The LK
// helpers are shared through vo_klt_lk.h (k_klt_track's ISA is unchanged by that); the per-level body below is k_klt_track's, made a function
// of the level images so that the kernel can run it twice.
#include "vo_klt_lk.h"

#include <math.h>

// the backward pass's levels: template image + derivatives of the current frame, target = the previous frame
struct klt_fb_args {
  klt_level_args bw[VO_MAX_LEVELS];
  size_t fb_seq;                 // byte stride between the sequences' rows of the check
  size_t off_err, off_ok;        // fb_err and ok rows (p0r at 0)
  float max_err;
};

// Pyramidal LK of the keypoint (p0x, p0y) (wave-uniform) through levels A.top .. 0 with template lv[l].imgI / derI and target lv[l].imgJ:
// k_klt_track's body.  Results are wave-uniform: outx, outy = nextPts, st = status, errv = the error before the status mask.  iters (this
// sequence's table) gets the iterations per level, or null.
__device__ __forceinline__ void klt_fb_point(const klt_args& A, const klt_level_args (&lv)[VO_MAX_LEVELS], int bseq, int pt, int lane,
                                             float p0x, float p0y, int32_t* iters, float& outx, float& outy, int& st, float& errv) {
  const int cp = lane & 15, r = lane >> 4;
  const int win = A.win;
  const float half = (float)(win - 1) * 0.5f;
  const float FLT_SCALE = 1.f / (float)(1 << 20);

  outx = 0.f; outy = 0.f;   // nextPts[pt]
  st = 1;
  errv = 0.f;

  // validity of the lane's two columns as 16-bit masks (lo = column 2cp, hi = column 2cp + 1)
  const uint32_t colmask = ((2 * cp < win) ? 0x0000FFFFu : 0u) | ((2 * cp + 1 < win) ? 0xFFFF0000u : 0u);
  const uint32_t colones = colmask & 0x00010001u;
  // v_perm selector "upper halves of (a, b)" with the constant-zero code 0x0c for the columns outside the window
  const uint32_t colsel = (0x07060302u & colmask) | (0x0c0c0c0cu & ~colmask);

  for (int level = A.top; level >= 0; level--) {
    klt_level_args L = lv[level];
    L.imgI += (size_t)bseq * L.seq_px; L.derI += (size_t)bseq * L.seq_px; L.imgJ += (size_t)bseq * L.seq_px;
    const float scale = __int_as_float((127 - level) << 23);       // 2^-level, exactly what 1.f / (float)(1 << level) gives (no division)
    float prevx = p0x * scale, prevy = p0y * scale;
    float nextx, nexty;
    if (level == A.top) { nextx = prevx; nexty = prevy; }
    else { nextx = outx * 2.f; nexty = outy * 2.f; }
    outx = nextx; outy = nexty;
    int n_it = -1;

    prevx -= half; prevy -= half;
    const float fpx = floorf(prevx), fpy = floorf(prevy);        // (float)(int)floorf(x) == floorf(x): the fraction needs no int -> float convert
    const int ipx = (int)fpx, ipy = (int)fpy;
    if (ipx < -win || ipx >= L.w || ipy < -win || ipy >= L.h) {
      if (level == 0) { st = 0; errv = 0.f; }
      if (iters && lane == 0) iters[pt * A.iters_stride + level] = n_it;
      continue;
    }
    const uint32_t lane_off = (uint32_t)(8 * r * L.pitch + 2 * cp);    // the lane's corner of the 32 x 34 footprint
    uint32_t wt, wb;
    lk_weights(prevx - fpx, prevy - fpy, wt, wb);

    // ---- template: packed pairs of I (5 frac bits), Ix, Iy for the lane's 16 pixels; exact A11, A12, A22 ----
    uint32_t tI[8], tX[8], tY[8];
    {
      uint32_t T[8], D0[8], D1[8], D2[8];
      // addresses = level base (scalar registers) + a 32-bit offset: the wave-uniform window origin, advanced per row on the
      // scalar unit, plus ONE per-lane offset that is fixed for the level (it was a chain of 64-bit vector adds per row)
      const uint32_t uo = (uint32_t)(ipy + VO_PAD) * (uint32_t)L.pitch + (uint32_t)(ipx + VO_PAD);
      const __amdgpu_buffer_rsrc_t rI = klt_rsrc(L.imgI), rD = klt_rsrc(L.derI);
#pragma unroll
      for (int s = 0; s < 8; s++) {
        const uint32_t o = uo + (uint32_t)s * (uint32_t)L.pitch;          // wave-uniform
        T[s] = __builtin_amdgcn_raw_buffer_load_b32(rI, (int)lane_off, (int)o, 0);
        // three consecutive pixels: one 12-byte load.  (8 bytes + the neighbour lane's first pixel through a DPP row shift was
        // measured: the same kernel time -- the data path is not priced per byte.)
        const u32x3 d3 = __builtin_amdgcn_raw_buffer_load_b96(rD, (int)(lane_off * 4u), (int)(o * 4u), 0);
        D0[s] = d3[0]; D1[s] = d3[1]; D2[s] = d3[2];
      }
      // row 8r + 8 = step 0 of row group r + 1 (lanes of r == 3 receive a row that only masked pixels use)
      const uint32_t T8 = row_next(T[0], lane), D08 = row_next(D0[0], lane), D18 = row_next(D1[0], lane), D28 = row_next(D2[0], lane);
      int a11 = 0, a12 = 0, a22 = 0;
#pragma unroll
      for (int s = 0; s < 8; s++) {
        const uint32_t B = (s < 7) ? T[(s + 1) & 7] : T8;
        const uint32_t E0 = (s < 7) ? D0[(s + 1) & 7] : D08;
        const uint32_t E1 = (s < 7) ? D1[(s + 1) & 7] : D18;
        const uint32_t E2 = (s < 7) ? D2[(s + 1) & 7] : D28;
        tI[s] = sample2(T[s], B, wt, wb);
        const uint32_t x0 = deriv1(pack_lo(D0[s], D1[s]), pack_lo(E0, E1), wt, wb);
        const uint32_t y0 = deriv1(pack_hi(D0[s], D1[s]), pack_hi(E0, E1), wt, wb);
        const uint32_t x1 = deriv1(pack_lo(D1[s], D2[s]), pack_lo(E1, E2), wt, wb);
        const uint32_t y1 = deriv1(pack_hi(D1[s], D2[s]), pack_hi(E1, E2), wt, wb);
        const uint32_t sel = (8 * r + s < win) ? colsel : 0x0c0c0c0cu;    // rows / columns outside the window contribute nothing
        const uint32_t xp = __builtin_amdgcn_perm(x1, x0, sel), yp = __builtin_amdgcn_perm(y1, y0, sel);
        tX[s] = xp; tY[s] = yp;
        // the first step starts the three sums from an inline zero (three-address form: no preload)
        a11 = s ? dot2(xp, xp, a11) : dot2k(xp, xp, 0);
        a12 = s ? dot2(xp, yp, a12) : dot2k(xp, yp, 0);
        a22 = s ? dot2(yp, yp, a22) : dot2k(yp, yp, 0);
      }
      float A11, A12, A22;
      {
        // per lane 16 products of two int16 derivatives (|Scharr| <= 4080): < 2^28.01, a quad's sum < 2^30.01
        int l11, h11, l12, h12, l22, h22;
        wave_sum3_wide(a11, a12, a22, lane, l11, h11, l12, h12, l22, h22);
        A11 = klt_combine(h11, l11) * FLT_SCALE; A12 = klt_combine(h12, l12) * FLT_SCALE; A22 = klt_combine(h22, l22) * FLT_SCALE;
      }
      float D = A11 * A22 - A12 * A12;
      // minEig = num / (2 win^2) < minEigThreshold, decided on the numerator (threshold pre-divided exactly on the host)
      const float num = A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12);
      if (num < A.min_eig_num || D < 1.1920929e-07f) {
        if (level == 0) st = 0;
        if (iters && lane == 0) iters[pt * A.iters_stride + level] = n_it;
        continue;
      }
      D = 1.f / D;

      nextx -= half; nexty -= half;
      const __amdgpu_buffer_rsrc_t rJ = klt_rsrc(L.imgJ);
      float pdx = 0.f, pdy = 0.f;
      int j = 0;
      for (; j < A.max_count; j++) {
        const float fnx = floorf(nextx), fny = floorf(nexty);
        const int inx = (int)fnx, iny = (int)fny;
        if (inx < -win || inx >= L.w || iny < -win || iny >= L.h) {
          if (level == 0) st = 0;
          break;
        }
        uint32_t jt, jb;
        lk_weights(nextx - fnx, nexty - fny, jt, jb);
        uint32_t Tj[8];
        const uint32_t uj = (uint32_t)(iny + VO_PAD) * (uint32_t)L.pitch + (uint32_t)(inx + VO_PAD);
#pragma unroll
        for (int s = 0; s < 8; s++) Tj[s] = __builtin_amdgcn_raw_buffer_load_b32(rJ, (int)lane_off, (int)(uj + (uint32_t)s * (uint32_t)L.pitch), 0);
        const uint32_t Tj8 = row_next(Tj[0], lane);
        int b1 = 0, b2 = 0;
#pragma unroll
        for (int s = 0; s < 8; s++) {
          const uint32_t B = (s < 7) ? Tj[(s + 1) & 7] : Tj8;
          const uint32_t d = pk_sub(sample2(Tj[s], B, jt, jb), tI[s]);   // (diff0 | diff1 << 16), |diff| <= 8160
          b1 = s ? dot2(d, tX[s], b1) : dot2k(d, tX[0], 0);
          b2 = s ? dot2(d, tY[s], b2) : dot2k(d, tY[0], 0);
        }
        // per lane 16 products |diff| <= 8160 (255 << 5) times |derivative| <= 4080: < 2^28.99, a quad's sum < 2^30.99
        int l1, h1, l2, h2;
        wave_sum2_wide(b1, b2, lane, l1, h1, l2, h2);
        const float fb1 = klt_combine(h1, l1) * FLT_SCALE;
        const float fb2 = klt_combine(h2, l2) * FLT_SCALE;
        const float dx = (A12 * fb2 - A22 * fb1) * D;
        const float dy = (A12 * fb1 - A11 * fb2) * D;
        nextx += dx; nexty += dy;
        outx = nextx + half; outy = nexty + half;
        // |delta|^2 <= eps^2 is OpenCV's float64 test; its float32 value is within 2^-22 of it, so only a value between the
        // two guard constants needs the float64 evaluation
        const float d2 = dx * dx + dy * dy;
        bool conv;
        if (d2 < A.eps_lo) conv = true;
        else if (d2 > A.eps_hi) conv = false;
        else conv = (double)dx * (double)dx + (double)dy * (double)dy <= A.eps2;
        if (conv) { j++; break; }
        // fabs((double)x) < 0.01 for a float x  <=>  fabsf(x) <= (float)0.01: 0.01 lies strictly between that float and the next
        if (j > 0 && fabsf(dx + pdx) <= 0.01f && fabsf(dy + pdy) <= 0.01f) {
          outx -= dx * 0.5f; outy -= dy * 0.5f;
          j++;
          break;
        }
        pdx = dx; pdy = dy;
      }
      n_it = j;
      if (iters && lane == 0) iters[pt * A.iters_stride + level] = n_it;

      if (st && level == 0) {
        const float nx = outx - half, ny = outy - half;
        const float fnx = floorf(nx), fny = floorf(ny);
        const int inx = (int)fnx, iny = (int)fny;
        if (inx < -win || inx >= L.w || iny < -win || iny >= L.h) {
          st = 0;
        } else {
          uint32_t jt, jb;
          lk_weights(nx - fnx, ny - fny, jt, jb);
          uint32_t Tj[8];
          const uint32_t uj = (uint32_t)(iny + VO_PAD) * (uint32_t)L.pitch + (uint32_t)(inx + VO_PAD);
#pragma unroll
          for (int s = 0; s < 8; s++) Tj[s] = __builtin_amdgcn_raw_buffer_load_b32(rJ, (int)lane_off, (int)(uj + (uint32_t)s * (uint32_t)L.pitch), 0);
          const uint32_t Tj8 = row_next(Tj[0], lane);
          int e = 0;
#pragma unroll
          for (int s = 0; s < 8; s++) {
            const uint32_t B = (s < 7) ? Tj[(s + 1) & 7] : Tj8;
            const uint32_t d = pk_abs(pk_sub(sample2(Tj[s], B, jt, jb), tI[s]));
            const uint32_t ones = (8 * r + s < win) ? colones : 0u;
            e = s ? dot2(d, ones, e) : dot2k(d, ones, 0);
          }
          const int ierr = wave_sum_i32(e);
          errv = (float)ierr * 1.f / (float)(32 * win * win);
        }
      }
    }
  }
}

// WAVES = minimum waves per SIMD the register allocation must allow: ONE instantiation, 6 (k_klt_track's default; 80 VGPRs, no scratch)
template <int WAVES>
__global__ void __launch_bounds__(64, WAVES) k_klt_track_fb(klt_args A, klt_fb_args F, const float* __restrict__ p0, float* __restrict__ p1,
                                                     uint8_t* __restrict__ status, float* __restrict__ err, int32_t* __restrict__ iters,
                                                     const int32_t* __restrict__ counts, uint8_t* __restrict__ fb) {
  int pt = blockIdx.x, bseq = blockIdx.y;
  if (A.xcd_remap) {             // one sequence per XCD (k_klt_track)
    const unsigned id = blockIdx.y * gridDim.x + blockIdx.x;
    const unsigned q = id >> 3;
    bseq = (int)(id & 7u) + 8 * (int)(q / (unsigned)A.n);
    pt = (int)(q % (unsigned)A.n);
  }
  if (pt >= A.n) return;
  const int lane = threadIdx.x;
  if (iters) iters += (size_t)bseq * A.iters_seq;
  fb += (size_t)bseq * F.fb_seq;
  float* const p0r = reinterpret_cast<float*>(fb);
  float* const fb_err = reinterpret_cast<float*>(fb + F.off_err);
  uint8_t* const ok = fb + F.off_ok;
  const bool dead = counts && pt >= counts[bseq];    // track table: this sequence has fewer live points
  if (iters && lane < A.iters_stride && (dead || lane > A.top)) iters[pt * A.iters_stride + lane] = -1;
  if (dead) {                                        // a dead slot is never good (its check reads as NaN)
    if (lane == 0) { p0r[2 * pt] = p0r[2 * pt + 1] = fb_err[pt] = __builtin_nanf(""); ok[pt] = 0; }
    return;
  }
  p0 = vo_seq(p0, A.slab_seq, bseq); p1 = vo_seq(p1, A.slab_seq, bseq);
  status = vo_seq(status, A.slab_seq, bseq); err = vo_seq(err, A.slab_seq, bseq);

  const float p0x = uniform_f(p0[2 * pt]), p0y = uniform_f(p0[2 * pt + 1]);
  float outx, outy, errv;
  int st;
  klt_fb_point(A, A.lv, bseq, pt, lane, p0x, p0y, iters, outx, outy, st, errv);
  if (lane == 0) {
    p1[2 * pt] = outx; p1[2 * pt + 1] = outy;
    status[pt] = (uint8_t)st;
    err[pt] = st ? errv : 0.f;
  }
  // backward from the tracked position whatever its status (the reference hands every p1 to the second call)
  float rx, ry, rerr;
  int rst;
  klt_fb_point(A, F.bw, bseq, pt, lane, outx, outy, nullptr, rx, ry, rst, rerr);
  if (lane == 0) {
    const float ex = fabsf(p0x - rx), ey = fabsf(p0y - ry);
    const float e = (ex != ex || ey != ey) ? __builtin_nanf("") : (ex >= ey ? ex : ey);     // numpy's max: NaN propagates
    p0r[2 * pt] = rx; p0r[2 * pt + 1] = ry;
    fb_err[pt] = e;
    ok[pt] = (e < F.max_err) ? 1 : 0;
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static int32_t fb_reserve(vo_ctx* c) {
  if (c->d_fb) return VO_OK;
  auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t M = (size_t)c->max_pts;
  c->fb_off_err = al(8 * M); c->fb_off_ok = c->fb_off_err + al(4 * M); c->fb_seq = c->fb_off_ok + al(M);
  VO_HIP(c, hipMalloc((void**)&c->d_fb, c->fb_seq * (size_t)c->batch));
  return VO_OK;
}

void vo_fb_destroy(vo_ctx* c) {
  if (c->d_fb) (void)hipFree(c->d_fb);
  c->d_fb = nullptr;
}

static int32_t fb_launch(vo_ctx* c, int n, const vo_klt_params* prm, size_t off_in, size_t off_out, const int32_t* counts) {
  c->fb_n = -1;
  klt_args A;
  { const int32_t r = vo_klt_make_args(c, n, prm, A); if (r != VO_OK) return r; }
  if (n == 0) { c->fb_n = 0; return VO_OK; }
  { const int32_t r = fb_reserve(c); if (r != VO_OK) return r; }
  klt_fb_args F;
  const vo_frame& P = c->fr[c->cur ^ 1];
  const vo_frame& C = c->fr[c->cur];
  for (int l = 0; l <= A.top; l++) {
    F.bw[l] = A.lv[l];
    F.bw[l].imgI = C.img[l]; F.bw[l].derI = reinterpret_cast<const uint32_t*>(C.der[l]); F.bw[l].imgJ = P.img[l];
  }
  F.fb_seq = c->fb_seq; F.off_err = c->fb_off_err; F.off_ok = c->fb_off_ok;
  F.max_err = c->fb_max_err;
  {
    vo_prof_scope prof(c, VO_PROF_KLT);
    hipLaunchKernelGGL(k_klt_track_fb<6>, dim3(n, c->batch), dim3(64), 0, c->stream, A, F, vo_slab<const float>(c, off_in),
                       vo_slab<float>(c, off_out), vo_slab<uint8_t>(c, c->off_status), vo_slab<float>(c, c->off_err), c->d_iters, counts, c->d_fb);
  }
  VO_HIP(c, hipGetLastError());
  c->fb_n = n;
  return VO_OK;
}

static hipError_t rows_d2h(vo_ctx* c, void* h, const uint8_t* d, size_t d_stride, size_t row_bytes) {
  return hipMemcpy2DAsync(h, row_bytes, d, d_stride, row_bytes, c->batch, hipMemcpyDeviceToHost, c->stream);
}

extern "C" int32_t vo_klt_track_fb(vo_ctx* c, const float* p0, int32_t n, const vo_klt_params* prm, float* p1, uint8_t* status, float* err,
                                   float* p0r, float* fb_err, int32_t* iters) {
  if (!c) return VO_E_INVALID;
  vo_klt_params def;
  if (!prm) { vo_klt_default_params(&def); prm = &def; }
  VO_CHECK(c, n >= 0 && n <= c->max_pts, VO_E_CAPACITY, "n exceeds max_pts");
  if (n == 0) return VO_OK;
  VO_CHECK(c, p0 && p1 && status && err && p0r && fb_err, VO_E_INVALID, "null buffer");
  VO_HIP(c, hipSetDevice(c->device));
  { const int32_t rq = vo_quiesce_side(c); if (rq != VO_OK) return rq; }
  const size_t off_in = vo_off_p(c), off_out = vo_off_p_next(c);
  VO_HIP(c, hipMemcpy2DAsync(c->d_slab + off_in, c->slab_seq, p0, sizeof(float) * 2 * n, sizeof(float) * 2 * n, c->batch,
                             hipMemcpyHostToDevice, c->stream));
  const int32_t r = fb_launch(c, n, prm, off_in, off_out, nullptr);
  if (r != VO_OK) return r;
  VO_HIP(c, rows_d2h(c, p1, c->d_slab + off_out, c->slab_seq, sizeof(float) * 2 * n));
  VO_HIP(c, rows_d2h(c, status, c->d_slab + c->off_status, c->slab_seq, n));
  VO_HIP(c, rows_d2h(c, err, c->d_slab + c->off_err, c->slab_seq, sizeof(float) * n));
  VO_HIP(c, rows_d2h(c, p0r, c->d_fb, c->fb_seq, sizeof(float) * 2 * n));
  VO_HIP(c, rows_d2h(c, fb_err, c->d_fb + c->fb_off_err, c->fb_seq, sizeof(float) * n));
  if (iters) {
    const size_t row = sizeof(int32_t) * (size_t)n * (prm->max_level + 1);
    VO_HIP(c, hipMemcpy2DAsync(iters, row, c->d_iters, sizeof(int32_t) * (size_t)c->max_pts * VO_MAX_LEVELS, row, c->batch,
                               hipMemcpyDeviceToHost, c->stream));
  }
  VO_HIP(c, hipStreamSynchronize(c->stream));
  return VO_OK;
}

// the resident form (vo_tracks_track, the closed loop's TRACK stage): vo_klt_track_resident_counts with the check
int32_t vo_klt_track_resident_fb(vo_ctx* c, int32_t n, const vo_klt_params* prm, const int32_t* d_counts) {
  vo_klt_params def;
  if (!prm) { vo_klt_default_params(&def); prm = &def; }
  VO_CHECK(c, n >= 0 && n <= c->n_resident, VO_E_INVALID, "n exceeds the resident point set");
  VO_HIP(c, hipSetDevice(c->device));
  { const int32_t rq = vo_quiesce_side(c); if (rq != VO_OK) return rq; }
  const int32_t r = fb_launch(c, n, prm, vo_off_p(c), vo_off_p_next(c), d_counts);
  if (r != VO_OK) return r;
  c->p_parity ^= 1;   // tracked positions become the resident set
  return VO_OK;
}

extern "C" int32_t vo_set_fb_check(vo_ctx* c, float max_err) {
  if (!c) return VO_E_INVALID;
  VO_CHECK(c, max_err == max_err, VO_E_INVALID, "NaN threshold (+inf turns the check off)");
  if (!(max_err == __builtin_inff())) {       // the rows of the check exist before the first enqueue that needs them
    VO_HIP(c, hipSetDevice(c->device));
    const int32_t r = fb_reserve(c);
    if (r != VO_OK) return r;
  }
  c->fb_max_err = max_err;
  return VO_OK;
}

extern "C" int32_t vo_get_fb_check(vo_ctx* c, float* max_err) {
  if (!c || !max_err) return VO_E_INVALID;
  *max_err = c->fb_max_err;
  return VO_OK;
}

extern "C" int32_t vo_fb_read(vo_ctx* c, uint8_t* ok, float* fb_err, int32_t n) {
  if (!c) return VO_E_INVALID;
  VO_CHECK(c, !vo_pipe_busy(c) && c->steps_enq == c->steps_fetched, VO_E_STATE, "steps in flight: fetch them first");
  VO_CHECK(c, c->fb_n >= 0, VO_E_STATE, "the last track ran without the forward-backward check");
  VO_CHECK(c, n >= 0 && n <= c->fb_n, VO_E_INVALID, "n exceeds the points of the last track");
  VO_HIP(c, hipSetDevice(c->device));
  { const int32_t rq = vo_quiesce_side(c); if (rq != VO_OK) return rq; }
  if (n > 0) {
    if (ok) VO_HIP(c, rows_d2h(c, ok, c->d_fb + c->fb_off_ok, c->fb_seq, n));
    if (fb_err) VO_HIP(c, rows_d2h(c, fb_err, c->d_fb + c->fb_off_err, c->fb_seq, sizeof(float) * n));
  }
  VO_HIP(c, hipStreamSynchronize(c->stream));
  return VO_OK;
}
