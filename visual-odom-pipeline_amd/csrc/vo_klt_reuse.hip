// The plain tracker with the target window kept while LK stays in one pixel cell: k_klt_track_r is k_klt_track (vo_klt.hip) around
// klt_lk_point<false, true> (vo_klt_lk.h).  Inside one pyramid level most LK iterations after the first, and the level-0 error pass, sample the
// target image at the integer cell of the sampling before them: only the four bilinear weights have moved.  k_klt_track loads and widens the
// 32 x 34-byte window again every time (8 buffer_load_dword, 1 ds_bpermute, 18 v_perm); here the widened rows wait in LDS (4608 bytes per
// one-wave workgroup) and are fetched again only when the cell changes.  The same bytes go through the same integer arithmetic: k_klt_track's bits.
// In a translation unit of its own, like vo_klt_seed.hip: co-compiled kernels perturb each other's register allocation, and k_klt_track /
// k_klt_track_fb are pinned.  Chosen by klt_launch_plain (vo_klt.hip; vo_tuning.klt_reuse).
#include "vo_klt_lk.h"

// WAVES = minimum waves per SIMD the register allocation must allow (see klt_launch_plain for the instance launched)
template <int WAVES>
__global__ void __launch_bounds__(64, WAVES) k_klt_track_r(klt_args A, const float* __restrict__ p0, float* __restrict__ p1,
                                                    uint8_t* __restrict__ status, float* __restrict__ err,
                                                    int32_t* __restrict__ iters, unsigned long long* __restrict__ dbg,
                                                    const int32_t* __restrict__ counts) {
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
  const bool dead = counts && pt >= counts[bseq];    // track table: this sequence has fewer live points
  if (iters && lane < A.iters_stride && (dead || lane > A.top)) iters[pt * A.iters_stride + lane] = -1;
  if (dead) return;
  p0 = vo_seq(p0, A.slab_seq, bseq); p1 = vo_seq(p1, A.slab_seq, bseq);
  status = vo_seq(status, A.slab_seq, bseq); err = vo_seq(err, A.slab_seq, bseq);
  unsigned long long* dbgk = (pt == A.n / 2 && bseq == 0 && dbg) ? dbg + 24 : nullptr;   // diagnostic stamps of one wave
  const float p0x = uniform_f(p0[2 * pt]), p0y = uniform_f(p0[2 * pt + 1]);
  float outx, outy, errv;
  int st;
  klt_lk_point<false, true>(A, A.lv, bseq, pt, lane, p0x, p0y, iters, dbgk, outx, outy, st, errv);
  if (lane == 0) {
    p1[2 * pt] = outx; p1[2 * pt + 1] = outy;
    status[pt] = (uint8_t)st;
    err[pt] = st ? errv : 0.f;
  }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
void vo_klt_launch_reuse(vo_ctx* c, const klt_launch_rows& L, const klt_args& A) {
  hipLaunchKernelGGL(k_klt_track_r<6>, dim3(L.n, c->batch), dim3(64), 0, L.q, A, L.p0, L.p1, L.status, L.err, c->d_iters, c->d_dbg, L.counts);
}
