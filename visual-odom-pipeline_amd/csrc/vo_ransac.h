// What the five RANSAC searches (vo_pnp.hip, vo_essential.hip, vo_homography.hip, vo_fundamental.hip, vo_sim3.hip) have in common, in one place:
//   device  the counter-based splitmix64 sample generator, OpenCV's iteration bound, the head of a sequence's control block (bound,
//           hypotheses done, done flag) with its reset, and the tail of a select kernel: the winner of a batch and the advance of the head
//   host    the round loop of the synchronous entry points: enqueue a round, read the control blocks back, stop when every sequence is done
// The generator and the bound are part of each search's definition: oracle/pnp_oracle.py, oracle/essential_oracle.py,
// tests/homography_model.py, tests/fundamental_model.py and tests/sim3_model.py each carry their own copy and are compared with the device
// hypothesis by hypothesis.
// What only the two-view units share -- workspace, upload and read-back, the passes of the finish kernels with their 45-sum reduction and
// the 9 x 9 eigenvector -- is vo_twoview.h, on top of this header; PnP needs none of it.
#pragma once
#include "vo_internal.h"

#include <stddef.h>

__device__ __forceinline__ unsigned long long vo_splitmix64(unsigned long long x) {
  x += 0x9E3779B97F4A7C15ull;
  unsigned long long z = x;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// M distinct indices in [0, n), n >= M, of hypothesis h: draw k is splitmix64(seed, h, k) mod n, a draw that repeats an index is skipped
// (M = 4: sample4(seed, h, n) of oracle/pnp_oracle.py and tests/homography_model.py, M = 5: sample5 of oracle/essential_oracle.py, M = 7: sample7 of tests/fundamental_model.py,
// M = 3: sample3 of tests/sim3_model.py)
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

__device__ inline int vo_ransac_update_iters(double p, double ep, int model_points, int max_iters) {   // OpenCV RANSACUpdateNumIters (calib3d/ptsetreg.cpp)
  p = fmin(fmax(p, 0.0), 1.0); ep = fmin(fmax(ep, 0.0), 1.0);
  double num = fmax(1.0 - p, 2.2250738585072014e-308);
  double denom = 1.0 - pow(1.0 - ep, (double)model_points);
  if (denom < 2.2250738585072014e-308) return 0;
  num = log(num); denom = log(denom);
  return (denom >= 0 || -num >= max_iters * (-denom)) ? max_iters : (int)rint(num / denom);
}

// Head of a search's per-sequence control block (its first member `s`): the iteration bound, the hypotheses evaluated, bound reached.
// The closed loop reads the PnP block as int32 words (vo_pnp_view::ctrl): these are the words' indices.
struct vo_ransac_state { int niters, h_done, done; };
enum { VO_RANSAC_WORD_H_DONE = 1, VO_RANSAC_WORD_DONE = 2 };
static_assert(offsetof(vo_ransac_state, h_done) == sizeof(int32_t) * VO_RANSAC_WORD_H_DONE &&
              offsetof(vo_ransac_state, done) == sizeof(int32_t) * VO_RANSAC_WORD_DONE && sizeof(vo_ransac_state) == 12, "vo_ransac_state layout");

__device__ inline void vo_ransac_reset(vo_ransac_state* s, int max_iters) { s->niters = max_iters; s->h_done = 0; s->done = 0; }

// The batch's winner: the slot of the largest cnt[0..nb) strictly above `floor` (the running best's count), the first such slot on a
// tie -- batch order is ascending h; -1 if none is
__device__ inline int vo_ransac_best_slot(const int* cnt, int nb, int floor) {
  int bi = -1;
  for (int i = 0; i < nb; i++) if (cnt[i] > floor) { floor = cnt[i]; bi = i; }
  return bi;
}

// After a batch of nb hypotheses on n correspondences: count them, tighten the bound by the running best (if there is one), raise done
__device__ inline void vo_ransac_advance(vo_ransac_state* s, int nb, int n, int best_count, bool have_best, double conf, int model_points, int max_iters) {
  s->h_done += nb;
  if (have_best) {
    const int ni = vo_ransac_update_iters(conf, (double)(n - best_count) / (double)n, model_points, max_iters);
    if (ni < s->niters) s->niters = ni;
  }
  s->done = (s->h_done >= s->niters) ? 1 : 0;
}

// Host: up to max_rounds rounds on stream q.  enqueue_round(round) launches one round's kernels; the B control blocks (Ctrl: a block
// that starts with `vo_ransac_state s`) are then read back into the pinned h_ctrl, and the loop ends when every sequence is done.
template <class Ctrl, class Enqueue>
inline int32_t vo_ransac_rounds(vo_ctx* c, hipStream_t q, const Ctrl* d_ctrl, Ctrl* h_ctrl, size_t B, int max_rounds, Enqueue enqueue_round) {
  static_assert(offsetof(Ctrl, s) == 0, "the control block starts with its vo_ransac_state");
  for (int round = 0; round < max_rounds; round++) {
    enqueue_round(round);
    VO_HIP(c, hipGetLastError());
    VO_HIP(c, hipMemcpyAsync(h_ctrl, d_ctrl, sizeof(Ctrl) * B, hipMemcpyDeviceToHost, q));
    VO_HIP(c, hipStreamSynchronize(q));
    bool all = true;
    for (size_t b = 0; b < B; b++) all = all && h_ctrl[b].s.done;
    if (all) break;
  }
  return VO_OK;
}
