"""Time per call of VoContext.find_fundamental (vo_fundamental_ransac) beside VoContext.essential_ransac and VoContext.find_homography on the
same points, in one process, and the split of the fundamental-matrix call over its kernels.

Points: synthetic correspondences of a scene with structure and a baseline, 0.3 px noise and 30 % gross outliers (the lines print the
hypotheses each search evaluated and its inliers; the homography finds only a dominant plane's worth); n = 200 and 2000, batch 1 and 64 (every
sequence of a batch gets the same points, so every sequence stops in the same round).  All three calls are synchronous with their uploads and
read-backs: the call a user makes.  Time: host clock around CALLS calls after WARM warm-up calls, the searches alternating over ROUNDS rounds;
median and minimum of the rounds are printed.  The per-kernel split comes from hipEvent pairs around each launch (vo_profile_enable, regions
VO_PROF_FUND_*) in a separate loop, so that the events do not sit in the timed calls.
usage: tools/fundamental_timing.py"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-odom-pipeline_amd"))
import numpy as np
from vo_mi355x import VoContext, synthetic as syn

ROUNDS, WARM, CALLS = 5, 3, 20
K = syn.KITTI_K


def points(n, seed=2):
    rng = np.random.default_rng(seed)
    R, t = syn.rodrigues(np.array([0.02, -0.04, 0.01])), np.array([0.7, 0.2, -0.6])
    X = np.stack([rng.uniform(-15, 15, n), rng.uniform(-3, 3, n), rng.uniform(8, 45, n)], 1)
    p1 = X @ K.T; p1 = p1[:, :2] / p1[:, 2:3] + rng.normal(0, 0.3, (n, 2))
    Xc = X @ R.T + t; p2 = Xc @ K.T; p2 = p2[:, :2] / p2[:, 2:3] + rng.normal(0, 0.3, (n, 2))
    out = rng.choice(n, int(0.3 * n), replace=False)
    p2[out] += rng.uniform(-60, 60, (len(out), 2)) + 10
    return p1.astype(np.float32), p2.astype(np.float32)


for n in (200, 2000):
    p1, p2 = points(n)
    for B in (1, 64):
        q1 = np.ascontiguousarray(np.broadcast_to(p1, (B, n, 2))) if B > 1 else p1
        q2 = np.ascontiguousarray(np.broadcast_to(p2, (B, n, 2))) if B > 1 else p2
        Ks = np.ascontiguousarray(np.broadcast_to(K, (B, 3, 3))) if B > 1 else K
        with VoContext(64, 64, max_pts=64, batch=B) as c:
            calls = (("find_fundamental", lambda: c.find_fundamental(q1, q2, seed=7), 2), ("find_fundamental refit", lambda: c.find_fundamental(q1, q2, seed=7, refit=1), 2),
                     ("essential_ransac", lambda: c.essential_ransac(Ks, q1, q2, seed=7), 4), ("find_homography", lambda: c.find_homography(q1, q2, seed=7), 2))
            times = {name: [] for name, _, _ in calls}
            last = {}
            for rnd in range(ROUNDS):
                for name, fn, _ in calls:
                    for k in range(WARM):
                        fn()
                    t0 = time.perf_counter()
                    for k in range(CALLS):
                        last[name] = fn()
                    times[name].append(1e6 * (time.perf_counter() - t0) / CALLS)
            for name, _, k in calls:
                st = last[name][k] if B == 1 else last[name][k][0]
                print("n=%4d B=%2d %-22s: median %9.1f us, min %9.1f us per call (%d rounds of %d calls); %d hypotheses, %d inliers"
                      % (n, B, name, np.median(times[name]), min(times[name]), ROUNDS, CALLS, st["hypotheses"], st["n_inliers"]), flush=True)
            regions = (("k_f7_solve", c.PROF_FUND_SOLVE), ("k_f7_score", c.PROF_FUND_SCORE), ("k_f7_select", c.PROF_FUND_SELECT), ("k_f7_finish", c.PROF_FUND_FINISH))
            c.profile_enable([r for _, r in regions])
            for k in range(CALLS):
                c.find_fundamental(q1, q2, seed=7, refit=1)
            for name, r in regions:
                ms, cnt = c.profile_read(r)
                print("n=%4d B=%2d   %-12s %4d launches in %d calls, %8.1f us per launch, %8.1f us per call" % (n, B, name, cnt, CALLS, 1e3 * ms / max(cnt, 1), 1e3 * ms / CALLS),
                      flush=True)
            c.profile_enable(())
