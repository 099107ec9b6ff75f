"""Time per call of VoContext.estimate_sim3 (vo_sim3_ransac) and VoContext.fit_sim3 beside VoContext.find_homography and
VoContext.find_fundamental on the same point count, in one process, and the split of the Sim(3) call over its kernels.

Points: for the Sim(3) search a cloud of n 3-D points with its copy under a similarity, 1e-3 noise and 30 % gross outliers; for the two 2-D
searches synthetic correspondences of a scene with structure and a baseline, 0.3 px noise and 30 % gross outliers (the lines print the
hypotheses each search evaluated and its inliers); n = 200 and 2000, batch 1 and 64 (every sequence of a batch gets the same points, so every
sequence stops in the same round).  All calls are synchronous with their uploads and read-backs: the call a user makes.  Time: host clock
around CALLS calls after WARM warm-up calls, the searches alternating over ROUNDS rounds; median and minimum of the rounds are printed.  The
per-kernel split comes from hipEvent pairs around each launch (vo_profile_enable, regions VO_PROF_SIM3_*) in a separate loop, so that the
events do not sit in the timed calls.
usage: tools/sim3_timing.py"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-odom-pipeline_amd"))
import numpy as np
from vo_mi355x import VoContext, synthetic as syn

ROUNDS, WARM, CALLS = 5, 3, 20
K = syn.KITTI_K


def points2d(n, seed=2):
    rng = np.random.default_rng(seed)
    R, t = syn.rodrigues(np.array([0.02, -0.04, 0.01])), np.array([0.7, 0.2, -0.6])
    X = np.stack([rng.uniform(-15, 15, n), rng.uniform(-3, 3, n), rng.uniform(8, 45, n)], 1)
    p1 = X @ K.T; p1 = p1[:, :2] / p1[:, 2:3] + rng.normal(0, 0.3, (n, 2))
    Xc = X @ R.T + t; p2 = Xc @ K.T; p2 = p2[:, :2] / p2[:, 2:3] + rng.normal(0, 0.3, (n, 2))
    out = rng.choice(n, int(0.3 * n), replace=False)
    p2[out] += rng.uniform(-60, 60, (len(out), 2)) + 10
    return p1.astype(np.float32), p2.astype(np.float32)


def points3d(n, seed=2):
    rng = np.random.default_rng(seed)
    R, t, s = syn.rodrigues(np.array([0.3, -0.7, 0.4])), np.array([2.0, -1.0, 4.0]), 1.7
    X = rng.uniform(-10, 10, (n, 3))
    Y = s * (X @ R.T) + t + rng.normal(0, 1e-3, (n, 3))
    out = rng.choice(n, int(0.3 * n), replace=False)
    Y[out] = rng.uniform(-60, 60, (len(out), 3))
    return X.astype(np.float32), Y.astype(np.float32)


for n in (200, 2000):
    p1, p2 = points2d(n)
    x, y = points3d(n)
    for B in (1, 64):
        rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape)) if B > 1 else a
        q1, q2, xs, ys = rep(p1), rep(p2), rep(x), rep(y)
        with VoContext(64, 64, max_pts=64, batch=B) as c:
            calls = (("estimate_sim3", lambda: c.estimate_sim3(xs, ys, threshold=0.1, seed=7), 4), ("estimate_sim3 refit=0", lambda: c.estimate_sim3(xs, ys, threshold=0.1, seed=7, refit=0), 4),
                     ("fit_sim3", lambda: c.fit_sim3(xs, ys), 3), ("find_homography", lambda: c.find_homography(q1, q2, seed=7), 2),
                     ("find_fundamental", lambda: c.find_fundamental(q1, q2, seed=7), 2))
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
            regions = (("k_s3_solve", c.PROF_SIM3_SOLVE), ("k_s3_score", c.PROF_SIM3_SCORE), ("k_s3_select", c.PROF_SIM3_SELECT), ("k_s3_finish", c.PROF_SIM3_FINISH))
            c.profile_enable([r for _, r in regions])
            for k in range(CALLS):
                c.estimate_sim3(xs, ys, threshold=0.1, seed=7)
            for name, r in regions:
                ms, cnt = c.profile_read(r)
                print("n=%4d B=%2d   %-12s %4d launches in %d calls, %8.1f us per launch, %8.1f us per call" % (n, B, name, cnt, CALLS, 1e3 * ms / max(cnt, 1), 1e3 * ms / CALLS),
                      flush=True)
            c.profile_enable(())
