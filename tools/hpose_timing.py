"""Time per call of VoContext.homography_pose (vo_homography_pose: the search with the decomposition enqueued behind it) beside
VoContext.find_homography followed by VoContext.decompose_homography on its H and inliers, and beside VoContext.essential_ransac, on the same
points, in one process; and the k_hpose launch on its own.

Points: the planar scene of the tests with 0.3 px noise and 30 % gross outliers; n = 200 and 2000, batch 1 and 64 (every sequence of a batch
gets the same points, so every sequence stops in the same round).  All calls are synchronous with their uploads and read-backs: the call a
user makes.  Time: host clock around CALLS calls after WARM warm-up calls, the calls alternating over ROUNDS rounds; median and minimum of
the rounds are printed.  The kernel's own time comes from hipEvent pairs around its launch (vo_profile_enable, region VO_PROF_HPOSE) in a
separate loop, so that the events do not sit in the timed calls.
usage: tools/hpose_timing.py"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-odom-pipeline_amd"))
import numpy as np
from vo_mi355x import VoContext, synthetic as syn

ROUNDS, WARM, CALLS = 5, 3, 20
K = syn.KITTI_K


def points(n, seed=2):
    rng = np.random.default_rng(seed)
    R, t = syn.rodrigues(np.array([0.01, 0.03, -0.005])), np.array([0.6, 0.1, -0.5])
    X = np.stack([rng.uniform(-15, 15, n), rng.uniform(-3, 3, n), np.zeros(n)], 1)
    X[:, 2] = 22.0 + 0.5 * X[:, 0] + 0.3 * X[:, 1]
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
            def two_calls():
                H, inl, st, _H0 = c.find_homography(q1, q2, seed=7)
                mask = np.zeros((B, n), np.uint8)
                for b in range(B):
                    mask[b, inl[b] if B > 1 else inl] = 1
                return c.decompose_homography(Ks, H, q1, q2, mask) + (st,)
            calls = (("homography_pose", lambda: c.homography_pose(Ks, q1, q2, seed=7), 2), ("find + decompose", two_calls, 4),
                     ("find_homography", lambda: c.find_homography(q1, q2, seed=7), 2), ("essential_ransac", lambda: c.essential_ransac(Ks, q1, q2, seed=7), 4))
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
                print("n=%4d B=%2d %-18s: median %9.1f us, min %9.1f us per call (%d rounds of %d calls); %d hypotheses, %d inliers"
                      % (n, B, name, np.median(times[name]), min(times[name]), ROUNDS, CALLS, st["hypotheses"], st["n_inliers"]), flush=True)
            ps = last["homography_pose"][6] if B == 1 else last["homography_pose"][6][0]
            print("n=%4d B=%2d   pose: n_mask %d, n_good %s, n_off %s, ambiguous %d" % (n, B, ps["n_mask"], ps["n_good"], ps["n_off"], ps["ambiguous"]), flush=True)
            c.profile_enable([c.PROF_HPOSE])
            for k in range(CALLS):
                c.homography_pose(Ks, q1, q2, seed=7)
            ms, cnt = c.profile_read(c.PROF_HPOSE)
            print("n=%4d B=%2d   k_hpose %4d launches in %d calls, %8.1f us per launch" % (n, B, cnt, CALLS, 1e3 * ms / max(cnt, 1)), flush=True)
            c.profile_enable(())
