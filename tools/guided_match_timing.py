"""Time of VoContext.match_guided (vo_match_guided_l2 / vo_match_guided_hamming) beside the plain matchers (match_knn2 / match_hamming_knn2) on
the same descriptor sets, in one process.

Sets: n1 = n2 = 1000 and 2000; SIFT-like float rows (dim 128, integer-valued 0..255) and random 256-bit rows; positions uniform over a
1241 x 376 image; F from a camera that moves sideways and forward with a small rotation.  Gates: none (gate 0), a window and an epipolar band
whose distances are the 5 % quantiles of the respective pair distance over a 400 x 400 sub-sample (the share the kernels admitted is printed
from n_admitted); each without and with cross-check (a second, reverse pass).
Two clocks.  `call`: the host clock around CALLS synchronous calls after WARM warm-up calls -- what a user waits for, uploads and read-backs
included; the plain matchers are timed the same way, the calls alternating over ROUNDS rounds, median and minimum printed.  `kernels`: hipEvent
pairs around the forward pass, the reverse pass and the accept kernel (vo_profile_enable, regions VO_PROF_GMATCH_*), in a separate loop so that
the events do not sit in the timed calls.  The plain matchers' launches carry no events: their kernel time is to be read from a kernel trace.
usage: tools/guided_match_timing.py"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-odom-pipeline_amd"))
import numpy as np
from vo_mi355x import VoContext, synthetic as syn

ROUNDS, WARM, CALLS = 5, 3, 10
W, H, SHARE = 1241.0, 376.0, 0.05
K = syn.KITTI_K


def fundamental():
    R, t = syn.rodrigues(np.array([0.02, -0.04, 0.01])), np.array([0.7, 0.2, -0.6])
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    Ki = np.linalg.inv(K)
    F = Ki.T @ tx @ R @ Ki
    return F / np.linalg.norm(F)


def epi_err(F, p1, p2):
    """sqrt of the larger squared point-to-epiline distance over all pairs, (n1, n2)"""
    x1 = np.concatenate([p1, np.ones((len(p1), 1))], 1).astype(np.float64); x2 = np.concatenate([p2, np.ones((len(p2), 1))], 1).astype(np.float64)
    l2, l1 = x1 @ F.T, x2 @ F                                      # lines in view 2 of the queries, in view 1 of the train rows
    d = x2 @ l2.T                                                   # (n2, n1): x2^T F x1
    e2 = (d * d).T / (l2[:, 0] ** 2 + l2[:, 1] ** 2)[:, None]
    e1 = (d * d).T / (l1[:, 0] ** 2 + l1[:, 1] ** 2)[None, :]
    return np.sqrt(np.maximum(e1, e2))


def sets(n, seed=3):
    rng = np.random.default_rng([seed, n])
    f1 = np.minimum(np.floor(rng.gamma(0.6, 30.0, (n, 128))), 255).astype(np.float32)
    f2 = np.minimum(np.floor(rng.gamma(0.6, 30.0, (n, 128))), 255).astype(np.float32)
    f2[:n // 2] = np.clip(f1[:n // 2] + rng.integers(-2, 3, (n // 2, 128)), 0, 255)
    b1 = rng.integers(0, 256, (n, 32), dtype=np.uint8); b2 = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    b2[:n // 2] = b1[:n // 2] ^ (rng.integers(0, 256, (n // 2, 32), dtype=np.uint8) & rng.integers(0, 256, (n // 2, 32), dtype=np.uint8) & 0x11)
    p1 = (rng.uniform(0, 1, (n, 2)) * (W, H)).astype(np.float32); p2 = (rng.uniform(0, 1, (n, 2)) * (W, H)).astype(np.float32)
    return f1, f2, b1, b2, p1, p2


def main():
    F = fundamental()
    for n in (1000, 2000):
        f1, f2, b1, b2, p1, p2 = sets(n)
        s1, s2 = p1[:400].astype(np.float64), p2[:400].astype(np.float64)
        radius = float(np.quantile(np.hypot(s2[None, :, 0] - s1[:, None, 0], s2[None, :, 1] - s1[:, None, 1]), SHARE))
        epi = float(np.quantile(epi_err(F, s1, s2), SHARE))
        gates = (("gate 0", {}), ("window %.1f px" % radius, dict(pts1=p1, pts2=p2, radius=radius)),
                 ("epipolar %.2f px" % epi, dict(pts1=p1, pts2=p2, F=F, epi_dist=epi)))
        with VoContext(64, 64, max_pts=64) as c:
            for kind, d1, d2, plain in (("L2 dim 128", f1, f2, c.match_knn2), ("Hamming 32 B", b1, b2, c.match_hamming_knn2)):
                calls = [("plain", lambda: plain(d1, d2))]
                for gname, kw in gates:
                    for cross in (False, True):
                        calls.append(("%s%s" % (gname, ", cross-check" if cross else ""), lambda kw=kw, cross=cross: c.match_guided(d1, d2, ratio=0.8, cross_check=cross, **kw)))
                times = {name: [] for name, _ in calls}
                last = {}
                for rnd in range(ROUNDS):
                    for name, fn in calls:
                        for k in range(WARM):
                            fn()
                        t0 = time.perf_counter()
                        for k in range(CALLS):
                            last[name] = fn()
                        times[name].append(1e6 * (time.perf_counter() - t0) / CALLS)
                regions = (c.PROF_GMATCH_FORWARD, c.PROF_GMATCH_REVERSE, c.PROF_GMATCH_ACCEPT)
                for name, fn in calls:
                    line = "n=%4d %-12s %-34s call: median %8.1f us, min %8.1f us" % (n, kind, name, np.median(times[name]), min(times[name]))
                    if name != "plain":
                        c.profile_enable(regions)
                        for k in range(CALLS):
                            fn()
                        us = [1e3 * c.profile_read(r)[0] / CALLS for r in regions]
                        c.profile_enable(())
                        r = last[name]
                        line += "; kernels: forward %8.1f us, reverse %8.1f us, accept %5.1f us; admitted %.4f, accepted %d" % (
                            us[0], us[1], us[2], r["n_admitted"].mean() / n, (r["match"] >= 0).sum())
                    print(line, flush=True)


if __name__ == "__main__":
    main()
