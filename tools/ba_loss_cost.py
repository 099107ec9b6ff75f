"""Cost of the robust losses of the bundle adjustment, A/B in ONE process: the resident solve of a batch of 256 problems of 2 000
landmarks x window 10 (bench.py's BA shape, ~5 % outlier observations), per loss, in alternating regions; a fixed iteration count
(ftol = xtol = 0) so that every loss does the same number of LM iterations.

    python tools/ba_loss_cost.py [--batch 256] [--iters 10] [--regions 3] [--out FILE.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "visual-odom-pipeline_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

LOSSES = ("huber", "linear", "soft_l1", "cauchy", "arctan")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ba_loss_model as lm
    from vo_mi355x import VoContext
    probs = [lm.outlier_scene(2000, 10, s) for s in range(8)]          # 8 distinct problems dealt round-robin over the batch
    K = np.stack([probs[b % 8][0] for b in range(a.batch)]); P = np.stack([probs[b % 8][1] for b in range(a.batch)])
    X = np.stack([probs[b % 8][2] for b in range(a.batch)]); O = np.stack([probs[b % 8][3] for b in range(a.batch)])
    ms = {k: [] for k in LOSSES}
    with VoContext(64, 64, max_pts=64, batch=a.batch) as c:
        c.ba_upload(K, P, X, O)
        prm = {k: c.ba_params(max_iters=a.iters, ftol=0.0, xtol=0.0, gtol=0.0, loss=k) for k in LOSSES}
        for k in LOSSES:                                                   # warm-up
            c.ba_solve_resident(prm[k]); c.ba_fetch()
        for _ in range(a.regions):
            for k in LOSSES:
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    c.ba_solve_resident(prm[k])
                c.ba_fetch()
                ms[k].append(1e3 * (time.perf_counter() - t0) / a.reps)
    res = {k: dict(ms_per_solve=float(np.median(v)), ms_per_iter=float(np.median(v)) / a.iters, regions=v) for k, v in ms.items()}
    base = res["huber"]["ms_per_solve"]
    for k in LOSSES:
        res[k]["vs_huber"] = res[k]["ms_per_solve"] / base
        print("%-8s %8.3f ms per solve (%d iterations, batch %d x 2000 x W10)  %.3fx huber" % (k, res[k]["ms_per_solve"], a.iters, a.batch, res[k]["vs_huber"]))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
