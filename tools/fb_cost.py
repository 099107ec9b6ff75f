"""Cost of the forward-backward KLT check (csrc/vo_klt_fb.hip), A/B in ONE process: regions with the check off and on alternate.

  track table  256 sequences x 1241x376 x 2 000 points: vo_tracks_track, the tracker launch timed by in-stream events (VO_PROF_KLT brackets
               k_klt_track or k_klt_track_fb) and the whole call to a device synchronise
  closed loop  bench.py's shape (256 sequences in one context, window 10, resident frames, 3 steps in flight): frames per second

    python tools/fb_cost.py [--batch 256] [--regions 4] [--out FILE.json]
    python tools/fb_cost.py --kstats        (a short track-table run only, for rocprofv3 --kernel-trace --stats)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "visual-odom-pipeline_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

W, H = 1241, 376
PROF_KLT = 1


def track_table(batch, n_pts, regions, reps, thr):
    from vo_mi355x import VoContext, synthetic as syn
    seqs = [syn.make_sequence(2, seed=500 + k)[0] for k in range(8)]          # 8 distinct pairs, dealt round-robin over the batch
    frames = np.stack([seqs[b % 8] for b in range(batch)])
    pts = np.stack([syn.grid_points(n_pts, W, H, seed=60 + b % 8) for b in range(batch)])
    out = {"off": {"kernel_ms": [], "call_ms": []}, "on": {"kernel_ms": [], "call_ms": []}}
    with VoContext(W, H, max_pts=n_pts, batch=batch) as c:
        c.upload_sequence(frames)

        def once(fb):
            c.set_fb_check(thr if fb else np.inf)
            c.push_frame_resident(0); c.push_frame_resident(1)
            c.tracks_seed(pts, t=0)
            c.sync()
            t0 = time.perf_counter()
            c.tracks_track(1)
            c.sync()
            return time.perf_counter() - t0

        for fb in (False, True):                                             # warm-up of both shapes
            once(fb)
        for r in range(regions):
            for mode in ("off", "on"):
                c.profile_enable((PROF_KLT,))
                calls = [once(mode == "on") for _ in range(reps)]
                ms, n = c.profile_read(PROF_KLT)
                c.profile_enable(())
                out[mode]["kernel_ms"].append(ms / max(n, 1))
                out[mode]["call_ms"].append(1e3 * float(np.median(calls)))
        ok, _ = c.fb_read(n_pts)
    rej = 1.0 - float(np.mean(ok))
    return out, rej


def closed_loop(batch, window, regions, steps, warmup, thr):
    import bench
    from vo_mi355x import VoContext
    scenes = bench.pipe_scenes(2, 40, 4321)
    boot = VoContext(bench.W_IMG, bench.H_IMG, max_pts=4096)
    g = bench.PipeGroup(0, scenes, boot, 0, batch, 10, 2048, False, window, True)
    out = {"off": [], "on": []}
    for _ in range(warmup):
        g.step()
    g.drain()
    for r in range(regions):
        for mode in ("off", "on"):
            g.c.set_fb_check(thr if mode == "on" else np.inf)
            for _ in range(3):                                              # the switch's own frames are not timed
                g.step()
            g.drain()
            t0 = time.perf_counter()
            for _ in range(steps):
                g.step()
            g.drain()
            out[mode].append(batch * steps / (time.perf_counter() - t0))
    lost = sum(int(r["status"] != 0) for r in g.last)
    return out, lost


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--pts", type=int, default=2000)
    ap.add_argument("--window", type=int, default=10)
    ap.add_argument("--regions", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--thr", type=float, default=1.0)
    ap.add_argument("--kstats", action="store_true", help="a short track-table run only (kernel statistics under rocprofv3)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kstats:
        track_table(a.batch, a.pts, 1, 3, a.thr)
        return
    res = {"batch": a.batch, "pts": a.pts, "window": a.window, "thr": a.thr}
    tt, rej = track_table(a.batch, a.pts, a.regions, a.reps, a.thr)
    res["track_table"] = {m: {k: [round(x, 4) for x in v] for k, v in d.items()} for m, d in tt.items()}
    res["track_table"]["rejected_share"] = round(rej, 4)
    res["track_table"]["kernel_ratio"] = round(float(np.median(tt["on"]["kernel_ms"]) / np.median(tt["off"]["kernel_ms"])), 3)
    cl, lost = closed_loop(a.batch, a.window, a.regions, a.steps, a.warmup, a.thr)
    res["closed_loop_fps"] = {m: [round(x, 1) for x in v] for m, v in cl.items()}
    res["closed_loop_fps"]["ratio_on_off"] = round(float(np.median(cl["on"]) / np.median(cl["off"])), 3)
    res["closed_loop_fps"]["lost_sequences"] = lost
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
