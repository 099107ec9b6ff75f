"""Time of VoContext.depth_update (vo_depth_update) at 1241 x 376 with 2000 seeds, batch 1 and batch 256, beside VoContext.klt_track of the
same point count: the k_depth_update launch alone from hipEvent pairs (vo_profile_enable, region VO_PROF_DEPTH; the tracker's launch from
VO_PROF_KLT), and the whole synchronous call with its uploads and read-backs from the host clock.  Split by the length of the epipolar
segments: fresh seeds (sigma a sixth of the inverse-depth range), seeds after three updates, and nearly converged ones.

Frames: synthetic.sway_scene with its true poses; seeds: random pixels of frame 0.  The seeds of a timed call are always the same input
rows (the call updates a copy), so every call does the same work.  ROUNDS rounds of CALLS calls after WARM warm-up calls; median and minimum
of the rounds.  Every step runs in a child process of its own under `timeout`; the first step that fails ends the run.
usage: tools/depth_timing.py            (all steps)
       tools/depth_timing.py --step NAME"""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-odom-pipeline_amd"))
import numpy as np

ROUNDS, WARM, CALLS = 5, 2, 10
STEPS = (("batch1", 240), ("batch256", 420))


def pose6(Hm):
    from vo_mi355x.so3 import rodrigues_mat_to_vec
    return np.concatenate([np.asarray(rodrigues_mat_to_vec(Hm[:3, :3])).reshape(3), Hm[:3, 3]])


def segment_lengths(K, pose, sd):
    """max(|B.x - A.x|, |B.y - A.y|) of the seeds' epipolar segments under pose (rvec, tvec), as include/vo_mi355x.h states them"""
    from vo_mi355x.so3 import rodrigues_vec_to_mat
    R, t = rodrigues_vec_to_mat(pose[:3]), pose[3:]
    x, y = (sd["u"] - K[0, 2]) / K[0, 0], (sd["v"] - K[1, 2]) / K[1, 1]
    f = np.stack([x, y, np.ones_like(x)], 1) / np.sqrt(x * x + y * y + 1.0)[:, None]
    s = np.sqrt(sd["sigma2"])
    out = []
    for d in (1.0 / (sd["mu"] + s), 1.0 / np.maximum(sd["mu"] - s, 1e-8)):
        X = (f @ R.T) * d[:, None] + t
        out.append(np.stack([K[0, 0] * X[:, 0] / X[:, 2] + K[0, 2], K[1, 1] * X[:, 1] / X[:, 2] + K[1, 2]], 1))
    return np.abs(out[1] - out[0]).max(1)


def timing(B):
    from vo_mi355x import DepthSeeds, VoContext, synthetic as syn
    W, H, N, T = 1241, 376, 2000, 6
    sc = syn.sway_scene(T + 1, w=W, h=H, f=718.0, pose_fn=lambda t: syn.sway_pose(t, period=60.0))
    K = sc["K"]
    rng = np.random.default_rng(1)
    uv = np.stack([rng.uniform(16, W - 16, N), rng.uniform(16, H - 16, N)], 1).astype(np.float32)
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape)) if B > 1 else a
    poses = [rep(pose6(sc["poses"][t])[None]) for t in range(T + 1)]
    with VoContext(W, H, max_pts=N, batch=B) as c:
        c.push_frame(rep(sc["frames"][0]))
        seeds = c.depth_seeds(rep(uv), 8.0, 3.0)
        states = {}
        for t in range(1, T + 1):
            c.push_frame(rep(sc["frames"][t]))
            states[t] = seeds.seeds.copy()
            res, match, z, st = c.depth_update(rep(K), poses[t], seeds)
        # timed: frame T against the states the seeds had before their 1st, 4th and last update
        p0 = rep(uv)
        for label, t_state in (("fresh seeds", 1), ("after 3 updates", 4), ("after %d updates" % (T - 1), T)):
            work = DepthSeeds(states[t_state].copy(), seeds.patches, seeds.ok)
            first = work.seeds[0] if B > 1 else work.seeds
            seg = segment_lengths(K, pose6(sc["poses"][T]), first)

            def call():
                work.seeds[...] = states[t_state]
                return c.depth_update(rep(K), poses[T], work)
            host, dev = [], []
            for rnd in range(ROUNDS):
                for k in range(WARM):
                    call()
                c.profile_enable([c.PROF_DEPTH])
                t0 = time.perf_counter()
                for k in range(CALLS):
                    out = call()
                host.append(1e6 * (time.perf_counter() - t0) / CALLS)
                ms, cnt = c.profile_read(c.PROF_DEPTH)
                c.profile_enable(())
                dev.append(1e3 * ms / max(cnt, 1))
            st = out[3][0] if B > 1 else out[3]
            res = out[0][0] if B > 1 else out[0]
            print("n=%d B=%3d depth_update, %-16s: launch median %9.1f us, min %9.1f us; call median %9.1f us (%d rounds of %d calls); "
                  "segments: mean %.1f, median %.1f pixels; %s" % (N, B, label, np.median(dev), min(dev), np.median(host), ROUNDS, CALLS, seg.mean(), np.median(seg), st), flush=True)
        host, dev = [], []
        for rnd in range(ROUNDS):
            for k in range(WARM):
                c.klt_track(p0)
            c.profile_enable([c.PROF_KLT])
            t0 = time.perf_counter()
            for k in range(CALLS):
                c.klt_track(p0)
            host.append(1e6 * (time.perf_counter() - t0) / CALLS)
            ms, cnt = c.profile_read(c.PROF_KLT)
            c.profile_enable(())
            dev.append(1e3 * ms / max(cnt, 1))
        print("n=%d B=%3d klt_track                     : launch median %9.1f us, min %9.1f us; call median %9.1f us" % (N, B, np.median(dev), min(dev), np.median(host)),
              flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        {"batch1": lambda: timing(1), "batch256": lambda: timing(256)}[sys.argv[2]]()
        sys.exit(0)
    for name, limit in STEPS:
        rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name])
        if rc != 0:
            print("step %s ended with status %d: the run ends here" % (name, rc), flush=True)
            sys.exit(rc)
