"""Time per call of VoContext.sparse_align (vo_sparse_align) at 1241 x 376 with 2000 points, batch 1 and batch 256, beside VoContext.klt_track
of the same points and VoContext.pnp_ransac; its split over the pyramid levels; both forms of the reference-patch decision (kept in a
workspace / recomputed every iteration); and what the aligned pose is worth to the tracker on a sway_scene pair: the sum of the tracker's
iterations and its survivors when it starts at the aligned projections, at the constant-velocity guess and where the points were.

Frames: synthetic.sway_scene with ground-truth poses; points: random pixels with their true 3-D points.  All calls are synchronous with
their uploads and read-backs: the call a user makes.  Time: host clock around CALLS calls after WARM warm-up calls, the calls alternating over
ROUNDS rounds; median and minimum of the rounds.  The per-level split comes from hipEvent pairs around each launch (vo_profile_enable,
region VO_PROF_ALIGN) in a separate loop of single-level calls, each started at the pose the coarser levels left.
Every step runs in a child process of its own under `timeout`; the first step that fails ends the run.
usage: tools/align_timing.py            (all steps)
       tools/align_timing.py --step NAME"""
import os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-odom-pipeline_amd"))
import numpy as np

ROUNDS, WARM, CALLS = 5, 2, 10
STEPS = (("batch1", 240), ("batch256", 420), ("seeded", 180))


def scene_points(sc, t, n, seed, margin=16):
    """n random pixels of frame t with their true 3-D points in camera t's coordinates"""
    h, w = sc["frames"][t].shape
    rng = np.random.default_rng(seed)
    uv = np.stack([rng.uniform(margin, w - margin, n), rng.uniform(margin, h - margin, n)], 1)
    Z, p0 = sc["surface"](t, uv)
    K, G = sc["K"], sc["poses"][t]
    X0 = np.stack([(p0[:, 0] - K[0, 2]) / K[0, 0] * Z, (p0[:, 1] - K[1, 2]) / K[1, 1] * Z, Z], 1)
    return (X0 @ G[:3, :3].T + G[:3, 3]).astype(np.float32)


def project(K, X):
    return np.stack([K[0, 0] * X[:, 0] / X[:, 2] + K[0, 2], K[1, 1] * X[:, 1] / X[:, 2] + K[1, 2]], 1)


def timing(B):
    from vo_mi355x import VoContext, synthetic as syn
    W, H, N = 1241, 376, 2000
    sc = syn.sway_scene(2, w=W, h=H, f=718.0)
    K = sc["K"]
    X = scene_points(sc, 0, N, 1)
    rel = sc["poses"][1] @ np.linalg.inv(sc["poses"][0])
    p0 = project(K, X.astype(np.float64)).astype(np.float32)
    p1 = project(K, X.astype(np.float64) @ rel[:3, :3].T + rel[:3, 3]).astype(np.float32)
    rep = lambda a: np.ascontiguousarray(np.broadcast_to(a, (B,) + a.shape)) if B > 1 else a
    Xs, p0s, p1s, Ks = rep(X), rep(p0), rep(p1), rep(K)
    first = lambda v: v if B == 1 else v[0]
    with VoContext(W, H, max_pts=N, batch=B) as c:
        c.push_frame(rep(sc["frames"][0])); c.push_frame(rep(sc["frames"][1]))
        calls = (("sparse_align (rule)", lambda: c.sparse_align(Ks, Xs)),
                 ("sparse_align workspace", lambda: c.sparse_align(Ks, Xs, params=c.align_params(form=1))),
                 ("sparse_align recompute", lambda: c.sparse_align(Ks, Xs, params=c.align_params(form=2))),
                 ("klt_track", lambda: c.klt_track(p0s)),
                 ("pnp_ransac", lambda: c.pnp_ransac(Ks, Xs, p1s, seed=7)))
        times, last = {name: [] for name, _ in calls}, {}
        for rnd in range(ROUNDS):
            for name, fn in calls:
                for k in range(WARM):
                    fn()
                t0 = time.perf_counter()
                for k in range(CALLS):
                    last[name] = fn()
                times[name].append(1e6 * (time.perf_counter() - t0) / CALLS)
        for name, _ in calls:
            print("n=%d B=%3d %-24s: median %9.1f us, min %9.1f us per call (%d rounds of %d calls)"
                  % (N, B, name, np.median(times[name]), min(times[name]), ROUNDS, CALLS), flush=True)
        rv, tv, used, st = last["sparse_align (rule)"]
        st, rv, tv = first(st), first(rv), first(tv)
        Rm = syn.rodrigues(rv)
        err = np.median(np.linalg.norm(project(K, X.astype(np.float64) @ Rm.T + tv) - p1, axis=1))
        print("n=%d B=%3d   aligned: iters %s, %d used, chi2 %.2f; median image motion %.2f px, median prediction error %.3f px"
              % (N, B, st["iters"][:c.max_level + 1], st["n_used"], st["chi2"], np.median(np.linalg.norm(p1 - p0, axis=1)), err), flush=True)
        a, b = last["sparse_align workspace"], last["sparse_align recompute"]
        print("n=%d B=%3d   the two forms give the same bits: %s" % (N, B, np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])), flush=True)
        # the split over the levels: single-level calls, each from the pose the coarser levels left
        top = max(l for l in range(8) if st["iters"][l] != 0)
        for form, fname in ((1, "workspace"), (2, "recompute")):
            r0, t0 = None, None
            for l in range(top, -1, -1):
                prm = c.align_params(max_level=l, min_level=l, form=form)
                c.profile_enable([c.PROF_ALIGN])
                for k in range(CALLS):
                    out = c.sparse_align(Ks, Xs, r0, t0, prm)
                ms, cnt = c.profile_read(c.PROF_ALIGN)
                c.profile_enable(())
                print("n=%d B=%3d   %-9s level %d (%4d x %3d): %8.1f us per launch, %d linearisations" % ((N, B, fname, l) + c.level_size(l) + (1e3 * ms / max(cnt, 1), first(out[3])["iters"][l])),
                      flush=True)
                r0, t0 = out[0], out[1]


def seeded():
    from vo_mi355x import VoContext, synthetic as syn
    W, H, N = 416, 240, 512
    sc = syn.sway_scene(4, w=W, h=H)
    K = sc["K"]
    for t in (1, 2):
        X = scene_points(sc, t, N, 10 + t, margin=20)
        rel = sc["poses"][t + 1] @ np.linalg.inv(sc["poses"][t])
        back = sc["poses"][t - 1] @ np.linalg.inv(sc["poses"][t])
        Xd = X.astype(np.float64)
        p0 = project(K, Xd).astype(np.float32)
        pm = project(K, Xd @ back[:3, :3].T + back[:3, 3]).astype(np.float32)
        truth = project(K, Xd @ rel[:3, :3].T + rel[:3, 3])
        with VoContext(W, H, max_pts=N) as c:
            c.push_frame(sc["frames"][t]); c.push_frame(sc["frames"][t + 1])
            rv, tv, used, st = c.sparse_align(K, X)
            g_al = project(K, Xd @ syn.rodrigues(rv).T + tv).astype(np.float32)
            g_cv = p0 + (p0 - pm)
            for name, g in (("aligned", g_al), ("constant velocity", g_cv), ("none", None)):
                p1, status, err, it = c.klt_track(p0, return_iters=True, init=g)
                ok = (status != 0) & (np.linalg.norm(p1 - truth, axis=1) < 1.0)
                start = np.median(np.linalg.norm((p0 if g is None else g) - truth, axis=1))
                print("pair %d -> %d, %d points, start %-17s: median start error %6.3f px, sum of the tracker's iterations %6d, %3d tracked, %3d within 1 px of the truth"
                      % (t, t + 1, N, name, start, int(np.maximum(it, 0).sum()), int((status != 0).sum()), int(ok.sum())), flush=True)
            print("pair %d -> %d: alignment iters %s, %d used, chi2 %.2f" % (t, t + 1, st["iters"][:3], st["n_used"], st["chi2"]), flush=True)


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--step":
        {"batch1": lambda: timing(1), "batch256": lambda: timing(256), "seeded": seeded}[sys.argv[2]]()
        sys.exit(0)
    for name, limit in STEPS:
        rc = subprocess.call(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name])
        if rc != 0:
            print("step %s ended with status %d: the run ends here" % (name, rc), flush=True)
            sys.exit(rc)
