"""What the GPU tests of the frame-ingest steps (undistortion, CLAHE, the bilateral pre-filter) share: the fused-step plan loop, the
closed-loop runner and its comparison, the loop scene, the store comparison.  A plain module like build_helpers.py; every comparison is exact."""
import contextlib
import copy

import numpy as np
import pytest

import pipe_helpers as ph

STEP_KEYS = ("points2d", "status", "err", "corners")


def code(fn):
    """the VoError code `fn` raises"""
    from vo_mi355x import VoError
    with pytest.raises(VoError) as ei:
        fn()
    return ei.value.code


def same_store(a, b, seq=0, which=1, levels=3):
    """the frame stores of two contexts: image and derivative of every level"""
    for l in range(levels):
        xa, xb = a.pyramid_read(which, l, seq=seq), b.pyramid_read(which, l, seq=seq)
        assert np.array_equal(xa[0], xb[0]) and np.array_equal(xa[1], xb[1]), (seq, which, l)


# ---- the fused frame steps --------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def fused_pair(w, h, frames, pts, graph_a, graph_b, first_b):
    """context a with `frames` uploaded and frame 0 pushed from that sequence, context b with `first_b` pushed; both hold `pts`"""
    from vo_mi355x import VoContext
    with VoContext(w, h, max_pts=512) as a, VoContext(w, h, max_pts=512) as b:
        a.set_graph_mode(graph_a); b.set_graph_mode(graph_b)
        for c in (a, b):
            c.points_upload(pts)
        a.upload_sequence(frames)
        a.push_frame_resident(0); b.push_frame(first_b)
        yield a, b


def fused_plan(a, b, frames, order, plan, fed, n, host, apply, after=None):
    """Step k: a takes the raw frames[order[k]] (from its uploaded sequence, or with `host` handed over by the host), b takes fed[k] through
    frame_step_host, which always uses plain launches.  apply(entry) runs before every step whose plan entry differs from the last one's.
    The tracker's and the detector's outputs and the stores must be equal step by step; after(k, f, entry) checks what else a test needs."""
    cur = None
    for k, (f, s) in enumerate(zip(order, plan)):
        if s != cur:
            apply(s)
            cur = s
        if host:
            a.frame_step_host(frames[f].copy(), n, do_dlt=False, do_ba=False)
        else:
            a.frame_step_resident(f, n, do_dlt=False, do_ba=False)
        b.frame_step_host(fed[k], n, do_dlt=False, do_ba=False)
        ga, gb = a.frame_fetch(), b.frame_fetch()
        for key in STEP_KEYS:
            assert np.array_equal(ga[key], gb[key]), (k, f, s, key)
        same_store(a, b)
        if after is not None:
            after(k, f, s)


# ---- the closed loop --------------------------------------------------------------------------------------------------------------------
W, H, T1 = 256, 160, 3


def loop_scene(model):
    """-> the scene, its bootstrap state and the scene's frames through model(frame, scene)"""
    from vo_mi355x import VoContext
    sc = ph.scene(T1 + 8, w=W, h=H, f=260.0, seed=2024, pose_fn=lambda t: ph.sway_pose(t, period=24.0))
    with VoContext(W, H, max_pts=1024) as boot:
        state, t1 = ph.gt_bootstrap(boot, sc, 0, T1)
    assert t1 == T1
    out = np.stack([model(f, sc) for f in sc["frames"]])
    assert (out != sc["frames"]).mean() > 0.2
    return sc, state, out


def run_loop(sc, state, frames, host, side, inflight, getter, **kw):
    """four closed-loop steps over `frames` with ResidentPipeline(**kw) -> the records, the tables, the store; `getter` names the context's
    get_* that must report a setting exactly when kw names one"""
    from vo_mi355x import VoContext
    from vo_mi355x.resident import INFLIGHT, ResidentPipeline
    assert inflight <= INFLIGHT
    n = 4
    with VoContext(W, H, max_pts=1024) as c:
        c.set_side_stream(side)
        rp = ResidentPipeline(c, sc["K"], ba_max_iters=12, pnp_blind_batches=8, **kw)
        assert (getattr(c, getter)() is not None) == bool(kw)
        rp.seed(copy.deepcopy(state), [], [], 1)
        c.upload_sequence(frames)
        c.push_frame_resident(T1)
        recs, pending = [], 0
        for s in range(n):
            if host:
                rp.step_host(frames[T1 + 1 + s].copy())
            else:
                rp.step(T1 + 1 + s)
            pending += 1
            if pending == inflight or s == n - 1:
                while pending:
                    recs.append(rp.fetch()); pending -= 1
        return recs, rp.read_tables(), [c.pyramid_read(1, l) for l in range(3)]


def same_loop(run_a, run_b):
    """two run_loop results: every record field, every table, the store"""
    (ra, Ta, pa), (rb, Tb, pb) = run_a, run_b
    for s, (x, y) in enumerate(zip(ra, rb)):
        for k, v in x.items():
            assert (np.array_equal(y[k], v, equal_nan=True) if isinstance(v, np.ndarray) else y[k] == v), (s, k)
    for name in Ta:
        assert np.array_equal(Ta[name], Tb[name], equal_nan=Ta[name].dtype.kind == "f"), name
    for x, y in zip(pa, pb):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
