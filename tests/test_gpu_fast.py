"""GPU: the FAST-9/16 corner response (csrc/vo_fast.hip, vo_st_params.fast_threshold) on every detection path, against tests/fast_model.py.

Every comparison is exact: the score is integer arithmetic, the selection behind it is the one the Shi-Tomasi path runs.  1. the synchronous
call: response map, mask, candidate count and the ordered corners on the smallest shapes at which the kernel can go wrong (one pixel of
interior, a width that is no multiple of a thread's four pixels, a second column block, a batch with its sequence strides); 2. the resident
forms and the track table, with sub-pixel refinement behind it; 3. the fused frame steps with and without graph replay, the detector
switched between steps; 4. the closed loop on every stream layout; 5. the drop-in Extractor; 6. errors.

FAST scores are small integers, so ties are the rule (a checkerboard: one value for all corners): the rank order among equal scores -- pixel
index descending -- is part of what is compared."""
import copy

import numpy as np
import pytest

import fast_model as fm
import ingest_helpers as ih
import pipe_helpers as ph
from ingest_helpers import H, T1, W, code as _code

pytestmark = pytest.mark.gpu

KINDS = ("zeros", "checker", "noise", "narrow", "blocks", "extremes")
SHAPES = [(7, 7), (8, 7), (101, 37), (96, 64), (259, 41)]
THRESHOLDS = (1, 20, 100, 254)


def _points(w, h, n, seed):
    """disc centres: anywhere in the frame, borders and the corners included, fractional (np.int32 truncates)"""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], axis=1).astype(np.float32)
    p[0] = (0.0, 0.0); p[1] = (w - 1, h - 1)
    return p


def _user_mask(w, h, seed):
    rng = np.random.default_rng(seed)
    m = (rng.integers(0, 5, (h, w)) > 0).astype(np.uint8) * 255
    m[:, w // 2:w // 2 + 3] = 0
    return m


def _check(c, img, t, got, mask, max_corners=1000, quality=0.03, min_distance=7, tag=None):
    """corners `got` of one sequence and what vo_shi_tomasi_read returns for it = the model on `img` behind `mask`; -> the model's corner count"""
    R, gmask, ncand = c
    want_R = fm.score_map(img, t).astype(np.float32)
    assert np.array_equal(R, want_R), (tag, "R", int((R != want_R).sum()))
    assert np.array_equal(gmask, np.full(img.shape, 255, np.uint8) if mask is None else mask), (tag, "mask")
    assert ncand == len(fm.candidates(want_R, mask, quality)[1]), (tag, "n_candidates")
    want = fm.select(want_R, mask, max_corners, quality, min_distance)
    assert got.shape == want.shape and np.array_equal(got, want), (tag, "corners", len(got), len(want))
    return len(want)


# ---- 1. the synchronous call ------------------------------------------------------------------------------------------------------------
def test_the_models_outputs_are_not_empty():
    """the conditions under which agreement below means something (the model alone; kept with the GPU tests that rely on them)"""
    def corners(kind, t):
        R = fm.score_map(fm.make_image(kind, 101, 37), t)
        return int((R > 0).sum()), np.unique(R[R > 0])
    n, v = corners("noise", 20); assert n == 770 and len(v) == 99
    for t in (1, 20, 100):
        n, v = corners("checker", t); assert n == 190 and list(v) == [159]                    # one score for every corner: the tie-order case
    n, v = corners("narrow", 1); assert n == 499 and list(v) == [1, 2, 3, 4, 5]
    n, v = corners("extremes", 254); assert n == 41 and list(v) == [254]                      # the upper edge
    R = fm.score_map(fm.ring_7x7(), 1); assert (R > 0).sum() == 1 and R[3, 3] == 254


@pytest.mark.parametrize("w,h", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_response_map_and_default_selection_equal_the_model(w, h):
    from vo_mi355x import VoContext
    imgs = [(k, fm.make_image(k, w, h)) for k in KINDS]
    if h == 7:                                         # the hand-made frame (in the 8-wide context: one more column of its background)
        imgs.append(("ring", np.pad(fm.ring_7x7(), ((0, 0), (0, w - 7)), constant_values=128)))
    total = 0
    with VoContext(w, h, max_pts=64) as c:
        assert c.st_params().fast_threshold == 0
        for kind, img in imgs:
            c.push_frame(img)
            for t in THRESHOLDS:
                got = c.shi_tomasi(None, params=c.st_params(fast_threshold=t, min_distance=3, block_size=3))     # (block_size plays no part)
                n = _check(c.shi_tomasi_read(), img, t, got, None, min_distance=3, tag=(kind, t))
                n_model = int((fm.score_map(img, t) > 0).sum())
                if kind == "ring":
                    assert n == 1 and np.array_equal(got, [[3, 3]]) and fm.score_map(img, t)[3, 3] == 254 and (w > 7 or n_model == 1)
                total += n
    assert total > 0


MASKS = ["none", "user", "discs0", "discs3", "discs7"]


@pytest.mark.parametrize("variant", MASKS)
def test_masks_and_every_selection_parameter(variant):
    """(image, t) = noise at 20 (99 distinct scores), checker at 20 (all ties), narrow noise at 1 (scores 1..5), extremes at 254; two shapes"""
    from vo_mi355x import VoContext
    for (w, h) in ((101, 37), (259, 41)):
        pts = _points(w, h, 14, w + h)
        user = _user_mask(w, h, w * h)
        if variant == "none":
            kw, mask = dict(), None
        elif variant == "user":
            kw, mask = dict(mask=user, cur_pts=pts, mask_radius=3), fm.disc_mask(w, h, pts, 3, base=user)
        else:
            r = int(variant[5:])
            kw, mask = dict(cur_pts=pts, mask_radius=r), fm.disc_mask(w, h, pts, r)
        with VoContext(w, h, max_pts=64) as c:
            for kind, t in (("noise", 20), ("checker", 20), ("narrow", 1), ("extremes", 254)):
                img = fm.make_image(kind, w, h)
                c.push_frame(img)
                assert int((fm.score_map(img, t) > 0).sum()) > 0
                for md in (0, 1, 7):
                    for mc in (0, 5, 1000):
                        for q in (0.03, 0.5):
                            got = c.shi_tomasi(params=c.st_params(max_corners=mc, quality_level=q, min_distance=md, fast_threshold=t), **kw)
                            n = _check(c.shi_tomasi_read(), img, t, got, mask, mc, q, md, tag=(w, h, kind, t, md, mc, q))
                            assert n > 0


def test_batch_of_three_uses_every_sequence_stride():
    from vo_mi355x import VoContext
    w, h = 101, 37
    imgs = np.stack([fm.make_image(k, w, h) for k in ("noise", "checker", "narrow")])
    pts = np.stack([_points(w, h, 9, s) for s in (1, 2, 3)])
    user = np.stack([_user_mask(w, h, s) for s in (4, 5, 6)])
    with VoContext(w, h, max_pts=64, batch=3) as c:
        c.push_frame(imgs)
        for t in (1, 20):
            got = c.shi_tomasi(pts, mask_radius=3, mask=user, params=c.st_params(fast_threshold=t, min_distance=1))
            R, gm, nc = c.shi_tomasi_read()
            for b in range(3):
                n = _check((R[b], gm[b], int(nc[b])), imgs[b], t, got[b], fm.disc_mask(w, h, pts[b], 3, base=user[b]), min_distance=1, tag=(b, t))
                assert n > 0 or (b == 2 and t == 20)


# ---- 2. the resident forms --------------------------------------------------------------------------------------------------------------
def test_resident_call_and_fetch():
    from vo_mi355x import VoContext
    w, h, t = 259, 41, 20
    img, pts = fm.make_image("noise", w, h), _points(w, h, 20, 8)
    with VoContext(w, h, max_pts=64) as c:
        c.push_frame(img)
        c.points_upload(pts)
        for r in (0, 7):
            c.shi_tomasi_resident(len(pts), mask_radius=r, params=c.st_params(fast_threshold=t, max_corners=50))
            got = c.shi_tomasi_fetch()
            assert _check(c.shi_tomasi_read(), img, t, got, fm.disc_mask(w, h, pts, r), max_corners=50, tag=r) == 50
        # the default response after it (the FAST launch leaves the discs in the mask: the next launch must start from a clean one)
        c.shi_tomasi_resident(len(pts), mask_radius=7)
        import vo_oracle as o
        assert np.array_equal(c.shi_tomasi_fetch(), o.good_features(img, fm.disc_mask(w, h, pts, 7)))


@pytest.mark.parametrize("subpix", [False, True], ids=["integer", "subpix"])
def test_track_table_spawns_the_models_corners(seq_small, subpix):
    from vo_mi355x import VoContext, synthetic as syn
    frames = seq_small[0]
    w, h, t = 320, 240, 20
    seeds = syn.grid_points(60, w, h, margin=10, seed=4)
    with VoContext(w, h, max_pts=512) as c:
        if subpix:
            c.set_subpix(dict(win=(4, 4), max_count=20))
        c.push_frame(frames[0]); c.tracks_seed(seeds, t=0)
        c.push_frame(frames[1]); c.tracks_track(1)
        live = c.tracks_read()["uv"]
        assert len(live) > 30
        c.tracks_detect(1, mask_radius=7, params=c.st_params(fast_threshold=t, max_corners=200), max_new=40)
        r = c.tracks_read()
        new = r["t_first"] == 1
        want = fm.select(fm.score_map(frames[1], t), fm.disc_mask(w, h, live, 7), 200, 0.03, 7)
        assert len(want) > 40 and new.sum() == 40 and np.array_equal(r["uv"][~new], live)
        if subpix:
            info = c.subpix_read()
            assert np.array_equal(info["raw"], want)
            ref = c.corner_subpix(want, "cur", c.subpix_params(win=(4, 4), max_count=20))
            assert (ref != want).any() and np.array_equal(r["uv"][new].view(np.uint32), ref[:40].view(np.uint32))
        else:
            assert np.array_equal(r["uv"][new], want[:40]) and np.array_equal(c.shi_tomasi_fetch(), want)


# ---- 3. the fused frame steps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["launches", "graph"])
@pytest.mark.parametrize("host", [False, True], ids=["resident", "host"])
def test_fused_steps_alternate_the_detector(host, graph):
    """FAST(20) -> Shi-Tomasi -> FAST(100) over nine steps: with graph replay on, steps 6 .. 8 meet the captures of steps 0 .. 2 (same detector,
    same store parity) -- a step that replayed another detector's capture, or trusted a mask the FAST launch left its discs in, would show.
    Every step's corners = the synchronous call of a second context on the same frame and points (and the model, for the FAST steps)."""
    from vo_mi355x import VoContext, synthetic as syn
    import vo_oracle as o
    w, h, n = W, H, 120
    frames, _ = syn.make_sequence(4, w=w, h=h, seed=21, margin=64)
    # contrast stretched threefold about mid-grey: the rendered texture as it is holds no FAST corner at threshold 100 (with it: ~400 per frame)
    frames = np.clip((frames.astype(np.int32) - 128) * 3 + 128, 0, 255).astype(np.uint8)
    assert all((fm.score_map(f, 100) > 0).sum() > 300 for f in frames)
    order = [1, 2, 3, 2, 1, 2, 3, 2, 1]
    pts = syn.grid_points(n, w, h, seed=4)
    with VoContext(w, h, max_pts=512) as a, VoContext(w, h, max_pts=512) as b:
        a.set_graph_mode(graph)
        a.points_upload(pts)
        a.upload_sequence(frames)
        a.push_frame_resident(0)
        plan = [dict(fast_threshold=20), dict(), dict(fast_threshold=100)]
        n_fast = 0
        for k, f in enumerate(order):
            kw = plan[k % 3]
            st = a.st_params(max_corners=300, **kw)
            if host:
                a.frame_step_host(frames[f].copy(), n, do_dlt=False, do_ba=False, st=st)
            else:
                a.frame_step_resident(f, n, do_dlt=False, do_ba=False, st=st)
            ga = a.frame_fetch()
            p1 = ga["points2d"]
            b.push_frame(frames[f])
            sync = b.shi_tomasi(p1, mask_radius=7, params=b.st_params(max_corners=300, **kw))
            assert len(sync) > 20 and np.array_equal(ga["corners"], sync), (k, f, kw)
            if np.isfinite(p1).all():
                mask = fm.disc_mask(w, h, p1, 7)
                if kw:
                    want = fm.select(fm.score_map(frames[f], kw["fast_threshold"]), mask, 300, 0.03, 7)
                    n_fast += 1
                else:
                    want = o.good_features(frames[f], mask, maxCorners=300)
                assert np.array_equal(ga["corners"], want), (k, f, kw, "model")
        assert n_fast >= 3


# ---- 4. the closed loop -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loop_scene():
    from vo_mi355x import VoContext
    sc = ph.scene(T1 + 8, w=W, h=H, f=260.0, seed=2024, pose_fn=lambda t: ph.sway_pose(t, period=24.0))
    with VoContext(W, H, max_pts=1024) as boot:
        state, t1 = ph.gt_bootstrap(boot, sc, 0, T1)
    assert t1 == T1
    return sc, state


def _run_loop(sc, state, host, side, inflight, check=None, **kw):
    """three closed-loop steps -> the records, the tables; check(s, record, tables) after every fetch of a run with one step in flight"""
    from vo_mi355x import VoContext
    from vo_mi355x.resident import ResidentPipeline
    n = 3
    with VoContext(W, H, max_pts=1024) as c:
        c.set_side_stream(side)
        rp = ResidentPipeline(c, sc["K"], ba_max_iters=12, pnp_blind_batches=8, **kw)
        rp.seed(copy.deepcopy(state), [], [], 1)
        c.upload_sequence(sc["frames"])
        c.push_frame_resident(T1)
        recs, pending = [], 0
        for s in range(n):
            if host:
                rp.step_host(sc["frames"][T1 + 1 + s].copy())
            else:
                rp.step(T1 + 1 + s)
            pending += 1
            if pending == inflight or s == n - 1:
                while pending:
                    recs.append(rp.fetch()); pending -= 1
                    if check is not None and inflight == 1:
                        check(s, recs[-1], rp.read_tables())
        return recs, rp.read_tables()


def _same_runs(run_a, run_b):
    (ra, Ta), (rb, Tb) = run_a, run_b
    for s, (x, y) in enumerate(zip(ra, rb)):
        for k, v in x.items():
            assert (np.array_equal(y[k], v, equal_nan=True) if isinstance(v, np.ndarray) else y[k] == v), (s, k)
    for name in Ta:
        assert np.array_equal(Ta[name], Tb[name], equal_nan=Ta[name].dtype.kind == "f"), name


_REFERENCE = {}


def _fast_loop_reference(loop_scene, host):
    """the FAST loop with one step in flight on the side-stream layout, every step's new candidates checked against the model (run once
    per frame source)"""
    if host in _REFERENCE:
        return _REFERENCE[host]
    sc, state = loop_scene
    t = 20
    seen = []

    def check(s, rec, T):
        n_new, n_c, n_l = rec["n_detected"], int(T["counts"][0, 0]), int(T["counts"][0, 1])
        rows = np.concatenate([T["lm_k"][0, :n_l], T["cand"][0, :n_c - n_new]])
        mask = fm.disc_mask(W, H, T["k_uv"][0, rows], 7)
        want = fm.select(fm.score_map(sc["frames"][T1 + 1 + s], t), mask, 1000, 0.03, 7)
        assert len(rows) + len(want) < 1024                               # room for every corner: nothing but the selection limits the spawn
        assert n_new == len(want) > 0, (s, n_new, len(want))
        assert np.array_equal(T["k_uv"][0, T["cand"][0, n_c - n_new:n_c]], want), s
        seen.append(n_new)

    run = _run_loop(sc, state, host, True, 1, check, detector='fast', fast_threshold=t)
    assert len(seen) == 3 and all(r["status"] == 0 for r in run[0])
    print("closed loop with FAST(20): detected %s" % seen)
    _REFERENCE[host] = run
    return run


@pytest.mark.parametrize("side,inflight", [(True, 1), (False, 1), (True, 4)], ids=["side", "one_stream", "side_inflight"])
@pytest.mark.parametrize("host", [False, True], ids=["step", "step_host"])
def test_closed_loop_detects_the_models_corners_on_every_layout(loop_scene, host, side, inflight):
    sc, state = loop_scene
    ref = _fast_loop_reference(loop_scene, host)       # (side stream, one step in flight: checked against the model step by step)
    if (side, inflight) != (True, 1):
        _same_runs(ref, _run_loop(sc, state, host, side, inflight, detector='fast', fast_threshold=20))


def test_closed_loop_named_shi_tomasi_is_the_default_loop(loop_scene):
    from vo_mi355x import VoContext
    from vo_mi355x.resident import ResidentPipeline
    sc, state = loop_scene
    plain = _run_loop(sc, state, False, True, 1)
    _same_runs(plain, _run_loop(sc, state, False, True, 1, detector='shi-tomasi', fast_threshold=33))
    fast = _fast_loop_reference(loop_scene, False)
    assert [r["n_detected"] for r in plain[0]] != [r["n_detected"] for r in fast[0]]                      # the two detectors do differ here
    with VoContext(W, H, max_pts=256) as c:
        with pytest.raises(ValueError):
            ResidentPipeline(c, sc["K"], detector='orb')
        assert ResidentPipeline(c, sc["K"], detector='fast').params.st.fast_threshold == 20
        assert ResidentPipeline(c, sc["K"]).params.st.fast_threshold == 0


# ---- 5. the drop-in Extractor -----------------------------------------------------------------------------------------------------------
def test_dropin_extractor_detects_with_fast(seq_small):
    from vo_mi355x import lazy
    from vo_mi355x.extractor import Extractor
    from vo_mi355x.state import Keypoint
    img = seq_small[0][0]
    h, w = img.shape
    pts = _points(w, h, 30, 12)
    cur = [Keypoint(t_first=0, t_total=1, uv_first=p.reshape(2, 1).copy(), uv=p.reshape(2, 1).copy(), des=np.zeros((1, 1)), uv_history=[]) for p in pts]
    for thr in (20, 40):
        e = Extractor(lazy=False, min_kp_dist=7, fast_threshold=thr)
        assert e._fast_params == dict(threshold=thr, nonmaxSuppression=True)
        kps = e.extract(img, 5, cur, detector='fast', mask_radius=5)
        want = fm.select(fm.score_map(img, thr), fm.disc_mask(w, h, pts, 5), 1000, 0.03, 7)
        assert len(want) > 20 and len(kps) == len(want)
        assert np.array_equal(np.stack([k.uv.reshape(2) for k in kps]), want)
        for k in kps:
            assert k.t_first == 5 and k.t_total == 1 and k.uv.shape == (2, 1) and len(k.uv_history) == 1
            assert np.shares_memory(k.uv, k.uv_first) and np.shares_memory(k.uv, k.uv_history[0])
        # the Shi-Tomasi path of the same object is untouched by the FAST settings
        plain = Extractor(lazy=False, min_kp_dist=7).extract(img, 5, cur, detector='shi-tomasi', mask_radius=5)
        mine = e.extract(img, 5, cur, detector='shi-tomasi', mask_radius=5)
        assert len(plain) == len(mine) > 20 and all(np.array_equal(x.uv, y.uv) for x, y in zip(plain, mine))
        assert not np.array_equal(np.stack([k.uv.reshape(2) for k in mine])[:20], want[:20])
    assert Extractor(lazy=False)._fast_params["threshold"] == 20
    with pytest.raises(NotImplementedError):
        e.extract(img, 5, cur, detector='fast', describe=True)
    with pytest.raises(ValueError):
        e.extract(img, 5, cur, detector='orb')
    assert lazy.Session.extract(None, img, 5, cur, 5, detector='fast') is NotImplemented      # a session does not serve it: the plain path runs


# ---- 6. errors --------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_is_invalid_and_leaves_the_default_detection_alone(loop_scene):
    import ctypes as C
    import vo_oracle as o
    from vo_mi355x import VoContext, VoError, _lib
    from vo_mi355x.resident import ResidentPipeline
    w, h = 101, 37
    img, pts = fm.make_image("blocks", w, h), _points(w, h, 10, 3)
    frames = np.stack([img, fm.make_image("noise", w, h)])
    p = _lib.StParams()
    C.memset(C.byref(p), 0x5A, C.sizeof(p))
    assert C.sizeof(p) == 40 and _lib.load().vo_st_default_params(C.byref(p)) == 0 and p.fast_threshold == 0 and p.use_harris == 0
    with VoContext(w, h, max_pts=64) as c:
        c.upload_sequence(frames)
        c.push_frame_resident(0)
        c.points_upload(pts)
        before = c.shi_tomasi(pts, params=c.st_params(block_size=5))
        assert len(before) > 0 and np.array_equal(before, o.good_features(img, fm.disc_mask(w, h, pts, 7), blockSize=5))
        bad = [c.st_params(block_size=5, fast_threshold=-1), c.st_params(block_size=5, fast_threshold=255),
               c.st_params(block_size=5, fast_threshold=20, use_harris=True), c.st_params(block_size=5, fast_threshold=1 << 20)]
        for prm in bad:
            assert _code(lambda: c.shi_tomasi(pts, params=prm)) == -1
            assert _code(lambda: c.shi_tomasi_resident(len(pts), params=prm)) == -1
            assert _code(lambda: c.frame_step_resident(1, len(pts), do_dlt=False, do_ba=False, st=prm)) == -1
            assert np.array_equal(c.pyramid_read(1, 0)[0], img)            # nothing was enqueued: the store still holds frame 0
            assert np.array_equal(c.shi_tomasi(pts, params=c.st_params(block_size=5)), before)
        got = c.shi_tomasi(pts, params=c.st_params(block_size=5, fast_threshold=254))                     # the largest threshold is accepted
        assert np.array_equal(got, fm.select(fm.score_map(img, 254), fm.disc_mask(w, h, pts, 7), 1000, 0.03, 7))
        assert np.array_equal(c.shi_tomasi(pts, params=c.st_params(block_size=5)), before)
    sc = loop_scene[0]
    with VoContext(W, H, max_pts=256) as c:
        with pytest.raises(VoError) as ei:
            ResidentPipeline(c, sc["K"], detector='fast', fast_threshold=255)
        assert ei.value.code == -1
