"""GPU: lens undistortion (cv2.undistort restated by tests/undistort_model.py) on every frame-ingest path.

Every comparison with the model is exact: one float64 map on the host, integers behind it.  1. the table; 2. the synchronous call; 3. the
ingest paths (push_frame, push_frame_resident, with the bilateral pre-filter, the tracker); 4. the fused frame steps with and without graph
replay, coefficients switched between steps; 5. the closed loop on every stream layout; 6. the drop-in Extractor; 7. errors."""
import numpy as np
import pytest

import ingest_helpers as ih
import undistort_model as um
from ingest_helpers import H, W, code as _code

pytestmark = pytest.mark.gpu

K = (260.0, 255.0, 158.3, 61.7)
# (name, dist, new_K)
SETS = [("barrel", (-0.3, 0.0, 0.0, 0.0), None),
        ("pincushion", (0.12, 0.05, 0.0, 0.0, 0.02), None),
        ("tangential", (0.0, 0.0, 0.004, -0.003), None),
        ("rational", (-0.25, 0.08, 0.001, -0.0005, 0.01, 0.05, 0.02, 0.003), None),
        ("zoom_out_shift", (-0.3, 0.1, 0.0, 0.0), (130.0, 128.0, 100.0, 90.0)),
        ("zero", (), None)]
IDS = [s[0] for s in SETS]


def _cam(w, h):
    """a camera for a w x h image: principal point off centre, fx != fy"""
    return (0.8 * w, 0.78 * w, 0.49 * w + 0.3, 0.51 * h - 0.3)


def _images(w, h):
    from vo_mi355x import synthetic as syn
    rng = np.random.default_rng(7)
    return [rng.integers(0, 256, (h, w)).astype(np.uint8),
            syn.make_sequence(1, w=w, h=h, seed=5, margin=32)[0][0],
            np.tile((np.arange(w) * 255 // (w - 1)).astype(np.uint8), (h, 1)),
            np.full((h, w), 200, np.uint8)]


# ---- 1. the table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dist,new_K", SETS, ids=IDS)
def test_table_equals_the_model(name, dist, new_K):
    from vo_mi355x import VoContext
    for w, h in ((203, 97), (321, 123)):
        with VoContext(w, h, max_pts=64) as c:
            c.set_undistort(K, dist, new_K)
            got, want = c.undistort_map_read(), um.table(w, h, K, dist, new_K)
            for k in ("sxy", "frac", "outside"):
                assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (w, h, k, int((got[k] != want[k]).sum()))
            if name == "zoom_out_shift":
                assert want["outside"].mean() > 0.2 and want["sxy"].min() == -2 and (want["outside"] == 0).any()
            g = c.get_undistort()
            assert np.array_equal(g["K"], K) and np.array_equal(g["new_K"], K if new_K is None else new_K)
            assert np.array_equal(g["dist"], list(dist) + [0.0] * (8 - len(dist)))


# ---- 2. the synchronous call --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,dist,new_K", SETS, ids=IDS)
def test_synchronous_call_equals_the_model(name, dist, new_K):
    from vo_mi355x import VoContext
    for w, h in ((203, 97), (320, 64)):                                   # rows that are / are not a multiple of 4: byte tail, unaligned stores
        with VoContext(w, h, max_pts=64) as c:
            c.set_undistort(K, dist, new_K)
            tab = um.table(w, h, K, dist, new_K)
            for k, img in enumerate(_images(w, h)):
                got, want = c.undistort(img), um.remap(img, tab)
                assert got.dtype == np.uint8 and np.array_equal(got, want), (w, h, k, int((got != want).sum()))
            if name == "zero":
                assert np.array_equal(c.undistort(img), img)


def test_synchronous_call_takes_a_matrix_a_batch_and_leaves_the_frame_store_alone():
    from vo_mi355x import VoContext
    w, h = 203, 97
    a, b, f0, f1 = _images(w, h)[0], _images(w, h)[1], _images(w, h)[2], _images(w, h)[1][::-1].copy()
    K3 = np.array([[K[0], 0, K[2]], [0, K[1], K[3]], [0, 0, 1.0]])
    dist = SETS[3][1]
    with VoContext(w, h, max_pts=64, batch=2) as c:
        c.push_frame(np.stack([f0, f1])); c.push_frame(np.stack([f1, f0]))
        before = [c.pyramid_read(which, l, seq=s) for which in (0, 1) for l in range(2) for s in (0, 1)]
        c.set_undistort(K3, dist)
        got = c.undistort(np.stack([a, b]))
        assert got.shape == (2, h, w)
        assert np.array_equal(got[0], um.undistort(a, K, dist)) and np.array_equal(got[1], um.undistort(b, K, dist))
        assert not np.array_equal(got[0], got[1])
        after = [c.pyramid_read(which, l, seq=s) for which in (0, 1) for l in range(2) for s in (0, 1)]
        for x, y in zip(before, after):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


# ---- 3. the ingest paths ------------------------------------------------------------------------------------------------------------
def _store_equals(c, img, seq=0, which=1):
    import vo_oracle as o
    lv = o.build_pyramid(img)
    for l in range(len(lv)):
        img_l, der_l = c.pyramid_read(which, l, seq=seq)
        assert np.array_equal(img_l, lv[l]) and np.array_equal(der_l, o.scharr(lv[l])), (seq, l)


@pytest.mark.parametrize("name,dist,new_K", [SETS[0], SETS[3], SETS[4]], ids=[IDS[0], IDS[3], IDS[4]])
def test_pushed_frames_enter_the_store_undistorted(name, dist, new_K):
    import vo_oracle as o
    from vo_mi355x import VoContext
    w, h = 321, 123
    cam = _cam(w, h)
    noise, tex = _images(w, h)[0], _images(w, h)[1]
    with VoContext(w, h, max_pts=64) as c:
        c.set_undistort(cam, dist, new_K)
        c.push_frame(tex)
        want = um.undistort(tex, cam, dist, new_K)
        assert (want != tex).mean() > 0.3
        _store_equals(c, want)
        c.set_prefilter()                                                  # undistortion first, then the bilateral filter
        c.push_frame(noise)
        assert np.array_equal(c.pyramid_read(1, 0)[0], o.bilateral(um.undistort(noise, cam, dist, new_K)))
        _store_equals(c, want, which=0)                                    # the previous frame is still there
        c.set_prefilter(0); c.clear_undistort()
        assert c.get_undistort() is None
        c.push_frame(noise)
        assert np.array_equal(c.pyramid_read(1, 0)[0], noise)


def test_resident_frames_of_a_batch_feed_pyramid_and_tracker():
    import vo_oracle as o
    from vo_mi355x import VoContext, synthetic as syn
    w, h, n = 640, 240, 400
    cam, dist = _cam(w, h), (-0.12, 0.03, 0.001, -0.0008, 0.002)
    fa, _ = syn.make_sequence(3, w=w, h=h, seed=31, margin=64)
    fb, _ = syn.make_sequence(3, w=w, h=h, seed=32, margin=64)
    pts = syn.grid_points(n, w, h, seed=2)
    with VoContext(w, h, max_pts=512, batch=2) as c:
        c.set_undistort(cam, dist)
        c.upload_sequence(np.stack([fa, fb]))
        c.points_upload(np.stack([pts, pts]))
        c.push_frame_resident(0)
        c.push_frame_resident(1)
        c.klt_track_resident(n)
        p1, st, err = c.points_download(n)
        for b, fr in enumerate((fa, fb)):
            f0, f1 = um.undistort(fr[0], cam, dist), um.undistort(fr[1], cam, dist)
            assert (f1 != fr[1]).mean() > 0.3
            _store_equals(c, f1, seq=b)
            _store_equals(c, f0, seq=b, which=0)
            q1, qs, qe = o.klt(f0, f1, pts)
            assert np.array_equal(p1[b], q1) and np.array_equal(st[b], qs) and np.array_equal(err[b], qe)
            assert qs.sum() > n // 2


# ---- 4. the fused frame steps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["launches", "graph"])
@pytest.mark.parametrize("host", [False, True], ids=["resident", "host"])
def test_fused_steps_see_undistorted_frames_and_every_change_of_the_setting(host, graph):
    """a context with undistortion, fed raw frames, against one without, fed the model's frames: outputs and stores, step by step.  The
    setting changes between steps whose launch lists are otherwise identical -- set A twice over both store parities (capture, then replay),
    set B (a new table behind the same pointers), off: a stale captured step would show the earlier setting"""
    from vo_mi355x import VoContext, synthetic as syn
    w, h, n = 320, 240, 300
    cam = _cam(w, h)
    A, B = ((-0.2, 0.05, 0.0, 0.0), None), ((0.1, 0.0, 0.002, 0.001, 0.0), (0.7 * w, 0.7 * w, 0.5 * w, 0.5 * h))
    plan = [A, A, A, A, B, B, None, None, A]
    frames, _ = syn.make_sequence(4, w=w, h=h, seed=21, margin=64)
    order = [1, 2, 3, 2, 1, 2, 3, 2, 1]
    pts = syn.grid_points(n, w, h, seed=4)
    fed = [frames[f] if s is None else um.undistort(frames[f], cam, s[0], s[1]) for f, s in zip(order, plan)]
    with ih.fused_pair(w, h, frames, pts, graph, graph, frames[0]) as (a, b):
        def after(k, f, s):
            assert np.array_equal(a.pyramid_read(1, 0)[0], fed[k]), k
        ih.fused_plan(a, b, frames, order, plan, fed, n, host, lambda s: a.clear_undistort() if s is None else a.set_undistort(cam, s[0], s[1]),
                      after)


# ---- 5. the closed loop -------------------------------------------------------------------------------------------------------------------
LOOP_DIST = (-0.02, 0.004, 0.0003, -0.0002)          # about a pixel at the corners: the rendered scene's geometry survives it


@pytest.fixture(scope="module")
def loop_scene():
    return ih.loop_scene(lambda f, sc: um.undistort(f, sc["K"], LOOP_DIST))


@pytest.mark.parametrize("side,inflight", [(True, 1), (False, 1), (True, 4)], ids=["side", "one_stream", "side_inflight"])
@pytest.mark.parametrize("host", [False, True], ids=["step", "step_host"])
def test_closed_loop_equals_a_loop_fed_the_models_frames(loop_scene, host, side, inflight):
    sc, state, und = loop_scene
    run_a = ih.run_loop(sc, state, sc["frames"], host, side, inflight, "get_undistort", undistort=dict(K=sc["K"], dist=LOOP_DIST))
    run_b = ih.run_loop(sc, state, und, host, side, inflight, "get_undistort")
    ra = run_a[0]
    assert sum(r["n_tracked"] for r in ra) > 100
    print("closed loop with undistortion: status %s, tracked %s" % ([r["status"] for r in ra], [r["n_tracked"] for r in ra]))
    ih.same_loop(run_a, run_b)


def test_pipeline_camera_must_be_the_undistorted_camera(loop_scene):
    from vo_mi355x import VoContext
    from vo_mi355x.resident import ResidentPipeline
    sc = loop_scene[0]
    Kp = np.asarray(sc["K"], np.float64)
    new_K = (200.0, 200.0, 128.0, 80.0)
    N3 = np.array([[200.0, 0, 128.0], [0, 200.0, 80.0], [0, 0, 1.0]])
    with VoContext(W, H, max_pts=256) as c:
        with pytest.raises(ValueError):
            ResidentPipeline(c, Kp, undistort=dict(K=Kp, dist=LOOP_DIST, new_K=new_K))      # frames come out in new_K's camera
        with pytest.raises(ValueError):
            ResidentPipeline(c, N3, undistort=dict(K=Kp, dist=LOOP_DIST))                   # ... and in K's without one
        with pytest.raises(ValueError):
            ResidentPipeline(c, Kp, undistort=dict(K=Kp, dist=LOOP_DIST, newK=new_K))       # unknown key
        assert c.get_undistort() is None
        ResidentPipeline(c, N3, undistort=dict(K=Kp, dist=LOOP_DIST, new_K=new_K))
        assert np.array_equal(c.get_undistort()["new_K"], new_K)
        ResidentPipeline(c, Kp)                                                             # None switches a context's setting off
        assert c.get_undistort() is None


# ---- 6. the drop-in Extractor ---------------------------------------------------------------------------------------------------------------
def test_dropin_extractor_tracks_on_undistorted_images():
    from vo_mi355x import synthetic as syn
    from vo_mi355x.extractor import Extractor
    w, h = 320, 240
    cam, dist = _cam(w, h), (-0.15, 0.02, 0.001, 0.0005)
    frames, _ = syn.make_sequence(2, w=w, h=h, seed=9, margin=64)
    u0, u1 = um.undistort(frames[0], cam, dist), um.undistort(frames[1], cam, dist)
    with pytest.raises(ValueError):
        Extractor(lazy=False, undistort=dict(dist=dist))
    plain, und = Extractor(lazy=False), Extractor(undistort=dict(K=cam, dist=dist))
    kp_p = plain.extract(u0, 0, [], detector='shi-tomasi', mask_radius=7)
    kp_u = und.extract(frames[0], 0, [], detector='shi-tomasi', mask_radius=7)
    assert len(kp_p) == len(kp_u) > 50
    assert all(np.array_equal(x.uv, y.uv) for x, y in zip(kp_p, kp_u))
    plain._im_prev, und._im_prev = u0, frames[0]
    out_p = plain.extend_tracks(u1, kp_p, max_bidir_error=np.inf)
    out_u = und.extend_tracks(frames[1], kp_u, max_bidir_error=np.inf)
    assert len(out_p) == len(out_u) > 30
    for x, y in zip(out_p, out_u):
        assert np.array_equal(x.uv, y.uv) and x.t_total == y.t_total and len(x.uv_history) == len(y.uv_history)
    assert any(not np.array_equal(k.uv, k.uv_first) for k in out_u)


# ---- 7. argument and state errors -------------------------------------------------------------------------------------------------------------
def _raw_set(c, K4, dist, n_dist, new_K):
    import ctypes as C
    arr = lambda v: None if v is None else (C.c_double * len(v))(*v)
    return c._L.vo_set_undistort(c._h, arr(K4), arr(dist), n_dist, arr(new_K))


def test_every_refusal_leaves_the_setting_and_the_next_frame_as_they_were():
    from vo_mi355x import VoContext
    w, h = 203, 97
    img = _images(w, h)[1]
    good = (-0.2, 0.03, 0.0, 0.0)
    nan, inf = float("nan"), float("inf")
    bad = [(K, (0.1,) * 8, 3, None), (K, (0.1,) * 8, 6, None), (K, (0.1,) * 8, 9, None), (K, (0.1,) * 8, -1, None),     # n_dist
           (K, None, 4, None),                                                                                          # dist == NULL
           ((nan,) + K[1:], good, 4, None), (K[:2] + (inf, K[3]), good, 4, None), (K, (0.1, nan, 0, 0), 4, None),       # not finite
           (K, (0.1, 0, 0, 0, -inf), 5, None), (K, good, 4, (200.0, nan, 1.0, 1.0)),
           ((0.0,) + K[1:], good, 4, None), ((K[0], -1.0) + K[2:], good, 4, None),                                      # focal lengths
           (K, good, 4, (0.0, 200.0, 1.0, 1.0)), (K, good, 4, (200.0, -3.0, 1.0, 1.0))]
    with VoContext(w, h, max_pts=64) as c:
        assert _code(lambda: c.undistort(img)) == -4 and _code(c.undistort_map_read) == -4                              # nothing set yet
        for args in bad:
            assert _raw_set(c, *args) == -1, args
            assert c.get_undistort() is None
        c.push_frame(img)
        assert np.array_equal(c.pyramid_read(1, 0)[0], img)
        c.set_undistort(K, good)
        before, tab = c.get_undistort(), c.undistort_map_read()
        for args in bad:
            assert _raw_set(c, *args) == -1, args
        after = c.get_undistort()
        assert all(np.array_equal(before[k], after[k]) for k in before)
        assert all(np.array_equal(tab[k], v) for k, v in c.undistort_map_read().items())
        c.push_frame(img)
        assert np.array_equal(c.pyramid_read(1, 0)[0], um.undistort(img, K, good))
        with pytest.raises(ValueError):
            c.set_undistort(np.eye(2), good)
        with pytest.raises(ValueError):
            c.undistort(img.astype(np.float32))
        c.clear_undistort()
        assert _code(lambda: c.undistort(img)) == -4 and _code(c.undistort_map_read) == -4
