"""GPU: CLAHE (cv2.createCLAHE(..).apply restated by tests/clahe_model.py) on every frame-ingest path.

Every comparison with the model is exact: integer histograms, three float32 divisions made on the host, float32 arithmetic with no fused
multiply-add behind them.  1. the tables and the synchronous call on the smallest shapes at which each branch can go wrong; 2. the ingest
paths (push_frame, push_frame_resident, the tracker and the detector), alone and with undistortion and the bilateral pre-filter around it;
3. the fused frame steps with and without graph replay, the setting switched between steps; 4. the closed loop on every stream layout;
5. the drop-in Extractor; 6. errors."""
import numpy as np
import pytest

import clahe_model as cm
import ingest_helpers as ih
import undistort_model as um
from ingest_helpers import H, W, code as _code, same_store as _same_store

pytestmark = pytest.mark.gpu

# (w, h, tiles): no extension; width remainder and full extra rows; height remainder and full extra columns; non-square non-default tiles;
# one tile (both clamps collapse to tile 0); 7 x 5 tiles (clip at its floor of 1, residual path with step > 1)
SHAPES = [(96, 64, (8, 8)), (99, 64, (8, 8)), (96, 61, (8, 8)), (101, 67, (4, 3)), (101, 67, (1, 1)), (99, 67, (16, 16))]
IDS = ["%dx%d_%dx%d" % (w, h, t[0], t[1]) for w, h, t in SHAPES]
CLIPS = (0.0, 0.5, 2.0, 40.0)


def _images(w, h):
    """two batches of three: (zeros, full, checker), (ramp, noise, narrow noise)"""
    rng = np.random.default_rng(w * 1000 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([np.zeros((h, w), np.uint8), np.full((h, w), 255, np.uint8),
                  np.where(((xx // 5) + (yy // 3)) % 2 == 0, 40, 200).astype(np.uint8)])
    b = np.stack([np.tile((np.arange(w) * 255 // (w - 1)).astype(np.uint8), (h, 1)), rng.integers(0, 256, (h, w)).astype(np.uint8),
                  rng.integers(100, 111, (h, w)).astype(np.uint8)])
    return a, b


# ---- 1. the tables and the synchronous call -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,tiles", SHAPES, ids=IDS)
def test_tables_and_synchronous_call_equal_the_model(w, h, tiles):
    from vo_mi355x import VoContext
    with VoContext(w, h, max_pts=64, batch=3) as c:
        for clip in CLIPS:
            c.set_clahe(clip, tiles)
            assert c.get_clahe() == (clip, tiles)
            assert not c.clahe_lut_read().any()                            # no launch of this setting yet
            for k, batch in enumerate(_images(w, h)):
                got = c.clahe(batch)
                lut = c.clahe_lut_read()
                assert got.shape == (3, h, w) and got.dtype == np.uint8 and lut.shape == (3, tiles[1], tiles[0], 256)
                wide = np.full((3, h, w + 29), 77, np.uint8)               # rows 29 bytes further apart than they are long
                wide[:, :, :w] = batch
                got_wide = c.clahe(wide[:, :, :w])
                for s in range(3):
                    want_lut = cm.luts(batch[s], clip, tiles)
                    assert np.array_equal(lut[s], want_lut), (clip, k, s, int((lut[s] != want_lut).sum()))
                    want = cm.interpolate(batch[s], want_lut, tiles)
                    assert np.array_equal(got[s], want), (clip, k, s, int((got[s] != want).sum()))
                    assert np.array_equal(got_wide[s], want), (clip, k, s, "stride")


def test_synchronous_call_leaves_the_frame_store_alone_and_skips_the_undistortion():
    from vo_mi355x import VoContext
    w, h = 99, 67
    a, b = _images(w, h)
    with VoContext(w, h, max_pts=64, batch=3) as c:
        c.push_frame(b); c.push_frame(a)
        before = [c.pyramid_read(which, 0, seq=s) for which in (0, 1) for s in range(3)]
        c.set_undistort((80.0, 78.0, 49.0, 33.0), (-0.2, 0.05, 0.0, 0.0))
        c.set_clahe(2.0, (4, 3))
        got = c.clahe(b)
        for s in range(3):
            assert np.array_equal(got[s], cm.clahe(b[s], 2.0, (4, 3)))     # CLAHE alone
        after = [c.pyramid_read(which, 0, seq=s) for which in (0, 1) for s in range(3)]
        for x, y in zip(before, after):
            assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


# ---- 2. the ingest paths --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h,tiles", [SHAPES[1], SHAPES[2], SHAPES[5]], ids=[IDS[1], IDS[2], IDS[5]])
def test_pushed_frames_enter_the_store_equalised(w, h, tiles):
    from vo_mi355x import VoContext
    _, b = _images(w, h)
    with VoContext(w, h, max_pts=64, batch=3) as c, VoContext(w, h, max_pts=64, batch=3) as ref:
        c.set_clahe(2.0, tiles)
        c.push_frame(b)
        want = np.stack([cm.clahe(b[s], 2.0, tiles) for s in range(3)])
        assert (want != b).mean() > 0.3
        ref.push_frame(want)
        for s in range(3):
            assert np.array_equal(c.pyramid_read(1, 0, seq=s)[0], want[s])
            assert np.array_equal(c.clahe_lut_read()[s], cm.luts(b[s], 2.0, tiles))
            _same_store(c, ref, seq=s, levels=1)
        c.clear_clahe()
        assert c.get_clahe() is None
        c.push_frame(b)
        for s in range(3):
            assert np.array_equal(c.pyramid_read(1, 0, seq=s)[0], b[s])


def _cam(w, h):
    return (0.8 * w, 0.78 * w, 0.49 * w + 0.3, 0.51 * h - 0.3)


UND_DIST = (-0.12, 0.03, 0.001, -0.0008, 0.002)


def test_the_chain_is_undistort_then_clahe_then_the_bilateral_filter():
    import vo_oracle as o
    from vo_mi355x import VoContext, synthetic as syn
    w, h, tiles, clip = 323, 123, (8, 8), 3.0
    cam = _cam(w, h)
    tex = syn.make_sequence(1, w=w, h=h, seed=5, margin=32)[0][0]
    und = um.undistort(tex, cam, UND_DIST)
    want = cm.clahe(und, clip, tiles)
    other = um.undistort(cm.clahe(tex, clip, tiles), cam, UND_DIST)
    assert (want != other).mean() > 0.05                                   # the two orders differ: the test can tell them apart
    with VoContext(w, h, max_pts=64) as c:
        c.set_undistort(cam, UND_DIST)
        c.set_clahe(clip, tiles)
        c.push_frame(tex)
        assert np.array_equal(c.pyramid_read(1, 0)[0], want)
        assert np.array_equal(c.clahe_lut_read(), cm.luts(und, clip, tiles))
        c.set_prefilter()
        c.push_frame(tex)
        assert np.array_equal(c.pyramid_read(1, 0)[0], o.bilateral(want))
        c.clear_undistort()
        c.push_frame(tex)
        assert np.array_equal(c.pyramid_read(1, 0)[0], o.bilateral(cm.clahe(tex, clip, tiles)))
        c.set_prefilter(0); c.clear_clahe()
        c.push_frame(tex)
        assert np.array_equal(c.pyramid_read(1, 0)[0], tex)


def test_resident_frames_of_a_batch_feed_pyramid_tracker_and_detector():
    from vo_mi355x import VoContext, synthetic as syn
    w, h, n, tiles, clip = 642, 241, 400, (8, 8), 4.0                       # both sides leave a remainder
    fa, _ = syn.make_sequence(3, w=w, h=h, seed=31, margin=64)
    fb, _ = syn.make_sequence(3, w=w, h=h, seed=32, margin=64)
    pts = syn.grid_points(n, w, h, seed=2)
    raw = np.stack([fa, fb])
    eq = np.stack([[cm.clahe(f, clip, tiles) for f in fr] for fr in raw])
    assert (eq != raw).mean() > 0.3
    with VoContext(w, h, max_pts=512, batch=2) as c, VoContext(w, h, max_pts=512, batch=2) as ref:
        c.set_clahe(clip, tiles)
        out = []
        for ctx, frames in ((c, raw), (ref, eq)):
            ctx.upload_sequence(frames)
            ctx.points_upload(np.stack([pts, pts]))
            ctx.push_frame_resident(0)
            ctx.push_frame_resident(1)
            ctx.klt_track_resident(n)
            out.append(ctx.points_download(n))
        for b in range(2):
            _same_store(c, ref, seq=b)
            _same_store(c, ref, seq=b, which=0)
            assert np.array_equal(c.pyramid_read(1, 0, seq=b)[0], eq[b, 1])
        for x, y in zip(out[0], out[1]):
            assert np.array_equal(x, y)
        assert out[0][1].sum() > n // 2


# ---- 3. the fused frame steps ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["launches", "graph"])
@pytest.mark.parametrize("host", [False, True], ids=["resident", "host"])
def test_fused_steps_see_equalised_frames_and_every_change_of_the_setting(host, graph):
    """a context with CLAHE, fed raw frames, against one without, fed the model's frames: outputs and stores, step by step.  The setting
    changes between steps whose launch lists are otherwise identical -- A over both store parities twice (capture, then replay), B (same
    buffers, other tiles and clip), off, A again: a stale captured step would show the earlier setting"""
    from vo_mi355x import VoContext, synthetic as syn
    w, h, n = 322, 240, 300
    A, B = (40.0, (8, 8)), (1.5, (5, 3))
    plan = [A, A, A, A, B, B, None, None, A]
    frames, _ = syn.make_sequence(4, w=w, h=h, seed=21, margin=64)
    order = [1, 2, 3, 2, 1, 2, 3, 2, 1]
    pts = syn.grid_points(n, w, h, seed=4)
    fed = [frames[f] if s is None else cm.clahe(frames[f], s[0], s[1]) for f, s in zip(order, plan)]
    with ih.fused_pair(w, h, frames, pts, graph, graph, frames[0]) as (a, b):
        def after(k, f, s):
            assert np.array_equal(a.pyramid_read(1, 0)[0], fed[k]), k
            if s is not None:
                assert np.array_equal(a.clahe_lut_read(), cm.luts(frames[f], s[0], s[1])), k
        ih.fused_plan(a, b, frames, order, plan, fed, n, host, lambda s: a.clear_clahe() if s is None else a.set_clahe(*s), after)


def test_fused_steps_with_undistortion_and_the_bilateral_filter_around_it():
    from vo_mi355x import VoContext, synthetic as syn
    w, h, n, tiles, clip = 322, 240, 300, (8, 8), 40.0
    cam = _cam(w, h)
    frames, _ = syn.make_sequence(3, w=w, h=h, seed=22, margin=64)
    pts = syn.grid_points(n, w, h, seed=4)
    fed = [cm.clahe(um.undistort(f, cam, UND_DIST), clip, tiles) for f in frames]
    with VoContext(w, h, max_pts=512) as a, VoContext(w, h, max_pts=512) as b:
        a.set_undistort(cam, UND_DIST); a.set_clahe(clip, tiles)
        for c in (a, b):
            c.set_prefilter()
            c.points_upload(pts)
        a.upload_sequence(frames)
        a.push_frame_resident(0); b.push_frame(fed[0])
        for k in (1, 2):
            a.frame_step_resident(k, n, do_dlt=False, do_ba=False) if k == 1 else a.frame_step_host(frames[k].copy(), n, do_dlt=False, do_ba=False)
            b.frame_step_host(fed[k], n, do_dlt=False, do_ba=False)
            ga, gb = a.frame_fetch(), b.frame_fetch()
            for key in ("points2d", "status", "err", "corners"):
                assert np.array_equal(ga[key], gb[key]), (k, key)
            _same_store(a, b)


# ---- 4. the closed loop ---------------------------------------------------------------------------------------------------------------
LOOP_CLAHE = (3.0, (5, 3))                                                 # 256 % 5 and 160 % 3 both leave a remainder


@pytest.fixture(scope="module")
def loop_scene():
    return ih.loop_scene(lambda f, sc: cm.clahe(f, *LOOP_CLAHE))


@pytest.mark.parametrize("side,inflight", [(True, 1), (False, 1), (True, 4)], ids=["side", "one_stream", "side_inflight"])
@pytest.mark.parametrize("host", [False, True], ids=["step", "step_host"])
def test_closed_loop_equals_a_loop_fed_the_models_frames(loop_scene, host, side, inflight):
    sc, state, eq = loop_scene
    run_a = ih.run_loop(sc, state, sc["frames"], host, side, inflight, "get_clahe", clahe=LOOP_CLAHE)
    run_b = ih.run_loop(sc, state, eq, host, side, inflight, "get_clahe")
    ra = run_a[0]
    print("closed loop with CLAHE: status %s, tracked %s" % ([r["status"] for r in ra], [r["n_tracked"] for r in ra]))
    assert sum(r["n_tracked"] for r in ra) > 0                             # the comparison below is not of two empty loops
    ih.same_loop(run_a, run_b)


def test_pipeline_argument_sets_and_clears_the_contexts_setting(loop_scene):
    from vo_mi355x import VoContext
    from vo_mi355x.resident import ResidentPipeline
    sc = loop_scene[0]
    with VoContext(W, H, max_pts=256) as c:
        with pytest.raises(ValueError):
            ResidentPipeline(c, sc["K"], clahe=(2.0, 8))                   # tiles is a pair
        with pytest.raises(ValueError):
            ResidentPipeline(c, sc["K"], clahe=dict(clip=2.0))             # unknown key
        assert c.get_clahe() is None
        ResidentPipeline(c, sc["K"], clahe=dict(clip_limit=2.0, tiles=(4, 4)))
        assert c.get_clahe() == (2.0, (4, 4))
        ResidentPipeline(c, sc["K"])                                       # None switches a context's setting off
        assert c.get_clahe() is None


# ---- 5. the drop-in Extractor ---------------------------------------------------------------------------------------------------------
def test_dropin_extractor_tracks_on_equalised_images():
    from vo_mi355x import synthetic as syn
    from vo_mi355x.extractor import Extractor
    w, h, cl = 322, 240, (40.0, (8, 8))
    frames, _ = syn.make_sequence(2, w=w, h=h, seed=9, margin=64)
    e0, e1 = cm.clahe(frames[0], *cl), cm.clahe(frames[1], *cl)
    with pytest.raises(ValueError):
        Extractor(lazy=False, clahe=(40.0, 8))
    plain, eq = Extractor(lazy=False), Extractor(clahe=cl)
    kp_p = plain.extract(e0, 0, [], detector='shi-tomasi', mask_radius=7)
    kp_e = eq.extract(frames[0], 0, [], detector='shi-tomasi', mask_radius=7)
    assert len(kp_p) == len(kp_e) > 50
    assert all(np.array_equal(x.uv, y.uv) for x, y in zip(kp_p, kp_e))
    plain._im_prev, eq._im_prev = e0, frames[0]
    out_p = plain.extend_tracks(e1, kp_p, max_bidir_error=np.inf)
    out_e = eq.extend_tracks(frames[1], kp_e, max_bidir_error=np.inf)
    assert len(out_p) == len(out_e) > 30
    for x, y in zip(out_p, out_e):
        assert np.array_equal(x.uv, y.uv) and x.t_total == y.t_total and len(x.uv_history) == len(y.uv_history)
    assert any(not np.array_equal(k.uv, k.uv_first) for k in out_e)


# ---- 6. argument and state errors -----------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_setting_and_the_next_frame_as_they_were():
    from vo_mi355x import VoContext
    w, h = 16, 9
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (h, w)).astype(np.uint8)
    nan, inf = float("nan"), float("inf")
    bad = [(-1.0, 4, 3), (-1e-300, 4, 3), (nan, 4, 3), (inf, 4, 3), (-inf, 4, 3),                                 # clip_limit
           (2.0, 0, 3), (2.0, 4, 0), (2.0, 17, 3), (2.0, 4, 17), (2.0, -1, 3), (2.0, 4, -8),                      # tiles outside 1 .. 16
           (2.0, 16, 16)]      # 16 % 16 == 0 but 9 % 16 != 0: BOTH sides grow, the width by a whole 16 columns -- not smaller than 16
    # accepted: 9 % 10 = 9 -> 1 extra row, and the width (16 % 1 == 0) still grows by 1; 16 % 3 = 1 -> 2 extra columns, 9 % 16 -> 7 extra rows
    valid = [(2.0, 1, 10), (2.0, 3, 16)]
    with VoContext(w, h, max_pts=16) as c:
        assert _code(lambda: c.clahe(img)) == -4 and _code(c.clahe_lut_read) == -4                                # nothing set yet
        for args in bad:
            assert c._L.vo_set_clahe(c._h, *args) == -1, args
            assert c.get_clahe() is None
        c.push_frame(img)
        assert np.array_equal(c.pyramid_read(1, 0)[0], img)                # nothing was enqueued in front of level 0
        for args in valid:
            c.set_clahe(args[0], args[1:])
            assert np.array_equal(c.clahe(img), cm.clahe(img, args[0], args[1:]))
        c.set_clahe(2.0, (4, 3))
        tab = cm.luts(img, 2.0, (4, 3))
        assert np.array_equal(c.clahe(img), cm.interpolate(img, tab, (4, 3)))
        for args in bad:
            assert c._L.vo_set_clahe(c._h, *args) == -1, args
            assert c.get_clahe() == (2.0, (4, 3))
            assert np.array_equal(c.clahe_lut_read(), tab)                 # no launch and no reset of the tables either
        c.push_frame(img)
        assert np.array_equal(c.pyramid_read(1, 0)[0], cm.clahe(img, 2.0, (4, 3)))
        with pytest.raises(ValueError):
            c.clahe(img.astype(np.float32))
        with pytest.raises(ValueError):
            c.set_clahe(2.0, 8)
        c.clear_clahe()
        assert _code(lambda: c.clahe(img)) == -4 and _code(c.clahe_lut_read) == -4
    with VoContext(8, 9, max_pts=16) as c:
        # 8 % 16 = 8: 8 extra columns, not smaller than the 8 the image has
        assert c._L.vo_set_clahe(c._h, 2.0, 16, 1) == -1 and c.get_clahe() is None
        # 9 % 8 = 1 forces both: 8 % 8 == 0 still grows by 8 columns
        assert c._L.vo_set_clahe(c._h, 2.0, 8, 8) == -1 and c.get_clahe() is None
        c.set_clahe(2.0, (8, 9))                                           # both divide: no extension at all
        assert c.get_clahe() == (2.0, (8, 9))
