"""GPU: sub-pixel corner refinement (csrc/vo_subpix.hip; vo_corner_subpix / vo_set_subpix / vo_get_subpix / vo_subpix_read) through every
layer.

The contract is the numpy model tests/subpix_model.py (cv2.cornerSubPix restated; shown against analytic truth by
tests/test_subpix_model.py): positions, iteration counts and flags of k_corner_subpix equal it bit for bit.  The resident detections --
the track table's and the closed loop's -- are pinned against the synchronous call on the integer corners of a context that does not
refine, and everything else those detections write must be identical between the two."""
import copy

import numpy as np
import pytest

import pipe_helpers as ph
import subpix_model as sm

pytestmark = pytest.mark.gpu

WIN7 = dict(win=(7, 7), zero=(-1, -1), max_count=40, eps=0.001)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _prm(c, p):
    return c.subpix_params(win=p["win"], zero_zone=p["zero"], max_count=p["max_count"], epsilon=p["eps"])


def _same(got, want, what=""):
    """(out, iters, flags) bit for bit"""
    bad = np.nonzero((_bits(got[0]) != _bits(want[0])).any(-1) | (got[1] != want[1]) | (got[2] != want[2]))[0]
    assert len(bad) == 0, (what, bad[:5], got[0][bad[:5]], want[0][bad[:5]], got[1][bad[:5]], want[1][bad[:5]], got[2][bad[:5]], want[2][bad[:5]])


def _with_block(img, x0, y0):
    """the image with a constant 40 x 40 block at (x0, y0): a corner in its middle is singular"""
    img = img.copy()
    img[y0:y0 + 40, x0:x0 + 40] = 91
    return img


def _hostile(corners, w, h, win, block, n_max):
    """the corner set of a test: detected corners, rows within win + 1 of every border (integer and fractional), the four image corners,
    one in the constant block, one NaN, rows outside; n is not a multiple of 4"""
    m = win + 1
    extra = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (m - 0.5, h / 2), (w - m, h / 3), (w / 2, m - 1.25), (w / 3, h - m + 0.5),
             (1, h / 2 + 3), (w - 1.25, h / 2 - 3), (w / 2 + 5, 0.5), (w / 2 - 5, h - 1), (block[0] + 20, block[1] + 20),
             (np.nan, 9), (w, 5), (5, -0.5), (w - 0.5, h - 0.5)]
    out = np.concatenate([np.asarray(extra, np.float32), np.asarray(corners, np.float32)])[:n_max]
    if len(out) % 4 == 0:
        out = out[:-1]
    return out


@pytest.fixture(scope="module")
def images():
    board, truth = sm.checkerboard(320, 240, 24, 0.2)
    board = _with_block(board, 200, 30)
    noise = _with_block(sm.noise_image(320, 240, 5), 40, 150)
    wide = _with_block(sm.noise_image(1241, 376, 6), 900, 200)
    return dict(board=(board, sm.board_starts(truth, 11), (200, 30)), noise=(noise, sm.eig_maxima(noise), (40, 150)),
                wide=(wide, sm.eig_maxima(wide)[::9], (900, 200)))


# ---- 1. the synchronous call = the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prm", [sm.DEFAULTS, WIN7], ids=["default", "win7"])
@pytest.mark.parametrize("name", ["board", "noise", "wide"])
def test_corner_subpix_is_the_model(images, name, prm):
    from vo_mi355x import VoContext
    img, corners, block = images[name]
    h, w = img.shape
    pts = _hostile(corners, w, h, prm["win"][0], block, 150 if name != "wide" else 110)
    assert len(pts) % 4 and len(pts) <= 300
    want = sm.corner_subpix_np(img, pts, **prm)
    counts = np.bincount(want[2], minlength=5)
    print(name, prm["win"], len(pts), "corners, flags 0..4:", counts, "iters max", want[1].max())
    assert counts[0] > 0 and counts[1] > 0 and counts[4] >= 3
    with VoContext(w, h, max_pts=512) as c:
        c.push_frame(img)
        got = c.corner_subpix(pts, "cur", _prm(c, prm), return_info=True)
        _same(got, want, name)
        assert np.array_equal(_bits(c.corner_subpix(pts, params=_prm(c, prm))), _bits(want[0]))
        if prm is sm.DEFAULTS:                       # no parameters = the defaults
            assert np.array_equal(_bits(c.corner_subpix(pts)), _bits(want[0]))


def test_small_window_zero_zone_and_few_iterations(images):
    """win = (3, 4) (a window that is not square), a zero zone, max_count = 5, a coarse epsilon; max_count and epsilon clamp like the model"""
    from vo_mi355x import VoContext
    img, corners, block = images["noise"]
    h, w = img.shape
    pts = _hostile(corners, w, h, 4, block, 101)
    with VoContext(w, h, max_pts=512) as c:
        c.push_frame(img)
        for p in (dict(win=(3, 4), zero=(1, 1), max_count=5, eps=0.01), dict(win=(1, 7), zero=(0, 2), max_count=0, eps=-1.0),
                  dict(win=(6, 2), zero=(6, 0), max_count=1000, eps=0.25)):
            want = sm.corner_subpix_np(img, pts, **p)
            _same(c.corner_subpix(pts, "cur", _prm(c, p), return_info=True), want, str(p))
        assert want[1].max() <= 100


def test_which_selects_the_frame(images):
    from vo_mi355x import VoContext
    board, starts, _ = images["board"]
    noise = images["noise"][0]
    pts = starts[:61]
    with VoContext(320, 240, max_pts=64) as c:
        c.push_frame(board); c.push_frame(noise)
        on_prev, on_cur = sm.corner_subpix_np(board, pts), sm.corner_subpix_np(noise, pts)
        assert not np.array_equal(on_prev[0], on_cur[0])
        _same(c.corner_subpix(pts, "prev", return_info=True), on_prev, "prev")
        _same(c.corner_subpix(pts, "cur", return_info=True), on_cur, "cur")
        _same(c.corner_subpix(pts, 0, return_info=True), on_prev, "0")
        c.push_frame(board)                          # the store's halves swap
        _same(c.corner_subpix(pts, "prev", return_info=True), on_cur, "prev after a push")
        _same(c.corner_subpix(pts, 1, return_info=True), on_prev, "cur after a push")
        z = c.corner_subpix(np.zeros((0, 2), np.float32), return_info=True)
        assert z[0].shape == (0, 2) and z[1].shape == (0,)


# ---- 2. a batch ------------------------------------------------------------------------------------------------------------------------------
def test_batched_context_equals_single_contexts():
    """batch = 8 (the XCD remap), a frame per sequence, unequal counts padded with NaN rows: every sequence = its own context's result"""
    from vo_mi355x import VoContext
    B, w, h = 8, 160, 96
    imgs = np.stack([sm.noise_image(w, h, 20 + b) for b in range(B)])
    sets = [sm.eig_maxima(imgs[b])[: 50 - 5 * b] for b in range(B)]
    n = max(len(s) for s in sets)
    assert len({len(s) for s in sets}) > 3
    pts = np.full((B, n, 2), np.nan, np.float32)
    for b in range(B):
        pts[b, :len(sets[b])] = sets[b]
    with VoContext(w, h, max_pts=64, batch=B) as c:
        c.push_frame(imgs)
        out, it, fl = c.corner_subpix(pts, return_info=True)
    with VoContext(w, h, max_pts=64) as one:
        for b in range(B):
            one.push_frame(imgs[b])
            _same((out[b], it[b], fl[b]), one.corner_subpix(pts[b], return_info=True), "sequence %d" % b)
            k = len(sets[b])
            assert (fl[b, k:] == 4).all() and (it[b, k:] == 0).all() and np.isnan(out[b, k:]).all()
    _same((out[3], it[3], fl[3]), sm.corner_subpix_np(imgs[3], pts[3]), "sequence 3 against the model")


# ---- 3. the track table ----------------------------------------------------------------------------------------------------------------------
def test_track_table_spawns_refined_corners(seq_small):
    """two contexts on the same frames, one with set_subpix: after tracks_detect the refined context's new tracks sit where corner_subpix
    puts the other context's integer corners (uv, uv_first and the ring entry); everything else is identical"""
    from vo_mi355x import VoContext, VoError, synthetic as syn
    frames = seq_small[0]
    w, h = 320, 240
    seeds = syn.grid_points(60, w, h, margin=10, seed=4)
    prm = dict(win=(4, 4), max_count=20)
    with VoContext(w, h, max_pts=256) as a, VoContext(w, h, max_pts=256) as b:
        a.set_subpix(prm)
        got = a.get_subpix()
        assert (got.win_x, got.win_y, got.zero_x, got.zero_y, got.max_count, got.epsilon) == (4, 4, -1, -1, 20, 0.001)
        assert b.get_subpix() is None
        for c in (a, b):
            c.push_frame(frames[0]); c.tracks_seed(seeds, t=0)
            c.push_frame(frames[1]); c.tracks_track(1)
            c.tracks_detect(1, max_new=40)
        ra, rb = a.tracks_read(), b.tracks_read()
        for k in ("t_first", "t_total", "tag", "dead_tag"):
            assert np.array_equal(ra[k], rb[k]), k
        new = rb["t_first"] == 1
        assert new.sum() == 40 and not new[: len(new) - 40].any()
        assert np.array_equal(_bits(ra["uv"][~new]), _bits(rb["uv"][~new])) and np.array_equal(_bits(ra["uv_first"][~new]), _bits(rb["uv_first"][~new]))
        raw = rb["uv"][new]
        assert np.array_equal(raw, np.rint(raw))
        want, w_it, w_fl = b.corner_subpix(raw, "cur", b.subpix_params(**prm), return_info=True)
        assert (want != raw).any()                                         # (else the comparison below shows nothing)
        assert np.array_equal(_bits(ra["uv"][new]), _bits(want)) and np.array_equal(_bits(ra["uv_first"][new]), _bits(want))
        n = len(new)
        obs_a, obs_b = a.tracks_obs(1, 2), b.tracks_obs(1, 2)
        assert np.array_equal(obs_a[0, :n][new], want.astype(np.float64)) and np.isnan(obs_a[1, :n][new]).all()
        assert np.array_equal(obs_a[:, :n][:, ~new], obs_b[:, :n][:, ~new], equal_nan=True)
        info = a.subpix_read()
        assert len(info["raw"]) >= 40                                     # every detected corner was refined, the first max_new were spawned
        assert np.array_equal(info["raw"][:40], raw) and np.array_equal(info["iters"][:40], w_it) and np.array_equal(info["flags"][:40], w_fl)
        assert np.array_equal(a.shi_tomasi_fetch()[:40], want)            # the detection's rows hold the refined corners
        with pytest.raises(VoError) as ei:
            b.subpix_read()                                               # this context's detection did not refine
        assert ei.value.code == -4
        # the next frame tracks from the refined positions; switched off, a detection forgets the rows
        a.push_frame(frames[2]); a.tracks_track(2)
        a.set_subpix(None); assert a.get_subpix() is None
        a.tracks_detect(2, max_new=10)
        r2 = a.tracks_read()
        born = r2["uv"][r2["t_first"] == 2]
        assert len(born) and np.array_equal(born, np.rint(born))
        with pytest.raises(VoError) as ei:
            a.subpix_read()
        assert ei.value.code == -4


# ---- 4. the closed loop ----------------------------------------------------------------------------------------------------------------------
W, H, T1 = 256, 160, 3


@pytest.fixture(scope="module")
def loop_scene():
    from vo_mi355x import VoContext
    sc = ph.scene(T1 + 8, w=W, h=H, f=260.0, seed=2024, pose_fn=lambda t: ph.sway_pose(t, period=24.0))
    with VoContext(W, H, max_pts=1024) as boot:
        state, t1 = ph.gt_bootstrap(boot, sc, 0, T1)
    assert t1 == T1
    return sc, state


def _loop(c, sc, state, **kw):
    from vo_mi355x.resident import ResidentPipeline
    rp = ResidentPipeline(c, sc["K"], ba_max_iters=12, pnp_blind_batches=8, **kw)
    rp.seed(copy.deepcopy(state), [], [], 1)
    c.upload_sequence(sc["frames"])
    c.push_frame_resident(T1)
    return rp


def test_closed_loop_detect_stage_spawns_refined_candidates(loop_scene):
    """a frame up to the adjustment on two contexts (identical: refinement only touches DETECT), then the DETECT stage alone: the refined
    context's new candidates = the synchronous refinement of the other context's; counts, lists and records identical"""
    from vo_mi355x import VoContext
    from vo_mi355x.resident import ALL, DETECT
    sc, state = loop_scene
    prm = dict(win=(5, 5), zero_zone=(-1, -1), max_count=40, epsilon=0.001)
    with VoContext(W, H, max_pts=1024) as a, VoContext(W, H, max_pts=1024) as b:
        ra_, rb_ = _loop(a, sc, state, subpix=prm), _loop(b, sc, state)
        assert a.get_subpix() is not None and b.get_subpix() is None
        recs = []
        for rp in (ra_, rb_):
            rp.step(T1 + 1, stages=ALL & ~DETECT); r0 = rp.fetch()
            rp.step(stages=DETECT); recs.append((r0, rp.fetch()))
        for x, y in zip(recs[0], recs[1]):
            for k, v in x.items():
                assert (np.array_equal(y[k], v, equal_nan=True) if isinstance(v, np.ndarray) else y[k] == v), k
        n_new = recs[0][1]["n_detected"]
        assert n_new > 30
        Ta, Tb = ra_.read_tables(), rb_.read_tables()
        assert np.array_equal(Ta["counts"], Tb["counts"])
        n_c = int(Tb["counts"][0, 0])
        rows = Tb["cand"][0, n_c - n_new:n_c]
        for name in Ta:
            if name not in ("k_uv", "k_uvfirst", "k_hist"):
                assert np.array_equal(Ta[name], Tb[name], equal_nan=Ta[name].dtype.kind == "f"), name
        raw = Tb["k_uv"][0, rows]
        assert np.array_equal(raw, np.rint(raw)) and (Tb["k_histlen"][0, rows] == 1).all()
        assert np.array_equal(_bits(Tb["k_uvfirst"][0, rows]), _bits(raw)) and np.array_equal(_bits(Tb["k_hist"][0, 0, rows]), _bits(raw))
        want, w_it, w_fl = b.corner_subpix(raw, "cur", b.subpix_params(**prm), return_info=True)
        assert (want != raw).any()                                         # (else the comparison below shows nothing)
        for name, got in (("k_uv", Ta["k_uv"][0, rows]), ("k_uvfirst", Ta["k_uvfirst"][0, rows]), ("k_hist", Ta["k_hist"][0, 0, rows])):
            assert np.array_equal(_bits(got), _bits(want)), name
        others = np.setdiff1d(np.arange(Ta["k_uv"].shape[1]), rows)
        for name in ("k_uv", "k_uvfirst"):
            assert np.array_equal(Ta[name][0, others], Tb[name][0, others], equal_nan=True), name
        assert np.array_equal(Ta["k_hist"][0][:, others], Tb["k_hist"][0][:, others], equal_nan=True)
        info = a.subpix_read()
        assert np.array_equal(info["raw"][:n_new], raw) and np.array_equal(info["iters"][:n_new], w_it) and np.array_equal(info["flags"][:n_new], w_fl)
        print("DETECT stage: %d new candidates, flags 0..4 %s, %d at max_count" % (n_new, np.bincount(w_fl, minlength=5), (w_it == 40).sum()))


def test_closed_loop_with_refinement_is_the_same_on_every_stream_layout(loop_scene):
    """three whole frames with refinement on: status 0; records and final tables bit-identical with the side stream on and off, and with
    INFLIGHT steps in flight instead of one; the candidates born in the last frame are not integer"""
    from vo_mi355x import VoContext
    from vo_mi355x.resident import INFLIGHT
    sc, state = loop_scene
    n = 3

    def run(side, inflight):
        with VoContext(W, H, max_pts=1024) as c:
            c.set_side_stream(side)
            rp = _loop(c, sc, state, subpix={})
            recs, pending = [], 0
            for s in range(n):
                rp.step(T1 + 1 + s); pending += 1
                if pending == inflight or s == n - 1:
                    while pending:
                        recs.append(rp.fetch()); pending -= 1
            return recs, rp.read_tables(), c.subpix_read()

    ra, Ta, ia = run(True, 1)
    assert all(r["status"] == 0 for r in ra)
    n_c = int(Ta["counts"][0, 0])
    last = Ta["cand"][0, n_c - ra[-1]["n_detected"]:n_c]
    assert len(last) and (Ta["k_uv"][0, last] != np.rint(Ta["k_uv"][0, last])).any()
    assert len(ia["raw"]) >= len(last) and np.array_equal(ia["raw"], np.rint(ia["raw"]))
    for side, inflight in ((False, 1), (True, INFLIGHT)):
        rb, Tb, ib = run(side, inflight)
        for s, (x, y) in enumerate(zip(ra, rb)):
            for k, v in x.items():
                assert (np.array_equal(y[k], v, equal_nan=True) if isinstance(v, np.ndarray) else y[k] == v), (side, inflight, s, k)
        for name in Ta:
            assert np.array_equal(Ta[name], Tb[name], equal_nan=Ta[name].dtype.kind == "f"), (side, inflight, name)
        for k in ia:
            assert np.array_equal(ia[k], ib[k]), (side, inflight, k)


# ---- 5. the drop-in Extractor -----------------------------------------------------------------------------------------------------------------
def test_dropin_extractor_refines_what_it_detects(seq_small):
    from vo_mi355x.extractor import Extractor
    img = seq_small[0][1]
    with pytest.raises(ValueError):
        Extractor(lazy=False, subpix=dict(window=(5, 5)))
    plain = Extractor(lazy=False).extract(img, 3, [], detector='shi-tomasi', mask_radius=7)
    raw = np.asarray([k.uv for k in plain], np.float32).reshape(-1, 2)
    assert len(raw) > 50 and np.array_equal(raw, np.rint(raw))
    for kw, prm in ((dict(), sm.DEFAULTS), (dict(win=(3, 4), zero_zone=(1, 1), criteria=(3, 5, 0.01)), dict(win=(3, 4), zero=(1, 1), max_count=5, eps=0.01))):
        want = sm.corner_subpix_np(img, raw, **prm)[0]
        kps = Extractor(subpix=kw).extract(img, 3, [], detector='shi-tomasi', mask_radius=7)
        assert len(kps) == len(raw)
        for k, q in zip(kps, want):
            assert (k.t_first, k.t_total, len(k.uv_history)) == (3, 1, 1)
            for v in (k.uv, k.uv_first, k.uv_history[0]):
                assert np.asarray(v).shape == (2, 1) and np.array_equal(_bits(np.asarray(v).reshape(2)), _bits(q))
    assert (want != raw).any()


# ---- 6. argument and state errors ---------------------------------------------------------------------------------------------------------------
def _code(fn):
    from vo_mi355x import VoError
    with pytest.raises(VoError) as ei:
        fn()
    return ei.value.code


@pytest.fixture()
def small_ctx():
    from vo_mi355x import VoContext
    with VoContext(64, 18, max_pts=16, win=5, max_level=0) as c:
        yield c


PTS = np.full((3, 2), 9, np.float32)


@pytest.mark.parametrize("win", [(0, 5), (5, 0), (8, 5), (5, 8), (-1, -1)])
def test_win_outside_1_to_7_is_invalid(small_ctx, win):
    c = small_ctx
    c.push_frame(np.zeros((18, 64), np.uint8))
    assert _code(lambda: c.corner_subpix(PTS, params=c.subpix_params(win=win))) == -1
    assert _code(lambda: c.set_subpix(dict(win=win))) == -1
    assert c.get_subpix() is None


def test_image_smaller_than_the_window_needs_is_invalid(small_ctx):
    c = small_ctx                                                         # 64 x 18: win_y = 7 needs 19 rows, 6 needs 17
    c.push_frame(np.zeros((18, 64), np.uint8))
    assert _code(lambda: c.corner_subpix(PTS, params=c.subpix_params(win=(5, 7)))) == -1
    assert _code(lambda: c.set_subpix(dict(win=(5, 7)))) == -1
    out, it, fl = c.corner_subpix(PTS, params=c.subpix_params(win=(7, 6)), return_info=True)
    assert np.array_equal(out, PTS) and (fl == 1).all() and (it == 0).all()        # a constant image: singular at once
    c.set_subpix(dict(win=(7, 6)))


def test_nan_epsilon_is_invalid(small_ctx):
    c = small_ctx
    c.push_frame(np.zeros((18, 64), np.uint8))
    assert _code(lambda: c.corner_subpix(PTS, params=c.subpix_params(epsilon=float("nan")))) == -1
    assert _code(lambda: c.set_subpix(dict(epsilon=float("nan")))) == -1


def test_more_corners_than_max_pts_is_invalid(small_ctx):
    c = small_ctx
    c.push_frame(np.zeros((18, 64), np.uint8))
    assert _code(lambda: c.corner_subpix(np.full((17, 2), 9, np.float32))) == -1
    assert c.corner_subpix(np.full((16, 2), 9, np.float32)).shape == (16, 2)


def test_frame_not_pushed_is_a_state_error(small_ctx):
    c = small_ctx
    assert _code(lambda: c.corner_subpix(PTS, "cur")) == -4
    c.push_frame(np.zeros((18, 64), np.uint8))
    assert _code(lambda: c.corner_subpix(PTS, "prev")) == -4
    assert c.corner_subpix(PTS, "cur").shape == (3, 2)
    assert _code(lambda: c.corner_subpix(PTS, 2)) == -1


def test_subpix_read_states(loop_scene):
    from vo_mi355x import VoContext
    sc, state = loop_scene
    with VoContext(W, H, max_pts=1024) as c:
        assert _code(lambda: c.subpix_read(1)) == -4                      # nothing has refined
        rp = _loop(c, sc, state, subpix={})
        rp.step(T1 + 1)
        assert _code(lambda: c.subpix_read(1)) == -4                      # a step in flight
        assert rp.fetch()["status"] == 0
        assert len(c.subpix_read()["raw"]) > 0
        assert _code(lambda: c.subpix_read(4097)) == -1
        c.corner_subpix(PTS)                                              # the synchronous call takes the rows over
        assert _code(lambda: c.subpix_read(1)) == -4
        c.set_subpix(None)
        rp.step(T1 + 2); assert rp.fetch()["status"] == 0
        assert _code(lambda: c.subpix_read(1)) == -4                      # the last detection did not refine
