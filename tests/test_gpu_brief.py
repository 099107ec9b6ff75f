"""GPU: the oriented BRIEF descriptor (csrc/vo_brief.hip; vo_brief_compute / vo_set_brief / vo_get_brief / vo_brief_read) and the Hamming
matcher (vo_match_hamming_knn2) through every layer.

The contract is the numpy model tests/brief_model.py (shown against brute-force loops and exact rotations by tests/test_brief_model.py):
descriptors and flags of k_brief_describe equal it bit for bit, the angle -- float32 from two different atan2s, nothing depends on it --
within 1e-3 degrees; vo_match_hamming_knn2 equals the model exactly.  The resident detections -- the track table's and the closed loop's --
are pinned against the model at the integer corners they spawned, and everything else those detections write must be identical with the
setting on and off."""
import copy
import ctypes as C

import numpy as np
import pytest

import brief_model as bm
import pipe_helpers as ph

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 257)
SIZES = {"49x49": (49, 49, 49), "64x52": (64, 52, 64), "131x67_stride": (131, 67, 160), "101x37": (101, 37, 101)}


def _image(kind, w, h, seed=0):
    return {"noise": lambda: bm.noise_image(w, h, 40 + seed), "blocks": lambda: bm.blocks_image(w, h, 50 + seed),
            "ramp": lambda: bm.ramp_image(w, h), "flat": lambda: bm.flat_image(w, h)}[kind]()


def _custom_pattern():
    """a random table whose first rows hold all four (+-15, +-15) points"""
    rs = np.random.RandomState(8)
    p = rs.randint(-15, 16, (256, 4)).astype(np.int8)
    p[:4] = [[15, 15, -15, -15], [-15, 15, 15, -15], [15, -15, -15, 15], [-15, -15, 15, 15]]
    same = (p[:, 0] == p[:, 2]) & (p[:, 1] == p[:, 3])
    p[same, 2] = -p[same, 2] + (p[same, 2] == 0)
    assert not ((p[:, 0] == p[:, 2]) & (p[:, 1] == p[:, 3])).any()
    return p


def _corners(w, h, n=257):
    """rows on both sides of each of the four margins, NaN and inf rows, rows that round both ways (half to even), then random rows around
    the describable rectangle; a describable row (if the image has one) comes first"""
    M = bm.M
    xm, ym = min(max(w // 2, M), max(w - 1 - M, M)), min(max(h // 2, M), max(h - 1 - M, M))
    rows = [(xm, ym), (M - 1, ym), (M, ym), (w - 1 - M, ym), (w - M, ym), (xm, M - 1), (xm, M), (xm, h - 1 - M), (xm, h - M),
            (np.nan, ym), (xm, np.inf), (-np.inf, np.nan), (M - 0.5, ym), (M + 0.5, ym), (M + 1.5, ym + 0.5), (xm + 0.4, ym - 0.4),
            (xm - 0.4, ym + 0.6), (w - 1 - M + 0.5, ym), (w - 1 - M - 0.5, h - 1 - M + 0.4), (0, 0), (w - 1, h - 1), (-3, ym), (xm, 1e9), (3e38, -3e38)]
    rs = np.random.RandomState(w * 1000 + h)
    k = n - len(rows)
    rnd = np.stack([rs.uniform(M - 2.5, w - M + 1.5, k), rs.uniform(M - 2.5, h - M + 1.5, k)], 1)
    rnd[::3] = np.rint(rnd[::3])
    return np.concatenate([np.asarray(rows, np.float64), rnd]).astype(np.float32)


def _push(c, img, stride):
    """vo_frame_push with a row stride that need not be the width"""
    h, w = img.shape
    buf = np.full((h, stride), 255, np.uint8)
    buf[:, :w] = img
    c._ck(c._L.vo_frame_push(c._h, buf.ctypes.data_as(C.POINTER(C.c_uint8)), stride))


def _same(got, want, what=""):
    """(desc, angle, flags): desc and flags bit for bit, angle within 1e-3 degrees (on the circle)"""
    bad = np.nonzero((got[0] != want[0]).any(-1) | (got[2] != want[2]))[0]
    assert len(bad) == 0, (what, bad[:5], got[2][bad[:5]], want[2][bad[:5]], got[0][bad[:2]], want[0][bad[:2]])
    d = np.abs(got[1].astype(np.float64) - want[1].astype(np.float64))
    d = np.minimum(d, 360.0 - d)
    assert d.max(initial=0.0) <= 1e-3, (what, d.max())


# ---- 1. the synchronous call = the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "blocks", "ramp", "flat"])
@pytest.mark.parametrize("size", list(SIZES))
def test_brief_compute_is_the_model(size, kind):
    from vo_mi355x import VoContext
    w, h, stride = SIZES[size]
    img, other = _image(kind, w, h), _image("noise", w, h, seed=3)
    pts = _corners(w, h)
    pat = _custom_pattern()
    want = bm.brief_np(img, pts)
    want_pat = bm.brief_np(img, pts, pat)
    want_other = bm.brief_np(other, pts)
    n_ok = int((want[2] == 0).sum())
    print(size, kind, "flags 0/1/2:", np.bincount(want[2], minlength=3), "angles", want[1][want[2] == 0][:4])
    assert (want[2] == 2).sum() == 3
    if size == "101x37":
        assert n_ok == 0 and (want[2][want[2] != 2] == 1).all()
    elif size == "49x49":
        assert n_ok >= 1 and all(tuple(np.rint(p)) == (24, 24) for p in pts[want[2] == 0])
    else:
        assert n_ok > 50 and (want[2] == 1).sum() > 20
    if kind == "ramp" and n_ok:
        a = want[1][want[2] == 0]
        assert (np.abs(a - 45.0) < 1.0).all()                       # the steered (+-15, +-15) rows reach 21 pixels
    if kind == "flat" and n_ok:
        assert not want[0].any() and (want[1] == 0).all()
    with VoContext(w, h, max_pts=512, win=5, max_level=0) as c:
        _push(c, img, stride)
        for n in COUNTS:
            got = c.brief_compute(pts[:n], "cur")
            _same(got, tuple(a[:n] for a in want), "n = %d" % n)
        _same(c.brief_compute(pts, 1, pattern=pat), want_pat, "uploaded pattern")
        _same(c.brief_compute(pts[:65], "cur", params=c.brief_params(), pattern=pat), tuple(a[:65] for a in want_pat), "uploaded pattern, 65")
        _same(c.brief_compute(pts, "cur"), want, "the default pattern again")
        _push(c, other, stride)                                      # the store's halves swap
        _same(c.brief_compute(pts[:64], "prev"), tuple(a[:64] for a in want), "which = prev")
        _same(c.brief_compute(pts[:64], 0), tuple(a[:64] for a in want), "which = 0")
        _same(c.brief_compute(pts, "cur"), want_other, "which = cur")
        z = c.brief_compute(np.zeros((0, 2), np.float32))
        assert z[0].shape == (0, 32) and z[1].shape == (0,) and z[2].shape == (0,)
    if kind == "noise" and n_ok > 1:
        assert (want_pat[0] != want[0]).any() and (want_other[0] != want[0]).any()


def test_default_pattern_and_settings_round_trip():
    from vo_mi355x import VoContext
    pat = _custom_pattern()
    assert np.array_equal(VoContext.brief_default_pattern(), bm.default_pattern())
    with VoContext(64, 52, max_pts=16, win=5, max_level=0) as c:
        assert c.get_brief() is None and np.array_equal(c.brief_pattern_read(), bm.default_pattern())
        c.set_brief(True)
        assert c.get_brief().n_bits == 256 and np.array_equal(c.brief_pattern_read(), bm.default_pattern())
        c.set_brief(c.brief_params(), pat)
        assert np.array_equal(c.brief_pattern_read(), pat)
        c.set_brief(None)
        assert c.get_brief() is None and np.array_equal(c.brief_pattern_read(), bm.default_pattern())


# ---- 2. a batch ------------------------------------------------------------------------------------------------------------------------------
def test_batched_context_equals_single_contexts():
    from vo_mi355x import VoContext
    B, w, h = 3, 64, 52
    imgs = np.stack([_image(k, w, h, seed=b) for b, k in enumerate(("noise", "blocks", "noise"))])
    base = _corners(w, h, 65)
    pts = np.stack([base, base[::-1], np.roll(base, 7, axis=0)])
    with VoContext(w, h, max_pts=128, batch=B, win=5, max_level=0) as c:
        c.push_frame(imgs)
        desc, ang, fl = c.brief_compute(pts)
    with VoContext(w, h, max_pts=128, win=5, max_level=0) as one:
        for b in range(B):
            one.push_frame(imgs[b])
            single = one.brief_compute(pts[b])
            assert np.array_equal(desc[b], single[0]) and np.array_equal(fl[b], single[2]) and np.array_equal(ang[b], single[1]), b
            _same((desc[b], ang[b], fl[b]), bm.brief_np(imgs[b], pts[b]), "sequence %d against the model" % b)
    assert (desc[0] != desc[2]).any()


# ---- 3. the Hamming matcher --------------------------------------------------------------------------------------------------------------------
PAIRS = ((1, 1), (2, 63), (63, 2), (64, 64), (65, 257), (257, 65), (257, 257), (64, 1), (5, 4700))


@pytest.mark.parametrize("nbytes", [4, 32, 64])
def test_hamming_knn2_is_the_model(nbytes):
    """batch 2; duplicated train rows (the lower index first), n2 = 1 (an empty second slot), a query present in the train set (distance 0);
    (5, 4700) runs over more than one LDS tile of the train set at every descriptor length"""
    from vo_mi355x import VoContext
    rs = np.random.RandomState(nbytes)
    with VoContext(64, 52, max_pts=16, batch=2, win=5, max_level=0) as c:
        for n1, n2 in PAIRS:
            d1 = rs.randint(0, 256, (2, n1, nbytes)).astype(np.uint8)
            d2 = rs.randint(0, 256, (2, n2, nbytes)).astype(np.uint8)
            if n2 >= 63:
                d2[:, 40] = d2[:, 7]; d2[:, n2 - 1] = d2[:, 7]          # duplicates, also across the tile boundary
                d1[:, 0] = d2[:, 7]                                     # present in the train set: distance 0, indices 7 and 40
                d1[1, n1 - 1] = d2[1, n2 - 1]
            idx, dist = c.match_hamming_knn2(d1, d2)
            assert idx.shape == (2, n1, 2) and idx.dtype == np.int32 and dist.dtype == np.int32
            for b in range(2):
                wi, wd = bm.hamming_knn2_np(d1[b], d2[b])
                assert np.array_equal(idx[b], wi) and np.array_equal(dist[b], wd), (nbytes, n1, n2, b)
            if n2 >= 63:
                assert (idx[:, 0] == [7, 40]).all() and (dist[:, 0] == 0).all()
            if n2 == 1:
                assert (idx[..., 0] == 0).all() and (idx[..., 1] == -1).all() and (dist[..., 1] == bm.INT32_MAX).all()


# ---- 4. the track table ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("subpix", [False, True], ids=["integer", "subpix"])
@pytest.mark.parametrize("fast", [0, 20], ids=["shi-tomasi", "fast20"])
def test_track_table_describes_the_integer_corners(seq_small, fast, subpix):
    """two contexts on the same frames, one with set_brief: brief_read = the model at the integer corners of the detection (with refinement on
    as well: still the integer corners, vo_subpix_read's raw rows), and the tracks are those of the context that does not describe"""
    from vo_mi355x import VoContext, VoError, synthetic as syn
    frames = seq_small[0]
    w, h = 320, 240
    seeds = syn.grid_points(60, w, h, margin=10, seed=4)
    with VoContext(w, h, max_pts=512) as a, VoContext(w, h, max_pts=512) as b:
        a.set_brief(True)
        for c in (a, b):
            if subpix:
                c.set_subpix({})
            c.push_frame(frames[0]); c.tracks_seed(seeds, t=0)
            c.push_frame(frames[1]); c.tracks_track(1)
            c.tracks_detect(1, params=c.st_params(fast_threshold=fast), max_new=200)
        ra, rb = a.tracks_read(), b.tracks_read()
        for k in ra:
            assert np.array_equal(ra[k].view(np.uint32) if ra[k].dtype == np.float32 else ra[k],
                                  rb[k].view(np.uint32) if rb[k].dtype == np.float32 else rb[k]), k
        raw = a.subpix_read()["raw"] if subpix else a.shi_tomasi_fetch()
        assert len(raw) > 100 and np.array_equal(raw, np.rint(raw))
        if subpix:
            assert (ra["uv"][ra["t_first"] == 1] != np.rint(ra["uv"][ra["t_first"] == 1])).any()
        got = a.brief_read()
        assert len(got["desc"]) == len(raw)
        want = bm.brief_np(frames[1], raw)
        assert (want[2] == 0).sum() > 50
        _same((got["desc"], got["angle"], got["flags"]), want, "detected corners")
        part = a.brief_read(10)
        assert np.array_equal(part["desc"], got["desc"][:10])
        with pytest.raises(VoError) as ei:
            b.brief_read()                                                # this context's detection did not describe
        assert ei.value.code == -4
        a.push_frame(frames[2]); a.tracks_track(2)
        a.set_brief(None)
        a.tracks_detect(2, max_new=10)
        with pytest.raises(VoError) as ei:
            a.brief_read()                                                # switched off: a detection forgets the rows
        assert ei.value.code == -4


# ---- 5. the closed loop ----------------------------------------------------------------------------------------------------------------------
W, H, T1 = 256, 160, 3
N_STEPS = 3


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


def _run(sc, state, side, inflight, graph, descriptor):
    from vo_mi355x import VoContext
    with VoContext(W, H, max_pts=1024) as c:
        c.set_side_stream(side)
        c.set_graph_mode(graph)
        rp = _loop(c, sc, state, descriptor=descriptor)
        assert (c.get_brief() is not None) == (descriptor == "brief")
        recs, pending = [], 0
        for s in range(N_STEPS):
            rp.step(T1 + 1 + s); pending += 1
            if pending == inflight or s == N_STEPS - 1:
                while pending:
                    recs.append(rp.fetch()); pending -= 1
        return recs, rp.read_tables(), (rp.brief_read() if descriptor else None)


@pytest.fixture(scope="module")
def loop_plain(loop_scene):
    """the run without descriptors on the default layout, and the model's descriptors at the corners its last frame spawned"""
    sc, state = loop_scene
    recs, T, _ = _run(sc, state, True, 1, False, None)
    assert all(r["status"] == 0 for r in recs)
    n_c, n_new = int(T["counts"][0, 0]), recs[-1]["n_detected"]
    raw = T["k_uv"][0, T["cand"][0, n_c - n_new:n_c]]
    assert n_new > 10 and np.array_equal(raw, np.rint(raw))
    want = bm.brief_np(sc["frames"][T1 + N_STEPS], raw)
    assert (want[2] == 0).sum() > 5
    return recs, T, want


@pytest.mark.parametrize("side,inflight,graph", [(True, 1, False), (False, 1, False), (True, "max", False), (2, 1, False), (True, 1, True), (False, 1, True)],
                         ids=["side", "inline", "side-inflight", "pipelined", "side-graph", "inline-graph"])
def test_closed_loop_with_descriptors_changes_nothing_else(loop_scene, loop_plain, side, inflight, graph):
    """a few whole frames with brief on: every record and every table (index lists among them) bit-equal to the run with brief off, and
    brief_read after the last fetch = the model at the corners the last frame spawned -- on every stream layout, with graph mode on and off"""
    from vo_mi355x.resident import INFLIGHT
    sc, state = loop_scene
    recs0, T0, want = loop_plain
    recs, T, got = _run(sc, state, side, INFLIGHT if inflight == "max" else inflight, graph, "brief")
    for s, (x, y) in enumerate(zip(recs0, recs)):
        for k, v in x.items():
            assert (np.array_equal(y[k], v, equal_nan=True) if isinstance(v, np.ndarray) else y[k] == v), (s, k)
    for name in T0:
        assert np.array_equal(T0[name], T[name], equal_nan=T0[name].dtype.kind == "f"), name
    n_new = len(want[0])
    assert len(got["desc"]) >= n_new                                    # every detected corner is described, the first n_new were spawned
    _same(tuple(got[k][:n_new] for k in ("desc", "angle", "flags")), want, "the last frame's corners")


# ---- 6. the drop-in Extractor -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("detector", ["shi-tomasi", "fast"])
def test_dropin_extractor_describes_and_matches(seq_small, detector):
    from vo_mi355x.extractor import Extractor
    img, nxt = seq_small[0][1], seq_small[0][2]
    with pytest.raises(ValueError):
        Extractor(lazy=False, descriptor="orb")
    with pytest.raises(NotImplementedError):
        Extractor(lazy=False).extract(img, 3, [], detector=detector, mask_radius=7, describe=True)       # the default still raises
    plain = Extractor(lazy=False).extract(img, 3, [], detector=detector, mask_radius=7)
    raw = np.asarray([k.uv for k in plain], np.float32).reshape(-1, 2)
    want = bm.brief_np(img, raw)
    keep = want[2] == 0
    assert keep.sum() > 50 and (~keep).any()
    ext = Extractor(descriptor="brief")
    kps = ext.extract(img, 3, [], detector=detector, mask_radius=7, describe=True)
    assert len(kps) == keep.sum()
    for k, uv, d in zip(kps, raw[keep], want[0][keep]):
        assert (k.t_first, k.t_total, len(k.uv_history)) == (3, 1, 1)
        assert np.asarray(k.uv).shape == (2, 1) and np.array_equal(np.asarray(k.uv).reshape(2), uv)
        assert k.des.shape == (32, 1) and k.des.dtype == np.uint8 and np.array_equal(k.des.reshape(32), d)
    plain_des = ext.extract(img, 3, [], detector=detector, mask_radius=7)
    assert len(plain_des) == len(raw) and plain_des[0].des.shape == (1, 1)                                 # describe=False: as ever
    # a frame's keypoints against themselves: the identity at distance 0 (duplicated descriptors go to the lower index)
    m = ext.match_lists(kps, kps)
    des = np.stack([k.des.reshape(32) for k in kps])
    first = [int(np.nonzero((des == d).all(1))[0][0]) for d in des]
    assert [x.queryIdx for x in m] == list(range(len(kps))) and [x.trainIdx for x in m] == first and all(x.distance == 0 for x in m)
    assert sum(f == i for i, f in enumerate(first)) > 0.9 * len(kps)
    # against the next frame's keypoints: the model's nearest neighbours
    kps2 = ext.extract(nxt, 4, [], detector=detector, mask_radius=7, describe=True)
    des2 = np.stack([k.des.reshape(32) for k in kps2])
    m2 = ext.match(des, des2)
    wi, wd = bm.hamming_knn2_np(des, des2)
    assert [x.trainIdx for x in m2] == wi[:, 0].tolist() and [x.distance for x in m2] == wd[:, 0].tolist()


# ---- 7. argument and state errors ---------------------------------------------------------------------------------------------------------------
def _code(fn):
    from vo_mi355x import VoError
    with pytest.raises(VoError) as ei:
        fn()
    return ei.value.code


def test_refusals_leave_the_next_detection_unchanged(seq_small):
    from vo_mi355x import VoContext
    img = seq_small[0][0]
    pts = np.full((3, 2), 100, np.float32)
    far = bm.default_pattern(); far[17, 2] = 16
    far_neg = bm.default_pattern(); far_neg[255, 1] = -16
    degenerate = bm.default_pattern(); degenerate[200, 2:] = degenerate[200, :2]
    with VoContext(320, 240, max_pts=64) as c, VoContext(320, 240, max_pts=64) as ref:
        assert _code(lambda: c.brief_compute(pts, "cur")) == -4             # no frame pushed
        c.push_frame(img); ref.push_frame(img)
        assert _code(lambda: c.brief_compute(pts, "prev")) == -4            # no previous frame
        assert _code(lambda: c.brief_compute(pts, 2)) == -1
        for bad in (far, far_neg, degenerate):
            assert _code(lambda: c.brief_compute(pts, "cur", pattern=bad)) == -1
            assert _code(lambda: c.set_brief(True, bad)) == -1
            assert c.get_brief() is None
        assert _code(lambda: c.brief_compute(pts, "cur", params=c.brief_params(n_bits=128))) == -1
        assert _code(lambda: c.set_brief(c.brief_params(n_bits=512))) == -1
        assert _code(lambda: c.brief_compute(np.full((65, 2), 100, np.float32))) == -1          # n > max_pts
        assert c.brief_compute(np.full((64, 2), 100, np.float32))[0].shape == (64, 32)
        for nb in (1, 3, 6, 68, 128):
            assert _code(lambda: c.match_hamming_knn2(np.zeros((4, nb), np.uint8), np.zeros((5, nb), np.uint8))) == -1
        assert c.match_hamming_knn2(np.zeros((4, 8), np.uint8), np.zeros((5, 8), np.uint8))[0].tolist() == [[0, 1]] * 4
        # the next default detection is what a context that saw none of this detects
        assert np.array_equal(c.shi_tomasi(None), ref.shi_tomasi(None))
        assert _code(lambda: c.brief_read(1)) == -4                         # nothing has described


def test_brief_read_states(loop_scene):
    from vo_mi355x import VoContext
    sc, state = loop_scene
    with VoContext(W, H, max_pts=1024) as c:
        assert _code(lambda: c.brief_read(1)) == -4                       # nothing has described
        rp = _loop(c, sc, state, descriptor="brief")
        rp.step(T1 + 1)
        assert _code(lambda: c.brief_read(1)) == -4                       # a step in flight
        assert rp.fetch()["status"] == 0
        assert len(c.brief_read()["desc"]) > 0
        assert _code(lambda: c.brief_read(4097)) == -1
        c.brief_compute(np.full((3, 2), 60, np.float32))                  # the synchronous call takes the rows over
        assert _code(lambda: c.brief_read(1)) == -4
        c.set_brief(None)
        rp.step(T1 + 2); assert rp.fetch()["status"] == 0
        assert _code(lambda: c.brief_read(1)) == -4                       # the last detection did not describe


# ---- 8. the four per-point side stores at once --------------------------------------------------------------------------------------------------
def _all_four(sc, state, side, inflight):
    """the closed loop with the forward-backward check, the predicted start, cornerSubPix and BRIEF all on; afterwards, in the same context, each
    synchronous corner call takes over its own rows only"""
    from vo_mi355x import VoContext
    with VoContext(W, H, max_pts=1024) as c:
        c.set_side_stream(side)
        rp = _loop(c, sc, state, fb_max_error=1.0, klt_predict="constant_velocity", subpix={}, descriptor="brief")
        recs, pending = [], 0
        for s in range(N_STEPS):
            rp.step(T1 + 1 + s); pending += 1
            if pending == inflight or s == N_STEPS - 1:
                while pending:
                    recs.append(rp.fetch()); pending -= 1
        n = recs[-1]["n_tracked"]
        reads = dict(fb=c.fb_read(n), guess=(c.klt_guess_read(n),), subpix=tuple(c.subpix_read().values()), brief=tuple(c.brief_read().values()))
        tables = rp.read_tables()
        pts = np.full((3, 2), 60, np.float32)
        c.corner_subpix(pts)
        assert _code(lambda: c.subpix_read(1)) == -4
        assert len(c.brief_read()["desc"]) == len(reads["brief"][0]) and c.fb_read(n)[0].shape == (n,) and c.klt_guess_read(n).shape == (n, 2)
        c.brief_compute(pts)
        assert _code(lambda: c.brief_read(1)) == -4 and _code(lambda: c.subpix_read(1)) == -4
        assert c.fb_read(n)[0].shape == (n,) and c.klt_guess_read(n).shape == (n, 2)
        return recs, tables, reads


def test_closed_loop_with_all_four_side_stores_is_the_same_on_every_layout(loop_scene):
    """records, tables and the four side reads (fb_read, klt_guess_read, subpix_read, brief_read) bit-equal with the side stream on, off, and on
    with the maximum number of steps in flight"""
    from vo_mi355x.resident import INFLIGHT
    sc, state = loop_scene
    recs0, T0, reads0 = _all_four(sc, state, True, 1)
    assert all(r["status"] == 0 for r in recs0) and recs0[-1]["n_tracked"] > 10 and recs0[-1]["n_detected"] > 10
    assert all(len(a) > 0 for v in reads0.values() for a in v)
    for side, inflight in ((False, 1), (True, INFLIGHT)):
        recs, T, reads = _all_four(sc, state, side, inflight)
        for s, (x, y) in enumerate(zip(recs0, recs)):
            for k, v in x.items():
                assert (np.array_equal(y[k], v, equal_nan=True) if isinstance(v, np.ndarray) else y[k] == v), (side, inflight, s, k)
        for name in T0:
            assert np.array_equal(T0[name], T[name], equal_nan=T0[name].dtype.kind == "f"), (side, inflight, name)
        for name, want in reads0.items():
            assert len(reads[name]) == len(want)
            for a, b in zip(want, reads[name]):
                assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (side, inflight, name)
