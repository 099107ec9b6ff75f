"""The ORB kernels (csrc/vo_orb.hip) against the numpy definition (tests/orb_model.py), bit for bit: n_out, every field of every vo_orb_kp, every
descriptor, the level table and every level image.  The one exception is `angle`, within 1e-3 degrees on the circle (the device's atan2 is not
numpy's to the last bit; the angle is reported only -- the BRIEF test's rule).  Images are small on purpose: at scale 1.2 the 150 x 110 and
131 x 97 frames leave levels 0-3 (0-2 of the smaller frame) populated and the levels above smaller than 63 pixels, which is the empty-level
path."""
import ctypes as C

import numpy as np
import pytest

import orb_model as om

pytestmark = pytest.mark.gpu

SHAPES = ((150, 110, 150), (131, 97, 160))          # width, height, stride
FIELDS = ("x", "y", "size", "response", "octave", "lx", "ly")


@pytest.fixture(scope="module")
def contexts():
    from vo_mi355x import VoContext
    made = {}

    def get(w, h, batch=1):
        if (w, h, batch) not in made:
            made[(w, h, batch)] = VoContext(w, h, max_pts=256, batch=batch)
        return made[(w, h, batch)]
    yield get
    for c in made.values():
        c.close()


def raw_call(ctx, imgs, stride, masks=None, pattern=None, max_out=512, prm=None, **params):
    """vo_orb_detect_compute through ctypes with a row stride of the caller's choice -> (rc, kps [B][max_out], desc, n_out)"""
    from vo_mi355x import _lib
    B, h, w = ctx.batch, ctx.height, ctx.width
    buf = np.full((B, h, stride), 7, np.uint8)
    buf[:, :, :w] = np.asarray(imgs, np.uint8).reshape(B, h, w)
    mbuf = None
    if masks is not None:
        mbuf = np.full((B, h, stride), 255, np.uint8)
        mbuf[:, :, :w] = np.asarray(masks, np.uint8).reshape(B, h, w)
    if prm is None:
        prm = ctx.orb_params(**params)
    pat = None if pattern is None else np.ascontiguousarray(pattern, np.int8)
    kps = np.full((B, max_out), 0, _lib.ORB_KP_DTYPE)
    kps["octave"] = -77
    desc = np.full((B, max_out, 32), 0xA5, np.uint8)
    n_out = np.full(B, -77, np.int32)
    rc = ctx._L.vo_orb_detect_compute(ctx._h, _lib.ptr(buf, C.c_uint8), stride, _lib.ptr(mbuf, C.c_uint8), C.byref(prm), _lib.ptr(pat, C.c_int8),
                                      max_out, kps.ctypes.data_as(C.POINTER(_lib.OrbKp)), _lib.ptr(desc, C.c_uint8), _lib.ptr(n_out, C.c_int32))
    return rc, kps, desc, n_out


def same_keypoints(k, d, ref):
    assert len(k) == len(ref["kps"]), (len(k), len(ref["kps"]), ref["n_l"])
    for f in FIELDS:
        assert k[f].tobytes() == ref["kps"][f].tobytes(), f
    da = np.abs(k["angle"].astype(np.float64) - ref["kps"]["angle"].astype(np.float64))
    assert (np.minimum(da, 360.0 - da) <= 1e-3).all()
    assert np.array_equal(d, ref["desc"])


def same_levels(ctx, refs):
    lv = ctx.orb_levels()
    n = len(refs[0]["w_l"])
    assert lv["nlevels"] == n
    pad = lambda a: list(a) + [0] * (8 - n)
    assert list(lv["w_l"]) == pad(refs[0]["w_l"]) and list(lv["h_l"]) == pad(refs[0]["h_l"]) and list(lv["quota_l"]) == pad(refs[0]["quota_l"])
    assert lv["scale_l"][:n].tobytes() == refs[0]["scale_l"].tobytes() and not lv["scale_l"][n:].any()
    for b, ref in enumerate(refs):
        assert list(lv["n_l"][b]) == pad(ref["n_l"])
        for l in range(n):
            assert np.array_equal(lv["images"][b][l], ref["levels"][l]), (b, l)


def run_and_compare(ctx, imgs, stride, masks=None, pattern=None, max_out=512, **params):
    rc, kps, desc, n_out = raw_call(ctx, imgs, stride, masks, pattern, max_out, **params)
    assert rc == 0, ctx._L.vo_last_error(ctx._h)
    B = ctx.batch
    imgs = np.asarray(imgs).reshape(B, ctx.height, ctx.width)
    refs = [om.orb_np(imgs[b], None if masks is None else np.asarray(masks).reshape(imgs.shape)[b], pattern=pattern, **params) for b in range(B)]
    for b in range(B):
        assert n_out[b] == len(refs[b]["kps"]), (b, n_out[b], refs[b]["n_l"])
        same_keypoints(kps[b, :n_out[b]], desc[b, :n_out[b]], refs[b])
        assert (kps[b, n_out[b]:]["octave"] == -77).all() and (desc[b, n_out[b]:] == 0xA5).all()      # nothing written past n_out
    same_levels(ctx, refs)
    return refs


# ---- bit for bit ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["noise", "blocks", "flat", "twin"])
@pytest.mark.parametrize("shape", SHAPES)
def test_the_kinds_of_image_at_the_defaults_and_a_binding_quota(contexts, shape, kind):
    w, h, stride = shape
    refs = run_and_compare(contexts(w, h), om.make_image(kind, w, h), stride, nfeatures=30)
    n = refs[0]["n_l"]
    assert len(n) == 8 and not any(n[4:])                                   # levels 4-7 are too small for a keypoint
    if kind == "flat":
        assert sum(n) == 0
    if kind in ("noise", "twin"):
        assert sum(n) > 0


CASES = {
    "one_level": dict(nlevels=1, nfeatures=30),
    "scale_two": dict(scale_factor=2.0, nfeatures=30),
    "one_level_scale_two": dict(nlevels=1, scale_factor=2.0, nfeatures=100000),
    "no_quota_binds": dict(nfeatures=100000),
    "no_quota_binds_scale_two": dict(nfeatures=100000, scale_factor=2.0),
    "threshold_60": dict(fast_threshold=60, nfeatures=30),
    "threshold_60_no_quota": dict(fast_threshold=60, nfeatures=100000),
    "the_defaults": dict(),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("shape", SHAPES)
def test_parameter_cases(contexts, shape, case):
    w, h, stride = shape
    refs = run_and_compare(contexts(w, h), om.make_image("texture", w, h), stride, max_out=2048, **CASES[case])
    assert sum(refs[0]["n_l"]) > 0
    if CASES[case].get("nfeatures") == 30 and CASES[case].get("nlevels", 8) == 8 and "scale_factor" not in CASES[case]:
        assert refs[0]["n_l"][0] >= refs[0]["quota_l"][0]                   # the quota binds on level 0


def test_ties_make_a_level_return_more_than_its_quota(contexts):
    for w, h, stride in SHAPES:
        refs = run_and_compare(contexts(w, h), om.twin_squares(w, h), stride, nfeatures=1, nlevels=1)
        assert refs[0]["quota_l"] == [1] and refs[0]["n_l"] == [2]


def test_a_wide_image_spans_several_tile_columns():
    """600 x 72: three tile columns of 256 on level 0 and on level 1 (scale 1.1: 545 x 65), whose eligible band is three rows high"""
    from vo_mi355x import VoContext
    w, h = 600, 72
    with VoContext(w, h, max_pts=256) as c:
        refs = run_and_compare(c, om.make_image("texture", w, h), 608, max_out=4096, nfeatures=100000, scale_factor=1.1, nlevels=3)
        k = refs[0]["kps"]
        assert refs[0]["n_l"][0] > 0 and refs[0]["n_l"][1] > 0 and refs[0]["n_l"][2] == 0
        assert (k["lx"] < 256).any() and ((k["lx"] >= 256) & (k["lx"] < 512)).any() and (k["lx"] >= 512).any()
        refs = run_and_compare(c, om.make_image("noise", w, h), 608, max_out=4096, nfeatures=60, scale_factor=1.1, nlevels=3)
        assert refs[0]["n_l"][0] >= refs[0]["quota_l"][0]


def _random_pattern(seed):
    rs = np.random.RandomState(seed)
    p = rs.randint(-15, 16, (256, 4)).astype(np.int8)
    same = (p[:, 0] == p[:, 2]) & (p[:, 1] == p[:, 3])
    p[same, 2] = np.where(p[same, 0] > 0, p[same, 0] - 1, p[same, 0] + 1)
    return p


def test_a_custom_pattern(contexts):
    w, h, stride = SHAPES[1]
    im = om.make_image("texture", w, h)
    pat = _random_pattern(12)
    refs = run_and_compare(contexts(w, h), im, stride, pattern=pat, nfeatures=30)
    assert not np.array_equal(refs[0]["desc"], om.orb_np(im, nfeatures=30)["desc"])


@pytest.mark.parametrize("shape", SHAPES)
def test_masks(contexts, shape):
    w, h, stride = shape
    im = om.make_image("texture", w, h)
    half = np.full((h, w), 255, np.uint8)
    half[:, :w // 2] = 0
    refs = run_and_compare(contexts(w, h), im, stride, masks=half, nfeatures=100000)
    k = refs[0]["kps"]
    assert len(k) > 0 and (np.rint(k["x"]) >= w // 2).all() and (k["octave"] > 0).any()
    refs = run_and_compare(contexts(w, h), im, stride, masks=np.zeros((h, w), np.uint8), nfeatures=100000)
    assert sum(refs[0]["n_l"]) == 0


@pytest.mark.parametrize("shape", SHAPES)
def test_a_batch_of_three_different_images_one_of_them_flat(contexts, shape):
    w, h, stride = shape
    imgs = np.stack([om.make_image("texture", w, h), om.make_image("flat", w, h), om.make_image("noise", w, h)])
    refs = run_and_compare(contexts(w, h, 3), imgs, stride, nfeatures=30)
    assert sum(refs[0]["n_l"]) > 0 and sum(refs[1]["n_l"]) == 0 and sum(refs[2]["n_l"]) > 0
    mask = np.full((3, h, w), 255, np.uint8)
    mask[0, :, w // 2:] = 0
    mask[2] = 0
    refs = run_and_compare(contexts(w, h, 3), imgs, stride, masks=mask, nfeatures=100000, max_out=2048)
    assert sum(refs[0]["n_l"]) > 0 and sum(refs[2]["n_l"]) == 0


def test_two_calls_in_a_row_with_different_parameters(contexts):
    w, h, stride = SHAPES[0]
    from vo_mi355x import VoContext
    with VoContext(w, h, max_pts=256) as c:                                   # a context of its own: the first call reserves, the second regrows
        im = om.make_image("texture", w, h)
        run_and_compare(c, im, stride, nfeatures=30, scale_factor=2.0, nlevels=3)
        run_and_compare(c, om.make_image("noise", w, h), stride, nfeatures=100000, scale_factor=1.1, nlevels=8, fast_threshold=35, max_out=4096)
        run_and_compare(c, im, stride, nfeatures=30, scale_factor=2.0, nlevels=3)


# ---- truths on the device -----------------------------------------------------------------------------------------------------------------------
def test_doubling_the_image_moves_the_keypoints_one_octave_up(contexts):
    I = om.make_image("texture", 100, 80)
    U = np.kron(I, np.ones((2, 2), np.uint8))
    k0, d0 = contexts(100, 80).orb_detect_compute(I, nfeatures=100000, nlevels=1)
    ku, du = contexts(200, 160).orb_detect_compute(U, nfeatures=100000, scale_factor=2.0, nlevels=2)
    up = ku["octave"] == 1
    k1, d1 = ku[up], du[up]
    assert len(k0) > 10 and len(k0) == len(k1)
    for f in ("lx", "ly", "response", "angle"):
        assert k0[f].tobytes() == k1[f].tobytes(), f
    assert np.array_equal(k1["x"], 2 * k0["x"]) and np.array_equal(k1["y"], 2 * k0["y"]) and (k1["size"] == 62).all()
    assert np.array_equal(d0, d1)
    assert np.array_equal(contexts(200, 160).orb_levels()["images"][0][1], I)


@pytest.fixture(scope="module")
def crops():
    tex = om.smooth_noise(200, 150, 9)
    dx, dy = 13, 7
    return np.ascontiguousarray(tex[10:120, 10:160]), np.ascontiguousarray(tex[10 + dy:120 + dy, 10 + dx:160 + dx]), dx, dy


def test_integer_translation_displaces_the_keypoints_exactly(contexts, crops):
    A, B, dx, dy = crops
    c = contexts(150, 110)
    ka, da = c.orb_detect_compute(A, nfeatures=100000, nlevels=1)
    kb, db = c.orb_detect_compute(B, nfeatures=100000, nlevels=1)
    ia, ib = om.common_after_translation(ka, kb, dx, dy, 150, 110, 150, 110)
    ja, _ = om.common_after_translation(kb, ka, -dx, -dy, 150, 110, 150, 110)
    assert len(ia) > 10 and len(ia) == len(ja)
    assert np.array_equal(da[ia], db[ib])
    assert ka["response"][ia].tobytes() == kb["response"][ib].tobytes() and ka["angle"][ia].tobytes() == kb["angle"][ib].tobytes()
    # through the matcher: every common keypoint's nearest neighbour is at distance 0, and it is its displaced self (or a twin descriptor)
    idx, dist = c.match_hamming_knn2(da, db)
    assert (dist[ia, 0] == 0).all()
    assert np.array_equal(db[idx[ia, 0]], db[ib])


# ---- errors -----------------------------------------------------------------------------------------------------------------------------------
def test_max_out_too_small_is_a_capacity_error_and_leaves_the_outputs_alone(contexts):
    w, h, stride = SHAPES[0]
    c = contexts(w, h)
    im = om.make_image("texture", w, h)
    n = len(om.orb_np(im, nfeatures=30)["kps"])
    assert n > 4
    for max_out in (1, n - 1):
        rc, kps, desc, n_out = raw_call(c, im, stride, max_out=max_out, nfeatures=30)
        assert rc == -5, rc                                                  # VO_E_CAPACITY
        assert (kps["octave"] == -77).all() and (desc == 0xA5).all() and (n_out == -77).all()
    run_and_compare(c, im, stride, max_out=n, nfeatures=30)                   # exactly enough room


def test_more_rows_than_the_intermediate_capacity_is_an_error_not_a_truncation():
    """640 x 400 of noise: 19 388 strict maxima on level 0.  With a quota that keeps them all the rows behind the FAST cut exceed the 8 192 the
    library holds per (sequence, level): VO_E_CAPACITY, nothing written; with a quota that cuts, the same image equals the model"""
    from vo_mi355x import VoContext
    w, h = 640, 400
    im = om.make_image("noise", w, h)
    with VoContext(w, h, max_pts=256) as c:
        rc, kps, desc, n_out = raw_call(c, im, w, max_out=32768, nfeatures=100000, nlevels=1)
        assert rc == -5, rc
        assert (kps["octave"] == -77).all() and (desc == 0xA5).all() and (n_out == -77).all()
        refs = run_and_compare(c, im, w, max_out=1024, nfeatures=200, nlevels=2)
        assert refs[0]["n_l"][0] >= 109 and refs[0]["n_l"][1] >= 91


def test_invalid_parameters_and_a_bad_pattern(contexts):
    w, h, stride = SHAPES[0]
    c = contexts(w, h)
    im = om.make_image("texture", w, h)
    bad = [dict(nfeatures=0), dict(nfeatures=-3), dict(scale_factor=1.0), dict(scale_factor=2.0001), dict(scale_factor=float("nan")), dict(nlevels=0),
           dict(nlevels=9), dict(fast_threshold=0), dict(fast_threshold=255)]
    for kw in bad:
        rc, kps, desc, n_out = raw_call(c, im, stride, **kw)
        assert rc == -1, kw                                                  # VO_E_INVALID
        assert (kps["octave"] == -77).all() and (n_out == -77).all()
    for field, value in (("edge_threshold", 19), ("harris_k", 0.06)):
        prm = c.orb_params()
        setattr(prm, field, value)
        assert raw_call(c, im, stride, prm=prm)[0] == -1, field
    assert raw_call(c, im, stride, max_out=0)[0] == -1
    pat = _random_pattern(3)
    pat[17, 2] = 16
    assert raw_call(c, im, stride, pattern=pat)[0] == -1
    pat = _random_pattern(3)
    pat[200] = (4, -2, 4, -2)
    assert raw_call(c, im, stride, pattern=pat)[0] == -1
    from vo_mi355x import VoError
    with pytest.raises(VoError) as e:
        c.orb_detect_compute(im, nlevels=9)
    assert e.value.code == -1
    run_and_compare(c, im, stride, nfeatures=30)                             # the context still works


# ---- Extractor --------------------------------------------------------------------------------------------------------------------------------
def test_extractor_orb_matches_two_translated_crops(crops):
    from vo_mi355x import Extractor
    A, B, dx, dy = crops
    ex = Extractor(feature_method='orb', orb_params=dict(nfeatures=100000, nlevels=1), lazy=False)
    ka = ex.extract(A, 0, detector='custom', describe=True)
    kb = ex.extract(B, 1, detector='custom', describe=True)
    assert len(ka) > 10 and ka[0].des.shape == (32, 1) and ka[0].des.dtype == np.uint8 and ka[0].uv.shape == (2, 1)
    ref = om.orb_np(A, nfeatures=100000, nlevels=1)
    assert np.array_equal(np.asarray([k.uv.ravel() for k in ka]), np.stack([ref["kps"]["x"], ref["kps"]["y"]], 1))
    assert np.array_equal(np.asarray([k.des.ravel() for k in ka]), ref["desc"])
    ms = ex.match_lists(ka, kb)                                               # the 'orb' branch: one DMatch per query, nearest under Hamming
    assert len(ms) == len(ka) and [m.queryIdx for m in ms] == list(range(len(ka)))
    moved = 0
    for m in ms:
        a, b = ka[m.queryIdx], kb[m.trainIdx]
        x, y = a.uv.ravel() - (dx, dy)
        if om.EDGE <= x < 150 - om.EDGE and om.EDGE <= y < 110 - om.EDGE:   # a keypoint of both crops: its match is its displaced self
            assert m.distance == 0 and np.array_equal(a.des, b.des)
            moved += bool(np.array_equal(b.uv.ravel(), (x, y)))
    assert moved > 10
    plain = ex.extract(A, 0, detector='custom')
    assert len(plain) == len(ka) and plain[0].des.shape == (1, 1)
    with pytest.raises(NotImplementedError):
        ex.extract(A, 0, current_kp=ka[:3], detector='custom')
    ex._ctx.close()


def test_extractor_feature_method_argument():
    from vo_mi355x import Extractor
    assert Extractor(lazy=False)._feature_method == 'sift' and Extractor(feature_method='sift', lazy=False)._feature_method == 'sift'
    assert Extractor(feature_method='orb', lazy=False)._feature_method == 'orb'
    for bad in ('surf', None, 'ORB'):
        with pytest.raises(ValueError):
            Extractor(feature_method=bad)
    with pytest.raises(ValueError):
        Extractor(feature_method='orb', orb_params=dict(levels=3))
