"""GPU: the tracker and the corner detector at full contrast and at the parameters no other GPU test varies, bit for bit against the CPU oracle.

The inputs are those of tests/range_cases.py: images of 0 and 255 only, which carry the tracker's window sums to the top of the ranges argued
in csrc/vo_klt_lk.h (template sums up to 14.9 x 2^30, mismatch sums beyond 2^30 of both signs: the float64 branch of klt_combine for A and for
b, the 16-bit splits of wave_sum2_wide / wave_sum3_wide with every quad sum at its bound) and the corner detector's window sums to 0.4656 x 2^31
with prefixes that pass 2^32 (k_st_eig_fused); point sets with bilinear weights on exact .5 ties; minEigThreshold from 0 to +inf, NaN, negative
and one float either side of a point's own eigenvalue (klt_min_eig_numerator); the criteria at and beyond their clamps.
tests/test_range_cases.py shows on the CPU that the inputs reach those ranges, that the oracle is right there, and that a kernel wrong in any
of these ways would change an output.  No tolerance anywhere."""
import functools

import numpy as np
import pytest

import klt_seed_model as km
import range_cases as rc
from tracks_model import fb_np, oracle_fb

pytestmark = pytest.mark.gpu


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(got, want, what):
    """(p1, status, err, iters) bit for bit"""
    for k, (x, y) in enumerate(zip(got[:4], want[:4])):
        assert np.array_equal(_bits(x), _bits(y)), (what, ("p1", "status", "err", "iters")[k])


@functools.lru_cache(maxsize=None)
def _oracle(name, kind, size):
    import vo_oracle as o
    a, b = rc.pair(name, kind, *size)
    return o.klt(a, b, rc.points(*size), return_iters=True)


def _cases():
    return [(n, k) for n in rc.IMAGES for k in rc.PAIRS]


# ---- pyramid and derivatives -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", rc.KLT_SIZES + rc.ST_SIZES)
def test_pyramid_and_scharr_at_full_contrast(size):
    """|Scharr| = 4080 at every pixel of the stripes: its 4 x store fills int16 to 16320"""
    import vo_oracle as o
    from vo_mi355x import VoContext
    w, h = size
    with VoContext(w, h, max_pts=64) as c:
        for name in rc.IMAGES:
            img = rc.image(name, w, h)
            c.push_frame(img)
            pyr = o.build_pyramid(img)
            assert len(pyr) >= 2
            for l, ref in enumerate(pyr):
                got, der = c.pyramid_read(1, l)
                assert np.array_equal(got, ref), (name, l)
                assert np.array_equal(der, o.scharr(ref)), (name, l)
            if name in ("vstripes2", "mix"):
                assert np.abs(o.scharr(img)).max() == 4080


# ---- the tracker on every pair ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [4, 5, 6])
@pytest.mark.parametrize("size", rc.KLT_SIZES)
def test_tracker_every_pair_every_instantiation(size, waves):
    from vo_mi355x import VoContext
    w, h = size
    p0 = rc.points(w, h)
    with VoContext(w, h, max_pts=64) as c:
        c.set_tuning(klt_waves=waves)
        for name, kind in _cases():
            a, b = rc.pair(name, kind, w, h)
            c.push_frame(a); c.push_frame(b)
            _same(c.klt_track(p0, return_iters=True), _oracle(name, kind, size), (name, kind))


@pytest.mark.parametrize("size", rc.KLT_SIZES)
def test_tracker_forward_backward_and_seeded_forms(size):
    """klt_track_fb against the oracle's two passes; klt_track(init) two pixels off and the seeded forward-backward form against the numpy
    model of the seeded tracker (tests/klt_seed_model.py)"""
    import vo_oracle as o
    from vo_mi355x import VoContext
    w, h = size
    p0 = rc.points(w, h)
    g = (p0 + np.float32([2.0, -2.0])).astype(np.float32)
    with VoContext(w, h, max_pts=64) as c:
        c.set_fb_check(0.5)
        for name, kind in _cases():
            a, b = rc.pair(name, kind, w, h)
            c.push_frame(a); c.push_frame(b)
            f1, fst, ferr, p0r, fbe, fit = c.klt_track_fb(p0, return_iters=True)
            _same((f1, fst, ferr, fit), _oracle(name, kind, size), (name, kind, "fb forward"))
            r0 = oracle_fb(a, b, p0)[3]
            e, ok = fb_np(p0, r0, 0.5)
            assert np.array_equal(p0r, r0, equal_nan=True) and np.array_equal(fbe, e, equal_nan=True), (name, kind, "fb backward")
            got_ok, got_e = c.fb_read(len(p0))
            assert np.array_equal(got_ok, ok) and np.array_equal(got_e, e, equal_nan=True), (name, kind, "fb flags")
            if name in rc.SATURATED:
                want = km.klt_np(a, b, p0, init=g)
                _same(c.klt_track(p0, return_iters=True, init=g), want, (name, kind, "seeded"))
                s1, sst, serr, s0r, sfbe, sit = c.klt_track_fb(p0, return_iters=True, init=g)
                _same((s1, sst, serr, sit), want, (name, kind, "seeded fb forward"))
                r0 = o.klt(b, a, want[0])[0]                          # the backward pass is unseeded
                assert np.array_equal(s0r, r0, equal_nan=True), (name, kind, "seeded fb backward")
                assert np.array_equal(sfbe, fb_np(p0, r0, 0.5)[0], equal_nan=True), (name, kind, "seeded fb error")


@pytest.mark.parametrize("size", rc.KLT_SIZES)
def test_tracker_resident_path(size):
    from vo_mi355x import VoContext
    w, h = size
    p0 = rc.points(w, h)
    cases = _cases()
    frames = np.stack([f for name, kind in cases for f in rc.pair(name, kind, w, h)])
    with VoContext(w, h, max_pts=64) as c:
        c.upload_sequence(frames)
        for i, (name, kind) in enumerate(cases):
            c.points_upload(p0)
            c.push_frame_resident(2 * i); c.push_frame_resident(2 * i + 1)
            c.klt_track_resident(len(p0))
            _same(c.points_download(len(p0), return_iters=True), _oracle(name, kind, size), (name, kind))


@pytest.mark.parametrize("size", rc.KLT_SIZES)
def test_tracker_batch_of_three_different_images(size):
    """a different saturated image, pair and point set per sequence: a mix-up between sequences cannot hide"""
    import vo_oracle as o
    from vo_mi355x import VoContext
    w, h = size
    for rot in range(3):
        pick = [(rc.SATURATED[(b + rot) % 4], rc.PAIRS[(b + rot) % 3]) for b in range(3)]
        prs = [rc.pair(n, k, w, h) for n, k in pick]
        p0 = np.stack([rc.points(w, h, seed=b + 1) for b in range(3)])
        with VoContext(w, h, max_pts=64, batch=3) as c:
            c.push_frame(np.stack([p[0] for p in prs])); c.push_frame(np.stack([p[1] for p in prs]))
            got = c.klt_track(p0, return_iters=True)
            fb = c.klt_track_fb(p0, return_iters=True)
        for b in range(3):
            want = o.klt(prs[b][0], prs[b][1], p0[b], return_iters=True)
            _same([x[b] for x in got], want, (pick[b], "batch"))
            _same((fb[0][b], fb[1][b], fb[2][b], fb[5][b]), want, (pick[b], "batch fb"))
            assert np.array_equal(fb[3][b], o.klt(prs[b][1], prs[b][0], want[0])[0], equal_nan=True), (pick[b], "batch fb backward")


def test_tracker_two_keypoints_per_wave():
    from vo_mi355x import VoContext, VoError
    size = rc.KLT_SIZES[1]
    w, h = size
    p0 = rc.points(w, h)
    with VoContext(w, h, max_pts=64) as c:
        try:
            c.set_tuning(klt_pair=3)
        except VoError:
            pytest.skip("the library was built without -DVO_EXPERIMENTS (the default): k_klt_track2 is not in it")
        for name, kind in _cases():
            a, b = rc.pair(name, kind, w, h)
            c.push_frame(a); c.push_frame(b)
            for mode in (3, 4):
                c.set_tuning(klt_pair=mode)
                _same(c.klt_track(p0, return_iters=True), _oracle(name, kind, size), (name, kind, mode))


# ---- thresholds and criteria -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1], ids=["checker2", "edges_320x240"])
def test_min_eig_threshold_sweep(which):
    """minEig < threshold is decided on the device as num < min_eig_num, the numerator found by bisection on the host: every exit of that
    search, and the status flips between a point's own level-0 minEig and its float neighbour exactly where the oracle's does"""
    import vo_oracle as o
    from vo_mi355x import VoContext
    tag, a, b, p0 = rc.sweep_pairs()[which]
    h, w = a.shape
    own = rc.own_thresholds(a, b, p0)
    with VoContext(w, h, max_pts=256) as c:
        c.push_frame(a); c.push_frame(b)
        tracked = {}
        for thr in rc.THRESHOLDS + own:
            got = c.klt_track(p0, c.klt_params(min_eig_threshold=thr), return_iters=True)
            _same(got, o.klt(a, b, p0, minEigThreshold=thr, return_iters=True), (tag, thr))
            tracked[float(thr)] = int(got[1].sum())
    assert tracked[np.inf] == 0 and tracked[-1.0] > 0
    for k in range(0, len(own), 3):
        assert tracked[float(own[k])] == tracked[float(own[k + 1])] > tracked[float(own[k + 2])], (tag, own[k + 1])


@pytest.mark.parametrize("which", [0, 1], ids=["checker2", "edges_320x240"])
def test_criteria_at_and_beyond_their_clamps(which):
    import vo_oracle as o
    from vo_mi355x import VoContext
    tag, a, b, p0 = rc.sweep_pairs()[which]
    h, w = a.shape
    with VoContext(w, h, max_pts=256) as c:
        c.push_frame(a); c.push_frame(b)
        res = {}
        for mc, eps in rc.CRITERIA + [(1000, 0.0)]:
            got = c.klt_track(p0, c.klt_params(max_count=mc, epsilon=eps), return_iters=True)
            _same(got, o.klt(a, b, p0, criteria=(3, mc, eps), return_iters=True), (tag, mc, eps))
            res[(mc, eps)] = got
    assert res[(0, 0.03)][3].max() <= 0 and res[(-5, 0.03)][3].max() <= 0 and res[(0, 0.0)][3].max() <= 0
    _same(res[(1000, 0.0)], res[(100, 0.0)], (tag, "max_count clamps at 100"))
    _same(res[(30, -1.0)], res[(30, 0.0)], (tag, "epsilon clamps at 0"))
    _same(res[(30, 11.0)], res[(30, 10.0)], (tag, "epsilon clamps at 10"))


# ---- the corner detector ---------------------------------------------------------------------------------------------------------------------
ST_CONFIGS = {"fused": {}, "band8": dict(st_band_rows=8), "band17": dict(st_band_rows=17), "separate_nms": dict(st_separate_nms=1),
              "two_kernels": dict(st_two_kernels=1)}


@functools.lru_cache(maxsize=None)
def _st_oracle(name, size, block, harris, masked, seed=0):
    import vo_oracle as o
    w, h = size
    m = rc.disc_mask(w, h, seed=seed)[1] if masked else np.full((h, w), 255, np.uint8)
    return o.good_features(rc.image(name, w, h), m, maxCorners=300, qualityLevel=0.03, minDistance=7.0, blockSize=block, return_aux=True,
                           useHarrisDetector=harris, k=0.04) + (m,)


def _check_st(c, B, corners, names, size, block, harris, masked, what):
    from vo_mi355x import VoError
    resp, mask, nc = c.shi_tomasi_read()
    if B == 1:
        resp, mask, nc = resp[None], mask[None], [nc]
        corners = corners if isinstance(corners, VoError) else [corners]
    for b in range(B):
        ref, rresp, rnc, m = _st_oracle(names[b], size, block, harris, masked, b)
        assert np.array_equal(mask[b], m), what
        assert np.array_equal(_bits(resp[b]), _bits(rresp)), (what, names[b], "response map")
        assert int(nc[b]) == rnc, (what, names[b], "candidate count")
    if isinstance(corners, VoError):
        # plateaus: more candidates than the selection holds and the strongest 16384 do not fill max_corners (tests/test_gpu_fuzz.py)
        assert corners.code == -5 and max(_st_oracle(names[b], size, block, harris, masked, b)[2] for b in range(B)) > 16384, what
    else:
        for b in range(B):
            assert np.array_equal(np.asarray(corners[b]).reshape(-1, 2), _st_oracle(names[b], size, block, harris, masked, b)[0].reshape(-1, 2)), (what, names[b])


def _detect(c, pts, prm):
    from vo_mi355x import VoError
    try:
        return c.shi_tomasi(pts, 7, params=prm)
    except VoError as e:
        return e


@pytest.mark.parametrize("config", list(ST_CONFIGS))
@pytest.mark.parametrize("size", rc.ST_SIZES)
def test_corner_detector_at_full_contrast(size, config):
    from vo_mi355x import VoContext
    w, h = size
    pts = rc.disc_mask(w, h)[0]
    with VoContext(w, h, max_pts=64) as c:
        c.set_tuning(**ST_CONFIGS[config])
        for name in rc.SATURATED + ("flat255",):
            c.push_frame(rc.image(name, w, h))
            for block in (31, 15, 3):
                for harris in (False, True):
                    prm = c.st_params(max_corners=300, quality_level=0.03, min_distance=7.0, block_size=block, use_harris=harris, harris_k=0.04)
                    for masked in (False, True):
                        corners = _detect(c, pts if masked else None, prm)
                        _check_st(c, 1, corners, [name], size, block, harris, masked, (config, name, block, harris, masked))


@pytest.mark.parametrize("size", rc.ST_SIZES)
def test_corner_detector_batch_of_three_different_images(size):
    from vo_mi355x import VoContext
    w, h = size
    for names in (("mix", "checker2", "vstripes2"), ("diag", "mix", "checker2")):
        pts = np.stack([rc.disc_mask(w, h, seed=b)[0] for b in range(3)])
        with VoContext(w, h, max_pts=64, batch=3) as c:
            c.push_frame(np.stack([rc.image(n, w, h) for n in names]))
            for block in (31, 15, 3):
                for harris in (False, True):
                    prm = c.st_params(max_corners=300, quality_level=0.03, min_distance=7.0, block_size=block, use_harris=harris, harris_k=0.04)
                    for masked in (False, True):
                        corners = _detect(c, pts if masked else None, prm)
                        _check_st(c, 3, corners, names, size, block, harris, masked, (names, block, harris, masked))
