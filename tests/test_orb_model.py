"""CPU-only: the numpy definition of the multi-scale ORB detector (tests/orb_model.py) against restatements and exact truths.  Nothing here
touches the library; tests/test_gpu_orb.py holds the kernels to this model bit for bit."""
import numpy as np
import pytest

import brief_model as bm
import orb_model as om


# ---- resize ---------------------------------------------------------------------------------------------------------------------------------
def test_a_constant_image_stays_constant_at_every_level():
    for v in (0, 77, 255):
        for lvl in om.pyramid(np.full((97, 131), v, np.uint8), 1.2, 8):
            assert lvl.size and (lvl == v).all()


def test_scale_two_is_the_rounded_mean_of_2x2():
    im = bm.noise_image(132, 96, 3)
    lv = om.pyramid(im, 2.0, 3)
    for a, b in zip(lv[:-1], lv[1:]):
        I = a.astype(np.int64)
        want = (I[0::2, 0::2] + I[0::2, 1::2] + I[1::2, 0::2] + I[1::2, 1::2] + 2) >> 2
        assert np.array_equal(b, want.astype(np.uint8))


@pytest.mark.parametrize("sf", [1.2, 1.37, 2.0])
def test_transposing_the_image_transposes_every_level(sf):
    im = bm.noise_image(131, 97, 4)
    for a, b in zip(om.pyramid(im, sf, 8), om.pyramid(np.ascontiguousarray(im.T), sf, 8)):
        assert np.array_equal(a.T, b)


def test_geometry_and_quotas():
    wl, hl, sc = om.level_geometry(1241, 376, 1.2, 8)
    assert wl == [1241, 1034, 862, 718, 598, 499, 416, 346] and hl == [376, 313, 261, 218, 181, 151, 126, 105]
    assert sc.dtype == np.float32 and sc[0] == 1 and sc[3] == np.float32(1.2 ** 3)
    q = om.quotas(500, 1.2, 8)
    # by hand: nd = 500 (1 - 1/1.2) / (1 - 1.2^-8) = 108.59 -> 109, then 90.49, 75.41, 62.84, 52.37, 43.64, 36.37; the last level gets the rest
    assert q == [109, 90, 75, 63, 52, 44, 36, 31] and sum(q) == 500
    assert om.quotas(500, 1.2, 1) == [500]
    assert om.quotas(1, 2.0, 8) == [1, 0, 0, 0, 0, 0, 0, 0]                   # nd = 0.502 -> 1, 0.251 -> 0, ...; max(1 - 1, 0) for the last level
    wl, hl, _ = om.level_geometry(40, 30, 2.0, 8)                             # 30 / 64 rounds to 0: level 6 has no pixels, nor has level 7
    assert wl == [40, 20, 10, 5, 2, 1, 0, 0] and hl == [30, 15, 8, 4, 2, 1, 0, 0]


# ---- Harris ---------------------------------------------------------------------------------------------------------------------------------
def _harris_f64(img, x, y):
    """brute force, float64 throughout, pixel by pixel"""
    I = img.astype(np.float64)
    a = b = c = 0.0
    for v in range(-3, 4):
        for u in range(-3, 4):
            px, py = x + u, y + v
            ix = 2 * (I[py, px + 1] - I[py, px - 1]) + (I[py - 1, px + 1] - I[py - 1, px - 1]) + (I[py + 1, px + 1] - I[py + 1, px - 1])
            iy = 2 * (I[py + 1, px] - I[py - 1, px]) + (I[py + 1, px - 1] - I[py - 1, px - 1]) + (I[py + 1, px + 1] - I[py - 1, px + 1])
            a += ix * ix; b += iy * iy; c += ix * iy
    return ((a * b - c * c) - 0.04 * (a + b) * (a + b)) * (1.0 / (4 * 7 * 255)) ** 4


def test_harris_equals_a_float64_restatement():
    rs = np.random.RandomState(11)
    for im in (bm.noise_image(64, 48, 5), bm.blocks_image(64, 48, 6), om.smooth_noise(64, 48, 7)):
        for _ in range(40):
            x, y = int(rs.randint(4, 60)), int(rs.randint(4, 44))
            got, want = float(om.harris(im, x, y)), _harris_f64(im, x, y)
            assert abs(got - want) <= 1e-5 * abs(want), (x, y, got, want)       # (nine float32 roundings, 6e-8 each, and no point of these cancels 20-fold)


def test_harris_sign_on_corner_edge_flat():
    im = np.full((40, 40), 50, np.uint8)
    im[20:, 20:] = 200                                   # a block corner at (20, 20)
    assert om.harris(im, 20, 20) > 0
    edge = np.full((40, 40), 50, np.uint8)
    edge[:, 20:] = 200                                   # a straight vertical edge
    assert om.harris(edge, 20, 20) < 0
    assert om.harris(np.full((40, 40), 123, np.uint8), 20, 20) == 0


def test_harris_is_bit_equal_under_transposition():
    im = om.smooth_noise(64, 48, 8)
    imT = np.ascontiguousarray(im.T)
    for x, y in ((10, 9), (33, 20), (59, 43), (4, 4)):
        a, b = om.harris(im, x, y), om.harris(imT, y, x)
        assert a.tobytes() == b.tobytes()


# ---- retention ------------------------------------------------------------------------------------------------------------------------------
def _retain_best_sorted(values, n):
    """OpenCV's KeyPointsFilter::retainBest, by sorting: the n best and everything that ties with the n-th"""
    v = np.asarray(values)
    if n <= 0:
        return np.zeros(len(v), bool)
    if len(v) <= n:
        return np.ones(len(v), bool)
    nth = np.sort(v)[::-1][n - 1]
    return v >= nth


def test_retention_equals_sort_based_retain_best_with_ties():
    rs = np.random.RandomState(2)
    for trial in range(200):
        n = int(rs.randint(0, 40))
        v = rs.randint(0, 12, n).astype(np.float32) if trial % 2 else rs.randint(0, 255, n)
        for keep in (0, 1, 3, 10, 100):
            assert np.array_equal(om.retain(v, keep), _retain_best_sorted(v, keep)), (v, keep)


def test_twin_squares_return_the_tied_corners():
    for w, h in ((150, 110), (131, 97)):
        r = om.orb_np(om.twin_squares(w, h), nfeatures=1, nlevels=1)
        k = r["kps"]
        assert len(k) == 2 and k["response"][0] == k["response"][1] and k["ly"][0] == k["ly"][1] and k["lx"][1] - k["lx"][0] == 40


# ---- exact truths of the whole model ----------------------------------------------------------------------------------------------------------
def _as_set(k, fields=("octave", "lx", "ly")):
    return sorted(tuple(int(r[f]) for f in fields) + (r["response"].tobytes(),) for r in k)


@pytest.mark.parametrize("kind", ["noise", "texture"])
def test_transposing_the_image_transposes_the_keypoints(kind):
    im = om.make_image(kind, 150, 110)
    a = om.orb_np(im, nfeatures=40)
    b = om.orb_np(np.ascontiguousarray(im.T), nfeatures=40)
    assert len(a["kps"]) > 10
    assert _as_set(a["kps"]) == _as_set(b["kps"], ("octave", "ly", "lx"))


def test_one_level_is_fast_harris_and_brief_at_the_keypoints():
    im = om.make_image("texture", 150, 110)
    r = om.orb_np(im, nfeatures=25, nlevels=1)
    k = r["kps"]
    assert len(k) >= 25 and (k["octave"] == 0).all() and (k["size"] == 31).all()
    d, ang, fl = bm.brief_np(im, np.stack([k["lx"], k["ly"]], 1).astype(np.float32))
    assert not fl.any() and np.array_equal(d, r["desc"]) and np.array_equal(ang, k["angle"])
    assert np.array_equal(k["x"], k["lx"].astype(np.float32)) and np.array_equal(k["y"], k["ly"].astype(np.float32))
    assert (np.diff(k["response"]) <= 0).all()


def test_doubling_the_image_moves_the_keypoints_one_octave_up():
    I = om.make_image("texture", 100, 80)
    U = np.kron(I, np.ones((2, 2), np.uint8))
    big = 100000
    a = om.orb_np(I, nfeatures=big, nlevels=1)
    b = om.orb_np(U, nfeatures=big, scale_factor=2.0, nlevels=2)
    assert np.array_equal(b["levels"][1], I)
    k0, k1 = a["kps"], b["kps"][b["kps"]["octave"] == 1]
    d1 = b["desc"][b["kps"]["octave"] == 1]
    assert len(k0) > 10 and len(k0) == len(k1)
    for f in ("lx", "ly", "response", "angle"):
        assert k0[f].tobytes() == k1[f].tobytes(), f
    assert np.array_equal(k1["x"], 2 * k0["x"]) and np.array_equal(k1["y"], 2 * k0["y"]) and (k1["size"] == 62).all()
    assert np.array_equal(a["desc"], d1)


def test_integer_translation_displaces_the_keypoints_exactly():
    tex = om.smooth_noise(200, 150, 9)
    dx, dy = 13, 7
    A, B = tex[10:120, 10:160], tex[10 + dy:120 + dy, 10 + dx:160 + dx]
    a = om.orb_np(A, nfeatures=100000, nlevels=1)
    b = om.orb_np(B, nfeatures=100000, nlevels=1)
    ia, ib = om.common_after_translation(a["kps"], b["kps"], dx, dy, 150, 110, 150, 110)
    ja, jb = om.common_after_translation(b["kps"], a["kps"], -dx, -dy, 150, 110, 150, 110)
    assert len(ia) > 10 and len(ia) == len(ja)
    assert np.array_equal(a["desc"][ia], b["desc"][ib])                      # Hamming distance 0
    assert a["kps"]["response"][ia].tobytes() == b["kps"]["response"][ib].tobytes()
