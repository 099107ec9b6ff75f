"""CPU-only: the numpy definition of the oriented BRIEF descriptor and of the Hamming matcher (tests/brief_model.py) against truths that do
not go through it -- brute-force loops, a constant image, exact rotations by 90 degrees -- and the library's default sampling table against
its generator (tools/gen_brief_pattern.py)."""
import ctypes

import numpy as np
import pytest

import brief_model as bm


def test_default_pattern_is_the_generators_output():
    """vo_brief_default_pattern needs no context (and no GPU): the committed table = RandomState(31), N(0, 6^2) rounded, rejection"""
    from vo_mi355x import _lib
    out = np.zeros(1024, np.int8)
    assert _lib.load().vo_brief_default_pattern(out.ctypes.data_as(ctypes.POINTER(ctypes.c_int8))) == 0
    want = bm.default_pattern()
    assert want.shape == (256, 4) and want.dtype == np.int8
    assert np.array_equal(out.reshape(256, 4), want)
    assert np.abs(want).max() <= 15 and ((want[:, 0] != want[:, 2]) | (want[:, 1] != want[:, 3])).all()
    # the generator's definition, restated
    rs, rows = np.random.RandomState(31), []
    while len(rows) < 256:
        d = np.rint(rs.normal(0, 6, 4))
        if (np.abs(d) > 15).any() or (d[0] == d[2] and d[1] == d[3]):
            continue
        rows.append(d)
    assert np.array_equal(want, np.asarray(rows))


def test_default_params_and_struct_size():
    from vo_mi355x import _lib
    assert ctypes.sizeof(_lib.BriefParams) == 32
    p = _lib.BriefParams()
    p.n_bits = 7
    assert _lib.load().vo_brief_default_params(ctypes.byref(p)) == 0
    assert p.n_bits == 256 and p._pad == 0 and not any(p.reserved)


def test_blur_of_a_constant_image_is_the_image():
    for v in (0, 1, 77, 128, 254, 255):
        S = bm.blur(bm.flat_image(20, 15, v))
        assert S.shape == (9, 14) and (S == v).all(), v
    assert bm.G.sum() == 256 and np.array_equal(bm.G, bm.G[::-1])


def test_blur_equals_a_brute_force_loop():
    img = bm.noise_image(16, 13, 3)
    S = bm.blur(img)
    for y in range(3, 10):
        for x in range(3, 13):
            v = sum(int(bm.G[a]) * int(bm.G[b]) * int(img[y + a - 3, x + b - 3]) for a in range(7) for b in range(7))
            assert S[y - 3, x - 3] == (v + 32768) >> 16


def test_flat_patch_has_no_orientation():
    img = bm.flat_image(64, 52, 200)
    assert bm.moments(img, 30, 25) == (0, 0)
    c, s, a = bm.orientation(0, 0)
    assert (c, s, a) == (1.0, 0.0, 0.0)
    d, ang, fl = bm.brief_np(img, [[30, 25]])
    assert fl[0] == 0 and ang[0] == 0 and not d.any()          # every test compares equal values: no bit is set


def test_moments_equal_a_brute_force_loop_over_the_disc():
    img = bm.noise_image(64, 52, 11)
    assert bm.DISC.sum() == sum(2 * int(u) + 1 for u in bm.UMAX) * 2 - (2 * 15 + 1)
    for x, y in ((24, 24), (39, 27), (30, 25)):
        m10 = m01 = 0
        for v in range(-15, 16):
            for u in range(-int(bm.UMAX[abs(v)]), int(bm.UMAX[abs(v)]) + 1):
                m10 += u * int(img[y + v, x + u]); m01 += v * int(img[y + v, x + u])
        assert bm.moments(img, x, y) == (m10, m01)
        assert abs(m10) < 2 ** 31 and abs(m01) < 2 ** 31
    # the bound of the sums: every pixel 255 on one side
    assert 255 * int(np.abs(bm._U).sum()) < 2 ** 31


def test_orientation_of_a_ramp_is_its_gradient_direction():
    y, x = np.mgrid[0:60, 0:60]
    for gx, gy, want in ((1, 0, 0.0), (0, 1, 90.0), (1, 1, 45.0), (-1, 0, 180.0), (0, -1, 270.0), (1, -1, 315.0)):
        img = (120 + gx * (x - 30) + gy * (y - 30)).astype(np.uint8)
        c, s, a = bm.orientation(*bm.moments(img, 30, 30))
        assert abs(float(a) - want) < 1e-4, (gx, gy, a)
        assert abs(float(c) - np.cos(np.radians(want))) < 1e-6 and abs(float(s) - np.sin(np.radians(want))) < 1e-6


def test_steered_samples_stay_within_21_pixels():
    pat = np.array([[15, 15, -15, -15], [-15, 15, 15, -15]] * 128, np.int8)
    worst = 0
    for deg in np.arange(0, 360, 0.25):
        c, s = np.float32(np.cos(np.radians(deg))), np.float32(np.sin(np.radians(deg)))
        worst = max(worst, max(np.abs(v).max() for v in bm.steer(pat, c, s)))
    assert worst == 21


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("name", ["noise", "blocks"])
def test_rotating_the_image_by_90_degrees_keeps_every_bit(name, k):
    """numpy.rot90 maps the offset (u, v) to (v, -u): the moments rotate exactly, c and s swap and negate exactly, half-to-even is odd
    symmetric and the blur's taps are symmetric -- so the descriptor at the rotated corner is bit-equal, and the angle moves by -90 k"""
    w, h = 70, 61
    img = bm.noise_image(w, h, 5) if name == "noise" else bm.blocks_image(w, h, 6)
    rs = np.random.RandomState(9)
    pts = np.stack([rs.randint(bm.M, w - bm.M, 12), rs.randint(bm.M, h - bm.M, 12)], 1).astype(np.float32)
    d0, a0, f0 = bm.brief_np(img, pts)
    assert (f0 == 0).all() and d0.any() and all(bm.moments(img, int(x), int(y)) != (0, 0) for x, y in pts)
    rot, q, ww = img, pts.copy(), w
    for _ in range(k):                                            # (x, y) -> (y, w - 1 - x), the width taking its turn
        rot = np.rot90(rot)
        q = np.stack([q[:, 1], ww - 1 - q[:, 0]], 1)
        ww = rot.shape[1]
    d1, a1, f1 = bm.brief_np(np.ascontiguousarray(rot), q.astype(np.float32))
    assert (f1 == 0).all() and np.array_equal(d0, d1)
    diff = (a1.astype(np.float64) - a0.astype(np.float64) + 90.0 * k) % 360.0
    assert (np.minimum(diff, 360.0 - diff) < 1e-3).all(), diff


def test_margins_and_unusable_rows():
    w, h = 64, 52
    img = bm.noise_image(w, h, 2)
    pts = np.array([[24, 24], [23, 24], [24, 23], [w - 25, h - 25], [w - 24, h - 25], [w - 25, h - 24], [23.5, 24], [24.5, 24.4], [39.5, 27.5],
                    [np.nan, 30], [30, np.inf], [-np.inf, np.nan], [1e30, 30], [-5, 30]], np.float32)
    d, a, f = bm.brief_np(img, pts)
    assert f.tolist() == [0, 1, 1, 0, 1, 1, 0, 0, 1, 2, 2, 2, 1, 1]     # 23.5 -> 24, 24.5 -> 24, 39.5 -> 40 (half to even)
    assert not d[f != 0].any() and (a[f != 0] == 0).all() and d[f == 0].any(axis=1).all()
    assert np.array_equal(d[6], d[0]) and np.array_equal(d[7], d[0])
    # smaller than 49 on an axis: nothing is describable
    assert (bm.brief_np(bm.noise_image(101, 37, 1), [[50, 18], [24, 24]])[2] == 1).all()
    assert bm.brief_np(bm.noise_image(49, 49, 1), [[24, 24], [25, 24]])[2].tolist() == [0, 1]


def test_hamming_model_equals_a_double_loop_with_ties():
    rs = np.random.RandomState(4)
    for n1, n2, nb in ((5, 1, 4), (7, 2, 32), (9, 40, 8), (3, 70, 64)):
        d1 = rs.randint(0, 256, (n1, nb)).astype(np.uint8)
        d2 = rs.randint(0, 256, (n2, nb)).astype(np.uint8)
        if n2 > 4:
            d2[3] = d2[1]; d2[n2 - 1] = d2[1]                      # duplicated train rows: the lower index wins
            d1[0] = d2[1]                                          # a query in the train set: distance 0
        idx, dist = bm.hamming_knn2_np(d1, d2)
        for q in range(n1):
            cand = sorted((sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(d1[q], d2[j])), j) for j in range(n2))
            cand += [(bm.INT32_MAX, -1)] * 2
            assert [(int(dist[q, s]), int(idx[q, s])) for s in range(2)] == cand[:2], (n1, n2, nb, q)
        if n2 > 4:
            assert (idx[0] == [1, 3]).all() and (dist[0] == 0).all()
        if n2 == 1:
            assert (idx[:, 1] == -1).all() and (dist[:, 1] == bm.INT32_MAX).all()
