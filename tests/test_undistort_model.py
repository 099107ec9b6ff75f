"""CPU-only: the numpy model of the lens undistortion (tests/undistort_model.py) is what it says it is.

The GPU tests (test_gpu_undistort.py) pin the HIP path to the model bit for bit; these pin the model: identity, the quantised table against an
independent plain-Python evaluation of the stated formulas, an accuracy anchor against an analytic ground truth and the zero rim of a barrel
lens."""
import math

import numpy as np
import pytest

import undistort_model as um

K = (260.0, 255.0, 158.3, 61.7)
W, H = 321, 123
# (name, dist, new_K)
SETS = [("barrel", (-0.3, 0.0, 0.0, 0.0), None),
        ("pincushion", (0.12, 0.05, 0.0, 0.0, 0.02), None),
        ("tangential", (0.0, 0.0, 0.004, -0.003), None),
        ("rational", (-0.25, 0.08, 0.001, -0.0005, 0.01, 0.05, 0.02, 0.003), None),
        ("zoom_out_shift", (-0.3, 0.1, 0.0, 0.0), (130.0, 128.0, 100.0, 90.0)),
        ("zero", (), None)]


def _images(w=W, h=H):
    rng = np.random.default_rng(11)
    return [rng.integers(0, 256, (h, w)).astype(np.uint8),
            np.tile((np.arange(w) * 255 // (w - 1)).astype(np.uint8), (h, 1)),
            np.full((h, w), 137, np.uint8)]


def test_zero_coefficients_are_the_identity():
    for dist in ((), (0, 0, 0, 0), (0,) * 5, (0,) * 8):
        for img in _images():
            assert np.array_equal(um.undistort(img, K, dist), img)
            assert np.array_equal(um.undistort(img, K, dist, K), img)
    t = um.table(W, H, K, ())
    jj, ii = np.meshgrid(np.arange(W), np.arange(H))
    assert np.array_equal(t["sxy"][..., 0], jj) and np.array_equal(t["sxy"][..., 1], ii) and not t["frac"].any() and not t["outside"].any()


def _py_entry(j, i, w, h, K4, d, N4):
    """the formulas of the model's docstring on plain Python floats"""
    fx, fy, cx, cy = (float(v) for v in K4)
    nfx, nfy, ncx, ncy = (float(v) for v in N4)
    k1, k2, p1, p2, k3, k4, k5, k6 = (float(v) for v in d)
    x = (float(j) - ncx) / nfx
    y = (float(i) - ncy) / nfy
    x2 = x * x
    y2 = y * y
    r2 = x2 + y2
    _2xy = 2.0 * x * y
    kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
    u = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2.0 * x2)) + cx
    v = fy * (y * kr + p1 * (r2 + 2.0 * y2) + p2 * _2xy) + cy
    res, outside = [], False
    for val, length in ((u, w), (v, h)):
        t = val * 32.0
        if not math.isfinite(t):
            res += [-2, 0]; outside = True
            continue
        q = int(max(-2.0 ** 30, min(2.0 ** 30, round(t))))          # Python's round: half to even
        s, f = q >> 5, q & 31
        outside |= s < -2 or s > length
        res += [max(-2, min(length, s)), f]
    return res[0], res[2], res[3] * 32 + res[1], int(outside)


@pytest.mark.parametrize("name,dist,new_K", SETS, ids=[s[0] for s in SETS])
def test_table_equals_an_independent_evaluation(name, dist, new_K):
    for w, h in ((203, 97), (W, H)):
        t = um.table(w, h, K, dist, new_K)
        d = list(dist) + [0.0] * (8 - len(dist))
        pix = [(j, i) for i in range(0, h, 7) for j in range(0, w, 11)] + [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1)]
        for j, i in pix:
            sx, sy, fr, out = _py_entry(j, i, w, h, K, d, K if new_K is None else new_K)
            assert (int(t["sxy"][i, j, 0]), int(t["sxy"][i, j, 1]), int(t["frac"][i, j]), int(t["outside"][i, j])) == (sx, sy, fr, out), (j, i)


def test_a_map_that_is_not_finite_is_outside():
    # the rational denominator crosses zero inside the image: 1 + k4 r2 = 0 on a circle; pixels near it overflow, none may raise or wrap
    t = um.table(64, 48, (50.0, 50.0, 32.0, 24.0), (0.0, 0.0, 0.0, 0.0, 0.0, -25.0, 0.0, 0.0))
    u, v = um.map_uv(64, 48, (50.0, 50.0, 32.0, 24.0), (0.0, 0.0, 0.0, 0.0, 0.0, -25.0, 0.0, 0.0))
    bad = ~np.isfinite(u * 32.0) | ~np.isfinite(v * 32.0)
    assert np.all(t["outside"][bad] == 1)
    assert t["sxy"].min() >= -2 and t["sxy"][..., 0].max() <= 64 and t["sxy"][..., 1].max() <= 48
    img = np.full((48, 64), 255, np.uint8)
    assert np.all(um.remap(img, t)[t["outside"] == 1] == 0)


# ---- accuracy anchor: an analytic texture seen through the lens and undistorted again ------------------------------------------------
def texture(x, y):
    """smooth, 8-bit range, periods >= 16 px, in IDEAL pixel coordinates"""
    return 127.5 + 40.0 * np.sin(2 * np.pi * x / 37.0) + 35.0 * np.cos(2 * np.pi * y / 23.0) + 30.0 * np.sin(2 * np.pi * (x + y) / 16.0 + 0.7) + \
        20.0 * np.cos(2 * np.pi * (x - 2.0 * y) / 51.0)


def ideal_of_distorted(w, h, K4, dist):
    """for every pixel p of the DISTORTED image the ideal pixel it shows: the distortion inverted by Newton iterations in float64"""
    fx, fy, cx, cy = K4
    k1, k2, p1, p2, k3, k4, k5, k6 = um._dist8(dist)
    jj, ii = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    xd, yd = (jj - cx) / fx, (ii - cy) / fy
    x, y = xd.copy(), yd.copy()
    for _ in range(30):
        r2 = x * x + y * y
        num, den = 1 + ((k3 * r2 + k2) * r2 + k1) * r2, 1 + ((k6 * r2 + k5) * r2 + k4) * r2
        dnum, dden = (3 * k3 * r2 + 2 * k2) * r2 + k1, (3 * k6 * r2 + 2 * k5) * r2 + k4
        kr, dkr = num / den, (dnum * den - num * dden) / (den * den)
        fu = x * kr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x) - xd
        fv = y * kr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y - yd
        a = kr + 2 * x * x * dkr + 2 * p1 * y + 6 * p2 * x
        b = 2 * x * y * dkr + 2 * p1 * x + 2 * p2 * y
        c_ = 2 * x * y * dkr + 2 * p1 * x + 2 * p2 * y
        d = kr + 2 * y * y * dkr + 6 * p1 * y + 2 * p2 * x
        det = a * d - b * c_
        x, y = x - (d * fu - b * fv) / det, y - (a * fv - c_ * fu) / det
    assert np.abs(fu).max() < 1e-12 and np.abs(fv).max() < 1e-12
    return fx * x + cx, fy * y + cy


# (name, dist, measured maximum absolute error of the model in grey levels, bound = measured + 40 %); EXPERIMENTS.md has the record.  The
# error is the bilinear interpolation error of the texture's curvature as the LENS image shows it (the barrel set compresses the rim by up to
# 1 / 0.6, which is why it is the largest), the 1/32-pixel quantisation of the map and the two roundings to 8 bit.
ANCHOR_SETS = [("barrel", (-0.3, 0.05, 0.0, 0.0), 3.153, 4.4),
               ("pincushion", (0.12, 0.05, 0.0, 0.0, 0.02), 2.333, 3.3),
               ("tangential", (0.0, 0.0, 0.004, -0.003), 2.363, 3.3)]


@pytest.mark.parametrize("name,dist,measured,bound", ANCHOR_SETS, ids=[s[0] for s in ANCHOR_SETS])
def test_undistorting_a_rendered_lens_image_recovers_the_texture(name, dist, measured, bound):
    xi, yi = ideal_of_distorted(W, H, K, dist)
    distorted = np.clip(np.rint(texture(xi, yi)), 0, 255).astype(np.uint8)
    t = um.table(W, H, K, dist)
    got = um.remap(distorted, t).astype(np.float64)
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    inside = um.taps_inside(t)
    assert inside.mean() > 0.5
    err = np.abs(got - texture(jj, ii))[inside].max()
    print("undistort accuracy anchor %s: max |error| %.3f grey levels over %d pixels (bound %.2f)" % (name, err, int(inside.sum()), bound))
    assert bound <= 1.5 * measured and err <= bound


def test_barrel_distortion_leaves_a_zero_rim():
    """k1 < 0 pulls the source of an output pixel TOWARDS the centre, so with new_K = K a moderate field of view has no forced zeros at all;
    they appear where the field is wide enough for the radial polynomial to fold over (1 + k1 r2 < -1, r2 > 6.7 here): a 139 degree lens"""
    w, h, K4 = 320, 240, (60.0, 60.0, 159.5, 119.5)
    t = um.table(w, h, K4, (-0.3, 0.0, 0.0, 0.0))
    forced = t["outside"] != 0
    assert forced.sum() > 0
    # the rim only: the complement is one block that holds the centre, and every row / column of it is an interval
    ok = ~forced
    assert ok[h // 2, w // 2]
    for line in list(ok) + list(ok.T):
        idx = np.flatnonzero(line)
        assert idx.size == 0 or idx[-1] - idx[0] + 1 == idx.size
    assert forced[0].all() or forced[:, 0].all() or forced[0, 0]            # it touches the border
    out = um.undistort(np.full((h, w), 255, np.uint8), K4, (-0.3, 0.0, 0.0, 0.0))
    assert np.all(out[forced] == 0) and np.all(out[um.taps_inside(t)] == 255)
