"""The numpy model of sub-pixel corner refinement (tests/subpix_model.py) against analytic truth, and its branches.  CPU only.

The model is the definition k_corner_subpix is pinned to (tests/test_gpu_subpix.py); here it is shown to find the corners of rendered
checkerboards, to take every exit, and not to depend on the order of its float64 sums."""
import numpy as np
import pytest

import subpix_model as sm

BOARDS = [dict(w=320, h=240, square=24, angle=0.2, seed=11), dict(w=96, h=64, square=16, angle=0.35, seed=12)]


@pytest.fixture(scope="module")
def boards():
    out = []
    for b in BOARDS:
        img, truth = sm.checkerboard(b["w"], b["h"], b["square"], b["angle"])
        out.append((img, truth, sm.board_starts(truth, b["seed"])))
    return out


@pytest.fixture(scope="module")
def noise():
    img = sm.noise_image(320, 240, 5)
    return img, sm.eig_maxima(img)


def _worst(out, truth):
    return float(np.linalg.norm(out.astype(np.float64) - truth, axis=1).max())


def test_checkerboard_corners_default_parameters(boards):
    """default parameters: every corner ends at a stopping test within 0.1 px of the true corner (the integer starts are up to 2.47 px
    away).  Measured with this model: 0.063 px (320 x 240, 117 corners, 3..7 iterations) and 0.051 px (96 x 64, 13 corners, 4..7)."""
    for img, truth, start in boards:
        assert len(truth) >= 4
        out, iters, flags = sm.corner_subpix_np(img, start, **sm.DEFAULTS)
        worst = _worst(out, truth)
        print(f"{img.shape[1]}x{img.shape[0]}: {len(truth)} corners, worst {worst:.4f} px, iters {iters.min()}..{iters.max()}, "
              f"worst start {_worst(start, truth):.3f} px")
        assert (flags == 0).all()
        assert worst <= 0.1                      # measured: 0.0627 / 0.0505


def test_checkerboard_corners_small_window_zero_zone(boards):
    """win = (3, 4), zero zone (1, 1), 5 iterations at most, eps = 0.01: still within 0.1 px.
    Measured with this model: 0.078 px and 0.051 px; every corner ends with flag 0."""
    for img, truth, start in boards:
        out, iters, flags = sm.corner_subpix_np(img, start, win=(3, 4), zero=(1, 1), max_count=5, eps=0.01)
        worst = _worst(out, truth)
        print(f"{img.shape[1]}x{img.shape[0]}: worst {worst:.4f} px, iters {iters.min()}..{iters.max()}, flags {np.bincount(flags, minlength=5)}")
        assert (iters <= 5).all()
        assert worst <= 0.1                      # measured: 0.0777 / 0.0512


def test_every_branch(noise):
    img, corners = noise
    H, W = img.shape
    out, iters, flags = sm.corner_subpix_np(img, corners, **sm.DEFAULTS)
    counts = np.bincount(flags, minlength=5)
    print(f"{len(corners)} corners: flags 0/1/2/3/4 = {counts}, at max_count {(iters == 40).sum()}")
    assert counts[0] >= 1 and counts[2] >= 1 and counts[3] >= 1
    assert (iters[flags == 0] == 40).any()                    # some wander until max_count ...
    assert (iters[flags == 0] < 40).any()                     # ... and some converge
    assert np.array_equal(out[flags == 3], corners[flags == 3])
    kept = flags == 2                                          # a step that left the image and stayed within the window is kept
    assert ((out[kept, 0] < 0) | (out[kept, 0] >= W) | (out[kept, 1] < 0) | (out[kept, 1] >= H)).all()
    assert (np.abs(out - corners) <= 5).all()
    # a constant region is singular at once; rows that are not usable pass through
    flat = img.copy()
    flat[100:140, 100:140] = 77
    rows = np.array([[120, 120], [np.nan, 30], [30, np.inf], [W, 50], [50, H], [-1, 50], [W - 0.5, H - 0.5]], np.float32)
    o, it, fl = sm.corner_subpix_np(flat, rows, **sm.DEFAULTS)
    assert fl[0] == 1 and it[0] == 0 and np.array_equal(o[0], rows[0])
    assert (fl[1:6] == 4).all() and (it[1:6] == 0).all()
    assert np.array_equal(o[1:6], rows[1:6], equal_nan=True)
    assert fl[6] != 4


def test_outputs_do_not_depend_on_the_summation_order(boards, noise):
    """the lane-and-butterfly order of the five float64 sums against a plain raster-order sum: no output bit changes on any test image, so
    the kernel's agreement with the model does not hang on the last bits of the sums"""
    cases = [(img, start) for img, _t, start in boards] + [noise]
    for img, corners in cases:
        for prm in (sm.DEFAULTS, dict(win=(7, 7), zero=(-1, -1), max_count=40, eps=0.001)):
            a = sm.corner_subpix_np(img, corners, order="wave", **prm)
            b = sm.corner_subpix_np(img, corners, order="raster", **prm)
            for x, y in zip(a, b):
                assert np.array_equal(x, y)


def test_mask_table():
    m = sm.mask_table((5, 5))
    assert m.shape == (11, 11) and m.dtype == np.float32 and m[5, 5] == 1.0
    assert m[0, 0] == np.float32(np.float32(np.exp(-1.0)) * np.float32(np.exp(-1.0)))
    assert np.array_equal(m, m[::-1, ::-1]) and np.array_equal(m, m.T)
    z = sm.mask_table((3, 4), (1, 1))
    assert z.shape == (9, 7) and (z[3:6, 2:5] == 0).all() and (z != 0).sum() == 63 - 9
    assert np.array_equal(sm.mask_table((3, 4), (3, 1)), sm.mask_table((3, 4)))     # a zone as wide as the window is ignored
