"""CPU-only: what OpenCV does with keypoints that are NaN, infinite or beyond int32 (tests/nonfinite_cases.py), stated twice -- by the C oracle
(cv_floor, the clipped circle) and by the numpy model (klt_seed_model.cv_floor / to_int32) -- so that the GPU tests of
tests/test_gpu_nonfinite.py have a second opinion on exactly these rows; and the conditions under which agreement there means something:
a disc at the origin or on column 0 changes the corner list of the case image."""
import numpy as np
import pytest

import klt_seed_model as km
import nonfinite_cases as nc
import vo_oracle as o

INT_MIN = -(1 << 31)


@pytest.fixture(scope="module")
def case():
    p0, kind = nc.points()
    return nc.frames(), p0, kind


def _same(a, b, what):
    assert np.array_equal(a[1], b[1]), (what, "status")
    assert np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)), (what, "err")
    assert np.array_equal(a[3], b[3]), (what, "iters")
    assert np.array_equal(a[0], b[0], equal_nan=True), (what, "p1")


def test_the_case_rows_are_what_they_claim(case):
    fr, p0, kind = case
    assert fr.shape == (2, nc.H, nc.W) and len(p0) % 4 != 0 and len(p0) % 64 != 0
    assert (kind == "honest").sum() == nc.N_HONEST and (kind != "honest").sum() == len(nc.SPECIAL)
    bits = p0.view(np.uint32)
    assert (bits == 0xFFC00001).sum() == 2 and (bits[(bits == 0xFFC00001)] & 0xFFFF).all()       # the payload's low 16 bits are not zero
    assert (p0 == np.float32(2147483520.0)).sum() == 2 and np.nextafter(np.float32(2147483520.0), np.float32(np.inf)) == 2.0 ** 31
    assert (p0 == np.float32(-2147483904.0)).sum() == 2 and np.nextafter(np.float32(-2.0 ** 31), np.float32(-np.inf)) == -2147483904.0
    assert nc.has_nan(p0).sum() == 7 and np.isinf(p0).any(-1).sum() == 8
    # every batch-of-3 sequence holds the same special rows at other indices
    _, pb, kb = nc.batch3()
    where = [set(np.flatnonzero(kb[b] != "honest")) for b in range(3)]
    assert where[0] != where[1] != where[2] != where[0]
    for b in range(3):
        assert sorted(pb[b][kb[b] != "honest"].view(np.uint32).tolist()) == sorted(p0[kind != "honest"].view(np.uint32).tolist())


def test_cv_floor_and_to_int32():
    f = np.float32
    for x, want in ((np.nan, INT_MIN), (np.inf, INT_MIN), (-np.inf, INT_MIN), (2.0 ** 31, INT_MIN), (2147483520.0, 2147483520),
                    (-2.0 ** 31, INT_MIN), (-2147483904.0, INT_MIN), (1e10, INT_MIN), (-3e38, INT_MIN), (-0.5, -1), (-0.0, 0), (2.75, 2),
                    (-7.9, -8), (1e6, 1000000)):
        assert km.cv_floor(f(x)) == want, x
    got = km.to_int32(np.array([np.nan, np.inf, -np.inf, 2.0 ** 31, 2147483520.0, -2.0 ** 31, -2147483904.0, 1e10, -0.5, -7.9, 7.9, -0.0], f))
    assert got.dtype == np.int32
    assert got.tolist() == [INT_MIN, INT_MIN, INT_MIN, INT_MIN, 2147483520, INT_MIN, INT_MIN, INT_MIN, 0, -7, 7, 0]      # toward zero
    assert km.to_int32(np.zeros((3, 2), f)).shape == (3, 2)


def test_oracle_equals_the_numpy_model_on_every_row_unseeded(case):
    fr, p0, kind = case
    want = km.klt_np(fr[0], fr[1], p0)
    got = o.klt(fr[0], fr[1], p0, return_iters=True)
    _same(got, want, "unseeded")
    assert got[1][kind == "honest"].all()                       # the honest rows are tracked: the pair is not degenerate
    # the rows OpenCV leaves alone: outside at every level through cvFloor = INT_MIN (or an honest huge int)
    dead = (kind == "dead") | (kind == "far")
    print("special rows %d, of them outside every level %d, status 0 in all %d" % ((kind != "honest").sum(), dead.sum(), (got[1] == 0).sum()))
    assert dead.sum() == 28
    assert (got[1][dead] == 0).all() and (got[2][dead] == 0).all() and (got[3][dead] == -1).all()
    assert np.array_equal(got[0][dead].view(np.uint32), p0[dead].view(np.uint32))          # p1 is p0, payload and sign included
    # ... and they disturb nobody: the other rows are what a call without them returns
    rest = ~dead
    alone = o.klt(fr[0], fr[1], p0[rest], return_iters=True)
    for k in range(4):
        assert np.array_equal(got[k][rest], alone[k], equal_nan=True), k


@pytest.mark.parametrize("name", ["finite_guess_special_p0", "special_guess_honest_p0"])
def test_oracle_equals_the_numpy_model_on_every_row_seeded(case, name):
    fr = case[0]
    p0, g, kind = nc.seed_cases()[name]
    want = km.klt_np(fr[0], fr[1], p0, init=g)
    got = o.klt(fr[0], fr[1], p0, return_iters=True, init=g)
    _same(got, want, name)
    dead = (kind == "dead") | (kind == "far")
    if name == "finite_guess_special_p0":
        # the template is outside whatever the guess: no level entered, and the scaled guess is passed down unchanged
        assert (got[1][dead] == 0).all() and (got[2][dead] == 0).all() and (got[3][dead] == -1).all()
        assert np.array_equal(got[0][dead], g[dead])
    else:
        # a guess that is not finite starts from p0: the unseeded bits; a huge finite one starts outside: status 0 without an iteration
        plain = o.klt(fr[0], fr[1], p0, return_iters=True)
        nonfin = ~np.isfinite(g).all(-1)
        assert nonfin.sum() == 13
        for k in range(4):
            assert np.array_equal(got[k][nonfin], plain[k][nonfin]), k
        huge = dead & ~nonfin
        top = o.pyr_levels(nc.W, nc.H)
        assert top == 1 and huge.sum() == 15 and (got[1][huge] == 0).all() and (got[2][huge] == 0).all()
        assert (got[3][huge][:, :top + 1] == 0).all() and (got[3][huge][:, top + 1:] == -1).all()
        assert np.array_equal(got[0][huge], g[huge])
    assert got[1][kind == "honest"].all()


@pytest.mark.parametrize("radius", nc.RADII)
def test_circle_mask_at_the_special_centres(case, radius):
    _, p0, kind = case
    centres = km.to_int32(p0)
    hw = o.circle_rows(radius)
    assert hw[0] == radius and (hw >= 0).all() and (np.diff(hw) <= 0).all()
    n_dead = 0
    for (cx, cy), k in zip(centres, kind):
        mask = np.full((nc.H, nc.W), 255, np.uint8)
        o.circle_mask(mask, (int(cx), int(cy)), radius, 0)
        if k in ("dead", "far"):
            assert (mask == 255).all(), (cx, cy, radius)         # non-finite, beyond int, or far away: no pixel
            n_dead += 1
        else:
            assert np.array_equal(mask == 0, nc.brute_disc(cx, cy, radius, hw)), (cx, cy, radius)
    assert n_dead == 28
    # the extreme int centres the issue names, whatever row they came from
    for c in ((INT_MIN, 60), (2 ** 31 - 1, 60), (2 ** 31 - 8, 60), (80, INT_MIN), (80, 2 ** 31 - 1), (INT_MIN, INT_MIN), (-radius - 1, 5),
              (nc.W + radius, 5), (5, -radius - 1), (5, nc.H + radius)):
        mask = np.full((nc.H, nc.W), 255, np.uint8)
        o.circle_mask(mask, c, radius, 0)
        assert (mask == 255).all(), (c, radius)
    # ... and just inside the clip: one pixel column / row of the disc is drawn
    for c in ((-radius, 5), (nc.W - 1 + radius, 5), (5, -radius), (5, nc.H - 1 + radius)):
        mask = np.full((nc.H, nc.W), 255, np.uint8)
        o.circle_mask(mask, c, radius, 0)
        assert np.array_equal(mask == 0, nc.brute_disc(c[0], c[1], radius, hw)) and (mask == 0).any(), (c, radius)
    whole = nc.disc_mask(p0, radius)
    want = np.zeros((nc.H, nc.W), bool)
    for (cx, cy), k in zip(centres, kind):
        if k not in ("dead", "far"):
            want |= nc.brute_disc(cx, cy, radius, hw)
    print("radius %d: %d pixels cleared by %d centres" % (radius, (whole == 0).sum(), (kind != "dead").sum()))
    assert np.array_equal(whole == 0, want)


def test_brute_disc_is_the_euclidean_disc_up_to_the_outline():
    """the half widths are those of dx^2 + dy^2 <= r^2, or one more where the midpoint outline steps outside it"""
    for radius in nc.RADII:
        hw = o.circle_rows(radius)
        for dy in range(radius + 1):
            eu = int(np.floor(np.sqrt(radius * radius - dy * dy)))
            assert eu <= hw[dy] <= eu + 1, (radius, dy)


def test_a_spurious_disc_at_the_origin_or_on_column_0_changes_the_corner_list(case):
    """a NaN centre converted to 0 would carve a disc at (0, 0), (0, y) or (x, 0): the case image has corners there, so it cannot hide"""
    fr, p0, kind = case
    p0, kind = nc.without_border(p0, kind)                      # (the border rows' own discs cover the origin: the GPU tests keep them apart too)
    assert len(p0) % 4 != 0 and (kind == "dead").sum() == 27
    base = nc.disc_mask(p0, 7)
    assert (base == 0).sum() > 0 and (base[:12, :12] == 255).all() and (base[50:70, :12] == 255).all()
    c0 = o.good_features(fr[1], base)
    assert len(c0) > 20
    near0 = np.hypot(c0[:, 0], c0[:, 1]) <= 7
    assert near0.any(), c0[:6]                                  # a strong corner within 7 pixels of pixel (0, 0)
    m1 = base.copy(); o.circle_mask(m1, (0, 0), 7, 0)
    c1 = o.good_features(fr[1], m1)
    assert not (c1.shape == c0.shape and np.array_equal(c1, c0))
    m2 = m1.copy(); o.circle_mask(m2, (0, 60), 7, 0)
    c2 = o.good_features(fr[1], m2)
    assert not (c2.shape == c1.shape and np.array_equal(c2, c1))
    m3 = base.copy(); o.circle_mask(m3, (0, 60), 7, 0)
    c3 = o.good_features(fr[1], m3)
    assert not (c3.shape == c0.shape and np.array_equal(c3, c0))
