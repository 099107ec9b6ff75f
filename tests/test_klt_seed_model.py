"""CPU-only: the numpy model of the seeded tracker (tests/klt_seed_model.py), which the GPU tests of vo_klt_track_init are pinned against.

Unseeded it is the C oracle bit for bit; a guess equal to p0 changes nothing; and on two small sequences a constant-velocity guess from the
previous track saves iterations and lands within the tracker's own epsilon of the unseeded result."""
import numpy as np
import pytest

import klt_seed_model as km
import vo_oracle as o


def _klt_points(w, h, n, seed):
    """points inside, on and beyond the border (as tests/test_oracle_crosscheck.py draws them)"""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-20, w + 20, n), rng.uniform(-20, h + 20, n)], 1)
    p[: n // 2] = np.stack([rng.uniform(20, w - 20, n // 2), rng.uniform(20, h - 20, n // 2)], 1)
    p[n // 2] = (0.0, 0.0); p[n // 2 + 1] = (w - 1.0, h - 1.0); p[n // 2 + 2] = (w - 0.5, 3.25)
    return p.astype(np.float32)


def _same_bits(a, b):
    return (np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])
            and np.array_equal(a[2].view(np.uint32), b[2].view(np.uint32)) and np.array_equal(a[3], b[3]))


@pytest.fixture(scope="module", params=["1241x376", "320x240"])
def unseeded(request):
    """frames, points, the model's unseeded result -- computed once per size"""
    from vo_mi355x import synthetic as syn
    if request.param == "1241x376":
        fr, _ = syn.make_sequence(2)
        p0 = _klt_points(1241, 376, 160, 3)
    else:
        fr, _ = syn.make_sequence(2, w=320, h=240, seed=77, margin=64)       # the pyramid truncates at level 2
        p0 = _klt_points(320, 240, 120, 4)
    return fr, p0, km.klt_np(fr[0], fr[1], p0)


def test_unseeded_model_is_the_oracle_bit_for_bit(unseeded):
    fr, p0, got = unseeded
    want = o.klt(fr[0], fr[1], p0, return_iters=True)
    assert _same_bits(got, want)
    assert 0 < want[1].sum() < len(p0)                     # both outcomes occur (border points)


def test_guess_equal_to_p0_is_the_unseeded_tracker(unseeded):
    fr, p0, want = unseeded
    assert _same_bits(km.klt_np(fr[0], fr[1], p0, init=p0), want)
    # a guess that is not finite starts from p0 as well
    g = p0.copy()
    g[0::3, 0] = np.nan; g[1::3, 1] = np.inf; g[2::3] = -np.inf
    assert _same_bits(km.klt_np(fr[0], fr[1], p0, init=g), want)


@pytest.mark.parametrize("w,h,seed", [(320, 240, 77), (256, 160, 5)])
def test_constant_velocity_guess_saves_iterations_and_agrees(w, h, seed):
    """tracking 1 -> 2 from the result of 0 -> 1: the guess p1 + (p1 - p0) against the unseeded start p1.  Measured when this was written:
    summed iterations 653 against 912 (320x240, seed 77) and 643 against 930 (256x160, seed 5), largest difference 0.0026 px.  The bound on
    the difference is the tracker's epsilon, 0.03 px: both runs stop within it of the same fixed point."""
    from vo_mi355x import synthetic as syn
    fr, _ = syn.make_sequence(3, w=w, h=h, seed=seed, margin=64)
    p0 = syn.grid_points(120, w, h, margin=24, seed=3)
    p1 = km.klt_np(fr[0], fr[1], p0)[0]
    g = km.predict(p1, p0)
    plain = km.klt_np(fr[1], fr[2], p1)
    seeded = km.klt_np(fr[1], fr[2], p1, init=g)
    it_plain, it_seeded = int(np.maximum(plain[3], 0).sum()), int(np.maximum(seeded[3], 0).sum())
    both = (plain[1] == 1) & (seeded[1] == 1)
    d = np.abs(plain[0][both] - seeded[0][both]).max()
    print("%dx%d seed %d: iterations %d -> %d, %d / %d tracked in both runs, largest difference %.4f px" % (w, h, seed, it_plain, it_seeded,
                                                                                                         both.sum(), len(p0), d))
    assert it_seeded < it_plain
    assert both.sum() > 100 and d <= 0.03
