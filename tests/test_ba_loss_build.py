"""CPU-only: the robust-loss kernels of the bundle adjustment as hipcc builds them, the C ABI mirror, and the loss-generic model.

The build / update kernels are templated on the loss (last template argument): the Huber instances (LOSS = 0) keep the figures they had as
kernels of their own (VGPRs, SGPRs, scratch, occupancy from -Rpass-analysis=kernel-resource-usage), and every robust instance keeps its
figures too: no scratch, no lower occupancy."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

from build_helpers import kernel_resources

import ba_loss_model as lm

MAIN = {   # the Huber instances: (VGPRs, SGPRs, scratch, occupancy)
    "_Z12k_ba_build_wILi4ELi2ELi5ELi0EE": (256, 102, 0, 2), "_Z12k_ba_build_wILi4ELi2ELi8ELi0EE": (256, 92, 12, 2),
    "_Z12k_ba_build_wILi4ELi1ELi8ELi0EE": (218, 90, 0, 2), "_Z12k_ba_build_wILi3ELi1ELi8ELi0EE": (186, 90, 0, 2),
    "_Z12k_ba_build_wILi2ELi1ELi8ELi0EE": (162, 90, 0, 3), "_Z12k_ba_build_wILi2ELi1ELi4ELi0EE": (162, 90, 0, 3),
    "_Z12k_ba_build_wILi1ELi1ELi8ELi0EE": (144, 90, 0, 3), "_Z12k_ba_build_wILi1ELi1ELi4ELi0EE": (144, 90, 0, 3),
    "_Z13k_ba_update_wILi2ELi5ELi0EE": (230, 76, 0, 2), "_Z13k_ba_update_wILi2ELi8ELi0EE": (228, 74, 0, 2),
    "_Z13k_ba_update_wILi1ELi4ELi0EE": (150, 70, 0, 3), "_Z13k_ba_update_wILi1ELi8ELi0EE": (150, 70, 0, 3),
    "_Z10k_ba_buildILi1024ELi0ELi0EE": (127, 106, 0, 4), "_Z10k_ba_buildILi512ELi0ELi0EE": (127, 106, 0, 4),
    "_Z10k_ba_buildILi256ELi0ELi0EE": (127, 106, 0, 4), "_Z10k_ba_buildILi256ELi8ELi0EE": (126, 106, 0, 4),
    "_Z11k_ba_updateILi256ELi8ELi0EE": (72, 55, 0, 7), "_Z11k_ba_updateILi256ELi0ELi0EE": (72, 56, 0, 7),
    "_Z11k_ba_updateILi512ELi0ELi0EE": (72, 56, 0, 7), "_Z11k_ba_updateILi1024ELi0ELi0EE": (72, 56, 0, 7),
}

ROBUST = {   # soft_l1 (2), cauchy (3), arctan (4).  The updates came out better as kernels than behind one-line wrapper kernels:
             # k_ba_update_w 2 VGPRs fewer (cauchy <1, *> occupancy 2 -> 3), k_ba_update 66-70 VGPRs at occupancy 7 (was 72-76, mostly 6)
    "_Z12k_ba_build_wILi1ELi1ELi4ELi2EE": (140, 90, 0, 3), "_Z12k_ba_build_wILi1ELi1ELi4ELi3EE": (140, 90, 0, 3), "_Z12k_ba_build_wILi1ELi1ELi4ELi4EE": (140, 90, 0, 3),
    "_Z12k_ba_build_wILi1ELi1ELi8ELi2EE": (140, 90, 0, 3), "_Z12k_ba_build_wILi1ELi1ELi8ELi3EE": (140, 90, 0, 3), "_Z12k_ba_build_wILi1ELi1ELi8ELi4EE": (140, 90, 0, 3),
    "_Z12k_ba_build_wILi2ELi1ELi4ELi2EE": (156, 90, 0, 3), "_Z12k_ba_build_wILi2ELi1ELi4ELi3EE": (156, 90, 0, 3), "_Z12k_ba_build_wILi2ELi1ELi4ELi4EE": (156, 90, 0, 3),
    "_Z12k_ba_build_wILi2ELi1ELi8ELi2EE": (156, 90, 0, 3), "_Z12k_ba_build_wILi2ELi1ELi8ELi3EE": (156, 90, 0, 3), "_Z12k_ba_build_wILi2ELi1ELi8ELi4EE": (156, 90, 0, 3),
    "_Z12k_ba_build_wILi3ELi1ELi8ELi2EE": (180, 90, 0, 2), "_Z12k_ba_build_wILi3ELi1ELi8ELi3EE": (180, 90, 0, 2), "_Z12k_ba_build_wILi3ELi1ELi8ELi4EE": (180, 90, 0, 2),
    "_Z12k_ba_build_wILi4ELi1ELi8ELi2EE": (212, 90, 0, 2), "_Z12k_ba_build_wILi4ELi1ELi8ELi3EE": (212, 90, 0, 2), "_Z12k_ba_build_wILi4ELi1ELi8ELi4EE": (212, 90, 0, 2),
    "_Z12k_ba_build_wILi4ELi2ELi5ELi2EE": (248, 98, 0, 2), "_Z12k_ba_build_wILi4ELi2ELi5ELi3EE": (248, 98, 0, 2), "_Z12k_ba_build_wILi4ELi2ELi5ELi4EE": (248, 98, 0, 2),
    "_Z12k_ba_build_wILi4ELi2ELi8ELi2EE": (250, 90, 0, 2), "_Z12k_ba_build_wILi4ELi2ELi8ELi3EE": (250, 90, 0, 2), "_Z12k_ba_build_wILi4ELi2ELi8ELi4EE": (250, 90, 0, 2),
    "_Z13k_ba_update_wILi1ELi4ELi2EE": (146, 68, 0, 3), "_Z13k_ba_update_wILi1ELi4ELi3EE": (168, 76, 0, 3), "_Z13k_ba_update_wILi1ELi4ELi4EE": (174, 78, 0, 2),
    "_Z13k_ba_update_wILi1ELi8ELi2EE": (146, 68, 0, 3), "_Z13k_ba_update_wILi1ELi8ELi3EE": (168, 76, 0, 3), "_Z13k_ba_update_wILi1ELi8ELi4EE": (174, 78, 0, 2),
    "_Z13k_ba_update_wILi2ELi5ELi2EE": (226, 74, 0, 2), "_Z13k_ba_update_wILi2ELi5ELi3EE": (228, 102, 0, 2), "_Z13k_ba_update_wILi2ELi5ELi4EE": (229, 106, 0, 2),
    "_Z13k_ba_update_wILi2ELi8ELi2EE": (224, 72, 0, 2), "_Z13k_ba_update_wILi2ELi8ELi3EE": (226, 100, 0, 2), "_Z13k_ba_update_wILi2ELi8ELi4EE": (227, 106, 0, 2),
    "_Z10k_ba_buildILi1024ELi0ELi2EE": (120, 106, 0, 4), "_Z10k_ba_buildILi1024ELi0ELi3EE": (120, 106, 0, 4), "_Z10k_ba_buildILi1024ELi0ELi4EE": (120, 106, 0, 4),
    "_Z10k_ba_buildILi512ELi0ELi2EE": (120, 106, 0, 4), "_Z10k_ba_buildILi512ELi0ELi3EE": (120, 106, 0, 4), "_Z10k_ba_buildILi512ELi0ELi4EE": (120, 106, 0, 4),
    "_Z10k_ba_buildILi256ELi0ELi2EE": (120, 106, 0, 4), "_Z10k_ba_buildILi256ELi0ELi3EE": (120, 106, 0, 4), "_Z10k_ba_buildILi256ELi0ELi4EE": (120, 106, 0, 4),
    "_Z10k_ba_buildILi256ELi8ELi2EE": (118, 106, 0, 4), "_Z10k_ba_buildILi256ELi8ELi3EE": (118, 106, 0, 4), "_Z10k_ba_buildILi256ELi8ELi4EE": (118, 106, 0, 4),
    "_Z11k_ba_updateILi256ELi8ELi2EE": (66, 58, 0, 7), "_Z11k_ba_updateILi256ELi8ELi3EE": (70, 58, 0, 7), "_Z11k_ba_updateILi256ELi8ELi4EE": (70, 58, 0, 7),
    "_Z11k_ba_updateILi256ELi0ELi2EE": (66, 56, 0, 7), "_Z11k_ba_updateILi256ELi0ELi3EE": (70, 56, 0, 7), "_Z11k_ba_updateILi256ELi0ELi4EE": (70, 56, 0, 7),
    "_Z11k_ba_updateILi512ELi0ELi2EE": (66, 56, 0, 7), "_Z11k_ba_updateILi512ELi0ELi3EE": (70, 56, 0, 7), "_Z11k_ba_updateILi512ELi0ELi4EE": (70, 56, 0, 7),
    "_Z11k_ba_updateILi1024ELi0ELi2EE": (66, 56, 0, 7), "_Z11k_ba_updateILi1024ELi0ELi3EE": (70, 56, 0, 7), "_Z11k_ba_updateILi1024ELi0ELi4EE": (70, 56, 0, 7),
}


@pytest.fixture(scope="module")
def ba_resources():
    return kernel_resources("vo_ba.hip")


def _fig(r):
    return (r["VGPRs"], r["TotalSGPRs"], r["ScratchSize"], r["Occupancy"])


def test_huber_kernels_keep_their_resources(ba_resources):
    for prefix, want in MAIN.items():
        (r,) = [v for k, v in ba_resources.items() if k.startswith(prefix + "v")]
        assert _fig(r) == want, (prefix, _fig(r))


def test_robust_kernels_keep_their_resources(ba_resources):
    for prefix, want in ROBUST.items():
        (r,) = [v for k, v in ba_resources.items() if k.startswith(prefix + "v")]
        assert _fig(r) == want, (prefix, _fig(r))


def test_robust_kernels_exist_for_every_loss_and_geometry(ba_resources):
    for loss in (2, 3, 4):
        wave = [k for k in ba_resources if re.match(r"_Z12k_ba_build_wILi\dELi\dELi\dELi%dEEv" % loss, k)]
        wupd = [k for k in ba_resources if re.match(r"_Z13k_ba_update_wILi\dELi\dELi%dEEv" % loss, k)]
        lane = [k for k in ba_resources if re.match(r"_Z10k_ba_buildILi\d+ELi\dELi%dEEv" % loss, k)]
        lupd = [k for k in ba_resources if re.match(r"_Z11k_ba_updateILi\d+ELi\dELi%dEEv" % loss, k)]
        assert (len(wave), len(wupd), len(lane), len(lupd)) == (8, 4, 4, 4), loss


def test_robust_kernels_have_no_scratch(ba_resources):
    """every robust build / update / cost kernel runs without scratch; the lane-per-observation builds keep the Huber occupancy (4)"""
    new = [k for k in ba_resources if re.match(r"_Z1[0-3]k_ba_(build|update)(_w)?I(Li\d+E)+Li[234]EEv|_Z\d+k_ba_cost_r", k)]
    assert len(new) == 3 * (8 + 4 + 4 + 4) + 3, len(new)
    for k in new:
        assert ba_resources[k]["ScratchSize"] == 0, (k, ba_resources[k])
        if re.match(r"_Z10k_ba_buildI", k):
            assert ba_resources[k]["Occupancy"] == 4, (k, ba_resources[k])


def test_ctypes_mirror_has_the_loss():
    from vo_mi355x import _lib
    assert _lib.BaParams.loss.offset == 4 and ctypes.sizeof(_lib.BaParams) == 56
    L = _lib.load()
    b = _lib.BaParams(); b.loss = 7
    L.vo_ba_default_params(ctypes.byref(b))
    assert b.loss == 0
    assert [_lib.loss_code(n) for n in ("huber", "linear", "soft_l1", "cauchy", "arctan")] == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError):
        _lib.loss_code("tukey")
    with pytest.raises(NotImplementedError):
        _lib.loss_code(lambda z: z)


def test_model_huber_is_the_oracle_bit_for_bit(golden_dir):
    import ba_oracle as bo
    from helpers import golden_ba_problem, ref_stub_cv2
    cv2 = ref_stub_cv2()
    paths = sorted(glob.glob(os.path.join(golden_dir, "ba_s[0-9]*.npz")))      # the reference's vectors ba_s<seed>_n<N>_w<W> (not the model's ba_so3_<case>)
    assert paths
    for path in paths:
        K, poses, points, obs, _ = golden_ba_problem(np.load(path), lambda R: cv2.Rodrigues(R)[0])
        a = lm.solve(K, poses, points, obs, "huber", max_iters=10)
        b = bo.solve(K, poses, points, obs, max_iters=10)
        assert np.array_equal(a["poses"], b["poses"]) and np.array_equal(a["points"], b["points"]) and a["cost"] == b["cost"]


def test_model_losses_are_consistent():
    """rho' is the derivative of rho (central differences), and the linear / huber-with-a-far-knee costs agree"""
    s = np.array([0.0, 1e-6, 0.3, 1.0, 4.0, 250.0, 1600.0])
    for loss in lm.LOSSES:
        for C in (1.0, 2.5):
            h = 1e-6 * np.maximum(s, 1.0)
            d = (lm.rho(s + h, loss, C) - lm.rho(np.maximum(s - h, 0), loss, C)) / (s + h - np.maximum(s - h, 0))
            assert np.allclose(d, lm.weight(s, loss, C), rtol=1e-5, atol=1e-7), (loss, C)
    assert np.allclose(lm.rho(s, "linear"), lm.rho(s, "huber", 1e30))


def test_model_robust_solves_reject_outliers():
    """each robust loss on an outlier scene reduces its own cost and lands away from the linear fit"""
    K, poses, points, obs = lm.outlier_scene(64, 4, 0)
    lin = lm.solve(K, poses, points, obs, "linear", max_iters=30)
    for loss in ("soft_l1", "cauchy", "arctan"):
        r = lm.solve(K, poses, points, obs, loss, max_iters=30)
        assert r["cost"] < r["cost0"] and r["accepted"] > 0
        assert np.abs(r["poses"] - lin["poses"]).max() > 1e-6, loss
