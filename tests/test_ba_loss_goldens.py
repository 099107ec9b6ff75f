"""CPU: the robust-loss goldens (tests/golden/gen_golden_loss.py: the reference's own BundleAdjuster with `loss=`, scipy's
least_squares) against the loss-generic model, how discriminative the scenes are, and the drop-in's method='lm' boundary."""
import glob
import os

import numpy as np
import pytest

import ba_loss_model as lm
from helpers import BA6_POINT, BA6_ROT, BA6_TRANS, ba_solution_parity, golden_ba_problem, ref_stub_cv2, solution_delta, unpack_ref_x


def loss_goldens(golden_dir):
    return sorted(p for p in glob.glob(os.path.join(golden_dir, "baloss_*.npz")) if str(np.load(p)["loss"]) != "linear")


def load(path):
    cv2 = ref_stub_cv2()
    g = np.load(path)
    gp = np.load(path.replace("baloss_", "balosspolish_"))
    K, poses, points, obs, _ = golden_ba_problem(g, lambda R: cv2.Rodrigues(R)[0])
    return g, gp, str(g["loss"]), K, poses, points, obs


def test_goldens_exist(golden_dir):
    names = {os.path.basename(p) for p in loss_goldens(golden_dir)}
    assert {"baloss_soft_l1_s0_n64_w4.npz", "baloss_cauchy_s0_n64_w4.npz", "baloss_arctan_s0_n64_w4.npz",
            "baloss_soft_l1_s2_n256_w10.npz", "baloss_cauchy_s2_n256_w10.npz"} <= names


def test_model_matches_the_reference_anchors(golden_dir):
    for path in loss_goldens(golden_dir):
        g, gp, loss, K, poses, points, obs = load(path)

        def solve(mi, ftol, xtol):
            r = lm.solve(K, poses, points, obs, loss, max_iters=mi, ftol=ftol, xtol=xtol)
            return r["poses"], r["points"], r["cost"]
        ba_solution_parity(solve, g, gp, K, poses, points, obs)


def test_scenes_tell_the_losses_from_linear(golden_dir):
    """the linear anchor of each scene is at least 10x the BA-6 tolerances away from every robust anchor: a solver that fitted plain
    least squares (what every name but 'huber' ran before) fails ba_solution_parity here"""
    for path in loss_goldens(golden_dir):
        g, gp, loss, K, poses, points, obs = load(path)
        W, N = obs.shape[:2]
        glp = np.load(re_linear(path, "balosspolish_"))
        d = solution_delta(*unpack_ref_x(glp["polish_x"], N, W), *unpack_ref_x(gp["polish_x"], N, W))
        assert d[0] >= 10 * BA6_ROT or d[1] >= 10 * BA6_TRANS or d[2] >= 10 * BA6_POINT, (path, d)


def re_linear(path, prefix):
    """the linear golden of the same scene"""
    base = os.path.basename(path)[len("baloss_"):]
    for loss in ("soft_l1", "cauchy", "arctan"):
        if base.startswith(loss + "_"):
            return os.path.join(os.path.dirname(path), prefix + "linear_" + base[len(loss) + 1:])
    raise ValueError(path)


@pytest.mark.parametrize("n_obs_delta", [-1, 0, 1])
def test_lm_boundary(n_obs_delta):
    """the reference solves with method='lm' (and the linear loss) when the residuals -- ONE per observation, the norm -- outnumber
    the variables 3 N + 6 W (:180-186); otherwise scipy refuses 'lm' (ValueError)"""
    from vo_mi355x.bundle_adjuster import BundleAdjuster
    W, N = 4, 30
    n_var = 3 * N + 6 * W                  # 114 of 120 possible observations
    obs = np.full((W, N, 2), np.nan)
    obs.reshape(-1, 2)[:n_var + n_obs_delta] = 1.0
    ba = BundleAdjuster(method="lm", loss="cauchy")
    if n_obs_delta <= 0:
        with pytest.raises(ValueError):
            ba._solve_loss(obs, N, W)
    else:
        assert ba._solve_loss(obs, N, W) == "linear"
    assert BundleAdjuster(method="trf", loss="cauchy")._solve_loss(obs, N, W) == "cauchy"
