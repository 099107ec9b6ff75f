"""CPU-only: the loss-generic model (oracle/ba_oracle.py loss_*) is scipy.optimize.least_squares' operation at every f_scale -- the cost and
the gradient at x0 of the reference's objective (one residual per observation, the pixel-error norm) under scipy's own loss = ..., f_scale = C
equal the model's cost and its IRLS gradient sum w J^T e.  Also the OracleContext back end of the closed-loop model with a robust loss."""
import numpy as np
import pytest

import ba_loss_model as lm
from ba_loss_model import bo


def _problem():
    K, poses, points, obs = lm.outlier_scene(24, 3, 2)
    obs[1, 5] = np.nan
    return K, poses, points, obs


def _fun_jac(K, obs):
    W, N = obs.shape[:2]

    def fun(x):
        poses, points = bo.unpack_x(x, N, W)
        return bo.residual_norm(K, poses, points, obs)

    def jac(x):
        """d r / dx = e^T J_e / r, rows in residual_norm's order (slot-major, ascending landmark), columns in pack_x0's"""
        poses, points = bo.unpack_x(x, N, W)
        e, Jp, Jl, m = bo.jacobian_blocks(K, poses, points, obs)
        rows = []
        for i, j in np.argwhere(m):
            r = np.linalg.norm(e[i, j])
            row = np.zeros(3 * N + 6 * W)
            row[3 * j:3 * j + 3] = e[i, j] @ Jl[i, j] / r
            row[3 * N + 6 * i:3 * N + 6 * i + 6] = e[i, j] @ Jp[i, j] / r
            rows.append(row)
        return np.array(rows)
    return fun, jac


@pytest.mark.parametrize("C", (0.3, 1.0, 4.0))
@pytest.mark.parametrize("loss", lm.LOSSES)
def test_model_cost_and_gradient_are_scipys(loss, C):
    from scipy.optimize import least_squares
    K, poses, points, obs = _problem()
    fun, jac = _fun_jac(K, obs)
    x0 = bo.pack_x0(poses, points)
    ne = lm.normal_equations(K, poses, points, obs, loss, C)
    g = np.concatenate([ne["gl"].reshape(-1), ne["gp"].reshape(-1)])
    assert abs(lm.cost(K, poses, points, obs, loss, C) - ne["cost"]) <= 1e-14 * ne["cost"]
    # scipy with the analytic Jacobian of the residual norms: its loss scaling is all that differs from the model
    res = least_squares(fun, x0, jac=jac, loss=loss, f_scale=C, max_nfev=1)
    assert np.array_equal(res.x, x0)
    assert abs(res.cost - ne["cost"]) <= 1e-13 * ne["cost"], (res.cost, ne["cost"])
    assert np.abs(res.grad - g).max() <= 1e-11 * np.abs(g).max(), np.abs(res.grad - g).max() / np.abs(g).max()
    # and with scipy's own finite differences (the reference's jac = '2-point'): the gradient to their accuracy
    res = least_squares(fun, x0, loss=loss, f_scale=C, max_nfev=1)
    assert abs(res.cost - ne["cost"]) <= 1e-13 * ne["cost"]
    assert np.abs(res.grad - g).max() <= 1e-4 * np.abs(g).max()


def test_huber_of_the_loss_model_is_ba_oracle_bit_for_bit():
    K, poses, points, obs = _problem()
    a = lm.solve(K, poses, points, obs, "huber", 1.0, max_iters=15)
    b = bo.solve(K, poses, points, obs, max_iters=15)
    assert np.array_equal(a["poses"], b["poses"]) and np.array_equal(a["points"], b["points"]) and a["cost"] == b["cost"]
    assert (a["iters"], a["accepted"], a["status"]) == (b["iters"], b["accepted"], b["status"])
    assert a["margin"] > 0


@pytest.mark.parametrize("loss", ("huber", "soft_l1", "cauchy", "arctan"))
def test_oracle_context_routes_the_loss(loss):
    """OracleContext (the closed-loop model's CPU back end): Huber through ba_oracle.solve, every other loss through loss_solve with its
    f_scale; an unknown name is refused"""
    import oracle_context_impl as oc
    K, poses, points, obs = _problem()
    ctx = oc.OracleContext.__new__(oc.OracleContext)
    po, pt, st = ctx.ba_adjust(K, poses, points, obs, ctx.ba_params(max_iters=10, loss=loss, huber_delta=2.0))
    ref = lm.solve(K, poses, points, obs, loss, 2.0, max_iters=10)
    assert np.array_equal(po, ref["poses"]) and np.array_equal(pt, ref["points"]) and st["cost"] == ref["cost"]
    assert (st["iters"], st["accepted"], st["status"]) == (ref["iters"], ref["accepted"], ref["status"])
    with pytest.raises(ValueError):
        ctx.ba_params(loss="tukey")
