"""The loss-generic model of the bundle adjustment under the names the tests use: oracle/ba_oracle.py's loss_rho / loss_weight / loss_cost /
loss_normal_equations / loss_solve (scipy's robust losses huber, linear, soft_l1, cauchy, arctan with f_scale C; s = |e|^2, z = s / C^2,
cost = 1/2 C^2 sum rho(z), IRLS weight w = rho'(z)), and the outlier scenes of the robust-loss tests."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import ba_oracle as bo  # noqa: E402

LOSSES = bo.LOSSES
rho = bo.loss_rho
weight = bo.loss_weight
cost = bo.loss_cost
normal_equations = bo.loss_normal_equations
solve = bo.loss_solve


def outlier_scene(n_pts, n_slots, seed, frac=0.05):
    """synthetic.make_ba_scene with a deterministic ~5 % of the observations moved 10-40 px"""
    from vo_mi355x import synthetic as syn
    s = syn.make_ba_scene(n_pts=n_pts, n_slots=n_slots, seed=seed)
    obs = np.array(s["obs"], np.float64)
    rng = np.random.default_rng(1000 + seed)
    seen = np.argwhere(~np.isnan(obs[..., 0]))
    pick = seen[rng.random(len(seen)) < frac]
    ang = rng.uniform(0, 2 * np.pi, len(pick))
    mag = rng.uniform(10.0, 40.0, len(pick))
    obs[pick[:, 0], pick[:, 1], 0] += mag * np.cos(ang)
    obs[pick[:, 0], pick[:, 1], 1] += mag * np.sin(ang)
    return s["K"], np.array(s["poses0"], np.float64), np.array(s["points0"], np.float64), obs
