"""Loss-generic restatement of oracle/ba_oracle.py's cost / normal_equations / solve: scipy's robust losses (huber, linear, soft_l1,
cauchy, arctan) with f_scale C.  s = |e|^2, z = s / C^2; cost = 1/2 C^2 sum rho(z), IRLS weight w = rho'(z).  The Jacobian blocks, the
Schur step and the LM schedule are ba_oracle's own."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import ba_oracle as bo  # noqa: E402

LOSSES = ("huber", "linear", "soft_l1", "cauchy", "arctan")


def rho(s, loss, C=1.0):
    """C^2 rho(s / C^2): the cost term of one observation (before the 1/2)"""
    if loss == "huber":
        return bo.huber_rho(s, C)
    d2 = C * C
    z = s / d2
    if loss == "linear":
        return s
    if loss == "soft_l1":
        return d2 * 2.0 * z / (np.sqrt(1.0 + z) + 1.0)
    if loss == "cauchy":
        return d2 * np.log1p(z)
    if loss == "arctan":
        return d2 * np.arctan(z)
    raise ValueError(loss)


def weight(s, loss, C=1.0):
    """rho'(z)"""
    if loss == "huber":
        return bo.huber_weight(s, C)
    z = s / (C * C)
    if loss == "linear":
        return np.ones_like(s)
    if loss == "soft_l1":
        return 1.0 / np.sqrt(1.0 + z)
    if loss == "cauchy":
        return 1.0 / (1.0 + z)
    if loss == "arctan":
        return 1.0 / (1.0 + z * z)
    raise ValueError(loss)


def cost(K, poses, points, obs, loss="huber", C=1.0):
    if loss == "huber":
        return bo.cost(K, poses, points, obs, C)
    r = bo.residual_norm(K, poses, points, obs)
    return 0.5 * rho(r * r, loss, C).sum()


def normal_equations(K, poses, points, obs, loss="huber", C=1.0):
    if loss == "huber":
        return bo.normal_equations(K, poses, points, obs, C)
    e, Jp, Jl, m = bo.jacobian_blocks(K, poses, points, obs)
    s = (e * e).sum(-1)
    w = weight(s, loss, C) * m
    Hpp = np.einsum('wn,wnka,wnkb->wab', w, Jp, Jp)
    Hpl = np.einsum('wn,wnka,wnkb->wnab', w, Jp, Jl)
    Hll = np.einsum('wn,wnka,wnkb->nab', w, Jl, Jl)
    gp = np.einsum('wn,wnka,wnk->wa', w, Jp, e)
    gl = np.einsum('wn,wnka,wnk->na', w, Jl, e)
    c = 0.5 * (rho(s, loss, C) * m).sum()
    return dict(Hpp=Hpp, Hpl=Hpl, Hll=Hll, gp=gp, gl=gl, cost=c)


def solve(K, poses0, points0, obs, loss="huber", C=1.0, max_iters=50, lam0=1e-4, ftol=1e-3, xtol=1e-3, gtol=1e-8, lam_min=1e-3):
    """ba_oracle.solve with the loss as a parameter (the same statements in the same order)"""
    if loss == "huber":
        return bo.solve(K, poses0, points0, obs, max_iters=max_iters, lam0=lam0, ftol=ftol, xtol=xtol, gtol=gtol, delta=C, lam_min=lam_min)
    poses, points = np.array(poses0, np.float64), np.array(points0, np.float64)
    lam, nu = lam0, 2.0
    F = cost(K, poses, points, obs, loss, C)
    F0 = F
    status, it, n_acc = 0, 0, 0
    for it in range(1, max_iters + 1):
        ne = normal_equations(K, poses, points, obs, loss, C)
        ginf = max(np.abs(ne['gp']).max(), np.abs(ne['gl']).max())
        if ginf < gtol:
            status = 1; it -= 1
            break
        dp, dl, pred = bo.lm_step(ne, lam)
        tp, tl = poses + dp, points + dl
        Ft = cost(K, tp, tl, obs, loss, C)
        step = np.sqrt((dp * dp).sum() + (dl * dl).sum())
        xn = np.sqrt((poses * poses).sum() + (points * points).sum())
        r = (F - Ft) / pred if pred > 0 else -1.0
        if Ft < F and r > 0:
            dF = F - Ft
            poses, points, F = tp, tl, Ft
            n_acc += 1
            lam = lam * max(1.0 / 3.0, 1.0 - (2.0 * r - 1.0) ** 3); nu = 2.0
            lam = max(lam, lam_min)
            if dF < ftol * F:
                status = 2
                break
            if step < xtol * (xtol + xn):
                status = 3
                break
        else:
            if step < xtol * (xtol + xn):
                status = 3
                break
            lam *= nu; nu *= 2.0
            if lam > 1e12:
                status = 4
                break
    return dict(poses=poses, points=points, cost=F, cost0=F0, iters=it, accepted=n_acc, status=status, lam=lam)


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
