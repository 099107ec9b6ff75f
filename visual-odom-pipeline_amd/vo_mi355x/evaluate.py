"""Trajectory evaluation: the scale-aligned absolute trajectory error (ATE) of an estimated trajectory against its ground truth.

A monocular trajectory has an arbitrary scale and frame, so it is first aligned to the ground truth by the similarity (with_scale=False:
the rigid motion) that maps its camera centres onto the ground truth's in the least-squares sense -- Umeyama's closed form on the device
(VoContext.fit_sim3), or its RANSAC where some poses are grossly wrong (VoContext.estimate_sim3).  The residual statistics are plain numpy
on the host: a trajectory holds hundreds of points."""
import numpy as np

from .state import Trajectory


def _poses(x):
    """a Trajectory, a dict t_step -> 4x4, or an array (m, 4, 4) of world->camera poses -> dict t_step -> 4x4"""
    if isinstance(x, Trajectory):
        x = x._poses
    if isinstance(x, dict):
        return {t: np.asarray(H, np.float64).reshape(4, 4) for t, H in x.items()}
    return dict(enumerate(np.asarray(x, np.float64).reshape(-1, 4, 4)))


def camera_centres(est, gt):
    """the camera centres -R^T t of two trajectories over their common time steps -> (steps, est (m, 3), gt (m, 3)) float64"""
    a, b = _poses(est), _poses(gt)
    steps = sorted(set(a) & set(b))
    c = lambda H: -H[:3, :3].T @ H[:3, 3]
    return steps, np.array([c(a[t]) for t in steps]).reshape(-1, 3), np.array([c(b[t]) for t in steps]).reshape(-1, 3)


def align_trajectory(est, gt, ctx, with_scale=True, robust=False, **kw):
    """The similarity gt ~ s R est + t between the camera centres of two trajectories (Trajectory objects, dicts, or arrays of 4 x 4
    world->camera poses) over their common time steps, on the context ctx (batch 1).  robust=False: the least-squares fit over every step
    (fit_sim3); robust=True: RANSAC with a re-fit on the consensus set (estimate_sim3; keywords threshold, confidence, max_iters, seed).
    -> dict s, R, t, S (4 x 4, S[:3, :3] = s R), steps, inliers (indices into steps), stats.  Raises ValueError without a model (fewer than
    three common steps, or centres on one line)."""
    steps, a, b = camera_centres(est, gt)
    if len(steps) < 3:
        raise ValueError("align_trajectory needs at least three common time steps, got %d" % len(steps))
    if robust:
        s, R, t, inliers, st, _ = ctx.estimate_sim3(a, b, with_scale=with_scale, **kw)
    else:
        s, R, t, st = ctx.fit_sim3(a, b, None, with_scale=with_scale)
        inliers = np.arange(len(steps))
    if st["status"] != 0:
        raise ValueError("align_trajectory: no alignment (status %d): the camera centres are degenerate" % st["status"])
    S = np.eye(4)
    S[:3, :3], S[:3, 3] = s * R, t
    return dict(s=float(s), R=R, t=t, S=S, steps=steps, inliers=np.asarray(inliers), stats=st)


def ate(est, gt, ctx, with_scale=True, robust=False, **kw):
    """Absolute trajectory error after align_trajectory -> dict rmse, mean, median, max (of |gt - (s R est + t)| over the common steps, in
    the ground truth's units), scale, S, n"""
    al = align_trajectory(est, gt, ctx, with_scale=with_scale, robust=robust, **kw)
    _, a, b = camera_centres(est, gt)
    e = np.linalg.norm(b - (al["s"] * (a @ al["R"].T) + al["t"]), axis=1)
    return dict(rmse=float(np.sqrt(np.mean(e * e))), mean=float(e.mean()), median=float(np.median(e)), max=float(e.max()), scale=al["s"],
                S=al["S"], n=len(e))
