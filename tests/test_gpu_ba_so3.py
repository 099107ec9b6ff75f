"""GPU: the bundle adjustment's linearisation, reduced system, LM step and trial cameras at rotations the rest of the suite never feeds them,
against the INDEPENDENT high-precision model tests/so3_model.py (mpmath at 60 digits, Jacobians by central differences, no Jr anywhere) through
its committed results tests/golden/ba_so3_<case>.npz.  This file needs no mpmath and nothing outside the repository.

Every other BA problem of the suite has rotation vectors (0, yaw, 0) -- four of the nine entries of R and of Jr in d_camera (csrc/vo_ba_dev.h)
are then identically zero -- KITTI's K and every point in front of every camera, and is judged by oracle/ba_oracle.py, which shares the kernels'
formulas.  The cases here (so3_model's docstring): one edge angle per slot about an axis with no small component -- 0, 1e-9, either side of the
series switch th2 = 1e-8, pi - 1e-6, pi + 0.2, 2 pi - 1e-3 where Jr is nearly singular, 7.5 -- a K with skew and a third row, outliers, missing
observations, a landmark at camera-frame depth 0.5 and one BEHIND a camera.

  family                  vo_tuning.ba_kernels   cases     losses                                   batch
  wave-private            2                      A, B, C   all five at C = 1 + Huber at C = 2.5     1
  lane-per-observation    1                      A, C, D   the same                                 1      (D: W 12)
  rule -> k_ba_build_f    0                      A, B      Huber, linear                            3      (problem 0 = the case, 1 = its landmarks
                                                                                                            reversed, 2 = its slots rolled by one)
Tolerances: block-relative for Hpp, gp, Hll, gl (each block against its own largest magnitude), relative for the cost, norm-relative for S, rhs,
dposes, dpoints; each is 8 x the recorded CPU value so3_model.ORACLE_DEV[case][quantity] -- what oracle/ba_oracle.py achieves against the model,
measured and asserted by tests/test_so3_model.py -- capped at the suite's existing bounds so3_model.CAPS (1e-10 blocks, 1e-12 cost, 1e-8 S and rhs,
1e-6 steps).  Why 8: FMA contraction and another summation order over <= 240 terms cost a few ulps of the largest term; 8 x stays eleven orders
below what a wrong sign in Jr costs: tests/test_so3_model.py::test_mutants_fail_the_probe_comparison shows, on the CPU, the same comparison
(so3_model.check_probe at these tolerances) rejecting three mutated linearisations in every case and loss run (so3_model.MUTANT_MARGIN).  None
comes from a device result.
Solves (case A, Huber and Cauchy, <= 8 iterations, every family): cost0 is the fixture's cost; the reported cost is so3_model.cost_ld -- the cost
in numpy.longdouble -- at the returned (poses, points) to 1e-12, which pins the trial cameras of k_ba_solve and k_ba_update at off-axis rotations.
(Under the rule the Cauchy solve runs the wave-private kernels: the factored ones take the Huber and linear losses.)"""
import numpy as np
import pytest

import so3_model as sm

pytestmark = pytest.mark.gpu

ALL_RUNS = tuple(tag for tag, _, _ in sm.LOSS_RUNS)
FAMILIES = {"wave": (2, ("A", "B", "C"), ALL_RUNS, 1), "lane": (1, ("A", "C", "D"), ALL_RUNS, 1), "rule": (0, ("A", "B"), ("huber", "linear"), 3)}
PROBES = [(fam, name) for fam, (_, names, _, _) in FAMILIES.items() for name in names]


@pytest.fixture(scope="module")
def fixtures():
    return {name: sm.load(name) for name in sm.CASES}


@pytest.fixture(scope="module")
def contexts():
    """one context per batch size"""
    from vo_mi355x import VoContext
    cs = {B: VoContext(64, 64, max_pts=64, batch=B) for B in (1, 3)}
    yield cs
    for c in cs.values():
        c.close()


def variant(fx, v):
    """v = 0: the case; 1: its landmarks in reversed order; 2: its slots rolled by one.  The same observations: the same cost, term by term"""
    poses, points, obs = fx["poses0"], fx["points0"], fx["obs"]
    if v == 1:
        points, obs = points[::-1], obs[:, ::-1]
    elif v == 2:
        poses, obs = np.roll(poses, 1, axis=0), np.roll(obs, 1, axis=0)
    return fx["K"], np.ascontiguousarray(poses), np.ascontiguousarray(points), np.ascontiguousarray(obs)


def batch_of(fx, B):
    if B == 1:
        return variant(fx, 0)
    return tuple(np.stack(a) for a in zip(*(variant(fx, v) for v in range(B))))


@pytest.mark.parametrize("fam,name", PROBES, ids=["%s-%s" % p for p in PROBES])
def test_probe_matches_the_model(contexts, fixtures, fam, name):
    kernels, _, tags, B = FAMILIES[fam]
    c, fx = contexts[B], fixtures[name]
    tol = {k: sm.gpu_tol(name, k) for k in sm.CAPS}
    c.set_tuning(ba_kernels=kernels)
    assert c.tuning()["ba_kernels"] == kernels
    c.ba_upload(*batch_of(fx, B))
    got = {}
    for tag in tags:
        r = fx["runs"][tag]
        got[tag] = c.ba_probe(lam=float(fx["lam"]), huber_delta=r["C"], loss=r["loss"])
    if fam == "rule":
        # the factored kernels really ran (tests/test_gpu_ba_factored.py's method): against the wave-private kernels on the same batch the camera
        # sums and the reduced system are formed in another order -- were the rule to launch k_ba_build_w after all, they would be bitwise equal
        c.set_tuning(ba_kernels=2)
        c.ba_upload(*batch_of(fx, B))
        for tag in tags:
            w = c.ba_probe(lam=float(fx["lam"]), huber_delta=fx["runs"][tag]["C"], loss=fx["runs"][tag]["loss"])
            assert not np.array_equal(got[tag]["Hpp"], w["Hpp"]) and not np.array_equal(got[tag]["S"], w["S"]), tag
    for tag in tags:
        for k in sm.CAPS:
            assert np.isfinite(got[tag][k]).all(), (tag, k)
    failed = []
    for tag in tags:                     # every run is printed before the first one is judged
        try:
            sm.check_probe(got[tag], fx["runs"][tag], tol, "%s %s %s:" % (fam, name, tag))
        except AssertionError as e:
            failed.append(e.args[0])
    assert not failed, failed


@pytest.mark.parametrize("loss", ["huber", "cauchy"])
@pytest.mark.parametrize("fam", list(FAMILIES))
def test_solve_costs_are_the_models(contexts, fixtures, fam, loss):
    kernels, _, _, B = FAMILIES[fam]
    c, fx = contexts[B], fixtures["A"]
    c.set_tuning(ba_kernels=kernels)
    K, poses, points, obs = batch_of(fx, B)
    po, pt, st = c.ba_adjust(K, poses, points, obs, c.ba_params(max_iters=8, loss=loss))
    if fam == "rule" and loss == "huber":
        # the factored kernels really ran in the solve too (the probe test's method): the wave-private kernels on the same batch form
        # their sums in another order -- were the rule to launch them after all, the solutions would be bitwise equal
        c.set_tuning(ba_kernels=2)
        qo, qt, qs = c.ba_adjust(K, poses, points, obs, c.ba_params(max_iters=8, loss=loss))
        print("rule against wave-private: poses differ by %.1e" % np.abs(po - qo).max(), [(s["iters"], s["accepted"], s["status"]) for s in qs])
        assert not np.array_equal(po, qo)
    if B == 1:
        K, obs, po, pt, st = K[None], obs[None], po[None], pt[None], [st]
    want0 = fx["runs"][loss]["cost"]
    failed = []
    for b in range(B):
        assert np.isfinite(po[b]).all() and np.isfinite(pt[b]).all() and np.isfinite([st[b]["cost"], st[b]["cost0"], st[b]["lam"]]).all(), b
        assert 1 <= st[b]["iters"] <= 8 and st[b]["n_obs"] == int((~np.isnan(obs[b][..., 0])).sum()), st[b]
        want = sm.cost_ld(K[b], po[b], pt[b], obs[b], loss, 1.0)
        d0, d1 = abs(st[b]["cost0"] - want0) / want0, abs(st[b]["cost"] - want) / want
        print("%s %s problem %d: iters %d accepted %d status %d  cost0 %.17g (model %.17g: %.1e / %.1e)  cost %.17g (longdouble at x %.17g: %.1e / 1e-12)"
              % (fam, loss, b, st[b]["iters"], st[b]["accepted"], st[b]["status"], st[b]["cost0"], want0, d0, sm.gpu_tol("A", "cost"), st[b]["cost"], want, d1))
        if not (d0 <= sm.gpu_tol("A", "cost") and d1 <= 1e-12 and st[b]["cost"] <= st[b]["cost0"]):
            failed.append((b, d0, d1, st[b]))
    assert not failed, failed
