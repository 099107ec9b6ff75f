"""CPU: the independent high-precision model of the BA linearisation and the SO(3) maps (tests/so3_model.py) against itself, against the
committed fixtures tests/golden/ba_so3_*.npz, and against the float64 code the GPU tests otherwise trust: oracle/ba_oracle.py and
vo_mi355x/so3.py.

The comparisons with the oracle MEASURE what the float64 oracle achieves against the model; the measured worst deviations are
recorded in so3_model.ORACLE_DEV / SO3_EXP_DEV / SO3_LOG_DEV and asserted here with a factor 2 of slack.  They are the baseline of every GPU
tolerance of tests/test_gpu_ba_so3.py and tests/test_gpu_pipe_fuzz.py (8 x, capped).  If the oracle missed 1e-10 on a block quantity or 1e-12
on a cost, the case would have to change, not the cap: the test asserts that too."""
import os

import numpy as np
import pytest

import so3_model as sm


def _axis_of(k):
    return sm.AXES[k % len(sm.AXES)]


def _rvecs():
    """(angle, rvec): the edge list and the log's own edges about axes k, k + 1, ...; the closed loop's angles about THEIR axes (axis k for angle k)"""
    out = [(th, th * _axis_of(k)) for k, th in enumerate(sm.EDGE_ANGLES + sm.LOG_ANGLES)]
    return out + [(th, th * sm.AXES[k]) for k, th in enumerate(sm.PIPE_ANGLES)]


def test_model_self_checks():
    """doubling the digits and dividing the difference step by 1e5 changes no float64 output by more than 1 ulp"""
    for name in ("A", "C"):          # A: the general K, the landmarks next to and behind a camera plane, 2 pi - 1e-3 and 7.5; every loss run
        worst = sm.self_check(name)
        print("%s: worst change %.2f ulp" % (name, worst))
        assert worst <= 1.0, name
    # exp and log at the edges: the same at twice the digits, and inverse to each other
    for th, r in _rvecs():
        R = sm.exp(r)
        assert sm.ulps(R, sm.exp(r, 2 * sm.DPS)) <= 1.0
        assert np.abs(R @ R.T - np.eye(3)).max() <= 4 * sm.EPS and abs(np.linalg.det(R) - 1) <= 4 * sm.EPS
        assert sm.ulps(sm.log(R), sm.log(R, 2 * sm.DPS)) <= 1.0
        # log(exp(r)) as a rotation: the float64 rounding of R moves the angle by ~ulp / sin th at most (acos' conditioning), ulp otherwise
        assert sm.rotation_distance(sm.log(R), r) <= 4 * sm.EPS / max(abs(np.sin(th)), 1e-8), th
    assert np.array_equal(sm.exp(np.zeros(3)), np.eye(3))


def test_cases_are_what_the_docstring_says():
    from vo_mi355x import synthetic as syn
    assert np.array_equal(sm.KITTI_K, syn.KITTI_K)
    assert np.abs(sm.AXES).min() >= 0.3 and np.allclose(np.linalg.norm(sm.AXES, axis=1), 1.0, atol=1e-15)
    for name, (W, N) in (("A", (10, 25)), ("B", (9, 13)), ("C", (4, 13)), ("D", (12, 25))):
        fx = sm.load(name)
        assert fx["obs"].shape == (W, N, 2)
        th = np.linalg.norm(fx["poses0"][:, :3], axis=1)
        small = fx["angles"] < 1e-3
        assert (np.abs(th[small] - fx["angles"][small]) <= 4 * sm.EPS * fx["angles"][small]).all()         # on the edge: no noise on these slots
        th2 = (fx["poses0"][:, :3] ** 2).sum(1)
        assert (th2[fx["angles"] == 9.9e-5] < 1e-8).all() and (th2[fx["angles"] == 9.9e-5] > 0).all()                       # the series side of the switch
        assert (th2[fx["angles"] == 1.01e-4] >= 1e-8).all()                                                                 # the closed-form side
        m = ~np.isnan(fx["obs"][..., 0])
        assert 0.05 < 1 - m.mean() < 0.25 and m.sum(0).min() >= 3 and m.sum(1).min() >= 3
        assert np.array_equal(fx["K"], sm.GENERAL_K if name in "AD" else sm.KITTI_K)
        if name in "AD":
            for (i, j, depth) in (sm.NEAR_PLANE, sm.BEHIND):
                zc = (sm.exp(fx["poses0"][i, :3]) @ fx["points0"][j] + fx["poses0"][i, 3:])[2]
                assert abs(zc - depth) <= 1e-12 and m[i, j], (name, i, j, zc)
    # float64 throughout; S per loss run is most of it (its upper triangles alone: 6 x (1830 + 1485 + 300 + 2628) doubles = 300 kB)
    assert sum(os.path.getsize(sm.path(n)) for n in sm.CASES) < 600e3 and max(os.path.getsize(sm.path(n)) for n in sm.CASES) < 256e3


@pytest.mark.parametrize("name", sm.CASES)
def test_fixture_regenerates_bit_for_bit(name):
    new = sm.build_fixture(name)
    with np.load(sm.path(name)) as z:
        assert sorted(z.files) == sorted(new)
        for k in z.files:
            a, b = z[k], np.asarray(new[k])
            assert a.dtype == np.float64 and a.shape == b.shape and np.array_equal(a, b, equal_nan=True), (name, k)


def test_exp_of_so3_and_of_the_oracle_against_the_model():
    import ba_oracle as bo
    from vo_mi355x import so3
    worst = 0.0
    for th, r in _rvecs():
        R = sm.exp(r)
        for f in (so3.rodrigues_vec_to_mat, bo.rodrigues_exp):
            worst = max(worst, np.abs(f(r) - R).max())
    print("exp: worst entry deviation %.2e (recorded %.2e)" % (worst, sm.SO3_EXP_DEV))
    assert worst <= 2 * sm.SO3_EXP_DEV


def measure_log():
    """so3.rodrigues_mat_to_vec against the exact log of the SAME float64 matrix, as a rotation angle -> {angle: deviation} outside the snap zones"""
    from vo_mi355x import so3
    out = {}
    for th, r in _rvecs():
        if abs(np.sin(th)) < 1.01e-5:
            continue
        R = sm.exp(r)
        out[th] = max(out.get(th, 0.0), sm.rotation_distance(so3.rodrigues_mat_to_vec(R), sm.log(R)))
    return out


def test_log_of_so3_outside_the_snap_zones():
    got = measure_log()
    print({("%.9g" % k): "%.2e" % v for k, v in got.items()})
    assert sorted(got) == sorted(sm.SO3_LOG_DEV)
    for th, d in got.items():
        assert d <= 2 * sm.SO3_LOG_DEV[th], (th, d)


def test_log_of_so3_inside_the_snap_zones():
    """OpenCV's rule for s = |sin th| < 1e-5: exactly zero below, the axis from the diagonal near pi -- within 2e-5 rad of the exact log"""
    from vo_mi355x import so3
    seen = 0
    for th, r in _rvecs():
        if abs(np.sin(th)) >= 0.99e-5:
            continue
        seen += 1
        R = sm.exp(r)
        r = so3.rodrigues_mat_to_vec(R)
        if th < 1e-5:
            assert np.array_equal(r, np.zeros(3)), th
        else:
            assert abs(th - np.pi) < 1e-5
            d = sm.rotation_distance(r, sm.log(R))
            print("th = pi - %.1e: %.2e rad from the exact log" % (np.pi - th, d))
            assert d <= 2e-5, (th, d)
    assert seen == 7          # 0, 1e-9, 1e-6 twice | pi - 1e-6 three times (edge list, log list, closed loop)


def measure_oracle(name):
    """worst deviation of oracle/ba_oracle.py from the fixture of case `name` over the six loss runs (the cost both through
    loss_normal_equations and through loss_cost), floored at one ulp -> {quantity: deviation, + e, Jp, Jl}"""
    import ba_oracle as bo
    fx = sm.load(name)
    K, poses, points, obs = fx["K"], fx["poses0"], fx["points0"], fx["obs"]
    e, Jp, Jl, m = bo.jacobian_blocks(K, poses, points, obs)
    assert np.array_equal(m, ~np.isnan(obs[..., 0]))
    worst = {"e": float(np.abs(e - fx["e"]).max() / np.abs(fx["e"]).max())}
    # Jacobians: every column of every slot relative to that column's largest entry
    worst["Jp"] = float((np.abs(Jp - fx["Jp"]).max(axis=(1, 2)) / np.abs(fx["Jp"]).max(axis=(1, 2))).max())
    worst["Jl"] = float((np.abs(Jl - fx["Jl"]).max(axis=(1, 2)) / np.abs(fx["Jl"]).max(axis=(1, 2))).max())
    for tag, r in fx["runs"].items():
        ne = bo.loss_normal_equations(K, poses, points, obs, r["loss"], r["C"])
        S, rhs, _, _, _ = bo.schur_system(ne, float(fx["lam"]))
        dp, dl, _ = bo.lm_step(ne, float(fx["lam"]))
        a = dict(ne, S=S, rhs=rhs, dposes=dp, dpoints=dl)
        b = dict(a, cost=bo.loss_cost(K, poses, points, obs, r["loss"], r["C"]))
        for got in (a, b):
            for k, v in sm.deviations(got, r).items():
                worst[k] = max(worst.get(k, 0.0), v)
    return {k: max(v, sm.EPS) for k, v in worst.items()}


def measure_helper(name):
    """the same for so3_model.mutant_probe WITHOUT a mutation: the float64 linearisation the mutants are made from has a table of its own
    (so3_model.HELPER_DEV); it sets no tolerance"""
    fx = sm.load(name)
    worst = {}
    for tag, r in fx["runs"].items():
        for k, v in sm.deviations(sm.mutant_probe(fx, r["loss"], r["C"], None, float(fx["lam"])), r).items():
            worst[k] = max(worst.get(k, sm.EPS), v)
    return worst


@pytest.mark.parametrize("name", sm.CASES)
def test_oracle_against_the_fixtures(name):
    got = measure_oracle(name)
    rec = sm.ORACLE_DEV[name]
    print(name, {k: "%.1e" % v for k, v in got.items()})
    for k, v in got.items():
        assert v <= 2 * rec[k], (name, k, v, rec[k])
    # the condition the cases were chosen under: the caps of the GPU tolerances are not what holds the device
    for k in sm.BLOCK_KEYS + ("Jp", "Jl", "e"):
        assert rec[k] <= 1e-10 / 8, (name, k)
    assert rec["cost"] <= 1e-12 / 8
    for k in sm.NORM_KEYS:
        assert 8 * rec[k] <= sm.CAPS[k]


@pytest.mark.parametrize("name", sm.CASES)
def test_helper_without_a_mutation_against_the_fixtures(name):
    got = measure_helper(name)
    print(name, {k: "%.1e" % v for k, v in got.items()})
    for k, v in got.items():
        assert v <= 2 * sm.HELPER_DEV[name][k] and sm.HELPER_DEV[name][k] <= 1e-11, (name, k, v)


@pytest.mark.parametrize("name", sm.CASES)
def test_mutants_fail_the_probe_comparison(name):
    """the comparison the device passes in tests/test_gpu_ba_so3.py (so3_model.check_probe at the same tolerances) rejects a float64 linearisation
    with the sign of Jr's a z term or of its b x y term wrong, or with R transposed, in every loss run of every case"""
    margins = sm.check_mutants(name)
    print(name, {k: "%.1e" % v for k, v in margins.items()})
    for k, v in margins.items():
        assert v >= sm.MUTANT_MARGIN[k] / 2, (name, k, v)


def test_cost_ld_is_the_models_cost():
    """numpy.longdouble against mpmath at x0 of every case and loss: the run-time yardstick of the solves' costs (1e-12) is itself good to 1e-15"""
    if np.finfo(np.longdouble).eps > 1.1e-19:
        pytest.fail("numpy.longdouble is not the 80-bit extended format here: cost_ld would be no better than the code under test")
    for name in sm.CASES:
        fx = sm.load(name)
        for tag, r in fx["runs"].items():
            c = sm.cost_ld(fx["K"], fx["poses0"], fx["points0"], fx["obs"], r["loss"], r["C"])
            assert abs(c - r["cost"]) <= 1e-15 * r["cost"], (name, tag, c, r["cost"])
