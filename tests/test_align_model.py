"""CPU-only: the model of sparse direct image alignment (tests/align_model.py) against itself and against ground truth -- its Jacobian
against finite differences, the pose it finds on rendered frames with known motion, its parameters and degenerate rows, and the condition on
the inputs of tests/test_gpu_align.py: which of them the model alone decides.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import align_model as am


def _E(xi):
    return am.rodrigues(xi[3:]), np.asarray(xi[:3], np.float64)


def test_geometric_jacobian_against_finite_differences():
    rng = np.random.default_rng(5)
    K = np.array([[400.0, 0, 103.5], [0, 380.0, 59.5], [0, 0, 1]])
    X = np.stack([rng.uniform(-2, 2, 20), rng.uniform(-1, 1, 20), rng.uniform(4, 12, 20)], 1)
    worst = 0.0
    for l in (0, 1):
        J = am.jacobian(K, l, X)
        for k in range(6):
            h = 1e-6
            xi = np.zeros(6); xi[k] = h
            Rp, vp = _E(xi); Rm, vm = _E(-xi)
            fd = (am.project(K, l, X @ Rp.T + vp) - am.project(K, l, X @ Rm.T + vm)) / (2 * h)
            worst = max(worst, np.abs(fd - J[:, :, k]).max() / max(np.abs(J[:, :, k]).max(), 1.0))
    print("J_p against central differences of pi_l(E(xi) X): worst relative difference %.3g" % worst)
    # central differences at h = 1e-6 on coordinates of a few hundred pixels: truncation h^2, rounding 1e-16 x 400 / 1e-6 = 4e-8
    assert worst <= 1e-6


def test_photometric_jacobian_against_finite_differences_of_the_models_own_residual():
    # on an image that is linear in x and y bilinear sampling and central differences are exact, so the residual's derivative is -g J_p
    ys, xs = np.mgrid[0:60, 0:104].astype(np.float64)
    prev = 20.0 + 0.75 * xs + 1.5 * ys
    cur = prev + 3.0
    K = np.array([[200.0, 0, 51.75], [0, 190.0, 29.75], [0, 0, 1]])
    rng = np.random.default_rng(9)
    X = np.stack([rng.uniform(-1.0, 1.0, 12), rng.uniform(-0.5, 0.5, 12), rng.uniform(5, 9, 12)], 1)
    ref = am.reference(prev, K, 0, X)
    assert ref["ok"].all() and np.allclose(ref["gx"], 0.75) and np.allclose(ref["gy"], 1.5)
    lin = am.linearise(ref, cur, K, 0, np.eye(3), np.zeros(3), 0.0)
    assert np.allclose(lin["res"], 3.0) and lin["n_used"] == 12
    worst = 0.0
    for k in range(6):
        h = 1e-6
        xi = np.zeros(6); xi[k] = h
        r = []
        for s in (1, -1):
            R, v = _E(s * xi)
            moved = am.reference(prev, K, 0, X @ R.T + v)            # I_prev(pi(E(xi) X) + o)
            r.append(lin["res"] + ref["I"] - moved["I"])
        fd = (r[0] - r[1]) / (2 * h)                                # d r / d xi_k per pixel
        an = -(ref["gx"] * ref["J"][:, 0, k][:, None] + ref["gy"] * ref["J"][:, 1, k][:, None])
        worst = max(worst, np.abs(fd - an).max() / max(np.abs(an).max(), 1.0))
    print("-(gx J_p[0] + gy J_p[1]) against central differences of the residual: worst relative difference %.3g" % worst)
    assert worst <= 1e-5
    # and the normal equations are what those Jacobians sum to
    Jpix = ref["gx"][:, :, None] * ref["J"][:, None, 0, :] + ref["gy"][:, :, None] * ref["J"][:, None, 1, :]
    assert np.allclose(lin["H"], np.einsum("npi,npj->ij", Jpix, Jpix), rtol=1e-12) and np.allclose(lin["b"], np.einsum("npi,np->i", Jpix, lin["res"]), rtol=1e-12)


@pytest.mark.parametrize("n", [64, 128])
def test_pose_on_rendered_frames_is_within_a_tenth_of_the_image_motion(n):
    sc = am.scene(am.W, am.H)
    for seed in range(4):
        t = seed
        X = am.scene_points(sc, t, n, seed)
        P, C = am.pyramid(sc["frames"][t], am.LEVELS), am.pyramid(sc["frames"][t + 1], am.LEVELS)
        m = am.run(P, C, sc["K"], X, huber=10.0)
        motion, err = am.prediction_error(sc["K"], X, m["R"], m["t"], *am.true_pose(sc, t))
        print("n %d seed %d pair %d: median image motion %.3f px, median prediction error %.4f px (1/%.0f), iters %s, chi %.2f"
              % (n, seed, t, motion, err, motion / err, m["iters"][:2], m["chi2"]))
        assert m["status"] == 0 and m["levels_run"] == 2 and err <= motion / 10.0


def _case(name):
    (c,) = [c for c in am.gpu_cases() if c["name"] == name]
    return c, am.case_runs(c)[0]


def test_parameters_behave_as_specified():
    sc = am.scene(am.W, am.H)
    c, m = _case("huber0")
    P, C = am.pyramid(sc["frames"][c["t"]], am.LEVELS), am.pyramid(sc["frames"][c["t"] + 1], am.LEVELS)
    ref = am.reference(P[0], c["K"], 0, c["X"].astype(np.float64))
    l0, l10 = am.linearise(ref, C[0], c["K"], 0, np.eye(3), np.zeros(3), 0.0), am.linearise(ref, C[0], c["K"], 0, np.eye(3), np.zeros(3), 10.0)
    big = np.abs(l0["res"]) > 10.0
    assert (l0["w"] == 1.0).all() and big.any() and np.allclose(l10["w"][big], 10.0 / np.abs(l10["res"][big])) and (l10["w"][~big] == 1.0).all()
    assert l10["chi"] < l0["chi"]
    c, m = _case("min_level1")
    assert m["iters"][0] == 0 and m["iters"][1] > 0 and m["levels_run"] == 1
    c, m = _case("max_iters1")
    assert list(m["iters"][:2]) == [1, 1] and m["levels_run"] == 2
    # an initial pose: starting at the truth the first linearisation of the top level already has the small residual, and the result stays there
    c, m = _case("n64")
    Rt, tt = am.true_pose(sc, c["t"])
    P, C = am.pyramid(sc["frames"][c["t"]], am.LEVELS), am.pyramid(sc["frames"][c["t"] + 1], am.LEVELS)
    m2 = am.run(P, C, c["K"], c["X"], am.log_so3(Rt), tt)
    d = am.displacement(c["K"], c["X"], m2["R"], m2["t"], Rt, tt)
    print("started at the truth: ends %.3f px from it (largest displacement), from identity %.3f px" % (d, am.displacement(c["K"], c["X"], m["R"], m["t"], Rt, tt)))
    assert d <= 1.0 and m2["status"] == 0
    c, m = _case("init_pose")
    assert m["status"] == 0 and m["levels_run"] == 2


def test_degenerate_rows_and_too_few_points():
    c, m = _case("nan_and_behind")
    X = c["X"]
    bad = ~(np.isfinite(X).all(1) & (X[:, 2] > 0))
    print("nan_and_behind: %d of %d rows are NaN or not in front; used %d" % (bad.sum(), len(X), m["n_used"]))
    assert bad.sum() == 17 and not m["used"][bad].any() and m["n_used"] == int(m["used"].sum()) == len(X) - 17 and m["status"] == 0
    # the same rows alone give the same pose: the bad rows contribute nothing
    sc = am.scene(am.W, am.H)
    P, C = am.pyramid(sc["frames"][c["t"]], am.LEVELS), am.pyramid(sc["frames"][c["t"] + 1], am.LEVELS)
    m2 = am.run(P, C, c["K"], X[~bad])
    assert am.displacement(c["K"], X, m["R"], m["t"], m2["R"], m2["t"]) <= 1e-9
    c, m = _case("n9")
    assert m["status"] == am.VO_E_NUMERIC and list(m["iters"][:2]) == [-1, -1] and m["levels_run"] == 0 and not m["used"].any()
    assert np.array_equal(m["rvec"], c["rvec0"]) and np.array_equal(m["tvec"], c["tvec0"])
    # points that leave the interior while the level iterates: the count of used points changes from one pass to a later one
    for name in ("leaving", "leaving_n200"):
        c, m = _case(name)
        counts = [v for k, v, _ in m["margins"] if k == "min_points"]
        print(name, "used per pass:", counts)
        assert len(set(counts)) > 1 and m["n_used"] < len(c["X"])


def test_the_gpu_tests_inputs_are_decided_by_the_model_alone():
    cases = am.gpu_cases()
    dec = []
    for c in cases:
        a, b = am.case_runs(c)
        dec.append(am.decided(a, b))
        print("%-16s n %3d iters %s n_used %3d decided %s; float32 switch moves the pose by %.3g px"
              % (c["name"], len(c["X"]), a["iters"][:2], a["n_used"], dec[-1], am.displacement(c["K"], c["X"], a["R"], a["t"], b["R"], b["t"])))
    assert {len(c["X"]) for c in cases} >= {9, 10, 17, 64, 200}
    assert sum(dec) >= 0.8 * len(cases), dec
