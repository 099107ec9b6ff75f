"""CPU-only: the numpy model of the Sim(3) search (tests/sim3_model.py) against its 40-digit truth, the factors of the bounds the GPU tests
use, and the proof that every problem of the GPU tests is `decided`, so that winner, counts and masks can be compared for equality.

kappa = s1 / (s2 + d3) of Sigma's signed singular values (sim3_model's header): the factors are measured here, on the model alone, over the
scene families general, planar, near_collinear, two_equal (two nearly equal singular values), mirrored, small_scale / large_scale (1e-3 and
1e3) and far_centroid (centroids 1e4 x the spread from the origin), with and without scale.  Every figure is printed before it is asserted."""
import math

import numpy as np
import pytest

import sim3_model as sm

SEEDS = (1, 2, 3)
N = 48


def _ratio(u, X, Y, with_scale):
    t = sm.truth(X, Y, with_scale)
    return sm.diff(u["m"], t, u["tscale"]) / (sm.EPS * u["kappa"])


@pytest.fixture(scope="module")
def measured():
    """family -> (worst ratio of solve3 over 24 triples per seed and scale mode, worst ratio of fit over the cloud and two subsets)"""
    out = {}
    for name in sm.FAMILIES:
        ws, wf, ns, nf = 0.0, 0.0, 0, 0
        for seed in SEEDS:
            s = sm.family(name, N, seed)
            X, Y = sm.widen(s["src"]), sm.widen(s["dst"])
            rng = np.random.default_rng([seed, 5])
            for with_scale in (True, False):
                for _ in range(24):
                    idx = rng.choice(N, 3, replace=False)
                    u = sm.solve3(X[idx], Y[idx], with_scale)
                    if u["m"] is None or not u["kappa"] <= sm.KAPPA_CUT:
                        continue
                    ws, ns = max(ws, _ratio(u, X[idx], Y[idx], with_scale)), ns + 1
                for mask in (None, np.arange(N) % 2 == 0, np.arange(N) < 7):
                    f = sm.fit(s["src"], s["dst"], mask, with_scale)
                    if f["m"] is None or not f["kappa"] <= sm.KAPPA_CUT:
                        continue
                    wf, nf = max(wf, _ratio(f, X[f["mask"]], Y[f["mask"]], with_scale)), nf + 1
        out[name] = (ws, ns, wf, nf)
    return out


def test_the_factors_are_four_times_the_measured_maxima(measured):
    for name, (ws, ns, wf, nf) in measured.items():
        print("%-15s solve3: worst |model - truth| / (2^-52 kappa) = %7.3f over %3d samples; fit: %7.3f over %2d sets (truth: %s)"
              % (name, ws, ns, wf, nf, sm.HP_NAME))
    ws, wf = max(v[0] for v in measured.values()), max(v[2] for v in measured.values())
    print("measured maxima: solve %.4g (recorded %.4g, SOLVE_FACTOR %g), refit %.4g (recorded %.4g, REFIT_FACTOR %g)"
          % (ws, sm.MEASURED["solve"], sm.SOLVE_FACTOR, wf, sm.MEASURED["refit"], sm.REFIT_FACTOR))
    assert all(v[1] >= 40 for k, v in measured.items()), "every family contributes samples"
    assert all(v[3] >= 2 for k, v in measured.items() if k != "mirrored"), "every family but the mirrored one contributes sets"
    assert ws <= sm.MEASURED["solve"] and wf <= sm.MEASURED["refit"]
    assert ws >= sm.MEASURED["solve"] / 2 and wf >= sm.MEASURED["refit"] / 2, "the record is the measurement, not a guess"
    assert sm.SOLVE_FACTOR == math.ceil(4 * sm.MEASURED["solve"]) and sm.REFIT_FACTOR == math.ceil(4 * sm.MEASURED["refit"])


def test_umeyama_recovers_the_true_transform_and_a_proper_rotation():
    for name in sm.FAMILIES:
        s = sm.family(name, N, 1)
        f = sm.fit(s["src"], s["dst"])
        assert f["m"] is not None, name
        sc, R, t = sm.unpack(f["m"])
        print("%-15s s %.6g (true %g), det R - 1 = %.3g, |R^T R - I| = %.3g, kappa %.3g" % (name, sc, s["s"], np.linalg.det(R) - 1,
                                                                                              np.abs(R.T @ R - np.eye(3)).max(), f["kappa"]))
        assert abs(np.linalg.det(R) - 1) <= 1e-12 and np.abs(R.T @ R - np.eye(3)).max() <= 1e-12
        if name != "mirrored":                                  # 1e-3 noise on a cloud 20 across (near_collinear: 0.02 thick)
            assert abs(sc - s["s"]) <= 1e-3 * s["s"] and np.abs(R - s["R"]).max() <= (5e-2 if name == "near_collinear" else 1e-3)
    # a three-point sample of a mirrored pair: rank 2, the determinant rule decides, and the three points are met exactly
    s = sm.family("mirrored", N, 2)
    X, Y = sm.widen(s["src"])[:3], sm.widen(s["dst"])[:3]
    u = sm.solve3(X, Y)
    assert abs(np.linalg.det(u["R"]) - 1) <= 1e-12 and sm.err(u["m"], X, Y).max() <= 1e-6 * s["s"] ** 2 * 100
    # without scale: s is exactly 1
    assert sm.fit(s["src"], s["dst"], None, False)["s"] == 1.0


def test_degenerate_samples_and_sets_have_no_model():
    a = np.array([[0.0, 0, 0], [1, 1, 1], [2, 2, 2]])
    b = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]])
    assert sm.solve3(a, b)["m"] is None and sm.solve3(b, a)["m"] is None and sm.solve3(b, b)["m"] is not None
    assert sm.solve3(np.array([[0.0, 0, 0], [0, 0, 0], [0, 1, 0]]), b)["m"] is None                   # coincident
    c = b.copy(); c[1, 1] = np.nan
    assert sm.solve3(c, b)["m"] is None and sm.solve3(b, c)["m"] is None
    line = np.stack([np.arange(6.0), np.zeros(6), np.zeros(6)], 1).astype(np.float32)
    assert sm.fit(line, line)["m"] is None and sm.fit(line[:2], line[:2])["m"] is None
    s = sm.collinear_consensus()
    f = sm.fit(s["src"], s["dst"], s["inliers"])
    print("collinear_consensus: scatter ratios %.3g, %.3g (tolerance %g)" % (f["ratios"] + (sm.DEGENERATE,)))
    assert f["m"] is None and not f["ambiguous"] and max(f["ratios"]) < sm.DEGENERATE / sm.AMBIGUOUS


def test_the_sampler_and_the_bound():
    assert sm.sample3(7, 0, 3) != sm.sample3(7, 1, 3) or sm.sample3(7, 0, 3) != sm.sample3(7, 2, 3)
    for h in range(50):
        i = sm.sample3(7, h, 5)
        assert len(set(i)) == 3 and all(0 <= k < 5 for k in i)
    assert sm.ransac_num_iters(0.99, 160 / 200) == 573 and sm.ransac_num_iters(0.99, 0.0) == 0 and sm.ransac_num_iters(0.99, 1.0) == 1000


_SEARCHES = {}


def searched(name):
    if name not in _SEARCHES:
        s, kw = sm.problems()[name]
        _SEARCHES[name] = (s, kw, sm.search(s["src"], s["dst"], **kw))
    return _SEARCHES[name]


@pytest.mark.parametrize("name", sorted(sm.problems()))
def test_every_gpu_problem_is_decided(name):
    s, kw, m = searched(name)
    fin = sm.finish(s["src"], s["dst"], m, 1, kw.get("with_scale", True))
    f = fin["fit"]
    print("%-20s n=%3d: best %4d of %4d hypotheses, %3d inliers (scene %3d), %3d degenerate, kappa %.3g, refit %d%s; decided %s %s"
          % (name, len(s["src"]), m["best"], m["hypotheses"], m["count"], int(s["inliers"].sum()), m["degenerate"], m["kappa"], fin["refit"],
             "" if f is None or f["m"] is None else " kappa %.3g" % f["kappa"], m["decided"], m["why"][:3]))
    assert m["decided"], m["why"]
    assert m["best"] >= 0 and m["count"] >= 3
    if f is not None:
        assert not f["ambiguous"], f["ratios"]
        if f["m"] is not None:
            assert f["kappa"] <= sm.KAPPA_CUT
    # no point's squared error within the rounding band of threshold^2, at the winner
    e = sm.err(m["m0"], s["src"], s["dst"])
    band = sm.err_band(m["m0"], s["src"], s["dst"], sm.SOLVE_FACTOR * sm.EPS * m["kappa"], m["tscale"])
    assert not np.any(np.abs(e - kw["thr"] ** 2) <= band)


def test_the_problems_take_the_paths_they_are_named_for():
    assert searched("n3")[2]["hypotheses"] == 256 and searched("n3")[2]["best"] == 0
    assert searched("rounds")[2]["hypotheses"] == 768 and searched("rounds")[2]["count"] == 40
    assert sm.ransac_num_iters(0.99, 160 / 200) == 573
    assert searched("capped")[2]["hypotheses"] == 256
    s, kw, m = searched("rigid_on_scale2")
    full = sm.search(s["src"], s["dst"], **dict(kw, with_scale=True))
    print("rigid_on_scale2: %d inliers without scale, %d with" % (m["count"], full["count"]))
    assert 3 <= m["count"] < full["count"]
    s, kw, m = searched("mirrored")
    assert m["count"] < len(s["src"]) // 2 and abs(np.linalg.det(sm.unpack(m["m0"])[1]) - 1) <= 1e-12
    s, kw, m = searched("collinear_consensus")
    fin = sm.finish(s["src"], s["dst"], m)
    assert fin["refit"] == 0 and m["count"] == 25 and sm.bits_equal(fin["m"], m["m0"])
    s, kw, m = searched("nan_rows")
    assert m["degenerate"] > 0 and not m["mask"][[5, 17, 40]].any()
    s, kw, m = searched("planar")
    assert sm.finish(s["src"], s["dst"], m)["refit"] == 1
    assert len({searched("batch%d" % i)[2]["hypotheses"] for i in range(3)}) >= 2
