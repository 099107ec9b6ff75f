"""CPU-only: the fundamental-matrix model of tests/fundamental_model.py against brute-force loops, its own longdouble truths and the scenes'
ground truths -- and the place where every constant the GPU test uses is measured (on the model alone) and checked against what the model
file records, and where every problem of the GPU test is shown to be decided.  Run with -s to see the figures."""
import itertools
import math

import numpy as np
import pytest

import essential_model as em
import fundamental_model as fm
import homography_model as hm

_CACHE = {}


def _searched(name, n):
    """(scene, the model's whole search on it with the search seed the GPU test uses), computed once"""
    if (name, n) not in _CACHE:
        s = fm.scene(name, n)
        _CACHE[(name, n)] = (s, fm.search(s["p1"], s["p2"], seed=fm.full_search_seed(name, n)))
    return _CACHE[(name, n)]


def _exact_points(s):
    """the scene's projections in float64, before the float32 rounding of its p1, p2"""
    p1 = s["X"] @ s["K"].T
    p2 = (s["X"] @ s["R"].T + s["t"]) @ s["K"].T
    return p1[:, :2] / p1[:, 2:3], p2[:, :2] / p2[:, 2:3]


# ---- the pieces ------------------------------------------------------------------------------------------------------------------------------
def test_sample7_is_the_documented_generator():
    for seed, h, n in itertools.product((0, 7, 123456789), (0, 1, 255, 256, 70000), (7, 8, 40, 200, 100000)):
        idx = fm.sample7(seed, h, n)
        assert len(set(idx)) == 7 and all(0 <= i < n for i in idx)
        assert idx[:4] == hm.sample4(seed, h, n)                 # the same draws as the other searches, three more of them
    assert sorted(fm.sample7(3, 9, 7)) == list(range(7))


def test_ransac_num_iters_at_its_edges():
    assert fm.ransac_num_iters(0.99, 0.0) == 0                                 # every point an inlier: the first round is the last
    assert fm.ransac_num_iters(0.99, 1.0) == fm.MAX_ITERS
    assert fm.ransac_num_iters(0.99, 0.5) == round(math.log(0.01) / math.log(1 - 0.5 ** 7)) == 587
    assert fm.ransac_num_iters(0.99, 0.3) == round(math.log(0.01) / math.log(1 - 0.7 ** 7)) == 54
    assert fm.ransac_num_iters(0.99, 0.9) == fm.MAX_ITERS                      # ln 0.01 / ln(1 - 1e-7) = 4.6e7 > 1000
    assert fm.ransac_num_iters(0.99, 0.5, max_iters=500) == 500
    assert fm.ransac_num_iters(1.0, 0.5) == fm.MAX_ITERS                       # confidence 1: 1 - p is clamped to the smallest double


def test_seven_point_returns_the_true_F_among_one_or_three_roots():
    """on the scenes' float64 projections (no float32 rounding) the ground truth is a root: within the bound every solve is held to"""
    worst, n_roots = 0.0, {1: 0, 3: 0}
    for name in fm.EXACT + ("small_baseline",):
        s = fm.scene(name, 40)
        p1, p2 = _exact_points(s)
        gt = fm.ground_truth(s)
        for h in range(32):
            idx = fm.sample7(fm.SEARCH_SEED, h, 40)
            m = fm.seven_point(p1[idx], p2[idx])
            if name == "plane_off" and not m["models"]:                # seven points of the plane itself: a third null dimension
                assert m["rank"] <= fm.RANK_TOL / fm.AMBIGUOUS, (h, m["rank"])
                continue
            assert len(m["models"]) in (1, 3), (name, h, len(m["models"]))
            n_roots[len(m["models"])] += 1
            d, kap = min((fm.same_F(r["F"], gt), r["kappa"]) for r in m["models"])
            if kap <= fm.KAPPA_CUT:
                worst = max(worst, d / (fm.EPS * kap))
                assert d <= fm.SOLVE_FACTOR * fm.EPS * kap, (name, h, d, kap)
    print("fundamental model: |nearest root - F_gt| / (2^-52 kappa) at most %.3g (bound %g); samples with 1 / 3 roots: %d / %d"
          % (worst, fm.SOLVE_FACTOR, n_roots[1], n_roots[3]))
    assert n_roots[1] > 0 and n_roots[3] > 0


def test_degenerate_samples_have_no_model():
    s = fm.scene("general", 7, 1)
    p1, p2 = hm.widen(s["p1"]), hm.widen(s["p2"])
    assert len(fm.seven_point(p1, p2)["models"]) in (1, 3)
    q1, q2 = p1.copy(), p2.copy()
    q1[4], q2[4] = q1[1], q2[1]                                             # a repeated correspondence: six equations
    m = fm.seven_point(q1, q2)
    assert m["models"] == [] and m["rank"] <= fm.RANK_TOL / fm.AMBIGUOUS and not m["ambiguous"], m
    x = 100.0 + 140 * np.arange(7)
    line = np.stack([x, x // 5 + 40], 1)                                    # exactly on a line
    for a, b in ((line, line + [5.0, 1.0]), (line, line[::-1] * [1.0, 0.5])):
        m = fm.seven_point(a, b)
        assert m["models"] == [] and m["rank"] <= fm.RANK_TOL / fm.AMBIGUOUS, m
    q1 = p1.copy(); q1[2, 0] = np.nan
    assert fm.seven_point(q1, p2)["models"] == []


def test_err_is_the_distance_to_the_epipolar_line():
    s = fm.scene("general", 40)
    F = fm.ground_truth(s)
    p1, p2 = s["p1"].astype(np.float64), s["p2"].astype(np.float64)
    e, rounding = fm.err(F, s["p1"], s["p2"]), fm.err_band(F, s["p1"], s["p2"], 0.0)
    for i in range(40):
        l2, l1 = F @ [p1[i, 0], p1[i, 1], 1.0], F.T @ [p2[i, 0], p2[i, 1], 1.0]
        d2 = (l2 @ [p2[i, 0], p2[i, 1], 1.0]) ** 2 / (l2[0] ** 2 + l2[1] ** 2)
        d1 = (l1 @ [p1[i, 0], p1[i, 1], 1.0]) ** 2 / (l1[0] ** 2 + l1[1] ** 2)
        assert abs(e[i] - max(d1, d2)) <= rounding[i]                          # another order of the same sums: the rounding part of the band
    assert e.max() <= 1e-6                                                   # float32 rounding of a pixel: (2^-13 px)^2 at most
    q1, q2 = s["p1"].copy(), s["p2"].copy()
    q1[3] = np.nan; q2[5, 1] = np.nan
    m = fm.consensus(F, q1, q2)
    assert not m[3] and not m[5] and m.sum() == 38
    Z = np.zeros((3, 3)); Z[2, 2] = 1.0                                      # every epipolar line has a = b = 0
    assert not fm.consensus(Z, s["p1"], s["p2"]).any() and np.isinf(fm.err(Z, s["p1"], s["p2"])).all()
    # the band: moving every entry of F by delta never moves err by more than err_band says
    rng = np.random.default_rng(5)
    for delta in (1e-14, 1e-11):
        band = fm.err_band(F, s["p1"], s["p2"], delta)
        for _ in range(20):
            e2 = fm.err(F + delta * rng.choice([-1.0, 1.0], (3, 3)), s["p1"], s["p2"])
            assert np.all(np.abs(e2 - e) <= band)


def test_search_against_loops_and_the_planted_outliers():
    for n in (40, 200):
        s = fm.with_outliers("general", n, 0.3, 5)
        r = fm.search(s["p1"], s["p2"], seed=fm.SEARCH_SEED)
        truth = np.ones(n, bool)
        truth[s["outliers"]] = False
        leak = int((r["mask"] & ~truth).sum())
        print("fundamental model general+30%% n=%d: best %d of %d hypotheses, %d inliers of %d true, %d planted outliers among them (bound %.1f)"
              % (n, r["best"], r["hypotheses"], r["count"], truth.sum(), leak, em.outlier_leak(n)))
        assert np.all(r["mask"][truth]) and leak <= em.outlier_leak(n)       # the ground-truth inlier set, up to outliers that fell on their line
        # the winner restated with loops
        best, best_count, models = -1, 6, 0
        for h in range(r["hypotheses"]):
            idx = fm.sample7(fm.SEARCH_SEED, h, n)
            top = None
            for m in fm.seven_point(hm.widen(s["p1"])[idx], hm.widen(s["p2"])[idx])["models"]:
                models += 1
                e = fm.err(m["F"], s["p1"], s["p2"])
                key = (-int((e <= 9.0).sum()), float(e[e <= 9.0].sum()))
                top = key if top is None or key < top else top
            if top is not None and -top[0] > best_count:
                best, best_count = h, -top[0]
        assert (best, best_count, models) == (r["best"], r["count"], r["models"])
        assert r["hypotheses"] == hm.BATCH * -(-max(1, fm.ransac_num_iters(fm.CONFIDENCE, (n - best_count) / n)) // hm.BATCH)


# ---- the measured constants ------------------------------------------------------------------------------------------------------------------
def _fresh_ok(name, worst, factor):
    print("fundamental model: %s worst ratio %.4g (recorded %.4g), x 8 = %.4g, factor %.4g" % (name, worst, fm.MEASURED[name], 8 * worst, factor))
    assert 8 * fm.MEASURED[name] <= factor <= 8.5 * fm.MEASURED[name], (name, factor)       # the factor is 8 x the record, rounded up
    # the fresh measurement against the record: equal on the LAPACK build it was taken with; another build rounds the worst of several
    # thousand samples differently, so a factor of two either way is allowed before the record counts as stale
    assert 0.5 * fm.MEASURED[name] <= worst <= 2 * fm.MEASURED[name], (name, worst)


def test_seven_point_against_its_longdouble_truth_meets_its_points_and_has_rank_two():
    worst, n_all, n_cut, kappas, worst_meet, worst_det = 0.0, 0, 0, [], 0.0, 0.0
    for name in fm.SCENES:
        for n in fm.FULL_NS:
            s = fm.scene(name, n)
            P1, P2 = hm.widen(s["p1"]), hm.widen(s["p2"])
            for h in range(fm.BATCH):
                idx = fm.sample7(fm.SEARCH_SEED, h, n)
                for m in fm.seven_point(P1[idx], P2[idx], truth=True)["models"]:
                    n_all += 1
                    kappas.append(m["kappa"])
                    assert abs(np.linalg.norm(m["F"]) - 1) <= 4 * fm.EPS and m["F"].reshape(9)[np.argmax(np.abs(m["F"]))] > 0
                    if m["kappa"] > fm.KAPPA_CUT:
                        n_cut += 1
                        continue
                    worst = max(worst, m["ratio"])
                    # the longdouble root meets its seven points and has det 0; this F lies within delta of it, so each point lies within
                    # err_band(delta) of its line and sigma3 within 3 delta of 0.  delta is the bound itself: 8 x the measured difference
                    delta = fm.SOLVE_FACTOR * fm.EPS * m["kappa"]
                    e, band = fm.err(m["F"], P1[idx], P2[idx]), fm.err_band(m["F"], P1[idx], P2[idx], delta)
                    assert np.all(e <= band), (name, n, h, e, band)
                    s3 = fm.sigma3_rel(m["F"])
                    assert s3 <= 3 * delta / np.linalg.svd(m["F"], compute_uv=False)[0], (name, n, h, s3)
                    worst_meet = max(worst_meet, float((e / band).max()))
                    worst_det = max(worst_det, s3 / (3 * delta))
    print("fundamental model: %d models of the first-round samples, %d over KAPPA_CUT; kappa median %.3g, 99th centile %.3g, max %.3g; "
          "err at the seven points at most %.3g of its bound, sigma3 / sigma1 at most %.3g of its bound"
          % (n_all, n_cut, np.median(kappas), np.percentile(kappas, 99), max(kappas), worst_meet, worst_det))
    _fresh_ok("solve", worst, fm.SOLVE_FACTOR)


def test_eight_point_against_truth_and_ground_truth():
    worst = dict(refit=0.0, gt=0.0, rank2=0.0)
    for name in fm.SCENES:
        for n in fm.FULL_NS:
            s, r = _searched(name, n)
            f = fm.eight_point(s["p1"], s["p2"], r["mask"], truth=True)
            worst["refit"] = max(worst["refit"], f["ratio_eigh"])
            worst["rank2"] = max(worst["rank2"], fm.sigma3_rel(f["F_eigh"]) / fm.EPS)
            assert fm.same_F(f["F"], f["F_eigh"]) <= fm.REFIT_FACTOR * fm.EPS * f["kappa2"]       # the two routes of the model agree
            line = "fundamental model %-14s n=%3d: best %4d, %4d hypotheses, %3d inliers; kappa2 %.3g, kappa8 %.3g, cost %.3g px^2" \
                % (name, n, r["best"], r["hypotheses"], r["count"], f["kappa2"], f["kappa8"], fm.cost(f["F_eigh"], s["p1"], s["p2"], r["mask"]))
            if name in fm.EXACT:
                assert r["count"] == n and r["hypotheses"] == fm.BATCH, (name, n, r["count"])
                g = fm.judge_gt(f["F_eigh"], s, f["kappa8"])
                worst["gt"] = max(worst["gt"], g["ratio"])
                assert fm.err(fm.ground_truth(s), s["p1"], s["p2"]).max() <= 1e-6               # the truth holds every point to float32 rounding
                assert fm.err(f["F_eigh"], s["p1"], s["p2"]).max() <= 1e-6                      # and so does the re-fit
            print(line)
    for k in ("refit", "gt", "rank2"):
        _fresh_ok(k, worst[k], dict(refit=fm.REFIT_FACTOR, gt=fm.GT_FACTOR, rank2=fm.RANK2_FACTOR)[k])


# ---- every problem of the GPU test is decided ------------------------------------------------------------------------------------------------
def _decided(tag, s, r):
    print("fundamental model %-22s: best %3d of %4d hypotheses, %3d inliers, %d roots, %4d models, kappa %.3g, tie margin %.3g, decided %s %s"
          % (tag, r["best"], r["hypotheses"], r["count"], r["n_roots"], r["models"], r["kappa"], r["tie_margin"], r["decided"], r["why"][:2]))
    assert r["decided"] and r["best"] >= 0 and r["kappa"] <= 0.1 * fm.KAPPA_CUT, (tag, r["why"], r["kappa"])
    assert r["tie_margin"] > 1e-6


@pytest.mark.parametrize("n", fm.FULL_NS)
@pytest.mark.parametrize("name", fm.SCENES)
def test_full_problems_are_decided(name, n):
    s, r = _searched(name, n)
    _decided("%s n=%d" % (name, n), s, r)
    band = fm.err_band(r["F0"], s["p1"], s["p2"], fm.SOLVE_FACTOR * fm.EPS * r["kappa"])
    e = fm.err(r["F0"], s["p1"], s["p2"])
    assert not np.any(np.abs(e - fm.THRESHOLD ** 2) <= band)                  # no point within the rounding band of the threshold


@pytest.mark.parametrize("n", fm.EDGE_NS[1:])
def test_loop_edge_problems_are_decided(n):
    s = fm.edge_scene(n)
    _decided(s["name"] + " n=%d" % n, s, fm.search(s["p1"], s["p2"], seed=fm.SEARCH_SEED))


def test_batch_problems_are_decided_and_stop_in_different_rounds():
    rounds = []
    for s in fm.batch_scenes():
        r = fm.search(s["p1"], s["p2"], seed=fm.SEARCH_SEED)
        _decided(s["name"], s, r)
        rounds.append(r["hypotheses"])
    assert tuple(rounds) == fm.BATCH_ROUNDS


def test_the_tie_problem_is_decided_by_the_sum_of_err():
    s = fm.tie_scene()
    r = fm.search(s["p1"], s["p2"], seed=fm.SEARCH_SEED)
    _decided("tie n=8", s, r)
    assert r["count"] == 8 and r["n_roots"] == 3 and 1e-6 < r["tie_margin"] < 1.0, r["tie_margin"]     # two roots hold all eight points


def test_the_two_seed_problem_has_one_consensus_set():
    s = fm.with_outliers("general", 200, 0.3, fm.TWO_SEEDS_SCENE_SEED)
    a, b = fm.search(s["p1"], s["p2"], seed=3), fm.search(s["p1"], s["p2"], seed=4)
    _decided("two seeds, seed 3", s, a)
    _decided("two seeds, seed 4", s, b)
    assert a["best"] != b["best"] and np.array_equal(a["mask"], b["mask"])
