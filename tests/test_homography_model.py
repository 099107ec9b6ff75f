"""CPU-only: the homography model of tests/homography_model.py against brute-force loops, its own longdouble truths and the scenes' ground
truths -- and the place where every constant the GPU test uses is measured (on the model alone) and checked against what the model file
records.  Run with -s to see the figures."""
import itertools
import math

import numpy as np
import pytest

import essential_model as em
import homography_model as hm

NS = (40, 200)
_CACHE = {}


def _scene(name, n):
    return hm.planar_noisy(n) if name == "plane+noise" else hm.scene(name, n, hm.FULL_SEED)


def _searched(name, n, thr=hm.THRESHOLD):
    """(scene, the model's whole search on it), computed once"""
    key = (name, n, thr)
    if key not in _CACHE:
        s = _scene(name, n)
        _CACHE[key] = (s, hm.search(s["p1"], s["p2"], thr=thr, seed=hm.SEARCH_SEED))
    return _CACHE[key]


# ---- the pieces against brute force --------------------------------------------------------------------------------------------------------
def test_sample4_is_the_documented_generator():
    import pnp_oracle as po                                  # the 3D-2D search draws from the same generator
    for seed, h, n in itertools.product((0, 7, 123456789), (0, 1, 255, 256, 70000), (4, 5, 40, 200, 100000)):
        idx = hm.sample4(seed, h, n)
        assert len(set(idx)) == 4 and all(0 <= i < n for i in idx)
        assert idx == list(po.sample4(seed, h, n))
    assert sorted(hm.sample4(3, 9, 4)) == [0, 1, 2, 3]


def test_check_subset_on_hand_made_quads():
    sq = np.array([[0.0, 0], [10, 0], [10, 10], [0, 10]])
    assert hm.check_subset(sq, sq + 5.0)
    assert hm.check_subset(sq, sq * [-1.0, 1.0])                               # a mirror image reverses all four orientations: kept
    bow = sq[[0, 1, 3, 2]]                                                     # two vertices exchanged: two triples flip, two do not
    assert not hm.check_subset(sq, bow)
    inside = np.array([[0.0, 0], [10, 0], [5, 10], [5, 3]])                    # the fourth point moved across an edge of the triangle
    across = inside.copy(); across[3] = [5, -3]
    assert not hm.check_subset(inside, across)
    for view in (0, 1):
        for trip in itertools.combinations(range(4), 3):                       # any three collinear, in either view
            q = np.array([[0.0, 0], [10, 1], [3, 7], [8, 12]])
            a, b, c = trip
            q[c] = q[a] + 0.4 * (q[b] - q[a])
            pair = (q, sq) if view == 0 else (sq, q)
            assert not hm.check_subset(*pair), (view, trip)
    twice = sq.copy(); twice[2] = twice[0]                                     # a repeated point is collinear with every other
    assert not hm.check_subset(twice, sq)
    # the threshold itself: FLT_EPSILON x the L1 size of the two edges
    near = np.array([[0.0, 0], [100, 0], [50, 0.5 * hm.FLT_EPSILON], [20, 80]])      # |cross| = 100 y against FLT_EPSILON x (100 + 2 y)
    assert not hm.check_subset(near, near + 3.0)
    near[2, 1] = 8 * hm.FLT_EPSILON
    assert hm.check_subset(near, near + 3.0)


def test_ransac_num_iters_hand_values():
    assert hm.ransac_num_iters(0.995, 0.0) == 0                                # every point an inlier: the first round is the last
    assert hm.ransac_num_iters(0.995, 1.0) == hm.MAX_ITERS
    assert hm.ransac_num_iters(0.995, 0.5) == 82                               # ln 0.005 / ln(1 - 0.5^4) = -5.2983 / -0.064539 = 82.09
    assert hm.ransac_num_iters(0.995, 0.9) == hm.MAX_ITERS                     # ln 0.005 / ln(1 - 1e-4) = 52981 > 2000
    assert hm.ransac_num_iters(0.995, 0.25) == round(math.log(0.005) / math.log(1 - 0.75 ** 4)) == 14
    assert hm.hypotheses_bounds(200, 200) == (0, 2048) and hm.hypotheses_bounds(200, 100) == (82, 2048)


def test_consensus_and_search_against_loops():
    s, r = _searched("general", 40)
    n = 40
    p1, p2 = s["p1"].astype(np.float64), s["p2"].astype(np.float64)
    best, best_count, counts = -1, 3, []
    for h in range(r["hypotheses"]):
        idx = hm.sample4(hm.SEARCH_SEED, h, n)
        cnt = -1
        if hm.check_subset(p1[idx], p2[idx]):
            H = hm.four_point(p1[idx], p2[idx])["H"]
            if H is not None:
                cnt = 0
                for i in range(n):                                             # the forward transfer error, point by point
                    x = H @ np.array([p1[i, 0], p1[i, 1], 1.0])
                    if x[2] != 0 and math.isfinite(x[2]) and math.hypot(p2[i, 0] - x[0] / x[2], p2[i, 1] - x[1] / x[2]) <= hm.THRESHOLD:
                        cnt += 1
        counts.append(cnt)
        if cnt > best_count:
            best, best_count = h, cnt
    assert counts == r["counts"] and (best, best_count) == (r["best"], r["count"])
    assert int(r["mask"].sum()) == r["count"] >= 4
    # the stopping rule: the round that ended the search is the first whose bound was met
    rounds = r["hypotheses"] // hm.BATCH
    for k in range(1, rounds + 1):
        top = max(counts[:k * hm.BATCH])
        need = min(hm.MAX_ITERS, hm.ransac_num_iters(hm.CONFIDENCE, (n - top) / n)) if top >= 4 else hm.MAX_ITERS
        assert (k * hm.BATCH >= need) == (k == rounds), (k, need)
    # special rows
    H = r["H0"]
    q1, q2 = s["p1"].copy(), s["p2"].copy()
    q1[3] = np.nan; q2[5, 1] = np.nan
    m, _ = hm.consensus(H, q1, q2)
    assert not m[3] and not m[5] and np.array_equal(np.delete(m, [3, 5]), np.delete(r["mask"], [3, 5]))
    Hinf = np.array([[1.0, 0, 0], [0, 1, 0], [0, 0, 0]])                       # w = 0 everywhere
    assert not hm.consensus(Hinf, s["p1"], s["p2"])[0].any()


# ---- the measured constants ----------------------------------------------------------------------------------------------------------------
def _fresh_ok(name, worst, factor):
    print("homography model: %s worst ratio %.4g (recorded %.4g), x 8 = %.4g, factor %.4g" % (name, worst, hm.MEASURED[name], 8 * worst, factor))
    assert 8 * hm.MEASURED[name] <= factor <= 8.5 * hm.MEASURED[name], (name, factor)       # the factor is 8 x the record, rounded up
    # the fresh measurement against the record: equal on the LAPACK build it was taken with; another build rounds the worst of several
    # thousand samples differently, so a factor of two either way is allowed before the record counts as stale
    assert 0.5 * hm.MEASURED[name] <= worst <= 2 * hm.MEASURED[name], (name, worst)


def test_four_point_solve_against_its_longdouble_truth():
    worst, n_all, n_cut, kappas = 0.0, 0, 0, []
    for name in hm.SCENES:
        for n in NS:
            s = _scene(name, n)
            P1, P2 = hm.widen(s["p1"]), hm.widen(s["p2"])
            for h in range(hm.BATCH):
                idx = hm.sample4(hm.SEARCH_SEED, h, n)
                if not hm.check_subset(P1[idx], P2[idx]):
                    continue
                m = hm.four_point(P1[idx], P2[idx], truth=True)
                if m["H"] is None:
                    continue
                n_all += 1
                kappas.append(m["kappa"])
                if m["kappa"] > hm.KAPPA_CUT:
                    n_cut += 1
                    continue
                worst = max(worst, m["ratio"])
                assert abs(np.linalg.norm(m["H"]) - 1) <= 4 * hm.EPS and m["H"][2, 2] >= 0
    for name, seed in hm.MINIMAL_SETS:                       # the n = 4 problems of the GPU test
        s = hm.scene(name, 4, seed)
        assert hm.check_subset(hm.widen(s["p1"]), hm.widen(s["p2"])), (name, seed)
        m = hm.four_point(hm.widen(s["p1"]), hm.widen(s["p2"]), truth=True)
        assert m["kappa"] <= hm.KAPPA_CUT, (name, seed, m["kappa"])
        worst = max(worst, m["ratio"])
        assert hm.transfer_px(m["H"], s["p1"], s["p2"]).max() <= 1e-9 * m["kappa"]       # the solve interpolates its four points
    print("homography model: %d first-round samples, %d over KAPPA_CUT; kappa median %.3g, 99th centile %.3g, max %.3g"
          % (n_all, n_cut, np.median(kappas), np.percentile(kappas, 99), max(kappas)))
    _fresh_ok("solve", worst, hm.SOLVE_FACTOR)
    assert n_cut <= 0.01 * n_all


def test_refit_and_refinement_against_truth_and_ground_truth():
    worst = dict(refine=0.0, dlt=0.0, cost=0.0, gt=0.0)
    for name in hm.SCENES + ("plane+noise",):
        for n in NS:
            s, r = _searched(name, n)
            f = hm.refine(s["p1"], s["p2"], r["mask"], truth=True)
            d = hm.refit(s["p1"], s["p2"], r["mask"], truth=True)
            worst["refine"] = max(worst["refine"], f["ratio"])
            worst["dlt"] = max(worst["dlt"], d["ratio_eigh"])
            worst["cost"] = max(worst["cost"], f["cost_ratio"])
            assert hm.same_H(d["H"], d["H_eigh"]) <= hm.DLT_FACTOR * hm.EPS * d["kappa2"]      # the two routes of the model agree
            assert f["cost"] <= float(hm.cost_px(d["H"], s["p1"], s["p2"], r["mask"])) * (1 + 1e-12)     # refining never costs
            line = "homography model %-14s n=%3d: best %4d, %4d hypotheses, %3d inliers; refine %d steps, kappa %.3g, cost %.3g px^2" \
                % (name, n, r["best"], r["hypotheses"], r["count"], f["iters"], f["kappa"], f["cost"])
            if name in hm.EXACT:
                assert r["count"] == n and r["hypotheses"] == hm.BATCH, (name, n, r["count"])
                g = hm.judge_gt(f["H"], s, f["kappa"])
                worst["gt"] = max(worst["gt"], g["ratio"])
                assert hm.transfer_px(hm.ground_truth(s), s["p1"], s["p2"]).max() <= 1e-3     # the truth holds every point to float32 rounding
                assert hm.transfer_px(f["H"], s["p1"], s["p2"]).max() <= 1e-4                 # and so does the re-fit (the issue's table)
                line += "; worst transfer error %.2e px" % hm.transfer_px(f["H"], s["p1"], s["p2"]).max()
            print(line)
    for k in ("refine", "dlt", "cost", "gt"):
        _fresh_ok(k, worst[k], dict(refine=hm.REFINE_FACTOR, dlt=hm.DLT_FACTOR, cost=hm.COST_FACTOR, gt=hm.GT_FACTOR)[k])


def test_no_winner_is_excused():
    lo, hi = math.inf, 0.0
    for name in hm.SCENES + ("plane+noise",):
        for n in NS:
            s, r = _searched(name, n)
            idx = hm.sample4(hm.SEARCH_SEED, r["best"], n)
            j = hm.judge_minimal(r["H0"], s["p1"][idx], s["p2"][idx])
            assert not j["excused"] and j["ok"] and j["ratio"] <= 0.1, (name, n, j)        # the model's own winner (re-normalised: a few ulps)
            lo, hi = min(lo, j["kappa"]), max(hi, j["kappa"])
    print("homography model: kappa of the winning samples %.3g .. %.3g (cut %.3g)" % (lo, hi, hm.KAPPA_CUT))
    assert hi <= 0.01 * hm.KAPPA_CUT


def test_outliers_of_the_planar_noisy_scene_stay_out():
    for n in NS:
        s, r = _searched("plane+noise", n)
        leak = len(np.intersect1d(np.nonzero(r["mask"])[0], s["outliers"]))
        print("homography model plane+noise n=%d: %d inliers, %d planted outliers among them (bound %.1f)" % (n, r["count"], leak, em.outlier_leak(n)))
        assert leak <= em.outlier_leak(n) and r["count"] >= 0.6 * n


def test_bootstrap_ratio_table():
    """h_ratio of Extractor.bootstrap_check as the model sees it, at its 1 px threshold and n = 200: the model's homography search over the
    epipolar consensus of the true E (every point of a noise-free scene; a scene without a baseline is fitted by any [t]x R).  The GPU test
    asserts `degenerate` only where this ratio lies outside 0.7 .. 0.9"""
    n, table = hm.BOOTSTRAP_N, {}
    for name in hm.SCENES:
        s, r = _searched(name, n, thr=hm.BOOTSTRAP_THR)
        e = n if s["E_gt"] is None else int(em.consensus(s["E_gt"], s["p1"], s["p2"], hm.BOOTSTRAP_THR)[0].sum())
        table[name] = r["count"] / max(e, 1)
        print("bootstrap model %-14s: h %3d / e %3d = %.3f" % (name, r["count"], e, table[name]))
    asserted = {k: v > 0.8 for k, v in table.items() if not 0.7 <= v <= 0.9}
    assert asserted == hm.BOOTSTRAP_DEGENERATE, asserted
    assert "small_baseline" not in asserted and 0.7 <= table["small_baseline"] <= 0.9
    s, r = _searched("small_baseline", n)                                        # the same scene at 3 px
    e = int(em.consensus(s["E_gt"], s["p1"], s["p2"], hm.THRESHOLD)[0].sum())
    print("bootstrap model small_baseline at 3 px: h %3d / e %3d = %.3f" % (r["count"], e, r["count"] / e))
    assert {"small_baseline": r["count"] / e > 0.8} == hm.BOOTSTRAP_DEGENERATE_3PX and r["count"] / e > 0.9
