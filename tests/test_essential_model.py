"""CPU-only: the model of tests/essential_model.py certifies itself, its scenes are what their names say, and every bound the GPU test
(test_gpu_essential_model.py) asserts on the kernel holds for oracle/essential_oracle.py, the same algorithm in float64 on the CPU.

The verdict functions are the model's (judge_*): the GPU test applies the very same ones.  Each test prints the maxima it measured; the
tolerance constants of essential_model.py were fixed from these prints (worst case x the stated margin), never from a kernel run.

A run of the oracle costs 256 five-point solves per round in pure Python, so `_run` asks it for rounds of 8: a model that already holds every
point ends the search (RANSACUpdateNumIters returns 0), and since only a strictly larger consensus replaces the best model, the winner of a
256-round would be the same hypothesis.  Anything else is run again in rounds of 256 as the library does."""
import numpy as np
import pytest

import essential_model as em

_RUNS = {}


def _run(p1, p2, thr=1.0, seed=7, max_iters=1000, key=None):
    """-> dict E, R, t, inl, info (hyps as the library would report them), or E None"""
    import essential_oracle as eo
    if key is not None and key in _RUNS:
        return _RUNS[key]
    n = len(p1)
    E, R, t, inl, info = eo.essential_ransac(em.K, p1, p2, thr=thr, seed=seed, max_iters=max_iters, batch=8, return_info=True)
    if E is not None and info["count"] == n:
        info = dict(info, hyps=em.BATCH)
    else:
        E, R, t, inl, info = eo.essential_ransac(em.K, p1, p2, thr=thr, seed=seed, max_iters=max_iters, return_info=True)
    out = dict(E=E, R=R, t=t, inl=inl, info=info)
    if key is not None:
        _RUNS[key] = out
    return out


def _full(name, n):
    s = em.scene(name, n, seed=em.FULL_SEED)
    return s, _run(s["p1"], s["p2"], key=("full", name, n))


# ---- the model certifies itself ------------------------------------------------------------------------------------------------------------
def test_model_certifies_itself():
    worst_epi = worst_cub = worst_gt = 0.0
    n_roots = n_low = 0
    for name in em.ROOT_SCENES:
        for seed in em.ROOT_SEEDS:
            p = em.root_problem(name, seed)
            sol, s = p["sol"], p["s"]
            assert len(sol["uncertified"]) == 0, (name, seed, "a real candidate did not certify")
            assert 2 <= len(sol["roots"]) <= 10 and len(sol["roots"]) % 2 == 0, (name, seed, len(sol["roots"]))   # complex roots pair up
            for E, sg in zip(sol["roots"], sol["sigma"]):
                epi, cub, nrm = em.residual_maxima(E, sol["A"])
                worst_epi, worst_cub = max(worst_epi, epi), max(worst_cub, cub)
                assert em.certified(E, sol["A"]) and abs(np.linalg.norm(E) - 1) <= 4 * em.EPS
                n_roots += 1
                n_low += sg < em.SIGMA_CUT
            d = [em.same_E(E, s["E_gt"]) for E in sol["roots"]]
            k = int(np.argmin(d))
            if sol["sigma"][k] >= em.SIGMA_CUT:
                worst_gt = max(worst_gt, d[k] * sol["sigma"][k] / em.GT_DELTA)
                assert d[k] <= em.GT_FACTOR * em.GT_DELTA / sol["sigma"][k], (name, seed, d[k], sol["sigma"][k])
            assert len(sol["roots"]) >= 1, (name, "the scene lost all of its roots")
    print("essential model: %d roots, residual maxima epipolar %.2e cubic %.2e; [t]x R within %.2f d / sigma; %d roots under the cut-off (%.1f %%)"
          % (n_roots, worst_epi, worst_cub, worst_gt, n_low, 100.0 * n_low / n_roots))
    assert n_low <= em.EXCUSED_MAX * n_roots


def test_model_solver_is_chart_independent():
    """the same five points in another order and with the two views swapped (E -> E^T): the same roots"""
    p = em.root_problem("general", 2)
    perm = [3, 0, 4, 1, 2]
    a = em.five_point(p["q1"][perm], p["q2"][perm])
    b = em.five_point(p["q2"], p["q1"])
    assert len(a["roots"]) == len(b["roots"]) == len(p["sol"]["roots"])
    for E, sg in zip(p["sol"]["roots"], p["sol"]["sigma"]):
        assert min(em.same_E(E, r) for r in a["roots"]) <= 64 * em.EPS / sg
        assert min(em.same_E(E.T, r) for r in b["roots"]) <= 64 * em.EPS / sg


def test_scenes_are_what_they_say():
    for name in em.ROOT_SCENES:
        for seed in em.ROOT_SEEDS:
            sv = np.linalg.svd(em.root_problem(name, seed)["sol"]["A"], compute_uv=False)
            assert sv[4] >= 1e-6 * sv[0], (name, seed, sv)                                 # rank 5
    X = em.scene("plane", 40)["X"]
    sv = np.linalg.svd(np.concatenate([X, np.ones((40, 1))], 1), compute_uv=False)
    assert sv[3] <= 1e-13 * sv[0] and sv[2] >= 1e-3 * sv[0]                                # coplanar, not collinear
    assert np.ptp(em.scene("fronto", 40)["X"][:, 2]) == 0
    s = em.scene("forward", 40)
    ep = (em.K @ (s["t"] / s["t"][2]))[:2]
    assert 0 < ep[0] < em.W_IMG and 0 < ep[1] < em.H_IMG                                   # epipole inside the image
    assert 0.45 <= np.linalg.norm(em._MOTION["big_rotation"][0]) <= 0.55
    s = em.scene("small_baseline", 40)
    assert np.linalg.norm(s["t"]) <= 0.01 * s["X"][:, 2].min()
    w = em.scene("wide", 40)
    assert np.array_equal(w["p1"][:4], np.float32([[0, 0], [em.W_IMG, 0], [0, em.H_IMG], [em.W_IMG, em.H_IMG]]))
    assert np.array_equal(w["p1"][4], np.float32([em.K[0, 2], em.K[1, 2]]))
    s = em.scene("noisy", 200)
    assert len(s["outliers"]) == 60
    # no baseline to speak of: all four candidates score 0 under distanceThresh = 50, whatever E the search returns.  For a pure rotation
    # every [t]x R fits the points exactly, so three arbitrary directions stand for "whatever E"
    s = em.scene("pure_rotation", 40)
    q1, q2 = em.normalise(s["p1"]), em.normalise(s["p2"])
    for t in ((1.0, 0, 0), (0.3, -0.5, 0.8), (0.0, 0.1, -1.0)):
        E = em.skew(np.asarray(t)) @ s["R"]
        assert em.sampson_px(E, s["p1"], s["p2"]).max() <= 1e-3
        assert [c[2] for c in em.pose_counts(E, q1, q2)] == [0, 0, 0, 0]
    s = em.scene("small_baseline", 40)
    assert [c[2] for c in em.pose_counts(s["E_gt"], em.normalise(s["p1"]), em.normalise(s["p2"]))] == [0, 0, 0, 0]
    s = em.scene("general", 40)
    counts = [c[2] for c in em.pose_counts(s["E_gt"], em.normalise(s["p1"]), em.normalise(s["p2"]))]
    assert sorted(counts) == [0, 0, 0, 40]


def test_iteration_bound_restated():
    import pnp_oracle as po
    for prob in (0.9999, 0.99, 0.5):
        for ep in (0.0, 0.01, 0.3, 0.5, 0.75, 0.9, 0.99, 1.0):
            for mi in (1, 256, 1000, 100000):
                assert em.ransac_num_iters(prob, ep, 5, mi) == po.update_num_iters(prob, ep, 5, mi), (prob, ep, mi)
    assert em.ransac_num_iters(0.9999, 0.0) == 0 and em.ransac_num_iters(0.9999, 1.0) == 1000
    assert em.ransac_num_iters(0.9999, 0.5) == 290                                          # log(1e-4) / log(1 - 2^-5) = 290.1


# ---- (a) every root through a sixth correspondence -----------------------------------------------------------------------------------------
def test_oracle_finds_every_root():
    n = excused = late = 0
    worst = dict(ratio=0.0, validity=0.0, fit=0.0)
    failed = []
    for name in em.ROOT_SCENES:
        kept = 0
        for seed in em.ROOT_SEEDS:
            p = em.root_problem(name, seed)
            for k, call in enumerate(p["calls"]):
                assert call["residual"] < 1e-3 and call["thr"] < 1e-2
                r = _run(call["p1"], call["p2"], thr=call["thr"], max_iters=256)
                n += 1
                if r["E"] is None or len(r["inl"]) != 6:
                    failed.append((name, seed, k, "n_inliers %s" % (None if r["E"] is None else len(r["inl"]))))
                    continue
                j = em.judge_sixth(r["E"], p, k)
                if j["excused"]:
                    excused += 1
                    continue
                kept += 1
                late += r["info"]["best"] != 0
                worst["ratio"] = max(worst["ratio"], j["ratio"])
                worst["fit"] = max(worst["fit"], j["fit"] * j["sigma"] / (call["thr"] / em.F))
                worst["validity"] = max(worst["validity"], j["validity"] * j["sigma"] / em.EPS)
                if not (j["accurate"] and j["complete"] and j["valid"]):
                    failed.append((name, seed, k, j))
        assert kept > 0, (name, "every root of the scene is excused")
    print("essential oracle, sixth-point calls: %d roots, %d excused (%.1f %%), best != 0 in %d (%.1f %%); worst |E - E'| sigma / 2^-52 = %.3g, "
          "|E - E_k| sigma / tn = %.3g, validity sigma / 2^-52 = %.3g; failed: %s"
          % (n, excused, 100.0 * excused / n, late, 100.0 * late / n, worst["ratio"], worst["fit"], worst["validity"], failed))
    assert excused <= em.EXCUSED_MAX * n
    assert late <= em.LATE_MAX
    assert not failed, failed


# ---- the solver itself: one sample, every root ---------------------------------------------------------------------------------------------
# (the ABI shows a root only through a search over 256 samples, which draws the same points in many orders; here a single solve must do)
FAR_ROOT = (("fronto", 10), ("fronto", 24))      # sets with a root whose last null-space coordinate is 3e-6 of the others: next to the solver's
#                                                  rejection of roots "at infinity" (1e-10), found by a search over seeds 5 .. 159
LOST = {("fronto", 1): "one of 6 roots is missed: two roots 2e-3 apart in the hidden variable come out of the 10th-degree determinant 1e-2 off, "
                       "both refinements then run into the same root; nearest returned E is 8.0e-2 away",
        ("fronto", 3): "one of 6 roots is missed in the same way; nearest returned E is 1.3e-1 away"}


@pytest.mark.parametrize("name,seed", [pytest.param(n, s, marks=pytest.mark.xfail(strict=True, reason=LOST[(n, s)]) if (n, s) in LOST else ())
                                       for n, s in [(n, s) for n in em.ROOT_SCENES for s in em.ROOT_SEEDS] + list(FAR_ROOT)])
def test_oracle_single_solve_returns_every_root(name, seed):
    import essential_oracle as eo
    p = em.root_problem(name, seed)
    got = eo.five_point(p["q1"].tolist(), p["q2"].tolist())
    assert len(got) <= 10
    for E in got:                                                                          # nothing but roots comes back
        j = em.judge_five(E, p["q1"], p["q2"], p["sol"]["roots"])
        assert j["excused"] or (j["accurate"] and j["valid"] and j["listed"]), (name, seed, j)
    for Ek, sg in zip(p["sol"]["roots"], p["sol"]["sigma"]):                               # and every root does
        if sg >= em.SIGMA_CUT:
            d = min([em.same_E(Ek, E) for E in got] or [np.inf])
            assert d <= em.root_tolerance(sg), (name, seed, sg, d)


# ---- (b) the minimal case ------------------------------------------------------------------------------------------------------------------
def test_oracle_minimal_case():
    worst = 0.0
    for name in em.ROOT_SCENES:
        for seed in em.ROOT_SEEDS:
            p = em.root_problem(name, seed)
            r = _run(p["s"]["p1"], p["s"]["p2"], thr=1.0, max_iters=256)
            assert r["E"] is not None and len(r["inl"]) == 5 and r["info"]["hyps"] == 256
            j = em.judge_five(r["E"], p["q1"], p["q2"], p["sol"]["roots"])
            if j["excused"]:
                continue
            worst = max(worst, j["ratio"])
            assert j["accurate"] and j["valid"] and j["sampson_ok"] and j["listed"], (name, seed, j)
    print("essential oracle, n = 5: worst |E - E_k| sigma / 2^-52 = %.3g" % worst)


# ---- (c) full problems ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [40, 200])
@pytest.mark.parametrize("name", em.SCENES)
def test_oracle_full_problem(name, n):
    import essential_oracle as eo
    s, r = _full(name, n)
    assert r["E"] is not None
    c = em.judge_consensus(r["E"], s["p1"], s["p2"], r["inl"], r["info"]["count"])
    assert c["count_ok"] and c["outside_band"] == 0 and c["differs"] <= em.BAND_POINTS, c
    idx = eo.sample5(7, r["info"]["best"], n)
    q1, q2 = em.normalise(s["p1"]), em.normalise(s["p2"])
    j = em.judge_five(r["E"], q1[idx], q2[idx])
    gt = None
    assert not j["excused"] or name == "pure_rotation", j                                  # only the singular system may go unjudged
    if not j["excused"]:
        assert j["accurate"] and j["valid"], j
        if s["E_gt"] is not None and name not in em.PLANAR + em.NO_BASELINE + ("noisy",):
            gt = em.same_E(r["E"], s["E_gt"]) * j["sigma"] / em.GT_DELTA
            assert gt <= em.GT_FACTOR, (gt, j)
            assert len(r["inl"]) == n
    if name == "noisy":
        assert len(np.intersect1d(r["inl"], s["outliers"])) <= em.outlier_leak(n) and len(r["inl"]) >= 0.6 * n
    lo, hi = em.hypotheses_bounds(n, len(r["inl"]))
    assert r["info"]["hyps"] % em.BATCH == 0 and lo <= r["info"]["hyps"] <= hi
    if len(r["inl"]) == n:
        assert r["info"]["hyps"] == em.BATCH
    print("essential oracle %s n=%d: %d inliers, sigma %.2e%s, ratio %.3g, validity %.2e, |E - E_gt| = %s d / sigma, best %d, hyps %d"
          % (name, n, len(r["inl"]), j["sigma"], " (excused)" if j["excused"] else "", j["ratio"], j["validity"],
             "-" if gt is None else "%.2f" % gt, r["info"]["best"], r["info"]["hyps"]))


@pytest.mark.parametrize("n", [5, 63, 64, 65, 255, 256, 257])
def test_oracle_loop_edges(n):
    s = em.scene("noisy", n, seed=2)
    r = _run(s["p1"], s["p2"], max_iters=256)
    c = em.judge_consensus(r["E"], s["p1"], s["p2"], r["inl"], r["info"]["count"])
    assert c["count_ok"] and c["outside_band"] == 0 and c["differs"] <= em.BAND_POINTS, c


# ---- (d) recoverPose -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", em.SCENES)
def test_oracle_recover_pose(name):
    s, r = _full(name, 40)
    j = em.judge_pose(r["E"], r["R"], r["t"], r["info"]["n_good"], s["p1"], s["p2"], r["inl"])
    print("essential oracle pose %s: candidate %d at %.2e, counts %s near %s, n_good %d" % (name, j["k"], j["cand_dist"], j["counts"], j["near"], r["info"]["n_good"]))
    assert j["cand_dist"] <= em.CAND_TOL and j["proper"] <= em.POSE_TOL
    assert j["count_ok"] and j["max_ok"], j
    if name in em.NO_BASELINE:
        assert j["counts"] == [0, 0, 0, 0] and r["info"]["n_good"] == 0
        assert np.all(np.isfinite(r["R"])) and np.all(np.isfinite(r["t"]))
        Rt, tt = em.tie_choice(r["E"])                                                     # the documented choice on a four-way tie
        assert np.abs(r["R"] - Rt).max() <= em.CAND_TOL and np.abs(r["t"] - tt).max() <= em.CAND_TOL
        near = min(np.abs(r["R"] - s["R"]).max(), np.abs(em.twisted_pair(r["R"], r["E"]) - s["R"]).max())
        print("  four-way tie: max |R - R_gt| = %.2e (or its twisted pair: %.2e)" % (np.abs(r["R"] - s["R"]).max(), near))
        assert near <= em.TIE_R_TOL
        assert np.abs(r["R"] - s["R"]).max() <= em.TIE_R_TOL                                # the smaller angle is the true one here
    if name not in em.PLANAR + em.NO_BASELINE + ("noisy",):
        assert np.abs(r["R"] - s["R"]).max() <= 1e-2                                        # x2 ~ R x1 + t, the true pose (noise-free scenes:
        #                                        E is within GT_FACTOR d / sigma of [t]x R; an unrefitted five-point model of noisy points is not)


@pytest.mark.parametrize("name", em.NO_BASELINE)
def test_oracle_tie_across_seeds_with_the_same_E(name):
    """n = 5: every seed searches the same five points, and seeds whose first hypothesis draws them in the same order return bit-equal E.
    Equal E must give equal R, t and counts; the seeds are chosen so that both cases occur"""
    s = em.scene(name, 5, seed=em.FULL_SEED)
    runs = [_run(s["p1"], s["p2"], seed=sd, max_iters=256) for sd in em.TIE_SEEDS]
    assert all(r["E"] is not None and len(r["inl"]) == 5 for r in runs)
    if name == "pure_rotation":                           # a tie at any n; of small_baseline's five points the first root is a spurious one
        assert all(r["info"]["n_good"] == 0 and r["info"]["good"] == [0, 0, 0, 0] for r in runs)
    same = 0
    for i in range(len(runs)):
        for j in range(i):
            if em.bits_equal(runs[i]["E"], runs[j]["E"]):
                same += 1
                assert em.bits_equal(runs[i]["R"], runs[j]["R"]) and em.bits_equal(runs[i]["t"], runs[j]["t"])
                assert np.array_equal(runs[i]["inl"], runs[j]["inl"]) and runs[i]["info"] == runs[j]["info"]
    print("essential oracle tie %s: %d of %d seed pairs return bit-equal E" % (name, same, len(runs) * (len(runs) - 1) // 2))
    assert same >= 10                                    # the five seeds of one draw order at least: the check is not vacuous


def test_oracle_tie_rule_does_not_depend_on_labels():
    """a four-way tie: E, -E and E with the roles of R1 / R2 exchanged by an SVD that lists its vectors differently all give the rule's pose"""
    import essential_oracle as eo
    s = em.scene("pure_rotation", 40)
    q1, q2 = em.normalise(s["p1"]), em.normalise(s["p2"])
    for t in ((1.0, 0, 0), (0.3, -0.5, 0.8), (0.0, 0.1, -1.0), (-0.2, 0.9, 0.1)):
        for sign in (1.0, -1.0):
            E = sign * em.skew(np.asarray(t)) @ s["R"]
            E = E / np.linalg.norm(E)
            R, tt, g, good = eo.recover_pose(E, q1, q2)
            assert good == [0, 0, 0, 0] and g == 0
            assert np.abs(R - s["R"]).max() <= 1e-12
            assert np.abs(tt - sign * np.asarray(t) / np.linalg.norm(t)).max() <= 1e-12      # E = +[t]x R
            Rm, tm = em.tie_choice(E)
            assert np.abs(R - Rm).max() <= em.CAND_TOL and np.abs(tt - tm).max() <= em.CAND_TOL


def test_oracle_nonzero_tie_keeps_the_order_of_preference():
    """half of the points seen under (R, t), half under its twisted pair: two candidates tie at a non-zero count and the first in OpenCV's
    order (R1 = U W V^T before R2 = U W^T V^T, +t before -t) wins"""
    import essential_oracle as eo
    s = em.scene("forward", 40)
    E = s["E_gt"]
    t = s["t"] / np.linalg.norm(s["t"])
    R2 = (2 * np.outer(t, t) - np.eye(3)) @ s["R"]
    X = s["X"][20:]
    Xc = X @ R2.T + s["t"]
    assert (Xc[:, 2] > 1).all()
    q1 = np.concatenate([em.normalise(s["p1"])[:20], X[:, :2] / X[:, 2:3]])
    q2 = np.concatenate([em.normalise(s["p2"])[:20], Xc[:, :2] / Xc[:, 2:3]])
    counts = [c[2] for c in em.pose_counts(E, q1, q2)]
    assert sorted(counts) == [0, 0, 20, 20], counts
    R, tt, g, good = eo.recover_pose(E, q1, q2)
    assert list(good) == counts and g == 20
    k, d = em.which_candidate(E, R, tt)
    assert d <= em.CAND_TOL and k == counts.index(20)


def test_oracle_threshold_is_inclusive():
    """a point whose squared distance equals the squared threshold to the bit is an inlier (OpenCV: err <= thresh).  One point of a clean scene
    is moved off its epipolar line; with the threshold at exactly its distance the winner of the 1 px search still holds all n points, no
    earlier hypothesis can (it would have won at 1 px), so the same model must come back with the same consensus"""
    import essential_oracle as eo
    s = em.scene("general", 40)
    tested = 0
    for j in range(24):
        p2 = s["p2"].copy()
        p2[39, 1] += np.float32(0.30 + 0.01 * j)
        r = _run(s["p1"], p2)
        e2 = eo.sampson_err2(r["E"], eo.normalise(em.K, s["p1"]), eo.normalise(em.K, p2))
        assert len(r["inl"]) == 40 and np.argmax(e2) == 39 and 0.1 < em.F * np.sqrt(e2[39]) < 0.6
        base = em.F * np.sqrt(e2[39])
        exact = [thr for thr in (base, np.nextafter(base, np.inf), np.nextafter(base, -np.inf)) if (thr / em.F) ** 2 == e2[39]]
        if not exact:
            continue                                                                       # e2 is not the square of a representable threshold
        r2 = _run(s["p1"], p2, thr=float(exact[0]))
        assert r2["E"] is not None and em.bits_equal(r2["E"], r["E"]) and r2["info"]["count"] == 40 and 39 in r2["inl"], (j, r2["info"])
        tested += 1
        break
    assert tested == 1


# ---- inputs without a model ----------------------------------------------------------------------------------------------------------------
def test_oracle_no_hypothesis_has_a_model():
    p = np.tile(np.float32([[300.0, 100.0]]), (8, 1))
    p[5:] = np.float32([[10, 20], [700, 300], [1200, 50]])
    r = _run(p, p + np.float32(3.0), max_iters=256)
    assert r["E"] is None or len(r["inl"]) >= 5
    x = np.linspace(100, 1100, 8)
    line = np.stack([x, 0.2 * x + 40], 1).astype(np.float32)
    r = _run(line, line + np.float32([5.0, 1.0]), max_iters=256)
    assert r["E"] is None or (np.all(np.isfinite(r["E"])) and len(r["inl"]) >= 5)
