"""GPU: five-point RANSAC + recoverPose (csrc/vo_essential.hip) against the independent float64 model of tests/essential_model.py, through
VoContext.essential_ransac only.

The model solves the minimal problem by another route (LAPACK null space, action matrix, eigenvectors), certifies every root by its own
residuals and scales every tolerance by the root's conditioning; tests/test_essential_model.py shows on the CPU that the oracle stays inside
the very same verdict functions (judge_*) and records where each constant comes from.  Nothing here refers to Nister's chain or to a Jacobi
SVD; the one thing taken from oracle/essential_oracle.py is `sample5`, the documented draw of hypothesis `best`, to know which five points
the winner was solved from (were the kernel to draw otherwise, the model would find no root next to E and the test would fail).
Covered: every root of 32 five-point sets through a sixth correspondence, the minimal case, validity and consensus of the winner on full problems,
recoverPose against LAPACK's four candidates as a set, the documented choice on a four-way tie, and bit-for-bit structure tests."""
import numpy as np
import pytest

import essential_model as em

pytestmark = pytest.mark.gpu
SEED = 7


def _stack(items):
    return np.stack([np.asarray(x) for x in items])


def _call_batch(problems, **kw):
    """problems: list of (p1, p2) of one n -> list of dict E, R, t, inl, st (one batched context, one call)"""
    from vo_mi355x import VoContext
    B = len(problems)
    with VoContext(64, 64, max_pts=64, batch=B) as c:
        out = c.essential_ransac(_stack([em.K] * B), _stack([p[0] for p in problems]), _stack([p[1] for p in problems]), seed=SEED, **kw)
    if B == 1:
        return [dict(zip(("E", "R", "t", "inl", "st"), out))]
    return [dict(E=out[0][b], R=out[1][b], t=out[2][b], inl=out[3][b], st=out[4][b]) for b in range(B)]


def _call(c, p1, p2, **kw):
    return dict(zip(("E", "R", "t", "inl", "st"), c.essential_ransac(em.K, p1, p2, **kw)))


def _same_result(a, b):
    return all(em.bits_equal(a[k], b[k]) for k in ("E", "R", "t")) and np.array_equal(a["inl"], b["inl"]) and a["st"] == b["st"]


def _check_hypotheses(st, n, max_iters=1000):
    lo, hi = em.hypotheses_bounds(n, st["n_inliers"], max_iters=max_iters)
    assert st["hypotheses"] % em.BATCH == 0 and lo <= st["hypotheses"] <= hi, (st, lo, hi)
    if st["n_inliers"] == n:
        assert st["hypotheses"] == em.BATCH, st


@pytest.fixture(scope="module")
def ctx():
    from vo_mi355x import VoContext
    with VoContext(64, 64, max_pts=64) as c:
        yield c


@pytest.fixture(scope="module")
def sixth():
    """every sixth-point call of every root problem, in one batch of n = 6"""
    keys = [(name, seed, k) for name in em.ROOT_SCENES for seed in em.ROOT_SEEDS for k in range(len(em.root_problem(name, seed)["calls"]))]
    calls = [em.root_problem(name, seed)["calls"][k] for name, seed, k in keys]
    return keys, _call_batch([(c["p1"], c["p2"]) for c in calls], threshold=em.SIXTH_THR, max_iters=256)


@pytest.fixture(scope="module")
def minimal():
    keys = [(name, seed) for name in em.ROOT_SCENES for seed in em.ROOT_SEEDS]
    return keys, _call_batch([(em.root_problem(*k)["s"]["p1"], em.root_problem(*k)["s"]["p2"]) for k in keys], max_iters=256)


_FULL = {}


@pytest.fixture(scope="module")
def full():
    """n -> {scene name: (scene, result)} at the default 1 px threshold, the eleven scenes of one n in one batch"""
    def get(n):
        if n not in _FULL:
            scenes = [em.scene(name, n, seed=em.FULL_SEED) for name in em.SCENES]
            res = _call_batch([(s["p1"], s["p2"]) for s in scenes])
            _FULL[n] = {s["name"]: (s, r) for s, r in zip(scenes, res)}
        return _FULL[n]
    yield get
    _FULL.clear()


# ---- (a) every root through a sixth correspondence -----------------------------------------------------------------------------------------
def test_every_root_is_found_and_accurate(sixth):
    keys, res = sixth
    excused = late = 0
    worst = dict(ratio=0.0, fit=0.0, validity=0.0)
    failed, kept = [], {name: 0 for name in em.ROOT_SCENES}
    for (name, seed, k), r in zip(keys, res):
        p = em.root_problem(name, seed)
        if r["st"]["status"] != 0 or r["st"]["n_inliers"] != 6 or len(r["inl"]) != 6 or r["st"]["hypotheses"] != 256:
            failed.append((name, seed, k, r["st"]))
            continue
        j = em.judge_sixth(r["E"], p, k)
        if j["excused"]:
            excused += 1
            continue
        kept[name] += 1
        late += r["st"]["best"] != 0
        worst["ratio"] = max(worst["ratio"], j["ratio"])
        worst["fit"] = max(worst["fit"], j["fit"] * j["sigma"] / (em.SIXTH_THR / em.F))
        worst["validity"] = max(worst["validity"], j["validity"] * j["sigma"] / em.EPS)
        if not (j["accurate"] and j["complete"] and j["valid"]):
            failed.append((name, seed, k, j))
    n = len(keys)
    print("k_e5 sixth-point calls: %d roots, %d excused (%.1f %%), best != 0 in %d (%.1f %%); worst |E - E'| sigma / 2^-52 = %.3g, "
          "|E - E_k| sigma / tn = %.3g, validity sigma / 2^-52 = %.3g; failed: %s"
          % (n, excused, 100.0 * excused / n, late, 100.0 * late / n, worst["ratio"], worst["fit"], worst["validity"], failed))
    assert not failed, failed
    assert excused <= em.EXCUSED_MAX * n and min(kept.values()) > 0, kept
    assert late <= em.LATE_MAX


# ---- (b) the minimal case ------------------------------------------------------------------------------------------------------------------
def test_minimal_case(minimal):
    keys, res = minimal
    worst = 0.0
    for (name, seed), r in zip(keys, res):
        p = em.root_problem(name, seed)
        assert r["st"]["status"] == 0 and r["st"]["n_inliers"] == 5 and len(r["inl"]) == 5 and r["st"]["hypotheses"] == 256, (name, seed, r["st"])
        j = em.judge_five(r["E"], p["q1"], p["q2"], p["sol"]["roots"])
        if j["excused"]:
            continue
        worst = max(worst, j["ratio"])
        assert j["accurate"] and j["valid"] and j["sampson_ok"] and j["listed"], (name, seed, j)
    print("k_e5 n = 5: worst |E - E_k| sigma / 2^-52 = %.3g" % worst)


# ---- (c) the winner on full problems -------------------------------------------------------------------------------------------------------
def _check_full(s, r, n, seed=SEED, max_iters=1000, gt=True):
    import essential_oracle as eo                                         # only for the documented sample of hypothesis `best`
    assert r["st"]["status"] == 0, r["st"]
    c = em.judge_consensus(r["E"], s["p1"], s["p2"], r["inl"], r["st"]["n_inliers"])
    assert c["count_ok"] and c["outside_band"] == 0 and c["differs"] <= em.BAND_POINTS, c
    idx = eo.sample5(seed, r["st"]["best"], n)
    q1, q2 = em.normalise(s["p1"]), em.normalise(s["p2"])
    j = em.judge_five(r["E"], q1[idx], q2[idx])
    dev = None
    assert not j["excused"] or s["name"] == "pure_rotation", j            # only the singular system may go unjudged
    if not j["excused"]:
        assert j["accurate"] and j["valid"], j
        if gt and s["E_gt"] is not None and s["name"] not in em.PLANAR + em.NO_BASELINE + ("noisy",):
            dev = em.same_E(r["E"], s["E_gt"]) * j["sigma"] / em.GT_DELTA
            assert dev <= em.GT_FACTOR, (dev, j)
            assert len(r["inl"]) == n
    _check_hypotheses(r["st"], n, max_iters)
    print("k_e5 %s n=%d: %d inliers, sigma %.2e%s, ratio %.3g, validity %.2e, |E - E_gt| = %s d / sigma, best %d, hyps %d"
          % (s["name"], n, len(r["inl"]), j["sigma"], " (excused)" if j["excused"] else "", j["ratio"], j["validity"],
             "-" if dev is None else "%.2f" % dev, r["st"]["best"], r["st"]["hypotheses"]))


@pytest.mark.parametrize("n", [40, 200])
@pytest.mark.parametrize("name", em.SCENES)
def test_winner_on_full_problem(full, name, n):
    s, r = full(n)[name]
    _check_full(s, r, n)
    if name == "noisy":
        assert len(np.intersect1d(r["inl"], s["outliers"])) <= em.outlier_leak(n) and len(r["inl"]) >= 0.6 * n


# ---- (d) recoverPose -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", em.SCENES)
def test_recover_pose_against_lapack(full, name):
    s, r = full(40)[name]
    j = em.judge_pose(r["E"], r["R"], r["t"], r["st"]["n_good"], s["p1"], s["p2"], r["inl"])
    print("k_e5 pose %s: candidate %d at %.2e, counts %s near %s, n_good %d" % (name, j["k"], j["cand_dist"], j["counts"], j["near"], r["st"]["n_good"]))
    assert j["cand_dist"] <= em.CAND_TOL and j["proper"] <= em.POSE_TOL
    assert j["count_ok"] and j["max_ok"], j
    if name not in em.PLANAR + em.NO_BASELINE + ("noisy",):             # noise-free: E is within GT_FACTOR d / sigma of [t]x R
        assert np.abs(r["R"] - s["R"]).max() <= 1e-2


@pytest.mark.parametrize("name", em.NO_BASELINE)
def test_four_way_tie(ctx, full, name):
    """no baseline to speak of: all four counts are 0 (distanceThresh = 50), and the library returns the rotation with the larger trace and
    the t with E = +[t]x R -- a property of E, whichever way an SVD labels its vectors"""
    s, r = full(40)[name]
    for seed in (SEED, 8, 9):
        a = _call(ctx, s["p1"], s["p2"], seed=seed)
        b = _call(ctx, s["p1"], s["p2"], seed=seed)
        assert _same_result(a, b)
        if seed == SEED:
            assert _same_result(a, r)                                      # alone = in the batch of eleven
        j = em.judge_pose(a["E"], a["R"], a["t"], a["st"]["n_good"], s["p1"], s["p2"], a["inl"])
        assert a["st"]["status"] == 0 and j["counts"] == [0, 0, 0, 0] and a["st"]["n_good"] == 0
        assert all(np.all(np.isfinite(a[k])) for k in ("E", "R", "t"))
        assert j["cand_dist"] <= em.CAND_TOL and j["proper"] <= em.POSE_TOL
        Rt, tt = em.tie_choice(a["E"])
        assert np.abs(a["R"] - Rt).max() <= em.CAND_TOL and np.abs(a["t"] - tt).max() <= em.CAND_TOL
        d = np.abs(a["R"] - s["R"]).max()
        print("k_e5 four-way tie %s seed %d: max |R - R_gt| = %.2e" % (name, seed, d))
        assert min(d, np.abs(em.twisted_pair(a["R"], a["E"]) - s["R"]).max()) <= em.TIE_R_TOL
        assert d <= em.TIE_R_TOL                                           # the smaller angle is the true rotation here


@pytest.mark.parametrize("name", em.NO_BASELINE)
def test_four_way_tie_across_seeds_with_the_same_E(ctx, name):
    """n = 5: every seed searches the same five points, and seeds whose first hypothesis draws them in the same order return bit-equal E
    (test_essential_model.py shows on the oracle that 10 of the 15 pairs do).  Equal E must give equal R, t, inliers and stats"""
    s = em.scene(name, 5, seed=em.FULL_SEED)
    runs = [_call(ctx, s["p1"], s["p2"], seed=sd, max_iters=256) for sd in em.TIE_SEEDS]
    same = 0
    for i, a in enumerate(runs):
        assert a["st"]["status"] == 0 and a["st"]["n_inliers"] == 5, a["st"]
        j = em.judge_pose(a["E"], a["R"], a["t"], a["st"]["n_good"], s["p1"], s["p2"], a["inl"])
        assert j["cand_dist"] <= em.CAND_TOL and j["count_ok"] and j["max_ok"], j
        if name == "pure_rotation":                       # a tie at any n; of small_baseline's five points the first root is a spurious one
            assert j["counts"] == [0, 0, 0, 0] and a["st"]["n_good"] == 0
            Rt, tt = em.tie_choice(a["E"])
            assert np.abs(a["R"] - Rt).max() <= em.CAND_TOL and np.abs(a["t"] - tt).max() <= em.CAND_TOL
        for b in runs[:i]:
            if em.bits_equal(a["E"], b["E"]):
                same += 1
                assert _same_result(a, b)
    print("k_e5 tie %s: %d of 15 seed pairs return bit-equal E" % (name, same))
    assert same >= 10                                    # the five seeds of one draw order at least: the check is not vacuous


# ---- (e) structure, bit for bit ------------------------------------------------------------------------------------------------------------
def _with_outliers(frac, seed):
    s = em.scene("general", 200, seed=seed)
    rng = np.random.default_rng(seed)
    out = rng.choice(200, int(frac * 200), replace=False)
    p2 = s["p2"].copy()
    p2[out] += (rng.uniform(-60, 60, (len(out), 2)) + 10).astype(np.float32)
    return dict(s, p2=p2, outliers=np.sort(out), name="general+%d%%" % int(100 * frac))


def test_batch_of_three_that_stop_in_different_rounds():
    from vo_mi355x import VoContext
    scenes = [_with_outliers(0.0, 11), _with_outliers(0.5, 12), _with_outliers(0.75, 13)]
    got = _call_batch([(s["p1"], s["p2"]) for s in scenes])
    rounds = [g["st"]["hypotheses"] for g in got]
    print("k_e5 batch of three: hypotheses %s, inliers %s" % (rounds, [g["st"]["n_inliers"] for g in got]))
    assert rounds[0] == 256 and rounds[0] < rounds[1] < rounds[2] == 1024
    for s, g in zip(scenes, got):
        with VoContext(64, 64, max_pts=64) as c:
            assert _same_result(_call(c, s["p1"], s["p2"], seed=SEED), g), s["name"]
        _check_full(s, g, 200, gt=False)
        assert len(np.intersect1d(g["inl"], s["outliers"])) <= em.outlier_leak(200)


def test_workspace_reuse_and_reallocation():
    from vo_mi355x import VoContext
    big, small, bigger = em.scene("noisy", 300, seed=3), em.scene("noisy", 40, seed=4), em.scene("noisy", 400, seed=5)
    fresh = []
    for s in (big, small, bigger):
        with VoContext(64, 64, max_pts=64) as c:
            fresh.append(_call(c, s["p1"], s["p2"], seed=SEED))
    with VoContext(64, 64, max_pts=64) as c:
        for s, f in zip((big, small, bigger), fresh):                     # 300 allocates, 40 reuses, 400 > capacity reallocates
            assert _same_result(_call(c, s["p1"], s["p2"], seed=SEED), f), len(s["p1"])


@pytest.mark.parametrize("n", [5, 63, 64, 65, 255, 256, 257])
def test_loop_edges(ctx, n):
    s = em.scene("noisy", n, seed=2)
    r = _call(ctx, s["p1"], s["p2"], seed=SEED, max_iters=256)
    assert r["st"]["status"] == 0 and r["st"]["hypotheses"] == 256
    c = em.judge_consensus(r["E"], s["p1"], s["p2"], r["inl"], r["st"]["n_inliers"])
    assert c["count_ok"] and c["outside_band"] == 0 and c["differs"] <= em.BAND_POINTS, c
    j = em.judge_pose(r["E"], r["R"], r["t"], r["st"]["n_good"], s["p1"], s["p2"], r["inl"])
    assert j["cand_dist"] <= em.CAND_TOL and j["count_ok"] and j["max_ok"], j


def test_nan_rows_are_never_inliers(ctx):
    s = em.scene("general", 192, seed=6)
    p1, p2 = s["p1"].copy(), s["p2"].copy()
    p1[64], p2[64] = np.nan, np.nan
    p1[95, 0] = np.nan
    p2[127, 1] = np.nan
    r = _call(ctx, p1, p2, seed=SEED)
    assert r["st"]["status"] == 0 and not np.isin([64, 95, 127], r["inl"]).any()
    c = em.judge_consensus(r["E"], p1, p2, r["inl"], r["st"]["n_inliers"])
    assert c["count_ok"] and c["outside_band"] == 0 and c["differs"] <= em.BAND_POINTS and r["st"]["n_inliers"] == 189, (c, r["st"])
    # fewer than five finite correspondences: a status, a NaN pose, an empty mask, and the call itself succeeds
    q1, q2 = s["p1"][:8].copy(), s["p2"][:8].copy()
    q1[4:] = np.nan
    r = _call(ctx, q1, q2, seed=SEED, max_iters=256)
    assert r["st"]["status"] != 0 and len(r["inl"]) == 0 and np.isnan(r["R"]).all() and np.isnan(r["t"]).all() and np.isnan(r["E"]).all()
    assert r["st"]["n_inliers"] == 0 and r["st"]["n_good"] == 0 and r["st"]["hypotheses"] == 256 and r["st"]["best"] == -1


def test_no_hypothesis_has_a_model(ctx):
    same = np.tile(np.float32([[300.0, 100.0]]), (8, 1))
    same[5:] = np.float32([[10, 20], [700, 300], [1200, 50]])
    x = np.linspace(100, 1100, 8)
    line = np.stack([x, 0.2 * x + 40], 1).astype(np.float32)
    for p1, p2 in ((same, same + np.float32(3.0)), (line, line + np.float32([5.0, 1.0]))):
        r = _call(ctx, p1, p2, seed=SEED, max_iters=256)
        st = r["st"]
        assert st["hypotheses"] == 256 and 0 <= st["n_inliers"] <= 8 and 0 <= st["n_good"] <= st["n_inliers"] and -1 <= st["best"] < 256, st
        if st["status"] == 0:
            assert st["n_inliers"] >= 5 and len(r["inl"]) == st["n_inliers"] and all(np.all(np.isfinite(r[k])) for k in ("E", "R", "t"))
        else:
            assert st["best"] == -1 and st["n_inliers"] == 0 and len(r["inl"]) == 0 and np.isnan(r["R"]).all()
