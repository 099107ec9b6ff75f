"""GPU: homography RANSAC, DLT re-fit and Levenberg-Marquardt (csrc/vo_homography.hip) against the independent float64 model of
tests/homography_model.py, through VoContext.find_homography only (Extractor.bootstrap_check for the degeneracy verdict).

The model solves the minimal problem and the re-fit by LAPACK's SVD, refines by Gauss-Newton to convergence, and carries a longdouble truth
for each; tests/test_homography_model.py measures on the model alone the factor of every bound used here (FACTOR x u x kappa) and records
the search seed, the scene seed and the scenes whose degeneracy verdict is asserted.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import essential_model as em
import homography_model as hm

pytestmark = pytest.mark.gpu
SEED = hm.SEARCH_SEED
KEYS = ("H", "inl", "st", "H0")


def _stack(items):
    return np.stack([np.asarray(x) for x in items])


def _call_batch(problems, **kw):
    """problems: list of (p1, p2) of one n -> list of dict H, inl, st, H0 (one batched context, one call)"""
    from vo_mi355x import VoContext
    B = len(problems)
    kw.setdefault("seed", SEED)
    with VoContext(64, 64, max_pts=64, batch=B) as c:
        out = c.find_homography(_stack([p[0] for p in problems]), _stack([p[1] for p in problems]), **kw)
    if B == 1:
        return [dict(zip(KEYS, out))]
    return [dict(zip(KEYS, (out[0][b], out[1][b], out[2][b], out[3][b]))) for b in range(B)]


def _call(c, p1, p2, **kw):
    kw.setdefault("seed", SEED)
    return dict(zip(KEYS, c.find_homography(p1, p2, **kw)))


def _same_result(a, b):
    return em.bits_equal(a["H"], b["H"]) and em.bits_equal(a["H0"], b["H0"]) and np.array_equal(a["inl"], b["inl"]) and \
        {k: v for k, v in a["st"].items() if k != "cost"} == {k: v for k, v in b["st"].items() if k != "cost"} and \
        em.bits_equal(np.float64(a["st"]["cost"]), np.float64(b["st"]["cost"]))


def _mask(r, n):
    m = np.zeros(n, bool)
    m[r["inl"]] = True
    return m


@pytest.fixture(scope="module")
def ctx():
    from vo_mi355x import VoContext
    with VoContext(64, 64, max_pts=64) as c:
        yield c


_FULL = {}
FULL_SCENES = hm.SCENES + ("plane+noise",)


@pytest.fixture(scope="module")
def full():
    """n -> {scene name: (scene, result)} at the default parameters, the twelve scenes of one n in one batch"""
    def get(n):
        if n not in _FULL:
            scenes = [hm.planar_noisy(n) if name == "plane+noise" else hm.scene(name, n, hm.FULL_SEED) for name in FULL_SCENES]
            res = _call_batch([(s["p1"], s["p2"]) for s in scenes])
            _FULL[n] = {s["name"]: (s, r) for s, r in zip(scenes, res)}
        return _FULL[n]
    yield get
    _FULL.clear()


def _check_search(s, r, n, thr=hm.THRESHOLD, max_iters=hm.MAX_ITERS, seed=SEED):
    """the search part of a result against the model: the mask is the consensus of the returned H0, H0 is the solve of the documented sample
    of `best`, no evaluated hypothesis has a larger consensus in the model, the number of hypotheses is inside the model's bounds"""
    st = r["st"]
    assert st["status"] == 0 and 0 <= st["best"] < st["hypotheses"], st
    c = hm.judge_consensus(r["H0"], s["p1"], s["p2"], r["inl"], st["n_inliers"], thr)
    idx = hm.sample4(seed, st["best"], n)
    j = hm.judge_minimal(r["H0"], s["p1"][idx], s["p2"][idx])
    counts = [hm.hypothesis(s["p1"], s["p2"], seed, h, thr)[2] for h in range(st["hypotheses"])]
    lo, hi = hm.hypotheses_bounds(n, st["n_inliers"], max_iters=max_iters)
    print("k_h4 %s n=%d: best %d of %d hypotheses (bounds %d .. %d), %d inliers (model: %d for best, at most %d); mask differs in %d (outside band %d); "
          "kappa %.3g%s, |H0 - model| / (2^-52 kappa) = %.3g (bound %g)"
          % (s["name"], n, st["best"], st["hypotheses"], lo, hi, st["n_inliers"], counts[st["best"]], max(counts), c["differs"], c["outside_band"],
             j["kappa"], " (excused)" if j["excused"] else "", j["ratio"], hm.SOLVE_FACTOR))
    assert c["count_ok"] and c["outside_band"] == 0 and c["differs"] <= hm.BAND_POINTS, c
    assert not j["excused"] and j["ok"], j
    assert abs(counts[st["best"]] - st["n_inliers"]) <= hm.BAND_POINTS
    assert counts[st["best"]] >= max(counts) - hm.BAND_POINTS                                 # most inliers win ...
    assert all(cnt < counts[st["best"]] + hm.BAND_POINTS for cnt in counts[:st["best"]])       # ... and of equals the first
    assert st["hypotheses"] % hm.BATCH == 0 and lo <= st["hypotheses"] <= hi, (st, lo, hi)
    if st["n_inliers"] == n:
        assert st["hypotheses"] == hm.BATCH, st


def _check_refit(s, r, n, gt=False):
    """H against the model's re-fit and converged refinement on the returned mask; cost; on an exact scene the ground truth"""
    m = _mask(r, n)
    j = hm.judge_refit(r["H"], r["st"]["cost"], s["p1"], s["p2"], m)
    g = hm.judge_gt(r["H"], s, j["kappa"]) if gt else None
    print("k_h4 %s n=%d: %d LM steps (model: %d Gauss-Newton), kappa %.3g, |H - H*| / (2^-52 kappa) = %.3g (bound %g); cost %.6g, model %.6g, excess %.3g "
          "of the slack unit (bound %g)%s" % (s["name"], n, r["st"]["lm_iters"], j["model"]["iters"], j["kappa"], j["ratio"], hm.REFINE_FACTOR, r["st"]["cost"],
                                             j["model"]["cost"], j["cost_excess"], hm.COST_FACTOR,
                                             "" if g is None else "; |H - H_gt| / (2^-14 kappa) = %.3g (bound %g)" % (g["ratio"], hm.GT_FACTOR)))
    assert 1 <= r["st"]["lm_iters"] <= hm.REFINE_ITERS, r["st"]
    assert j["ok"], j["ratio"]
    assert j["cost_ok"] and j["cost_consistent"], (r["st"]["cost"], j["model"]["cost"], j["cost_excess"])
    if gt:
        assert g["ok"], g


# ---- (a) the minimal case ------------------------------------------------------------------------------------------------------------------
def test_minimal_case():
    sets = [hm.scene(name, 4, seed) for name, seed in hm.MINIMAL_SETS]
    res = _call_batch([(s["p1"], s["p2"]) for s in sets])
    worst = 0.0
    for (name, seed), s, r in zip(hm.MINIMAL_SETS, sets, res):
        st = r["st"]
        assert st["status"] == 0 and st["hypotheses"] == 256 and st["n_inliers"] == 4 and len(r["inl"]) == 4 and st["lm_iters"] == 0, (name, seed, st)
        assert em.bits_equal(r["H"], r["H0"]) and r["H0"][2, 2] == 1.0, (name, seed)            # (as cv2 returns it: divided by h33)
        idx = hm.sample4(SEED, st["best"], 4)
        j = hm.judge_minimal(r["H0"], s["p1"][idx], s["p2"][idx])
        worst = max(worst, j["ratio"])
        assert not j["excused"] and j["ok"], (name, seed, j)
        assert hm.hypothesis(s["p1"], s["p2"], SEED, st["best"])[2] == 4 and \
            all(hm.hypothesis(s["p1"], s["p2"], SEED, h)[2] < 4 for h in range(st["best"])), (name, seed, st)
        every = np.ones(4, bool)                                             # the cost is that of the returned H over the four points
        assert abs(st["cost"] - float(hm.cost_px(r["H"], s["p1"], s["p2"], every))) <= hm.cost_rounding_bound(r["H"], s["p1"], s["p2"], every)
    print("k_h4 n = 4: worst |H0 - model| / (2^-52 kappa) = %.3g (bound %g)" % (worst, hm.SOLVE_FACTOR))


# ---- (b) the winner, the re-fit and the refinement on full problems ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [40, 200])
@pytest.mark.parametrize("name", FULL_SCENES)
def test_winner_on_full_problem(full, name, n):
    s, r = full(n)[name]
    _check_search(s, r, n)
    _check_refit(s, r, n, gt=name in hm.EXACT)
    if name in hm.EXACT:
        assert r["st"]["n_inliers"] == n and len(r["inl"]) == n
    if name == "plane+noise":                                              # planted outliers on a scene that has a homography
        leak = len(np.intersect1d(r["inl"], s["outliers"]))
        print("k_h4 plane+noise n=%d: %d planted outliers in the mask (bound %.1f)" % (n, leak, em.outlier_leak(n)))
        assert leak <= em.outlier_leak(n) and len(r["inl"]) >= 0.6 * n


# ---- (c) structure -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 255, 256, 257])
def test_loop_edges(ctx, n):
    s = hm.planar_noisy(n, seed=2)
    r = _call(ctx, s["p1"], s["p2"], max_iters=256)
    assert r["st"]["hypotheses"] == 256
    _check_search(s, r, n, max_iters=256)
    if n == 4:
        assert em.bits_equal(r["H"], r["H0"]) and r["st"]["lm_iters"] == 0
    else:
        assert np.all(np.isfinite(r["H"])) and r["st"]["cost"] <= hm.THRESHOLD ** 2 * r["st"]["n_inliers"]


def _with_outliers(frac, seed):
    s = dict(hm.scene("plane", 200, seed))
    rng = np.random.default_rng(seed)
    out = rng.choice(200, int(frac * 200), replace=False)
    p2 = s["p2"].copy()
    p2[out] += (rng.uniform(-60, 60, (len(out), 2)) + 10).astype(np.float32)
    s.update(p2=p2, outliers=np.sort(out), name="plane+%d%%" % int(100 * frac))
    return s


def test_batch_of_three_that_stop_in_different_rounds():
    from vo_mi355x import VoContext
    scenes = [_with_outliers(0.0, 11), _with_outliers(0.65, 12), _with_outliers(0.75, 13)]      # the model: 256, 512 and 1536 hypotheses
    got = _call_batch([(s["p1"], s["p2"]) for s in scenes])
    rounds = [g["st"]["hypotheses"] for g in got]
    print("k_h4 batch of three: hypotheses %s, inliers %s" % (rounds, [g["st"]["n_inliers"] for g in got]))
    assert rounds[0] == 256 and rounds[0] < rounds[1] < rounds[2]
    for s, g in zip(scenes, got):
        with VoContext(64, 64, max_pts=64) as c:
            assert _same_result(_call(c, s["p1"], s["p2"]), g), s["name"]
        _check_search(s, g, 200)
        assert len(np.intersect1d(g["inl"], s["outliers"])) <= em.outlier_leak(200)


def test_workspace_reuse_and_regrowth():
    from vo_mi355x import VoContext
    big, small, bigger = hm.planar_noisy(300, seed=3), hm.planar_noisy(40, seed=4), hm.planar_noisy(400, seed=5)
    fresh = []
    for s in (big, small, bigger):
        with VoContext(64, 64, max_pts=64) as c:
            fresh.append(_call(c, s["p1"], s["p2"]))
    with VoContext(64, 64, max_pts=64) as c:
        for s, f in zip((big, small, bigger), fresh):                     # 300 allocates, 40 reuses, 400 > capacity regrows
            assert _same_result(_call(c, s["p1"], s["p2"]), f), len(s["p1"])


def test_same_seed_same_result(ctx):
    s = hm.planar_noisy(200, seed=6)
    a, b, other = _call(ctx, s["p1"], s["p2"], seed=3), _call(ctx, s["p1"], s["p2"], seed=3), _call(ctx, s["p1"], s["p2"], seed=4)
    assert _same_result(a, b)
    assert a["st"]["best"] != other["st"]["best"] or not em.bits_equal(a["H0"], other["H0"])      # (the seed does reach the generator)


def test_nan_rows_are_never_inliers(ctx):
    s = hm.scene("plane", 192, seed=6)
    p1, p2 = s["p1"].copy(), s["p2"].copy()
    p1[64], p2[64] = np.nan, np.nan
    p1[95, 0] = np.nan
    p2[127, 1] = np.nan
    r = _call(ctx, p1, p2)
    assert r["st"]["status"] == 0 and not np.isin([64, 95, 127], r["inl"]).any() and r["st"]["n_inliers"] == 189, r["st"]
    c = hm.judge_consensus(r["H0"], p1, p2, r["inl"], r["st"]["n_inliers"])
    assert c["count_ok"] and c["outside_band"] == 0 and c["differs"] <= hm.BAND_POINTS, c
    assert np.all(np.isfinite(r["H"])) and np.isfinite(r["st"]["cost"])
    # fewer than four finite correspondences: a status, NaN matrices, an empty mask, and the call itself succeeds
    q1, q2 = s["p1"][:8].copy(), s["p2"][:8].copy()
    q1[3:] = np.nan
    r = _call(ctx, q1, q2, max_iters=256)
    assert r["st"]["status"] == -6 and len(r["inl"]) == 0 and np.isnan(r["H"]).all() and np.isnan(r["H0"]).all(), r
    assert r["st"]["n_inliers"] == 0 and r["st"]["hypotheses"] == 256 and r["st"]["best"] == -1 and r["st"]["lm_iters"] == 0


def test_all_points_collinear_have_no_model(ctx):
    x = 100 + 140 * np.arange(8)
    line = np.stack([x, x // 5 + 40], 1).astype(np.float32)               # exactly on y = x / 5 + 40 in float32
    for p1, p2 in ((line, line + np.float32([5.0, 1.0])), (line, hm.scene("plane", 8, 1)["p2"]), (hm.scene("plane", 8, 1)["p1"], line)):
        r = _call(ctx, p1, p2, max_iters=256)
        assert r["st"]["status"] == -6 and r["st"]["best"] == -1 and r["st"]["n_inliers"] == 0 and r["st"]["hypotheses"] == 256, r["st"]
        assert len(r["inl"]) == 0 and np.isnan(r["H"]).all() and np.isnan(r["H0"]).all()


@pytest.mark.parametrize("name,n", [("general", 40), ("plane+noise", 200), ("pure_rotation", 40)])
def test_refine_iters_zero_returns_the_dlt_refit(ctx, full, name, n):
    s, ref = full(n)[name]
    r = _call(ctx, s["p1"], s["p2"], refine_iters=0)
    assert r["st"]["lm_iters"] == 0 and em.bits_equal(r["H0"], ref["H0"]) and np.array_equal(r["inl"], ref["inl"])
    j = hm.judge_dlt(r["H"], s["p1"], s["p2"], _mask(r, n))
    own = float(hm.cost_px(r["H"], s["p1"], s["p2"], _mask(r, n)))
    print("k_h4 %s n=%d refine_iters=0: |H - eigh| / (2^-52 kappa2) = %.3g (bound %g), kappa2 %.3g; cost %.6g against %.6g after refinement"
          % (name, n, j["ratio"], hm.DLT_FACTOR, j["kappa2"], r["st"]["cost"], ref["st"]["cost"]))
    assert j["ok"], j
    assert abs(r["st"]["cost"] - own) <= hm.COST_FACTOR * hm.cost_slack_unit(r["H"], s["p1"], s["p2"], _mask(r, n))
    assert ref["st"]["cost"] <= r["st"]["cost"] * (1 + 1e-9)               # the refinement never costs


def test_invalid_parameters(ctx):
    from vo_mi355x import VoError
    s = hm.scene("plane", 8, 1)
    bad = [dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")), dict(confidence=0.0), dict(confidence=1.0),
           dict(confidence=float("nan")), dict(max_iters=0), dict(refine_iters=-1), dict(refine_iters=101)]
    for kw in bad:
        with pytest.raises(VoError) as e:
            _call(ctx, s["p1"], s["p2"], **kw)
        assert e.value.code == -1, kw
    with pytest.raises(VoError) as e:
        _call(ctx, s["p1"][:3], s["p2"][:3])
    assert e.value.code == -1
    r = _call(ctx, s["p1"], s["p2"], refine_iters=100, max_iters=1)        # the edges of the valid ranges
    assert r["st"]["status"] == 0 and r["st"]["hypotheses"] == 256


# ---- (d) the degeneracy verdict ------------------------------------------------------------------------------------------------------------
def _keypoints(p):
    from vo_mi355x import Keypoint
    return [Keypoint(0, 1, uv.reshape(2, 1), uv.reshape(2, 1), np.zeros((1, 1)), [uv.reshape(2, 1)]) for uv in np.asarray(p, np.float32)]


def test_bootstrap_check(ctx):
    from vo_mi355x import Extractor
    ext = Extractor(lazy=False, min_kp_dist=7, ctx=ctx)
    cases = [(name, {}, want) for name, want in hm.BOOTSTRAP_DEGENERATE.items()] + \
        [(name, dict(threshold=hm.THRESHOLD), want) for name, want in hm.BOOTSTRAP_DEGENERATE_3PX.items()]
    for name, kw, want in cases:
        s = hm.scene(name, hm.BOOTSTRAP_N, hm.FULL_SEED)
        k1, k2 = _keypoints(s["p1"]), _keypoints(s["p2"])
        got = ext.bootstrap_check(em.K, k1, k2, seed=SEED, **kw)
        print("bootstrap_check %s %s: %s" % (name, kw, got))
        assert set(got) == {"e_inliers", "h_inliers", "h_ratio", "degenerate"}
        assert got["h_ratio"] == got["h_inliers"] / max(got["e_inliers"], 1) and got["degenerate"] == (got["h_ratio"] > 0.8)
        assert got["degenerate"] is want, (name, got)
    s = hm.scene("plane", 40, hm.FULL_SEED)
    H, inl, st, H0 = ext.find_homography(_keypoints(s["p1"]), _keypoints(s["p2"]), seed=SEED)
    assert isinstance(inl, list) and len(inl) == 40 and st["status"] == 0 and H[2, 2] == 1.0 and H0[2, 2] == 1.0
    assert hm.transfer_px(H, s["p1"], s["p2"]).max() <= 1e-3
