"""GPU: fundamental-matrix RANSAC and the eight-point re-fit (csrc/vo_fundamental.hip) against the independent float64 model of
tests/fundamental_model.py, through VoContext.find_fundamental (Extractor.find_fundamental for the keypoint lists).

The model solves the minimal problem by LAPACK's SVD and numpy's companion-matrix roots and the re-fit by SVD / eigh, and carries a longdouble
truth for each; tests/test_fundamental_model.py measures on the model alone the factor of every bound used here (FACTOR x u x kappa) and shows
that every problem used here is `decided`: no point's err within the rounding band of threshold^2, the winner decided by count or by a tie sum
with a relative margin above 1e-6.  So the winner, the counts and the mask are compared for equality.  Every figure is printed before it is
asserted."""
import numpy as np
import pytest

import essential_model as em
import fundamental_model as fm

pytestmark = pytest.mark.gpu
SEED = fm.SEARCH_SEED
KEYS = ("F", "inl", "st", "F0")


def _stack(items):
    return np.stack([np.asarray(x) for x in items])


def _call_batch(problems, **kw):
    """problems: list of (p1, p2) of one n -> list of dict F, inl, st, F0 (one batched context, one call)"""
    from vo_mi355x import VoContext
    B = len(problems)
    kw.setdefault("seed", SEED)
    with VoContext(64, 64, max_pts=64, batch=B) as c:
        out = c.find_fundamental(_stack([p[0] for p in problems]), _stack([p[1] for p in problems]), **kw)
    if B == 1:
        return [dict(zip(KEYS, out))]
    return [dict(zip(KEYS, (out[0][b], out[1][b], out[2][b], out[3][b]))) for b in range(B)]


def _call(c, p1, p2, **kw):
    kw.setdefault("seed", SEED)
    return dict(zip(KEYS, c.find_fundamental(p1, p2, **kw)))


def _same_result(a, b):
    return em.bits_equal(a["F"], b["F"]) and em.bits_equal(a["F0"], b["F0"]) and np.array_equal(a["inl"], b["inl"]) and \
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


_MODEL = {}


def _model(key, s, **kw):
    """the model's search on a scene, computed once per key"""
    if key not in _MODEL:
        _MODEL[key] = fm.search(s["p1"], s["p2"], **kw)
    return _MODEL[key]


def _check_search(tag, s, r, m):
    """a result against the model's search `m` (decided): winner, counts and mask equal; F0 within the model's bound of the winning root"""
    st, n = r["st"], len(s["p1"])
    assert m["decided"] and m["tie_margin"] > 1e-6, (tag, m["why"])
    j = fm.judge_minimal(r["F0"], s["p1"][fm.sample7(m["seed"], m["best"], n)], s["p2"][fm.sample7(m["seed"], m["best"], n)])
    d0 = fm.same_F(fm.unit(r["F0"]), m["F0"]) / (fm.EPS * m["kappa"])
    print("k_f7 %s n=%d: best %d (model %d) of %d hypotheses (model %d), %d inliers (model %d), %d roots (model %d), %d models (model %d); mask differs "
          "in %d; kappa %.3g, |F0 - model| / (2^-52 kappa) = %.3g (bound %g)"
          % (tag, n, st["best"], m["best"], st["hypotheses"], m["hypotheses"], st["n_inliers"], m["count"], st["n_roots"], m["n_roots"], st["models"],
             m["models"], int((_mask(r, n) != m["mask"]).sum()), m["kappa"], d0, fm.SOLVE_FACTOR))
    assert st["status"] == 0
    assert (st["best"], st["n_inliers"], st["hypotheses"]) == (m["best"], m["count"], m["hypotheses"]), st
    assert np.array_equal(_mask(r, n), m["mask"]) and len(r["inl"]) == st["n_inliers"]
    assert (st["n_roots"], st["models"]) == (m["n_roots"], m["models"]), st
    assert not j["excused"] and j["ok"] and d0 <= fm.SOLVE_FACTOR, (j, d0)


def _searched(tag, s, **kw):
    kw.setdefault("seed", SEED)
    m = dict(_model((tag, len(s["p1"])) + tuple(sorted(kw.items())), s, **kw))
    m["seed"] = kw["seed"]
    return m


# ---- (a) winner and mask against the model's search ---------------------------------------------------------------------------------------------
_FULL = {}


@pytest.fixture(scope="module")
def full():
    """n -> {scene name: (scene, result at refit=0, result at refit=1)}; the scenes of one n that share a search seed go in one batch"""
    def get(n):
        if n not in _FULL:
            _FULL[n] = {}
            seeds = sorted({fm.full_search_seed(name, n) for name in fm.SCENES})
            for seed in seeds:
                names = [name for name in fm.SCENES if fm.full_search_seed(name, n) == seed]
                scenes = [fm.scene(name, n) for name in names]
                r0 = _call_batch([(s["p1"], s["p2"]) for s in scenes], seed=seed)
                r1 = _call_batch([(s["p1"], s["p2"]) for s in scenes], seed=seed, refit=1)
                for name, s, a, b in zip(names, scenes, r0, r1):
                    _FULL[n][name] = (s, a, b)
        return _FULL[n]
    yield get
    _FULL.clear()


@pytest.mark.parametrize("n", fm.FULL_NS)
@pytest.mark.parametrize("name", fm.SCENES)
def test_winner_and_mask_on_full_problem(full, name, n):
    s, r, _ = full(n)[name]
    m = _searched(name, s, seed=fm.full_search_seed(name, n))
    _check_search(name, s, r, m)
    assert em.bits_equal(r["F"], r["F0"])                                    # refit = 0, the default: F is the winner's own model, bit for bit
    assert abs(r["st"]["cost"] - fm.cost(fm.unit(r["F0"]), s["p1"], s["p2"], m["mask"])) <= \
        fm.err_band(fm.unit(r["F0"]), s["p1"], s["p2"], 4 * fm.EPS)[m["mask"]].sum()            # (the unit-norm F0 re-made from F0 / f33: a few ulps)
    if name in fm.EXACT:
        assert r["st"]["n_inliers"] == n
    if name == "noisy":
        leak = len(np.intersect1d(r["inl"], s["outliers"]))
        print("k_f7 noisy n=%d: %d planted outliers in the mask (bound %.1f)" % (n, leak, em.outlier_leak(n)))
        assert leak <= em.outlier_leak(n) and len(r["inl"]) >= 0.6 * n


def test_the_tie_between_two_roots_goes_to_the_smaller_sum_of_err(ctx):
    s = fm.tie_scene()
    m = _searched("tie", s)
    r = _call(ctx, s["p1"], s["p2"])
    assert m["tie_margin"] < 1.0                                              # two roots of the winning sample hold all eight points
    _check_search("tie", s, r, m)


# ---- (b) structure ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", fm.EDGE_NS)
def test_loop_edges(ctx, n):
    if n == 7:                                                               # the one possible sample: every root holds all seven points
        s = fm.scene("general", 7, 1)
        r = _call(ctx, s["p1"], s["p2"])
        st = r["st"]
        roots = fm.seven_point(fm.widen(s["p1"]), fm.widen(s["p2"]))["models"]
        j = fm.judge_minimal(r["F0"], s["p1"], s["p2"])
        print("k_f7 n=7: %s, %d roots in the model, |F0 - nearest root| / (2^-52 kappa) = %.3g (bound %g)" % (st, len(roots), j["ratio"], fm.SOLVE_FACTOR))
        assert st["status"] == 0 and st["best"] == 0 and st["n_inliers"] == 7 and st["hypotheses"] == 256 and len(r["inl"]) == 7, st
        assert st["n_roots"] == len(roots) and not j["excused"] and j["ok"], j
        assert em.bits_equal(r["F"], r["F0"]) and r["F0"][2, 2] == 1.0          # (as cv2 returns it: divided by f33)
        return
    s = fm.edge_scene(n)
    _check_search(s["name"], s, _call(ctx, s["p1"], s["p2"]), _searched("edge", s))


def test_batch_of_three_that_stop_in_different_rounds():
    from vo_mi355x import VoContext
    scenes = fm.batch_scenes()
    got = _call_batch([(s["p1"], s["p2"]) for s in scenes])
    rounds = tuple(g["st"]["hypotheses"] for g in got)
    print("k_f7 batch of three: hypotheses %s, inliers %s" % (rounds, [g["st"]["n_inliers"] for g in got]))
    assert rounds == fm.BATCH_ROUNDS
    for s, g in zip(scenes, got):
        with VoContext(64, 64, max_pts=64) as c:
            assert _same_result(_call(c, s["p1"], s["p2"]), g), s["name"]
        _check_search(s["name"], s, g, _searched(s["name"], s))


def test_workspace_reuse_and_regrowth():
    from vo_mi355x import VoContext
    small, big, small2 = fm.edge_scene(63), fm.with_outliers("general", 300, 0.2, 3), fm.edge_scene(65)
    fresh = []
    for s in (small, big, small2):
        with VoContext(64, 64, max_pts=64) as c:
            fresh.append(_call(c, s["p1"], s["p2"], refit=1))
    with VoContext(64, 64, max_pts=64) as c:
        for s, f in zip((small, big, small2), fresh):                       # 63 allocates (64 slots), 300 > capacity regrows, 65 reuses
            assert _same_result(_call(c, s["p1"], s["p2"], refit=1), f), len(s["p1"])


def test_same_seed_same_result_and_another_seed_the_same_consensus_set(ctx):
    s = fm.with_outliers("general", 200, 0.3, fm.TWO_SEEDS_SCENE_SEED)
    ma, mb = _searched("two seeds", s, seed=3), _searched("two seeds", s, seed=4)
    assert ma["decided"] and mb["decided"] and ma["best"] != mb["best"] and np.array_equal(ma["mask"], mb["mask"])       # unambiguous in the model
    a, b, other = _call(ctx, s["p1"], s["p2"], seed=3), _call(ctx, s["p1"], s["p2"], seed=3), _call(ctx, s["p1"], s["p2"], seed=4)
    assert _same_result(a, b)
    assert a["st"]["best"] == ma["best"] and other["st"]["best"] == mb["best"] and np.array_equal(_mask(a, 200), ma["mask"])
    assert a["st"]["best"] != other["st"]["best"] or not em.bits_equal(a["F0"], other["F0"])      # (the seed does reach the generator)
    assert np.array_equal(a["inl"], other["inl"])                           # noise-free inliers, gross outliers: one consensus set
    truth = np.setdiff1d(np.arange(200), s["outliers"])
    assert np.all(np.isin(truth, a["inl"])) and len(a["inl"]) - len(truth) <= em.outlier_leak(200)


def test_nan_rows_are_never_inliers(ctx):
    s = fm.scene("general", 192, 6)
    p1, p2 = s["p1"].copy(), s["p2"].copy()
    p1[64], p2[64] = np.nan, np.nan
    p1[95, 0] = np.nan
    p2[127, 1] = np.nan
    r = _call(ctx, p1, p2)
    assert r["st"]["status"] == 0 and not np.isin([64, 95, 127], r["inl"]).any() and r["st"]["n_inliers"] == 189, r["st"]
    assert np.array_equal(_mask(r, 192), fm.consensus(fm.unit(r["F0"]), p1, p2))
    assert np.all(np.isfinite(r["F"])) and np.isfinite(r["st"]["cost"])
    # fewer than seven finite correspondences: a status, NaN matrices, an empty mask, and the call itself succeeds
    q1, q2 = s["p1"][:9].copy(), s["p2"][:9].copy()
    q1[6:] = np.nan
    r = _call(ctx, q1, q2, max_iters=256)
    assert r["st"]["status"] == -6 and len(r["inl"]) == 0 and np.isnan(r["F"]).all() and np.isnan(r["F0"]).all(), r
    assert r["st"]["n_inliers"] == 0 and r["st"]["hypotheses"] == 256 and r["st"]["best"] == -1 and r["st"]["n_roots"] == 0 and r["st"]["models"] == 0


def test_all_points_on_one_line_have_no_model(ctx):
    x = 100 + 140 * np.arange(9)
    line = np.stack([x, x // 5 + 40], 1).astype(np.float32)               # exactly on y = x / 5 + 40 in float32
    for p1, p2 in ((line, line + np.float32([5.0, 1.0])), (line, (line[::-1] * np.float32([1.0, 0.5])).astype(np.float32))):
        for refit in (0, 1):
            r = _call(ctx, p1, p2, max_iters=256, refit=refit)
            assert r["st"]["status"] == -6 and r["st"]["best"] == -1 and r["st"]["n_inliers"] == 0 and r["st"]["hypotheses"] == 256, r["st"]
            assert len(r["inl"]) == 0 and np.isnan(r["F"]).all() and np.isnan(r["F0"]).all() and r["st"]["models"] == 0


# ---- (c) the re-fit --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", fm.FULL_NS)
@pytest.mark.parametrize("name", fm.SCENES)
def test_refit(full, name, n):
    s, r0, r = full(n)[name]
    assert em.bits_equal(r["F0"], r0["F0"]) and np.array_equal(r["inl"], r0["inl"])          # the search does not depend on refit
    assert {k: v for k, v in r["st"].items() if k != "cost"} == {k: v for k, v in r0["st"].items() if k != "cost"}
    j = fm.judge_refit(r["F"], r["st"]["cost"], s["p1"], s["p2"], _mask(r, n))
    g = fm.judge_gt(r["F"], s, j["kappa8"]) if name in fm.EXACT else None
    own = fm.cost(fm.unit(r["F"]), s["p1"], s["p2"], _mask(r, n))
    print("k_f7 %s n=%d refit: kappa2 %.3g, |F - eigh| / (2^-52 kappa2) = %.3g (bound %g); sigma3 / sigma1 = %.3g x 2^-52 (bound %g); cost %.6g, "
          "model %.6g + slack %.3g, winner's %.6g%s"
          % (name, n, j["kappa2"], j["ratio"], fm.REFIT_FACTOR, j["rank2"], fm.RANK2_FACTOR, r["st"]["cost"], j["cost_model"], j["cost_slack"],
             r0["st"]["cost"], "" if g is None else "; |F - F_gt| / (2^-14 kappa8) = %.3g (bound %g)" % (g["ratio"], fm.GT_FACTOR)))
    assert j["ok"], j["ratio"]
    assert j["rank2_ok"], j["rank2"]
    assert j["cost_ok"] and abs(r["st"]["cost"] - own) <= j["cost_slack"] + 1e-300, (r["st"]["cost"], own, j["cost_model"], j["cost_slack"])
    if g is not None:
        assert g["ok"], g


def test_refit_with_seven_inliers_returns_the_winner(ctx):
    s = fm.scene("general", 7, 1)
    r0, r1 = _call(ctx, s["p1"], s["p2"]), _call(ctx, s["p1"], s["p2"], refit=1)
    assert r1["st"]["n_inliers"] == 7 and em.bits_equal(r1["F"], r1["F0"]) and _same_result(r0, r1)


# ---- (d) parameters and the Python layer -----------------------------------------------------------------------------------------------------
def test_invalid_parameters(ctx):
    import ctypes as C
    from vo_mi355x import VoError, _lib
    from vo_mi355x._lib import ptr
    s = fm.scene("general", 8, 1)
    bad = [dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan")), dict(threshold=float("inf")), dict(confidence=0.0),
           dict(confidence=1.0), dict(confidence=float("nan")), dict(max_iters=0), dict(refit=-1), dict(refit=2)]
    for kw in bad:
        with pytest.raises(VoError) as e:
            _call(ctx, s["p1"], s["p2"], **kw)
        assert e.value.code == -1, kw
    with pytest.raises(VoError) as e:
        _call(ctx, s["p1"][:6], s["p2"][:6])
    assert e.value.code == -1
    # the outputs are untouched
    L = _lib.load()
    prm = _lib.FundParams()
    L.vo_fundamental_default_params(C.byref(prm))
    prm.threshold = -1.0
    F, F0, mask, st = np.full(9, 7.5), np.full(9, 7.5), np.full(8, 9, np.uint8), _lib.FundStats(cost=7.5, n_inliers=9, hypotheses=9, best=9, status=9, n_roots=9, models=9)
    p1, p2 = np.ascontiguousarray(s["p1"]), np.ascontiguousarray(s["p2"])
    assert L.vo_fundamental_ransac(ctx._h, ptr(p1, C.c_float), ptr(p2, C.c_float), 8, C.byref(prm), ptr(F, C.c_double), ptr(F0, C.c_double),
                                   ptr(mask, C.c_uint8), C.byref(st)) == -1
    assert np.all(F == 7.5) and np.all(F0 == 7.5) and np.all(mask == 9) and (st.cost, st.n_inliers, st.models) == (7.5, 9, 9)
    r = _call(ctx, s["p1"], s["p2"], refit=1, max_iters=1, confidence=0.5)      # the edges of the valid ranges
    assert r["st"]["status"] == 0 and r["st"]["hypotheses"] == 256


def _keypoints(p):
    from vo_mi355x import Keypoint
    return [Keypoint(0, 1, uv.reshape(2, 1), uv.reshape(2, 1), np.zeros((1, 1)), [uv.reshape(2, 1)]) for uv in np.asarray(p, np.float32)]


def test_extractor_layer_on_a_calibrated_scene(ctx):
    from vo_mi355x import Extractor
    ext = Extractor(lazy=False, min_kp_dist=7, ctx=ctx)
    s = fm.scene("general", 200)
    F, inl, st, F0 = ext.find_fundamental(_keypoints(s["p1"]), _keypoints(s["p2"]), seed=SEED, refit=1)
    assert isinstance(inl, list) and len(inl) == 200 and st["status"] == 0 and F[2, 2] == 1.0 and F0[2, 2] == 1.0
    # K^T F K of the re-fit is an essential matrix: two equal singular values and a zero one, as far as those of the model's re-fit are
    f = fm.eight_point(s["p1"], s["p2"], np.ones(200, bool))
    got, want = fm.essential_defect(F), fm.essential_defect(f["F_eigh"])
    slack = fm.essential_defect_slack(f["F_eigh"], fm.REFIT_FACTOR * fm.EPS * f["kappa2"])
    print("K^T F K general n=200: (s1 - s2) / s1 = %.3g (model %.3g), s3 / s1 = %.3g (model %.3g), slack %.3g" % (got[0], want[0], got[1], want[1], slack))
    assert abs(got[0] - want[0]) <= slack and abs(got[1] - want[1]) <= slack
