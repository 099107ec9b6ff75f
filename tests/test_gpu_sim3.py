"""GPU: Sim(3) / rigid 3D-3D alignment RANSAC and the Umeyama fit (csrc/vo_sim3.hip) against the independent float64 model of
tests/sim3_model.py, through VoContext.estimate_sim3 and VoContext.fit_sim3.

The model solves the closed form by LAPACK's SVD and carries a 40-digit truth; tests/test_sim3_model.py measures on the model alone the
factor of both bounds used here (FACTOR x 2^-52 x kappa) and shows that every problem used here is `decided`: no point's squared error within
the rounding band of threshold^2, the winner decided by count or by the smaller h on an exact tie, no degeneracy figure near its tolerance.
So the winner, the counts and the mask are compared for equality.  Every figure is printed before it is asserted."""
import ctypes as C

import numpy as np
import pytest

import sim3_model as sm

pytestmark = pytest.mark.gpu
KEYS = ("s", "R", "t", "inl", "st", "m0")
VO_E_INVALID, VO_E_NUMERIC = -1, -6


def _kw(kw):
    """the model's search keywords -> estimate_sim3's"""
    out = dict(kw)
    out["threshold"] = out.pop("thr")
    return out


def _call(c, s, kw, **more):
    return dict(zip(KEYS, c.estimate_sim3(s["src"], s["dst"], **dict(_kw(kw), **more))))


def _model_of(r):
    return sm.pack(r["s"], r["R"], r["t"])


def _mask(r, n):
    m = np.zeros(n, bool)
    m[r["inl"]] = True
    return m


def _same_result(a, b):
    return all(sm.bits_equal(np.float64(a[k]), np.float64(b[k])) for k in ("s", "R", "t", "m0")) and np.array_equal(a["inl"], b["inl"]) and \
        {k: v for k, v in a["st"].items() if k != "cost"} == {k: v for k, v in b["st"].items() if k != "cost"} and \
        sm.bits_equal(np.float64(a["st"]["cost"]), np.float64(b["st"]["cost"]))


@pytest.fixture(scope="module")
def ctx():
    from vo_mi355x import VoContext
    with VoContext(64, 64, max_pts=64) as c:
        yield c


_PROBLEMS, _MODEL = {}, {}


def problem(name):
    """-> (scene, keywords, the model's search), computed once"""
    if not _PROBLEMS:
        _PROBLEMS.update(sm.problems())
    if name not in _MODEL:
        s, kw = _PROBLEMS[name]
        _MODEL[name] = sm.search(s["src"], s["dst"], **kw)
    return _PROBLEMS[name] + (_MODEL[name],)


def check(tag, s, kw, m, r, refit=1):
    """a result against the model's search `m` (decided): winner, counts and mask equal; model0 within SOLVE_FACTOR of the winning sample's
    model; the returned model within REFIT_FACTOR of the model's fit over the mask, or (refit 0) model0 itself; the cost within what the
    bound on the model lets it move"""
    st, n, ws = r["st"], len(s["src"]), kw.get("with_scale", True)
    assert m["decided"], (tag, m["why"])
    d0 = sm.diff(r["m0"], m["m0"], m["tscale"]) / (sm.EPS * m["kappa"])
    fin = sm.finish(s["src"], s["dst"], m, refit, ws)
    print("k_s3 %s n=%d: best %d (model %d) of %d hypotheses (model %d), %d inliers (model %d), %d degenerate (model %d), refit %d (model %d); mask "
          "differs in %d; kappa %.3g, |model0 - model| / (2^-52 kappa) = %.3g (bound %g)"
          % (tag, n, st["best"], m["best"], st["hypotheses"], m["hypotheses"], st["n_inliers"], m["count"], st["degenerate"], m["degenerate"],
             st["refit"], fin["refit"], int((_mask(r, n) != m["mask"]).sum()), m["kappa"], d0, sm.SOLVE_FACTOR))
    assert st["status"] == 0
    assert (st["best"], st["n_inliers"], st["hypotheses"], st["degenerate"]) == (m["best"], m["count"], m["hypotheses"], m["degenerate"]), st
    assert np.array_equal(_mask(r, n), m["mask"]) and len(r["inl"]) == st["n_inliers"]
    assert d0 <= sm.SOLVE_FACTOR, d0
    assert st["refit"] == fin["refit"]
    got = _model_of(r)
    if fin["refit"]:
        f = fin["fit"]
        d1 = sm.diff(got, f["m"], f["tscale"]) / (sm.EPS * f["kappa"])
        slack = float(sm.err_band(f["m"], s["src"], s["dst"], sm.REFIT_FACTOR * sm.EPS * f["kappa"], f["tscale"])[m["mask"]].sum())
        print("k_s3_finish %s: fit kappa %.3g, |model - fit| / (2^-52 kappa) = %.3g (bound %g); cost %.17g (model %.17g, slack %.3g)"
              % (tag, f["kappa"], d1, sm.REFIT_FACTOR, st["cost"], fin["cost"], slack))
        assert d1 <= sm.REFIT_FACTOR, d1
    else:
        slack = float(sm.err_band(m["m0"], s["src"], s["dst"], sm.SOLVE_FACTOR * sm.EPS * m["kappa"], m["tscale"])[m["mask"]].sum())
        print("k_s3_finish %s: the winner's model returned as found; cost %.17g (model %.17g, slack %.3g)" % (tag, st["cost"], fin["cost"], slack))
        assert sm.bits_equal(got, np.asarray(r["m0"], float))
    assert abs(st["cost"] - fin["cost"]) <= slack


# ---- minimal and small -----------------------------------------------------------------------------------------------------------------------
def test_three_points_are_the_only_sample(ctx):
    s, kw, m = problem("n3")
    r = _call(ctx, s, kw)
    check("n3", s, kw, m, r)
    r0 = _call(ctx, s, kw, refit=0)
    check("n3 refit=0", s, kw, m, r0, refit=0)
    assert r0["st"]["best"] == 0 and r0["st"]["refit"] == 0 and sm.bits_equal(_model_of(r0), r0["m0"])      # the model as found


def test_four_points(ctx):
    s, kw, m = problem("n4")
    check("n4", s, kw, m, _call(ctx, s, kw))


def test_three_collinear_points_have_no_model(ctx):
    src = np.array([[0, 0, 0], [1, 1, 1], [2, 2, 2]], np.float32)
    r = dict(zip(KEYS, ctx.estimate_sim3(src, src + np.float32(1), threshold=sm.THR, seed=sm.SEARCH_SEED)))
    print("collinear n=3:", r["st"], r["s"], r["inl"])
    assert r["st"]["status"] == VO_E_NUMERIC and r["st"]["n_inliers"] == 0 and r["st"]["best"] == -1 and r["st"]["degenerate"] == r["st"]["hypotheses"] == 1024
    assert np.isnan(r["s"]) and np.isnan(r["R"]).all() and np.isnan(r["t"]).all() and np.isnan(r["m0"]).all() and len(r["inl"]) == 0


# ---- strides: the wave's 64-lane loop, the finish kernel's 256-thread stride, and the workspace growing under them ---------------------------
@pytest.mark.parametrize("n", sm.STRIDE_NS)
def test_loop_strides(ctx, n):
    s, kw, m = problem("stride%d" % n)
    assert abs(s["inliers"].mean() - 0.7) < 0.01
    check("stride%d" % n, s, kw, m, _call(ctx, s, kw))


def test_workspace_regrowth_keeps_the_results():
    from vo_mi355x import VoContext
    small, big = problem("stride63"), problem("stride300")
    with VoContext(64, 64, max_pts=64) as c:
        a0 = _call(c, small[0], small[1])
        b0 = _call(c, big[0], big[1])                           # 300 > 64: the workspace is replaced
        a1 = _call(c, small[0], small[1])                       # and serves the smaller problem again
    with VoContext(64, 64, max_pts=512) as c:
        b1 = _call(c, big[0], big[1])
    check("stride300 after regrowth", big[0], big[1], big[2], b0)
    assert _same_result(a0, a1) and _same_result(b0, b1)


# ---- more than one round ---------------------------------------------------------------------------------------------------------------------
def test_three_rounds_and_the_cap(ctx):
    s, kw, m = problem("rounds")
    assert sm.ransac_num_iters(sm.CONFIDENCE, 160 / 200) == 573 and m["hypotheses"] == 768
    r = _call(ctx, s, kw)
    check("rounds", s, kw, m, r)
    assert r["st"]["hypotheses"] == 768
    s, kw, m = problem("capped")
    r = _call(ctx, s, kw)
    check("capped", s, kw, m, r)
    assert r["st"]["hypotheses"] == 256 and kw["max_iters"] == 100


# ---- branches --------------------------------------------------------------------------------------------------------------------------------
def test_without_scale_on_a_rigid_pair(ctx):
    s, kw, m = problem("rigid")
    r = _call(ctx, s, kw)
    check("rigid", s, kw, m, r)
    assert r["s"] == 1.0 and r["m0"][0] == 1.0


def test_without_scale_on_a_pair_of_scale_two(ctx):
    s, kw, m = problem("rigid_on_scale2")
    r = _call(ctx, s, kw)
    check("rigid_on_scale2", s, kw, m, r)
    full = _call(ctx, s, dict(kw, with_scale=True))
    print("rigid_on_scale2: %d inliers without scale, %d with" % (r["st"]["n_inliers"], full["st"]["n_inliers"]))
    assert r["s"] == 1.0 and r["st"]["n_inliers"] == m["count"] < full["st"]["n_inliers"]


def test_mirrored_dst_gives_a_proper_rotation(ctx):
    s, kw, m = problem("mirrored")
    r = _call(ctx, s, kw)
    check("mirrored", s, kw, m, r)
    det, det0 = np.linalg.det(r["R"]), np.linalg.det(sm.unpack(r["m0"])[1])
    print("mirrored: det R - 1 = %.3g, det R0 - 1 = %.3g, %d of %d inliers" % (det - 1, det0 - 1, r["st"]["n_inliers"], len(s["src"])))
    assert abs(det - 1) <= 1e-12 and abs(det0 - 1) <= 1e-12 and r["st"]["n_inliers"] == m["count"] < len(s["src"]) // 2


def test_planar_cloud(ctx):
    s, kw, m = problem("planar")
    r = _call(ctx, s, kw)
    check("planar", s, kw, m, r)
    assert r["st"]["refit"] == 1 and abs(np.linalg.det(r["R"]) - 1) <= 1e-12


def test_collinear_consensus_set_returns_the_winner(ctx):
    s, kw, m = problem("collinear_consensus")
    r = _call(ctx, s, kw)
    check("collinear_consensus", s, kw, m, r)
    assert r["st"]["refit"] == 0 and r["st"]["n_inliers"] == 25 and sm.bits_equal(_model_of(r), r["m0"])


def test_nan_rows_are_never_inliers_and_their_samples_count_as_degenerate(ctx):
    s, kw, m = problem("nan_rows")
    r = _call(ctx, s, kw)
    check("nan_rows", s, kw, m, r)
    assert r["st"]["degenerate"] == m["degenerate"] > 0 and not _mask(r, 65)[[5, 17, 40]].any()


# ---- batch -----------------------------------------------------------------------------------------------------------------------------------
def test_batch_of_three_equals_each_alone_and_repeats_itself(ctx):
    from vo_mi355x import VoContext
    P = [problem("batch%d" % i) for i in range(3)]
    kw = _kw(P[0][1])
    src, dst = np.stack([p[0]["src"] for p in P]), np.stack([p[0]["dst"] for p in P])
    with VoContext(64, 64, max_pts=64, batch=3) as c:
        o1 = c.estimate_sim3(src, dst, **kw)
        o2 = c.estimate_sim3(src, dst, **kw)
    rounds = []
    for b, (s, k, m) in enumerate(P):
        r1, r2 = (dict(zip(KEYS, (o[0][b], o[1][b], o[2][b], o[3][b], o[4][b], o[5][b]))) for o in (o1, o2))
        check("batch%d" % b, s, k, m, r1)
        alone = _call(ctx, s, k)
        assert _same_result(r1, alone), b
        assert _same_result(r1, r2), b
        rounds.append(r1["st"]["hypotheses"])
    print("batch: hypotheses", rounds)
    assert len(set(rounds)) >= 2


# ---- the fit alone -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("stride65", "stride300", "planar", "rigid"))
def test_fit_on_the_returned_mask_is_the_search_bit_for_bit(ctx, name):
    s, kw, m = problem(name)
    ws = kw.get("with_scale", True)
    r = _call(ctx, s, kw)
    assert r["st"]["refit"] == 1
    fs, fR, ft, fst = ctx.fit_sim3(s["src"], s["dst"], _mask(r, len(s["src"])), with_scale=ws)
    print("fit %s: s %.17g (search %.17g), cost %.17g (search %.17g), %d rows" % (name, fs, r["s"], fst["cost"], r["st"]["cost"], fst["n_inliers"]))
    assert sm.bits_equal(np.float64(fs), np.float64(r["s"])) and sm.bits_equal(fR, r["R"]) and sm.bits_equal(ft, r["t"])
    assert sm.bits_equal(np.float64(fst["cost"]), np.float64(r["st"]["cost"])) and fst["n_inliers"] == r["st"]["n_inliers"] and fst["status"] == 0


@pytest.mark.parametrize("name", ("n4", "stride257", "nan_rows"))
def test_fit_on_every_row_against_the_model(ctx, name):
    s, kw, _ = problem(name)
    if name == "stride257":                                     # every row: the inliers only, so that the fit means something
        src, dst = s["src"][s["inliers"]], s["dst"][s["inliers"]]
    else:
        src, dst = s["src"], s["dst"]
    f = sm.fit(src, dst, None)
    fs, fR, ft, fst = ctx.fit_sim3(src, dst)
    d = sm.diff(sm.pack(fs, fR, ft), f["m"], f["tscale"]) / (sm.EPS * f["kappa"])
    print("fit %s all rows: %d rows (model %d), kappa %.3g, |fit - model| / (2^-52 kappa) = %.3g (bound %g)"
          % (name, fst["n_inliers"], f["count"], f["kappa"], d, sm.REFIT_FACTOR))
    assert fst["status"] == 0 and fst["n_inliers"] == f["count"] and d <= sm.REFIT_FACTOR


def test_fit_without_a_model(ctx):
    line = np.stack([np.arange(6.0), np.zeros(6), np.zeros(6)], 1).astype(np.float32)
    fs, fR, ft, fst = ctx.fit_sim3(line, line)
    assert fst["status"] == VO_E_NUMERIC and np.isnan(fs) and np.isnan(fR).all() and np.isnan(ft).all()
    s, _, _ = problem("n4")
    fs, fR, ft, fst = ctx.fit_sim3(s["src"], s["dst"], np.array([1, 1, 0, 0]))
    assert fst["status"] == VO_E_NUMERIC and np.isnan(fs)


# ---- invalid arguments -----------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_rejected_and_leave_the_context_as_it_was(ctx):
    from vo_mi355x import _lib
    s, kw, m = problem("stride64")
    before = _call(ctx, s, kw)
    L, h = ctx._L, ctx._h
    src, dst = np.ascontiguousarray(s["src"]), np.ascontiguousarray(s["dst"])
    ps, pd = _lib.ptr(src, C.c_float), _lib.ptr(dst, C.c_float)
    sc, R, t = np.zeros(1), np.zeros(9), np.zeros(3)
    out = (_lib.ptr(sc, C.c_double), _lib.ptr(R, C.c_double), _lib.ptr(t, C.c_double))

    def prm(**f):
        p = _lib.Sim3Params()
        L.vo_sim3_default_params(C.byref(p))
        for k, v in f.items():
            setattr(p, k, v)
        return C.byref(p)

    bad = dict(threshold_zero=prm(threshold=0.0), threshold_negative=prm(threshold=-1.0), threshold_nan=prm(threshold=float("nan")),
               confidence_zero=prm(confidence=0.0), confidence_one=prm(confidence=1.0), max_iters_zero=prm(max_iters=0),
               with_scale_two=prm(with_scale=2), with_scale_negative=prm(with_scale=-1), refit_two=prm(refit=2), refit_negative=prm(refit=-1))
    for name, p in bad.items():
        rc = L.vo_sim3_ransac(h, ps, pd, 64, p, *out, None, None, None)
        print("vo_sim3_ransac %s -> %d" % (name, rc))
        assert rc == VO_E_INVALID, name
    assert L.vo_sim3_ransac(h, ps, pd, 2, prm(), *out, None, None, None) == VO_E_INVALID
    assert L.vo_sim3_ransac(h, None, pd, 64, prm(), *out, None, None, None) == VO_E_INVALID
    assert L.vo_sim3_ransac(h, ps, None, 64, prm(), *out, None, None, None) == VO_E_INVALID
    assert L.vo_sim3_fit(h, ps, pd, None, 2, 1, *out, None) == VO_E_INVALID
    assert L.vo_sim3_fit(h, None, pd, None, 64, 1, *out, None) == VO_E_INVALID
    assert L.vo_sim3_fit(h, ps, pd, None, 64, 2, *out, None) == VO_E_INVALID
    assert L.vo_sim3_ransac(h, ps, pd, 64, prm(threshold=sm.THR, seed=sm.SEARCH_SEED), None, None, None, None, None, None) == 0     # every output may be NULL
    assert _same_result(before, _call(ctx, s, kw))
