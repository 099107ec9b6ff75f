"""GPU: P3P RANSAC + refinement (csrc/vo_pnp.hip) against the independent float64 model of tests/pnp_model.py, through VoContext.pnp_ransac and
the resident calls only.

The model solves P3P by another route (resultant in the other depth ratio, companion eigenvalues, Newton in longdouble, Kabsch), certifies
every solution by its own residuals and scales every tolerance by the conditioning; consensus is true division with a borderline flag, the
minimiser is scipy's LM with a complex-step Jacobian.  tests/test_pnp_model.py shows on the CPU that the oracle stays inside the very same
verdict functions (judge_*) and records where each constant comes from.  The one thing taken from oracle/pnp_oracle.py is `sample4`, the
documented draw of hypothesis `best` (were the kernel to draw otherwise, the model would find no consensus next to the returned one).
Covered: every root of 32 three-point sets per kind through a fourth correspondence, the winner on full problems of every scene kind, the
sizes where the kernels' strides end, the rotation / K / cheirality / degenerate-sample edges, and bit-for-bit structure tests."""
import numpy as np
import pytest

import pnp_model as pm

pytestmark = pytest.mark.gpu
SEED = 7


def _stack(items):
    return np.stack([np.asarray(x) for x in items])


def _call_batch(problems, **kw):
    """problems: list of (K, X, uv) of one n -> list of dict rvec, t, inl, st (one batched context, one call)"""
    from vo_mi355x import VoContext
    B = len(problems)
    with VoContext(64, 64, max_pts=64, batch=B) as c:
        out = c.pnp_ransac(_stack([p[0] for p in problems]), _stack([p[1] for p in problems]), _stack([p[2] for p in problems]), **kw)
    if B == 1:
        return [dict(zip(("rvec", "t", "inl", "st"), out))]
    return [dict(rvec=out[0][b], t=out[1][b], inl=out[2][b], st=out[3][b]) for b in range(B)]


def _call(c, s, **kw):
    return dict(zip(("rvec", "t", "inl", "st"), c.pnp_ransac(s["K"], s["X"], s["uv"], **kw)))


def _same(a, b):
    return pm.bits_equal(a["rvec"], b["rvec"]) and pm.bits_equal(a["t"], b["t"]) and np.array_equal(a["inl"], b["inl"]) and a["st"] == b["st"]


def _judge_all(results, scenes, what, **kw):
    """judge_winner on every (result, scene); asserts the named verdicts, prints the worst ratios"""
    w = dict(stat=0.0, dist_ratio=0.0, cost_rel=0.0)
    n_border = n_diff = 0
    for res, s in zip(results, scenes):
        j = pm.judge_winner(res, s, seed=SEED, **kw)
        assert all(j[k] for k in pm.WINNER_KEYS), (what, s["kind"], s["n"], {k: j[k] for k in pm.WINNER_KEYS}, j)
        assert j["nan_free"] and np.isfinite(res["rvec"]).all() and np.isfinite(res["t"]).all()
        for k in w:
            w[k] = max(w[k], j[k])
        n_border += j["n_border"]; n_diff += j["n_diff"]
    print("pnp kernel %s: %d problems, stationarity at most %.2e (bound %.0e), distance to the model's minimiser %.2e of its bound, cost %.2e relative, "
          "%d borderline points, %d differing" % (what, len(scenes), w["stat"], pm.STAT_TOL, w["dist_ratio"], w["cost_rel"], n_border, n_diff))


@pytest.fixture(scope="module")
def ctx():
    from vo_mi355x import VoContext
    with VoContext(64, 64, max_pts=64) as c:
        yield c


# ---- (a) every root through a fourth correspondence ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", pm.P3P_KINDS)
def test_every_root_through_a_fourth_point(kind):
    """every call passes every verdict; only the calls pnp_model.FOURTH_KNOWN_MISSES names (roots the refined solver is documented to lose
    from hypothesis 0; tests/test_pnp_model.py pins them exactly on the CPU) may fail, and on `best_ok` alone"""
    fc = pm.fourth_calls(kind)
    res = _call_batch([(c["K"], c["X"], c["uv"]) for c in fc["calls"]], reproj_err=fc["thr"], max_iters=288, seed=pm.FOURTH_SEED)
    v = pm.fourth_verdicts(kind, res)
    print("pnp kernel %-11s: %d fourth-point calls at threshold %.3e px, %d excused; stationarity at most %.2e, distance to the model's minimiser "
          "at most %.2e of its bound; failing: %d %s" % (kind, v["n"], v["thr"], v["excused"], v["stat"], v["dist_ratio"], len(v["failing"]), sorted(v["failing"])))
    pm.check_fourth(kind, v, exact=False)


# ---- (b) winner on full problems -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [40, 200])
def test_winner_on_full_problems_of_every_kind(n):
    scenes = [pm.scene(kind, n) for kind in pm.KINDS]
    res = _call_batch([(s["K"], s["X"], s["uv"]) for s in scenes], seed=SEED)
    _judge_all(res, scenes, "full problems n = %d" % n)
    for s, r in zip(scenes, res):
        assert len(np.intersect1d(r["inl"], s["true_inl"])) >= 0.9 * len(s["true_inl"]), s["kind"]
        if s["kind"] == "behind":                          # the contract: no cheirality test, a point behind the camera counts
            assert s["behind"][r["inl"]].sum() >= 0.9 * s["behind"][s["true_inl"]].sum() > 0


# ---- (c) sizes where the kernels' strides end --------------------------------------------------------------------------------------------------
SIZES = (4097, 4096, 4095, 2049, 2048, 2047, 513, 512, 511, 257, 256, 255)     # descending: the context grows its buffers once


def test_sizes_where_the_strides_end(ctx):
    scenes = [pm.scene("general", n) for n in SIZES]
    _judge_all([_call(ctx, s, seed=SEED) for s in scenes], scenes, "stride ends")


@pytest.mark.parametrize("n", [4097, 2049, 513, 257])
def test_last_point_beyond_a_boundary(ctx, n):
    # the last point is the only outlier
    a = pm.scene("general", n, seed=3, frac_out=0.0)
    a["uv"][-1] += np.float32(50.0)
    a["true_inl"] = np.arange(n - 1)
    ra = _call(ctx, a, seed=SEED)
    # the last point is the only inlier beyond the boundary (the scene's own outliers stay; the last point is put back on its projection)
    b = pm.scene("general", n, seed=4)
    b["uv"][-1] = pm.project(b["K"], pm.rodrigues(b["r"]), b["t"], b["X"][-1:].astype(float))[0].astype(np.float32)
    rb = _call(ctx, b, seed=SEED)
    _judge_all([ra, rb], [a, b], "last point beyond %d" % (n - 1))
    assert n - 1 not in ra["inl"] and len(ra["inl"]) >= 0.95 * (n - 1)
    assert n - 1 in rb["inl"]


def test_two_nan_padded_lengths_across_a_boundary():
    a = pm.scene("general", 513, seed=5)
    b = pm.scene("plane", 511, seed=5)
    pad = lambda x: np.concatenate([x, np.full((2,) + x.shape[1:], np.nan, np.float32)])
    b = dict(b, n=513, X=pad(b["X"]), uv=pad(b["uv"]))
    res = _call_batch([(a["K"], a["X"], a["uv"]), (b["K"], b["X"], b["uv"])], seed=SEED)
    _judge_all(res, [a, b], "NaN-padded 513 / 511")
    assert res[1]["inl"].max() < 511


# ---- (d) branch edges ----------------------------------------------------------------------------------------------------------------------------
def test_scale_of_K_does_not_matter():
    s = pm.scene("general", 200, seed=6)
    s2 = dict(s, K=2.0 * s["K"])
    r1, r2 = _call_batch([(s["K"], s["X"], s["uv"]), (s2["K"], s2["X"], s2["uv"])], seed=SEED)
    _judge_all([r1, r2], [s, s2], "K and 2 K")
    assert np.array_equal(r1["inl"], r2["inl"]) and r1["st"]["best"] == r2["st"]["best"]
    X, uv = s["X"].astype(float), s["uv"].astype(float)
    j = pm.judge_minimiser(dict(rvec=r1["rvec"], t=r1["t"], cost=r1["st"]["cost"]), s["K"], X, uv, r1["inl"])
    m = j["model"]
    d = np.hypot(np.linalg.norm(r1["rvec"] - r2["rvec"]), np.linalg.norm(r1["t"] - r2["t"]))
    bound = 2 * (pm.MIN_MARGIN * 2 * pm.STAT_TOL * m["jnorm"] * m["enorm"] / m["smin"] ** 2 + 64 * pm.EPS * m["jnorm"] / m["smin"] * (1 + m["xnorm"]))
    print("pnp kernel K and 2 K: poses %.2e apart (bound %.2e)" % (d, bound))
    assert d <= bound


def test_degenerate_samples():
    """duplicate points (draws with a2, b2 or c2 = 0) and exactly collinear triples: the model's answer, never a NaN pose with status 0"""
    s = pm.scene("general", 40, seed=8)
    dup = dict(s, X=s["X"].copy(), uv=s["uv"].copy())
    for i in range(0, 24, 3):                                # eight points, three times each
        dup["X"][i + 1] = dup["X"][i + 2] = dup["X"][i]
        dup["uv"][i + 1] = dup["uv"][i + 2] = dup["uv"][i]
    line = dict(s, X=s["X"].copy(), uv=s["uv"].copy())
    line["X"][:16] = (np.array([1.0, 0.5, 12.0]) + np.arange(16)[:, None] * np.array([0.25, -0.125, 0.5])).astype(np.float32)     # exact in float32
    line["uv"][:16] = pm.project(s["K"], pm.rodrigues(s["r"]), s["t"], line["X"][:16].astype(float)).astype(np.float32)
    same = dict(s, X=np.repeat(s["X"][:1], 40, 0), uv=np.repeat(s["uv"][:1], 40, 0))                                      # no sample has a triangle
    res = _call_batch([(x["K"], x["X"], x["uv"]) for x in (dup, line, same)], seed=SEED, max_iters=288)
    for x in (dup, line):
        x["true_inl"] = np.nonzero(pm.residuals(x["K"], pm.rodrigues(x["r"]), x["t"], x["X"].astype(float), x["uv"].astype(float)) < 1.5)[0]
    _judge_all(res[:2], [dup, line], "duplicates and collinear triples", max_iters=288)
    r = res[2]
    assert r["st"]["status"] != 0 and r["st"]["n_inliers"] == 0 and len(r["inl"]) == 0, r["st"]
    for r in res:
        assert r["st"]["status"] != 0 or (np.isfinite(r["rvec"]).all() and np.isfinite(r["t"]).all())


# ---- (e) structure -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [600, 3000, 5000])             # one problem per refine form: 4 and 8 points per thread in registers, memory
def test_resident_repeat_and_synchronous_are_bit_equal(ctx, n):
    s = pm.scene("general", n, seed=9)
    a = _call(ctx, s, seed=SEED)
    b = _call(ctx, s, seed=SEED)
    assert _same(a, b)
    ctx.pnp_upload(s["K"], s["X"], s["uv"])
    ctx.pnp_solve_resident(ctx.pnp_params(seed=SEED), blind_batches=2)
    c = dict(zip(("rvec", "t", "inl", "st"), ctx.pnp_fetch()))
    assert _same(a, c), (a["st"], c["st"])


def test_two_seeds_with_one_consensus_set_agree(ctx):
    s = pm.scene("general", 200, seed=10, noise=0.05)       # low noise: the consensus set is the set of true inliers for every good sample
    X, uv = s["X"].astype(float), s["uv"].astype(float)
    res = [_call(ctx, s, seed=k) for k in (1, 2, 3, 4)]
    pairs = [(a, b) for i, a in enumerate(res) for b in res[i + 1:] if np.array_equal(a["inl"], b["inl"])]
    assert pairs, [len(r["inl"]) for r in res]
    worst = 0.0
    for a, b in pairs:
        m = pm.judge_minimiser(dict(rvec=a["rvec"], t=a["t"], cost=a["st"]["cost"]), s["K"], X, uv, a["inl"])["model"]
        bound = 2 * (pm.MIN_MARGIN * 2 * pm.STAT_TOL * m["jnorm"] * m["enorm"] / m["smin"] ** 2 + 64 * pm.EPS * m["jnorm"] / m["smin"] * (1 + m["xnorm"]))
        d = np.hypot(np.linalg.norm(a["rvec"] - b["rvec"]), np.linalg.norm(a["t"] - b["t"]))
        worst = max(worst, d / bound)
        assert d <= bound, (d, bound)
    print("pnp kernel two seeds, one consensus set: %d pairs, poses at most %.2e of the bound apart" % (len(pairs), worst))
