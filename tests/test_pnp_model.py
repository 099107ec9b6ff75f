"""CPU-only: the model of tests/pnp_model.py certifies itself, its scenes are what their names say, and every bound the GPU test
(test_gpu_pnp_model.py) asserts on the kernel holds for oracle/pnp_oracle.py, the same algorithm in float64 on the CPU.

The verdict functions are the model's (judge_*): the GPU test applies the very same ones.  Each test prints the maxima it measured; the
constants of pnp_model.py that are "measured" were fixed from the MODEL's figures in these prints (worst case x the stated margin), the
others from the derivations beside them; none from the oracle's or the kernel's output.

What the oracle (and the kernel, which restates it) still misses is recorded here as strict expected failures with the figures."""
import math

import numpy as np
import pytest

import pnp_model as pm

N_SETS = 400                      # three-point sets per kind
_P3P = {}


def _bearings64(K, uv):
    """unit bearings the way the library forms them (oracle hypothesis()): inverse of K times the pixel, normalised, float64"""
    Kinv = np.linalg.inv(K)
    out = []
    for u, v in uv:
        b = Kinv @ np.array([u, v, 1.0])
        out.append(b / math.sqrt(np.dot(b, b)))
    return out


def _oracle_p3p(kind):
    """kind -> list of judge_p3p verdicts of po.p3p over the N_SETS exact float64 sets"""
    import pnp_oracle as po
    if kind not in _P3P:
        out = []
        for seed in range(N_SETS):
            p = pm.triple(kind, seed)
            poses = po.p3p(_bearings64(p["K"], p["uv"][:3]), [p["X"][i] for i in range(3)])
            out.append(pm.judge_p3p(poses, p))
        _P3P[kind] = out
    return _P3P[kind]


def _oracle_call(K, X, uv, thr=2.0, seed=0, max_iters=1000000, conf=0.9999):
    """po.pnp_ransac in the shape VoContext.pnp_ransac returns"""
    import pnp_oracle as po
    r, t, inl, info = po.pnp_ransac(K, X, uv, thr=thr, conf=conf, max_iters=max_iters, seed=seed, return_info=True)
    if r is None:
        return dict(rvec=np.full(3, np.nan), t=np.full(3, np.nan), inl=inl, st=dict(cost=np.nan, n_inliers=0, hypotheses=info["hyps"], best=-1, status=-4))
    return dict(rvec=r, t=t, inl=inl, st=dict(cost=info["cost"], n_inliers=len(inl), hypotheses=info["hyps"], best=info["best"], status=0))


# ---- the model certifies itself ------------------------------------------------------------------------------------------------------------
def test_model_certifies_itself_and_finds_the_planted_pose():
    for kind in pm.P3P_KINDS:
        w_eq = w_px = w_pl = 0.0
        n_sol = n_unc = n_low = 0
        for seed in range(N_SETS):
            p = pm.triple(kind, seed)
            sols = p["sol"]["sols"]
            n_sol += len(sols); n_unc += len(p["sol"]["uncertified"])
            assert 1 <= len(sols) <= 4, (kind, seed, len(sols))
            for s in sols:
                w_eq, w_px = max(w_eq, s["res_eq"]), max(w_px, s["res_px"])
                assert s["res_eq"] <= pm.RES_EQ_MAX and s["res_px"] <= pm.RES_PX_MAX
                assert abs(np.linalg.det(s["R"]) - 1) <= 64 * pm.EPS and (s["s"] > 0).all()
                n_low += s["sigma_px"] < pm.SIGMA_PX_CUT
            # the planted pose is a solution of the exact set: within the model's own certificate over the conditioning
            d = [(pm.pose_dist(s["r"], s["t"], p["r"], p["t"], s["zbar"]), s) for s in sols]
            dmin, s = min(d, key=lambda x: x[0])
            bound = pm.ROOT_MARGIN * pm.RES_PX_MAX / s["sigma_px"]
            w_pl = max(w_pl, dmin / bound)
            assert dmin <= bound, (kind, seed, dmin, bound)
        print("pnp model %-11s: %4d certified solutions (%d real candidates did not certify), equation residual %.2e, own three points %.2e px, "
              "planted pose within %.2e of its bound, %d solutions under SIGMA_PX_CUT" % (kind, n_sol, n_unc, w_eq, w_px, w_pl, n_low))
        assert n_low <= pm.EXCUSED_MAX * n_sol


def _constructed(kind):
    """camera-frame triangles with a known number of solutions (Fischler & Bolles 1981: an equilateral triangle seen from near its axis has
    four; a generic scalene triangle in front of the camera has two), shifted off the symmetry so that no two roots come close"""
    K = pm.K0
    if kind == "four":
        Xc = np.array([[2.0 * math.cos(a) + 0.15, 2.0 * math.sin(a) - 0.1, 3.0 + 0.2 * math.cos(2 * a)] for a in (0.3, 0.3 + 2.1, 0.3 + 4.2)])
    else:
        Xc = np.array([[-3.0, 1.0, 12.0], [4.0, -0.5, 14.0], [0.5, 1.5, 10.0]])
    r, t = pm.kind_pose("general")
    X = pm.to_world(Xc, r, t)
    return K, X, pm.project(K, pm.rodrigues(r), t, X)


@pytest.mark.parametrize("kind,n", [("four", 4), ("two", 2)])
def test_model_counts_the_solutions(kind, n):
    K, X, uv = _constructed(kind)
    sol = pm.p3p(K, X, uv)
    assert pm.count_by_scan(K, X, uv) == n
    assert len(sol["sols"]) == n and not sol["uncertified"]
    sep = min(pm.pose_dist(a["r"], a["t"], b["r"], b["t"], a["zbar"]) for i, a in enumerate(sol["sols"]) for b in sol["sols"][i + 1:])
    print("pnp model constructed %s-solution set: %d certified, %d by the scan, closest pair %.3f apart" % (kind, len(sol["sols"]), n, sep))
    assert sep > 1e-2


def test_model_is_order_independent():
    """the same three points in another order: the same set of poses"""
    p = pm.triple("general", 3)
    a = pm.p3p(p["K"], p["X"][:3], p["uv"][:3])["sols"]
    b = pm.p3p(p["K"], p["X"][[2, 0, 1]], p["uv"][[2, 0, 1]])["sols"]
    assert len(a) == len(b)
    for s in a:
        assert min(pm.pose_dist(s["r"], s["t"], o["r"], o["t"], s["zbar"]) for o in b) <= pm.ROOT_MARGIN * pm.RES_PX_MAX / s["sigma_px"]


def test_scenes_are_what_their_names_say():
    for kind in pm.P3P_KINDS:
        p = pm.triple(kind, 5)
        Xc = p["X"][:3] @ pm.rodrigues(p["r"]).T + p["t"]
        d = [np.linalg.norm(Xc[i] - Xc[j]) for i, j in ((1, 2), (0, 2), (0, 1))]
        if kind == "plane":
            assert np.ptp(Xc[:, 2]) <= 1e-9
        elif kind == "far":
            assert (Xc[:, 2] >= 200).all()
        elif kind == "cluster":
            assert max(d) <= 0.05 * math.sqrt(3) and (Xc[:, 2] > 9).all()
        elif kind == "equilateral":
            assert np.ptp(d) <= 1e-2 and np.ptp(np.hypot(Xc[:, 0], Xc[:, 1])) <= 1e-2
        elif kind == "isosceles":
            assert abs(d[1] - d[2]) <= 1e-9
        elif kind == "collinear":
            assert np.linalg.norm(np.cross(Xc[1] - Xc[0], Xc[2] - Xc[0])) <= 1e-2 * max(d) ** 2
    for kind in ("rot_pi", "rot_zero"):
        th = np.linalg.norm(pm.kind_pose(kind)[0])
        assert (math.pi - 1e-5 < th < math.pi) if kind == "rot_pi" else (0 < th < 1e-9)
    s = pm.scene("behind", 40)
    z = (s["X"].astype(float) @ pm.rodrigues(s["r"]).T + s["t"])[:, 2]
    assert (z[s["behind"]] < 0).all() and (z[~s["behind"]] > 0).all() and s["behind"].sum() == 8
    assert pm.kind_K("skew")[0, 1] != 0 and np.array_equal(pm.kind_K("k2"), 2 * pm.K0)


# ---- the oracle's P3P inside the verdicts --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", pm.P3P_KINDS)
def test_oracle_p3p_backward_error(kind):
    """every pose po.p3p returns reprojects the three points it was solved from within P3P_BACK_PX.
    Before the depth-equation polish (Grunert's quartic + two Newton steps alone) the worst of these 400 sets was: general 1.8e-6, plane 74,
    far 1.2e-5, cluster 7.0, equilateral 4.9, isosceles 1.6e-4, collinear 2.8e-3 px; with it 1.2e-8, 8.1e-9, 1.3e-8, 6.0e-9, 1.8e-8, 1.6e-9, 4.9e-9."""
    J = _oracle_p3p(kind)
    worst = max(j["worst_back"] for j in J)
    print("pnp oracle %-11s: backward error on its own three points at most %.2e px over %d sets, %d poses" % (kind, worst, len(J), sum(j["n_poses"] for j in J)))
    assert all(j["back_ok"] for j in J), [(i, j["worst_back"]) for i, j in enumerate(J) if not j["back_ok"]][:5]


# Sets whose roots the refined solver still loses, by seed, with what was measured.  A change of this list in either direction fails.
KNOWN_MISSED_SETS = {
    # Grunert's coefficients are differences of cosines that all lie within 1e-6 of 1 for a triangle of under a pixel (5 cm at 10-40 m): the
    # quartic keeps four or five digits.  22 of the 400 sets come out with four complex roots (no pose at all); set 5 returns poses, the
    # nearest 2.7 (pose_dist) from the lost root.
    "cluster": (5, 9, 18, 23, 45, 50, 92, 93, 127, 128, 137, 161, 210, 218, 225, 243, 247, 258, 265, 291, 376, 384, 385),
    # two of the four roots of set 242 are lost, nearest returned poses 9.7e-2 and 0.17 away; before the split double roots and the quadratic
    # for u were handled it was 17 sets
    "equilateral": (242,),
}


def _missed_sets(kind):
    return [i for i, j in enumerate(_oracle_p3p(kind)) if not j["roots_ok"]]


@pytest.mark.parametrize("kind", pm.P3P_KINDS)
def test_oracle_p3p_finds_every_root(kind):
    """every certified model solution over SIGMA_PX_CUT has an oracle pose within ROOT_MARGIN x beta / sigma_px -- in every set but the
    documented ones, and those are exactly the ones that miss"""
    J = _oracle_p3p(kind)
    known = KNOWN_MISSED_SETS.get(kind, ())
    worst = max(j["worst_root"] for i, j in enumerate(J) if i not in known)
    n_roots, excused = sum(j["n_roots"] for j in J), sum(j["excused"] for j in J)
    missed = _missed_sets(kind)
    print("pnp oracle %-11s: %d roots, %d excused under SIGMA_PX_CUT, nearest pose at most %.2e of the bound outside the documented sets; sets with a "
          "missed root: %d %s" % (kind, n_roots, excused, worst, len(missed), [(i, ["%.2e" % d for d in J[i]["missed"]]) for i in missed[:3]]))
    assert excused <= pm.EXCUSED_MAX * n_roots
    assert missed == list(known), (missed, known)


@pytest.mark.parametrize("kind", [pytest.param("cluster", marks=pytest.mark.xfail(strict=True, reason="23 of 400 sets of three points within 5 cm at 10-40 m "
                                               "lose their roots in Grunert's quartic; nearest returned pose 2.7 away in set 5, none returned in the other 22")),
                                  pytest.param("equilateral", marks=pytest.mark.xfail(strict=True, reason="set 242 of 400 near-equilateral sets loses two of its four "
                                               "roots; nearest returned poses 9.7e-2 and 0.17 away"))])
def test_oracle_p3p_documented_misses_are_found(kind):
    """what remains: passes (and then fails the suite, strictly) once the solver finds every root of the kind"""
    assert not _missed_sets(kind)


def test_oracle_quartic_roots():
    """po.quartic_real_roots against quartics built from four known real roots: a pair 0.05 .. 1e-5 apart, and roots spread over 1e-5 .. 2e3,
    where the shift x = y - a / 4 of the depressed quartic leaves the smallest root 1e-11 relative and only the two Newton steps on the
    original quartic restore it (Ferrari alone: 3e9 .. 2e13 of the bound below, one step: 28 .. 1e7, two: 0.5).
    Bound: Horner's value of f at x carries at most gamma_8 sum |c_k| |x|^k = 8 eps sum |c_k| |x|^k (Higham, Accuracy and Stability, 5.1), so a
    Newton iteration on f cannot do better and a converged one does as well: |x - x*| <= 8 eps cond, cond = sum |c_k| |x|^k / |f'(x)|; x 2 for
    the rounding of f' and of the coefficients np.poly hands over: 16 eps cond.  The exact roots are those of the rounded coefficients, by
    Newton in longdouble."""
    import pnp_oracle as po
    rng = np.random.default_rng(0)
    worst = 0.0
    for it in range(600):
        if it % 6 < 4:
            gap = (0.05, 1e-2, 1e-3, 1e-5)[it % 6]
            b = rng.uniform(1.2, 1.8)
            r = np.array([rng.uniform(0.3, 0.9), b, b + gap * rng.uniform(1, 2), rng.uniform(2.2, 3.0)])
        else:
            small, big = ((1e-3, 3e2), (1e-5, 1e3))[it % 6 - 4]
            r = np.array([small * rng.uniform(1, 2), rng.uniform(0.3, 0.9), rng.uniform(1.5, 3), big * rng.uniform(1, 2)])
        c = rng.uniform(0.5, 3) * np.poly(r)
        got = po.quartic_real_roots(*c)
        assert len(got) == 4, (it, r, got)
        cl = c.astype(np.longdouble)
        for x in r:
            xl = np.longdouble(x)
            for _ in range(6 if it % 6 >= 4 else 0):         # (a close pair keeps np.poly's own root: Newton in longdouble is no better there)
                xl = xl - np.polyval(cl, xl) / np.polyval(np.polyder(cl), xl)
            cond = (np.abs(c) * np.abs(x) ** np.arange(4, -1, -1)).sum() / abs(np.polyval(np.polyder(c), x))
            e = float(min(abs(np.longdouble(g) - xl) for g in got)) / (pm.EPS * cond)
            worst = max(worst, e)
            assert e <= 16, (it, x, e)
    print("pnp oracle quartic: roots within %.2f eps x condition number" % worst)
    assert po.quartic_real_roots(0.0, 1.0, 1.0, 1.0, 1.0) == [] and po.quartic_real_roots(1.0, 0.0, 1.0, 0.0, 1.0) == []


# ---- (a) every root through a fourth correspondence ----------------------------------------------------------------------------------------
def _fourth_oracle(kind):
    fc = pm.fourth_calls(kind)
    return [_oracle_call(c["K"], c["X"], c["uv"], thr=fc["thr"], seed=pm.FOURTH_SEED, max_iters=288) for c in fc["calls"]]


@pytest.mark.parametrize("kind", pm.P3P_KINDS)
def test_fourth_point_calls_model_and_oracle(kind):
    fc = pm.fourth_calls(kind)
    calls, thr = fc["calls"], fc["thr"]
    assert len(fc["seeds"]) == pm.FOURTH_SETS and thr <= pm.FOURTH_MARGIN * pm.FOURTH_FLOOR_MAX
    # the model alone: the calls in which hypothesis 0 is not one it vouches for (so that an excuse is possible at all) stay under the cap
    open_calls = sum(1 for c in calls if pm.judge_fourth(dict(rvec=c["sol"]["r"], t=c["sol"]["t"], inl=np.arange(4),
                                                              st=dict(status=0, n_inliers=4, hypotheses=32, best=0, cost=0.0)), c, thr)["excused"])
    assert open_calls <= pm.EXCUSED_MAX * len(calls), (len(calls), open_calls)
    assert set(pm.FOURTH_KNOWN_MISSES.get(kind, ())) <= {(c["seed"], c["k"]) for c in calls}
    v = pm.fourth_verdicts(kind, _fourth_oracle(kind))
    print("pnp oracle %-11s: %d fourth-point calls (sets %d .. %d) at threshold %.3e px, %d open to an excuse by the model, %d excused; stationarity at most %.2e, "
          "distance to the model's minimiser at most %.2e of its bound; failing: %d %s" % (kind, len(calls), fc["seeds"][0], fc["seeds"][-1], thr, open_calls,
                                                                                           v["excused"], v["stat"], v["dist_ratio"], len(v["failing"]), sorted(v["failing"])))
    pm.check_fourth(kind, v, exact=True)


@pytest.mark.parametrize("kind", [pytest.param("cluster", marks=pytest.mark.xfail(strict=True, reason="5 of the 32 float32 sets of three points within 5 cm (10 calls): "
                                               "hypothesis 0 finds no pose, the quartic's roots come out complex")),
                                  pytest.param("collinear", marks=pytest.mark.xfail(strict=True, reason="call (18, 1): hypothesis 0 lands 0.22 (pose_dist) from its root, on "
                                               "the neighbouring one, at sigma_px 0.016"))])
def test_fourth_point_documented_misses_are_found(kind):
    """what remains: passes (and then fails the suite, strictly) once hypothesis 0 reaches the root in every documented call"""
    assert not pm.fourth_verdicts(kind, _fourth_oracle(kind))["failing"]


# ---- (b) winner, consensus, minimiser, iteration bound on full problems --------------------------------------------------------------------
@pytest.mark.parametrize("n", [40, 200])
def test_oracle_winner_on_full_problems(n):
    w = dict(stat=0.0, dist_ratio=0.0, cost_rel=0.0)
    n_border = n_diff = 0
    for kind in pm.KINDS:
        s = pm.scene(kind, n)
        res = _oracle_call(s["K"], s["X"], s["uv"], seed=7)
        j = pm.judge_winner(res, s, seed=7)
        assert all(j[k] for k in pm.WINNER_KEYS), (kind, n, {k: j[k] for k in pm.WINNER_KEYS}, j)
        for k in w:
            w[k] = max(w[k], j[k])
        n_border += j["n_border"]; n_diff += j["n_diff"]
        assert len(np.intersect1d(res["inl"], s["true_inl"])) >= 0.9 * len(s["true_inl"]), kind
        if kind == "behind":                               # the contract: no cheirality test
            assert s["behind"][res["inl"]].sum() >= 0.9 * s["behind"][s["true_inl"]].sum() > 0
    print("pnp oracle full problems n = %d: stationarity at most %.2e (bound %.0e), distance to the model's minimiser %.2e of its bound, cost %.2e "
          "relative, %d borderline points, %d differing" % (n, w["stat"], pm.STAT_TOL, w["dist_ratio"], w["cost_rel"], n_border, n_diff))


def test_oracle_refine_from_a_perturbed_start():
    """po.refine alone, from 1e-2 off the planted pose, over the true inliers: a stationary point, the model's minimiser"""
    import pnp_oracle as po
    worst = 0.0
    for kind in ("general", "plane", "rot_pi", "rot_zero", "skew"):
        s = pm.scene(kind, 200)
        idx = s["true_inl"]
        X, uv = s["X"].astype(float), s["uv"].astype(float)
        R0 = pm.rodrigues(np.array([0.004, -0.006, 0.003])) @ pm.rodrigues(s["r"])
        r, t, c = po.refine(s["K"], pm.rotvec(R0), s["t"] + [0.01, -0.01, 0.02], X[idx], uv[idx])
        j = pm.judge_minimiser(dict(rvec=r, t=t, cost=c), s["K"], X, uv, idx)
        worst = max(worst, j["stat"])
        assert j["stationary"] and j["agrees"] and j["cost_ok"], (kind, j)
    print("pnp oracle refine: stationarity at most %.2e" % worst)


def test_hypotheses_bounds_formula():
    # 70 % inliers at 0.9999: log(1e-4) / log(1 - 0.7^4) = 33.5 -> two batches; 50 %: 142.7 -> 288; all inliers: the first batch
    assert abs(pm.need_iters(100, 70, 0.9999) - math.log(1e-4) / math.log(1 - 0.7 ** 4)) < 1e-9
    assert pm.hypotheses_bounds(100, 70, best=3) == (288, 288)
    assert pm.hypotheses_bounds(100, 100, best=0) == (32, 32) and pm.hypotheses_bounds(100, 100, best=40) == (288, 288)
    assert pm.hypotheses_bounds(100, 98, best=5) == (32, 32)
    assert pm.hypotheses_bounds(100, 10, max_iters=288, best=100) == (288, 288)
    assert pm.batch_end(1) == 32 and pm.batch_end(32) == 32 and pm.batch_end(33) == 288 and pm.batch_end(289) == 544
    import pnp_oracle as po
    for n, c in ((40, 28), (200, 140), (200, 101), (1000, 333)):
        lo, hi = pm.hypotheses_bounds(n, c, best=0)
        assert lo <= pm.batch_end(max(1, po.update_num_iters(0.9999, (n - c) / n, 4, 1000000))) <= hi


def test_consensus_contract():
    K = pm.K0
    R, t = np.eye(3), np.zeros(3)
    X = np.array([[1.0, 0.5, 10.0], [-1.0, -0.5, -10.0], [1.0, 0.5, 10.0], [np.nan, 0.0, 5.0], [1.0, 1.0, 0.0], [2.0, 1.0, 10.0]])
    uv = pm.project(K, R, t, X[:1]).repeat(6, 0)
    uv[2] += [2.0, 0.0]                                     # exactly on the threshold: inside, and flagged
    uv[5] = [np.nan, 3.0]
    c = pm.consensus(K, R, t, X, uv, 2.0)
    assert c["inl"].tolist() == [True, True, True, False, False, False]      # behind the camera counts; NaN rows and p2 == 0 never do
    assert c["border"].tolist() == [False, False, True, False, False, False]
    far = uv.copy(); far[2] += [1e-6, 0.0]
    assert not pm.consensus(K, R, t, X, far, 2.0)["border"][2]


def test_rotation_branches_of_the_oracle():
    """po.rodrigues / po.log_so3 near pi and near 0 against scipy's quaternion route.  Within 1e-2 of pi the angle comes from atan2 and the axis
    from the symmetric part: a few eps of pi.  Outside, th / (2 sin th) with th = acos(c) loses eps / gap^2 relative (1 + c = gap^2 / 2 is a
    difference of numbers of size 1).  Before the fix the acos branch ran down to pi - 1e-6: 6e-6 rad off at pi - 1e-5, 2e-4 at pi - 2e-6."""
    import pnp_oracle as po
    worst_in = worst_out = 0.0
    for gap in (1e-12, 1e-8, 3e-7, 2e-6, 0.6e-5, 1e-4, 0.99e-2, 1.01e-2, 0.1, 1.0):
        for ax in (pm._AXIS, np.array([1.0, 0.0, 0.0]), np.array([0.6, 0.0, -0.8]), np.array([0.0, -1.0, 0.0])):
            r = ax * (math.pi - gap)
            R = po.rodrigues(r)
            assert np.abs(R - pm.rodrigues(r)).max() <= 8 * pm.EPS
            err = np.abs(po.log_so3(R) - r).max()
            assert err <= np.abs(pm.rotvec(R) - r).max() + (16 * pm.EPS * math.pi if gap < 1e-2 else 16 * pm.EPS * math.pi / gap ** 2), (gap, ax, err)
            if gap < 1e-2:
                worst_in = max(worst_in, err)
            else:
                worst_out = max(worst_out, err * gap ** 2)
    for th in (0.7e-9, 3e-13, 1e-6):
        r = pm._AXIS * th
        R = po.rodrigues(r)
        assert np.abs(R - pm.rodrigues(r)).max() <= 8 * pm.EPS
        assert np.abs(po.log_so3(R) - r).max() <= 8 * pm.EPS
    print("pnp oracle log_so3: within 1e-2 of pi off by at most %.2e rad, outside by at most %.2e / gap^2" % (worst_in, worst_out))
