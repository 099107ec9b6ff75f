"""GPU: every exit and branch of the bundle adjustment's LM loop (`ba_decide`, csrc/vo_ba.hip) against the float64 oracle, on the scenario table
of tests/ba_lm_cases.py (tests/test_ba_lm_cases.py proves on the CPU that each case reaches what it is named for, with margin).

The ABI returns only the final state, so a case whose oracle run takes T iterations is solved with max_iters = 1 .. T: prefix k is compared
with ba_oracle.solve(max_iters=k), and lambda after k iterations over lambda after k - 1 is the damping update iteration k made."""
import functools

import numpy as np
import pytest

import ba_lm_cases as lc

pytestmark = pytest.mark.gpu

STAT_KEYS = ("cost0", "cost", "lam", "iters", "accepted", "status")


@pytest.fixture(autouse=True, params=["wave_private", "lane_per_observation"])
def ba_kernels(request, monkeypatch, ctx):
    """every test of this module runs through BOTH kernel families (see tests/test_gpu_ba.py)"""
    from vo_mi355x import VoContext
    fam = 2 if request.param == "wave_private" else 1
    monkeypatch.setattr(VoContext, "default_tuning", {"ba_kernels": fam})
    ctx.set_tuning(ba_kernels=fam)
    return request.param


@pytest.fixture(scope="module")
def ctx():
    from vo_mi355x import VoContext
    c = VoContext(64, 64, max_pts=64)
    yield c
    c.close()


@functools.lru_cache(maxsize=None)
def _ref(name, k):
    """the oracle's run of a case cut at k iterations (None: the case's own max_iters); computed once, shared by both kernel families"""
    case = lc.BY_NAME.get(name) or {c["name"]: c for c in lc.BATCH}[name]
    return lc.reference(case, max_iters=k)


def _params(c, case, max_iters=None):
    p = lc.full_params(case)
    if max_iters is not None:
        p["max_iters"] = max_iters
    return c.ba_params(**p)


def _same(a, b):
    """two device results bit for bit: x and the state"""
    return (np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1], equal_nan=True)
            and all(a[2][k] == b[2][k] or (a[2][k] != a[2][k] and b[2][k] != b[2][k]) for k in STAT_KEYS))


def _solve(c, case, max_iters=None):
    """ba_adjust (chunks of 4 launch groups, a finalize and a host peek between them), and upload + resident solve + fetch (every launch made up
    front, no peek): the same bits"""
    K, poses0, points0, obs = lc.scene(case)
    prm = _params(c, case, max_iters)
    out = c.ba_adjust(K, poses0, points0, obs, prm)
    c.ba_upload(K, poses0, points0, obs)
    c.ba_solve_resident(prm)
    res = c.ba_fetch()
    assert _same(out, res), (case["name"], max_iters, out[2], res[2])
    return out


def _check_against_oracle(case, out, ref, tag):
    po, pt, st = out
    K, poses0, points0, obs = lc.scene(case)
    print(tag, {k: st[k] for k in STAT_KEYS}, "oracle", {k: ref[k] for k in ("cost0", "cost", "lam", "iters", "accepted", "status")})
    assert (st["iters"], st["accepted"], st["status"]) == (ref["iters"], ref["accepted"], ref["status"]), (tag, st, ref["iters"], ref["accepted"], ref["status"])
    assert abs(st["cost"] - ref["cost"]) <= 1e-7 * ref["cost"], (tag, st["cost"], ref["cost"])
    assert abs(st["cost0"] - ref["cost0"]) <= 1e-9 * ref["cost0"], (tag, st["cost0"], ref["cost0"])
    assert np.abs(po - ref["poses"]).max() <= 1e-6 and np.abs(pt - ref["points"]).max() <= 1e-5, tag
    if ref["accepted"] == 0:        # nothing accepted: the inputs come back bit for bit (a cut on a rejected step must not publish the trial)
        assert np.array_equal(po, poses0) and np.array_equal(pt, points0), tag
        assert st["cost"] == st["cost0"], tag


def _check_lambdas(case, lams, r, tag):
    """lams[k - 1]: the device's lambda after k iterations, k = 1 .. T; r: the oracle's classification of the case"""
    p = lc.full_params(case)
    prev, nu = p["lambda0"], 2.0
    third = 1.0 / 3.0
    for k, (lam, kind, f) in enumerate(zip(lams, r["kinds"], r["factors"]), 1):
        print(tag, "iteration", k, kind, "lambda", lam, "factor", lam / prev, "oracle", r["lams"][k - 1], f)
        if kind == "reject":
            leaves = r["exit"] == "xtol_reject" and k == len(r["kinds"])      # the rejected step that takes the xtol exit leaves lambda alone
            assert lam == (prev if leaves else prev * nu), (tag, k, lam, prev, nu)          # exact: a multiplication by a power of two
            nu *= 2.0
        else:
            nu = 2.0                                                   # an accepted step resets nu
            if kind == "accept-floored":
                assert lam == p["lambda_min"], (tag, k, lam)
            elif kind == "accept-clamped":
                assert abs(lam / prev - third) <= 4 * np.spacing(third), (tag, k, lam / prev)
            else:
                # loose on purpose: it tells 1 - (2 rho - 1)^3 from another formula, which moves an f >= 1/2 step by far more
                assert abs(lam / prev - f) <= 1e-2 * f, (tag, k, lam / prev, f)
        prev = lam


PREFIX_CASES = ["gtol_at_4_w2", "gtol_at_4_w4", "gtol_at_4_w10", "xtol_after_accept_w4", "xtol_after_accept_w10", "xtol_after_accept_w20",
                "ftol_floored_w4", "ftol_floored_w10", "rejections_w2", "rejections_w4", "rejections_w4b", "rejections_w10", "rejections_w10b",
                "unclamped_w4", "alternating_w10", "xtol_after_reject_w10", "xtol_after_reject_w4"]


@pytest.mark.parametrize("name", PREFIX_CASES)
def test_ba_lm_prefix_runs_follow_the_oracle(ctx, ba_kernels, name):
    """max_iters = 1 .. T, T + 1 and T + 2: iterations, accepted steps, status, cost, x and the damping update of every iteration = the oracle's;
    a cut with nothing accepted hands the inputs back bit for bit; a finished problem ignores the launch groups and the finalize behind its exit
    (the gtol exit is taken at the head of iteration T + 1, every other one at the end of iteration T); ba_adjust and the resident path agree
    bit for bit at every prefix."""
    case = lc.BY_NAME[name]
    r = lc.classify(case)
    T = r["ref"]["iters"]
    assert T >= 1
    outs = []
    for k in range(1, T + 3):
        out = _solve(ctx, case, k)
        _check_against_oracle(case, out, _ref(name, k), "%s[%s] prefix %d" % (name, ba_kernels, k))
        outs.append(out)
    _check_lambdas(case, [o[2]["lam"] for o in outs[:T]], r, "%s[%s]" % (name, ba_kernels))
    if case["exit"] in ("max_iters", "max_iters_reject"):          # (the case's own cut: the longer runs go on)
        assert outs[T - 1][2]["status"] == 0
        return
    left = T if case["exit"] == "gtol" else T - 1                  # index of the first run that saw the exit
    assert outs[left][2]["status"] == lc.STATUS[case["exit"]] == r["ref"]["status"]
    assert (case["exit"] == "gtol") == (outs[T - 1][2]["status"] == 0)
    for later in outs[left + 1:]:
        assert _same(later, outs[left]), (later[2], outs[left][2])


@pytest.mark.parametrize("name", [c["name"] for c in lc.FINITE])
def test_ba_lm_exits(ctx, ba_kernels, name):
    """every named exit with its literal status: gtol before the first step and at iteration 4, xtol behind an accepted and behind a rejected
    step, ftol, max_iters on both sides of the host's chunks of four (1, 3, 4, 5, 8) and on a rejected step"""
    case = lc.BY_NAME[name]
    ref = _ref(name, None)
    out = _solve(ctx, case)
    po, pt, st = out
    _check_against_oracle(case, out, ref, "%s[%s]" % (name, ba_kernels))
    assert st["status"] == lc.STATUS[case["exit"]]
    assert st["iters"] == case["iters"]
    assert st["lam"] == ref["lam"] or abs(st["lam"] - ref["lam"]) <= 1e-2 * ref["lam"]
    K, poses0, points0, obs = lc.scene(case)
    if case["exit"] == "gtol" and case["iters"] == 0:
        assert st["status"] == 1 and st["iters"] == 0 and st["accepted"] == 0
        assert st["cost"] == st["cost0"] and st["lam"] == lc.full_params(case)["lambda0"]
        assert np.array_equal(po, poses0) and np.array_equal(pt, points0)
    if case["exit"] == "max_iters_reject":
        # a cut on a rejected step answers with the last accepted x, not with the trial: the inputs while nothing was accepted, else the
        # device's own x after the accepted step before the run of rejections
        assert st["lam"] == ref["lam"]
        if ref["accepted"] == 0:
            assert np.array_equal(po, poses0) and np.array_equal(pt, points0)
        else:
            kinds = lc.classify(case)["kinds"]
            k_acc = max(i for i, kd in enumerate(kinds) if kd != "reject") + 1
            before = _solve(ctx, case, k_acc)
            assert np.array_equal(po, before[0]) and np.array_equal(pt, before[1])
            # (the cost of that x twice: as the trial cost of the accepted step, summed by the update kernel, and as the current cost of the
            #  rejected iterations, summed by the build kernel -- two orders of summing < 300 terms >= 0: n eps = 3e-14)
            assert abs(st["cost"] - before[2]["cost"]) <= 1e-12 * st["cost"]
            assert (st["accepted"], before[2]["iters"], st["iters"]) == (before[2]["accepted"], k_acc, case["iters"])


def test_ba_lm_mixed_batch(ctx, ba_kernels):
    """8 problems of one batch, clean and noisy in turn, 4 to 16 iterations, the noisy ones with rejected steps: rejections and early exits through the
    running-problem compaction (gdyn, ba2_select_work) and the fold path of k_ba_solve.  Every problem, at every cut, = the same problem solved
    alone (iterations, accepted steps, status; cost 1e-10, poses 1e-9), its final state = the oracle's, its damping updates the oracle's."""
    from vo_mi355x import VoContext
    B = len(lc.BATCH)
    cls = [lc.classify(c) for c in lc.BATCH]
    Ts = [r["ref"]["iters"] for r in cls]
    stack = lambda i: np.stack([lc.scene(c)[i] for c in lc.BATCH])
    ks = list(range(1, max(Ts) + 1)) + [None]
    batch = {}
    with VoContext(64, 64, max_pts=64, batch=B) as cb:
        for k in ks:
            batch[k] = cb.ba_adjust(stack(0), stack(1), stack(2), stack(3), _params(cb, lc.BATCH[0], k))
    for b, case in enumerate(lc.BATCH):
        K, poses0, points0, obs = lc.scene(case)
        lams = []
        for k in ks:
            po, pt, st = batch[k][0][b], batch[k][1][b], batch[k][2][b]
            if k is None or k <= Ts[b]:
                po1, pt1, st1 = ctx.ba_adjust(K, poses0, points0, obs, _params(ctx, case, k))
                alone = (po1, pt1, st1)
            else:
                po1, pt1, st1 = alone            # (the problem had finished: the last cut that still reached it)
            tag = "%s[%s] cut %s" % (case["name"], ba_kernels, k)
            print(tag, {q: st[q] for q in STAT_KEYS}, "alone", {q: st1[q] for q in STAT_KEYS})
            assert (st["iters"], st["accepted"], st["status"]) == (st1["iters"], st1["accepted"], st1["status"]), (tag, st, st1)
            assert abs(st["cost"] - st1["cost"]) <= 1e-10 * max(st1["cost"], 1e-30), (tag, st["cost"], st1["cost"])
            assert np.abs(po - po1).max() <= 1e-9, tag
            if k is not None and k <= Ts[b]:
                lams.append(st["lam"])
        _check_lambdas(case, lams, cls[b], "%s[%s]" % (case["name"], ba_kernels))
        po, pt, st = batch[None][0][b], batch[None][1][b], batch[None][2][b]
        _check_against_oracle(case, (po, pt, st), cls[b]["ref"], "%s[%s]" % (case["name"], ba_kernels))
        assert st["status"] == lc.STATUS[case["exit"]]
    its = [batch[None][2][b]["iters"] for b in range(B)]
    assert max(its) - min(its) >= 6, its


@pytest.mark.parametrize("name", ["nan_pose_w4", "nan_K_w4"])
def test_ba_lm_non_finite_problem(ctx, ba_kernels, name):
    """A NaN in one pose, or a calibration matrix of NaNs (no address, loop bound or table index of the build / solve / update kernels of either
    family is computed from a value of K, a pose or a point: the values only flow through arithmetic).
    * ba_adjust reports VO_E_NUMERIC, and the context then solves a finite scene as before;
    * resident path, batch of 2, beside a finite problem: the finite one = itself beside a finite neighbour bit for bit and = itself solved alone;
      the other follows the oracle -- every step rejected, status 4 after 10 iterations, lambda = lambda0 2^55 exactly, its input handed back.
      (With K all NaN every gradient entry is NaN and the maxima behind ginf, which drop NaN, deliver 0: without the non-finite rule of
      ba_decide the gtol exit reported status 1, 'converged', at iteration 0.)"""
    from vo_mi355x import VoContext, _lib
    bad = lc.BY_NAME[name]
    good = lc.BY_NAME["ftol_floored_w4"]            # the same scene without the NaN; 10 iterations, like the run of rejections beside it
    ref_bad, ref_good = lc.classify(bad)["ref"], lc.classify(good)["ref"]
    Kb, pb, xb, ob = lc.scene(bad)
    Kg, pg, xg, og = lc.scene(good)
    prm_kw = lc.full_params(bad)
    assert prm_kw == dict(lc.full_params(good), max_iters=20) and ref_good["iters"] <= ref_bad["iters"] == 10
    with pytest.raises(_lib.VoError) as ei:
        ctx.ba_adjust(Kb, pb, xb, ob, ctx.ba_params(**prm_kw))
    assert ei.value.code == -6          # VO_E_NUMERIC
    alone = ctx.ba_adjust(Kg, pg, xg, og, ctx.ba_params(**prm_kw))
    _check_against_oracle(good, alone, ref_good, "%s[%s] after the non-finite problem" % (good["name"], ba_kernels))
    with VoContext(64, 64, max_pts=64, batch=2) as c2:
        prm = c2.ba_params(**prm_kw)
        c2.ba_upload(np.stack([Kg, Kg]), np.stack([pg, pg]), np.stack([xg, xg]), np.stack([og, og]))
        c2.ba_solve_resident(prm)
        po_gg, pt_gg, st_gg = c2.ba_fetch()
        c2.ba_upload(np.stack([Kg, Kb]), np.stack([pg, pb]), np.stack([xg, xb]), np.stack([og, ob]))
        c2.ba_solve_resident(prm)
        po, pt, st = c2.ba_fetch()
    print(name, ba_kernels, "finite", {k: st[0][k] for k in STAT_KEYS}, "non-finite", {k: st[1][k] for k in STAT_KEYS})
    assert _same((po[0], pt[0], st[0]), (po_gg[0], pt_gg[0], st_gg[0])), (st[0], st_gg[0])
    assert (st[0]["iters"], st[0]["accepted"], st[0]["status"]) == (alone[2]["iters"], alone[2]["accepted"], alone[2]["status"])
    assert abs(st[0]["cost"] - alone[2]["cost"]) <= 1e-10 * alone[2]["cost"] and np.abs(po[0] - alone[0]).max() <= 1e-9
    assert (st[1]["status"], st[1]["iters"], st[1]["accepted"]) == (4, 10, 0) == (ref_bad["status"], ref_bad["iters"], ref_bad["accepted"]), st[1]
    assert st[1]["lam"] == prm_kw["lambda0"] * 2.0 ** 55 == ref_bad["lam"]
    assert np.array_equal(po[1], pb, equal_nan=True) and np.array_equal(pt[1], xb, equal_nan=True)
