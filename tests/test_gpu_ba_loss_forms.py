"""GPU: the robust losses of the bundle adjustment on every kernel instance a loss can launch, at f_scale C != 1, per observation against
mpmath, at the ends of the accepted f_scale range, through every summation form (fold, chunks, workgroups, shards, tail compaction) and in
the closed loop -- against the loss-generic model (oracle/ba_oracle.py loss_*, through tests/ba_loss_model.py).

Instances (csrc/vo_ba.hip ba_launch_iter_t, picked by ba_geometry from W, N and vo_tuning) and the case of MATRIX that reaches each:
  k_ba_build_w<1,1,4> / k_ba_update_w<1,4>   W 1-2                w1, w2
  k_ba_build_w<2,1,4> / k_ba_update_w<1,4>   W 3-4                w4
  k_ba_build_w<2,1,8> / k_ba_update_w<1,8>   W 5                  w5
  k_ba_build_w<3,1,8> / k_ba_update_w<1,8>   W 6-7                w7
  k_ba_build_w<4,1,8> / k_ba_update_w<1,8>   W 8                  w8
  k_ba_build_w<4,2,5> / k_ba_update_w<2,5>   W 9-10               w10
  k_ba_build_w<4,2,8> / k_ba_update_w<2,8>   W 9-10, ba_lanes 8   w9_lanes8
  k_ba_build<256,8> / k_ba_update<256,8>     ba_kernels 1, W <= 8 l6
  k_ba_build<256,0> / k_ba_update<256,0>     W 11-16, few landmarks   l13
  k_ba_build<1024,0> / k_ba_update<1024,0>   W 17-20 with N > 1280    l17
  k_ba_build<512,0> / k_ba_update<512,0>     ba_threads 512       l14_threads512
k_ba_build_w<1,1,8> is compiled but not reachable: windows of <= 2 slots (one column block) always take 4 lanes per landmark (v2_lpp is 4
for W <= 4 and ba_lanes = 8 only widens the 5-lane map), so no case here launches it."""
import copy
import ctypes

import numpy as np
import pytest
from hypothesis import given, settings, strategies as st

import ba_loss_model as lm

pytestmark = pytest.mark.gpu

ROBUST = ("soft_l1", "cauchy", "arctan")
LOSSES = ("huber",) + ROBUST

# (name, W, N, seed, tuning): N leaves the last chunk / landmark group part-filled
MATRIX = [
    ("w1", 1, 37, 3, {"ba_kernels": 2}),
    ("w2", 2, 45, 4, {"ba_kernels": 2}),
    ("w4", 4, 70, 5, {"ba_kernels": 2}),
    ("w5", 5, 77, 6, {"ba_kernels": 2}),
    ("w7", 7, 83, 7, {"ba_kernels": 2}),
    ("w8", 8, 91, 8, {"ba_kernels": 2}),
    ("w10", 10, 101, 9, {"ba_kernels": 2}),
    ("w9_lanes8", 9, 97, 10, {"ba_kernels": 2, "ba_lanes": 8}),
    ("l6", 6, 90, 11, {"ba_kernels": 1}),
    ("l13", 13, 150, 12, {"ba_kernels": 1}),
    ("l17", 17, 1290, 13, {"ba_kernels": 1}),
    ("l14_threads512", 14, 203, 14, {"ba_kernels": 1, "ba_threads": 512}),
]
# the rule form of each forced case: the same problem with only the family forced
RULE_OF = {"w9_lanes8": {"ba_kernels": 2}, "l14_threads512": {"ba_kernels": 1}}
C_CASE = 2.5          # f_scale of the matrix (scipy's default 1 is covered by tests/test_gpu_ba_loss.py)
MAX_IT = 20


def _scene(W, N, seed):
    """ba_loss_model.outlier_scene with the holes of test_ba_fuzz: one landmark nobody sees, one slot that sees nothing"""
    K, poses, points, obs = lm.outlier_scene(N, W, seed)
    rng = np.random.default_rng(seed)
    obs[:, rng.integers(0, N)] = np.nan
    if W > 2:
        obs[rng.integers(1, W)] = np.nan
    return K, poses, points, obs


@pytest.fixture(scope="module")
def ctx():
    from vo_mi355x import VoContext
    c = VoContext(64, 64, max_pts=64)
    yield c
    c.close()


def _tuned(ctx, tune):
    ctx.set_tuning(**dict(dict.fromkeys(ctx.tuning(), 0), **tune))


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def _check_probe(ctx, K, poses, points, obs, loss, C, tol_cost=1e-12, tol_blk=1e-10):
    ctx.ba_upload(K, poses, points, obs)
    pr = ctx.ba_probe(lam=1e-4, loss=loss, huber_delta=C)
    ne = lm.normal_equations(K, poses, points, obs, loss, C)
    assert abs(pr["cost"] - ne["cost"]) <= tol_cost * ne["cost"], (pr["cost"], ne["cost"])
    for k in ("Hpp", "gp", "Hll", "gl"):
        assert _rel(pr[k], ne[k]) <= tol_blk, (k, _rel(pr[k], ne[k]))
    return pr


def _check_solve(ctx, K, poses, points, obs, loss, C, max_iters=MAX_IT, pt_scaled=False):
    """pt_scaled: the points to 1e-5 of max(1, their distance) (a small f_scale lets outlier-led landmarks drift hundreds of units away)"""
    ref = lm.solve(K, poses, points, obs, loss, C, max_iters=max_iters)
    assert ref["margin"] >= 1e-6, ("marginal scene: an LM decision within", ref["margin"], "of its threshold")
    po, pt, st = ctx.ba_adjust(K, poses, points, obs, ctx.ba_params(max_iters=max_iters, loss=loss, huber_delta=C))
    assert (st["iters"], st["accepted"], st["status"]) == (ref["iters"], ref["accepted"], ref["status"]), (st, ref["iters"], ref["status"])
    assert abs(st["cost"] - ref["cost"]) <= 1e-7 * ref["cost"]
    assert np.abs(po - ref["poses"]).max() <= 1e-6
    scale = np.maximum(1.0, np.linalg.norm(ref["points"], axis=1))[:, None] if pt_scaled else 1.0
    assert (np.abs(pt - ref["points"]) / scale).max() <= 1e-5
    return po, pt, st


# ---------------------------------------------------------------------------------------------------------
# every instance, every loss, C != 1
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", LOSSES)
@pytest.mark.parametrize("case", MATRIX, ids=[m[0] for m in MATRIX])
def test_instance_matrix(ctx, case, loss):
    name, W, N, seed, tune = case
    K, poses, points, obs = _scene(W, N, seed)
    _tuned(ctx, tune)
    _check_probe(ctx, K, poses, points, obs, loss, C_CASE)
    po, pt, st = _check_solve(ctx, K, poses, points, obs, loss, C_CASE)
    if name in RULE_OF:
        _tuned(ctx, RULE_OF[name])
        po_r, pt_r, st_r = ctx.ba_adjust(K, poses, points, obs, ctx.ba_params(max_iters=MAX_IT, loss=loss, huber_delta=C_CASE))
        assert (st["iters"], st["accepted"], st["status"]) == (st_r["iters"], st_r["accepted"], st_r["status"])
        assert abs(st["cost"] - st_r["cost"]) <= 1e-9 * st_r["cost"]
        assert np.abs(po - po_r).max() <= 1e-9 and np.abs(pt - pt_r).max() <= 1e-9


# ---------------------------------------------------------------------------------------------------------
# the summation forms of each family
# ---------------------------------------------------------------------------------------------------------
FORMS = {
    "wave_private": (10, 300, 21, {"ba_kernels": 2},
                     [{"ba_fold": 1}, {"ba_fold": 2}, {"ba_workgroups": 1}, {"ba_workgroups": 3}, {"ba_workgroups": 999},
                      {"ba_workgroup_cap": 1}, {"ba_workgroup_cap": 2}, {"ba_workgroup_cap": 16}]),
    "lane_per_observation": (17, 300, 22, {"ba_kernels": 1},
                             [{"ba_fold": 1}, {"ba_fold": 2}, {"ba_chunks": 2}, {"ba_chunks": 3}, {"ba_threads": 512}, {"ba_threads": 1024}]),
}


@pytest.mark.parametrize("loss", ROBUST)
@pytest.mark.parametrize("family", sorted(FORMS))
def test_forms_agree(ctx, family, loss):
    W, N, seed, base, forms = FORMS[family]
    K, poses, points, obs = _scene(W, N, seed)
    _tuned(ctx, base)
    po0, pt0, st0 = _check_solve(ctx, K, poses, points, obs, loss, C_CASE)
    for f in forms:
        _tuned(ctx, dict(base, **f))
        po, pt, st = ctx.ba_adjust(K, poses, points, obs, ctx.ba_params(max_iters=MAX_IT, loss=loss, huber_delta=C_CASE))
        assert (st["iters"], st["accepted"], st["status"]) == (st0["iters"], st0["accepted"], st0["status"]), (f, st, st0)
        assert abs(st["cost"] - st0["cost"]) <= 1e-10 * st0["cost"] and abs(st["cost0"] - st0["cost0"]) <= 1e-12 * st0["cost0"], f
        assert np.abs(po - po0).max() <= 1e-9 and np.abs(pt - pt0).max() <= 1e-8, f


def test_tail_compaction_per_robust_loss(monkeypatch):
    """tests/test_gpu_ba_wave.py test_ba_running_problem_compaction with each robust loss at f_scale 2 (its tolerances)"""
    from vo_mi355x import VoContext, synthetic as syn
    monkeypatch.setattr(VoContext, "default_tuning", {"ba_kernels": 2})
    B, N, W = 64, 800, 10
    sc = []
    for b in range(B):
        kind = b % 4
        s = syn.make_ba_scene(n_pts=N, n_slots=W, seed=300 + b, visibility=(1.0, 0.9, 0.7, 0.5)[kind], obs_noise=(0.05, 0.3, 0.5, 1.0)[kind],
                              pt_noise=(0.02, 0.3, 0.6, 1.0)[kind])
        if b % 16 == 0:
            s["poses0"], s["points0"] = s["poses_gt"].copy(), s["points_gt"].copy()
        sc.append(s)
    stack = lambda k: np.stack([s[k] for s in sc])
    with VoContext(64, 64, max_pts=64, batch=B) as c, VoContext(64, 64, max_pts=64) as c1:
        for loss in ROBUST:
            prm = dict(max_iters=12, loss=loss, huber_delta=2.0)
            po, pt, st = c.ba_adjust(stack("K"), stack("poses0"), stack("points0"), stack("obs"), c.ba_params(**prm))
            its = [x["iters"] for x in st]
            assert min(its) + 2 <= max(its), (loss, its)
            for b in range(0, B, 3):
                s = sc[b]
                po1, pt1, st1 = c1.ba_adjust(s["K"], s["poses0"], s["points0"], s["obs"], c1.ba_params(**prm))
                assert (st[b]["iters"], st[b]["accepted"], st[b]["status"]) == (st1["iters"], st1["accepted"], st1["status"]), (loss, b, st[b], st1)
                assert abs(st[b]["cost"] - st1["cost"]) <= 1e-10 * max(st1["cost"], 1e-30), (loss, b, st[b]["cost"], st1["cost"])
                dp = np.linalg.norm(pt[b] - pt1, axis=1) / np.linalg.norm(pt1, axis=1)
                assert np.abs(po[b] - po1).max() <= 1e-9 and dp.max() <= 1e-6 and np.median(dp) <= 1e-11, (loss, b, dp.max(), np.median(dp))


@pytest.mark.parametrize("loss", ROBUST)
@pytest.mark.parametrize("W", (4, 10))
def test_virtual_shards_match_unsharded(loss, W):
    from test_gpu_shard import _solve_sharded, _solve_unsharded
    from vo_mi355x import synthetic as syn
    s = syn.make_ba_scene(n_pts=1000, n_slots=W, seed=11, visibility=0.9)
    kw = dict(max_iters=20, loss=loss, huber_delta=0.7)
    po, pt, st = _solve_unsharded(s, kw)
    po_s, pt_s, st_s, n_obs = _solve_sharded(s, 4, kw)
    assert (st_s["iters"], st_s["accepted"], st_s["status"]) == (st["iters"], st["accepted"], st["status"])
    assert abs(st_s["cost"] - st["cost"]) <= 1e-10 * st["cost"] and abs(st_s["cost0"] - st["cost0"]) <= 1e-10 * st["cost0"]
    assert np.abs(po_s - po).max() <= 1e-8 and np.abs(pt_s - pt).max() <= 1e-8


# ---------------------------------------------------------------------------------------------------------
# f_scale
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", (0.05, 0.5, 3.0, 40.0))
@pytest.mark.parametrize("loss", lm.LOSSES)
@pytest.mark.parametrize("family,W,N", [("wave_private", 3, 60), ("wave_private", 9, 120), ("lane_per_observation", 6, 80),
                                        ("lane_per_observation", 12, 130)])
def test_f_scale_sweep(ctx, family, W, N, loss, C):
    K, poses, points, obs = _scene(W, N, 40 + W)
    _tuned(ctx, {"ba_kernels": 2 if family == "wave_private" else 1})
    pr = _check_probe(ctx, K, poses, points, obs, loss, C)
    r = pr["residual"]
    assert abs(0.5 * lm.rho(r * r, loss, C).sum() - pr["cost"]) <= 1e-12 * pr["cost"]
    _check_solve(ctx, K, poses, points, obs, loss, C, pt_scaled=True)


def _one_observation(e0):
    """W = 1, N = 1, R = I, t = 0, K = diag(f, f, 1) + principal point: u = f a + cx exactly, one residual (e0, 0) with s = e0^2 exact"""
    K = np.array([[256.0, 0.0, 32.0], [0.0, 256.0, 32.0], [0.0, 0.0, 1.0]])
    poses, points = np.zeros((1, 6)), np.array([[0.125, -0.0625, 1.0]])
    obs = np.array([[[256.0 * 0.125 + 32.0 - e0, -256.0 * 0.0625 + 32.0]]])
    return K, poses, points, obs


def _mp_loss(loss, s, C):
    """50-digit 1/2 C^2 rho(s / C^2) and rho'(s / C^2) at the double inputs s, C"""
    import mpmath as mp
    with mp.workdps(50):
        s, C = mp.mpf(s), mp.mpf(C)
        z = s / (C * C)
        if loss == "soft_l1":
            r, w = 2 * (mp.sqrt(1 + z) - 1), 1 / mp.sqrt(1 + z)
        elif loss == "cauchy":
            r, w = mp.log1p(z), 1 / (1 + z)
        else:
            r, w = mp.atan(z), 1 / (1 + z * z)
        return float(C * C * r / 2), float(w), z


def _targets():
    import mpmath as mp
    out = [2.0 ** -60, 2.0 ** -53]
    for k in (0, 1, 5, 30):                                    # ba_log1p's reduction switches at 1 + z = sqrt(2) 2^k
        b = float(mp.sqrt(2) * mp.mpf(2) ** k - 1)
        out += [b * (1 - 1e-9), b * (1 + 1e-9)]
    for b in (float(mp.tan(mp.pi / 12)), 1.0, float(1 / mp.tan(mp.pi / 12))):     # ba_atan's: t = tan(pi/12), z = 1, 1/z = tan(pi/12)
        out += [b * (1 - 1e-9), b * (1 + 1e-9)]
    return out + [1e8, 1e16, 1e100]


@pytest.mark.parametrize("family", ("wave_private", "lane_per_observation"))
def test_per_observation_loss_against_mpmath(ctx, family):
    """the cost term and the weight of ONE observation against 50-digit mpmath over the branch points of ba_log1p / ba_atan and far
    beyond: the cost is 1/2 C^2 rho(z) itself, the weight is Hll(loss) / Hll(linear) of the same problem"""
    e0 = 3.0
    K, poses, points, obs = _one_observation(e0)
    _tuned(ctx, {"ba_kernels": 2 if family == "wave_private" else 1})
    ctx.ba_upload(K, poses, points, obs)
    lin = ctx.ba_probe(lam=1e-4, loss="linear")
    assert lin["residual"].tolist() == [e0] and lin["cost"] == 0.5 * e0 * e0
    s = e0 * e0
    bad = []
    for z in _targets():
        C = float(np.sqrt(s / z))
        for loss in ROBUST:
            pr = ctx.ba_probe(lam=1e-4, loss=loss, huber_delta=C)
            c_ref, w_ref, _ = _mp_loss(loss, s, C)
            w = pr["Hll"][0, 0, 0] / lin["Hll"][0, 0, 0]
            ec, ew = abs(pr["cost"] - c_ref) / c_ref, abs(w - w_ref) / w_ref
            if not (ec <= 1e-15 and ew <= 1e-15):
                bad.append((loss, z, ec, ew))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------
# the ends of the accepted f_scale range
# ---------------------------------------------------------------------------------------------------------
def _near_plane_scene():
    """the 64-landmark outlier scene with landmark 0 1e-9 in front of slot 0's camera plane: a residual of ~1e11 px"""
    from vo_mi355x import synthetic as syn
    K, poses, points, obs = lm.outlier_scene(64, 4, 0)
    R = syn.rodrigues(poses[0, :3])
    points[0] = R.T @ (np.array([0.01, 0.02, 1e-9]) - poses[0, 3:])
    obs[0, 0] = (30.0, 40.0)
    return K, poses, points, obs


ACCEPTED = (1e-150, 1e-100, 1e-20, 1e20, 1e100, 1e150)
REFUSED = (9.9e-151, 1e-200, 5e-324, 1.01e150, 1e200, 1.7e308, float("inf"))


@pytest.mark.parametrize("family", ("wave_private", "lane_per_observation"))
def test_f_scale_range_ends_give_finite_results(ctx, family):
    K, poses, points, obs = _near_plane_scene()
    _tuned(ctx, {"ba_kernels": 2 if family == "wave_private" else 1})
    ctx.ba_upload(K, poses, points, obs)
    lin = ctx.ba_probe(lam=1e-4, loss="linear")
    assert lin["residual"].max() > 1e9
    for loss in lm.LOSSES:
        for C in ACCEPTED + ((float("inf"), 1e300) if loss in ("huber", "linear") else ()):
            pr = ctx.ba_probe(lam=1e-4, loss=loss, huber_delta=C)
            assert np.isfinite(pr["cost"]) and pr["cost"] >= 0, (loss, C, pr["cost"])
            for k in ("Hpp", "Hll", "gp", "gl"):
                assert np.isfinite(pr[k]).all(), (loss, C, k)
            w = pr["Hll"][:, 0, 0] / lin["Hll"][:, 0, 0]                  # per-landmark weighted sums over the slots >= 0
            assert (w >= 0).all(), (loss, C)
            po, pt, st = ctx.ba_adjust(K, poses, points, obs, ctx.ba_params(max_iters=3, loss=loss, huber_delta=C))
            assert np.isfinite(po).all() and np.isfinite(pt).all() and np.isfinite(st["cost"]) and st["cost"] <= st["cost0"], (loss, C, st)


def test_f_scale_range_ends_are_refused(ctx):
    """a robust loss's f_scale outside [VO_BA_F_SCALE_MIN, VO_BA_F_SCALE_MAX]: VO_E_INVALID from vo_ba_adjust, vo_ba_probe_loss and
    vo_pipe_create, nothing written"""
    from vo_mi355x import VoContext, _lib
    from vo_mi355x.resident import ResidentPipeline
    K, poses, points, obs = lm.outlier_scene(64, 4, 0)
    L = ctx._L
    W, N = obs.shape[:2]
    f64 = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    po, pt = np.zeros((W, 6)), np.zeros((N, 3))
    ctx.ba_upload(K, poses, points, obs)
    for loss in ROBUST:
        code = _lib.loss_code(loss)
        for C in REFUSED:
            p = ctx.ba_params(max_iters=5, loss=loss)
            p.huber_delta = C
            r = L.vo_ba_adjust(ctx._h, f64(K), f64(poses), f64(points), f64(obs), W, N, ctypes.byref(p), f64(po), f64(pt), None)
            assert r == -1, (loss, C, r)
            assert not po.any() and not pt.any()
            assert L.vo_ba_probe_loss(ctx._h, 1e-4, code, C, None, None, None, None, None, None, None, None, None, None, None) == -1, (loss, C)
    with VoContext(256, 160, max_pts=1024) as c:
        for loss in ROBUST:
            for C in (REFUSED[0], REFUSED[-1]):
                with pytest.raises(_lib.VoError):
                    ResidentPipeline(c, np.eye(3) * 200, ba_loss=loss, ba_f_scale=C)
        for C in (ACCEPTED[0], ACCEPTED[-1]):
            ResidentPipeline(c, np.eye(3) * 200, ba_loss="arctan", ba_f_scale=C)
        ResidentPipeline(c, np.eye(3) * 200, ba_loss="huber", ba_f_scale=float("inf"))     # (Huber takes any C > 0: its terms stay finite)


# ---------------------------------------------------------------------------------------------------------
# fuzz
# ---------------------------------------------------------------------------------------------------------
from test_gpu_fuzz import FUZZ  # noqa: E402


@settings(**dict(FUZZ, max_examples=max(10, FUZZ["max_examples"] // 2)))
@given(st.sampled_from(lm.LOSSES), st.sampled_from([0.03, 0.4, 1.0, 2.5, 17.0]), st.integers(1, 20), st.integers(1, 300),
       st.integers(0, 2 ** 31 - 1), st.sampled_from([1.0, 0.8, 0.5]), st.integers(1, 2))
def test_ba_loss_fuzz(ctx, loss, C, n_slots, n_pts, seed, vis, fam):
    from vo_mi355x import synthetic as syn
    s = syn.make_ba_scene(n_pts=n_pts, n_slots=n_slots, seed=seed % 1000, visibility=vis, obs_noise=0.5)
    rng = np.random.default_rng(seed)
    obs = s["obs"].copy()
    seen = np.argwhere(~np.isnan(obs[..., 0]))
    pick = seen[rng.random(len(seen)) < 0.05]
    obs[pick[:, 0], pick[:, 1]] += rng.uniform(-30, 30, (len(pick), 2))
    if n_pts > 3:
        obs[:, rng.integers(0, n_pts)] = np.nan
    if n_slots > 2:
        obs[rng.integers(0, n_slots)] = np.nan
    if np.isfinite(obs[..., 0]).sum() < 1:
        return
    _tuned(ctx, {"ba_kernels": fam})
    K, P, X = s["K"], s["poses0"], s["points0"]
    ctx.ba_upload(K, P, X, obs)
    pr = ctx.ba_probe(lam=1e-3, loss=loss, huber_delta=C)
    ne = lm.normal_equations(K, P, X, obs, loss, C)
    rel = lambda a, b: np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)
    assert rel(pr["Hpp"], ne["Hpp"]) <= 1e-9 and rel(pr["Hll"], ne["Hll"]) <= 1e-9 and rel(pr["gp"], ne["gp"]) <= 1e-9
    assert abs(pr["cost"] - ne["cost"]) <= 1e-10 * ne["cost"] + 1e-14
    po, pt, stt = ctx.ba_adjust(K, P, X, obs, ctx.ba_params(max_iters=8, loss=loss, huber_delta=C))
    assert np.isfinite(po).all() and np.isfinite(pt).all() and np.isfinite(stt["cost"])
    assert abs(stt["cost0"] - ne["cost"]) <= 1e-10 * ne["cost"] + 1e-14
    assert abs(lm.cost(K, po, pt, obs, loss, C) - stt["cost"]) <= 1e-9 * stt["cost"] + 1e-14
    assert stt["cost"] <= stt["cost0"] * (1 + 1e-12)


# ---------------------------------------------------------------------------------------------------------
# the closed loop with a robust loss against oracle/pipe_oracle.py
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss", ROBUST)
@pytest.mark.parametrize("window", (4, 10))
def test_closed_loop_robust_loss_matches_the_model(loss, window):
    import pipe_helpers as ph
    import pipe_oracle as po
    from vo_mi355x import VoContext
    from vo_mi355x.resident import ResidentPipeline
    w, h, t1, n = 256, 160, 3, 8
    sc = ph.scene(t1 + n + 1, w=w, h=h, f=260.0, seed=2024, pose_fn=lambda t: ph.sway_pose(t, period=24.0))
    with VoContext(w, h, max_pts=2048) as ctx_a, VoContext(w, h, max_pts=2048) as ctx_b:
        state, _ = ph.gt_bootstrap(ctx_a, sc, 0, t1)
        model = po.PipeModel(ctx_a, sc["K"], w, h, cap=2048, params=po.Params(ba_window=window, ba_max_iters=12, ba_loss=loss, ba_f_scale=2.0))
        model.seed(copy.deepcopy(state), [], [], 1)
        ctx_a.push_frame(sc["frames"][t1])
        rp = ResidentPipeline(ctx_b, sc["K"], ba_window=window, ba_max_iters=12, pnp_blind_batches=8, ba_loss=loss, ba_f_scale=2.0)
        rp.seed(state, [], [], 1)
        ctx_b.push_frame(sc["frames"][t1])
        n_ba = 0
        for s in range(n):
            im = sc["frames"][t1 + 1 + s]
            model.step(im)
            ctx_b.push_frame(im); rp.step(); rec = rp.fetch()
            assert rec["status"] == 0 and model.status == 0
            n_ba += rec["ba_iters"] > 0
            e = rp.entries()
            assert (len(e["cand"]), len(e["lm"]), len(e["dead"])) == (len(model.cand), len(model.lm_L), len(model.dead_L)), s
            for (l, k), x in zip(zip(model.lm_L, model.lm_K), e["lm"]):
                y = model.entry(l, k)
                assert x[0] == y[0] and x[2:4] == y[2:4] and np.array_equal(x[5], y[5]) and np.linalg.norm(x[1] - y[1]) <= 1e-7 * np.linalg.norm(y[1])
        assert n_ba > 0
