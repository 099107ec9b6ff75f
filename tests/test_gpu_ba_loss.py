"""GPU: the robust losses of the bundle adjustment (vo_ba_params.loss: soft_l1, cauchy, arctan beside huber and linear) against the
loss-generic numpy model (tests/ba_loss_model.py), through both kernel families, on scenes with ~5 % outlier observations."""
import ctypes

import numpy as np
import pytest

import ba_loss_model as lm

pytestmark = pytest.mark.gpu

ROBUST = ("soft_l1", "cauchy", "arctan")
SCENES = ((64, 4, 0), (256, 10, 1))


@pytest.fixture(autouse=True, params=["wave_private", "lane_per_observation"])
def ba_kernels(request, monkeypatch, ctx):
    """the same two kernel families as tests/test_gpu_ba.py (vo_tuning.ba_kernels 2 / 1)"""
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


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


@pytest.mark.parametrize("loss", ("huber", "linear") + ROBUST)
@pytest.mark.parametrize("scene", SCENES)
def test_probe_at_x0_matches_model(ctx, loss, scene):
    K, poses, points, obs = lm.outlier_scene(*scene)
    ctx.ba_upload(K, poses, points, obs)
    pr = ctx.ba_probe(lam=1e-4, loss=loss)
    ne = lm.normal_equations(K, poses, points, obs, loss)
    assert abs(pr["cost"] - ne["cost"]) <= 1e-12 * ne["cost"], (pr["cost"], ne["cost"])
    for k in ("Hpp", "gp", "Hll", "gl"):
        assert _rel(pr[k], ne[k]) <= 1e-10, (k, _rel(pr[k], ne[k]))
    # the cost is 1/2 C^2 sum rho over the residual norms the probe returns
    r = pr["residual"]
    assert abs(0.5 * lm.rho(r * r, loss).sum() - pr["cost"]) <= 1e-12 * pr["cost"]


@pytest.mark.parametrize("loss", ROBUST)
@pytest.mark.parametrize("scene", SCENES)
def test_solve_matches_model(ctx, loss, scene):
    K, poses, points, obs = lm.outlier_scene(*scene)
    po, pt, st = ctx.ba_adjust(K, poses, points, obs, ctx.ba_params(max_iters=30, loss=loss))
    ref = lm.solve(K, poses, points, obs, loss, max_iters=30)
    assert (st["iters"], st["accepted"], st["status"]) == (ref["iters"], ref["accepted"], ref["status"])
    assert abs(st["cost"] - ref["cost"]) <= 1e-7 * ref["cost"]
    assert np.abs(po - ref["poses"]).max() <= 1e-6
    assert np.abs(pt - ref["points"]).max() <= 1e-5


@pytest.mark.parametrize("scene", SCENES)
def test_robust_fits_differ_from_linear(ctx, scene):
    """on outlier tracks every robust loss lands away from the plain least-squares window (what main ran for every name but 'huber')"""
    K, poses, points, obs = lm.outlier_scene(*scene)
    po_lin, pt_lin, _ = ctx.ba_adjust(K, poses, points, obs, ctx.ba_params(max_iters=30, loss="linear"))
    for loss in ROBUST:
        po, pt, _ = ctx.ba_adjust(K, poses, points, obs, ctx.ba_params(max_iters=30, loss=loss))
        ref = lm.solve(K, poses, points, obs, loss, max_iters=30)
        assert np.abs(po - po_lin).max() > 100 * np.abs(po - ref["poses"]).max(), loss


def test_linear_is_the_unreachable_knee(ctx):
    K, poses, points, obs = lm.outlier_scene(64, 4, 0)
    a = ctx.ba_adjust(K, poses, points, obs, ctx.ba_params(max_iters=20, loss="linear", huber_delta=3.0))
    b = ctx.ba_adjust(K, poses, points, obs, ctx.ba_params(max_iters=20, huber_delta=1e30))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2]["cost"] == b[2]["cost"]


def test_batch_equals_single_solves_cauchy():
    from vo_mi355x import VoContext
    probs = [lm.outlier_scene(64, 4, s) for s in range(8)]
    with VoContext(64, 64, max_pts=64, batch=8) as cb:
        K = np.stack([p[0] for p in probs]); P = np.stack([p[1] for p in probs]); X = np.stack([p[2] for p in probs])
        O = np.stack([p[3] for p in probs])
        po, pt, st = cb.ba_adjust(K, P, X, O, cb.ba_params(max_iters=20, loss="cauchy"))
    with VoContext(64, 64, max_pts=64) as c1:
        for q, (K1, P1, X1, O1) in enumerate(probs):
            p1, t1, s1 = c1.ba_adjust(K1, P1, X1, O1, c1.ba_params(max_iters=20, loss="cauchy"))
            ref = lm.solve(K1, P1, X1, O1, "cauchy", max_iters=20)
            assert np.abs(po[q] - p1).max() <= 1e-9 and np.abs(pt[q] - t1).max() <= 1e-9
            assert np.abs(p1 - ref["poses"]).max() <= 1e-6


def test_bad_loss_and_f_scale_are_rejected(ctx):
    from vo_mi355x import _lib
    K, poses, points, obs = lm.outlier_scene(64, 4, 0)
    L = ctx._L
    W, N = obs.shape[:2]
    f64 = lambda a: np.ascontiguousarray(a, np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    po, pt = np.zeros((W, 6)), np.zeros((N, 3))
    # (a robust loss's f_scale outside [1e-150, 1e150], +inf included: C^2 or 1 / C^2 would overflow -- tests/test_gpu_ba_loss_forms.py)
    for loss, fs in ((5, 1.0), (-1, 1.0), (3, 0.0), (3, -1.0), (2, float("nan")), (3, float("inf")), (4, 1e200), (2, 1e-200), (4, 5e-324)):
        p = ctx.ba_params(max_iters=5)
        p.loss, p.huber_delta = loss, fs
        r = L.vo_ba_adjust(ctx._h, f64(K), f64(poses), f64(points), f64(obs), W, N, ctypes.byref(p), f64(po), f64(pt), None)
        assert r == -1, (loss, fs, r)                                # VO_E_INVALID
        assert not po.any() and not pt.any()
    ctx.ba_upload(K, poses, points, obs)
    for loss, fs in ((7, 1.0), (3, 0.0), (3, float("nan")), (4, float("inf")), (2, 2e150), (3, 1e-151)):
        with pytest.raises(_lib.VoError):
            ctx._ck(L.vo_ba_probe_loss(ctx._h, 1e-4, loss, fs, None, None, None, None, None, None, None, None, None, None, None))
    with pytest.raises(ValueError):
        ctx.ba_params(loss="tukey")


def test_drop_in_loss_names_and_lm():
    from vo_mi355x.bundle_adjuster import BundleAdjuster
    ba = BundleAdjuster(loss="tukey")
    with pytest.raises(ValueError):
        ba.adjust(None, [], [], np.eye(3), 0)
    with pytest.raises(NotImplementedError):
        BundleAdjuster(loss=lambda z: z).adjust(None, [], [], np.eye(3), 0)
    K, poses, points, obs = lm.outlier_scene(64, 4, 0)
    lmb = BundleAdjuster(method="lm", loss="cauchy")
    assert lmb._solve_loss(obs, obs.shape[1], obs.shape[0]) == "linear"


def test_resident_pipeline_takes_a_loss():
    """the closed loop's ADJUST stage accepts every loss (vo_pipe_create validates vo_pipe_params.ba) and refuses an unknown name"""
    from vo_mi355x import VoContext
    from vo_mi355x.resident import ResidentPipeline
    with VoContext(256, 160, max_pts=1024) as c:
        for loss in ("huber", "linear") + ROBUST:
            ResidentPipeline(c, np.eye(3) * 200, ba_loss=loss, ba_f_scale=2.0)
        with pytest.raises(ValueError):
            ResidentPipeline(c, np.eye(3) * 200, ba_loss="bad")


def test_solution_parity_against_the_reference(ctx, golden_dir):
    """ba_solution_parity against the reference's own scipy anchors for every robust loss and scene (tests/golden/baloss_*):
    a solver that fits the linear anchor fails it (tests/test_ba_loss_goldens.py checks how far apart the anchors are)"""
    from test_ba_loss_goldens import load, loss_goldens
    from helpers import ba_solution_parity
    paths = loss_goldens(golden_dir)
    assert paths
    for path in paths:
        g, gp, loss, K, poses, points, obs = load(path)

        def solve(mi, ftol, xtol):
            po, pt, st = ctx.ba_adjust(K, poses, points, obs, ctx.ba_params(max_iters=mi, ftol=ftol, xtol=xtol, loss=loss))
            return po, pt, st["cost"]
        ba_solution_parity(solve, g, gp, K, poses, points, obs)


def _closed_loop(ba_loss=None, n=3):
    from vo_mi355x import VoContext, synthetic as syn
    from vo_mi355x.resident import ResidentPipeline
    sc = syn.sway_scene(8, w=256, h=160, f=260.0, seed=2024, pose_fn=lambda t: syn.sway_pose(t, period=24.0))
    with VoContext(256, 160, max_pts=1024) as c:
        state, t1 = syn.gt_bootstrap(c, sc, 0, 3)
        kw = {} if ba_loss is None else dict(ba_loss=ba_loss)
        rp = ResidentPipeline(c, sc["K"], ba_max_iters=12, **kw)
        rp.seed(state, [], [], 1)
        c.push_frame(sc["frames"][t1])
        recs, costs = [], []
        for s in range(n):
            c.push_frame(sc["frames"][t1 + 1 + s]); rp.step(); recs.append(rp.fetch())
            if ba_loss not in (None, "huber"):
                r = c.ba_probe(lam=1e-4, loss=ba_loss)["residual"]      # the frame's problem at its x0
                costs.append(0.5 * lm.rho(r * r, ba_loss).sum())
        return recs, rp.read_tables(), costs


def test_closed_loop_explicit_huber_is_the_default():
    a, ta, _ = _closed_loop(None)
    b, tb, _ = _closed_loop("huber")
    for ra, rb in zip(a, b):
        for k in ra:
            assert np.array_equal(np.asarray(ra[k]), np.asarray(rb[k])), k
    for x, y in zip(ta, tb):
        assert np.array_equal(np.asarray(x), np.asarray(y))


def test_closed_loop_cauchy_cost0_is_the_loss_of_the_frame():
    recs, _, costs = _closed_loop("cauchy")
    for rec, c in zip(recs, costs):
        if rec["ba_iters"] > 0:
            assert abs(rec["ba_cost0"] - c) <= 1e-10 * c, (rec["ba_cost0"], c)
    assert any(r["ba_iters"] > 0 for r in recs)


def test_virtual_shards_match_unsharded_cauchy():
    from test_gpu_shard import _solve_sharded, _solve_unsharded
    from vo_mi355x import synthetic as syn
    s = syn.make_ba_scene(n_pts=1000, n_slots=10, seed=11, visibility=0.9)
    kw = dict(max_iters=20, loss="cauchy")
    po, pt, st = _solve_unsharded(s, kw)
    po_s, pt_s, st_s, n_obs = _solve_sharded(s, 4, kw)
    assert (st_s["iters"], st_s["accepted"], st_s["status"]) == (st["iters"], st["accepted"], st["status"])
    assert abs(st_s["cost"] - st["cost"]) <= 1e-10 * st["cost"] and abs(st_s["cost0"] - st["cost0"]) <= 1e-10 * st["cost0"]
    assert np.abs(po_s - po).max() <= 1e-8 and np.abs(pt_s - pt).max() <= 1e-8
