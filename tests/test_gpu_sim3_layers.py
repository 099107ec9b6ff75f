"""GPU: the Python layers over the Sim(3) search -- Extractor.align_landmarks (two maps joined through matched landmarks) and
vo_mi355x.evaluate (the scale-aligned absolute trajectory error) -- against tests/sim3_model.py.  The two searches used here are among the
problems tests/test_sim3_model.py shows to be `decided`.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

import sim3_model as sm

pytestmark = pytest.mark.gpu
KW = dict(threshold=sm.THR, seed=sm.SEARCH_SEED)


@pytest.fixture(scope="module")
def ctx():
    from vo_mi355x import VoContext
    with VoContext(64, 64, max_pts=64) as c:
        yield c


def _rmse(m, a, b):
    s, R, t = sm.unpack(m)
    e = np.linalg.norm(b - (s * (a @ R.T) + t), axis=1)
    return float(np.sqrt(np.mean(e * e)))


def test_align_landmarks_joins_two_maps_through_matches_with_outliers(ctx):
    from vo_mi355x import DMatch, Extractor, Landmark
    sc = sm.landmark_scene()
    l1 = [Landmark(0, p.reshape(3, 1), np.zeros((1, 1))) for p in sc["p1"]]
    l2 = [Landmark(0, p.reshape(3, 1), np.zeros((1, 1))) for p in sc["p2"]]
    matches = [DMatch(q, t, 0.0) for q, t in sc["pairs"]]
    ext = Extractor(lazy=False, min_kp_dist=7, ctx=ctx)
    S, inl, st = ext.align_landmarks(l1, l2, matches, **KW)
    m = sm.search(sc["src"], sc["dst"], thr=sm.THR, seed=sm.SEARCH_SEED)
    fin = sm.finish(sc["src"], sc["dst"], m)
    f = fin["fit"]
    got = sm.pack(np.cbrt(np.linalg.det(S[:3, :3])), S[:3, :3] / np.cbrt(np.linalg.det(S[:3, :3])), S[:3, 3])
    d = sm.diff(got, f["m"], f["tscale"]) / (sm.EPS * f["kappa"])
    X, Y = sm.widen(sc["src"]), sm.widen(sc["dst"])
    e = np.linalg.norm(Y - (X @ S[:3, :3].T + S[:3, 3]), axis=1)
    em = np.sqrt(sm.err(f["m"], sc["src"], sc["dst"]))
    print("align_landmarks: %d inliers of %d matches (model %d, %d good), scale %.9g (true %g), |S - model| / (2^-52 kappa) = %.3g (bound %g + 4 for "
          "s R and the cube root), worst inlier error %.3g (model %.3g)" % (len(inl), len(matches), m["count"], int(sc["good"].sum()), got[0], sc["s"],
                                                                          d, sm.REFIT_FACTOR, e[inl].max(), em[m["mask"]].max()))
    assert m["decided"] and st["status"] == 0 and st["refit"] == 1
    assert isinstance(inl, list) and inl == np.nonzero(m["mask"])[0].tolist() == np.nonzero(sc["good"])[0].tolist()
    assert S.shape == (4, 4) and np.array_equal(S[3], [0, 0, 0, 1])
    # S[:3, :3] = s R is one rounding per entry away from the pair (s, R), and the cube root of its determinant a few more
    assert d <= sm.REFIT_FACTOR + 4
    assert np.abs(e[inl] - em[m["mask"]]).max() <= (sm.REFIT_FACTOR + 4) * sm.EPS * f["kappa"] * (2 * got[0] * np.abs(X).sum(1).max() + f["tscale"]) + 1e-12
    # index-aligned lists: the same pairs handed over as two lists
    S2, inl2, st2 = ext.align_landmarks([l1[q] for q, _ in sc["pairs"]], [l2[t] for _, t in sc["pairs"]], **KW)
    assert sm.bits_equal(S, S2) and inl2 == inl and st2 == st


def test_ate_of_a_scaled_trajectory(ctx):
    from vo_mi355x import Trajectory, evaluate
    sc = sm.trajectory_scene()
    est, gt = Trajectory({t: H for t, H in enumerate(sc["est"])}), Trajectory({t: H for t, H in enumerate(sc["gt"])})
    a, b = sc["centres_est"], sc["centres_gt"]
    r = evaluate.ate(est, gt, ctx)
    f = sm.fit(sc["src"], sc["dst"])
    want = _rmse(f["m"], a, b)
    d = abs(r["scale"] - f["s"]) / f["s"] / (sm.EPS * f["kappa"])
    print("ate: n %d, scale %.12g (model %.12g, true %g): |ds| / s / (2^-52 kappa) = %.3g (bound %g), kappa %.3g; rmse %.12g (model %.12g), mean %.4g, "
          "median %.4g, max %.4g" % (r["n"], r["scale"], f["s"], sc["s"], d, sm.REFIT_FACTOR, f["kappa"], r["rmse"], want, r["mean"], r["median"], r["max"]))
    assert r["n"] == 40 and set(r) == {"rmse", "mean", "median", "max", "scale", "S", "n"}
    assert d <= sm.REFIT_FACTOR and abs(r["rmse"] - want) <= 1e-9 * want
    assert r["median"] <= r["rmse"] <= r["max"] and 0.005 < r["rmse"] < 0.03            # 1 cm noise per coordinate: sqrt 3 cm per point
    # arrays of poses in place of Trajectory objects: the same result
    r2 = evaluate.ate(sc["est"], sc["gt"], ctx)
    assert r2["rmse"] == r["rmse"] and r2["scale"] == r["scale"]
    # without scale on a trajectory of scale 2.5: the model's larger value
    r0 = evaluate.ate(est, gt, ctx, with_scale=False)
    f0 = sm.fit(sc["src"], sc["dst"], None, False)
    want0 = _rmse(f0["m"], a, b)
    print("ate with_scale=False: scale %g, rmse %.12g (model %.12g)" % (r0["scale"], r0["rmse"], want0))
    assert r0["scale"] == 1.0 and abs(r0["rmse"] - want0) <= 1e-9 * want0 and r0["rmse"] > 100 * r["rmse"]


def test_robust_alignment_survives_five_gross_outlier_poses(ctx):
    from vo_mi355x import evaluate
    sc = sm.trajectory_scene(outliers=5)
    good = sc["good"]
    a, b = sc["centres_est"], sc["centres_gt"]
    plain = evaluate.align_trajectory(sc["est"], sc["gt"], ctx)
    rob = evaluate.align_trajectory(sc["est"], sc["gt"], ctx, robust=True, **KW)
    m = sm.search(sc["src"], sc["dst"], thr=sm.THR, seed=sm.SEARCH_SEED)
    err = lambda al: np.linalg.norm(b - (al["s"] * (a @ al["R"].T) + al["t"]), axis=1)
    ep, er = err(plain), err(rob)
    print("five outlier poses: least squares: scale %.6g, worst good pose %.4g; robust: scale %.6g (true %g), worst good pose %.4g, %d inliers (model %d)"
          % (plain["s"], ep[good].max(), rob["s"], sc["s"], er[good].max(), len(rob["inliers"]), m["count"]))
    assert m["decided"] and np.array_equal(rob["inliers"], np.nonzero(m["mask"])[0]) and np.array_equal(rob["inliers"], np.nonzero(good)[0])
    # 1 cm noise per coordinate on 35 poses along a path 50 long: every good pose within 5 cm, the scale within 1e-3 of the truth;
    # five poses 50 off among 40 pull the least-squares fit more than a metre off some good pose
    assert er[good].max() <= 0.05 and abs(rob["s"] - sc["s"]) <= 1e-3 * sc["s"]
    assert ep[good].max() > 1.0
    r = evaluate.ate(sc["est"], sc["gt"], ctx, robust=True, **KW)
    assert r["n"] == 40 and r["max"] > 40 and r["median"] < 0.05
