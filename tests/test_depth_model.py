"""CPU-only: the float64 model of the depth filter (tests/depth_model.py) against truths that do not come from it -- the exact posterior by
quadrature, a finite perturbation, synthetic depths, a float64 ZMSSD, the rendered scene -- and the case lists the GPU tests iterate over."""
import numpy as np
import pytest

import depth_model as dm


def simpson(y, x):
    try:
        from scipy.integrate import simpson as sp
        return float(sp(y, x=x))
    except ImportError:
        h = x[1] - x[0]
        return float(h / 3.0 * (y[0] + y[-1] + 4.0 * y[1:-1:2].sum() + 2.0 * y[2:-1:2].sum()))


def gauss(x, m, var):
    return np.exp(-(x - m) ** 2 / (2.0 * var)) / np.sqrt(2.0 * np.pi * var)


def posterior_moments(mu, sigma2, a, b, z_range, x, tau2, n):
    """E[Z], E[Z^2], E[pi], E[pi^2] under the exact posterior (N(x; Z, tau2) pi + U(x) (1 - pi)) N(Z; mu, sigma2) Beta(pi; a, b), U = 1 / z_range,
    by Simpson's rule on n + 1 points per axis.  The integrand is a sum of two products of a function of Z and a function of pi, so the double
    integral is taken as products of single ones; the Beta's normalisation cancels"""
    s = np.sqrt(sigma2)
    Z = np.linspace(min(mu, x) - 12.0 * s, max(mu, x) + 12.0 * s, n + 1)
    P = np.linspace(0.0, 1.0, n + 1)
    prior = gauss(Z, mu, sigma2)
    like = gauss(x, Z, tau2)
    beta = P ** (a - 1.0) * (1.0 - P) ** (b - 1.0)
    G = [simpson(Z ** k * like * prior, Z) for k in range(3)]
    N = [simpson(Z ** k * prior, Z) for k in range(3)]
    I = [simpson(P ** j * beta, P) for j in range(4)]
    U = 1.0 / z_range
    den = I[1] * G[0] + (I[0] - I[1]) * U * N[0]
    EZ = [(I[1] * G[k] + (I[0] - I[1]) * U * N[k]) / den for k in (1, 2)]
    EP = [(I[j + 1] * G[0] + (I[j] - I[j + 1]) * U * N[0]) / den for j in (1, 2)]
    return np.array(EZ + EP)


def test_the_bayes_update_matches_the_moments_of_the_exact_posterior():
    """The update of step 9 is a moment match: its (mu', sigma2') are the mean and the variance of Z, and its Beta(a', b') has the first two
    moments of pi, under the exact posterior.  Quadrature on 4096 intervals per axis.  Its error is estimated by |fine - coarse| with the
    same rule on 2048 intervals, which for Simpson's fourth order is about 15 x the fine grid's own error; the bound is 16 x that
    estimate (so some 240 x the fine grid's error) plus 1e-9 relative for the cancellation in E[Z^2] - E[Z]^2 (mu / sigma = 8 costs
    64 x the rounding of the two terms).  Both figures are printed for every combination"""
    mu, sigma, z_range = 0.4, 0.05, 1.0
    worst = 0.0
    for dx in (-3.0, -1.0, 0.0, 0.5, 2.0, 5.0):
        for tr in (0.2, 1.0, 3.0):
            for pi0 in (0.2, 0.5, 0.9):
                a, b = 20.0 * pi0, 20.0 * (1.0 - pi0)
                x, tau2 = mu + dx * sigma, (tr * sigma) ** 2
                fine = posterior_moments(mu, sigma * sigma, a, b, z_range, x, tau2, 4096)
                coarse = posterior_moments(mu, sigma * sigma, a, b, z_range, x, tau2, 2048)
                mu2, sg2, a2, b2 = dm.bayes(mu, sigma * sigma, a, b, z_range, x, tau2)
                got = np.array([mu2, sg2 + mu2 * mu2, a2 / (a2 + b2), a2 * (a2 + 1.0) / ((a2 + b2) * (a2 + b2 + 1.0))])
                qerr = np.abs(fine - coarse)
                var_q = fine[1] - fine[0] ** 2
                print("(x - mu) / sigma %4.1f, tau / sigma %.1f, a / (a + b) %.1f: model - quadrature %s, quadrature's own error %s; variance %.6g against %.6g"
                      % (dx, tr, pi0, np.abs(got - fine), qerr, sg2, var_q))
                assert (np.abs(got - fine) <= 16.0 * qerr + 1e-9 * np.abs(fine)).all()
                assert abs(sg2 - var_q) <= 16.0 * (qerr[1] + 2.0 * fine[0] * qerr[0]) + 1e-9 * fine[1]
                worst = max(worst, (np.abs(got - fine) / np.abs(fine)).max())
    print("largest relative deviation of a moment: %.3g" % worst)
    # an inlier at the prior's mean sharpens the estimate and raises the inlier ratio; an outlier far away does neither
    m, s2, a2, b2 = dm.bayes(0.4, 0.0025, 10.0, 10.0, 1.0, 0.4, 0.0025)
    assert s2 < 0.0025 and a2 / (a2 + b2) > 0.5
    m, s2, a2, b2 = dm.bayes(0.4, 0.0025, 10.0, 10.0, 1.0, 0.9, 0.0025)
    assert abs(m - 0.4) < 1e-6 and abs(s2 - 0.0025) < 1e-6 and a2 / (a2 + b2) < 0.5


def _true_matches(sc, t, uv):
    """for the frame-0 pixels uv: (f, R, t, Rf, d (the true distance along f), the true pixel in frame t)"""
    K = sc["K"]
    n = len(uv)
    f = dm.bearing(K, uv)
    d = 1.0 / dm.true_mu(sc, uv)
    R, tv = np.broadcast_to(sc["poses"][t][:3, :3], (n, 3, 3)), np.broadcast_to(sc["poses"][t][:3, 3], (n, 3))
    Rf = np.einsum("nij,nj->ni", R, f)
    X = Rf * d[:, None] + tv
    return f, R, tv, Rf, d, dm.project(K, X), X


def test_tau_is_the_depth_change_of_one_pixel_along_the_epipolar_line():
    """tau of step 8 against the matched pixel moved by px_noise along the epipolar line (towards larger depths) and triangulated again.  The
    law of sines is exact in the epipolar plane; what the formula approximates is the angle of one pixel, 2 atan(1 / (2 fx)), which is the
    angle at the principal point: at an angle theta off the axis a pixel step subtends between cos^2 theta (a radial step) and cos theta
    (a tangential one) of it.  z(beta) is convex, so the perturbed depth change is at most tau, and at least cos^2 theta tau less the
    curvature over the step, which is of relative size tau / z"""
    sc = dm.scene(dm.W, dm.H)
    K = sc["K"]
    uv = dm.random_uv(dm.W, dm.H, 60, 11, margin=12).astype(np.float64)
    for t, px in ((3, 1.0), (6, 1.0), (6, 0.25)):
        f, R, tv, Rf, d, p, X = _true_matches(sc, t, uv)
        tau_inv, tau = dm.noise(f, R, tv, d, px, K[0, 0])
        g = np.stack([K[0, 0] * (Rf[:, 0] * X[:, 2] - X[:, 0] * Rf[:, 2]), K[1, 1] * (Rf[:, 1] * X[:, 2] - X[:, 1] * Rf[:, 2])], 1)
        g /= np.linalg.norm(g, axis=1)[:, None]
        z2 = dm.triangulate(Rf, dm.bearing(K, p + px * g), tv)[0]
        ratio = (z2 - d) / tau
        cos2 = dm.bearing(K, p)[:, 2] ** 2
        slack = 2.0 * tau / d
        print("frame %d, %.2f px: tau / z in [%.4f, %.4f]; (perturbed depth change) / tau in [%.4f, %.4f]; cos^2 theta in [%.4f, 1]"
              % (t, px, (tau / d).min(), (tau / d).max(), ratio.min(), ratio.max(), cos2.min()))
        assert (tau > 0).all() and (ratio <= 1.0 + 1e-9).all() and (ratio >= cos2 - slack).all()
        # tau_inv is the half-width of [1 / (z + tau), 1 / (z - tau)]
        assert np.allclose(tau_inv, 0.5 * (1.0 / (d - tau) - 1.0 / (d + tau)), rtol=1e-12)


def test_triangulation_recovers_synthetic_depths():
    rng = np.random.default_rng(5)
    n = 500
    uv = np.stack([rng.uniform(0, 208, n), rng.uniform(0, 120, n)], 1)
    K = np.array([[400.0, 0, 103.5], [0, 380.0, 59.5], [0, 0, 1]])
    f = dm.bearing(K, uv)
    R = np.stack([dm.rodrigues(rng.normal(0, 0.05, 3)) for _ in range(n)])
    t = rng.normal(0, 0.5, (n, 3))
    d = rng.uniform(2.0, 20.0, n)
    Rf = np.einsum("nij,nj->ni", R, f)
    X = Rf * d[:, None] + t
    keep = X[:, 2] > 0.5
    z, det, tt = dm.triangulate(Rf, X / np.linalg.norm(X, axis=1)[:, None], t)
    # the normal equations square the condition: the error is the rounding of the inputs over det, the squared sine of the parallax angle
    print("largest |z - d| / d %.3g at det %.3g; smallest det %.3g" % ((np.abs(z - d) / d)[keep].max(), det[keep][np.argmax((np.abs(z - d) / d)[keep])], det[keep].min()))
    assert (np.abs(z - d)[keep] <= 1e-13 * d[keep] / det[keep]).all()
    # and through the pixel: the bearing of the projected pixel is the direction of X
    assert np.abs(dm.bearing(K, dm.project(K, X[keep])) - (X / np.linalg.norm(X, axis=1)[:, None])[keep]).max() < 1e-12
    # t = 0 and motion along the bearing are degenerate: det is 0 up to rounding
    assert dm.triangulate(f, f, np.zeros((n, 3)))[1].max() < 1e-15


def test_the_integer_score_is_64_times_the_zero_mean_ssd():
    rng = np.random.default_rng(6)
    P, Q = rng.integers(0, 256, (2000, 64)), rng.integers(0, 256, (2000, 64))
    P[0], Q[0] = 255 * (np.arange(64) % 2), 255 * (1 - np.arange(64) % 2)          # the largest score there is
    P[1], Q[1] = 255, 0
    P[2], Q[2] = P[3], P[3] + 0
    S = dm.score(P, Q)
    p, q = P.astype(np.float64), Q.astype(np.float64)
    zmssd = (((p - p.mean(1, keepdims=True)) - (q - q.mean(1, keepdims=True))) ** 2).sum(1)
    assert np.abs(S - 64.0 * zmssd).max() <= 1e-6 and S.min() >= 0 and S[1] == 0 and S[2] == 0
    assert S.max() == S[0] == 64 * 64 * 255 * 255 < 2 ** 31
    assert dm.DEFAULTS["max_score"] * 64 < 2 ** 31 and 4161600 == 64 * 255 * 255
    # the kernel's form, in 32-bit arithmetic: 64 (sum p^2 + sum q^2 - 2 sum p q) - (sum p - sum q)^2
    u = lambda a: a.astype(np.uint32)
    dS = P.sum(1).astype(np.int32) - Q.sum(1).astype(np.int32)
    S32 = np.uint32(64) * (u((P * P).sum(1)) + u((Q * Q).sum(1)) - np.uint32(2) * u((P * Q).sum(1))) - u(dS * dS)
    assert np.array_equal(S32.astype(np.int64), S)


def test_seed_creation():
    sc = dm.scene(dm.W, dm.H)
    img = sc["frames"][0]
    uv = np.array([[5.0, 5.0], [4.49, 60.0], [203.49, 115.49], [203.5, 60.0], [100.4, 115.5], [np.nan, 30.0], [30.0, np.inf], [1e30, 30.0], [-7.0, 20.0],
                   [57.5, 33.49]], np.float32)
    s, p, ok = dm.init_seeds(img, uv, 8.0, 3.0, ref_id=2)
    assert ok.tolist() == [1, 0, 1, 0, 0, 0, 0, 0, 0, 1]
    assert np.array_equal((s["flags"] & dm.DIVERGED) != 0, ok == 0) and (s["ref_id"] == 2).all()
    assert (s["mu"] == 1.0 / 8.0).all() and (s["z_range"] == 1.0 / 3.0).all() and (s["sigma2"] == (1.0 / 3.0) ** 2 / 36.0).all() and (s["a"] == 10).all()
    assert np.array_equal(p[0].reshape(10, 10), img[0:10, 0:10]) and np.array_equal(p[9].reshape(10, 10), img[28:38, 53:63])       # 57.5 rounds up
    assert np.array_equal(p[2].reshape(10, 10), img[110:120, 198:208]) and not p[1].any()


def test_the_filter_on_the_rendered_sequence():
    """200 random seeds of frame 0 and 7 updates; plus seeds off the image and twelve seeds on the background just right of the foreground
    plane, which covers them from the second or third frame on.  The four quantities come out as printed.  Asserted, against the scene's
    truth at the seed's own pixel: at least half of the random seeds converge; no converged seed is wrong by more than 3 of its own sigma;
    seeds off the image are flagged diverged at birth and only ever skipped.  Covered seeds: none converges.  None is flagged diverged
    within the seven frames either, and cannot be: an outlier is b += 1 and the flag needs a / (a + b) < min_inlier = 0.1, that is
    b > 9 a, from a prior of a = b = 10 -- some eighty outliers.  What holds instead and is asserted: a seed that stays covered takes an
    outlier in every frame, its state otherwise untouched, and is flagged diverged by exactly the update that brings b above 9 a"""
    sc = dm.scene(dm.W, dm.H)
    K = sc["K"]
    uv = dm.random_uv(dm.W, dm.H, 200, 1)
    off = np.array([[2.0, 50.0], [207.0, 3.0], [100.0, 118.0], [-20.0, 40.0], [300.0, 300.0]], np.float32)
    covered = np.stack([np.linspace(156.0, 166.0, 12), np.linspace(36.0, 86.0, 12)], 1).astype(np.float32)
    uv = np.concatenate([uv, off, covered])
    kind = np.array([0] * 200 + [1] * len(off) + [2] * len(covered))
    seeds, patches, ok = dm.init_seeds(sc["frames"][0], uv, dm.DEPTH_MEAN, dm.DEPTH_MIN)
    assert not ok[kind == 1].any() and ok[kind == 2].all()
    codes = []
    for t in range(1, dm.N_FRAMES):
        m = dm.update(seeds, patches, sc["frames"][t], K, dm.pose6(sc["poses"][t])[None])
        seeds = m["seeds"]
        codes.append(m["result"])
        print("frame %d: %s" % (t, dict(zip(dm.NAMES + ("converged", "diverged"), m["stats"].tolist()))))
    codes = np.stack(codes, 1)
    conv = (seeds["flags"] & dm.CONVERGED) != 0
    div = (seeds["flags"] & dm.DIVERGED) != 0
    err = np.abs(seeds["mu"] - dm.true_mu(sc, uv.astype(np.float64))) / np.sqrt(seeds["sigma2"])
    edge = dm.on_occlusion_edge(sc, uv)
    r = kind == 0
    print("random seeds: %d of %d converged within %d frames (%d of them with a patch over both planes), %d diverged"
          % (int((conv & r).sum()), int(r.sum()), dm.N_FRAMES - 1, int((conv & r & edge).sum()), int((div & r).sum())))
    print("their error in units of their own sigma: median %.3f, 90 %% %.3f, max %.3f" % (np.median(err[conv & r]), np.quantile(err[conv & r], 0.9), err[conv & r].max()))
    print("seeds off the image: codes %s" % sorted(set(codes[kind == 1].ravel().tolist())))
    print("covered seeds: converged %s, diverged %s, a / (a + b) %s, error in sigma %s, codes per frame\n%s"
          % (conv[kind == 2].astype(int), div[kind == 2].astype(int), np.round((seeds["a"] / (seeds["a"] + seeds["b"]))[kind == 2], 2), np.round(err[kind == 2], 2),
             codes[kind == 2]))
    assert (conv & r).sum() >= 100
    assert (err[conv] <= 3.0).all()
    assert (codes[kind == 1] == dm.SKIP_INACTIVE).all() and div[kind == 1].all()
    assert not conv[kind == 2].any() and not div[kind == 2].any()
    # the seeds that took an outlier in each of the last four frames stay covered: the last frame again and again
    outl = (codes == dm.OUTLIER_NOMATCH) | (codes == dm.OUTLIER_ALIGN)
    stay = np.nonzero((kind == 2) & outl[:, -4:].all(1))[0]
    assert len(stay) >= 8
    s2, p2 = seeds[stay].copy(), patches[stay]
    need = np.floor(9.0 * s2["a"] - s2["b"]).astype(int) + 1                 # the outliers that bring b above 9 a
    img, pose = sc["frames"][dm.N_FRAMES - 1], dm.pose6(sc["poses"][dm.N_FRAMES - 1])[None]
    taken = np.zeros(len(stay), int)
    for k in range(int(need.max()) + 1):
        m = dm.update(s2, p2, img, K, pose)
        live = (s2["flags"] & dm.DIVERGED) == 0
        assert (m["result"][~live] == dm.SKIP_INACTIVE).all() and np.isin(m["result"][live], (dm.OUTLIER_NOMATCH, dm.OUTLIER_ALIGN)).all()
        assert np.array_equal(m["seeds"]["mu"], s2["mu"]) and np.array_equal(m["seeds"]["sigma2"], s2["sigma2"]) and np.array_equal(m["seeds"]["a"], s2["a"])
        taken += live
        s2 = m["seeds"]
    print("seeds that stay covered: flagged diverged after %s more outliers (b > 9 a needs %s)" % (taken.tolist(), need.tolist()))
    assert ((s2["flags"] & dm.DIVERGED) != 0).all() and np.array_equal(taken, need) and not (s2["flags"] & dm.CONVERGED).any()


ALL_CASES = dm.gpu_cases() + dm.edge_cases()


@pytest.mark.parametrize("case", ALL_CASES, ids=lambda c: c["name"])
def test_the_model_alone_decides_nine_seeds_in_ten_of_every_case(case):
    """a seed is decided when perturbing A and B by +-1e-6 pixels and the float32 switch change none of its discrete outcomes, at this frame
    and at every frame before it"""
    for k, st in enumerate(dm.case_runs(case)):
        n, und = len(st["decided"]), int((~st["decided"]).sum())
        print("%s frame %d: %d of %d seeds undecided; counts %s" % (case["name"], k, und, n, st["m64"]["stats"].tolist()))
        assert und <= 0.1 * n
        with np.errstate(invalid="ignore"):
            moved = [key for key in dm.CONTINUOUS if np.nanmax(np.abs(dm.continuous(st["m32"])[key] - dm.continuous(st["m64"])[key]), initial=0.0) > 0]
        print("   the float32 switch moves: %s" % (moved or "nothing"))


def test_the_gpu_cases_reach_what_they_are_there_for():
    by = {c["name"]: dm.case_runs(c) for c in dm.gpu_cases()}
    last = by["chain_n200"][-1]["m64"]
    assert last["stats"][7] >= 50 and len(by["chain_n200"]) == 6
    assert all(st["m64"]["stats"][dm.UPDATED] >= 100 for st in by["chain_n200"])
    assert by["n257_edges"][0]["m64"]["stats"][dm.SKIP_INACTIVE] > 0                   # patches that leave the image
    assert by["best_pixel_n64"][0]["m64"]["stats"][dm.OUTLIER_NOMATCH] >= 50
    assert (by["iters1_n63"][0]["m64"]["iters"] <= 1).all() and by["iters1_n63"][0]["m64"]["stats"][dm.OUTLIER_ALIGN] > 0
    assert by["steps8_n64"][0]["m64"]["stats"][dm.SKIP_LONG] > 0
    assert max(st["m64"]["n_steps"].max() for st in by["chain_n200"]) > 16 and by["chain_n200"][0]["m64"]["iters"].max() >= 3


@pytest.mark.parametrize("case", dm.edge_cases(), ids=lambda c: c["name"])
def test_the_edge_cases_reach_every_exit_and_boundary(case):
    m = dm.case_runs(case)[0]["m64"]
    for i, l in enumerate(case["labels"]):
        e = case["expect"].get(l)
        if e is None:
            continue
        for key, v in e.items():
            got = m["result"][i] if key == "code" else m[key][i]
            assert got == v, (l, key, got, v)
        if e["code"] >= dm.SKIP_INVISIBLE:
            assert m["seeds"][i].tobytes() == dm.case_data(case)["seeds"][i].tobytes()
    if case["name"] == "leaves":
        assert m["best_px"][0, 0] == dm.W - 5                                             # the last scorable pixel
    if case["name"] == "edges":
        assert set(m["result"].tolist()) == {dm.UPDATED, dm.OUTLIER_ALIGN, dm.SKIP_INVISIBLE, dm.SKIP_LONG, dm.SKIP_DEGENERATE, dm.SKIP_INACTIVE}
        i = case["labels"].index("half_outside")
        assert m["best_k"][i] > 0 and m["n_steps"][i] == 60
        ns = {l: m["n_steps"][case["labels"].index(l)] for l in ("steps0_flat", "steps1", "steps2", "steps64", "steps65", "steps128")}
        assert list(ns.values()) == [0, 1, 2, 64, 65, 128]
