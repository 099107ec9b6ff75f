"""GPU: randomised parity sweeps (hypothesis) -- KLT and Shi-Tomasi bit-exact against the C oracle over random image
sizes, contents, parameters and point sets; bundle adjustment against the numpy oracle over random scene shapes and
visibility patterns.  Deterministic (derandomised) so that a failure reproduces."""
import numpy as np
import pytest
from hypothesis import HealthCheck, Phase, given, settings, strategies as st

pytestmark = pytest.mark.gpu
import os
# no shrink phase: an example costs a context creation + an oracle run, shrinking a failure would take tens of minutes of GPU time
FUZZ = dict(max_examples=int(os.environ.get("VO_FUZZ_EXAMPLES", "80")), deadline=None, derandomize=True, suppress_health_check=list(HealthCheck),
            phases=(Phase.explicit, Phase.reuse, Phase.generate))


def _image(rng, w, h, kind):
    if kind == 0:                                         # smooth texture
        a = rng.normal(0, 1, (h // 4 + 2, w // 4 + 2))
        img = np.kron(a, np.ones((4, 4)))[:h, :w]
        img = (img - img.min()) / (np.ptp(img) + 1e-9) * 255
    elif kind == 1:                                       # white noise
        img = rng.integers(0, 256, (h, w)).astype(float)
    elif kind == 2:                                       # blocks with hard edges and flat areas (zero-gradient windows)
        img = np.kron(rng.integers(0, 2, (h // 16 + 1, w // 16 + 1)) * 200.0 + 20, np.ones((16, 16)))[:h, :w]
    else:                                                 # saturated gradients
        img = np.clip(np.add.outer(np.arange(h) * 3.0, np.arange(w) * 2.0) + rng.normal(0, 8, (h, w)), 0, 255)
    return np.clip(img, 0, 255).astype(np.uint8)


@settings(**FUZZ)
@given(st.integers(40, 400), st.integers(40, 300), st.integers(0, 3), st.integers(0, 2 ** 31 - 1), st.sampled_from([5, 9, 15, 21, 31]),
       st.integers(0, 4), st.integers(1, 30), st.sampled_from([0.003, 0.03, 0.3]))
def test_klt_fuzz(w, h, kind, seed, win, max_level, max_count, eps):
    import vo_oracle as o
    from vo_mi355x import VoContext
    rng = np.random.default_rng(seed)
    im0 = _image(rng, w, h, kind)
    sh = rng.integers(-3, 4, 2)
    im1 = np.clip(np.roll(im0, tuple(sh), (0, 1)).astype(int) + rng.integers(-4, 5, (h, w)), 0, 255).astype(np.uint8)
    n = int(rng.integers(1, 120))
    pts = np.stack([rng.uniform(-20, w + 20, n), rng.uniform(-20, h + 20, n)], 1).astype(np.float32)
    with VoContext(w, h, max_pts=128, max_level=max_level, win=win) as c:
        c.push_frame(im0); c.push_frame(im1)
        prm = c.klt_params(win=win, max_level=max_level, max_count=max_count, epsilon=eps)
        p1, s1, e1, it = c.klt_track(pts, prm, return_iters=True)
    q1, qs, qe, qi = o.klt(im0, im1, pts, winSize=(win, win), maxLevel=max_level, criteria=(3, max_count, eps), return_iters=True)
    assert np.array_equal(p1, q1) and np.array_equal(s1, qs) and np.array_equal(e1, qe) and np.array_equal(it, qi)


@settings(**FUZZ)
@given(st.integers(40, 500), st.integers(40, 300), st.integers(0, 3), st.integers(0, 2 ** 31 - 1), st.sampled_from([3, 7, 15, 31]),
       st.sampled_from([0.5, 1.0, 3.0, 7.0, 20.0]), st.sampled_from([0.001, 0.03, 0.5]), st.integers(0, 9), st.integers(1, 400))
def test_shi_tomasi_fuzz(w, h, kind, seed, bs, md, q, radius, maxc):
    import vo_oracle as o
    from vo_mi355x import VoContext
    if min(w, h) <= bs + 2:
        return
    rng = np.random.default_rng(seed)
    img = _image(rng, w, h, kind)
    n = int(rng.integers(0, 80))
    pts = np.stack([rng.uniform(-5, w + 5, n), rng.uniform(-5, h + 5, n)], 1).astype(np.float32)
    from vo_mi355x import VoError
    with VoContext(w, h, max_pts=128) as c:
        c.push_frame(img)
        try:
            corners = c.shi_tomasi(pts if n else None, radius, params=c.st_params(max_corners=maxc, quality_level=q, min_distance=md, block_size=bs))
        except VoError as e:
            corners = e
        eig, mask, nc = c.shi_tomasi_read()
    m = np.full((h, w), 255, np.uint8)
    for x, y in np.int32(pts):
        o.circle_mask(m, (int(x), int(y)), radius, 0)
    ref, reig, rnc = o.good_features(img, m, maxCorners=maxc, qualityLevel=q, minDistance=md, blockSize=bs, return_aux=True)
    assert np.array_equal(mask, m) and np.array_equal(eig, reig) and nc == rnc
    if isinstance(corners, VoError):
        # the selection's one capacity exit: more than 262144 candidates of one sequence (more than 16384 are consumed in rank-ordered chunks;
        # tests/test_gpu_st_select.py pins the exit).  The images drawn here have at most 150 000 pixels, so this branch should never run
        assert corners.code == -5 and rnc > 262144
    else:
        assert np.array_equal(corners, ref)


@settings(**dict(FUZZ, max_examples=max(10, FUZZ["max_examples"] * 5 // 8)))
@given(st.integers(1, 400), st.integers(1, 20), st.integers(0, 2 ** 31 - 1), st.sampled_from([1.0, 0.9, 0.6, 0.3]), st.sampled_from([0.1, 0.5, 3.0]))
def test_ba_fuzz(n_pts, n_slots, seed, vis, noise):
    import ba_oracle as bo
    from vo_mi355x import VoContext, synthetic as syn
    s = syn.make_ba_scene(n_pts=n_pts, n_slots=n_slots, seed=seed % 1000, visibility=vis, obs_noise=noise)
    rng = np.random.default_rng(seed)
    obs = s["obs"].copy()
    if n_pts > 3:
        obs[:, rng.integers(0, n_pts)] = np.nan                      # a landmark nobody sees
    if n_slots > 2:
        obs[rng.integers(0, n_slots)] = np.nan                       # a frame that sees nothing
    if np.isfinite(obs[..., 0]).sum() < 1:
        return
    # both kernel families (vo_tuning.ba_kernels): the wave-private build / update of windows <= 10 -- every lane map (4, 8 and 5
    # lanes per landmark), every panel width -- on even seeds, the lane-per-observation kernels (windows of 11-20 slots; here forced for every window) on odd ones
    with VoContext(64, 64, max_pts=64) as c:
        c.set_tuning(ba_kernels=2 if seed % 2 == 0 else 1)
        c.ba_upload(s["K"], s["poses0"], s["points0"], obs)
        pr = c.ba_probe(lam=1e-3)
        po, pt, stt = c.ba_adjust(s["K"], s["poses0"], s["points0"], obs, c.ba_params(max_iters=8))
    ne = bo.normal_equations(s["K"], s["poses0"], s["points0"], obs)
    rel = lambda a, b: np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)
    assert rel(pr["Hpp"], ne["Hpp"]) <= 1e-9 and rel(pr["Hll"], ne["Hll"]) <= 1e-9 and rel(pr["gp"], ne["gp"]) <= 1e-9
    assert abs(pr["cost"] - ne["cost"]) <= 1e-10 * ne["cost"] + 1e-14
    assert np.isfinite(po).all() and np.isfinite(pt).all() and np.isfinite(stt["cost"])
    assert abs(bo.cost(s["K"], po, pt, obs) - stt["cost"]) <= 1e-9 * stt["cost"] + 1e-14    # the reported cost is the cost of the returned x
    # (absolute slack: exactly solvable problems end at a cost ~1e-10 px^2 where the residuals are rounding noise)
    assert stt["cost"] <= stt["cost0"] * (1 + 1e-12)                                                 # LM never returns a worse point


@settings(**dict(FUZZ, max_examples=max(10, FUZZ["max_examples"] // 2)))
@given(st.integers(8, 300), st.integers(8, 200), st.integers(0, 3), st.integers(0, 2 ** 31 - 1), st.sampled_from([-1, 3, 5, 7]),
       st.sampled_from([0.5, 1.5, 10.0, 60.0]), st.sampled_from([0.5, 1.5, 3.0]))
def test_prefilter_fuzz(w, h, kind, seed, d, sc, ss):
    import vo_oracle as o
    from vo_mi355x import VoContext
    if d == -1 and ss > 2.0:
        return                                            # diameter from sigma_space would exceed 7
    img = _image(np.random.default_rng(seed), w, h, kind)
    with VoContext(w, h, max_pts=64, max_level=0, win=5) as c:
        c.set_prefilter(d, sc, ss)
        c.push_frame(img)
        got = c.pyramid_read(1, 0)[0]
    assert np.array_equal(got, o.bilateral(img, d, sc, ss))


@settings(**dict(FUZZ, max_examples=max(10, FUZZ["max_examples"] // 2)))
@given(st.integers(1, 500), st.integers(0, 2 ** 31 - 1), st.sampled_from([0.05, 0.5, 3.0]), st.sampled_from([0.0, 0.3, 2.0]))
def test_dlt_fuzz(n, seed, baseline, noise):
    """DLT-1 (SURVEY.md 8a'): relative position error <= 1e-4 against the oracle's SVD for well-conditioned pairs, the
    filter statistics (camera-1 depth, mean reprojection error) consistent for all"""
    import vo_oracle as o
    from vo_mi355x import VoContext, synthetic as syn
    rng = np.random.default_rng(seed)
    K = syn.KITTI_K
    X = np.stack([rng.uniform(-15, 15, n), rng.uniform(-3, 3, n), rng.uniform(6, 80, n)], 1)
    H0, H1 = np.eye(4), np.eye(4)
    H1[:3, :3] = syn.rodrigues(rng.normal(0, 0.02, 3)); H1[:3, 3] = [baseline, 0.05 * baseline, 0.3 * baseline]
    def proj(H):
        p = (X @ H[:3, :3].T + H[:3, 3]) @ K.T
        return (p[:, :2] / p[:, 2:3] + rng.normal(0, noise, (n, 2))).astype(np.float32)
    uv0, uv1 = proj(H0), proj(H1)
    P0, P1 = (K @ H0[:3]).astype(np.float32), (K @ H1[:3]).astype(np.float32)
    with VoContext(64, 64, max_pts=512) as c:
        X4, depth1, reproj = c.triangulate(P0, P1, uv0, uv1, K, H0, H1)
    R4 = o.triangulate(P0, P1, uv0, uv1)
    Xg, Xr = (X4[:3] / X4[3]).T.astype(np.float64), (R4[:3] / R4[3]).T.astype(np.float64)
    par = np.degrees(np.arccos(np.clip(np.sum((X / np.linalg.norm(X, axis=1, keepdims=True)) *
                                              ((X - (-H1[:3, :3].T @ H1[:3, 3])) / np.linalg.norm(X - (-H1[:3, :3].T @ H1[:3, 3]), axis=1, keepdims=True)), 1), -1, 1)))
    good = (par >= 1.0) & np.isfinite(Xr).all(1) & (np.linalg.norm(Xr, axis=1) < 100 * max(baseline, 1e-9) * 100)
    if good.any():
        assert (np.linalg.norm(Xg[good] - Xr[good], axis=1) / np.linalg.norm(Xr[good], axis=1)).max() <= 1e-4
    # statistics recomputed from the returned float32 point exactly as the reference does (extractor.py:271, triangulate.py:15-29)
    Xf = (X4[:3] / X4[3]).T.astype(np.float64)
    d1 = Xf @ H1[2, :3] + H1[2, 3]
    ok = np.isfinite(d1) & np.isfinite(depth1)
    assert np.allclose(depth1[ok], d1[ok], rtol=1e-9, atol=1e-9)


@settings(**dict(FUZZ, max_examples=max(6, FUZZ["max_examples"] // 6)))
@given(st.integers(8, 1500), st.sampled_from([0.0, 0.2, 0.5, 0.7]), st.integers(0, 2 ** 31 - 1), st.sampled_from([0.1, 0.5, 1.0]),
       st.sampled_from([1.0, 2.0, 4.0]))
def test_pnp_fuzz(n, frac, seed, noise, thr):
    """same search as the oracle (hypothesis count, winner, consensus set up to borderline points) and the same refined pose"""
    import pnp_oracle as po
    from vo_mi355x import VoContext, synthetic as syn
    rng = np.random.default_rng(seed)
    s = syn.make_ba_scene(n_pts=n, n_slots=2, seed=seed % 997, obs_noise=noise)
    X = s["points_gt"].astype(np.float32); uv = s["obs"][0].astype(np.float32)
    out = rng.choice(n, int(frac * n), replace=False)
    uv[out] += rng.uniform(-90, 90, (len(out), 2)).astype(np.float32) + np.float32(20)
    sd = int(seed % 1000)
    with VoContext(64, 64, max_pts=64) as c:
        rvec, t, inl, stt = c.pnp_ransac(s["K"], X, uv, reproj_err=thr, seed=sd, max_iters=4096)
    r_o, t_o, inl_o, info = po.pnp_ransac(s["K"], X, uv, thr=thr, seed=sd, max_iters=4096, return_info=True)
    if r_o is None:
        assert stt["status"] != 0
        return
    assert stt["hypotheses"] == info["hyps"]
    if stt["best"] == info["best"]:                          # (two hypotheses with equal support can swap on a borderline point)
        assert len(np.setxor1d(inl, inl_o)) <= 2
        if len(np.setxor1d(inl, inl_o)) == 0:
            assert np.abs(rvec - r_o).max() <= 1e-6 and np.abs(t - t_o).max() <= 1e-5
    else:
        assert abs(len(inl) - len(inl_o)) <= 2


@settings(**dict(FUZZ, max_examples=max(6, FUZZ["max_examples"] // 6)))
@given(st.integers(2, 8), st.integers(9, 700), st.integers(2, 20), st.integers(0, 999), st.sampled_from([1.0, 0.8, 0.5]))
def test_sharded_ba_fuzz(V, N, W, seed, vis):
    """landmark shards on one GPU (batch dimension) reproduce the unsharded solve"""
    from vo_mi355x import VoContext, sharding, synthetic as syn
    s = syn.make_ba_scene(n_pts=N, n_slots=W, seed=seed, visibility=vis)
    kw = dict(max_iters=12)
    with VoContext(64, 64, max_pts=64) as c:
        po, pt, st0 = c.ba_adjust(s["K"], s["poses0"], s["points0"], s["obs"], c.ba_params(**kw))
    Ks, po_s, pt_s, ob_s = sharding.shard_problem(s["K"], s["poses0"], s["points0"], s["obs"], V)
    with VoContext(64, 64, max_pts=64, batch=V) as c:
        c.ba_set_sharded(True)
        po2, pt2, st2 = c.ba_adjust(Ks, po_s, pt_s, ob_s, c.ba_params(**kw))
        pts = sharding.unshard_points(c.ba_gather_points(), N)
    st2 = st2 if isinstance(st2, list) else [st2]
    assert sum(x["n_obs"] for x in st2) == st0["n_obs"]
    assert (st2[0]["iters"], st2[0]["accepted"], st2[0]["status"]) == (st0["iters"], st0["accepted"], st0["status"])
    assert abs(st2[0]["cost"] - st0["cost"]) <= 1e-9 * st0["cost"] + 1e-14
    # (points relative to the scene's extent -- coordinates reach 60: a two-frame window leaves depths weakly determined, and the shards' partial
    #  sums are added in another order; found at VO_FUZZ_EXAMPLES=1500: V=6, N=696, W=2, seed=471 differs by 4.4e-7 at equal iterations and cost)
    assert np.abs(np.asarray(po2)[0] - po).max() <= 1e-7 and np.abs(pts - pt).max() <= 1e-7 * max(1.0, np.abs(pt).max())


@settings(**dict(FUZZ, max_examples=max(6, FUZZ["max_examples"] // 6)))
@given(st.integers(6, 900), st.sampled_from([0.0, 0.2, 0.5]), st.integers(0, 2 ** 31 - 1), st.sampled_from([0.0, 0.3, 1.0]),
       st.sampled_from([0.5, 1.0, 3.0]), st.integers(0, 3))
def test_essential_fuzz(n, frac, seed, noise, thr, motion):
    """five-point RANSAC + recoverPose: same search as the oracle (sample count, winner, model, consensus up to borderline
    points) and the same pose; motions: forward, sideways, rotation-dominant, planar scene"""
    import essential_oracle as eo
    import pnp_oracle as po
    from vo_mi355x import VoContext, synthetic as syn
    rng = np.random.default_rng(seed)
    K = syn.KITTI_K
    rv, tv = [((0.01, 0.03, -0.005), (0.1, -0.02, -0.9)), ((0.0, -0.05, 0.01), (1.0, 0.05, 0.1)), ((0.05, 0.2, -0.1), (0.05, 0.02, 0.05)),
              ((0.01, 0.02, 0.0), (0.4, 0.0, -0.6))][motion]
    R = po.rodrigues(np.asarray(rv, float)); t = np.asarray(tv, float)
    X = np.stack([rng.uniform(-15, 15, n), rng.uniform(-3, 3, n), rng.uniform(8, 45, n)], 1)
    if motion == 3:
        X[:, 2] = 20.0 + 0.3 * X[:, 0]                        # all points on one plane: degenerate for linear solvers, not for five-point
    p1 = X @ K.T; p1 = p1[:, :2] / p1[:, 2:3] + rng.normal(0, noise, (n, 2))
    Xc = X @ R.T + t; p2 = Xc @ K.T; p2 = p2[:, :2] / p2[:, 2:3] + rng.normal(0, noise, (n, 2))
    out = rng.choice(n, int(frac * n), replace=False)
    p2[out] += rng.uniform(-90, 90, (len(out), 2)) + 20
    p1 = p1.astype(np.float32); p2 = p2.astype(np.float32)
    sd = int(seed % 1000)
    with VoContext(64, 64, max_pts=64) as c:
        E, Rg, tg, inl, stt = c.essential_ransac(K, p1, p2, threshold=thr, seed=sd, max_iters=512)
    E_o, R_o, t_o, inl_o, info = eo.essential_ransac(K, p1, p2, thr=thr, seed=sd, max_iters=512, return_info=True)
    if E_o is None:
        assert stt["status"] != 0
        return
    assert stt["status"] == 0 and stt["hypotheses"] == info["hyps"]
    if stt["best"] == info["best"] and min(np.abs(E - E_o).max(), np.abs(E + E_o).max()) <= 1e-6:
        assert len(np.setxor1d(inl, inl_o)) <= 2
        if len(np.setxor1d(inl, inl_o)) == 0 and min([g for g in info["good"] if g != info["n_good"]], default=-10) < info["n_good"] - 2 \
                and sorted(info["good"])[-2] < info["n_good"] - 2:
            assert np.abs(Rg - R_o).max() <= 1e-5 and np.abs(tg - t_o).max() <= 1e-5
    else:                                                    # two models with equal support can swap on a borderline point
        assert abs(len(inl) - len(inl_o)) <= 2
    assert abs(np.linalg.det(Rg) - 1) <= 1e-9 and abs(np.linalg.norm(tg) - 1) <= 1e-9


@settings(**dict(FUZZ, max_examples=max(10, FUZZ["max_examples"] // 3)))
@given(st.integers(1, 300), st.integers(1, 400), st.sampled_from([1, 3, 8, 32, 64, 128, 130]), st.integers(0, 2 ** 31 - 1), st.integers(0, 2))
def test_match_fuzz(n1, n2, dim, seed, kind):
    import match_oracle as mo
    from vo_mi355x import VoContext
    rng = np.random.default_rng(seed)
    if kind == 0:                                             # integer-valued (SIFT-like): many exact ties
        d1 = rng.integers(0, 6, (n1, dim)).astype(np.float32); d2 = rng.integers(0, 6, (n2, dim)).astype(np.float32)
    elif kind == 1:
        d1 = rng.normal(0, 1, (n1, dim)).astype(np.float32); d2 = rng.normal(0, 1, (n2, dim)).astype(np.float32)
    else:                                                     # wide dynamic range
        d1 = (rng.normal(0, 1, (n1, dim)) * 10.0 ** rng.uniform(-3, 3, (n1, 1))).astype(np.float32)
        d2 = (rng.normal(0, 1, (n2, dim)) * 10.0 ** rng.uniform(-3, 3, (n2, 1))).astype(np.float32)
    with VoContext(64, 64, max_pts=64) as c:
        idx, dist = c.match_knn2(d1, d2)
    i_o, d_o = mo.knn2(d1, d2)
    same = idx == i_o
    # the float64 sum is rounded to float32 once on both sides; a sum within one float64 ulp of a rounding boundary may
    # differ in the last float32 bit and then swap two neighbours that are equal to float32 precision
    assert np.allclose(dist, d_o, rtol=2e-7, atol=0) or np.array_equal(dist, d_o)
    assert same.mean() >= 0.995
    if not same.all():
        q = np.nonzero(~same.all(1))[0]
        assert np.allclose(dist[q], d_o[q], rtol=2e-7)


@settings(**dict(FUZZ, max_examples=max(6, FUZZ["max_examples"] // 8)))
@given(st.integers(24, 260), st.integers(24, 200), st.integers(0, 4), st.integers(0, 2 ** 31 - 1), st.sampled_from([0, 40, 300]))
def test_sift_fuzz(w, h, kind, seed, nfeatures):
    """SIFT keypoints and descriptors bit-identical to the oracle over random sizes (odd sizes exercise the decimation and
    the reflection of kernels wider than the top octaves), contents and feature limits"""
    import sift_oracle as so
    from vo_mi355x import VoContext
    rng = np.random.default_rng(seed)
    if kind == 4:                                            # blurred blobs: strong, well-separated extrema
        img = np.zeros((h, w))
        for _ in range(12):
            cx, cy, s = rng.uniform(0, w), rng.uniform(0, h), rng.uniform(1.5, 9)
            yy, xx = np.mgrid[0:h, 0:w]
            img += rng.uniform(-1, 1) * np.exp(-((xx - cx) ** 2 + (yy - cy) ** 2) / (2 * s * s))
        img = np.clip(128 + 120 * img, 0, 255).astype(np.uint8)
    else:
        img = _image(rng, w, h, kind)
    with VoContext(w, h, max_pts=64) as c:
        kp, desc = c.sift_detect_compute(img, nfeatures=nfeatures, max_out=1 << 16)
    kp_o, desc_o = so.detect_and_compute(img, nfeatures=nfeatures)
    assert kp.shape == kp_o.shape and np.array_equal(kp, kp_o)
    assert np.array_equal(desc, desc_o)


@settings(**dict(FUZZ, max_examples=max(10, FUZZ["max_examples"] // 2)))
@given(st.integers(33, 760), st.integers(33, 420), st.integers(0, 3), st.integers(0, 2 ** 31 - 1), st.sampled_from([0, 1, 16, 31, 47, 94, 200]),
       st.sampled_from([1, 2, 5]))
def test_shi_tomasi_fused_kernel_fuzz(w, h, kind, seed, rb, batch):
    """block size 31 goes through k_st_eig_fused: image widths across 1..4 column strips, every band height (the launch picks
    it from the batch size; vo_tuning.st_band_rows forces it here), batches -- eigenvalue map, mask, candidates and corners bit-exact"""
    import os
    import vo_oracle as o
    from vo_mi355x import VoContext
    rng = np.random.default_rng(seed)
    imgs = [_image(rng, w, h, (kind + b) % 4) for b in range(batch)]
    n = int(rng.integers(0, 60))
    pts = np.stack([rng.uniform(-5, w + 5, (batch, n)), rng.uniform(-5, h + 5, (batch, n))], 2).astype(np.float32)
    with VoContext(w, h, max_pts=128, batch=batch) as c:
        c.set_tuning(st_band_rows=int(rb or 0))
        prm = c.st_params(max_corners=300, quality_level=0.03, min_distance=7.0, block_size=31)
        if batch == 1:
            c.push_frame(imgs[0])
            corners = [c.shi_tomasi(pts[0] if n else None, 7, params=prm)]
            eig, mask, nc = (x[None] if isinstance(x, np.ndarray) else np.array([x]) for x in c.shi_tomasi_read())
        else:
            c.push_frame(np.stack(imgs))
            corners = c.shi_tomasi(pts if n else None, 7, params=prm)
            eig, mask, nc = c.shi_tomasi_read()
    for b in range(batch):
        m = np.full((h, w), 255, np.uint8)
        for x, y in np.int32(pts[b]):
            o.circle_mask(m, (int(x), int(y)), 7, 0)
        ref, reig, rnc = o.good_features(imgs[b], m, maxCorners=300, qualityLevel=0.03, minDistance=7.0, blockSize=31, return_aux=True)
        assert np.array_equal(mask[b], m) and np.array_equal(eig[b], reig) and int(nc[b]) == rnc
        assert np.array_equal(np.asarray(corners[b]).reshape(-1, 2), ref.reshape(-1, 2))


@settings(**dict(FUZZ, max_examples=int(os.environ.get("VO_FUZZ_EXAMPLES", "60"))))
@given(st.integers(33, 300), st.integers(33, 200), st.integers(1, 6), st.integers(0, 2 ** 31 - 1), st.sampled_from(["pinned", "pinned_block", "pageable", "strided", "mixed"]),
       st.sampled_from([0, 1, 3, 7, 64]), st.sampled_from([0, 1, 2]))
def test_host_frames_fuzz(w, h, batch, seed, source, workgroups, layout):
    """`vo_frame_step_host` delivers exactly the caller's images: odd widths (the gather's byte tails), page-locked views at any alignment, one
    page-locked block, pageable arrays, rows with a stride, a mix of page-locked and pageable images, any workgroup count of the gather, every
    stream layout -- level 0 of the frame store after the step = the images handed over, and the tracker's results = the resident step's"""
    from vo_mi355x import VoContext
    rng = np.random.default_rng(seed)
    imgs = [[_image(rng, w, h, int(rng.integers(0, 4))) for _ in range(3)] for _ in range(batch)]       # [batch][frame]
    n = int(rng.integers(1, 40))
    pts = np.stack([rng.uniform(0, w, (batch, n)), rng.uniform(0, h, (batch, n))], 2).astype(np.float32)
    frames = np.array(imgs)                                                       # [batch, 3, h, w]

    def give(f):
        if source == "pinned_block":
            blk = VoContext.host_alloc((batch, h, w)); blk[:] = frames[:, f]
            return blk
        out = []
        extra = int(rng.integers(1, 40))                                          # (the images of a step share one row stride)
        for b in range(batch):
            if source == "pinned" or (source == "mixed" and b % 2 == 0):
                off = int(rng.integers(0, 17))                                    # any alignment
                raw = VoContext.host_alloc((h * w + 16,))
                a = raw[off:off + h * w].reshape(h, w); a[:] = frames[b, f]
            elif source == "strided":
                wide = np.zeros((h, w + extra), np.uint8); wide[:, :w] = frames[b, f]
                a = wide[:, :w]
            else:
                a = frames[b, f].copy()
            out.append(a)
        return out

    with VoContext(w, h, max_pts=64, batch=batch) as c:
        c.upload_sequence(frames if batch > 1 else frames[0])
        c.points_upload(pts if batch > 1 else pts[0])
        c.push_frame_resident(0)
        ref = []
        for f in (1, 2):
            c.frame_step_resident(f, n, do_dlt=False, do_ba=False, do_st=False)
            r = c.frame_fetch(); ref.append((r["points2d"].copy(), r["status"].copy(), r["err"].copy()))
    with VoContext(w, h, max_pts=64, batch=batch) as c:
        c.set_side_stream(layout)
        c.set_tuning(gather_workgroups=workgroups)
        c.points_upload(pts if batch > 1 else pts[0])
        c.push_frame(frames[:, 0] if batch > 1 else frames[0, 0])
        keep = []
        for k, f in enumerate((1, 2)):
            g = give(f); keep.append(g)
            c.frame_step_host(g, n, do_dlt=False, do_ba=False, do_st=False)
            r = c.frame_fetch()
            for x, y in zip((r["points2d"], r["status"], r["err"]), ref[k]):
                assert np.array_equal(x, y), (k, source)
            for b in range(batch):
                assert np.array_equal(c.pyramid_read(1, 0, seq=b)[0], frames[b, f]), (k, b, source)
