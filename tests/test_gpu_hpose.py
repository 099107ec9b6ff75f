"""GPU: the pose from a homography (csrc/vo_hpose.hip) against the float64 model of tests/hpose_model.py and its 60-digit restatement,
through VoContext.decompose_homography / homography_pose and Extractor.camera_pose_planar / bootstrap_pose.

Every candidate lies within FACTOR x s of the mpmath candidate (s its sensitivity to 2^-53 of an entry of H), and within twice that of the
model's at the same rank; tests/test_hpose_model.py shows that no voting point of any problem used here lies within 1e-9 of zero in a
visibility dot product or within 1e-6 of the Sampson threshold, so counts, order and verdict are compared for equality.  Every figure is
printed before it is asserted."""
import ctypes

import numpy as np
import pytest

import essential_model as em
import homography_model as hm
import hpose_model as hp

pytestmark = pytest.mark.gpu
SEED = hm.SEARCH_SEED
_REF, _WORST = {}, {}


@pytest.fixture(scope="module")
def ctx():
    from vo_mi355x import VoContext
    with VoContext(64, 64, max_pts=64) as c:
        yield c


def _ref(K, H):
    key = (np.asarray(K, np.float64).tobytes(), np.asarray(H, np.float64).tobytes())
    if key not in _REF:
        _REF[key] = hp.mp_model(K, H)
    return _REF[key]


def _call(c, K, H, p1=None, p2=None, mask=None, hint=None, **kw):
    return dict(zip(("R", "t", "n", "st"), c.decompose_homography(K, H, p1, p2, mask, normal_hint=hint, **kw)))


def _same(a, b):
    return em.bits_equal(a["R"], b["R"]) and em.bits_equal(a["t"], b["t"]) and em.bits_equal(a["n"], b["n"]) and \
        {k: v for k, v in a["st"].items() if k != "sigma"} == {k: v for k, v in b["st"].items() if k != "sigma"} and \
        em.bits_equal(a["st"]["sigma"], b["st"]["sigma"])


def _check(tag, r, K, H, p1=None, p2=None, mask=None, hint=None, **kw):
    """a result against the model (counts, order, verdict: equal) and the 60-digit candidates (within FACTOR x s) -> the worst ratio"""
    m = hp.hpose(K, H, p1, p2, mask, hint=hint, **kw)
    st, ns = r["st"], m["n_solutions"]
    ref = _ref(K, H)
    ratio = hp.worst_ratio(r["R"], r["t"], r["n"], st["n_solutions"], ref)
    smax = max(c["s"] for c in ref)
    pos = 0.0
    # where the model's order rests on a rounding (the traces of two coinciding pairs, the n_z of a horizontal normal when no point votes) the
    # candidates are compared with the 60-digit ones only, not rank by rank
    ranked = m["order_decided"]
    for k in range(min(ns, st["n_solutions"]) if ranked else 0):
        pos = max(pos, np.abs(r["R"][k] - m["R"][k]).max(), np.abs(r["n"][k] - m["n"][k]).max())
        if ns == 4:
            pos = max(pos, np.abs(r["t"][k] / np.linalg.norm(r["t"][k]) - m["t"][k] / np.linalg.norm(m["t"][k])).max())
    print("k_hpose %-18s %d solutions (%d distinct), n_good %s (model %s), n_off %s (model %s), ambiguous %d (model %d); error / s = %.3f (FACTOR %g), "
          "against the model at the same rank %.2e (s = %.2e)" % (tag, st["n_solutions"], st["n_distinct"], st["n_good"], [int(x) for x in m["n_good"]], st["n_off"],
                                                                  [int(x) for x in m["n_off"]], st["ambiguous"], m["ambiguous"], ratio, hp.FACTOR, pos, smax))
    assert st["status"] == 0 and (st["n_solutions"], st["n_distinct"], st["ambiguous"], st["n_mask"]) == (ns, m["n_distinct"], m["ambiguous"], m["n_mask"]), tag
    assert st["n_good"] == list(m["n_good"]) and st["n_off"] == list(m["n_off"]) and st["rotation_only"] == m["rotation_only"], tag
    assert np.isnan(r["R"][ns:]).all() and np.isnan(r["t"][ns:]).all() and np.isnan(r["n"][ns:]).all()
    assert np.abs(st["sigma"] - m["sigma"]).max() <= 2 * hp.FACTOR * smax
    assert ratio <= hp.FACTOR and pos <= 2 * hp.FACTOR * smax, tag
    _WORST[tag] = ratio
    return m


# ---- (a) candidates, counts, order and verdict; the loop edges of the vote; inputs --------------------------------------------------------
def test_every_problem_against_the_model(ctx):
    """fronto, plane, plane with each hint, plane + off-plane points, pure rotation, head-on wall, ground plane; n = 1 .. 257 on fronto; H at
    another scale and sign; a cleared subset of the mask; a K with unequal focal lengths and an off-centre principal point"""
    seen = {}
    for tag, K, H, p1, p2, mask, kw in hp.gpu_problems():
        r = _call(ctx, K, H, p1, p2, mask, **kw)
        seen[tag] = (r, _check(tag, r, K, H, p1, p2, mask, **kw))
    assert seen["fronto"][0]["st"]["n_good"] == [40, 24, 16, 0] and seen["fronto"][0]["st"]["ambiguous"] == 0
    assert seen["plane"][0]["st"]["ambiguous"] == 1 and seen["plane hint 0"][0]["st"]["ambiguous"] == 0
    assert np.abs(seen["plane hint 1"][0]["n"][0] - seen["plane"][0]["n"][1]).max() < 1e-12
    assert seen["plane+off"][0]["st"]["n_off"][:2] == [10, 1] and seen["plane+off"][0]["st"]["ambiguous"] == 0
    assert seen["pure_rotation"][0]["st"]["rotation_only"] and not seen["pure_rotation"][0]["t"][0].any()
    assert seen["wall"][0]["st"]["n_distinct"] == 2
    # the cleared points left n_good for the n_off test (on the plane they fit either candidate's epipolar geometry)
    assert seen["plane mask"][0]["st"]["n_good"][:2] == [37, 37] and seen["plane mask"][0]["st"]["n_off"] == [3, 3, 3, 3]
    for f in ("plane x -3.7", "plane x 1e+06"):
        a, b = seen["plane"][0], seen[f][0]
        assert {k: v for k, v in a["st"].items() if k != "sigma"} == {k: v for k, v in b["st"].items() if k != "sigma"}


def test_no_points_is_the_pure_decomposition(ctx):
    s = hp.exact_scene("plane", 40)
    r = _call(ctx, s["K"], s["H"])
    _check("plane n=0", r, s["K"], s["H"])
    assert r["st"]["n_good"] == [0, 0, 0, 0] and r["st"]["n_off"] == [0, 0, 0, 0] and r["st"]["n_mask"] == 0 and r["st"]["ambiguous"] == 1


def test_nan_rows_and_the_null_mask(ctx):
    s = hp.exact_scene("fronto", 65)
    p1, p2 = s["p1"].copy(), s["p2"].copy()
    p1[5] = np.nan
    p2[64, 1] = np.nan
    p2[11, 0] = np.inf
    r = _call(ctx, s["K"], s["H"], p1, p2)
    m = _check("fronto NaN rows", r, s["K"], s["H"], p1, p2)
    assert m["n_mask"] == 62
    keep = np.ones(65, bool)
    keep[[5, 11, 64]] = False
    assert _call(ctx, s["K"], s["H"], p1[keep], p2[keep])["st"]["n_good"] == r["st"]["n_good"]
    assert _same(_call(ctx, s["K"], s["H"], s["p1"], s["p2"]), _call(ctx, s["K"], s["H"], s["p1"], s["p2"], np.ones(65, np.uint8)))


def test_the_kernel_factor(ctx):
    """the kernel's worst error / s over the decompositions the model's own factor is measured on"""
    worst = 0.0
    for tag, K, H in hp.variants():
        r = _call(ctx, K, H)
        _check(tag, r, K, H)
        worst = max(worst, _WORST[tag])
    print("worst ratio of the kernel %.3f (recorded %.3f), of the model recorded %.3f; FACTOR %.1f" % (worst, hp.MEASURED["kernel"], hp.MEASURED["model"], hp.FACTOR))
    assert hp.MEASURED["kernel"] / 2 <= worst <= 2 * hp.MEASURED["kernel"]
    assert max(hp.MEASURED.values()) <= hp.FACTOR <= 10 * max(hp.MEASURED.values())


# ---- (b) batch, fused path, workspace ------------------------------------------------------------------------------------------------------
def test_batch_of_three(ctx):
    from vo_mi355x import VoContext
    a, b = hp.exact_scene("plane", 40), hp.exact_scene("pure_rotation", 40)
    Hs = np.stack([a["H"], b["H"], np.full((3, 3), np.nan)])
    p1, p2 = np.stack([a["p1"], b["p1"], a["p1"]]), np.stack([a["p2"], b["p2"], a["p2"]])
    with VoContext(64, 64, max_pts=64, batch=3) as c:
        R, t, n, st = c.decompose_homography(hp.K, Hs, p1, p2)          # returns (VO_OK) with a sequence that has no solution
    for i, s in enumerate((a, b)):
        assert _same(dict(R=R[i], t=t[i], n=n[i], st=st[i]), _call(ctx, s["K"], s["H"], s["p1"], s["p2"])), i
    assert st[2]["status"] == hp.VO_E_NUMERIC and st[2]["n_solutions"] == 0 and st[2]["n_good"] == [0, 0, 0, 0] and st[2]["n_mask"] == 0
    assert np.isnan(R[2]).all() and np.isnan(t[2]).all() and np.isnan(n[2]).all() and np.isnan(st[2]["sigma"]).all()
    assert _same(dict(R=R[2], t=t[2], n=n[2], st=st[2]), _call(ctx, hp.K, Hs[2], a["p1"], a["p2"]))
    for bad in (np.zeros((3, 3)), np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 0]])):
        assert _call(ctx, hp.K, bad)["st"]["status"] == hp.VO_E_NUMERIC
    K0 = hp.K.copy()
    K0[1, 1] = 0.0
    assert _call(ctx, K0, a["H"], a["p1"], a["p2"])["st"]["status"] == hp.VO_E_NUMERIC


def _unit_homography(c, p1, p2, **kw):
    """vo_homography_ransac as it returns: H of unit norm (VoContext.find_homography divides by h33), the mask"""
    from vo_mi355x import _lib
    prm = _lib.HomParams()
    c._L.vo_homography_default_params(ctypes.byref(prm))
    for k, v in kw.items():
        setattr(prm, k, v)
    n = len(p1)
    H, mask = np.zeros((3, 3)), np.zeros(n, np.uint8)
    q1, q2 = np.ascontiguousarray(p1, np.float32), np.ascontiguousarray(p2, np.float32)
    assert c._L.vo_homography_ransac(c._h, _lib.ptr(q1, ctypes.c_float), _lib.ptr(q2, ctypes.c_float), n, ctypes.byref(prm),
                                     _lib.ptr(H, ctypes.c_double), None, _lib.ptr(mask, ctypes.c_uint8), None) == 0
    return H, mask


@pytest.mark.parametrize("name,n", [("fronto", 40), ("plane+noise", 200)])
def test_fused_path_bit_for_bit(ctx, name, n):
    s = hm.planar_noisy(n) if name == "plane+noise" else hm.scene(name, n, hm.FULL_SEED)
    f = ctx.homography_pose(em.K, s["p1"], s["p2"], seed=SEED)
    Hu, mask = _unit_homography(ctx, s["p1"], s["p2"], seed=SEED)
    H, inl, hst, _H0 = ctx.find_homography(s["p1"], s["p2"], seed=SEED)
    two = _call(ctx, em.K, Hu, s["p1"], s["p2"], mask)
    fused = dict(zip(("R", "t", "n", "st"), f[3:]))
    print("homography_pose %s n=%d: %d inliers, n_good %s, n_off %s, ambiguous %d" % (name, n, hst["n_inliers"], fused["st"]["n_good"], fused["st"]["n_off"],
                                                                                      fused["st"]["ambiguous"]))
    assert em.bits_equal(f[0], H) and np.array_equal(f[1], inl) and np.array_equal(np.nonzero(mask)[0], inl) and f[2]["n_inliers"] == hst["n_inliers"]
    assert fused["st"]["status"] == 0 and fused["st"]["n_mask"] == hst["n_inliers"] and _same(fused, two)
    again = ctx.homography_pose(em.K, s["p1"], s["p2"], seed=SEED)
    assert em.bits_equal(again[0], f[0]) and _same(dict(zip(("R", "t", "n", "st"), again[3:])), fused)


def test_workspace_grows_and_is_reused():
    from vo_mi355x import VoContext
    small, big = hp.exact_scene("plane", 40), hp.exact_scene("plane", 2000)
    with VoContext(64, 64, max_pts=64) as c:
        first = _call(c, small["K"], small["H"], small["p1"], small["p2"])
        r = _call(c, big["K"], big["H"], big["p1"], big["p2"])
        assert r["st"]["n_good"] == [2000, 2000, 0, 0] and r["st"]["n_mask"] == 2000
        assert _same(_call(c, small["K"], small["H"], small["p1"], small["p2"]), first)
        f1 = c.homography_pose(em.K, small["p1"], small["p2"], seed=SEED)
        c.homography_pose(em.K, big["p1"], big["p2"], seed=SEED)
        f2 = c.homography_pose(em.K, small["p1"], small["p2"], seed=SEED)
        assert em.bits_equal(f1[0], f2[0]) and _same(dict(zip(("R", "t", "n", "st"), f1[3:])), dict(zip(("R", "t", "n", "st"), f2[3:])))


# ---- (c) parameters ----------------------------------------------------------------------------------------------------------------------------
def test_invalid_parameters(ctx):
    from vo_mi355x import VoError, _lib
    s = hp.exact_scene("plane", 40)
    bad = [dict(ratio=0.0), dict(ratio=1.5), dict(ratio=np.nan), dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=np.inf), dict(threshold=np.nan),
           dict(min_off=-1), dict(hint=(0.0, 0.0, 0.0)), dict(hint=(0.0, np.nan, 1.0)), dict(hint=(np.inf, 0.0, 0.0))]
    for kw in bad:
        with pytest.raises(VoError) as e:
            _call(ctx, s["K"], s["H"], s["p1"], s["p2"], **kw)
        assert e.value.code == -1 and str(e.value), kw
        with pytest.raises(VoError) as e:
            ctx.homography_pose(s["K"], s["p1"], s["p2"], **{dict(hint="normal_hint", threshold="pose_threshold").get(k, k): v for k, v in kw.items()})
        assert e.value.code == -1, kw
    L, h = ctx._L, ctx._h
    K, H = np.ascontiguousarray(s["K"], np.float64), np.ascontiguousarray(s["H"], np.float64)
    p1 = np.ascontiguousarray(s["p1"])
    kp, hp_, pp = _lib.ptr(K, ctypes.c_double), _lib.ptr(H, ctypes.c_double), _lib.ptr(p1, ctypes.c_float)
    for args in ((kp, hp_, None, None, None, -1), (kp, hp_, None, pp, None, 40), (kp, hp_, pp, None, None, 40), (None, hp_, None, None, None, 0),
                 (kp, None, None, None, None, 0)):
        assert L.vo_homography_decompose(h, *args, None, None, None, None, None) == -1
        assert L.vo_last_error(h)
    assert L.vo_homography_pose(h, kp, pp, pp, -1, None, None, hp_, None, None, None, None, None, None) == -1 and L.vo_last_error(h)
    assert L.vo_homography_pose(h, kp, None, pp, 40, None, None, hp_, None, None, None, None, None, None) == -1 and L.vo_last_error(h)
    r = _call(ctx, s["K"], s["H"], s["p1"], s["p2"], ratio=1.0, min_off=0)          # the edges of the valid ranges
    assert r["st"]["status"] == 0 and r["st"]["ambiguous"] == 0                      # a lead of 0 >= min_off = 0 decides


# ---- (d) Extractor -------------------------------------------------------------------------------------------------------------------------------
def _keypoints(p):
    from vo_mi355x import Keypoint
    return [Keypoint(0, 1, uv.reshape(2, 1), uv.reshape(2, 1), np.zeros((1, 1)), [uv.reshape(2, 1)]) for uv in np.asarray(p, np.float32)]


# the scenes' points are exact up to their float32 rounding (2^-14 px); a pose error e moves the far points by about f e = 718 e px, so 1e-4
# allows 0.07 px: a thousand roundings, and a fourteenth of the 1 px inlier threshold the fit was made at
POSE_FIT_TOL = 1e-4


def test_extractor(ctx):
    from vo_mi355x import Extractor
    ext = Extractor(lazy=False, min_kp_dist=7, ctx=ctx)
    n = hm.BOOTSTRAP_N
    s = hm.scene("general", n, hm.FULL_SEED)
    k1, k2 = _keypoints(s["p1"]), _keypoints(s["p2"])
    got = ext.bootstrap_pose(em.K, k1, k2)
    inl, H4 = ext.camera_pose(em.K, k1, k2, corr='2D-2D')
    print("bootstrap_pose general:", got["model"], got["check"])
    assert got["model"] == 'essential' and em.bits_equal(got["H"], H4) and got["inliers"] == inl and got["ambiguous"] is False
    assert got["check"] == ext.bootstrap_check(em.K, k1, k2)

    s = hm.scene("fronto", n, hm.FULL_SEED)
    k1, k2 = _keypoints(s["p1"]), _keypoints(s["p2"])
    got = ext.bootstrap_pose(em.K, k1, k2, seed=SEED)
    tu = s["t"] / np.linalg.norm(s["t"])
    eR, et = np.abs(got["H"][:3, :3] - s["R"]).max(), np.abs(got["H"][:3, 3] - tu).max()
    print("bootstrap_pose fronto:", got["model"], got["check"], "n_good", got["info"]["n_good"], "|dR| %.2e |dt| %.2e" % (eR, et))
    assert got["model"] == 'homography' and got["ambiguous"] is False and got["check"]["degenerate"]
    assert abs(np.linalg.norm(got["H"][:3, 3]) - 1.0) <= em.POSE_TOL and eR <= POSE_FIT_TOL and et <= POSE_FIT_TOL
    inl, H4, info = ext.camera_pose_planar(em.K, k1, k2, threshold=1.0, seed=SEED)
    Hh, h_inl, _st, _H0 = ext.find_homography(k1, k2, threshold=1.0, seed=SEED)
    assert inl == h_inl and em.bits_equal(H4, got["H"]) and em.bits_equal(info["homography"], Hh)
    assert len(info["alternatives"]) == 4 and not info["rotation_only"] and not info["ambiguous"]

    s = hm.scene("plane", n, hm.FULL_SEED)
    got = ext.bootstrap_pose(em.K, _keypoints(s["p1"]), _keypoints(s["p2"]), seed=SEED)
    print("bootstrap_pose plane:", got["model"], got["check"], "n_good", got["info"]["n_good"])
    assert got["model"] == 'homography' and got["ambiguous"] is True and len(got["info"]["alternatives"]) == 4
    hinted = ext.bootstrap_pose(em.K, _keypoints(s["p1"]), _keypoints(s["p2"]), seed=SEED, normal_hint=(-0.5, -0.3, 1.0))
    tu = s["t"] / np.linalg.norm(s["t"])
    assert hinted["ambiguous"] is False and np.abs(hinted["H"][:3, :3] - s["R"]).max() <= POSE_FIT_TOL and np.abs(hinted["H"][:3, 3] - tu).max() <= POSE_FIT_TOL

    s = hm.scene("pure_rotation", n, hm.FULL_SEED)
    got = ext.bootstrap_pose(em.K, _keypoints(s["p1"]), _keypoints(s["p2"]), seed=SEED)
    print("bootstrap_pose pure_rotation:", got["model"], got["check"], "sigma", got["info"]["sigma"])
    assert got["model"] == 'rotation' and not got["H"][:3, 3].any() and got["ambiguous"] is False
    assert np.abs(got["H"][:3, :3] - s["R"]).max() <= POSE_FIT_TOL

    with pytest.raises(RuntimeError):
        Extractor(lazy=False, min_kp_dist=7).bootstrap_pose(em.K, k1, k2)
