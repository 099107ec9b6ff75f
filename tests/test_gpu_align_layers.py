"""GPU: the Python layers over the sparse image alignment -- VoContext.sparse_align against the raw call, Extractor.align_frame /
project_landmarks / extend_landmarks(init=) against the context's own calls, and init=None against the call without the keyword."""
import copy

import numpy as np
import pytest

import align_model as am
from test_gpu_align import raw_align

pytestmark = pytest.mark.gpu


def _case(name):
    (c,) = [c for c in am.gpu_cases() if c["name"] == name]
    return c


def test_context_method_equals_the_raw_call():
    from vo_mi355x import VoContext
    sc = am.scene(am.W, am.H)
    with VoContext(am.W, am.H, max_pts=256) as c:
        for name in ("init_pose", "nan_and_behind", "n9"):
            case = _case(name)
            c.push_frame(sc["frames"][case["t"]]); c.push_frame(sc["frames"][case["t"] + 1])
            rc, rv, tv, mask, st = raw_align(c, case["K"], case["X"], case["rvec0"], case["tvec0"], **case["params"])
            r2, t2, used, stats = c.sparse_align(case["K"], case["X"], case["rvec0"], case["tvec0"], c.align_params(**case["params"]))
            assert rc == 0 and r2.tobytes() == rv[0].tobytes() and t2.tobytes() == tv[0].tobytes()
            assert used.dtype == bool and np.array_equal(used, mask[0] != 0)
            s = st[0]
            assert stats == dict(status=s.status, n_used=s.n_used, levels_run=s.levels_run, flags=s.flags, iters=list(s.iters), chi2=s.chi2, zbar=s.zbar)
        # the defaults are the defaults
        case = _case("n64")
        c.push_frame(sc["frames"][case["t"]]); c.push_frame(sc["frames"][case["t"] + 1])
        a, b = c.sparse_align(case["K"], case["X"]), c.sparse_align(case["K"], case["X"], params=c.align_params(-1, 0, 10, 10, 10.0, 1e-5))
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[3] == b[3]
        with pytest.raises(ValueError):
            c.sparse_align(case["K"], case["X"], rvec0=np.zeros(3))


def _world(case, H_prev):
    """landmarks and their keypoints in frame t for the case's points (rows in front of the camera), world = H_prev^-1 camera t"""
    from vo_mi355x import Keypoint, Landmark
    X = case["X"].astype(np.float64)
    Hi = np.linalg.inv(H_prev)
    P = X @ Hi[:3, :3].T + Hi[:3, 3]
    uv = am.project(case["K"], 0, X).astype(np.float32)
    lms = [Landmark(1, p.reshape(3, 1).copy(), np.zeros((1, 1))) for p in P]
    kps = [Keypoint(0, 2, u.reshape(2, 1).copy(), u.reshape(2, 1).copy(), np.zeros((1, 1)), [u.reshape(2, 1).copy()]) for u in uv]
    return lms, kps, uv


def test_align_frame_then_seeded_extend_landmarks_equals_the_contexts_calls_and_pushes_each_image_once():
    from vo_mi355x import Extractor, VoContext
    from vo_mi355x.so3 import rodrigues_vec_to_mat
    sc = am.scene(am.W, am.H)
    case = _case("n64")
    t, K = case["t"], case["K"]
    H_prev = np.eye(4)
    H_prev[:3, :3], H_prev[:3, 3] = am.rodrigues([0.01, -0.02, 0.03]), [0.3, -0.1, 0.2]
    lms, kps, p0 = _world(case, H_prev)
    im_prev, im_curr = sc["frames"][t], sc["frames"][t + 1]
    with VoContext(am.W, am.H, max_pts=256) as c:
        pushed = []
        push = c.push_frame
        c.push_frame = lambda img: (pushed.append(np.array(img)), push(img))[1]
        ext = Extractor(lazy=False, min_kp_dist=7, ctx=c)
        ext._im_prev = im_prev
        H_cur, info = ext.align_frame(K, im_curr, lms, H_prev)
        g = ext.project_landmarks(K, H_cur, lms)
        assert g.shape == (len(lms), 2) and g.dtype == np.float32
        l2, k2 = copy.deepcopy(lms), copy.deepcopy(kps)
        l_new, k_new, l_dead, k_dead = ext.extend_landmarks(im_curr, l2, k2, max_bidir_error=np.inf, init=g)
        assert len(pushed) == 2 and np.array_equal(pushed[0], im_prev) and np.array_equal(pushed[1], im_curr)
        # the pose: the context's call on the landmarks moved into the previous camera's frame on the host
        Xp = np.array([np.asarray(l.p, np.float64).reshape(3) for l in lms]) @ H_prev[:3, :3].T + H_prev[:3, 3]
        rv, tv, used, st = c.sparse_align(K, Xp.astype(np.float32))
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = rodrigues_vec_to_mat(rv), tv
        assert (T @ H_prev).tobytes() == H_cur.tobytes() and info["used"] == np.nonzero(used)[0].tolist()
        assert info["status"] == 0 and info["iters"] == st["iters"] and info["n_used"] == st["n_used"]
        motion, err = am.prediction_error(K, case["X"], T[:3, :3], T[:3, 3], *am.true_pose(sc, t))
        seed_err = np.median(np.linalg.norm(g - am.project(K, 0, case["X"].astype(np.float64) @ am.true_pose(sc, t)[0].T + am.true_pose(sc, t)[1]), axis=1))
        print("align_frame: median image motion %.3f px, prediction error %.4f px; the seeds are %.4f px from the true positions" % (motion, err, seed_err))
        assert err <= motion / 10.0 and seed_err <= motion / 10.0
        # the tracker: the context's seeded call, bit for bit
        p1, status, _err = c.klt_track(p0, ext._klt_prm(), init=g)
        h, w = im_curr.shape
        keep = ~np.isnan(p1).any(axis=1) & (p1[:, 0] >= 0) & (p1[:, 0] <= w) & (p1[:, 1] >= 0) & (p1[:, 1] <= h)
        print("seeded extend_landmarks: %d of %d landmarks survive" % (keep.sum(), len(lms)))
        assert len(k_new) == keep.sum() > 0.8 * len(lms) and len(l_dead) == len(lms) - keep.sum()
        got = np.array([k.uv.reshape(2) for k in k_new])
        assert got.tobytes() == p1[keep].astype(np.float64).tobytes()
        assert len(pushed) == 2
        # H_init: a guess for H_cur; the truth as the guess stays at the truth
        Rt, tt = am.true_pose(sc, t)
        Tt = np.eye(4); Tt[:3, :3], Tt[:3, 3] = Rt, tt
        H2, info2 = ext.align_frame(K, im_curr, lms, H_prev, H_init=Tt @ H_prev, max_iters=5)
        T2 = H2 @ np.linalg.inv(H_prev)
        _m, err2 = am.prediction_error(K, case["X"], T2[:3, :3], T2[:3, 3], Rt, tt)
        print("align_frame from the true pose as H_init: prediction error %.4f px, iters %s" % (err2, info2["iters"][:2]))
        assert err2 <= motion / 10.0 and max(info2["iters"]) <= 5 and len(pushed) == 2
        # too few landmarks: the guess comes back with a status
        H3, info3 = ext.align_frame(K, im_curr, lms[:5], H_prev)
        assert info3["status"] == am.VO_E_NUMERIC and np.abs(H3 - H_prev).max() <= 1e-15 and info3["used"] == []


@pytest.mark.parametrize("predict", ["off", "constant_velocity"])
def test_init_none_is_the_call_without_the_keyword(predict):
    from vo_mi355x import Extractor, VoContext
    sc = am.scene(am.W, am.H)
    case = _case("n64")
    t = case["t"]
    lms, kps, p0 = _world(case, np.eye(4))
    for k in kps:                                              # a history of two entries, so that constant velocity has something to predict from
        k.uv_history.insert(0, (k.uv - np.float32(1.5)).astype(np.float32))
    outs = []
    with VoContext(am.W, am.H, max_pts=256) as c:
        for kw in ({}, dict(init=None)):
            ext = Extractor(lazy=False, min_kp_dist=7, ctx=c, predict=predict)
            ext._im_prev = sc["frames"][t]
            l2, k2 = copy.deepcopy(lms), copy.deepcopy(kps)
            r = ext.extend_landmarks(sc["frames"][t + 1], l2, k2, max_bidir_error=np.inf, **kw)
            tr = ext.extend_tracks(sc["frames"][t + 1], copy.deepcopy(kps), max_bidir_error=np.inf, **kw)
            outs.append((np.array([k.uv for k in r[1]]), len(r[2]), np.array([k.uv for k in tr])))
        # and a given init is used: the tracker's own call with it
        ext = Extractor(lazy=False, min_kp_dist=7, ctx=c, predict=predict)
        ext._im_prev = sc["frames"][t]
        g = p0 + np.float32(2.0)
        tr = ext.extend_tracks(sc["frames"][t + 1], copy.deepcopy(kps), max_bidir_error=np.inf, init=g)
        p1, _s, _e = c.klt_track(p0, ext._klt_prm(), init=g)
        with pytest.raises(ValueError):
            ext.extend_tracks(sc["frames"][t + 1], copy.deepcopy(kps), max_bidir_error=np.inf, init=g[:-1])
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1] == outs[1][1] and outs[0][2].tobytes() == outs[1][2].tobytes()
    assert len(outs[0][0]) > 0
    h, w = sc["frames"][t].shape
    keep = ~np.isnan(p1).any(axis=1) & (p1[:, 0] >= 0) & (p1[:, 0] <= w) & (p1[:, 1] >= 0) & (p1[:, 1] <= h)
    assert np.array([k.uv.reshape(2) for k in tr]).tobytes() == p1[keep].tobytes()
