"""Randomised STATES through single stages of the device-resident pipeline against the table model (oracle/pipe_oracle.py, itself
pinned to the reference's loop over Python objects): lists with duplicates, landmark objects shared between several state entries and
dead entries, keypoint objects shared with the dead list, histories of every length up to beyond the 32-entry ring, empty lists, lists
that fill the tables exactly, tracks at and beyond the image border.  After each stage every list entry (row contents through the
indices, order, who shares what) must be equal; landmark positions / poses to 1e-9 where a solve ran."""
import copy

import numpy as np
import pytest

import pipe_helpers as ph

pytestmark = pytest.mark.gpu
W_IMG, H_IMG = 256, 160


def _z_turn_pose(t):
    H = np.eye(4)
    ang = 0.01 * t
    H[:2, :2] = [[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]]; H[:3, 3] = [0.1 * t, 0.02 * t, -0.05 * t]
    return H


def _random_state(rng, cap, t_step, n_l, n_c, n_d, share=0.3, long_hist=False, pose_fn=_z_turn_pose):
    """State + dead lists with object sharing like the reference produces (and a little worse); pose_fn(t) -> H 4 x 4 of trajectory entry t"""
    from vo_mi355x import Keypoint, Landmark, State, Trajectory

    def kp(t_first=None, border=False):
        L = int(rng.integers(1, 40 if long_hist else 9))
        t_first = t_step - L + 1 - int(rng.integers(0, 3)) if t_first is None else t_first
        hist = [np.float32(rng.uniform([4, 4], [W_IMG - 4, H_IMG - 4])).reshape(2, 1) for _ in range(L)]
        if border:
            hist[-1] = np.float32([[rng.choice([-3.0, 0.0, W_IMG, W_IMG + 2.5, 17.25])], [rng.choice([-1.0, 0.0, H_IMG, H_IMG + 4.0, 33.5])]])
        return Keypoint(int(t_first), L, hist[0].copy(), hist[-1].copy(), np.zeros((1, 1)), hist)

    def lm(k):
        return Landmark(int(k.t_first + len(k.uv_history) - 1 + rng.integers(0, 2)), rng.normal(0, 3, (3, 1)) + np.array([[0], [0], [12.0]]), np.zeros((1, 1)))
    lms, kps = [], []
    for _ in range(n_l):
        k = kp(border=rng.random() < 0.15)
        if lms and rng.random() < share:                 # another entry of an existing landmark object
            lms.append(lms[int(rng.integers(0, len(lms)))]); kps.append(k)
        else:
            lms.append(lm(k)); kps.append(k)
    cands = [kp(t_first=t_step - int(rng.integers(0, 4)), border=rng.random() < 0.15) for _ in range(n_c)]
    for c in cands:
        c.t_total = len(c.uv_history)
    dead, dead_kp = [], []
    for _ in range(n_d):
        r = rng.random()
        if lms and r < share:                            # shares landmark AND keypoint object with a state entry (just resurrected)
            j = int(rng.integers(0, len(lms))); dead.append(lms[j]); dead_kp.append(kps[j])
        elif lms and r < 2 * share:                      # shares only the landmark object (resurrected earlier, survived since)
            j = int(rng.integers(0, len(lms))); dead.append(lms[j]); dead_kp.append(kp())
        else:
            k = kp(); dead.append(lm(k)); dead_kp.append(k)
    traj = Trajectory({})
    for t in range(t_step + 1):
        traj.append(t, pose_fn(t))
    return State(lms, kps, cands, traj), dead, dead_kp


def _same(model, rp, what, p_tol=1e-9):
    e = rp.entries()
    m = dict(cand=[model.entry(None, k) for k in model.cand], lm=[model.entry(l, k) for l, k in zip(model.lm_L, model.lm_K)],
             dead=[model.entry(l, k) for l, k in zip(model.dead_L, model.dead_K)])
    assert e["status"] == model.status, (what, e["status"], model.status)
    assert e["n_dead_total"] == len(model.dead_L) + model.n_dead_inert, what
    for name in ("cand", "lm", "dead"):
        assert len(e[name]) == len(m[name]), (what, name, len(e[name]), len(m[name]))
        for i, (x, y) in enumerate(zip(e[name], m[name])):
            assert x[0] == y[0] and x[2:4] == y[2:4] and x[6] == y[6], (what, name, i, x[:4], y[:4])
            assert np.array_equal(x[4], y[4]) and np.array_equal(x[5], y[5]) and np.array_equal(x[7], y[7], equal_nan=True), (what, name, i)
            if y[1] is not None:
                assert np.abs(x[1] - y[1]).max() <= p_tol * max(1.0, np.abs(y[1]).max()), (what, name, i, x[1], y[1])
    # sharing structure: entries that refer to one row in the model refer to one row on the device (rows are numbered differently)
    def classes(ids):
        seen = {}
        return [seen.setdefault(int(v), len(seen)) for v in ids]
    r = e["rows"]
    assert classes(list(r["lm_l"]) + list(r["dead_l"])) == classes(model.lm_L + model.dead_L), what          # landmark rows
    assert classes(list(r["lm_k"]) + list(r["dead_k"])) == classes(model.lm_K + model.dead_K), what          # keypoint rows


@pytest.mark.parametrize("cap", [64, 1024, 1100, 2500, 5000, 8192])      # 1 / 2 / 4 / 8 entries per thread (above 4 096: row words in global scratch)
def test_random_states_stage_by_stage(cap):
    import pipe_oracle as po
    from vo_mi355x import VoContext
    from vo_mi355x.resident import ResidentPipeline, TRACK, TRIANGULATE, ADJUST, DETECT
    rng = np.random.default_rng(1000 + cap)
    sc = ph.scene(3, w=W_IMG, h=H_IMG, f=260.0, seed=5, pose_fn=lambda t: ph.sway_pose(t, period=24.0))
    ca, cb = VoContext(W_IMG, H_IMG, max_pts=cap), VoContext(W_IMG, H_IMG, max_pts=cap)
    for trial in range(14 if cap <= 64 else 6 if cap < 2000 else 3 if cap < 4096 else 2):
        full = trial % 3 == 2
        n_l = int(rng.integers(0, cap // 2)) if not full else cap // 2
        n_c = int(rng.integers(0, cap // 3)) if not full else cap - n_l          # the lists fill the table exactly
        n_d = int(rng.integers(0, cap // 2)) if trial % 4 else 0
        W = int(rng.choice([4, 10, 20]))
        t_step = int(rng.integers(6, 30))
        state, dead, dead_kp = _random_state(rng, cap, t_step, n_l, n_c, n_d, long_hist=trial % 2 == 1)
        for stage, name in ((TRACK, "track"), (ADJUST, "adjust"), (DETECT, "detect"), (TRIANGULATE, "triangulate")):
            model = po.PipeModel(ca, sc["K"], W_IMG, H_IMG, cap=cap, params=po.Params(ba_window=W, ba_max_iters=6))
            model.seed(copy.deepcopy(state), copy.deepcopy(dead), copy.deepcopy(dead_kp), t_step)
            # (deepcopy of the three lists one by one would break the sharing between them: copy them as ONE structure)
            st2, d2, dk2 = copy.deepcopy((state, dead, dead_kp))
            model = po.PipeModel(ca, sc["K"], W_IMG, H_IMG, cap=cap, params=po.Params(ba_window=W, ba_max_iters=6))
            model.seed(st2, d2, dk2, t_step)
            rp = ResidentPipeline(cb, sc["K"], ba_window=W, ba_max_iters=6)
            st3, d3, dk3 = copy.deepcopy((state, dead, dead_kp))
            rp.seed(st3, d3, dk3, t_step=t_step)
            what = "cap %d trial %d %s (n_l %d n_c %d n_d %d W %d)" % (cap, trial, name, n_l, n_c, n_d, W)
            _same(model, rp, what + " seed")
            if stage == TRACK:
                for c, mdl in ((ca, None), (cb, None)):
                    c.push_frame(sc["frames"][0])
                model.track(sc["frames"][1])
                cb.push_frame(sc["frames"][1]); rp.step(-1, TRACK)
            elif stage == ADJUST:
                model.adjust()
                rp.step(-1, ADJUST)
            elif stage == DETECT:
                ca.push_frame(sc["frames"][2]); cb.push_frame(sc["frames"][2])
                model.detect()
                rp.step(-1, DETECT)
            else:
                model.triangulate()
                rp.step(-1, TRIANGULATE)
            rec = rp.fetch()
            if stage == ADJUST and model.status == 0:
                _same(model, rp, what, p_tol=1e-6)       # a 6-iteration LM on random geometry: positions agree as far as the solve is conditioned
                assert rec["n_resurrected"] == model.info["n_resurrected"], what
            else:
                _same(model, rp, what)
            assert rec["overflow"] == model.info.get("overflow", 0), (what, rec["overflow"], model.info)
    ca.close(); cb.close()


# ---- the closed loop's own log and exp (pipe_log_so3 / pipe_rodrigues, csrc/vo_pipeline.hip) at their edges -------------------------------
def _edge_pose(t):
    """trajectory entry t: the rotation exp(r_t), r_t = so3_model.PIPE_ANGLES[t % 7] about an axis of its own with every component >= 0.3 in
    magnitude (the host's SVD projection cannot flip one of the sign tests of the near-pi branch).  so3.rodrigues_vec_to_mat is within
    so3_model.SO3_EXP_DEV of the 60-digit exp entry by entry (tests/test_so3_model.py)"""
    import so3_model as sm
    from vo_mi355x import so3
    k = t % len(sm.PIPE_ANGLES)
    H = np.eye(4)
    H[:3, :3] = so3.rodrigues_vec_to_mat(sm.PIPE_ANGLES[k] * sm.AXES[k])
    H[:3, 3] = np.array([0.1 * t, 0.02 * t, 12.0 - 0.05 * t]) - H[:3, :3] @ [0.0, 0.0, 12.0]      # the landmark cloud N((0, 0, 12), 3^2) stays in front
    return H


def _reproject_histories(rng, K, state, dead, dead_kp, t_step, pose_fn):
    """every history entry of every (landmark, keypoint) pair becomes the landmark's projection by the pose of its frame + 0.5 px (float32): the
    window problem has a minimum, so that the solve carries the ~1e-12 by which two correct logs differ near th = pi - 1e-4 to the positions
    as ~1e-12 and not, as six LM iterations on _random_state's unrelated points and tracks do, as 1e-3 (measured with oracle/ba_oracle.py)"""
    for L, k in list(zip(state._landmarks, state._landmarks_kp)) + list(zip(dead, dead_kp)):
        n = len(k.uv_history)
        for idx in range(n):
            t = L.t_latest - (n - 1) + idx                       # the frame PipeModel.ba_problem reads this entry for
            if 0 <= t <= t_step:
                q = K @ (pose_fn(t)[:3] @ np.append(np.asarray(L.p, np.float64).reshape(3), 1.0))
                k.uv_history[idx] = np.float32(q[:2] / q[2] + rng.normal(0.0, 0.5, 2)).reshape(2, 1)
        k.uv, k.uv_first = k.uv_history[-1].copy(), k.uv_history[0].copy()


def _angle_between(Ra, Rb):
    D = Ra @ Rb.T
    return 0.5 * np.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2) if np.trace(D) > 0 else np.pi


@pytest.mark.parametrize("cap,W", [(64, 4), (64, 10), (1100, 4), (1100, 10)])
def test_adjust_stage_with_edge_rotations(cap, W):
    """The ADJUST stage alone on windows whose poses are rotations by 1e-6 and 1e-4 (either side of the snap to zero, sin th < 1e-5), 0.3, 2.5,
    pi - 1e-4 and pi - 1e-6 (either side of the near-pi branch: axis from the diagonal, signs from the first row), pi + 0.2 -- every other
    pipeline test turns by <= 0.3 rad about one axis.  t_step = 13 puts all seven into a window of 10; windows of 4 see them in two states
    (t_step 10: the first four, t_step 13: the last four).
    (1) against PipeModel.adjust through _same: lists equal, positions and the window's poses to 1e-6, the poses outside the window equal;
    (2) with an LM budget of 0 the stage writes exp(log(R)) of every window pose back: against R itself, as a rotation angle, 8 x what the host
        twin so3.rodrigues_mat_to_vec achieves against the exact log (so3_model.SO3_LOG_DEV) outside the snap zones, OpenCV's 2e-5 rad inside
        them; translations equal."""
    import pipe_oracle as po
    import so3_model as sm
    from vo_mi355x import VoContext
    from vo_mi355x.resident import ResidentPipeline, ADJUST
    rng = np.random.default_rng(7000 + cap + W)
    sc = {"K": np.array([[260.0, 0, (W_IMG - 1) / 2], [0, 260.0, (H_IMG - 1) / 2], [0, 0, 1]])}      # (the other test's camera; no frames: ADJUST reads none)
    ca, cb = VoContext(W_IMG, H_IMG, max_pts=cap), VoContext(W_IMG, H_IMG, max_pts=cap)
    try:
        for t_step in ((10, 13) if W == 4 else (13,)):
            n_l, n_c, n_d = int(rng.integers(cap // 4, cap // 2)), int(rng.integers(0, cap // 3)), int(rng.integers(0, cap // 2))
            state, dead, dead_kp = _random_state(rng, cap, t_step, n_l, n_c, n_d, pose_fn=_edge_pose)
            _reproject_histories(rng, sc["K"], state, dead, dead_kp, t_step, _edge_pose)
            what = "cap %d W %d t_step %d edge rotations" % (cap, W, t_step)
            # (1) six LM iterations against the table model
            st2, d2, dk2 = copy.deepcopy((state, dead, dead_kp))
            model = po.PipeModel(ca, sc["K"], W_IMG, H_IMG, cap=cap, params=po.Params(ba_window=W, ba_max_iters=6))
            model.seed(st2, d2, dk2, t_step)
            rp = ResidentPipeline(cb, sc["K"], ba_window=W, ba_max_iters=6)
            st3, d3, dk3 = copy.deepcopy((state, dead, dead_kp))
            rp.seed(st3, d3, dk3, t_step=t_step)
            model.adjust()
            rp.step(-1, ADJUST)
            rec = rp.fetch()
            assert model.status == 0 and rec["ba_iters"] >= 1, (what, model.status, rec)
            _same(model, rp, what, p_tol=1e-6)
            assert rec["n_resurrected"] == model.info["n_resurrected"] and rec["overflow"] == model.info.get("overflow", 0), what
            got = rp.entries()["poses"]
            for t in range(t_step + 1):
                d = np.abs(got[t] - model.poses[t]).max()
                assert d <= (1e-6 * max(1.0, np.abs(model.poses[t]).max()) if t > t_step - W else 0.0), (what, t, d)
            # (2) budget 0: the window's poses go through the device's log and exp and nothing else
            rp = ResidentPipeline(cb, sc["K"], ba_window=W, ba_max_iters=6, ba_budget=0)
            st4, d4, dk4 = copy.deepcopy((state, dead, dead_kp))
            rp.seed(st4, d4, dk4, t_step=t_step)
            rp.step(-1, ADJUST)
            rec = rp.fetch()
            assert rec["status"] == 0 and rec["ba_iters"] == 0, (what, rec)
            got = rp.entries()["poses"]
            for t in range(t_step + 1):
                H, th = _edge_pose(t), sm.PIPE_ANGLES[t % len(sm.PIPE_ANGLES)]
                if t <= t_step - W:
                    assert np.array_equal(got[t], H), (what, t)
                    continue
                ang = _angle_between(got[t][:3, :3], H[:3, :3])
                tol = 2e-5 if abs(np.sin(th)) < 1e-5 else 8 * sm.SO3_LOG_DEV[th]
                print("%s t %d th %.9g: exp(log(R)) is %.2e rad from R (tolerance %.2e)" % (what, t, th, ang, tol))
                assert ang <= tol, (what, t, th, ang, tol)
                assert np.array_equal(got[t][:3, 3], H[:3, 3]) and np.array_equal(got[t][3], [0, 0, 0, 1]), (what, t)
                assert np.abs(got[t][:3, :3] @ got[t][:3, :3].T - np.eye(3)).max() <= 8 * sm.EPS, (what, t)
    finally:
        ca.close(); cb.close()
