"""GPU: the forward-backward KLT check (csrc/vo_klt_fb.hip, vo_klt_track_fb / vo_set_fb_check / vo_fb_read) through every layer.

The contract is the reference's extend_tracks / extend_landmarks check (extractor.py:44-47,65-68) with the image order of its second call fixed
as in the OpenCV sample it copies (notebooks/tracking.py:39-42):
    p1 = LK(prev, cur, p0);  p0r = LK(cur, prev, p1);  fb_err = max(|p0 - p0r|) over x, y (float32);  good = fb_err < max_err
Both passes are pinned bit for bit against the CPU oracle's KLT; the keep rules of the track table, the closed loop and the drop-in Extractor
against numpy / list restatements of the same rule."""
import copy

import numpy as np
import pytest

import pipe_helpers as ph
from tracks_model import fb_np as _fb_np, occlude as _occlude, oracle_fb as _oracle_fb      # (shared with tests/test_gpu_tracks_chunks.py)

pytestmark = pytest.mark.gpu


def _check_pair(c, im0, im1, p0, max_err, **kw):
    p1, st, err, it = c.klt_track(p0, return_iters=True)
    f1, fst, ferr, p0r, fbe, fit = c.klt_track_fb(p0, return_iters=True)
    # the forward pass is bit for bit the plain tracker's
    assert np.array_equal(f1, p1) and np.array_equal(fst, st) and np.array_equal(ferr, err) and np.array_equal(fit, it)
    q1, qs, qe, r0 = _oracle_fb(im0, im1, p0, **kw)
    assert np.array_equal(p1, q1) and np.array_equal(st, qs)
    assert np.array_equal(p0r, r0, equal_nan=True)
    e, ok = _fb_np(p0, r0, max_err)
    assert np.array_equal(fbe, e, equal_nan=True)
    got_ok, got_e = c.fb_read(len(p0))
    assert np.array_equal(got_ok, ok) and np.array_equal(got_e, e, equal_nan=True)
    return ok, e


def test_fb_pass_is_the_oracle_at_kitti_size(seq3):
    from vo_mi355x import VoContext, synthetic as syn
    frames, _ = seq3
    h, w = frames.shape[1:]
    p0 = syn.grid_points(2000, w, h, seed=21)
    with VoContext(w, h, max_pts=2048) as c:
        c.push_frame(frames[0]); c.push_frame(frames[1])
        assert c.get_fb_check() == np.inf
        c.set_fb_check(0.5)
        assert c.get_fb_check() == np.float32(0.5)
        ok, e = _check_pair(c, frames[0], frames[1], p0, 0.5)
        assert ok.sum() > 1000 and np.isfinite(e).all()
        # edge cases of test_klt_edge_cases: points outside / on the border, n = 0, n = 1
        pe = np.array([[0, 0], [w - 1, h - 1], [-40.0, 10.0], [w + 50.0, h + 50.0], [5.5, 370.25], [1240.9, 0.1],
                       [-15.0, -15.0], [620.123, 188.456], [w * 4.0, 10.0], [3.0, h - 0.01]], np.float32)
        _check_pair(c, frames[0], frames[1], pe, 0.5)
        z = c.klt_track_fb(np.zeros((0, 2), np.float32))
        assert z[0].shape == (0, 2) and z[3].shape == (0, 2) and z[4].shape == (0,)
        _check_pair(c, frames[0], frames[1], pe[7:8], 0.5)


def test_fb_pass_truncated_pyramid(seq_small):
    from vo_mi355x import VoContext, synthetic as syn
    frames, _ = seq_small
    with VoContext(320, 240, max_pts=512) as c:
        c.push_frame(frames[0]); c.push_frame(frames[2])
        c.set_fb_check(1.0)
        _check_pair(c, frames[0], frames[2], syn.grid_points(400, 320, 240, margin=8, seed=3), 1.0)


def test_fb_pass_batched_different_frames():
    from vo_mi355x import VoContext, synthetic as syn
    import vo_oracle as o
    B, w, h, n = 8, 320, 240, 300
    seqs = [syn.make_sequence(2, w=w, h=h, seed=100 + b, margin=64)[0] for b in range(B)]
    p0 = np.stack([syn.grid_points(n, w, h, margin=8, seed=40 + b) for b in range(B)])
    with VoContext(w, h, max_pts=512, batch=B) as c:
        c.push_frame(np.stack([s[0] for s in seqs])); c.push_frame(np.stack([s[1] for s in seqs]))
        c.set_fb_check(0.25)
        p1, st, err = c.klt_track(p0)
        f1, fst, ferr, p0r, fbe = c.klt_track_fb(p0)
        assert np.array_equal(f1, p1) and np.array_equal(fst, st) and np.array_equal(ferr, err)
        ok_d, e_d = c.fb_read(n)
        for b in range(B):
            q1, _, _, r0 = _oracle_fb(seqs[b][0], seqs[b][1], p0[b])
            assert np.array_equal(p1[b], q1) and np.array_equal(p0r[b], r0, equal_nan=True), b
            e, ok = _fb_np(p0[b], r0, 0.25)
            assert np.array_equal(fbe[b], e, equal_nan=True) and np.array_equal(ok_d[b], ok) and np.array_equal(e_d[b], e, equal_nan=True), b


def test_fb_check_rejects_an_occluder():
    """a block of unrelated texture appears in the second frame: the points under it are dragged somewhere and do not come back"""
    from vo_mi355x import VoContext, synthetic as syn
    w, h = 320, 240
    frames, _ = syn.make_sequence(2, w=w, h=h, seed=77, margin=64)
    x0, y0, size = 120, 80, 64
    im1 = _occlude(frames[1], x0, y0, size, seed=5)
    p0 = syn.grid_points(600, w, h, margin=8, seed=9)
    with VoContext(w, h, max_pts=1024) as c:
        c.push_frame(frames[0]); c.push_frame(im1)
        c.set_fb_check(1.0)
        ok, e = _check_pair(c, frames[0], im1, p0, 1.0)
        rej = ~ok
        assert rej.sum() > 0
        near = (p0[:, 0] >= x0 - 16) & (p0[:, 0] < x0 + size + 16) & (p0[:, 1] >= y0 - 16) & (p0[:, 1] < y0 + size + 16)
        assert (rej & near).sum() > rej.sum() / 2, (rej.sum(), (rej & near).sum())
        p1 = c.klt_track(p0)[0]
        inside = (p1[:, 0] >= 0) & (p1[:, 0] <= w) & (p1[:, 1] >= 0) & (p1[:, 1] <= h)
        assert (rej & inside).any()                       # the in-image test alone would have kept it
        c.set_fb_check(np.inf)
        c.klt_track_fb(p0)
        assert c.fb_read(len(p0))[0].all()                # a threshold of inf rejects nothing


def test_fb_check_nan_threshold_and_read_states():
    from vo_mi355x import VoContext, VoError
    with VoContext(64, 64, max_pts=64) as c:
        with pytest.raises(VoError) as ei:
            c.set_fb_check(np.nan)
        assert ei.value.code == -1
        assert c.get_fb_check() == np.inf
        with pytest.raises(VoError) as ei:
            c.fb_read(1)                                  # no track has run with the check
        assert ei.value.code == -4


def test_tracks_table_with_the_check_equals_list_model():
    """vo_tracks_track with a finite threshold over 7 frames (an occluder appears at frame 3 and stays): keep = inside AND good, in list order,
    with t_total, history and dead tags, against a numpy / list restatement on the CPU oracle's KLT"""
    import vo_oracle as o
    from vo_mi355x import VoContext, synthetic as syn
    w, h, T, thr = 240, 180, 7, 0.75
    frames, _ = syn.make_sequence(T, w=w, h=h, seed=31, margin=64)
    frames = np.stack([f if t < 3 else _occlude(f, 90, 60, 48, seed=11) for t, f in enumerate(frames)])
    seeds = syn.grid_points(200, w, h, seed=4, margin=10)
    tr = [dict(uv=p.copy(), first=p.copy(), tf=0, tt=1, tag=i, hist={0: p.copy()}) for i, p in enumerate(seeds)]
    with VoContext(w, h, max_pts=256) as c:
        c.set_fb_check(thr)
        c.push_frame(frames[0])
        c.tracks_seed(seeds, t=0)
        n_fb_dead = 0
        for t in range(1, T):
            c.push_frame(frames[t])
            c.tracks_track(t)
            p0 = np.array([k["uv"] for k in tr], np.float32).reshape(-1, 2)
            q1, _, _, r0 = _oracle_fb(frames[t - 1], frames[t], p0)
            _, good = _fb_np(p0, r0, thr)
            keep, dead = [], []
            for k, (x, y), g in zip(tr, q1, good):
                if 0 <= x <= w and 0 <= y <= h and g:
                    k["uv"] = np.array([x, y], np.float32); k["tt"] += 1; k["hist"][t] = k["uv"].copy(); keep.append(k)
                else:
                    dead.append(k["tag"])
                    n_fb_dead += int(0 <= x <= w and 0 <= y <= h)
            tr = keep
            ok_d, _ = c.fb_read(len(p0))
            assert np.array_equal(ok_d, good), t
            r = c.tracks_read()
            obs = c.tracks_obs(t, 8)
            assert np.array_equal(r["tag"], [k["tag"] for k in tr]), t
            assert np.array_equal(r["uv"], np.array([k["uv"] for k in tr]).reshape(-1, 2)), t
            assert np.array_equal(r["uv_first"], np.array([k["first"] for k in tr]).reshape(-1, 2)), t
            assert np.array_equal(r["t_total"], [k["tt"] for k in tr]) and np.array_equal(r["t_first"], [k["tf"] for k in tr]), t
            assert r["dead_tag"].tolist() == dead, t               # in list order
            for i, k in enumerate(tr):
                for s in range(8):
                    if t - s in k["hist"]:
                        assert np.array_equal(obs[s, i], k["hist"][t - s].astype(np.float64)), (t, i, s)
                    else:
                        assert np.isnan(obs[s, i]).all()
        assert n_fb_dead > 0                              # the check, not the border, killed some tracks


def _fb_model_class():
    import pipe_oracle as po
    import vo_oracle as o

    class FbModel(po.PipeModel):
        """oracle/pipe_oracle.py's table model with the forward-backward mask ANDed into `extend` (CPU oracle KLT for the backward pass)"""
        fb_max = np.inf
        prev_img = None

        def track_points(self, img):
            p0 = self.dense_points()
            p1 = super().track_points(img)
            self.fb_ok = np.ones(len(p0), bool)
            if len(p0) and self.fb_max != np.inf:
                p0r = o.klt(img, self.prev_img, p1)[0]
                self.fb_ok = _fb_np(p0, p0r, self.fb_max)[1]
            self.prev_img = img
            return p1

        def _inside(self, p):
            return super()._inside(p) & self.fb_ok

    return FbModel


def _occluded_scene(seed, t1, n, w, h):
    sc = ph.scene(t1 + n + 1, w=w, h=h, f=260.0, seed=seed, pose_fn=lambda t: ph.sway_pose(t, period=24.0))
    fr = sc["frames"].copy()
    for t in range(t1 + 3, len(fr)):                      # appears at t1 + 3, drifts right
        fr[t] = _occlude(fr[t], 60 + 4 * (t - t1), 50, 40, seed=t)
    sc["frames"] = fr
    return sc


@pytest.mark.parametrize("ba_window", [4, 10])
def test_closed_loop_with_the_check_equals_the_model(ba_window):
    """vo_pipe_step with fb_max_error = 1.0, a batch of 2 scenes, 10 frames: records and tables frame by frame = the table model with the
    check; vo_pipe_step_host gives the same bits; a context set back to inf = a context that never set it"""
    from vo_mi355x import VoContext
    from vo_mi355x.resident import ResidentPipeline
    FbModel = _fb_model_class()
    import pipe_oracle as po
    w, h, t1, n, B = 256, 160, 3, 10, 2
    scs = [_occluded_scene(sd, t1, n, w, h) for sd in (2024, 77)]
    boot = VoContext(w, h, max_pts=2048)
    states = [ph.gt_bootstrap(boot, sc, 0, t1)[0] for sc in scs]
    models = []
    for b in range(B):
        ca = VoContext(w, h, max_pts=2048)
        m = FbModel(ca, scs[b]["K"], w, h, cap=2048, params=po.Params(ba_window=ba_window, ba_max_iters=12))
        m.fb_max = 1.0
        m.seed(copy.deepcopy(states[b]), [], [], 1)
        ca.push_frame(scs[b]["frames"][t1]); m.prev_img = scs[b]["frames"][t1]
        models.append(m)
    Ks = np.stack([sc["K"] for sc in scs])
    frames = np.stack([sc["frames"] for sc in scs])

    def run(fb, host=False, set_inf_first=False):
        c = VoContext(w, h, max_pts=2048, batch=B)
        if set_inf_first:
            c.set_fb_check(3.0)
        kw = {} if fb is None else dict(fb_max_error=fb)
        rp = ResidentPipeline(c, Ks, ba_window=ba_window, ba_max_iters=12, pnp_blind_batches=8, **kw)
        rp.seed([copy.deepcopy(s) for s in states], None, None, 1)
        if not host:
            c.upload_sequence(frames)
            c.push_frame_resident(t1)
        else:
            c.push_frame(frames[:, t1])
        out = []
        for s in range(n):
            if host:
                rp.step_host([frames[b, t1 + 1 + s] for b in range(B)])
            else:
                rp.step(t1 + 1 + s)
            rec = rp.fetch()
            T = rp.read_tables()
            ents = [rp.entries(b, tables=T) for b in range(B)]
            out.append((rec, T, c.fb_read(int(max(r["n_tracked"] for r in rec))) if fb not in (None, np.inf) else None, ents))
        return out

    res = run(1.0)
    n_rej = 0
    for s in range(n):
        recs, T, (ok, _), ents = res[s]
        for b, m in enumerate(models):
            m.step(scs[b]["frames"][t1 + 1 + s])
            rec = recs[b]
            assert rec["status"] == 0 and m.status == 0, (s, b)
            n_rej += int((~m.fb_ok).sum())
            assert np.array_equal(ok[b][:len(m.fb_ok)], m.fb_ok), (s, b)
            assert rec["n_tracked"] == len(m.fb_ok)
            assert (rec["n_landmarks"], rec["n_candidates"], rec["n_dead_total"]) == \
                   (len(m.lm_L), len(m.cand), len(m.dead_L) + m.n_dead_inert), (s, b)
            assert np.abs(rec["H"] - m.poses[m.t]).max() <= 1e-7, (s, b)
            e = ents[b]
            for (l, k), x in zip(zip(m.lm_L, m.lm_K), e["lm"]):
                y = m.entry(l, k)
                assert x[0] == y[0] and x[2:4] == y[2:4] and np.array_equal(x[5], y[5]) and np.linalg.norm(x[1] - y[1]) <= 1e-7 * np.linalg.norm(y[1])
            for k, x in zip(m.cand, e["cand"]):
                y = m.entry(None, k)
                assert x[2:4] == y[2:4] and np.array_equal(x[4], y[4]) and np.array_equal(x[5], y[5]) and x[6] == y[6], (s, b)
    assert n_rej > 0

    # the host-frame form: the same bits
    hres = run(1.0, host=True)
    _same_runs(res, hres, n)
    # a setter at inf = a context that never set it
    _same_runs(run(None), run(np.inf, set_inf_first=True), n)


def _same_runs(a, b, n):
    for s in range(n):
        ra, Ta, fa, _ = a[s]
        rb, Tb, fb, _ = b[s]
        for x, y in zip(ra, rb):
            for k, v in x.items():
                assert (np.array_equal(y[k], v) if isinstance(v, np.ndarray) else y[k] == v), (s, k)
        for name in Ta:
            assert np.array_equal(Ta[name], Tb[name]), (s, name)
        if fa is not None:
            assert np.array_equal(fa[0], fb[0]) and np.array_equal(fa[1], fb[1], equal_nan=True), s


def test_fb_read_refuses_with_a_step_in_flight():
    from vo_mi355x import VoContext, VoError
    from vo_mi355x.resident import ResidentPipeline
    w, h, t1 = 256, 160, 3
    sc = ph.scene(t1 + 3, w=w, h=h, f=260.0, seed=2024, pose_fn=lambda t: ph.sway_pose(t, period=24.0))
    with VoContext(w, h, max_pts=1024) as c:
        state, _ = ph.gt_bootstrap(c, sc, 0, t1)
        rp = ResidentPipeline(c, sc["K"], ba_max_iters=12, fb_max_error=1.0)
        rp.seed(state, [], [], 1)
        c.push_frame(sc["frames"][t1])
        c.push_frame(sc["frames"][t1 + 1]); rp.step()
        with pytest.raises(VoError) as ei:
            c.fb_read(1)
        assert ei.value.code == -4
        rec = rp.fetch()
        ok, e = c.fb_read(rec["n_tracked"])
        assert ok.shape == (rec["n_tracked"],) and ok.dtype == bool


def test_dropin_extractor_backward_equals_fixed_reference():
    """the reference's call order (extend_tracks, then extend_landmarks on the same frame) over Extractor(bidir="backward") against a Python
    restatement of the reference's code with the second call's image order fixed, the CPU oracle's KLT for both passes"""
    import vo_oracle as o
    from vo_mi355x import synthetic as syn
    from vo_mi355x.extractor import Extractor
    from vo_mi355x.state import Keypoint, Landmark
    w, h, T, thr = 240, 180, 5, 1.0
    frames, _ = syn.make_sequence(T, w=w, h=h, seed=13, margin=64)
    frames = np.stack([f if t < 2 else _occlude(f, 100, 70, 48, seed=3) for t, f in enumerate(frames)])
    pts = syn.grid_points(160, w, h, seed=8, margin=10).astype(np.float64)

    def mk(lists):
        kp = [Keypoint(0, 1, p.reshape(2, 1).copy(), p.reshape(2, 1).copy(), None, [p.reshape(2, 1).copy()]) for p in pts[:100]]
        lk = [Keypoint(0, 1, p.reshape(2, 1).copy(), p.reshape(2, 1).copy(), None, [p.reshape(2, 1).copy()]) for p in pts[100:]]
        lm = [Landmark(0, np.array([[i], [0.0], [1.0]]), None) for i in range(len(lk))]
        return kp, lm, lk

    def ref_track(im_prev, im_curr, p0):
        p0 = np.asarray(p0, np.float32).reshape(-1, 2)
        p1 = o.klt(im_prev, im_curr, p0)[0]
        p0r = o.klt(im_curr, im_prev, p1)[0]
        good = np.abs(p0 - p0r).reshape(-1, 2).max(-1) < thr
        inside = (p1[:, 0] >= 0) & (p1[:, 0] <= w) & (p1[:, 1] >= 0) & (p1[:, 1] <= h)
        return p1, good & inside

    ex = Extractor(lazy=False, bidir="backward")
    kp_a, lm_a, lk_a = mk(None)
    kp_b, lm_b, lk_b = mk(None)
    dead_a, dead_b = [], []
    n_drop = 0
    for t in range(1, T):
        ex._im_prev = frames[t - 1]
        kp_a = ex.extend_tracks(frames[t], kp_a, max_bidir_error=thr)
        lm_a, lk_a, dl, dk = ex.extend_landmarks(frames[t], lm_a, lk_a, max_bidir_error=thr)
        dead_a += list(zip(dl, dk))
        # restatement (extractor.py:38-88 with LK(cur, prev, p1) as the second call)
        if kp_b:
            p1, keep = ref_track(frames[t - 1], frames[t], [k.uv for k in kp_b])
            out = []
            for i in np.nonzero(keep)[0]:
                k = kp_b[i]; k.uv = p1[i].reshape(2, 1); k.t_total += 1; k.uv_history.append(p1[i].reshape(2, 1)); out.append(k)
            n_drop += len(kp_b) - len(out)
            kp_b = out
        if lk_b:
            p1, keep = ref_track(frames[t - 1], frames[t], [k.uv for k in lk_b])
            nl, nk = [], []
            for i in range(len(lm_b)):
                l, k = lm_b[i], lk_b[i]
                if not keep[i]:
                    dead_b.append((l, k)); continue
                k.uv = np.float64(p1[i]).reshape(2, 1); k.t_total += 1; k.uv_history.append(np.float64(p1[i]).reshape(2, 1)); l.t_latest += 1
                nk.append(copy.deepcopy(k)); nl.append(l)
            lm_b, lk_b = nl, nk
        assert len(kp_a) == len(kp_b) and len(lk_a) == len(lk_b) and len(dead_a) == len(dead_b), t
        for a, b in zip(kp_a, kp_b):
            assert np.array_equal(np.float32(a.uv), np.float32(b.uv)) and a.t_total == b.t_total and len(a.uv_history) == len(b.uv_history)
        for a, b in zip(lk_a, lk_b):
            assert np.array_equal(a.uv, b.uv) and a.t_total == b.t_total
        for (la, ka), (lb, kb) in zip(dead_a, dead_b):
            assert np.array_equal(la.p, lb.p) and np.array_equal(ka.uv, kb.uv) and ka.t_total == kb.t_total
        assert [l.t_latest for l in lm_a] == [l.t_latest for l in lm_b]
    assert n_drop > 0 and len(dead_b) > 0
