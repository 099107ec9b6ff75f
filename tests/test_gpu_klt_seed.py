"""GPU: motion-predicted initial flow of the KLT tracker (csrc/vo_klt_seed.hip; vo_klt_track_init / vo_klt_track_fb_init /
vo_set_klt_predict / vo_klt_guess_read) through every layer.

The contract is OpenCV's OPTFLOW_USE_INITIAL_FLOW: the top pyramid level starts at the caller's guess, everything else is the unseeded
tracker; a guess that is not finite starts from p0.  The seeded kernels are pinned bit for bit against the numpy model
tests/klt_seed_model.py (itself pinned against the C oracle by tests/test_klt_seed_model.py); the predictors of the track table and the
closed loop against the numpy rule g = uv + (uv - prev); the keep rules against the synchronous seeded calls."""
import copy

import numpy as np
import pytest

import klt_seed_model as km
import pipe_helpers as ph

pytestmark = pytest.mark.gpu

CV = "constant_velocity"


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want, what=""):
    """(p1, status, err, iters) bit for bit"""
    assert np.array_equal(_bits(got[0]), _bits(want[0])), what
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(_bits(got[2]), _bits(want[2])), what
    assert np.array_equal(got[3], want[3]), what


def _border_points(w, h, n, seed):
    """points inside, on and beyond the border (tests/test_oracle_crosscheck.py)"""
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-20, w + 20, n), rng.uniform(-20, h + 20, n)], 1)
    p[: n // 2] = np.stack([rng.uniform(20, w - 20, n // 2), rng.uniform(20, h - 20, n // 2)], 1)
    p[n // 2] = (0.0, 0.0); p[n // 2 + 1] = (w - 1.0, h - 1.0); p[n // 2 + 2] = (w - 0.5, 3.25)
    return p.astype(np.float32)


def _hostile_guesses(p, w, h, seed):
    """far outside the image, on the border, NaN / inf components, and some honest ones in between"""
    rng = np.random.default_rng(seed)
    g = (p + rng.uniform(-3, 3, p.shape)).astype(np.float32)
    g[0] = (-500.0, 1.0e4); g[1] = (1.0e30, -1.0e30); g[2] = (w * 4.0, h * 0.5); g[3] = (-31.5, -31.5)
    g[4] = (0.0, 0.0); g[5] = (w - 1.0, h - 1.0); g[6] = (w, h); g[7] = (w - 0.5, 0.25)
    g[8] = (np.nan, 5.0); g[9] = (5.0, np.nan); g[10] = (np.inf, 5.0); g[11] = (5.0, -np.inf); g[12] = (np.nan, np.nan)
    return g


# ---- 1. the synchronous call = the model ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["320x240", "1241x376"])
def test_seeded_track_is_the_model(size, seq3, seq_small):
    from vo_mi355x import VoContext
    if size == "320x240":
        frames, (w, h, n) = seq_small[0], (320, 240, 120)              # the pyramid truncates at level 2
    else:
        frames, (w, h, n) = seq3[0], (1241, 376, 160)
    p0 = _border_points(w, h, n, 3)
    with VoContext(w, h, max_pts=256) as c:
        c.push_frame(frames[0]); c.push_frame(frames[1])
        plain = c.klt_track(p0, return_iters=True)
        _same(c.klt_track(p0, return_iters=True, init=None), plain, "init=None")
        _same(plain, km.klt_np(frames[0], frames[1], p0), "unseeded model")
        # g = p0: the unseeded tracker, bit for bit
        _same(c.klt_track(p0, return_iters=True, init=p0), plain, "g = p0")
        # hostile guesses
        g = _hostile_guesses(p0, w, h, 5)
        _same(c.klt_track(p0, return_iters=True, init=g), km.klt_np(frames[0], frames[1], p0, init=g), "hostile")
        # n = 0, n = 1
        z = c.klt_track(np.zeros((0, 2), np.float32), init=np.zeros((0, 2), np.float32))
        assert z[0].shape == (0, 2) and z[1].shape == (0,)
        _same(c.klt_track(p0[7:8], return_iters=True, init=g[7:8]), km.klt_np(frames[0], frames[1], p0[7:8], init=g[7:8]), "n = 1")
        # constant-velocity guesses from a previous track: frames 1 -> 2 from the result of 0 -> 1
        q0 = p0[: n // 2]                                              # (the inside half)
        q1 = c.klt_track(q0)[0]
        gv = km.predict(q1, q0)
        c.push_frame(frames[2])
        want = km.klt_np(frames[1], frames[2], q1, init=gv)
        got = c.klt_track(q1, return_iters=True, init=gv)
        _same(got, want, "constant velocity")
        unseeded = c.klt_track(q1, return_iters=True)
        print("%s: summed iterations %d unseeded, %d seeded" % (size, np.maximum(unseeded[3], 0).sum(), np.maximum(got[3], 0).sum()))


# ---- 2. a batch: different frames and guesses per sequence ---------------------------------------------------------------------------------
def test_seeded_track_batched_different_frames_and_guesses():
    from vo_mi355x import VoContext, synthetic as syn
    B, w, h, n = 8, 320, 240, 60
    seqs = [syn.make_sequence(2, w=w, h=h, seed=100 + b, margin=64)[0] for b in range(B)]
    p0 = np.stack([_border_points(w, h, n, 40 + b) for b in range(B)])
    g = np.stack([_hostile_guesses(p0[b], w, h, 60 + b) if b % 2 else (p0[b] + np.float32(1.5 * (b - 3))) for b in range(B)]).astype(np.float32)
    with VoContext(w, h, max_pts=64, batch=B) as c:                   # batch % 8 == 0: the XCD remap is on
        c.push_frame(np.stack([s[0] for s in seqs])); c.push_frame(np.stack([s[1] for s in seqs]))
        got = c.klt_track(p0, return_iters=True, init=g)
        for b in range(B):
            _same([x[b] for x in got], km.klt_np(seqs[b][0], seqs[b][1], p0[b], init=g[b]), b)


# ---- 3. the forward-backward form ----------------------------------------------------------------------------------------------------------
def test_seeded_forward_backward(seq_small):
    import vo_oracle as o
    from vo_mi355x import VoContext
    frames, (w, h, n) = seq_small[0], (320, 240, 120)
    p0 = _border_points(w, h, n, 9)
    g = _hostile_guesses(p0, w, h, 10)
    with VoContext(w, h, max_pts=128) as c:
        c.push_frame(frames[0]); c.push_frame(frames[2])
        c.set_fb_check(0.5)
        fwd = c.klt_track(p0, return_iters=True, init=g)
        f1, fst, ferr, p0r, fbe, fit = c.klt_track_fb(p0, return_iters=True, init=g)
        _same((f1, fst, ferr, fit), fwd, "forward pass")
        assert np.array_equal(p0r, o.klt(frames[2], frames[0], f1)[0], equal_nan=True)         # the backward pass is unseeded
        e = np.abs(p0 - p0r).max(-1)
        assert np.array_equal(fbe, e, equal_nan=True)
        ok, e_d = c.fb_read(n)
        assert np.array_equal(ok, e < np.float32(0.5)) and np.array_equal(e_d, e, equal_nan=True)
        # init=None: the unseeded call
        a, b = c.klt_track_fb(p0, return_iters=True, init=None), c.klt_track_fb(p0, return_iters=True)
        assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))
        z = c.klt_track_fb(np.zeros((0, 2), np.float32), init=np.zeros((0, 2), np.float32))
        assert z[0].shape == (0, 2) and z[3].shape == (0, 2)


# ---- 4. the track table --------------------------------------------------------------------------------------------------------------------
def _level_means(it):
    """mean iterations per pyramid level over the points that ran the level"""
    return [float(it[:, l][it[:, l] >= 0].mean()) if (it[:, l] >= 0).any() else float("nan") for l in range(it.shape[1])]


def test_track_table_predicts_from_its_ring():
    """batch 2 whose counts differ, frames 1..4 with re-detection in the loop (compaction, one-entry histories): at every step the guesses
    are the numpy rule on the two previous read-backs, and the table is klt_track(init=g) plus the keep rule; frame 1 (no history anywhere)
    is bit-identical to a context with prediction off"""
    from vo_mi355x import VoContext, synthetic as syn
    B, w, h, T, n0 = 2, 320, 240, 5, 90
    seqs = [syn.make_sequence(T, w=w, h=h, seed=77 + 5 * b, margin=64)[0] for b in range(B)]
    frames = np.stack(seqs)                                            # [B, T, h, w]
    seeds = np.stack([syn.grid_points(n0, w, h, margin=10, seed=4 + b) for b in range(B)])
    seeds[1, :12] = (-200.0, -200.0)                                   # sequence 1 loses twelve tracks at once: the counts differ from frame 1 on
    prm = dict(max_new=25)
    with VoContext(w, h, max_pts=256, batch=B) as c, VoContext(w, h, max_pts=256, batch=B) as sync, VoContext(w, h, max_pts=256, batch=B) as off:
        c.set_klt_predict(CV)
        assert c.get_klt_predict() == CV and off.get_klt_predict() == "off"
        for x in (c, sync, off):
            x.push_frame(frames[:, 0])
        c.tracks_seed(seeds, t=0); off.tracks_seed(seeds, t=0)
        before = c.tracks_read()                                       # the table after frame t - 1
        older = [dict(uv=np.zeros((0, 2), np.float32), tag=np.zeros(0, np.int32)) for _ in range(B)]      # ... and after frame t - 2
        it_on, it_off, counts_differed = [], [], False
        for t in range(1, T):
            for x in (c, sync, off):
                x.push_frame(frames[:, t])
            nb = [len(r["uv"]) for r in before]
            n_hi = max(nb)
            c.tracks_track(t); off.tracks_track(t)
            g = c.klt_guess_read(n_hi)
            p0 = np.zeros((B, n_hi, 2), np.float32)
            want_g = np.full((B, n_hi, 2), np.nan, np.float32)
            for b in range(B):
                p0[b, :nb[b]] = before[b]["uv"]
                prev = np.full((nb[b], 2), np.nan, np.float32)
                where = {int(tag): i for i, tag in enumerate(older[b]["tag"])}
                for i, tag in enumerate(before[b]["tag"]):
                    if int(tag) in where:
                        prev[i] = older[b]["uv"][where[int(tag)]]
                want_g[b, :nb[b]] = km.predict(before[b]["uv"], prev)
                if t >= 2:
                    assert np.isfinite(prev).all(-1).any() and np.isnan(prev).all(-1).any(), (t, b)      # old tracks and one-entry histories
            assert np.array_equal(_bits(g), _bits(want_g)), t          # (dead slots NaN, bit for bit)
            p1 = sync.klt_track(p0, init=np.where(np.isnan(want_g), p0, want_g))[0]
            it_on.append(np.concatenate([c.points_download(n_hi, return_iters=True)[3][b, :nb[b]] for b in range(B)]))
            it_off.append(np.concatenate([off.points_download(n_hi, return_iters=True)[3][b, :nb[b]] for b in range(B)]))
            after = c.tracks_read()
            for b in range(B):
                q = p1[b, :nb[b]]
                keep = (q[:, 0] >= 0) & (q[:, 0] <= w) & (q[:, 1] >= 0) & (q[:, 1] <= h)
                assert np.array_equal(after[b]["tag"], before[b]["tag"][keep]), (t, b)
                assert np.array_equal(_bits(after[b]["uv"]), _bits(q[keep])), (t, b)
            if t == 1:                                                 # no history anywhere: the unseeded tracker's bits
                for ra, rb in zip(after, off.tracks_read()):
                    assert all(np.array_equal(ra[k], rb[k]) for k in ra)
            else:
                off.tracks_read()                                      # (keeps both contexts' host-side bounds alike)
            c.tracks_detect(t, **prm); off.tracks_detect(t, **prm)
            older, before = before, c.tracks_read()
            off.tracks_read()
            counts_differed |= len(before[0]["uv"]) != len(before[1]["uv"])
        assert counts_differed
        print("track table, mean iterations per level (level 0 first), frames 2..%d: off %s  on %s" % (
            T - 1, _level_means(np.concatenate(it_off[1:])), _level_means(np.concatenate(it_on[1:]))))
        # an unpredicted track forgets the guesses
        c.set_klt_predict("off")
        c.push_frame(frames[:, 0]); c.tracks_track(T)
        from vo_mi355x import VoError
        with pytest.raises(VoError) as ei:
            c.klt_guess_read(1)
        assert ei.value.code == -4


# ---- 5. the closed loop --------------------------------------------------------------------------------------------------------------------
W, H, T1 = 256, 160, 3


@pytest.fixture(scope="module")
def loop_scene():
    from vo_mi355x import VoContext
    sc = ph.scene(T1 + 8, w=W, h=H, f=260.0, seed=2024, pose_fn=lambda t: ph.sway_pose(t, period=24.0))
    with VoContext(W, H, max_pts=1024) as boot:
        state, t1 = ph.gt_bootstrap(boot, sc, 0, T1)
    assert t1 == T1
    return sc, state


def _loop(c, sc, state, **kw):
    from vo_mi355x.resident import ResidentPipeline
    rp = ResidentPipeline(c, sc["K"], ba_max_iters=12, pnp_blind_batches=8, **kw)
    rp.seed(copy.deepcopy(state), [], [], 1)
    c.upload_sequence(sc["frames"])
    c.push_frame_resident(T1)
    return rp


def _dense(T, b=0):
    """the resident point set [landmarks | candidates] of the tables, its rows, and the rule's `prev` per entry"""
    from vo_mi355x.resident import HIST
    n_c, n_l = int(T["counts"][b, 0]), int(T["counts"][b, 1])
    rows = np.concatenate([T["lm_k"][b, :n_l], T["cand"][b, :n_c]])
    p0 = T["k_uv"][b, rows]
    ln = T["k_histlen"][b, rows]
    prev = np.full((len(rows), 2), np.nan, np.float32)
    has = ln >= 2
    prev[has] = T["k_hist"][b, (ln[has] - 2) % HIST, rows[has]]
    return p0, prev, n_l, n_c


@pytest.mark.parametrize("fb", [np.inf, 1.0])
def test_closed_loop_track_stage_predicts_from_the_history(loop_scene, fb):
    """one whole frame (so that histories of two entries, fresh candidates and resurrected entries all occur), then a TRACK-only step:
    guesses = the numpy rule on the tables read before it, K_UV after it = the synchronous seeded call plus the keep rule; with the
    forward-backward check on as well, the flags are the seeded forward-backward call's"""
    from vo_mi355x import VoContext
    from vo_mi355x.resident import TRACK
    sc, state = loop_scene
    with VoContext(W, H, max_pts=1024) as c, VoContext(W, H, max_pts=1024) as sync:
        rp = _loop(c, sc, state, klt_predict=CV, fb_max_error=fb)
        assert c.get_klt_predict() == CV
        rp.step(T1 + 1); assert rp.fetch()["status"] == 0
        T0 = rp.read_tables()
        p0, prev, n_l, n_c = _dense(T0)
        n = n_l + n_c
        assert (np.isfinite(prev).all(-1)).sum() > 50 and np.isnan(prev).all(-1).sum() > 0
        want_g = km.predict(p0, prev)
        rp.step(T1 + 2, stages=TRACK)
        rec = rp.fetch()
        assert rec["status"] == 0 and rec["n_tracked"] == n
        g = c.klt_guess_read(n + 1)
        assert np.array_equal(_bits(g[:n]), _bits(want_g)) and np.isnan(g[n]).all()
        sync.push_frame(sc["frames"][T1 + 1]); sync.push_frame(sc["frames"][T1 + 2])
        if fb == np.inf:
            p1 = sync.klt_track(p0, init=want_g)[0]
            good = np.ones(n, bool)
        else:
            sync.set_fb_check(fb)
            p1 = sync.klt_track_fb(p0, init=want_g)[0]
            good = sync.fb_read(n)[0]
            assert np.array_equal(c.fb_read(n)[0], good)
        keep = good & (p1[:, 0] >= 0) & (p1[:, 0] <= W) & (p1[:, 1] >= 0) & (p1[:, 1] <= H)
        T1_ = rp.read_tables()
        m_c, m_l = int(T1_["counts"][0, 0]), int(T1_["counts"][0, 1])
        assert (m_l, m_c) == (int(keep[:n_l].sum()), int(keep[n_l:].sum()))
        assert np.array_equal(_bits(T1_["k_uv"][0, T1_["lm_k"][0, :m_l]]), _bits(p1[:n_l][keep[:n_l]]))
        assert np.array_equal(T1_["cand"][0, :m_c], T0["cand"][0, :n_c][keep[n_l:]])
        assert np.array_equal(_bits(T1_["k_uv"][0, T1_["cand"][0, :m_c]]), _bits(p1[n_l:][keep[n_l:]]))


def test_closed_loop_with_prediction_is_the_same_on_every_stream_layout(loop_scene):
    """six frames of the whole loop with prediction on: status 0 throughout; records and final tables bit-identical with the side stream
    on and off, and with INFLIGHT steps in flight instead of one"""
    from vo_mi355x import VoContext
    from vo_mi355x.resident import INFLIGHT
    sc, state = loop_scene
    n = 6

    def run(side, inflight, predict=CV):
        with VoContext(W, H, max_pts=1024) as c:
            c.set_side_stream(side)
            rp = _loop(c, sc, state, klt_predict=predict)
            recs, its, pending = [], [], 0
            for s in range(n):
                rp.step(T1 + 1 + s); pending += 1
                if pending == inflight or s == n - 1:
                    while pending:
                        recs.append(rp.fetch()); pending -= 1
                        if inflight == 1:
                            k = recs[-1]["n_tracked"]
                            its.append(c.points_download(k, return_iters=True)[3])
            g = c.klt_guess_read(recs[-1]["n_tracked"]) if predict == CV else None
            return recs, rp.read_tables(), g, its

    ra, Ta, ga, its_on = run(True, 1)
    assert all(r["status"] == 0 for r in ra)
    assert np.isfinite(ga).all()
    for side, inflight in ((False, 1), (True, INFLIGHT)):
        rb, Tb, gb, _ = run(side, inflight)
        for s, (x, y) in enumerate(zip(ra, rb)):
            for k, v in x.items():
                assert (np.array_equal(y[k], v) if isinstance(v, np.ndarray) else y[k] == v), (side, inflight, s, k)
        for name in Ta:
            assert np.array_equal(Ta[name], Tb[name], equal_nan=Ta[name].dtype.kind == "f"), (side, inflight, name)
        assert np.array_equal(_bits(ga), _bits(gb))
    ro, _, _, its_off = run(True, 1, predict="off")
    assert all(r["status"] == 0 for r in ro)
    print("closed loop, mean iterations per level (level 0 first), frames 2..%d: off %s  on %s" % (
        n, _level_means(np.concatenate(its_off[1:])), _level_means(np.concatenate(its_on[1:]))))


# ---- 6. the drop-in Extractor ---------------------------------------------------------------------------------------------------------------
def test_dropin_extractor_constant_velocity_equals_list_restatement():
    """extend_tracks, then extend_landmarks on the same frame, over Extractor(predict="constant_velocity") on the object path against a
    Python restatement: g = uv + (uv - uv_history[-2]) in float32 (uv for a one-entry history), the numpy model's seeded KLT, the
    reference's keep rule"""
    from vo_mi355x import synthetic as syn
    from vo_mi355x.extractor import Extractor
    from vo_mi355x.state import Keypoint, Landmark
    w, h, T = 240, 180, 4
    frames, _ = syn.make_sequence(T, w=w, h=h, seed=13, margin=64)
    pts = syn.grid_points(110, w, h, seed=8, margin=6).astype(np.float64)

    def mk():
        kp = [Keypoint(0, 1, p.reshape(2, 1).copy(), p.reshape(2, 1).copy(), None, [p.reshape(2, 1).copy()]) for p in pts[:70]]
        lk = [Keypoint(0, 1, p.reshape(2, 1).copy(), p.reshape(2, 1).copy(), None, [p.reshape(2, 1).copy()]) for p in pts[70:]]
        lm = [Landmark(0, np.array([[i], [0.0], [1.0]]), None) for i in range(len(lk))]
        return kp, lm, lk

    def ref_track(im_prev, im_curr, kps):
        p0 = np.asarray([k.uv for k in kps], np.float64).reshape(-1, 2).astype(np.float32)
        g = p0.copy()
        for i, k in enumerate(kps):
            if len(k.uv_history) >= 2:
                g[i] = p0[i] + (p0[i] - np.float32(k.uv_history[-2]).reshape(2))
        p1 = km.klt_np(im_prev, im_curr, p0, init=g)[0]
        inside = (p1[:, 0] >= 0) & (p1[:, 0] <= w) & (p1[:, 1] >= 0) & (p1[:, 1] <= h)
        return p1, inside & ~np.isnan(p1).any(1)

    with pytest.raises(ValueError):
        Extractor(lazy=False, predict="linear")
    ex = Extractor(lazy=False, predict=CV)
    kp_a, lm_a, lk_a = mk()
    kp_b, lm_b, lk_b = mk()
    dead_a, dead_b = [], []
    for t in range(1, T):
        ex._im_prev = frames[t - 1]
        kp_a = ex.extend_tracks(frames[t], kp_a, max_bidir_error=np.inf)
        lm_a, lk_a, dl, dk = ex.extend_landmarks(frames[t], lm_a, lk_a, max_bidir_error=np.inf)
        dead_a += list(zip(dl, dk))
        p1, keep = ref_track(frames[t - 1], frames[t], kp_b)
        out = []
        for i in np.nonzero(keep)[0]:
            k = kp_b[i]; k.uv = p1[i].reshape(2, 1); k.t_total += 1; k.uv_history.append(p1[i].reshape(2, 1)); out.append(k)
        kp_b = out
        p1, keep = ref_track(frames[t - 1], frames[t], lk_b)
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
        assert [l.t_latest for l in lm_a] == [l.t_latest for l in lm_b]
    assert len(kp_b) > 30 and len(lk_b) > 15


# ---- 7. error codes ------------------------------------------------------------------------------------------------------------------------
def test_predict_modes_and_read_states(loop_scene):
    from vo_mi355x import VoContext, VoError
    with VoContext(64, 64, max_pts=64) as c:
        assert c.get_klt_predict() == "off"
        with pytest.raises(VoError) as ei:
            c.set_klt_predict(2)
        assert ei.value.code == -1
        with pytest.raises(VoError) as ei:
            c.set_klt_predict(-1)
        assert ei.value.code == -1
        assert c.get_klt_predict() == "off"
        c.set_klt_predict(CV); assert c.get_klt_predict() == CV
        c.set_klt_predict(0); assert c.get_klt_predict() == "off"
        c.set_klt_predict(1); assert c.get_klt_predict() == CV
        with pytest.raises(VoError) as ei:
            c.klt_guess_read(1)                               # no predicted track has run
        assert ei.value.code == -4
        im = np.zeros((64, 64), np.uint8)
        c.push_frame(im); c.push_frame(im)
        c.klt_track(np.full((3, 2), 30, np.float32), init=np.full((3, 2), 31, np.float32))
        with pytest.raises(VoError) as ei:
            c.klt_guess_read(1)                               # the synchronous call takes its guesses from the caller: nothing predicted
        assert ei.value.code == -4
    sc, state = loop_scene
    with VoContext(W, H, max_pts=1024) as c:
        rp = _loop(c, sc, state, klt_predict=CV)
        rp.step(T1 + 1)
        with pytest.raises(VoError) as ei:
            c.klt_guess_read(1)                               # a step in flight
        assert ei.value.code == -4
        rec = rp.fetch()
        assert c.klt_guess_read(rec["n_tracked"]).shape == (rec["n_tracked"], 2)
