"""GPU: the device-resident track table (csrc/vo_tracks.hip) beyond one 1024-track chunk, against the list model tests/tracks_model.py
(itself pinned to the reference's own output by tests/test_tracks_model.py).

k_trk_extend compacts every column of the table in place, one workgroup per sequence walking the list in chunks of 1024; k_trk_spawn
appends 256 corners per trip; k_trk_obs and k_trk_predict run 256-wide blocks over the capacity / the host's loose upper bound n_hi.
Every comparison is bit-exact: the table only copies float32 positions and counts integers.  Deaths are planted -- a seed at
(-100, -100) stays there under the oracle's tracker and fails the keep rule -- and every scenario asserts on the model's side that it
reaches what it claims (a survivor crossing index 1024, an append above 256, the capacity clamp, deaths on both sides of 1024).

Frames are 320x240 (synthetic.make_sequence(..., margin=96)), points synthetic.grid_points.  The tracker treats every point on its own, so
the oracle's KLT is taken from a per-point memo (MemoKlt) that the scenarios of this module share.
"""
import ctypes as C

import numpy as np
import pytest

import klt_seed_model as km
import tracks_model as tm

pytestmark = pytest.mark.gpu

W, H = 320, 240
PLANT = (-100.0, -100.0)
CHUNK = 1024                      # k_trk_extend's chunk
T0 = 29                           # the seed frame of the long scenarios: the ring index (t & 31) wraps inside the run
CAP_B, N_SEED_B = 1500, 900       # 1500: no multiple of 256 or 1024
ST_B = dict(max_corners=4000, quality_level=0.003, min_distance=2.0, block_size=5)
RADIUS_B, MAX_NEW_B = 2, 1000


class MemoKlt:
    """vo_oracle.klt(prev, cur, p0)[0] from a memo per (frame pair, point): pyramidal LK treats every point independently, so the rows of
    one call are the rows of any other call with the same point -- planted indices do not change the other points' results"""

    def __init__(self):
        self.memo = {}

    def __call__(self, prev, cur, p0):
        import vo_oracle as o
        p0 = np.ascontiguousarray(np.asarray(p0, np.float32).reshape(-1, 2))
        d = self.memo.setdefault((prev.ctypes.data, cur.ctypes.data), {})
        keys = [r.tobytes() for r in p0]
        miss = sorted(set(keys) - set(d))
        if miss:
            q = np.frombuffer(b"".join(miss), np.float32).reshape(-1, 2)
            for k, r in zip(miss, o.klt(prev, cur, q)[0]):
                d[k] = r.copy()
        return np.array([d[k] for k in keys], np.float32).reshape(-1, 2)


MEMO = MemoKlt()
_FRAMES = {}


def _frames(seed, n, occluded_from=None):
    """the first n frames of make_sequence(12, seed), rendered once and kept alive for the module (the memo is keyed by their addresses)"""
    from vo_mi355x import synthetic as syn
    key = (seed, occluded_from)
    assert n <= 12
    if key not in _FRAMES:
        fr = syn.make_sequence(12, w=W, h=H, seed=seed, margin=96)[0]
        if occluded_from is not None:
            fr = np.stack([f if t < occluded_from else tm.occlude(f, 120, 80, 64, seed=11) for t, f in enumerate(fr)])
        _FRAMES[key] = np.ascontiguousarray(fr)
    return _FRAMES[key][:n]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_obs(c, m, t, window, cap, what=""):
    got = c.tracks_obs(t, window)
    assert got.shape == (window, cap, 2) and np.array_equal(got, m.obs(t, window, cap), equal_nan=True), what
    return got


# ================================================================================================
# a. compaction patterns, one frame each, cap 4096
# ================================================================================================
CAP_A = 4096
PATTERNS = {
    "none": lambda n: [],
    "every_second": lambda n: range(1, n, 2),                                # (the odd ones: at n = 1025 index 1024 survives and moves)
    "first": lambda n: [0],
    "last": lambda n: [n - 1],
    "everything": lambda n: range(n),
    "chunk0": lambda n: range(CHUNK),                                        # out_n = 0 on entering chunk 1
    "last_chunk": lambda n: range(CHUNK * ((n - 1) // CHUNK), n),            # none in chunk 0, all of the last chunk
    "i1023": lambda n: [CHUNK - 1],
    "i1024": lambda n: [CHUNK],
}
# the patterns that move a survivor from a source index >= 1024 to a destination < 1024 whenever n > 1024
CROSSING = {"every_second", "first", "chunk0", "i1023"}


def _cases_a():
    """every pattern that has a meaning of its own at that n: at 1024 there is one chunk (chunk0 = last_chunk = everything, i1023 = last);
    at 1025 and 2049 the last chunk is the last index alone, and at 1025 that index is 1024"""
    out = []
    for n in (1024, 1025, 2048, 2049, 4096):
        names = ["none", "every_second", "first", "last", "everything"]
        if n > CHUNK:
            names += ["chunk0", "i1023"]
            if (n - 1) % CHUNK:
                names.append("last_chunk")
            if n - 1 > CHUNK:
                names.append("i1024")
        seen = {}
        for name in names:
            seen.setdefault(tuple(PATTERNS[name](n)), name)
        assert len(seen) == len(names)                                        # no two names for one index set
        out += [(n, name) for name in names]
    return out


def test_the_patterns_cross_the_chunk_boundary_at_every_n_above_one_chunk():
    cases = _cases_a()
    for n in (1025, 2048, 2049, 4096):
        assert {p for m, p in cases if m == n} >= CROSSING
    assert min(n for n, _ in cases if n > CHUNK) == CHUNK + 1                 # the smallest shape at which the loop body runs twice


@pytest.mark.parametrize("n,pattern", _cases_a())
def test_compaction_patterns(n, pattern):
    """seed n points, plant deaths by index pattern, track one frame: table, dead list in list order and observation table = the model's.
    On the model's side: the dead count is the pattern plus the natural deaths, and every CROSSING pattern at n > 1024 has a survivor whose
    source index is >= 1024 and whose destination is < 1024.  (n = 1024 is the one-chunk control of the same patterns; the patterns that
    plant nothing in front of index 1024 -- none, last, last_chunk, i1024 -- and "everything" move no survivor across the boundary by
    their meaning, so the crossing is asserted for the others and, over the whole case list, by the test above.)"""
    from vo_mi355x import VoContext, synthetic as syn
    fr = _frames(70, 3)
    pts = syn.grid_points(n, W, H, seed=5, margin=4)
    planted = np.array(list(PATTERNS[pattern](n)), np.int64)
    assert len(planted) == 0 or (0 <= planted.min() and planted.max() < n)
    seeds = pts.copy()
    seeds[planted] = PLANT
    m = tm.TrackModel(W, H, klt=MEMO)
    m.seed(seeds, 0)
    dead = m.track(fr[0], fr[1], 1)
    # ---- the model's side: the case exercises what it claims ----
    p1 = MEMO(fr[0], fr[1], pts)
    natural = ~((p1[:, 0] >= 0) & (p1[:, 0] <= W) & (p1[:, 1] >= 0) & (p1[:, 1] <= H))
    natural[planted] = False
    assert np.array_equal(MEMO(fr[0], fr[1], np.array([PLANT], np.float32)), [PLANT])          # a planted seed stays where it is
    assert len(dead) == len(planted) + natural.sum() and set(planted.tolist()) <= set(dead)
    src = m.table()["tag"]                                                    # seeded tags are the source indices
    dst = np.arange(len(src))
    if pattern in CROSSING and n > CHUNK:
        assert n > CHUNK and ((src >= CHUNK) & (dst < CHUNK)).any()
    if pattern == "everything":
        assert len(m) == 0 and len(dead) == n
    if pattern == "chunk0":
        assert len(m) > 0 and src.min() >= CHUNK                              # chunk 1 starts writing at slot 0
    # ---- the kernel ----
    with VoContext(W, H, max_pts=CAP_A) as c:
        c.push_frame(fr[0])
        c.tracks_seed(seeds, t=0)
        c.push_frame(fr[1])
        c.tracks_track(1)
        tm.assert_table(c.tracks_read(), m, dead, what=(n, pattern))
        _same_obs(c, m, 1, 3, CAP_A, (n, pattern))
        if pattern == "everything":                                           # the table ended empty: track it again, then repopulate it
            c.push_frame(fr[2])
            c.tracks_track(2)
            assert m.track(fr[1], fr[2], 2) == []
            tm.assert_table(c.tracks_read(), m, [], what="empty")
            c.tracks_detect(2, mask_radius=7, params=c.st_params(), max_new=1000)
            found, added = m.detect(fr[2], 2, 7, dict(max_corners=1000, quality_level=0.03, min_distance=7, block_size=31), 1000, CAP_A)
            assert added == found > 0 and m.table()["tag"][0] == n            # tags go on where the seeds ended
            tm.assert_table(c.tracks_read(), m, [], what="repopulated")
            _same_obs(c, m, 2, 3, CAP_A, "repopulated")


# ================================================================================================
# b, c. growth and clamps over 12 frames at cap 1500; the same with the host's bound left loose
# ================================================================================================
def _seeds_b():
    from vo_mi355x import synthetic as syn
    return syn.grid_points(N_SEED_B, W, H, seed=5, margin=4)


def _run(c, m, fr, T, reads=True, fb=None, predict=False, window=12, detect_every=2):
    """seed 900 points at frame index T0, track T - 1 frames, re-detect every second frame; the model runs alongside.  With `reads` every
    frame is compared (which tightens the host's bound n_hi each time); without, nothing is read back until the caller does.
    `n_hi` restates the host's bookkeeping: + min(max_corners, max_new) per detection, clamped to the capacity, = the largest count after
    a read.  -> per-frame statistics of the model"""
    stp = c.st_params(**ST_B)
    seeds = _seeds_b()
    c.push_frame(fr[0])
    c.tracks_seed(seeds, t=T0)
    m.seed(seeds, T0)
    n_hi, stats = len(seeds), []
    for k in range(1, T):
        t = T0 + k
        c.push_frame(fr[k])
        before = m.table()["tag"]
        want_g = m.guess(t, n_hi) if predict else None
        c.tracks_track(t)
        dead = m.track(fr[k - 1], fr[k], t, fb_thr=fb, predict=predict)
        idx = np.nonzero(np.isin(before, dead))[0]
        st = dict(k=k, n_before=len(before), n_hi=n_hi, dead_lo=int((idx < CHUNK).sum()), dead_hi=int((idx >= CHUNK).sum()), found=None, added=None,
                  fb_dead=0)
        if predict:                                                           # over the loose n_hi: NaN beyond the count, bit for bit
            assert np.array_equal(_bits(c.klt_guess_read(n_hi)), _bits(want_g)), k
            st["nan_slots"] = int(np.isnan(want_g).all(-1).sum())
        if fb is not None:
            ok, e = c.fb_read(len(before))
            assert np.array_equal(ok, m.fb_ok) and np.array_equal(e, m.fb_err, equal_nan=True), k
            st["fb_dead"] = int((~m.fb_ok).sum())
        if reads:
            r = c.tracks_read()
            tm.assert_table(r, m, dead, what=("track", k))
            _same_obs(c, m, t, window, CAP_B, ("track", k))
            n_hi = len(r["tag"])
        if k % detect_every == 0:
            c.tracks_detect(t, mask_radius=RADIUS_B, params=stp, max_new=MAX_NEW_B)
            n_was = len(m)
            st["found"], st["added"] = m.detect(fr[k], t, RADIUS_B, ST_B, MAX_NEW_B, CAP_B)
            st["cap_clamped"] = st["added"] == CAP_B - n_was < min(st["found"], MAX_NEW_B)
            n_hi = min(n_hi + min(ST_B["max_corners"], MAX_NEW_B), CAP_B)
            if reads:
                r = c.tracks_read()
                tm.assert_table(r, m, dead, what=("detect", k))           # (the dead list of the last track is still there)
                _same_obs(c, m, t, window, CAP_B, ("detect", k))
                n_hi = len(r["tag"])
        st["dead"] = dead
        stats.append(st)
    return stats


_RUN_B = {}


def _run_b():
    """scenario (b) with a read after every call; its final read-back is kept for (c)"""
    from vo_mi355x import VoContext
    if not _RUN_B:
        T = 12
        fr = _frames(70, T)
        m = tm.TrackModel(W, H, klt=MEMO)
        with VoContext(W, H, max_pts=CAP_B) as c:
            stats = _run(c, m, fr, T)
            final = c.tracks_read()
            obs = c.tracks_obs(T0 + T - 1, 12)
        _RUN_B.update(stats=stats, final=final, obs=obs, model=m)
    return _RUN_B


def test_growth_and_clamps_over_12_frames_at_cap_1500():
    """every frame's table, dead list (in list order) and 12-slot observation table = the model's; the scene grows past one chunk with an
    append that takes more than two trips of the 256-wide loop, is cut by cap - n, and then loses tracks on both sides of index 1024"""
    stats = _run_b()["stats"]
    first = next(s for s in stats if s["found"] is not None)
    assert first["added"] > 2 * 256 and first["n_before"] < CHUNK < first["n_before"] - len(first["dead"]) + first["added"]
    assert any(s.get("cap_clamped") for s in stats) and max(s["n_before"] for s in stats) == CAP_B
    assert any(s["dead_lo"] > 0 and s["dead_hi"] > 0 and s["n_before"] > CHUNK for s in stats)
    assert (T0 & 31) > ((T0 + 11) & 31)                                       # the ring index wrapped


def test_the_loose_bound_over_12_frames_equals_the_model_and_the_tight_run():
    """the same scenario on a fresh context with no read-back of any kind until the last frame: n_hi stays an upper bound (900, then the
    capacity) while KLT, the disc kernel and the extend are cut by the device counts"""
    from vo_mi355x import VoContext
    b = _run_b()
    T = 12
    fr = _frames(70, T)
    m = tm.TrackModel(W, H, klt=MEMO)
    with VoContext(W, H, max_pts=CAP_B) as c:
        stats = _run(c, m, fr, T, reads=False)
        assert stats[-1]["n_hi"] == CAP_B > stats[-1]["n_before"] - len(stats[-1]["dead"])     # the bound was loose at the last track
        obs = _same_obs(c, m, T0 + T - 1, 12, CAP_B, "loose")
        r = c.tracks_read()
        tm.assert_table(r, m, stats[-1]["dead"], what="loose")
    for k in r:
        assert np.array_equal(r[k], b["final"][k]), k
    assert np.array_equal(obs, b["obs"], equal_nan=True)


def test_max_new_is_the_binding_clamp_and_max_new_zero():
    """at the first detection of the scenario the scene offers more corners than max_new = 300 and the list has room for more: max_new
    binds; before it, max_new = 0 appends nothing and moves no tag"""
    from vo_mi355x import VoContext
    fr = _frames(70, 12)
    seeds = _seeds_b()
    m = tm.TrackModel(W, H, klt=MEMO)
    with VoContext(W, H, max_pts=CAP_B) as c:
        stp = c.st_params(**ST_B)
        c.push_frame(fr[0]); c.tracks_seed(seeds, t=T0); m.seed(seeds, T0)
        c.push_frame(fr[1]); c.tracks_track(T0 + 1)
        dead = m.track(fr[0], fr[1], T0 + 1)
        c.tracks_detect(T0 + 1, mask_radius=RADIUS_B, params=stp, max_new=0)
        n_was, tag_was = len(m), m.next_tag
        found, added = m.detect(fr[1], T0 + 1, RADIUS_B, ST_B, 0, CAP_B)
        assert found > 0 and added == 0 and (len(m), m.next_tag) == (n_was, tag_was)
        tm.assert_table(c.tracks_read(), m, dead, what="max_new = 0")
        c.tracks_detect(T0 + 1, mask_radius=RADIUS_B, params=stp, max_new=300)
        found, added = m.detect(fr[1], T0 + 1, RADIUS_B, ST_B, 300, CAP_B)
        assert added == 300 < min(found, CAP_B - n_was) and len(m) > CHUNK     # max_new binds, not the scene and not the capacity
        tm.assert_table(c.tracks_read(), m, dead, what="max_new = 300")
        c.push_frame(fr[2]); c.tracks_track(T0 + 2)
        dead = m.track(fr[1], fr[2], T0 + 2)
        tm.assert_table(c.tracks_read(), m, dead, what="after")
        _same_obs(c, m, T0 + 2, 4, CAP_B, "after")


# ================================================================================================
# d. ragged batch of 3, cap 2500
# ================================================================================================
def test_ragged_batch_of_3_at_cap_2500():
    """2500 real points / exactly 1024 real points + padding / padding only, all uploaded as 2500 slots; six frames, detection at frames
    2 and 4.  Each sequence against its own model, the model's tags shifted past the padding it never saw"""
    from vo_mi355x import VoContext, synthetic as syn
    cap, T, n_real = 2500, 6, (2500, 1024, 0)
    frs = [_frames(70 + b, T) for b in range(3)]
    real = [syn.grid_points(n, W, H, seed=5 + b, margin=4) if n else np.zeros((0, 2), np.float32) for b, n in enumerate(n_real)]
    up = np.stack([np.vstack([p, np.full((cap - len(p), 2), PLANT[0], np.float32)]) for p in real])
    models = [tm.TrackModel(W, H, klt=MEMO) for _ in range(3)]
    shifts = [(lambda tag, n=n: tag + (cap - n if tag >= n else 0)) for n in n_real]
    dead_seen = [0, 0, 0]
    with VoContext(W, H, max_pts=cap, batch=3) as c:
        stp = c.st_params(**ST_B)
        c.push_frame(np.stack([f[0] for f in frs]))
        c.tracks_seed(up, t=0)
        for b in range(3):
            models[b].seed(real[b], 0)
        for t in range(1, T):
            c.push_frame(np.stack([f[t] for f in frs]))
            c.tracks_track(t)
            deads = [models[b].track(frs[b][t - 1], frs[b][t], t) for b in range(3)]
            if t in (2, 4):
                c.tracks_detect(t, mask_radius=RADIUS_B, params=stp, max_new=MAX_NEW_B)
                grown = [models[b].detect(frs[b][t], t, RADIUS_B, ST_B, MAX_NEW_B, cap) for b in range(3)]
                if t == 2:
                    assert grown[2][1] > 0 and len(models[1]) > CHUNK         # the empty sequence is repopulated; sequence 1 crosses the chunk
            rs = c.tracks_read()
            obs = c.tracks_obs(t, 6)
            for b in range(3):
                want_dead = [shifts[b](d) for d in deads[b]]
                if t == 1:                                                    # the padding died here, behind the real deaths, in list order
                    want_dead += list(range(n_real[b], cap))
                assert np.array_equal(rs[b]["dead_tag"], want_dead), (t, b)
                tm.assert_table(rs[b], models[b], None, tag_shift=shifts[b], what=(t, b))
                assert np.array_equal(obs[b], models[b].obs(t, 6, cap), equal_nan=True), (t, b)
                dead_seen[b] += len(deads[b])
            if t == 1:
                assert len(models[2]) == 0 and len(rs[2]["tag"]) == 0
    assert dead_seen[0] > 0 and len({len(mm) for mm in models}) == 3             # real deaths, and the counts differ across the batch


# ================================================================================================
# e. the other forms at the shape of (b), 6 frames each
# ================================================================================================
def _gpu_seeded_tracker(sync, checked):
    """the seeded tracker of the model at 1500 points: the synchronous seeded call of a second context (pinned bit for bit to klt_np by
    tests/test_gpu_klt_seed.py at 120 and 160 points), and klt_np itself on 48 of the points -- both sides of index 1024 -- of every call"""
    def f(prev, cur, p0, g):
        sync.push_frame(prev); sync.push_frame(cur)
        p1 = sync.klt_track(p0, init=g)[0]
        n = len(p0)
        idx = np.unique(np.concatenate([np.arange(0, n, max(1, n // 24)), np.arange(max(0, min(n, CHUNK) - 12), min(n, CHUNK + 12))]))[:48]
        assert np.array_equal(_bits(p1[idx]), _bits(km.klt_np(prev, cur, p0[idx], init=g[idx])[0]))
        checked.append((n, int((idx >= CHUNK).sum())))
        return p1
    return f


def test_forward_backward_check_at_cap_1500():
    """set_fb_check(0.75), an occluder pasted in from frame 3: fb_read = the model's flags, keep = inside AND good"""
    from vo_mi355x import VoContext
    fr = _frames(70, 6, occluded_from=3)
    m = tm.TrackModel(W, H, klt=MEMO)
    with VoContext(W, H, max_pts=CAP_B) as c:
        c.set_fb_check(0.75)
        stats = _run(c, m, fr, 6, fb=0.75, window=6)
    assert max(s["n_before"] for s in stats) == CAP_B
    assert any(s["fb_dead"] > 0 and s["k"] >= 3 for s in stats)               # the check, not only the border, killed tracks


def test_constant_velocity_prediction_at_cap_1500():
    """set_klt_predict("constant_velocity"): every frame's guesses over the loose n_hi, NaN slots included (no table is read back in between:
    a read would tighten the bound, and every detection of this scene fills the list), and the table at the end"""
    from vo_mi355x import VoContext
    fr = _frames(70, 6)
    checked = []
    with VoContext(W, H, max_pts=CAP_B) as c, VoContext(W, H, max_pts=CAP_B) as sync:
        m = tm.TrackModel(W, H, klt=MEMO, seeded_klt=_gpu_seeded_tracker(sync, checked))
        c.set_klt_predict("constant_velocity")
        stats = _run(c, m, fr, 6, reads=False, predict=True)
        _same_obs(c, m, T0 + 5, 6, CAP_B)
        tm.assert_table(c.tracks_read(), m, stats[-1]["dead"])
    assert any(s["nan_slots"] > 0 and s["n_before"] > CHUNK for s in stats)   # the bound was loose over more than one chunk
    assert any(n > CHUNK and hi > 0 for n, hi in checked)


def test_prediction_and_forward_backward_together_at_cap_1500():
    from vo_mi355x import VoContext
    fr = _frames(70, 6, occluded_from=3)
    checked = []
    with VoContext(W, H, max_pts=CAP_B) as c, VoContext(W, H, max_pts=CAP_B) as sync:
        m = tm.TrackModel(W, H, klt=MEMO, seeded_klt=_gpu_seeded_tracker(sync, checked))
        c.set_klt_predict("constant_velocity")
        c.set_fb_check(0.75)
        stats = _run(c, m, fr, 6, reads=False, fb=0.75, predict=True)
        _same_obs(c, m, T0 + 5, 6, CAP_B)
        tm.assert_table(c.tracks_read(), m, stats[-1]["dead"])
    assert any(s["nan_slots"] > 0 and s["n_before"] > CHUNK for s in stats)
    assert any(s["fb_dead"] > 0 and s["k"] >= 3 for s in stats)


def test_ba_observations_from_the_track_ring_at_cap_1500():
    """vo_ba_obs_from_tracks at cap 1500, window 5: solving the device-gathered table = solving the table tracks_obs hands to the host"""
    from vo_mi355x import VoContext, synthetic as syn
    Wn = 5
    fr = _frames(70, 6)
    s = syn.make_ba_scene(n_pts=CAP_B, n_slots=Wn, seed=4)
    m = tm.TrackModel(W, H, klt=MEMO)
    with VoContext(W, H, max_pts=CAP_B) as c:
        _run(c, m, fr, 6, reads=False)
        t = T0 + 5
        obs_host = _same_obs(c, m, t, Wn, CAP_B)
        n_live = len(m)
        assert CHUNK < n_live < CAP_B and np.isnan(obs_host[:, n_live:]).all() and np.isfinite(obs_host[0, :n_live]).all()
        c.ba_upload(s["K"], s["poses0"], s["points0"], np.full((Wn, CAP_B, 2), np.nan))
        c.ba_obs_from_tracks(t)
        c.ba_solve_resident(c.ba_params(max_iters=3))
        po_a, pt_a, st_a = c.ba_fetch()
        po_b, pt_b, st_b = c.ba_adjust(s["K"], s["poses0"], s["points0"], obs_host, c.ba_params(max_iters=3))
    assert np.array_equal(po_a, po_b) and np.array_equal(pt_a, pt_b) and st_a["cost"] == st_b["cost"] and st_a["iters"] == st_b["iters"]


# ================================================================================================
# f. tracks_obs edges at cap 1500
# ================================================================================================
def test_tracks_obs_edges_at_cap_1500():
    """the largest window (32), which is also longer than the sequence so far (slots before the seed frame read NaN; so do the slots
    before the birth of a re-detected track), a short one, and the refused windows 33 and 0"""
    from vo_mi355x import VoContext, VoError
    from vo_mi355x._lib import ptr
    T = 5
    fr = _frames(70, 6)
    m = tm.TrackModel(W, H, klt=MEMO)
    with VoContext(W, H, max_pts=CAP_B) as c:
        _run(c, m, fr, T, reads=False)
        t = T0 + T - 1
        assert len(m) > CHUNK and len({k["tf"] for k in m.tr}) > 1 and (t & 31) < (T0 & 31)
        full = _same_obs(c, m, t, 32, CAP_B)
        born = np.array([k["tf"] for k in m.tr])
        assert born[0] == T0 and np.isfinite(full[:T, 0]).all() and np.isnan(full[T:]).all()      # the sequence is T frames old
        new = np.nonzero(born == t)[0]
        assert len(new) and np.isnan(full[1:, new]).all() and np.isfinite(full[0, new]).all()
        _same_obs(c, m, t, T + 1, CAP_B)
        _same_obs(c, m, t, 1, CAP_B)
        for window in (33, 0):
            buf = np.full((max(window, 1), CAP_B, 2), 7.25)
            with pytest.raises(VoError) as ei:
                c._ck(c._L.vo_tracks_obs(c._h, int(t), window, ptr(buf, C.c_double)))
            assert ei.value.code == -1 and (buf == 7.25).all()                # VO_E_INVALID, the output untouched
        _same_obs(c, m, t, 32, CAP_B)                                          # and the table is as it was
