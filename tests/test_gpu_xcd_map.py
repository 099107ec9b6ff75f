"""GPU: the one-sequence-per-XCD block mapping (vo_xcd_assign, csrc/vo_internal.h, and the tracker's own copies of it in vo_klt.hip,
vo_klt_fb.hip, vo_klt_reuse.hip, vo_klt_seed.hip) at batches of 16 and 24, where its 8 * (q / nblk) term is not zero.

Every sequence of a batch holds its own images and keypoints (tests/xcd_cases.py; tests/test_xcd_cases.py shows that a swap along the
stride of 8 would be seen), every comparison is bit for bit against the CPU references, per sequence, over ALL sequences: frame chain,
ingest stages, every form of the tracker, Shi-Tomasi, cornerSubPix, the xcd_remap_off tuning field, and one fused step against single
contexts.  Blocks per sequence: the tracker 1, 5 and 150; cornerSubPix 1, 2 and 38; the CLAHE table kernel 1 and 12; the frame chain from 1
(the 12 x 9 level of 47 x 33) upwards.

What these tests can and cannot see.  A block takes ONE (block, sequence) pair from the mapping and derives every read and every write
from it, so a mapping that is wrong but still a bijection of the grid -- 8 * ((q / nblk) ^ 1) at batch 16, say -- only changes which
hardware block does which piece of work: the library built that way passed every batch-16 test here, as it must.  What a wrong divisor,
stride or block count does is leave pairs out and do others twice; the pairs left out keep whatever the buffers held.  Hence _dirty():
before every case the store, and the outputs of the operation under test, are filled with another sequence's data, so that a pair left
out shows as a wrong result and not as the previous test's right one.  (The synchronous undistort / clahe calls never remap.)"""
import numpy as np
import pytest

import xcd_cases as xc

pytestmark = pytest.mark.gpu

BATCH_IDS = ["B%d" % B for B in xc.BATCHES]
W, H = xc.TRACK_SIZE


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _eq(got, want):
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(_bits(got), _bits(want))


@pytest.fixture(scope="module")
def contexts():
    """get(B, w, h, win) -> the one context of that shape, with every setting the tests touch back at its default"""
    from vo_mi355x import VoContext
    made = {}

    def get(B, w, h, win=31):
        key = (B, w, h, win)
        if key not in made:
            made[key] = VoContext(w, h, max_pts=256, win=win, batch=B)
        c = made[key]
        c.set_tuning(klt_reuse=0, xcd_remap_off=0)
        c.apply_ingest(None, None, clear_missing=True)
        c.set_prefilter(0)
        c.set_fb_check(np.inf)
        c.set_klt_predict("off")
        return c

    yield get
    for c in made.values():
        c.close()


def _push(c, B, w, h, resident=False):
    """frames 0 and 1 of the first B sequences into the store"""
    fr = xc.frames(w, h)[:B]
    if resident:
        c.upload_sequence(fr)
        c.push_frame_resident(0); c.push_frame_resident(1)
    else:
        c.push_frame(fr[:, 0]); c.push_frame(fr[:, 1])


def _dirty(c, B, w, h, op=None):
    """both halves of the store, and with `op` the outputs of the operation under test, filled from frames the test does not use, every
    sequence holding another one's: a block that never ran leaves something wrong behind, not the previous test's right answer"""
    other = np.roll(xc.frames(w, h)[:B, 2], 1, axis=0)
    c.push_frame(other); c.push_frame(other[::-1])
    if op is not None:
        op()


def _read_store(c, B):
    """[which][b] -> (levels, Scharr planes) as the context holds them"""
    from vo_mi355x import VoError
    n_lv = 0
    while n_lv < 8:
        try:
            c.level_size(n_lv)
        except VoError:                                                   # above the top level
            break
        n_lv += 1
    out = []
    for which in (0, 1):
        per_seq = []
        for b in range(B):
            rd = [c.pyramid_read(which, l, seq=b) for l in range(n_lv)]
            per_seq.append(([r[0] for r in rd], [r[1] for r in rd]))
        out.append(per_seq)
    return out


def _assert_store(store, B, w, h, win, what):
    for which in (0, 1):
        want = xc.stores(w, h, win, which)
        for b in range(B):
            got_img, got_der = store[which][b]
            want_img, want_der = want[b]
            assert len(got_img) == len(want_img), (what, which, b, len(got_img), len(want_img))
            for l in range(len(want_img)):
                assert _eq(got_img[l], want_img[l]), "%s: level %d image of sequence %d, half %d" % (what, l, b, which)
                assert _eq(got_der[l], want_der[l]), "%s: level %d Scharr planes of sequence %d, half %d" % (what, l, b, which)


# ---- 1. the frame chain -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["pushed", "resident"])
@pytest.mark.parametrize("w,h,win", xc.FRAME_SIZES, ids=["%dx%d" % s[:2] for s in xc.FRAME_SIZES])
@pytest.mark.parametrize("B", xc.BATCHES, ids=BATCH_IDS)
def test_frame_chain_fills_every_sequences_store(contexts, B, w, h, win, path):
    c = contexts(B, w, h, win)
    _dirty(c, B, w, h)
    _push(c, B, w, h, resident=path == "resident")
    _assert_store(_read_store(c, B), B, w, h, win, path)


# ---- 2. the ingest stages -----------------------------------------------------------------------------------------------------------------
def _set_stage(c, stage):
    if stage.startswith("undistort"):
        c.set_undistort(xc.cam(W, H), xc.UND_DIST)
    if stage in xc.CLAHE_TILES:
        c.set_clahe(xc.CLAHE_CLIP, xc.CLAHE_TILES[stage])
    if stage == "bilateral":
        c.set_prefilter()


@pytest.mark.parametrize("stage", xc.INGEST)
@pytest.mark.parametrize("B", xc.BATCHES, ids=BATCH_IDS)
def test_ingest_stage_reaches_every_sequences_store(contexts, B, stage):
    """frame 0 pushed from the host, frame 1 from the uploaded sequence: levels 0 and 1 of both halves = the pyramid of the stage's model"""
    c = contexts(B, W, H)
    _set_stage(c, stage)
    _dirty(c, B, W, H)
    fr = xc.frames(W, H)[:B]
    c.upload_sequence(fr)
    c.push_frame(fr[:, 0])
    luts0 = c.clahe_lut_read() if stage in xc.CLAHE_TILES else None
    c.push_frame_resident(1)
    luts1 = c.clahe_lut_read() if stage in xc.CLAHE_TILES else None
    for which in (0, 1):
        want = xc.ingest(stage, which)
        for b in range(B):
            lv, der = xc.store_of(want[b])
            for l in range(2):
                got = c.pyramid_read(which, l, seq=b)
                assert _eq(got[0], lv[l]), "%s: level %d image of sequence %d, frame %d" % (stage, l, b, which)
                assert _eq(got[1], der[l]), "%s: level %d Scharr planes of sequence %d, frame %d" % (stage, l, b, which)
    for t, luts in ((0, luts0), (1, luts1)):
        if luts is not None:
            for b in range(B):
                assert _eq(luts[b], xc.clahe_luts(stage, t)[b]), "%s: tables of sequence %d, frame %d" % (stage, b, t)


@pytest.mark.parametrize("B", xc.BATCHES, ids=BATCH_IDS)
def test_synchronous_undistort_and_clahe_take_the_batch(contexts, B):
    c = contexts(B, W, H)
    _set_stage(c, "undistort_clahe")
    fr = np.ascontiguousarray(xc.frames(W, H)[:B, 1])
    got = c.undistort(fr)
    for b in range(B):
        assert _eq(got[b], xc.ingest("undistort", 1)[b]), "undistort: sequence %d" % b
    got = c.clahe(fr)                                                     # CLAHE alone, not the undistortion in front of it
    luts = c.clahe_lut_read()
    for b in range(B):
        assert _eq(got[b], xc.ingest("clahe_4x3", 1)[b]), "clahe: sequence %d" % b
        assert _eq(luts[b], xc.clahe_luts("clahe_4x3", 1)[b]), "clahe: tables of sequence %d" % b
    c.set_clahe(xc.CLAHE_CLIP, xc.CLAHE_TILES["clahe_1x1"])
    got = c.clahe(fr)
    for b in range(B):
        assert _eq(got[b], xc.ingest("clahe_1x1", 1)[b]), "clahe 1 x 1: sequence %d" % b


# ---- 3. the tracker, every form -----------------------------------------------------------------------------------------------------------
# (name, the reference's form, klt_reuse, forward-backward, seeded)
TRACKERS = [("plain_shipped", "plain", -1, False, False), ("plain_reuse", "plain", 1, False, False), ("fb", "fb", 0, True, False),
            ("seeded", "seeded", 0, False, True), ("fb_seeded", "fb_seeded", 0, True, True)]


def _track(c, B, n, fb, seeded):
    """-> dict of the form's outputs [B, ...]"""
    p0 = xc.keypoints(n)[:B]
    init = xc.guesses(n)[:B] if seeded else None
    if not fb:
        p1, st, err, it = c.klt_track(p0, return_iters=True, init=init)
        return dict(p1=p1, status=st, err=err, iters=it)
    c.set_fb_check(xc.FB_MAX_ERR)
    p1, st, err, p0r, fbe, it = c.klt_track_fb(p0, return_iters=True, init=init)
    ok, e = c.fb_read(n)
    assert _eq(e, fbe)
    return dict(p1=p1, status=st, err=err, iters=it, p0r=p0r, fb_err=fbe, ok=ok)


def _assert_tracked(got, B, form, n, what):
    want = xc.tracked(form, n)
    for b in range(B):
        k, r = xc.live(n, b), want[b]
        for name in ("status", "err", "iters"):                          # dead rows included: status 0, err 0, no level entered
            assert _eq(got[name][b], r[name]), "%s n = %d: %s of sequence %d" % (what, n, name, b)
        for name in ("p1", "p0r", "fb_err", "ok"):
            if name in r:
                assert _eq(got[name][b, :k], r[name][:k]), "%s n = %d: %s of sequence %d" % (what, n, name, b)
        if "ok" in r:
            assert not got["ok"][b, k:].any(), "%s n = %d: a dead row of sequence %d passed the check" % (what, n, b)


@pytest.mark.parametrize("n", xc.NS)
@pytest.mark.parametrize("name,form,reuse,fb,seeded", TRACKERS, ids=[t[0] for t in TRACKERS])
@pytest.mark.parametrize("B", xc.BATCHES, ids=BATCH_IDS)
def test_tracker_form_tracks_every_sequence_on_its_own_frames(contexts, B, name, form, reuse, fb, seeded, n):
    c = contexts(B, W, H)
    c.set_tuning(klt_reuse=reuse)
    _dirty(c, B, W, H, lambda: _track(c, B, n, fb, seeded))
    _push(c, B, W, H)
    _assert_tracked(_track(c, B, n, fb, seeded), B, form, n, name)


# ---- 4. Shi-Tomasi ------------------------------------------------------------------------------------------------------------------------
def _detect(c, B, w, h):
    corners = c.shi_tomasi(xc.st_points(w, h)[:B], xc.ST_RADIUS, params=c.st_params(**xc.ST_PARAMS))
    eig, mask, nc = c.shi_tomasi_read()
    return dict(corners=corners, eig=eig, mask=mask, n_candidates=nc)


def _assert_detected(got, B, w, h, what):
    want = xc.detected(w, h)
    for b in range(B):
        r = want[b]
        assert _eq(got["eig"][b], r["eig"]), "%s: eigenvalue map of sequence %d" % (what, b)
        assert _eq(got["mask"][b], r["mask"]), "%s: mask of sequence %d" % (what, b)
        assert int(got["n_candidates"][b]) == r["n_candidates"], "%s: candidates of sequence %d" % (what, b)
        assert _eq(got["corners"][b], r["corners"]), "%s: corners of sequence %d" % (what, b)


@pytest.mark.parametrize("w,h", xc.ST_SIZES, ids=["%dx%d" % s for s in xc.ST_SIZES])
@pytest.mark.parametrize("B", xc.BATCHES, ids=BATCH_IDS)
def test_shi_tomasi_detects_on_every_sequences_frame_around_its_own_points(contexts, B, w, h):
    c = contexts(B, w, h)
    _dirty(c, B, w, h, lambda: _detect(c, B, w, h))
    _push(c, B, w, h)
    _assert_detected(_detect(c, B, w, h), B, w, h, "%d x %d" % (w, h))


# ---- 5. cornerSubPix ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", xc.NS)
@pytest.mark.parametrize("B", xc.BATCHES, ids=BATCH_IDS)
def test_corner_subpix_refines_every_sequences_corners_on_its_own_frame(contexts, B, n):
    c = contexts(B, W, H)
    _dirty(c, B, W, H, lambda: c.corner_subpix(xc.corners(n)[:B]))
    _push(c, B, W, H)
    out, it, fl = c.corner_subpix(xc.corners(n)[:B], return_info=True)
    want = xc.refined(n)
    for b in range(B):
        k = xc.live_corners(n, b)
        assert _eq(out[b, :k], want[b][0][:k]), "n = %d: positions of sequence %d" % (n, b)
        assert np.isnan(out[b, k:]).all(), "n = %d: NaN rows of sequence %d" % (n, b)
        assert _eq(it[b], want[b][1]), "n = %d: iterations of sequence %d" % (n, b)
        assert _eq(fl[b], want[b][2]), "n = %d: flags of sequence %d" % (n, b)


# ---- 6. xcd_remap_off ---------------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_xcd_remap_off(contexts):
    """frame chain (pushed and resident), the plain tracker and Shi-Tomasi on one context of batch 16 with the plain (block, sequence)
    grids and with the remap: bit-equal to each other and to the references"""
    B = 16
    c = contexts(B, W, H)
    assert "xcd_remap_off" in c.tuning()
    runs = []
    for off in (1, 0):
        c.set_tuning(xcd_remap_off=off)
        assert c.tuning()["xcd_remap_off"] == off
        what = "xcd_remap_off = %d" % off
        _dirty(c, B, W, H)
        _push(c, B, W, H, resident=True)
        resident = _read_store(c, B)
        _assert_store(resident, B, W, H, 31, what + ", resident")
        _dirty(c, B, W, H)
        _push(c, B, W, H)
        pushed = _read_store(c, B)
        _assert_store(pushed, B, W, H, 31, what + ", pushed")
        tracked = {}
        for n in xc.NS:
            for reuse in (-1, 1):
                c.set_tuning(klt_reuse=reuse)
                tracked[n, reuse] = _track(c, B, n, False, False)
                _assert_tracked(tracked[n, reuse], B, "plain", n, "%s, klt_reuse = %d" % (what, reuse))
        det = _detect(c, B, W, H)
        _assert_detected(det, B, W, H, what)
        runs.append((resident, pushed, tracked, det))
    (res_a, push_a, trk_a, det_a), (res_b, push_b, trk_b, det_b) = runs
    for store_a, store_b in ((res_a, res_b), (push_a, push_b)):
        for which in (0, 1):
            for b in range(B):
                for x, y in zip(store_a[which][b][0] + store_a[which][b][1], store_b[which][b][0] + store_b[which][b][1]):
                    assert _eq(x, y), b
    for key in trk_a:
        for name in trk_a[key]:
            assert _eq(trk_a[key][name], trk_b[key][name]), (key, name)    # (NaN rows included)
    for name in ("eig", "mask", "n_candidates"):
        assert _eq(det_a[name], det_b[name]), name
    for b in range(B):
        assert _eq(det_a["corners"][b], det_b["corners"][b]), b


# ---- 7. one fused step --------------------------------------------------------------------------------------------------------------------
def _dlt_in(s, n_new):
    from vo_mi355x import synthetic as syn
    K = s["K"]
    H0, H1 = np.eye(4), np.eye(4)
    H0[:3, :3], H0[:3, 3] = syn.rodrigues(s["poses_gt"][3, :3]), s["poses_gt"][3, 3:]
    H1[:3, :3], H1[:3, 3] = syn.rodrigues(s["poses_gt"][0, :3]), s["poses_gt"][0, 3:]
    return ((K @ H0[:3]).astype(np.float32), (K @ H1[:3]).astype(np.float32), s["obs"][3, :n_new].astype(np.float32),
            s["obs"][0, :n_new].astype(np.float32), K, H0, H1)


STEP_KEYS = ("points2d", "status", "err", "corners")


def _switch_stages_on(c):
    c.set_undistort(xc.cam(W, H), xc.UND_DIST)
    c.set_clahe(xc.CLAHE_CLIP, xc.CLAHE_TILES["clahe_4x3"])
    c.set_subpix({})


def test_fused_steps_of_a_batch_of_16_equal_single_contexts():
    """frame_step_resident over the three frames with undistortion, CLAHE and cornerSubPix switched on, fetched step by step and with two
    steps in flight on the pipelined layout, against 16 contexts of batch 1 (never remapped): tracker, detector and level 0 of the store
    per sequence.  The bundle adjustment runs and is not compared: a batch folds its partial sums in another order."""
    from vo_mi355x import VoContext, synthetic as syn
    B, n, n_new = 16, min(xc.live(150, b) for b in range(16)), 60
    order = (1, 2, 1)
    frames = xc.frames(W, H)[:B]
    pts = np.ascontiguousarray(xc.keypoints(150)[:B, :n])
    assert np.isfinite(pts).all()
    scenes = [syn.make_ba_scene(n_pts=80, n_slots=5, seed=30 + b, visibility=0.9) for b in range(B)]
    d = [_dlt_in(s, n_new) for s in scenes]
    st_kw = dict(xc.ST_PARAMS)

    def step(c, f):
        c.frame_step_resident(f, n, mask_radius=xc.ST_RADIUS, st=c.st_params(**st_kw), ba=c.ba_params(max_iters=5))

    ref = []
    for b in range(B):
        with VoContext(W, H, max_pts=256) as c:
            _switch_stages_on(c)
            s = scenes[b]
            c.upload_sequence(frames[b]); c.points_upload(pts[b]); c.dlt_upload(*d[b]); c.ba_upload(s["K"], s["poses0"], s["points0"], s["obs"])
            c.push_frame_resident(0)
            steps = []
            for f in order:
                step(c, f)
                steps.append(c.frame_fetch())
            ref.append((steps, c.pyramid_read(1, 0)[0]))
        assert _eq(ref[b][1], xc.ingest("undistort_clahe", order[-1])[b]), b
        assert ref[b][0][0]["status"].any() and len(ref[b][0][0]["corners"]) >= 5, b

    def compare(got_all, c, what):
        for k, got in enumerate(got_all):
            for b in range(B):
                for key in STEP_KEYS:
                    assert _eq(got[key][b], ref[b][0][k][key]), "%s: %s of sequence %d, step %d" % (what, key, b, k)
        for b in range(B):
            assert _eq(c.pyramid_read(1, 0, seq=b)[0], ref[b][1]), "%s: level 0 of sequence %d" % (what, b)

    with VoContext(W, H, max_pts=256, batch=B) as c:
        _switch_stages_on(c)
        c.upload_sequence(frames); c.points_upload(pts)
        c.dlt_upload(*[np.stack([d[b][k] for b in range(B)]) for k in range(7)])
        c.ba_upload(np.stack([s["K"] for s in scenes]), np.stack([s["poses0"] for s in scenes]),
                    np.stack([s["points0"] for s in scenes]), np.stack([s["obs"] for s in scenes]))
        c.push_frame_resident(0)
        got_all = []
        for f in order:
            step(c, f)
            got_all.append(c.frame_fetch())
        compare(got_all, c, "step by step")
        # the same steps in the pipelined stream layout with two steps in flight
        c.set_tuning(gate_groups=3, reserve_cus=32)
        c.set_side_stream("pipeline")
        assert c.step_layout()["layout"] == 2
        c.points_upload(pts)
        c.push_frame_resident(0)
        got_all = []
        step(c, order[0])
        for f in order[1:]:
            step(c, f)
            got_all.append(c.frame_fetch())
        got_all.append(c.frame_fetch())
        compare(got_all, c, "two steps in flight")
