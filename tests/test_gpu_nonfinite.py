"""GPU: keypoints that are NaN, infinite or beyond int32 (tests/nonfinite_cases.py) in every tracker form, in the exclusion discs of every
detector form, in the fused step and in the track table -- against the CPU oracle, whose outcome on these rows tests/test_nonfinite_cases.py
pins to a second restatement.

The contract (include/vo_mi355x.h): a p0 row with a NaN component leaves every tracker form as OpenCV leaves it -- status 0, err 0, no level
entered -- with a p1 row that is not finite; infinite rows and rows beyond int32 pass through exactly; no such row draws an exclusion disc,
disturbs a neighbour, or survives in a track table.  160 x 120 frames, 62 points (25 honest)."""
import numpy as np
import pytest

import fast_model as fm
import klt_seed_model as km
import nonfinite_cases as nc
import tracks_model as tm
import vo_oracle as o

pytestmark = pytest.mark.gpu

W, H = nc.W, nc.H
ST = dict(max_corners=1000, quality_level=0.03, min_distance=7, block_size=31)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def case():
    """frames [3, H, W], p0, kind and the oracle's unseeded result on frames 0 -> 1 -- computed once, never modified"""
    fr = nc.frames(n=3)
    p0, kind = nc.points()
    return fr, p0, kind, o.klt(fr[0], fr[1], p0, return_iters=True)


@pytest.fixture(scope="module")
def ctx(case):
    from vo_mi355x import VoContext
    with VoContext(W, H, max_pts=128) as c:
        c.push_frame(case[0][0]); c.push_frame(case[0][1])
        yield c


def _check_rows(got, want, p0, kind, what):
    """got / want = (p1, status, err, iters) over the rows p0"""
    nan = nc.has_nan(p0)
    special = kind != "honest"
    print("%s: %d rows, %d special (%d with a NaN), status 0 on %d (oracle %d)" % (what, len(p0), special.sum(), nan.sum(), (got[1] == 0).sum(),
                                                                                 (want[1] == 0).sum()))
    assert np.array_equal(got[1], want[1]), (what, "status", np.flatnonzero(got[1] != want[1]))
    assert np.array_equal(_bits(got[2]), _bits(want[2])), (what, "err", np.flatnonzero(got[2] != want[2]))
    assert np.array_equal(got[3], want[3]), (what, "iters", np.flatnonzero((got[3] != want[3]).any(-1)))
    assert np.array_equal(_bits(got[0][~nan]), _bits(want[0][~nan])), (what, "p1", np.flatnonzero((_bits(got[0]) != _bits(want[0])).any(-1) & ~nan))
    assert not np.isfinite(got[0][nan]).all(-1).any(), (what, "p1 of a NaN row is finite", got[0][nan])


def _check_alone(run, got, p0, kind, what):
    """the honest rows equal a run without the special rows: a special row cannot disturb a neighbour's wave"""
    hon = kind == "honest"
    alone = run(p0[hon])
    for k in range(4):
        assert np.array_equal(_bits(got[k][hon]), _bits(alone[k])), (what, "honest rows beside special ones", k)


# ---- 1. tracker against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,tuning", [("waves4", dict(klt_waves=4)), ("waves5", dict(klt_waves=5)), ("waves6", dict(klt_waves=6)),
                                         ("reuse_on", dict(klt_reuse=1)), ("reuse_off", dict(klt_reuse=-1))])
def test_klt_track_every_kernel(ctx, case, form, tuning):
    fr, p0, kind, want = case
    ctx.set_tuning(klt_waves=0, klt_reuse=0)
    ctx.set_tuning(**tuning)
    try:
        run = lambda p: ctx.klt_track(p, return_iters=True)
        got = run(p0)
        _check_rows(got, want, p0, kind, form)
        _check_alone(run, got, p0, kind, form)
        # the synchronous call hands the caller's own NaN row back, like the oracle's pass-through
        nan = nc.has_nan(p0)
        assert np.array_equal(_bits(got[0][nan]), _bits(p0[nan])), form
    finally:
        ctx.set_tuning(klt_waves=0, klt_reuse=0)


def test_klt_track_fb(ctx, case):
    fr, p0, kind, want = case
    nan = nc.has_nan(p0)
    thr = 1.0
    ctx.set_fb_check(thr)
    try:
        p1, st, err, p0r, fbe, it = ctx.klt_track_fb(p0, return_iters=True)
        ok, fbe2 = ctx.fb_read(len(p0))
    finally:
        ctx.set_fb_check(np.inf)
    _check_rows((p1, st, err, it), want, p0, kind, "fb forward")
    r0 = o.klt(fr[1], fr[0], want[0])[0]                      # the backward pass of the oracle's p1 (NaN rows pass through again)
    with np.errstate(invalid="ignore"):
        e_want, ok_want = tm.fb_np(p0, r0, thr)
    assert np.array_equal(_bits(p0r[~nan]), _bits(r0[~nan])) and np.array_equal(p0r, r0, equal_nan=True)
    assert np.array_equal(fbe, e_want, equal_nan=True) and np.array_equal(_bits(fbe), _bits(fbe2))
    assert np.array_equal(ok, ok_want)
    nonfin = ~np.isfinite(p0).all(-1)
    print("fb: ok on %d rows, %d NaN rows, %d rows that are not finite" % (ok.sum(), nan.sum(), nonfin.sum()))
    assert not ok[nonfin].any()                                # (a huge finite row comes back exactly: its check passes, its status is 0)
    assert not (fbe[nan] < np.float32(np.inf)).any()           # not below any threshold
    assert ok[kind == "honest"].all()


@pytest.mark.parametrize("name", ["finite_guess_special_p0", "special_guess_honest_p0"])
def test_klt_track_seeded(ctx, case, name):
    fr = case[0]
    p0, g, kind = nc.seed_cases()[name]
    want = o.klt(fr[0], fr[1], p0, return_iters=True, init=g)
    got = ctx.klt_track(p0, return_iters=True, init=g)
    _check_rows(got, want, p0, kind, name)
    hon = kind == "honest"
    alone = ctx.klt_track(p0[hon], return_iters=True, init=g[hon])
    for k in range(4):
        assert np.array_equal(_bits(got[k][hon]), _bits(alone[k])), (name, k)
    # with the forward-backward check in the same launch: the forward results are the same
    f = ctx.klt_track_fb(p0, return_iters=True, init=g)
    _check_rows((f[0], f[1], f[2], f[5]), want, p0, kind, name + " + fb")
    nan = nc.has_nan(p0)
    assert not (f[4][nan] < np.float32(np.inf)).any()


def test_klt_track_resident_after_points_upload(ctx, case):
    fr, p0, kind, want = case
    ctx.points_upload(p0)
    ctx.klt_track_resident(len(p0))
    got = ctx.points_download(len(p0), return_iters=True)
    _check_rows(got, want, p0, kind, "resident")


def test_klt_track_batch_of_three_with_rotated_rows():
    from vo_mi355x import VoContext
    fr, pb, kb = nc.batch3()
    with VoContext(W, H, max_pts=128, batch=3) as c:
        c.push_frame(fr[:, 0]); c.push_frame(fr[:, 1])
        got = c.klt_track(pb, return_iters=True)
        hon = np.stack([pb[b][kb[b] == "honest"] for b in range(3)])
        alone = c.klt_track(hon, return_iters=True)
    for b in range(3):
        want = o.klt(fr[b, 0], fr[b, 1], pb[b], return_iters=True)
        _check_rows([x[b] for x in got], want, pb[b], kb[b], "batch sequence %d" % b)
        for k in range(4):
            assert np.array_equal(_bits(got[k][b][kb[b] == "honest"]), _bits(alone[k][b])), (b, k)


# ---- 2. exclusion discs --------------------------------------------------------------------------------------------------------------------
def _group(p0, kind, group):
    """special: honest + every row OpenCV draws nothing for; border: honest + the rows whose disc the border cuts"""
    keep = (kind != "border") if group == "special" else ((kind == "honest") | (kind == "border"))
    return p0[keep], kind[keep]


def _check_detector(c, img, pts, r, response, user, what):
    """one sequence: corners, kept mask, response map and candidate count of vo_shi_tomasi / vo_shi_tomasi_read against the oracle"""
    got, (eig, mask, ncand) = c
    want_mask = nc.disc_mask(pts, r, base=user)
    cleared = int((want_mask == 0).sum()) - (0 if user is None else int((user == 0).sum()))
    print("%s: %d centres, %d of them INT_MIN, %d pixels cleared (GPU %d)" % (what, len(pts), (km.to_int32(pts) == km.INT_MIN).any(-1).sum(), cleared,
                                                                                   int((mask == 0).sum()) - (0 if user is None else int((user == 0).sum()))))
    assert np.array_equal(mask, want_mask), (what, "mask", np.argwhere(mask != want_mask)[:8])
    if response == "fast":
        R = fm.score_map(img, 20).astype(np.float32)
        assert np.array_equal(eig, R), (what, "response")
        assert ncand == len(fm.candidates(R, want_mask, 0.03)[1]), (what, "candidates")
        want = fm.select(R, want_mask, 1000, 0.03, 7)
    else:
        want, _, n_want = o.good_features(img, want_mask, return_aux=True, **{"maxCorners": 1000, "qualityLevel": 0.03, "minDistance": 7, "blockSize": 31})
        assert np.array_equal(eig, o.min_eig(img)), (what, "response")
        assert ncand == n_want, (what, "candidates")
    assert got.shape == want.shape and np.array_equal(got, want), (what, "corners", len(got), len(want))
    return cleared


@pytest.mark.parametrize("response", ["fused", "two_kernel", "fast"])
@pytest.mark.parametrize("r", nc.RADII)
@pytest.mark.parametrize("group", ["special", "border"])
def test_discs(ctx, case, group, r, response):
    fr, p0, kind, _ = case
    pts, _ = _group(p0, kind, group)
    assert len(pts) % 4 != 0
    prm = ctx.st_params(fast_threshold=20 if response == "fast" else 0, **ST)
    ctx.set_tuning(st_two_kernels=1 if response == "two_kernel" else 0)
    try:
        got = ctx.shi_tomasi(pts, r, params=prm)
        cleared = _check_detector((got, ctx.shi_tomasi_read()), fr[1], pts, r, response, None, (group, r, response))
        assert cleared > 0 and len(got) > 0
        if group == "special":                                 # the special rows draw nothing: the mask of the honest rows alone
            hon = p0[kind == "honest"]
            assert np.array_equal(ctx.shi_tomasi_read()[1], nc.disc_mask(hon, r))
    finally:
        ctx.set_tuning(st_two_kernels=0)


@pytest.mark.parametrize("group", ["special", "border"])
def test_discs_over_a_user_mask(ctx, case, group):
    fr, p0, kind, _ = case
    pts, _ = _group(p0, kind, group)
    user = np.full((H, W), 255, np.uint8)
    user[30:50, 100:140] = 0; user[::9, ::7] = 0
    got = ctx.shi_tomasi(pts, 7, mask=user, params=ctx.st_params(**ST))
    _check_detector((got, ctx.shi_tomasi_read()), fr[1], pts, 7, "fused", user, (group, "user mask"))


@pytest.mark.parametrize("group", ["special", "border"])
def test_discs_batch_of_three_with_rows_of_each_sequence(group):
    from vo_mi355x import VoContext
    fr, pb, kb = nc.batch3()
    sel = [_group(pb[b], kb[b], group)[0] for b in range(3)]
    assert len({len(s) for s in sel}) == 1
    pts = np.stack(sel)
    with VoContext(W, H, max_pts=128, batch=3) as c:
        c.push_frame(fr[:, 1])
        got = c.shi_tomasi(pts, 7, params=c.st_params(**ST))
        eig, mask, ncand = c.shi_tomasi_read()
    for b in range(3):
        _check_detector((got[b], (eig[b], mask[b], int(ncand[b]))), fr[b, 1], pts[b], 7, "fused", None, (group, "sequence", b))


# ---- 3. fused step -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graph", [False, True], ids=["launches", "graph"])
@pytest.mark.parametrize("entry", ["resident", "host"])
def test_fused_step_with_redetection(case, entry, graph):
    """two steps: the special rows of the uploaded set reach the tracker, then the discs of the re-detection, then -- as the p1 of step 1 --
    the tracker and the discs of step 2, with no host code in between.  The set holds no border row: a disc at the origin would show."""
    from vo_mi355x import VoContext
    fr, p0, kind, _ = case
    pts, knd = nc.without_border(p0, kind)
    n = len(pts)
    assert n % 4 != 0 and nc.has_nan(pts).sum() == 7
    with VoContext(W, H, max_pts=128) as c:
        c.set_graph_mode(graph)
        if entry == "resident":
            c.upload_sequence(fr); c.points_upload(pts); c.push_frame_resident(0)
        else:
            c.push_frame(fr[0]); c.points_upload(pts)
            host = [VoContext.host_alloc((H, W)) for _ in range(2)]
            host[0][:] = fr[1]; host[1][:] = fr[2]
        got = []
        for s in (1, 2):
            if entry == "resident":
                c.frame_step_resident(s, n, do_dlt=False, do_ba=False, do_st=True, mask_radius=7, st=c.st_params(**ST))
            else:
                c.frame_step_host(host[s - 1], n, do_dlt=False, do_ba=False, do_st=True, mask_radius=7, st=c.st_params(**ST))
            got.append(c.frame_fetch())
    q = pts
    for s, g in zip((1, 2), got):
        q1, qs, qe = o.klt(fr[s - 1], fr[s], q)
        nan = nc.has_nan(q)
        mask = nc.disc_mask(q1, 7)                              # discs at to_int32 of ALL n rows of the oracle's p1
        want = o.good_features(fr[s], mask, maxCorners=1000, qualityLevel=0.03, minDistance=7, blockSize=31)
        print("step %d (%s, %s): %d rows, %d special, status 0 on %d (oracle %d), %d pixels cleared, %d corners (oracle %d)" % (
            s, entry, "graph" if graph else "launches", n, (knd != "honest").sum(), (g["status"] == 0).sum(), (qs == 0).sum(), (mask == 0).sum(),
            len(g["corners"]), len(want)))
        assert np.array_equal(g["status"], qs), (s, "status")
        assert np.array_equal(_bits(g["err"]), _bits(qe)), (s, "err")
        assert np.array_equal(_bits(g["points2d"][~nan]), _bits(q1[~nan])), (s, "p1")
        assert not np.isfinite(g["points2d"][nan]).all(-1).any(), (s, "p1 of a NaN row is finite")
        assert g["corners"].shape == want.shape and np.array_equal(g["corners"], want), (s, "corners")
        # ... which a disc at the origin or on column 0 would have changed (tests/test_nonfinite_cases.py, here on this step's own mask)
        for centre in ((0, 0), (0, 60)):
            m = mask.copy(); o.circle_mask(m, centre, 7, 0)
            other = o.good_features(fr[s], m, maxCorners=1000, qualityLevel=0.03, minDistance=7, blockSize=31)
            assert not (other.shape == want.shape and np.array_equal(other, want)), (s, centre)
        q = q1


# ---- 4. track table ------------------------------------------------------------------------------------------------------------------------
def test_track_table_drops_every_special_row_in_the_first_frame():
    """batch of 3 with the rotated rows; sequence 1 also loses five honest rows, so the count vector is ragged when the discs are drawn"""
    from vo_mi355x import VoContext
    fr, pb, kb = nc.batch3()
    pb = pb.copy()
    lost = np.flatnonzero(kb[1] == "honest")[:5]
    pb[1, lost] = (-200.0, -200.0)
    cap, max_new = 128, 40
    models, deads = [], []
    for b in range(3):
        m = tm.TrackModel(W, H)
        m.seed(pb[b], 0)
        deads.append(m.track(fr[b, 0], fr[b, 1], 1))
        models.append(m)
    with VoContext(W, H, max_pts=cap, batch=3) as c:
        c.push_frame(fr[:, 0]); c.tracks_seed(pb, t=0)
        c.push_frame(fr[:, 1]); c.tracks_track(1)
        r1 = c.tracks_read()
        obs = c.tracks_obs(1, 3)
        c.tracks_detect(1, mask_radius=7, params=c.st_params(**ST), max_new=max_new)
        r2 = c.tracks_read()
    counts = [len(r["tag"]) for r in r1]
    print("live after the first frame:", counts, "dead:", [len(d) for d in deads])
    assert len(set(counts)) > 1
    for b in range(3):
        m = models[b]
        tm.assert_table(r1[b], m, deads[b], what=("tracked", b))
        assert np.array_equal(obs[b], m.obs(1, 3, cap), equal_nan=True), b
        gone = np.flatnonzero((kb[b] == "dead") | (kb[b] == "far"))
        assert len(gone) == 28 and not np.isin(gone, r1[b]["tag"]).any() and np.isin(gone, r1[b]["dead_tag"]).all(), b
        assert np.isfinite(r1[b]["uv"]).all() and np.isfinite(r1[b]["uv_first"]).all(), b
        found, added = m.detect(fr[b, 1], 1, 7, ST, max_new, cap)
        print("sequence %d: %d corners found, %d spawned" % (b, found, added))
        assert added > 0
        tm.assert_table(r2[b], m, deads[b], what=("detected", b))
