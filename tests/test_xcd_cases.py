"""CPU: the cases of tests/xcd_cases.py can show what tests/test_gpu_xcd_map.py looks for -- checked on the references alone.

A kernel whose block mapping sent sequence b + 8's blocks to sequence b (the stride of the one-sequence-per-XCD remap), or a neighbour's,
would pass a bit-for-bit comparison wherever the two sequences' expected outputs are equal.  So for every b < B - 8 every kind of expected
output of sequence b differs from that of b + 8 and of (b + 1) % B; no sequence is degenerate (every tracker case tracks, every detection
finds corners); the refinement's flags cover a stopped row and an unusable one.  Conditions, not tolerances."""
import numpy as np
import pytest

import xcd_cases as xc

W, H = xc.TRACK_SIZE


def _differs(per_seq, B, what):
    """per_seq(b) -> a tuple of arrays; every member differs between b and b + 8, and between b and (b + 1) % B"""
    for b in range(B - 8):
        x = per_seq(b)
        for other in (b + 8, (b + 1) % B):
            y = per_seq(other)
            for k, (u, v) in enumerate(zip(x, y)):
                assert u.shape != v.shape or not np.array_equal(u, v, equal_nan=u.dtype.kind == "f"), (what, k, b, other)


def test_the_batches_are_what_the_remap_needs():
    assert all(B % 8 == 0 and B // 8 >= 2 for B in xc.BATCHES) and 16 in xc.BATCHES and max(xc.BATCHES) <= xc.NSEQ
    assert any(B & (B - 1) for B in xc.BATCHES)                          # one batch is no power of two
    assert 1 in xc.NS and any(n > 1 and n % 2 for n in xc.NS) and any(n % 4 for n in xc.NS)


@pytest.mark.parametrize("B", xc.BATCHES)
@pytest.mark.parametrize("w,h,win", xc.FRAME_SIZES)
def test_every_level_and_scharr_plane_differs_along_the_stride(B, w, h, win):
    for t in range(2):
        st = xc.stores(w, h, win, t)
        n_lv = len(st[0][0])
        assert n_lv >= 2 and all(len(s[0]) == n_lv for s in st)
        _differs(lambda b: tuple(st[b][0]) + tuple(st[b][1]), B, ("store", w, h, t))
    top = xc.stores(w, h, win, 1)[0][0][-1]
    if (w, h) == xc.FRAME_SIZES[1][:2]:
        assert top.shape[0] * top.shape[1] <= 256                         # the coarsest level of the tiny size: one block


@pytest.mark.parametrize("B", xc.BATCHES)
@pytest.mark.parametrize("stage", xc.INGEST)
def test_every_ingest_stage_differs_along_the_stride_and_changes_the_frame(B, stage):
    for t in range(2):
        out = xc.ingest(stage, t)
        assert (out != xc.frames(W, H)[:, t]).mean() > 0.1                # the stage does something: a kernel that skipped it would show
        _differs(lambda b: tuple(xc.store_of(out[b])[0][:2]), B, (stage, t))
        if stage in xc.CLAHE_TILES:
            _differs(lambda b: (xc.clahe_luts(stage, t)[b],), B, (stage, t, "lut"))


@pytest.mark.parametrize("B", xc.BATCHES)
@pytest.mark.parametrize("n", xc.NS)
@pytest.mark.parametrize("form", xc.FORMS)
def test_every_tracker_case_tracks_and_differs_along_the_stride(B, n, form):
    p0, res = xc.keypoints(n), xc.tracked(form, n)
    for b in range(B):
        k = xc.live(n, b)
        assert np.isfinite(p0[b, :k]).all() and np.isnan(p0[b, k:]).all()
        r = res[b]
        assert r["status"][:k].sum() >= 1 and np.isfinite(r["p1"][:k][r["status"][:k] == 1]).all(), (form, n, b)
        assert (r["status"][k:] == 0).all() and (r["err"][k:] == 0).all() and (r["iters"][k:] == -1).all()
        if "ok" in r:
            assert r["ok"][:k].any() and not r["ok"][k:].any(), (form, n, b)
    assert len({xc.live(n, b) for b in range(B)}) > 1 or n == 1          # unequal live counts
    _differs(lambda b: (res[b]["p1"][:xc.live(n, b)], res[b]["err"][:xc.live(n, b)]), B, (form, n))
    if form.endswith("seeded"):                                          # the guesses matter: the seeded result is not the unseeded one
        plain = xc.tracked("plain", n)
        assert any(not np.array_equal(plain[b]["p1"], res[b]["p1"], equal_nan=True) for b in range(B))


def test_the_large_set_meets_the_border_and_loses_points():
    res = xc.tracked("plain", 150)
    assert all((r["status"][:xc.live(150, b)] == 0).any() for b, r in enumerate(res))
    assert any((r["iters"][:, 0] >= 3).any() for r in res)


@pytest.mark.parametrize("B", xc.BATCHES)
@pytest.mark.parametrize("w,h", xc.ST_SIZES)
def test_every_detection_finds_corners_and_differs_along_the_stride(B, w, h):
    det, pts = xc.detected(w, h), xc.st_points(w, h)
    assert np.isfinite(pts).all()
    for b in range(B):
        d = det[b]
        assert len(d["corners"]) >= 5 and d["n_candidates"] >= len(d["corners"]), (w, h, b)
        assert (d["mask"] == 0).any() and (d["mask"] == 255).any()       # the discs are there, and not everywhere
    _differs(lambda b: (det[b]["eig"], det[b]["mask"], det[b]["corners"]), B, ("shi-tomasi", w, h))


@pytest.mark.parametrize("B", xc.BATCHES)
@pytest.mark.parametrize("n", xc.NS)
def test_every_refinement_case_differs_along_the_stride_and_covers_the_flags(B, n):
    pts, res = xc.corners(n), xc.refined(n)
    flags = np.concatenate([res[b][2] for b in range(B)])
    assert (flags == 0).any() and (flags == 4).any(), np.bincount(flags, minlength=5)
    for b in range(B):
        k = xc.live_corners(n, b)
        assert (res[b][2][k:] == 4).all() and (res[b][2][:k] != 4).all()
    assert len({xc.live_corners(n, b) for b in range(B)}) > 1
    if n > 1:
        assert any((res[b][0][:xc.live_corners(n, b)] != pts[b, :xc.live_corners(n, b)]).any() for b in range(B))
    # (n = 1: a sequence without a corner has nothing to tell apart; those with one differ)
    have = [b for b in range(xc.NSEQ) if xc.live_corners(n, b)]
    for b in range(B - 8):
        for other in (b + 8, (b + 1) % B):
            if b in have and other in have:
                k = min(xc.live_corners(n, b), xc.live_corners(n, other))
                assert not np.array_equal(res[b][0][:k], res[other][0][:k]), (n, b, other)
            else:
                assert not np.array_equal(res[b][2], res[other][2]), (n, b, other)      # the flags tell them apart: 4 against not 4
