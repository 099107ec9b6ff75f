"""GPU: the four forms of the KLT tracker -- plain, forward-backward check, seeded, seeded with the check -- behind their common host path
(csrc/vo_klt.hip: vo_klt_enqueue), seen from outside: which form a track ran decides what fb_read / klt_guess_read answer afterwards, and
the forms agree bit for bit where their contracts say so.

What the kernels compute is pinned elsewhere (test_gpu_klt_fb.py, test_gpu_klt_seed.py); this file pins the selection and the book-keeping
around them, the n == 0 rules included: a track table without a live track skips the tracker altogether unless it predicts.
320 x 240 frames, batch 2, 16 points, default parameters."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B, W, H, N = 2, 320, 240, 16
CV = "constant_velocity"
FB_MAX = 1.0e30          # finite: the check runs; no honest fb_err reaches it, so the keep rule is the one of the check off
E_INVALID, E_STATE = -1, -4
SETTINGS = [(False, False), (True, False), (False, True), (True, True)]      # (check, predict)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(xs, ys):
    """tuples of arrays, bit for bit"""
    return len(xs) == len(ys) and all(np.array_equal(_bits(x), _bits(y)) if x.dtype.kind == "f" else np.array_equal(x, y) for x, y in zip(xs, ys))


def _same_tables(ta, tb):
    return all(_same([ra[k] for k in sorted(ra)], [rb[k] for k in sorted(ra)]) for ra, rb in zip(ta, tb))


def _code(fn, *a):
    """0, or the code a call is refused with"""
    from vo_mi355x import VoError
    try:
        fn(*a)
    except VoError as e:
        return e.code
    return 0


def _reads(c, n):
    return _code(c.fb_read, n), _code(c.klt_guess_read, n)


@pytest.fixture(scope="module")
def scene():
    from vo_mi355x import synthetic as syn
    frames = np.stack([syn.make_sequence(2, w=W, h=H, seed=77 + 5 * b, margin=64)[0] for b in range(B)])       # [B, 2, H, W]
    # quarter-pixel positions: p * 2^-level - 15 is exact in float32 on every level, so a track between two identical frames returns p itself
    seeds = np.stack([np.round(syn.grid_points(N, W, H, margin=40, seed=4 + b) * 4) / 4 for b in range(B)]).astype(np.float32)
    return frames, seeds


def _context(fb, predict):
    from vo_mi355x import VoContext
    c = VoContext(W, H, max_pts=64, batch=B)
    c.set_fb_check(FB_MAX if fb else np.inf)
    c.set_klt_predict(CV if predict else "off")
    return c


@pytest.fixture(scope="module")
def forms(scene):
    """per setting: the table tracked over a still frame (every history then has velocity zero) and then over a moving one; what the reads
    answer after that track, the guesses, and the tracker's own rows"""
    frames, seeds = scene
    out = {}
    for fb, predict in SETTINGS:
        with _context(fb, predict) as c:
            c.push_frame(frames[:, 0]); c.tracks_seed(seeds, t=0)
            c.push_frame(frames[:, 0]); c.tracks_track(1)
            still = c.tracks_read()
            c.push_frame(frames[:, 1]); c.tracks_track(2)
            out[fb, predict] = dict(still=still, reads=_reads(c, N), rows=c.points_download(N, return_iters=True), table=c.tracks_read(),
                                    guess=c.klt_guess_read(N) if predict else None, fb=c.fb_read(N) if fb else None)
    return out


@pytest.mark.parametrize("fb,predict", SETTINGS)
def test_reads_succeed_exactly_when_the_last_track_ran_that_form(forms, fb, predict):
    assert forms[fb, predict]["reads"] == (0 if fb else E_STATE, 0 if predict else E_STATE)


@pytest.mark.parametrize("fb", [False, True])
def test_zero_velocity_prediction_is_the_unpredicted_track(scene, forms, fb):
    seeds = scene[1]
    on, off = forms[fb, True], forms[fb, False]
    for b in range(B):                                       # the history the predictor saw: two entries, both the seed
        assert np.array_equal(_bits(on["still"][b]["uv"]), _bits(seeds[b])), b
    assert np.array_equal(_bits(on["guess"]), _bits(seeds))                  # g = uv + (uv - uv)
    assert _same(on["rows"], off["rows"])                    # p1, status, err, iters
    assert _same_tables(on["table"], off["table"])
    assert all(len(r["uv"]) > N // 2 for r in off["table"])


@pytest.mark.parametrize("predict", [False, True])
def test_the_check_leaves_p1_status_err_alone(forms, predict):
    on, off = forms[True, predict], forms[False, predict]
    assert on["fb"][0].all()                                 # (nothing fails FB_MAX: the keep rules agree)
    assert _same(on["rows"], off["rows"])
    assert _same_tables(on["table"], off["table"])


@pytest.mark.parametrize("fb,predict", SETTINGS)
def test_empty_table_skips_the_tracker_unless_it_predicts(scene, fb, predict):
    """tracks_track without a live track: without prediction nothing is enqueued, and the reads keep answering for the track before it; with
    prediction the tracker's path runs with n = 0 and notes its form"""
    frames, seeds = scene
    with _context(fb, predict) as c:
        c.push_frame(frames[:, 0]); c.push_frame(frames[:, 1])
        c.klt_track_fb(seeds)                                # the track before: the check on N points, nothing predicted
        assert _reads(c, N) == (0, E_STATE)
        c.tracks_seed(np.zeros((B, 0, 2), np.float32), t=0)
        c.tracks_track(1)
        if not predict:
            assert _reads(c, N) == (0, E_STATE)
        else:
            assert _reads(c, 0) == (0 if fb else E_STATE, 0)
            assert _reads(c, 1) == (E_INVALID if fb else E_STATE, E_INVALID)
        assert all(len(r["uv"]) == 0 for r in c.tracks_read())


def test_synchronous_forms(scene, forms):
    frames, seeds = scene
    empty = np.zeros((B, 0, 2), np.float32)
    with _context(True, True) as c:
        c.push_frame(frames[:, 0]); c.tracks_seed(seeds, t=0)
        c.push_frame(frames[:, 1]); c.tracks_track(1)
        assert _reads(c, N) == (0, 0)
        # n == 0: empty results, and neither read state is touched
        for call, init, n_out in ((c.klt_track, None, 4), (c.klt_track, empty, 4), (c.klt_track_fb, None, 6), (c.klt_track_fb, empty, 6)):
            z = call(empty, return_iters=True, init=init)
            assert len(z) == n_out and all(a.shape[:2] == (B, 0) for a in z)
            assert _reads(c, N) == (0, 0)
        # a guess at p0 is no guess
        plain = c.klt_track(seeds, return_iters=True)
        assert _reads(c, 0) == (E_STATE, E_STATE)
        assert _same(c.klt_track(seeds, return_iters=True, init=seeds), plain)
        assert _reads(c, 0) == (E_STATE, E_STATE)
        check = c.klt_track_fb(seeds, return_iters=True)
        assert _reads(c, N) == (0, E_STATE)
        assert _same(c.klt_track_fb(seeds, return_iters=True, init=seeds), check)
        assert _reads(c, N) == (0, E_STATE)
        assert _same((check[0], check[1], check[2], check[5]), plain)
    # the table runs tracked the seeds over this pair of frames: their tracker rows are the synchronous call's, their tables its p1 under the keep rule
    assert _same(forms[False, False]["rows"][1:], plain[1:])
    for b, row in enumerate(forms[False, False]["table"]):
        q = plain[0][b]
        keep = (q[:, 0] >= 0) & (q[:, 0] <= W) & (q[:, 1] >= 0) & (q[:, 1] <= H)
        assert np.array_equal(_bits(row["uv"]), _bits(q[keep])), b
