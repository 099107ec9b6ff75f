"""GPU: k_klt_track_r (csrc/vo_klt_reuse.hip; vo_tuning.klt_reuse = 1), the plain tracker that keeps the widened target window in LDS while LK stays
in one integer pixel cell, against k_klt_track (klt_reuse = -1) and against the CPU oracle: p1, status, err and the iteration table bit for bit.

What can go wrong is a window kept when it should have been fetched: after the cell moved in x only, in y only or in both, in the error pass behind
the last iteration, across a level change (the cell numbers can coincide while the images differ), or with no iteration at all (max_count = 0).
The frame pairs below put at least ten points into every one of these classes, asserted on the oracle's outputs alone.
320 x 240 frames, 200 points; the fused step and the closed loop at 256 x 160."""
import copy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W, H, N = 320, 240, 200
MARGIN = 96                                   # make_sequence's
PARAMS = [(31, 0, 30), (31, 0, 1), (31, 0, 0), (31, 3, 30), (21, 1, 30), (9, 2, 30)]        # (win, max_level, max_count)
EPS_TIGHT = 0.001                             # the sub-pixel pair: at the default 0.03 every point converges in two iterations
EDGE_POINTS = np.array([(0.3, 0.2), (0.6, 0.9), (0.4, 120.3), (160.2, 0.3), (319.2, 239.4), (0.2, 239.3), (319.4, 0.4), (158.7, 239.2), (319.3, 121.6)],
                       np.float32)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(xs, ys):
    return len(xs) == len(ys) and all(x.shape == y.shape and np.array_equal(_bits(x), _bits(y)) for x, y in zip(xs, ys))


@pytest.fixture(scope="module")
def pairs():
    """name -> (im0, im1, p0)"""
    from vo_mi355x import synthetic as syn
    fr, _ = syn.make_sequence(4, W, H, seed=5)
    p0 = syn.grid_points(N, W, H, seed=1)
    A = syn.frame_motion(0, W, H)
    A[:, 2] += (0.3, 0.2)                     # frame 0 again, moved by a fraction of a pixel
    sub = syn.render_frame(syn.make_texture(H + 2 * MARGIN, W + 2 * MARGIN, 5), A, W, H, MARGIN)
    return {"moving": (fr[0], fr[2], p0),
            "transposed": (np.ascontiguousarray(fr[0].T), np.ascontiguousarray(fr[2].T), np.ascontiguousarray(p0[:, ::-1])),
            "subpixel": (fr[0], sub, p0),
            "stationary": (fr[0], fr[0], EDGE_POINTS)}


_oracle_cache = {}


def _oracle(pairs, name, win, max_level, max_count, eps=0.03):
    """computed once per case, shared by the coverage test and the comparisons, never modified"""
    import vo_oracle as o
    key = (name, win, max_level, max_count, eps)
    if key not in _oracle_cache:
        im0, im1, p0 = pairs[name]
        _oracle_cache[key] = o.klt(im0, im1, p0, (win, win), max_level, (3, max_count, eps), return_iters=True)
    return _oracle_cache[key]


def _gpu(c, p0, win, max_level, max_count, eps, reuse):
    c.set_tuning(klt_reuse=reuse)
    assert c.tuning()["klt_reuse"] == reuse
    return c.klt_track(p0, c.klt_params(win=win, max_level=max_level, max_count=max_count, epsilon=eps), return_iters=True)


def _check(c, pairs, name, win, max_level, max_count, eps=0.03):
    im0, im1, p0 = pairs[name]
    c.push_frame(im0); c.push_frame(im1)
    want = _oracle(pairs, name, win, max_level, max_count, eps)
    new = _gpu(c, p0, win, max_level, max_count, eps, 1)
    old = _gpu(c, p0, win, max_level, max_count, eps, -1)
    for k, what in enumerate(("p1", "status", "err", "iters")):
        assert np.array_equal(_bits(new[k]), _bits(old[k])), (name, what, "klt_reuse 1 against -1")
        assert np.array_equal(_bits(new[k]), _bits(want[k])), (name, what, "klt_reuse 1 against the oracle")


@pytest.fixture(scope="module")
def ctx():
    from vo_mi355x import VoContext
    with VoContext(W, H, max_pts=256) as c:
        yield c
        c.set_tuning(klt_reuse=0)


@pytest.fixture(scope="module")
def ctx_t():
    from vo_mi355x import VoContext
    with VoContext(H, W, max_pts=256) as c:
        yield c


def _classes(pairs, name, max_count, eps=0.03):
    """points of max_level = 0 by how the window's cell moved from the first sampling to the result: (x only, y only, both, neither with >= 3
    iterations), from the oracle's arrays alone; and how many were tracked"""
    p0 = pairs[name][2]
    p1, st, _, it = _oracle(pairs, name, 31, 0, max_count, eps)
    half = np.float32(15)
    c0, c1 = np.floor(p0 - half), np.floor(p1 - half)
    dx, dy, ok = c0[:, 0] != c1[:, 0], c0[:, 1] != c1[:, 1], st == 1
    return int((dx & ~dy & ok).sum()), int((~dx & dy & ok).sum()), int((dx & dy & ok).sum()), int((~dx & ~dy & ok & (it[:, 0] >= 3)).sum()), int(ok.sum())


def test_the_pairs_cover_every_way_the_cell_can_move(pairs):
    assert _classes(pairs, "moving", 30) == (13, 0, 187, 0, 200)
    assert _classes(pairs, "moving", 1) == (91, 0, 109, 0, 200)           # the error pass lands in another cell than the only iteration
    assert _classes(pairs, "transposed", 30) == (0, 13, 187, 0, 200)
    assert _classes(pairs, "transposed", 1) == (0, 91, 109, 0, 200)
    x, y, both, stay, ok = _classes(pairs, "subpixel", 30, EPS_TIGHT)
    assert ok == N and stay >= 100 and min(x, y, both) >= 10, (x, y, both, stay)
    best = [max(_classes(pairs, n, mc, e)[k] for n, mc, e in (("moving", 30, 0.03), ("moving", 1, 0.03), ("transposed", 30, 0.03),
                                                               ("transposed", 1, 0.03), ("subpixel", 30, EPS_TIGHT))) for k in range(4)]
    assert min(best) >= 10, best


@pytest.mark.parametrize("win,max_level,max_count", PARAMS)
def test_moving_pair_equals_the_oracle_and_the_shipped_kernel(ctx, pairs, win, max_level, max_count):
    _check(ctx, pairs, "moving", win, max_level, max_count)


@pytest.mark.parametrize("max_count", [30, 1, 0])
def test_transposed_pair_moves_the_cell_in_y(ctx_t, pairs, max_count):
    _check(ctx_t, pairs, "transposed", 31, 0, max_count)
    _check(ctx_t, pairs, "transposed", 31, 3, max_count)


def test_subpixel_pair_iterates_inside_one_cell(ctx, pairs):
    _check(ctx, pairs, "subpixel", 31, 0, 30, EPS_TIGHT)
    _check(ctx, pairs, "subpixel", 31, 3, 30, EPS_TIGHT)
    _check(ctx, pairs, "subpixel", 31, 0, 30)


def test_corner_and_edge_points_on_a_stationary_pair(ctx, pairs):
    """the window origin of (0.3, 0.2) is (-15, -15) on every level: rows kept across a level change would show"""
    p0 = pairs["stationary"][2]
    for level in range(3):
        assert (np.floor(p0[0] * np.float32(0.5 ** level) - np.float32(15)) == -15).all()
    _check(ctx, pairs, "stationary", 31, 3, 30)
    _check(ctx, pairs, "stationary", 31, 3, 0)
    assert _oracle(pairs, "stationary", 31, 3, 30)[1].any()


def test_batch_of_three_with_dead_slots_and_nan_rows():
    """different frames per sequence.  (a) the track table after sequence 1 lost 12 and sequence 2 lost 40 tracks: the count vector has dead
    slots, whose rows of the iteration table the kernel writes itself; (b) a synchronous track whose point rows hold NaNs"""
    import vo_oracle as o
    from vo_mi355x import VoContext, synthetic as syn
    B, n = 3, 90
    frames = np.stack([syn.make_sequence(3, w=W, h=H, seed=77 + 5 * b, margin=64)[0] for b in range(B)])          # [B, 3, H, W]
    seeds = np.stack([syn.grid_points(n, W, H, margin=10, seed=4 + b) for b in range(B)])
    seeds[1, :12] = (-200.0, -200.0)
    seeds[2, 20:60] = (-200.0, -200.0)
    holes = seeds.copy()
    holes[0, 3] = (np.nan, 5.0); holes[1, 40] = (np.nan, np.nan); holes[2, 7] = (60.0, np.nan)

    def run(reuse):
        with VoContext(W, H, max_pts=128, batch=B) as c:
            c.set_tuning(klt_reuse=reuse)
            c.push_frame(frames[:, 0]); c.tracks_seed(seeds, t=0)
            c.push_frame(frames[:, 1]); c.tracks_track(1)
            before = c.tracks_read()
            c.push_frame(frames[:, 2]); c.tracks_track(2)
            nb = [len(r["uv"]) for r in before]
            rows = c.points_download(max(nb), return_iters=True)
            after = c.tracks_read()
            sync = c.klt_track(holes, return_iters=True)
        return before, nb, rows, after, sync

    b1, nb, rows1, after1, sync1 = run(1)
    b0, nb0, rows0, after0, sync0 = run(-1)
    assert nb == nb0 and len(set(nb)) == B and max(nb) - min(nb) >= 20, nb          # dead slots in two of the three sequences
    for b in range(B):
        want = o.klt(frames[b, 1], frames[b, 2], b1[b]["uv"], return_iters=True)
        assert _same([rows1[k][b, :nb[b]] for k in range(4)], list(want)), b
        assert _same([rows1[k][b, :nb[b]] for k in range(4)], [rows0[k][b, :nb[b]] for k in range(4)]), b
        assert (rows1[3][b, nb[b]:] == -1).all() and (rows0[3][b, nb[b]:] == -1).all(), b
        assert _same([after1[b][k] for k in sorted(after1[b])], [after0[b][k] for k in sorted(after0[b])]), b
    assert _same(list(sync1), list(sync0))                                           # NaN rows included, bit for bit
    finite = np.isfinite(holes).all(-1)
    assert (~finite).sum() == 3
    for b in range(B):
        want = o.klt(frames[b, 1], frames[b, 2], holes[b][finite[b]], return_iters=True)
        assert _same([sync1[k][b][finite[b]] for k in range(4)], list(want)), b
        # the NaN rows too: outside at every level (cvFloor(NaN) = INT_MIN), so status 0, err 0 and no level entered -- on both kernels
        full = o.klt(frames[b, 1], frames[b, 2], holes[b], return_iters=True)
        for got in (sync1, sync0):
            assert _same([got[k][b] for k in (1, 2, 3)], [full[k] for k in (1, 2, 3)]), b
        assert (full[1][~finite[b]] == 0).all() and (full[3][~finite[b]] == -1).all(), b


def test_fused_step_two_in_flight_is_identical_with_either_kernel():
    from vo_mi355x import VoContext, synthetic as syn
    B, w, h, n = 3, 256, 160, 150
    seqs = np.stack([syn.make_sequence(4, w=w, h=h, seed=40 + b, margin=48)[0] for b in range(B)])
    pts = np.stack([syn.grid_points(n, w, h, seed=9 + b) for b in range(B)])

    def run(reuse):
        with VoContext(w, h, max_pts=512, batch=B) as c:
            c.set_tuning(klt_reuse=reuse)
            c.upload_sequence(seqs); c.points_upload(pts); c.push_frame_resident(0)
            out = []
            c.frame_step_resident(1, n, do_dlt=False, do_ba=False, do_st=True)
            c.frame_step_resident(2, n, do_dlt=False, do_ba=False, do_st=True)         # two steps in flight
            out.append(c.frame_fetch())
            c.frame_step_resident(3, n, do_dlt=False, do_ba=False, do_st=True)
            out += [c.frame_fetch(), c.frame_fetch()]
            return out

    new, old = run(1), run(-1)
    assert len(new) == len(old) == 3
    for t, (x, y) in enumerate(zip(new, old)):
        assert set(x) == set(y) and {"points2d", "status", "err", "corners"} <= set(x)
        for k in x:
            if isinstance(x[k], np.ndarray):
                assert x[k].shape == y[k].shape and np.array_equal(_bits(x[k]), _bits(y[k])), (t, k)
            elif isinstance(x[k], (list, tuple)) and len(x[k]) and isinstance(x[k][0], np.ndarray):
                assert _same(list(x[k]), list(y[k])), (t, k)
            else:
                assert x[k] == y[k], (t, k)
        assert x["status"].any()


def test_closed_loop_is_identical_with_either_kernel():
    """vo_pipe_step, four frames of the small sway scene: records and tables"""
    from vo_mi355x import VoContext, synthetic as syn
    from vo_mi355x.resident import ResidentPipeline
    w, h, t1 = 256, 160, 3
    sc = syn.sway_scene(t1 + 5, w=w, h=h, f=260.0, seed=2024, pose_fn=lambda t: syn.sway_pose(t, period=24.0))
    with VoContext(w, h, max_pts=1024) as boot:
        state, t_loader = syn.gt_bootstrap(boot, sc, 0, t1)
    assert t_loader == t1

    def run(reuse):
        with VoContext(w, h, max_pts=1024) as c:
            c.set_tuning(klt_reuse=reuse)
            rp = ResidentPipeline(c, sc["K"], ba_max_iters=12, pnp_blind_batches=8)
            rp.seed(copy.deepcopy(state), [], [], 1)
            c.upload_sequence(sc["frames"])
            c.push_frame_resident(t1)
            recs = []
            for s in range(4):
                rp.step(t1 + 1 + s)
                recs.append(rp.fetch())
            return recs, rp.read_tables()

    ra, Ta = run(1)
    rb, Tb = run(-1)
    assert all(r["status"] == 0 for r in ra) and all(r["n_tracked"] > 50 for r in ra)
    for s, (x, y) in enumerate(zip(ra, rb)):
        assert set(x) == set(y)
        for k, v in x.items():
            assert (np.array_equal(y[k], v, equal_nan=v.dtype.kind == "f") if isinstance(v, np.ndarray) else y[k] == v), (s, k)
    assert set(Ta) == set(Tb)
    for name in Ta:
        assert np.array_equal(Ta[name], Tb[name], equal_nan=Ta[name].dtype.kind == "f"), name
