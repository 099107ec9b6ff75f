"""GPU: the grow / rebuild paths of the workspaces that no other test walks.  Every assertion has one form: a call on a context whose workspace
has been built, grown or rebuilt by the calls before it returns, bit for bit, what the same call returns on a fresh context.  (The two-view
searches, the pose from a homography, the guided matcher and ORB have such tests beside their own: test_workspace_reuse_and_regrowth,
test_workspace_grows_and_is_reused, test_the_workspace_grows_then_shrinks, the ORB reserve / regrow test.)

Shapes are the smallest that take the path: a 96 x 80 context of two sequences with max_pts 32, point counts 16 -> 64 (above max_pts, which
forces the rebuild) -> 16.  No test here makes an allocation fail: that side is tests/host/vo_buf_check.hip's."""
import numpy as np
import pytest

import pnp_model as pm

pytestmark = pytest.mark.gpu
W, H, MAX_PTS, B = 96, 80, 32, 2


def _ctx(**kw):
    from vo_mi355x import VoContext
    kw.setdefault("batch", B)
    kw.setdefault("max_pts", MAX_PTS)
    return VoContext(W, H, **kw)


def _flat(x):
    """every array, number and string of a nested result, as bytes"""
    if isinstance(x, dict):
        return b"{" + b"".join(str(k).encode() + b":" + _flat(x[k]) for k in sorted(x)) + b"}"
    if isinstance(x, (list, tuple)):
        return b"[" + b",".join(_flat(v) for v in x) + b"]"
    if isinstance(x, np.ndarray):
        return str((x.dtype, x.shape)).encode() + np.ascontiguousarray(x).tobytes()
    if isinstance(x, (float, np.floating)):
        return np.float64(x).tobytes()
    return repr(x).encode()


def _frames(n, seed=11):
    """[B][n][H][W] u8: two textured sequences with a small motion"""
    from vo_mi355x import synthetic as syn
    return np.stack([np.stack(syn.make_sequence(n, w=W, h=H, seed=seed + b, margin=24)[0]) for b in range(B)])


def _walk(calls, setup=lambda c: None, **ctx_kw):
    """calls: functions of a context.  Each on a fresh context (behind `setup`), then all of them in order on one: the same bytes"""
    fresh = []
    for f in calls:
        with _ctx(**ctx_kw) as c:
            setup(c)
            fresh.append(_flat(f(c)))
    with _ctx(**ctx_kw) as c:
        setup(c)
        for k, (f, want) in enumerate(zip(calls, fresh)):
            assert _flat(f(c)) == want, "call %d differs from the same call on a fresh context" % k


def test_pnp_workspace_grows_ascending():
    def call(n):
        s = [pm.scene("general", n, seed=3 + b) for b in range(B)]
        K, X, uv = (np.stack([np.asarray(q[k]) for q in s]) for k in ("K", "X", "uv"))
        return lambda c: c.pnp_ransac(K, X, uv, seed=5)
    _walk([call(16), call(64), call(16)])                       # 16: cap = max_pts; 64: rebuilt; 16: reused


def test_sift_output_rows_grow_then_shrink():
    img = _frames(1)[:, 0]

    def call(nfeatures, max_out):
        return lambda c: c.sift_detect_compute(img, nfeatures=nfeatures, max_out=max_out)
    _walk([call(6, 24), call(40, 160), call(6, 24)])            # the row stride of the descriptor launch follows the largest max_out


def test_ba_workspace_larger_then_more_partial_sets_then_first():
    from vo_mi355x import synthetic as syn

    def call(n, lanes):
        s = [syn.make_ba_scene(n_pts=n, n_slots=4, seed=20 + b, width=W, height=H) for b in range(B)]
        K = np.stack([q["K"] for q in s])
        poses, points, obs = (np.stack([q[k] for q in s]) for k in ("poses0", "points0", "obs"))

        def f(c):
            c.set_tuning(ba_lanes=lanes)                        # 16 lanes per landmark: half the landmarks per workgroup
            return c.ba_adjust(K, poses, points, obs, c.ba_params(max_iters=6))
        return f
    # (4, 40) builds; N = 100 > cap_N rebuilds (4 partial sets); N = 90 at 16 lanes needs 6 > cap_nblk: the rule at the top of ba_alloc
    # rebuilds for a SMALLER N; (4, 40) is then served by that workspace
    _walk([call(40, 0), call(100, 0), call(90, 16), call(40, 16)])


def test_tracks_obs_with_a_growing_window():
    from vo_mi355x import synthetic as syn
    fr = _frames(3)
    pts = np.stack([syn.grid_points(16, W, H, margin=12, seed=7 + b) for b in range(B)])

    def setup(c):
        c.push_frame(fr[:, 0])
        c.tracks_seed(pts, t=0)
        for t in (1, 2):
            c.push_frame(fr[:, t])
            c.tracks_track(t)

    def call(window):
        return lambda c: c.tracks_obs(2, window)
    _walk([call(1), call(3), call(1)], setup=setup)


def test_seq_upload_twice_with_different_lengths():
    fr = _frames(4)

    def call(n):
        def f(c):
            c.upload_sequence(fr[:, :n])
            c.push_frame_resident(n - 1)
            return [c.pyramid_read(1, 0, seq=b) for b in range(B)]
        return f
    _walk([call(2), call(4), call(1)])


def test_ba_upload_bank_after_a_plain_upload():
    from vo_mi355x import synthetic as syn
    s = [[syn.make_ba_scene(n_pts=24, n_slots=4, seed=40 + 2 * p + b, width=W, height=H) for b in range(B)] for p in range(2)]
    K = np.stack([s[0][b]["K"] for b in range(B)])
    bank = {k: np.stack([np.stack([q[k] for q in row]) for row in s]) for k in ("poses0", "points0", "obs")}

    def plain(c):
        c.ba_upload(K, bank["poses0"][0], bank["points0"][0], bank["obs"][0])
        return c.ba_fetch_after(c.ba_solve_resident, c.ba_params(max_iters=6))

    def banked(c):
        c.ba_upload_bank(K, bank["poses0"], bank["points0"], bank["obs"])
        out = []
        for k in (1, 0):
            c.ba_select(k)
            out.append(c.ba_fetch_after(c.ba_solve_resident, c.ba_params(max_iters=6)))
        return out
    _walk([plain, banked, plain])


def test_pipe_create_twice_on_one_context():
    """a second vo_pipe_create replaces the first pipeline's tables: the closed loop then runs as on a context that had none"""
    from vo_mi355x import VoContext, synthetic as syn
    from vo_mi355x.resident import ResidentPipeline
    w, h = 160, 96
    sc = syn.sway_scene(6, w=w, h=h, f=170.0, seed=2024, pose_fn=lambda t: syn.sway_pose(t, period=24.0), margin=48)
    with VoContext(w, h, max_pts=512) as c0:
        state, t1 = syn.gt_bootstrap(c0, sc, 0, 3)

    def run(c, creates):
        for k in range(creates):
            rp = ResidentPipeline(c, sc["K"], ba_window=3 + (creates - 1 - k), ba_max_iters=8, pnp_blind_batches=4)
        rp.seed(state, [], [], 1)
        c.push_frame(sc["frames"][t1])
        out = []
        for k in range(2):
            c.push_frame(sc["frames"][t1 + 1 + k])
            rp.step()
            out.append(bytes(rp.fetch_raw()))
        out.append(rp.read_tables())
        return out
    with VoContext(w, h, max_pts=512) as c:
        want = _flat(run(c, 1))
    with VoContext(w, h, max_pts=512) as c:
        assert _flat(run(c, 2)) == want
