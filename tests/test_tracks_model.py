"""CPU: the list model of the track table (tests/tracks_model.py) against the reference's own bookkeeping -- golden G3, tests/golden/glue_s0.npz:
extend_tracks x2 + extract run unmodified on the CPU oracle -- so that the GPU tests of tests/test_gpu_tracks_chunks.py compare the kernels
with a model that was itself checked.  Needs no GPU and no reference checkout."""
import os

import numpy as np

import tracks_model as tm

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _hist(g, pre):
    ln = g[pre + "_hist_len"]
    h, o = [], 0
    for n in ln:
        h.append(g[pre + "_hist"][o:o + n]); o += n
    return h


def _same_as_golden(m, g, pre, pos_of_tag, frames_of_hist):
    """the model's list = the golden Keypoint list `pre`: every column, the whole history, identities through in0_tag"""
    tb = m.table()
    assert np.array_equal(tb["tag"], [pos_of_tag[float(t)] for t in g[pre + "_tag"]])
    assert np.array_equal(tb["uv"].astype(np.float64), g[pre + "_uv"]) and np.array_equal(tb["uv_first"].astype(np.float64), g[pre + "_uv_first"])
    assert np.array_equal(tb["t_first"], g[pre + "_t_first"]) and np.array_equal(tb["t_total"], g[pre + "_t_total"])
    hist = _hist(g, pre)
    assert len(hist) == len(m.tr)
    for k, hh in zip(m.tr, hist):
        assert sorted(k["hist"]) == frames_of_hist and len(hh) == len(frames_of_hist)
        for tau, want in zip(frames_of_hist, hh):
            assert np.array_equal(k["hist"][tau].astype(np.float64), want)


def test_model_replays_the_reference_glue_golden():
    g = np.load(os.path.join(GOLD, "glue_s0.npz"))
    frames = g["frames"]
    h, w = frames[0].shape
    in_uv = g["in0_uv"].astype(np.float32)
    assert np.array_equal(in_uv.astype(np.float64), g["in0_uv"])                    # the golden inputs are float32 values
    pos_of_tag = {float(t): i for i, t in enumerate(g["in0_tag"])}
    m = tm.TrackModel(w, h)
    m.seed(in_uv, t=1)                                                              # extract(..., t=1) + the injected border tracks
    assert len(m) == 268 and m.next_tag == 268

    dead = m.track(frames[0], frames[1], 2)                                         # extend_tracks(frames[1], ...)
    _same_as_golden(m, g, "tr1", pos_of_tag, [1, 2])
    alive = {pos_of_tag[float(t)] for t in g["tr1_tag"]}
    assert dead == [i for i in range(268) if i not in alive] and len(dead) == 268 - 261     # the dead set, in list order
    obs = m.obs(2, 3, 300)
    for i, hh in enumerate(_hist(g, "tr1")):                                        # uv_history = [uv(t=1), uv(t=2)]
        assert np.array_equal(obs[0, i], hh[1]) and np.array_equal(obs[1, i], hh[0]) and np.isnan(obs[2, i]).all()
    assert np.isnan(obs[:, 261:]).all()

    before = [k["tag"] for k in m.tr]
    dead = m.track(frames[1], frames[2], 3)                                         # extend_tracks(frames[2], ...)
    _same_as_golden(m, g, "tr2", pos_of_tag, [1, 2, 3])
    alive = {pos_of_tag[float(t)] for t in g["tr2_tag"]}
    assert dead == [i for i in before if i not in alive] and len(dead) == 261 - 255

    found, added = m.detect(frames[2], 3, 7, dict(max_corners=1000, quality_level=0.03, min_distance=7, block_size=31), 1000, 512)
    assert found == added == len(g["ex2_uv"]) == 26                                 # extract(frames[2], 3, c2, 'shi-tomasi', 7)
    tb = m.table()
    new = slice(255, None)
    assert np.array_equal(tb["uv"][new].astype(np.float64), g["ex2_uv"]) and np.array_equal(tb["uv_first"][new].astype(np.float64), g["ex2_uv_first"])
    assert np.array_equal(tb["t_first"][new], g["ex2_t_first"]) and np.array_equal(tb["t_total"][new], g["ex2_t_total"])
    assert np.array_equal(tb["tag"][new], 268 + np.arange(26)) and m.next_tag == 268 + 26
    for k, hh in zip(m.tr[255:], _hist(g, "ex2")):
        assert list(k["hist"]) == [3] and len(hh) == 1 and np.array_equal(k["hist"][3].astype(np.float64), hh[0])
    assert np.array_equal(m.table()["uv"][:255].astype(np.float64), g["tr2_uv"])    # the survivors are untouched by the append


def test_model_clamps_guess_and_obs_on_a_hand_made_list():
    """the rules the golden does not reach: the max_new / capacity clamps of the append, the predictor's rule and its NaN tail, the NaN
    layout of obs -- on a list small enough to state the expected values by hand"""
    g = np.load(os.path.join(GOLD, "glue_s0.npz"))
    frames = g["frames"]
    h, w = frames[0].shape
    st = dict(max_corners=1000, quality_level=0.03, min_distance=7, block_size=31)
    m = tm.TrackModel(w, h)
    m.seed(np.array([[50, 60], [-100, -100], [120.5, 90.25]], np.float32), t=30)
    assert m.track(frames[0], frames[1], 31) == [1]                                 # the planted seed dies, the others stay
    assert [k["tag"] for k in m.tr] == [0, 2] and [k["tt"] for k in m.tr] == [2, 2]
    assert m.detect(frames[1], 31, 7, st, 0, 512)[1] == 0 and len(m) == 2 and m.next_tag == 3       # max_new = 0 appends nothing
    found, added = m.detect(frames[1], 31, 7, st, 5, 512)
    assert found > 5 and added == 5 and [k["tag"] for k in m.tr[2:]] == [3, 4, 5, 6, 7] and m.next_tag == 8
    found, added = m.detect(frames[1], 31, 7, st, 1000, 9)
    assert found > 2 and added == 2 and len(m) == 9 and m.next_tag == 10            # cut by cap - n
    assert m.detect(frames[1], 31, 7, st, 1000, 9)[1] == 0                          # a full list takes nothing
    # the predictor for the tracking to frame 32: the two seeds have an entry at frame 30, the tracks born at 31 have none
    gs = m.guess(32, 12)
    uv = m.points()
    for i in (0, 1):
        want = uv[i] + (uv[i] - m.tr[i]["hist"][30])
        assert gs[i].dtype == np.float32 and np.array_equal(gs[i], want)
    assert np.array_equal(gs[2:9], uv[2:]) and np.isnan(gs[9:]).all() and gs.shape == (12, 2)
    m.tr[0]["hist"][30] = np.array([np.inf, 1.0], np.float32)
    assert np.array_equal(m.guess(32)[0], uv[0])                                    # a history entry that is not finite: start at uv
    # obs: slot s <-> frame t_now - s, NaN before the birth and beyond the list
    ob = m.obs(31, 4, 11)
    assert ob.shape == (4, 11, 2) and ob.dtype == np.float64
    assert np.array_equal(ob[0, :9], uv.astype(np.float64)) and np.array_equal(ob[1, 1], [120.5, 90.25])
    assert np.isnan(ob[1, 2:]).all() and np.isnan(ob[2:]).all() and np.isnan(ob[:, 9:]).all()


def test_model_forward_backward_rule_is_inside_and_good():
    """keep = inside AND fb_err < thr with the oracle's two passes; flags are in the order of the list before the track"""
    import vo_oracle as o
    g = np.load(os.path.join(GOLD, "glue_s0.npz"))
    frames = g["frames"]
    h, w = frames[0].shape
    cur = tm.occlude(frames[1], 90, 60, 48, seed=11)
    p0 = g["in0_uv"].astype(np.float32)
    m = tm.TrackModel(w, h)
    m.seed(p0, t=0)
    dead = m.track(frames[0], cur, 1, fb_thr=0.75)
    q1, _, _, r0 = tm.oracle_fb(frames[0], cur, p0)
    e = np.abs(p0 - r0).max(-1)
    good = e < np.float32(0.75)
    inside = (q1[:, 0] >= 0) & (q1[:, 0] <= w) & (q1[:, 1] >= 0) & (q1[:, 1] <= h)
    assert np.array_equal(m.fb_ok, good) and np.array_equal(m.fb_err, e, equal_nan=True)
    assert dead == np.nonzero(~(inside & good))[0].tolist() and (inside & ~good).any() and (~inside).any()
    assert np.array_equal(m.table()["uv"], q1[inside & good])
    m.track(cur, frames[2], 2)                                                      # without a threshold the flags are gone
    assert m.fb_ok is None
