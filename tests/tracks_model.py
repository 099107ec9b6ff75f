"""Python-list model of the device-resident track table (csrc/vo_tracks.hip) -- TEST INFRASTRUCTURE, holds no test.

A restatement of the reference's `extend_tracks` and `extract` as include/vo_mi355x.h states them for vo_tracks_seed / vo_tracks_track /
vo_tracks_detect / vo_tracks_obs and the predictor of vo_set_klt_predict, on plain Python lists and numpy.  The OpenCV arithmetic comes from
the CPU oracle (vo_oracle.klt, vo_oracle.circle_mask, vo_oracle.good_features); the seeded tracker from tests/klt_seed_model.py.  The model
itself is pinned to the reference's own output (tests/golden/glue_s0.npz) by tests/test_tracks_model.py.

Per sequence: an ordered list of dict(uv, first, tf, tt, tag, hist={frame: uv}) and a `next_tag`.  The device keeps the last 32 history
entries only; the model keeps all of them, and nothing the table's calls can ask for (windows of 1..32, the predictor's frame t - 2) tells
the two apart.
"""
import numpy as np

import klt_seed_model as km


def fb_np(p0, p0r, max_err):
    """the forward-backward error and flag of the reference: max(|p0 - p0r|) over x, y in float32, good = err < max_err (NaN fails)"""
    e = np.abs(np.asarray(p0, np.float32) - np.asarray(p0r, np.float32)).reshape(-1, 2).max(-1)
    return e, e < np.float32(max_err)


def oracle_fb(im0, im1, p0, **kw):
    """-> forward p1, status, err and the backward pass p0r = LK(im1, im0, p1) of the CPU oracle"""
    import vo_oracle as o
    q1, qs, qe = o.klt(im0, im1, p0, **kw)
    r0 = o.klt(im1, im0, q1, **kw)[0]
    return q1, qs, qe, r0


def occlude(img, x0, y0, size, seed):
    """an occluder that appears in this frame only: a block of unrelated texture pasted over the scene"""
    rng = np.random.default_rng(seed)
    out = img.copy()
    blk = rng.integers(0, 256, (size // 4 + 1, size // 4 + 1)).astype(np.uint8)
    out[y0:y0 + size, x0:x0 + size] = np.kron(blk, np.ones((4, 4), np.uint8))[:size, :size]
    return out


def _oracle_klt(prev, cur, p0):
    import vo_oracle as o
    return o.klt(prev, cur, p0)[0]


def _seeded_klt(prev, cur, p0, g):
    return km.klt_np(prev, cur, p0, init=g)[0]


class TrackModel:
    """one sequence's table.  `klt(prev, cur, p0) -> p1` and `seeded_klt(prev, cur, p0, g) -> p1` may be replaced by callables of the same
    arithmetic (a memo of the oracle; a tracker that is itself pinned to klt_np): the list rules below are what this class states."""

    def __init__(self, w, h, klt=None, seeded_klt=None):
        self.w, self.h = int(w), int(h)
        self.tr, self.next_tag = [], 0
        self.klt = klt or _oracle_klt
        self.seeded_klt = seeded_klt or _seeded_klt
        self.fb_ok = None                   # flags of the last track with a finite threshold, in the order of the list before it
        self.fb_err = None

    def __len__(self):
        return len(self.tr)

    # ---- vo_tracks_seed ----
    def seed(self, pts, t):
        pts = np.asarray(pts, np.float32).reshape(-1, 2)
        self.tr = [dict(uv=p.copy(), first=p.copy(), tf=int(t), tt=1, tag=i, hist={int(t): p.copy()}) for i, p in enumerate(pts)]
        self.next_tag = len(self.tr)

    def points(self):
        return np.array([k["uv"] for k in self.tr], np.float32).reshape(-1, 2)

    # ---- the predictor of vo_set_klt_predict, for the tracking to frame t ----
    def guess(self, t, n_hi=None):
        """(n_hi, 2) float32: uv + (uv - hist[t - 2]) where that entry exists and is finite, else uv; NaN beyond the count"""
        n = len(self.tr)
        prev = np.full((n, 2), np.nan, np.float32)
        for i, k in enumerate(self.tr):
            if t - 2 in k["hist"]:
                prev[i] = k["hist"][t - 2]
        g = np.full((n if n_hi is None else int(n_hi), 2), np.nan, np.float32)
        assert len(g) >= n
        if n:
            g[:n] = km.predict(self.points(), prev)
        return g

    # ---- vo_tracks_track = extend_tracks ----
    def track(self, prev, cur, t, fb_thr=None, predict=False):
        """-> the dead tags in list order"""
        t = int(t)
        self.fb_ok = self.fb_err = None
        dead = []
        if not self.tr:
            return dead
        p0 = self.points()
        p1 = self.seeded_klt(prev, cur, p0, self.guess(t)) if predict else self.klt(prev, cur, p0)
        p1 = np.asarray(p1, np.float32).reshape(-1, 2)
        good = np.ones(len(p0), bool)
        if fb_thr is not None and np.isfinite(fb_thr):
            p0r = self.klt(cur, prev, p1)                      # the backward pass is never seeded
            self.fb_err, good = fb_np(p0, p0r, fb_thr)
            self.fb_ok = good
        keep = []
        for k, (x, y), g in zip(self.tr, p1, good):
            if 0 <= x <= self.w and 0 <= y <= self.h and g:    # ends included; NaN fails
                k["uv"] = np.array([x, y], np.float32); k["tt"] += 1; k["hist"][t] = k["uv"].copy(); keep.append(k)
            else:
                dead.append(k["tag"])
        self.tr = keep
        return dead

    # ---- vo_tracks_detect = extract(..., 'shi-tomasi') ----
    def detect(self, img, t, mask_radius, st_params, max_new, cap):
        """st_params: dict(max_corners, quality_level, min_distance, block_size).  -> (corners found, corners appended)"""
        import vo_oracle as o
        mask = np.full((self.h, self.w), 255, np.uint8)
        for k in self.tr:
            o.circle_mask(mask, tuple(np.int32(k["uv"])), mask_radius, 0)
        new = o.good_features(img, mask, maxCorners=st_params["max_corners"], qualityLevel=st_params["quality_level"],
                              minDistance=st_params["min_distance"], blockSize=st_params["block_size"])
        m = max(0, min(len(new), int(max_new), int(cap) - len(self.tr)))
        for q in new[:m]:
            q = q.astype(np.float32)
            self.tr.append(dict(uv=q.copy(), first=q.copy(), tf=int(t), tt=1, tag=self.next_tag, hist={int(t): q.copy()}))
            self.next_tag += 1
        return len(new), m

    # ---- vo_tracks_obs ----
    def obs(self, t_now, window, cap):
        """(window, cap, 2) float64, NaN = not observed: slot s <-> frame t_now - s"""
        out = np.full((int(window), int(cap), 2), np.nan)
        for i, k in enumerate(self.tr):
            for s in range(int(window)):
                if t_now - s in k["hist"]:
                    out[s, i] = k["hist"][t_now - s].astype(np.float64)
        return out

    # ---- what vo_tracks_read returns ----
    def table(self):
        n = len(self.tr)
        return dict(uv=self.points(), uv_first=np.array([k["first"] for k in self.tr], np.float32).reshape(n, 2),
                    t_first=np.array([k["tf"] for k in self.tr], np.int32), t_total=np.array([k["tt"] for k in self.tr], np.int32),
                    tag=np.array([k["tag"] for k in self.tr], np.int32))


def assert_table(got, model, dead, tag_shift=None, what=""):
    """a vo_tracks_read record = the model's table, bit for bit, and the dead tags in list order.  tag_shift(tag) maps the model's tags
    onto the device's where the device list was seeded with padding the model never saw."""
    want = model.table()
    shift = (lambda a: np.array([tag_shift(int(x)) for x in a], np.int32)) if tag_shift else (lambda a: np.asarray(a, np.int32))
    assert np.array_equal(got["tag"], shift(want["tag"])), what
    for k in ("uv", "uv_first"):
        assert got[k].dtype == np.float32 and np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (what, k)
    assert np.array_equal(got["t_first"], want["t_first"]) and np.array_equal(got["t_total"], want["t_total"]), what
    if dead is not None:
        assert np.array_equal(got["dead_tag"], shift(dead)), what
