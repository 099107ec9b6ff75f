"""Inputs and expected outputs of the one-sequence-per-XCD block mapping at batches of 16 and 24 -- TEST INFRASTRUCTURE, holds no test.

With batch % 8 == 0 the per-image kernels take their (block, sequence) pair from vo_xcd_assign (csrc/vo_internal.h) and the tracker's five
hand-written copies of it: sequence (id & 7) + 8 * (q / nblk).  Batch 16 is the smallest at which the 8 * (q / nblk) term is not zero, 24
has three groups and is no power of two.  tests/test_gpu_xcd_map.py runs every remapped kernel on the cases below; tests/test_xcd_cases.py
shows on the references alone that a swap of two sequences along the stride of 8, or of two neighbours, is visible in every assertion.

One pool of NSEQ = 24 sequences, every one different; a batch of B uses the first B, so sequence b is the same sequence in both batches.
Everything expected comes from the CPU references the suite already trusts -- vo_oracle, clahe_model, undistort_model, subpix_model,
klt_seed_model, tracks_model's forward-backward rule -- computed once per call (lru_cache) and handed out read-only."""
import functools

import numpy as np

import clahe_model as cm
import klt_seed_model as km
import subpix_model as sm
import undistort_model as um
import vo_oracle as o
from tracks_model import fb_np, oracle_fb
from vo_mi355x import synthetic as syn

NSEQ = 24
BATCHES = (16, 24)
N_FRAMES = 3
# (w, h, win) of the frame chain: 130 x 81 has several blocks per sequence on both of its levels; 47 x 33 with a window of 7 (tiny list of
# tests/test_gpu_sizes.py) keeps three levels, the coarsest (12 x 9) a single block
FRAME_SIZES = ((130, 81, 31), (47, 33, 7))
TRACK_SIZE = (130, 81)                      # tracker, cornerSubPix, ingest stages, the fused step
ST_SIZES = ((257, 129), (130, 81))          # 257 x 129: the Shi-Tomasi pass's bands
NS = (1, 5, 150)                            # keypoints per sequence: the tracker has one block per keypoint, cornerSubPix one per four
FB_MAX_ERR = 0.5
ST_PARAMS = dict(max_corners=300, quality_level=0.02, min_distance=4.0, block_size=15)
ST_RADIUS = 5
ST_POINTS = 40
UND_DIST = (-0.12, 0.03, 0.001, -0.0008, 0.002)
CLAHE_CLIP = 2.0
INGEST = ("undistort", "clahe_1x1", "clahe_4x3", "bilateral", "undistort_clahe")
CLAHE_TILES = {"clahe_1x1": (1, 1), "clahe_4x3": (4, 3), "undistort_clahe": (4, 3)}


def _frozen(a):
    a.setflags(write=False)
    return a


def cam(w, h):
    """a camera for a w x h image: principal point off centre, fx != fy"""
    return (0.8 * w, 0.78 * w, 0.49 * w + 0.3, 0.51 * h - 0.3)


# ---- images ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def frames(w, h):
    """uint8 [NSEQ, N_FRAMES, h, w]: a texture of its own per sequence, moving from frame to frame"""
    margin = 40 if min(w, h) > 64 else 24
    return _frozen(np.stack([syn.make_sequence(N_FRAMES, w=w, h=h, seed=9000 + 37 * b + w, margin=margin)[0] for b in range(NSEQ)]))


def store_of(img, win=31):
    """what the frame store holds of an image: (levels, Scharr planes)"""
    lv = o.build_pyramid(img, win=win)
    return [_frozen(l) for l in lv], [_frozen(o.scharr(l)) for l in lv]


@functools.lru_cache(maxsize=None)
def stores(w, h, win, t):
    """frame t of every sequence in the frame store: [NSEQ] of (levels, Scharr planes)"""
    return [store_of(frames(w, h)[b, t], win) for b in range(NSEQ)]


@functools.lru_cache(maxsize=None)
def ingest(stage, t):
    """frame t of every TRACK_SIZE sequence behind an ingest stage: uint8 [NSEQ, h, w]"""
    w, h = TRACK_SIZE
    fr = frames(w, h)[:, t]
    tab = um.table(w, h, cam(w, h), UND_DIST) if stage.startswith("undistort") else None
    out = []
    for img in fr:
        if tab is not None:
            img = um.remap(img, tab)
        if stage in CLAHE_TILES:
            img = cm.clahe(img, CLAHE_CLIP, CLAHE_TILES[stage])
        if stage == "bilateral":
            img = o.bilateral(img)
        out.append(img)
    return _frozen(np.stack(out))


@functools.lru_cache(maxsize=None)
def clahe_luts(stage, t):
    """the tables of a CLAHE stage on frame t: uint8 [NSEQ, tiles_y, tiles_x, 256]"""
    w, h = TRACK_SIZE
    src = ingest("undistort", t) if stage == "undistort_clahe" else frames(w, h)[:, t]
    return _frozen(np.stack([cm.luts(img, CLAHE_CLIP, CLAHE_TILES[stage]) for img in src]))


# ---- keypoints ---------------------------------------------------------------------------------------------------------------------------
def live(n, b):
    """live rows of sequence b in a set of n: unequal over the batch, n itself at b = 0; the rest of a set is NaN rows"""
    return {1: 1, 5: 5 - b % 3, 150: 150 - 9 * (b % 5)}[n]


@functools.lru_cache(maxsize=None)
def keypoints(n):
    """float32 [NSEQ, n, 2] on TRACK_SIZE, a set of its own per sequence.  n = 150 also holds rows on the image's corners and outside it"""
    w, h = TRACK_SIZE
    p = np.full((NSEQ, n, 2), np.nan, np.float32)
    for b in range(NSEQ):
        pool = syn.grid_points(150, w, h, margin=12, seed=100 + b)
        if n == 150:
            rows = pool.copy()
            rows[10] = (0.25 * b, 0.0); rows[11] = (w - 1.0, h - 1.0 - 0.125 * b); rows[12] = (-40.0 - b, 10.0)
        else:
            rows = pool[(13 * b + 31 * np.arange(n)) % 150]
        k = live(n, b)
        p[b, :k] = rows[:k]
    return _frozen(p)


@functools.lru_cache(maxsize=None)
def guesses(n):
    """start positions of the seeded forms: a flow of its own per sequence; NaN on dead rows, and on one live row where n allows it (a
    guess that is not finite starts from p0)"""
    p = keypoints(n)
    g = p.copy()
    for b in range(NSEQ):
        g[b] += np.float32((1.5 + 0.5 * (b % 4), -1.0 + 0.25 * (b % 7)))
        if n >= 5:
            g[b, 2] = (np.nan, 5.0)
        if n == 150:
            g[b, 20] = (np.inf, 5.0); g[b, 21] = (1.0e30, -1.0e30)
    return _frozen(g)


def _pair(b):
    fr = frames(*TRACK_SIZE)
    return fr[b, 0], fr[b, 1]


def _fb(b, p0, fwd):
    """the backward pass (unseeded, from the forward result) and the reference's check"""
    im0, im1 = _pair(b)
    p0r = o.klt(im1, im0, fwd[0])[0]
    e, ok = fb_np(p0, p0r, FB_MAX_ERR)
    return dict(p1=fwd[0], status=fwd[1], err=fwd[2], iters=fwd[3], p0r=p0r, fb_err=e, ok=ok)


@functools.lru_cache(maxsize=None)
def tracked(form, n):
    """[NSEQ] of dicts: p1, status, err, iters, and p0r, fb_err, ok with the forward-backward check.
    form: "plain" (vo_oracle.klt), "fb" (tracks_model.oracle_fb), "seeded" (klt_seed_model.klt_np), "fb_seeded" """
    out = []
    for b in range(NSEQ):
        im0, im1 = _pair(b)
        p0 = keypoints(n)[b]
        if form in ("plain", "fb"):
            fwd = o.klt(im0, im1, p0, return_iters=True)
        else:
            fwd = km.klt_np(im0, im1, p0, init=guesses(n)[b])
        if form == "plain" or form == "seeded":
            r = dict(p1=fwd[0], status=fwd[1], err=fwd[2], iters=fwd[3])
        else:
            r = _fb(b, p0, fwd)
            if form == "fb":
                q1, qs, qe, r0 = oracle_fb(im0, im1, p0)
                assert np.array_equal(q1, r["p1"], equal_nan=True) and np.array_equal(r0, r["p0r"], equal_nan=True)
        out.append({k: _frozen(v) for k, v in r.items()})
    return out


FORMS = ("plain", "fb", "seeded", "fb_seeded")


# ---- Shi-Tomasi --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def st_points(w, h):
    """float32 [NSEQ, ST_POINTS, 2]: the sequence's own tracked points (frame 0 -> frame 1 of a grid of its own), the discs' centres"""
    fr = frames(w, h)
    return _frozen(np.stack([o.klt(fr[b, 0], fr[b, 1], syn.grid_points(ST_POINTS, w, h, margin=10, seed=300 + b))[0] for b in range(NSEQ)]))


@functools.lru_cache(maxsize=None)
def detected(w, h):
    """[NSEQ] of dicts: eig, mask, n_candidates, corners of frame 1 with exclusion discs at st_points"""
    out = []
    for b in range(NSEQ):
        m = np.full((h, w), 255, np.uint8)
        for x, y in np.int32(st_points(w, h)[b]):
            o.circle_mask(m, (x, y), ST_RADIUS, 0)
        corners, eig, nc = o.good_features(frames(w, h)[b, 1], m, maxCorners=ST_PARAMS["max_corners"], qualityLevel=ST_PARAMS["quality_level"],
                                           minDistance=ST_PARAMS["min_distance"], blockSize=ST_PARAMS["block_size"], return_aux=True)
        out.append(dict(eig=_frozen(eig), mask=_frozen(m), n_candidates=nc, corners=_frozen(corners)))
    return out


# ---- cornerSubPix ------------------------------------------------------------------------------------------------------------------------
def live_corners(n, b):
    """as live(), but a set of one has no corner at all in every fifth sequence: unequal counts at n = 1 too"""
    return (0 if b % 5 == 4 else 1) if n == 1 else live(n, b)


@functools.lru_cache(maxsize=None)
def corners(n):
    """float32 [NSEQ, n, 2]: integer corners of frame 1 (TRACK_SIZE), unequal counts, NaN rows behind them"""
    w, h = TRACK_SIZE
    p = np.full((NSEQ, n, 2), np.nan, np.float32)
    for b in range(NSEQ):
        found = o.good_features(frames(w, h)[b, 1], None, maxCorners=200, qualityLevel=0.001, minDistance=3, blockSize=5)
        assert len(found) >= 160
        k = live_corners(n, b)
        p[b, :k] = found[b % 7: b % 7 + k]
    return _frozen(p)


@functools.lru_cache(maxsize=None)
def refined(n):
    """[NSEQ] of (out, iters, flags) of subpix_model on corners(n), default parameters"""
    w, h = TRACK_SIZE
    return [tuple(_frozen(x) for x in sm.corner_subpix_np(frames(w, h)[b, 1], corners(n)[b])) for b in range(NSEQ)]
