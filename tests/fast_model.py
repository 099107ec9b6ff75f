"""The definition of the FAST-9/16 detection path (vo_st_params.fast_threshold > 0): numpy, integer arithmetic, written from the
published algorithm (Rosten & Drummond, "Machine learning for high-speed corner detection", ECCV 2006: the 9-of-16 segment test on
the radius-3 Bresenham circle) and from OpenCV's documented behaviour -- cv2.FastFeatureDetector reports as a keypoint's `response`
the largest threshold at which the pixel still passes the segment test.  No OpenCV source or binary was at hand: where a real cv2 is
importable tests/test_fast_model.py compares `cv2_keypoints` with it, otherwise parity is with this restatement (the position
use_harris, vo_set_undistort and CLAHE take).

score_map(img, t)            the response map R (int32; the library stores (float)R, exact)
candidates(R, mask, q)       what passes the quality threshold, the 3 x 3 >= test and the mask, in rank order
select(R, mask, ...)         goodFeaturesToTrack's selection behind ANY response map: threshold, NMS, rank order (value descending, then
                             pixel index DESCENDING -- FAST scores are small integers, ties are the rule), greedy min-distance grid,
                             max_corners.  A restatement of what oracle/vo_oracle.c states in C; it does not import it.
cv2_keypoints(R)             the list cv2.FastFeatureDetector_create(t, True, TYPE_9_16).detect(img) returns: strict 3 x 3 maxima, row-major
"""
import numpy as np

# ring offsets (dx, dy), k = 0 .. 15
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3))


def score_map(img, t):
    """int32 [h, w]: m - 1 where m > t on the interior (3 <= x < w - 3, 3 <= y < h - 3), 0 elsewhere; m = max over the 16 cyclic arcs of 9
    consecutive ring pixels of max(min_arc d, min_arc -d), d_k = I(ring k) - I(centre)"""
    img = np.ascontiguousarray(img, np.uint8)
    assert img.ndim == 2
    h, w = img.shape
    out = np.zeros((h, w), np.int32)
    if h < 7 or w < 7:
        return out
    I = img.astype(np.int32)
    c = I[3:h - 3, 3:w - 3]
    d = np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - c for dx, dy in RING])
    m = np.full(c.shape, -256, np.int32)
    for s in range(16):
        arc = d[[(s + j) % 16 for j in range(9)]]
        m = np.maximum(m, np.maximum(arc.min(axis=0), (-arc).min(axis=0)))
    out[3:h - 3, 3:w - 3] = np.where(m > int(t), m - 1, 0)
    return out


def threshold(R, mask, quality):
    """(float)((double)max_{mask != 0} R * quality); the maximum is 0 if nothing is unmasked (or nothing unmasked is positive)"""
    R = np.asarray(R, np.float32)
    sel = R if mask is None else R[np.asarray(mask) != 0]
    mx = float(sel.max()) if sel.size else 0.0
    mx = max(mx, 0.0)
    return np.float32(np.float64(np.float32(mx)) * np.float64(quality))


def candidates(R, mask, quality):
    """-> (values f32 [n], flat pixel indices int64 [n]) of the candidates, ordered by (R descending, y * w + x descending)"""
    R = np.asarray(R, np.float32)
    h, w = R.shape
    thr = threshold(R, mask, quality)
    if h < 3 or w < 3:
        return np.zeros(0, np.float32), np.zeros(0, np.int64)
    ctr = R[1:h - 1, 1:w - 1]
    ok = ctr > thr
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                ok &= ctr >= R[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    if mask is not None:
        ok &= np.asarray(mask)[1:h - 1, 1:w - 1] != 0
    ys, xs = np.nonzero(ok)
    idx = (ys + 1).astype(np.int64) * w + (xs + 1)
    val = R.reshape(-1)[idx]
    order = np.lexsort((-idx, -val.astype(np.float64)))
    return val[order], idx[order]


def select(R, mask, max_corners=1000, quality=0.03, min_distance=7.0):
    """-> (m, 2) float32 corners (x, y) in rank order"""
    R = np.asarray(R, np.float32)
    h, w = R.shape
    _, idx = candidates(R, mask, quality)
    out = []
    use_grid = min_distance >= 1
    if use_grid:
        cell = int(np.rint(min_distance))            # lrint: round half to even
        gw, gh = (w + cell - 1) // cell, (h + cell - 1) // cell
        grid = {}
        md2 = float(min_distance) * float(min_distance)
    for i in idx:
        y, x = int(i) // w, int(i) % w
        if use_grid:
            xc, yc = x // cell, y // cell
            good = True
            for yy in range(max(yc - 1, 0), min(yc + 1, gh - 1) + 1):
                for xx in range(max(xc - 1, 0), min(xc + 1, gw - 1) + 1):
                    for (px, py) in grid.get((xx, yy), ()):
                        dx, dy = np.float32(x) - np.float32(px), np.float32(y) - np.float32(py)
                        if float(np.float32(dx * dx) + np.float32(dy * dy)) < md2:
                            good = False
                            break
                    if not good:
                        break
                if not good:
                    break
            if not good:
                continue
            grid.setdefault((xc, yc), []).append((x, y))
        out.append((x, y))
        if max_corners > 0 and len(out) == max_corners:
            break
    return np.asarray(out, np.float32).reshape(-1, 2)


def cv2_keypoints(R):
    """-> (pts int [n, 2] (x, y), scores [n]): strict 3 x 3 maxima (R > all 8 neighbours, R > 0) in row-major order"""
    R = np.asarray(R)
    h, w = R.shape
    if h < 3 or w < 3:
        return np.zeros((0, 2), np.int64), np.zeros(0, R.dtype)
    ctr = R[1:h - 1, 1:w - 1]
    ok = ctr > 0
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if dx or dy:
                ok &= ctr > R[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    ys, xs = np.nonzero(ok)
    return np.stack([xs + 1, ys + 1], axis=1).astype(np.int64), ctr[ys, xs]


# ---- the images of the tests (seeded by w * 1000 + h) ---------------------------------------------------------------------------------
def make_image(kind, w, h):
    """one generator per shape, drawn in a fixed order (noise, narrow noise, block greys, extremes) whichever image is asked for"""
    rng = np.random.default_rng(w * 1000 + h)
    y, x = np.mgrid[0:h, 0:w]
    noise = rng.integers(0, 256, (h, w)).astype(np.uint8)
    narrow = rng.integers(100, 111, (h, w)).astype(np.uint8)
    grey = rng.integers(0, 256, ((h + 7) // 8, (w + 7) // 8)).astype(np.uint8)
    extremes = np.where(rng.random((h, w)) < 0.5, 0, 255).astype(np.uint8)
    if kind == "zeros":
        return np.zeros((h, w), np.uint8)
    if kind == "checker":
        return np.where(((x // 5) + (y // 3)) % 2 == 1, 200, 40).astype(np.uint8)
    if kind == "blocks":
        return np.ascontiguousarray(np.kron(grey, np.ones((8, 8), np.uint8))[:h, :w])
    return {"noise": noise, "narrow": narrow, "extremes": extremes}[kind]


def ring_7x7():
    """centre 0, every ring pixel 255 (the rest 128): the single interior pixel scores 254"""
    im = np.full((7, 7), 128, np.uint8)
    im[3, 3] = 0
    for dx, dy in RING:
        im[3 + dy, 3 + dx] = 255
    return im


def disc_mask(w, h, pts, radius, base=None):
    """255 (or `base`) with filled circles of 0 at np.int32(pts): the oracle's midpoint circle (cv2.circle, thickness -1)"""
    import vo_oracle as o
    mask = np.full((h, w), 255, np.uint8) if base is None else np.ascontiguousarray(base, np.uint8).copy()
    for px, py in np.asarray(pts, np.float32).reshape(-1, 2):
        o.circle_mask(mask, (int(np.int32(px)), int(np.int32(py))), int(radius), 0)
    return mask
