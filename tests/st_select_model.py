"""Brute-force model of the corner selection behind the response map (cv2.goodFeaturesToTrack after cornerMinEigenVal): numpy, float64
distances, NO grid and no cells -- every candidate is tested against every corner accepted before it.  TEST INFRASTRUCTURE.

    threshold   float32(float64(max of resp over mask) * quality)
    candidates  pixels of rows / columns 1 .. n-2 with v > thr, v != 0, mask set and v >= its eight neighbours (of the thresholded map)
    rank        value descending, then pixel index descending (OpenCV's greaterThanPtr)
    distance    min_distance >= 1: accept iff no accepted corner has dx^2 + dy^2 < min_distance^2; below 1: no rule
    cut-off     max_corners, 0 = all; at most 4096 (the library's output capacity)
    limit       keeps the first min(max(limit, 0), that)

Besides the corners it returns the facts the landing checks of tests/test_st_select_cases.py need (class Selection)."""
import numpy as np

OUT_CAP = 4096          # corners one launch can put out
CHUNK = 16384           # candidates the selection kernel's LDS structures hold (unlimited instance)


class Selection:
    """corners (m, 2) float32 in rank order; n_valid; cand_xy (n_valid, 2) int32 in rank order; accepted (n_scanned,) bool;
    yield_at {k * 16384: corners among the k * 16384 strongest candidates, k = 1, 2, ...} (capped by the cut-off, up to where the scan stopped);
    chunk_of (n_scanned,) the rank-ordered chunk each scanned candidate falls into when the list is consumed 16384 - accepted at a time;
    n_chunks; later_rejected_by_earlier / later_accepted: candidates of a chunk > 0 refused ONLY by corners of earlier chunks / accepted"""


def threshold(resp, mask, quality):
    m = resp[mask != 0] if mask is not None else resp.ravel()
    mx = float(m.max()) if m.size else 0.0
    return np.float32(np.float64(mx) * np.float64(quality))


def candidates(resp, mask, quality):
    """-> (values float32, pixel indices int64) in rank order"""
    resp = np.asarray(resp, np.float32)
    h, w = resp.shape
    thr = threshold(resp, mask, quality)
    te = np.where(resp > thr, resp, np.float32(0))
    c = te[1:-1, 1:-1]
    ok = c != 0
    for dy in range(3):
        for dx in range(3):
            ok &= c >= te[dy:dy + h - 2, dx:dx + w - 2]
    if mask is not None:
        ok &= np.asarray(mask)[1:-1, 1:-1] != 0
    ys, xs = np.nonzero(ok)
    idx = (ys + 1).astype(np.int64) * w + (xs + 1)
    v = c[ys, xs]
    order = np.lexsort((-idx, -v.astype(np.float64)))
    return v[order], idx[order]


def cut_off(max_corners, limit=None):
    cut = min(max_corners, OUT_CAP) if max_corners > 0 else OUT_CAP
    if limit is not None:
        cut = min(cut, max(int(limit), 0))
    return cut


def select(resp, mask, max_corners, quality, min_distance, limit=None):
    resp = np.asarray(resp, np.float32)
    h, w = resp.shape
    v, idx = candidates(resp, mask, quality)
    n = len(idx)
    xy = np.stack([idx % w, idx // w], 1).astype(np.int32)
    cut = cut_off(max_corners, limit)
    s = Selection()
    s.n_valid, s.cand_xy, s.cand_v = n, xy, v
    md2 = np.float64(min_distance) * np.float64(min_distance)
    use_dist = min_distance >= 1
    ax = np.zeros(cut + 1, np.float64); ay = np.zeros(cut + 1, np.float64); ach = np.zeros(cut + 1, np.int64)
    acc = np.zeros(n, bool); chunk_of = np.zeros(n, np.int64)
    na, chunk, chunk_end = 0, 0, CHUNK
    s.yield_at, s.later_rejected_by_earlier, s.later_accepted = {}, 0, 0
    scanned = 0
    for i in range(n):
        if na >= cut:
            break
        if i == chunk_end:                       # the next chunk: what the structures hold beside the corners accepted so far
            chunk += 1
            chunk_end = i + (CHUNK - na)
        chunk_of[i] = chunk
        scanned = i + 1
        good = True
        if use_dist and na:
            x, y = float(xy[i, 0]), float(xy[i, 1])
            near = (ax[:na] - x) ** 2 + (ay[:na] - y) ** 2 < md2
            if near.any():
                good = False
                if chunk > 0 and (ach[:na][near] < chunk).all():
                    s.later_rejected_by_earlier += 1
        if good:
            ax[na], ay[na], ach[na] = xy[i, 0], xy[i, 1], chunk
            na += 1
            acc[i] = True
            if chunk > 0:
                s.later_accepted += 1
        if (i + 1) % CHUNK == 0:
            s.yield_at[i + 1] = na
    s.accepted, s.chunk_of, s.n_scanned = acc[:scanned], chunk_of[:scanned], scanned
    s.n_chunks = (chunk + 1) if scanned else 0
    s.corners = xy[:scanned][acc[:scanned]].astype(np.float32).reshape(-1, 2)
    return s


def _offsets(min_distance, w, h):
    """integer (dx, dy) != (0, 0) inside the image with dx^2 + dy^2 <= min_distance^2, and which of them are AT the distance"""
    md2 = np.float64(min_distance) * np.float64(min_distance)
    r = int(min(np.floor(min(float(min_distance), 1e9)), max(w, h)))
    d = np.arange(-r, r + 1)
    dx, dy = np.meshgrid(d, d)
    d2 = (dx.astype(np.float64) ** 2 + dy.astype(np.float64) ** 2)
    keep = (d2 <= md2) & ((dx != 0) | (dy != 0)) & (np.abs(dx) < w) & (np.abs(dy) < h)
    return dx[keep], dy[keep], d2[keep] == md2


def _shifted(a, dx, dy, fill):
    """b[y, x] = a[y + dy, x + dx], `fill` outside"""
    h, w = a.shape
    b = np.full_like(a, fill)
    y0, y1, x0, x1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
    b[y0:y1, x0:x1] = a[y0 + dy:y1 + dy, x0 + dx:x1 + dx]
    return b


def conflicts(sel, w, h, min_distance, max_offsets=6000):
    """-> (higher (n_valid,) int: for each candidate the number of higher-ranked candidates with dx^2 + dy^2 < min_distance^2,
           exact_pairs: candidate pairs at exactly min_distance, exact_kept: such pairs with BOTH ends accepted)
    by one shifted comparison of the rank image per integer offset (exact, every pair is visited; None when there are too many offsets)"""
    if min_distance < 1:
        return np.zeros(sel.n_valid, np.int64), 0, 0
    dx, dy, at = _offsets(min_distance, w, h)
    if len(dx) > max_offsets:
        return None, None, None
    big = np.iinfo(np.int64).max
    rank = np.full((h, w), big, np.int64)
    rank[sel.cand_xy[:, 1], sel.cand_xy[:, 0]] = np.arange(sel.n_valid)
    accimg = np.zeros((h, w), bool)
    a = sel.cand_xy[:sel.n_scanned][sel.accepted]
    accimg[a[:, 1], a[:, 0]] = True
    higher = np.zeros((h, w), np.int64)
    exact_pairs = exact_kept = 0
    for ox, oy, e in zip(dx, dy, at):
        other = _shifted(rank, int(ox), int(oy), big)
        if e:
            exact_pairs += int(((other < rank) & (rank != big)).sum())
            exact_kept += int((accimg & _shifted(accimg, int(ox), int(oy), False) & (other < rank)).sum())
        else:
            higher += (other < rank) & (rank != big)
    return higher[sel.cand_xy[:, 1], sel.cand_xy[:, 0]], exact_pairs, exact_kept
