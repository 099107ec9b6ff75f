"""The definition of the multi-scale ORB detector (csrc/vo_orb.hip, include/vo_mi355x.h: vo_orb_*), in numpy.  Neither OpenCV nor its learned
sampling table is part of this project, so this model -- not cv2.ORB -- is what the kernels are pinned to, bit for bit; everything below is
integer arithmetic or single IEEE operations in a fixed order.  The FAST score and its 3 x 3 maxima are fast_model's, the orientation, the blur
and the steered tests are brief_model's: they are used, not restated.

  geometry   float64 on the host: s_l = scale_factor ** l, w_l = rint(w / s_l), h_l = rint(h / s_l) (half to even); the reported scale is f32(s_l).
             A level with w_l < 1 or h_l < 1 has no pixels (and so has every level above it).
  quotas     OpenCV's rule in float64: f = 1 / scale_factor, nd = nfeatures * (1 - f) / (1 - f ** nlevels); levels 0 .. nlevels-2 get rint(nd),
             nd *= f after each; the last level gets max(nfeatures - sum, 0).  nlevels = 1: the single level gets nfeatures.
  pyramid    level 0 is the image; level l is resized from level l-1 by fixed-point bilinear interpolation.  Per axis, destination d samples the
             source at fx = (d + 0.5) * (src / dst) - 0.5 (float64), i0 = floor(fx), a = rint((fx - i0) * 2048); both taps i0, i0 + 1 are clamped to
             [0, src-1]; pixel = (sum of the four products of the (2048-a, a) weights + 2^21) >> 22.
  candidates strict 3 x 3 maxima of fast_model.score_map(level, fast_threshold) with 31 <= lx < w_l-31 and 31 <= ly < h_l-31 and, under a mask,
             mask[min(h-1, rint(f32(ly) * f32(s_l)))][min(w-1, rint(f32(lx) * f32(s_l)))] != 0.
  retention  (retainBest, ties kept; both rules define a set) keep i iff fewer than 2 * quota_l candidates have a strictly greater FAST score; then
             the Harris response of those; keep i iff fewer than quota_l of them have a strictly greater response.
  Harris     over the 7 x 7 block centred on the keypoint: Ix = 2 (I(x+1,y) - I(x-1,y)) + (I(x+1,y-1) - I(x-1,y-1)) + (I(x+1,y+1) - I(x-1,y+1)), Iy its
             transpose; a = sum Ix^2, b = sum Iy^2, c = sum Ix Iy in int32; in float32, every operation rounded on its own,
                 response = ((f32(a) * f32(b) - f32(c) * f32(c)) - (0.04f * (f32(a) + f32(b))) * (f32(a) + f32(b))) * sc4,
             sc4 = f32((1 / (4 * 7 * 255)) ** 4) (float64, rounded once).
  output     by level ascending, response descending, ly ascending, lx ascending; x = f32(lx) * f32(s_l), y = f32(ly) * f32(s_l), size = 31.0f * f32(s_l);
             angle and descriptor: brief_model on the level image at (lx, ly)."""
import math

import numpy as np

import brief_model as bm
import fast_model as fm

EDGE = 31
HARRIS_K = np.float32(0.04)
SC4 = np.float32((1.0 / (4 * 7 * 255)) ** 4)
MAX_LEVELS = 8

KP_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4"), ("lx", "<i4"),
                     ("ly", "<i4")])
assert KP_DTYPE.itemsize == 32


def check_params(nfeatures, scale_factor, nlevels, fast_threshold):
    return nfeatures >= 1 and 1.0 < scale_factor <= 2.0 and 1 <= nlevels <= MAX_LEVELS and 1 <= fast_threshold <= 254


def level_geometry(w, h, scale_factor, nlevels):
    """-> w_l, h_l (int lists), scale_l (float32 array)"""
    s = [math.pow(float(scale_factor), float(l)) for l in range(nlevels)]
    wl = [max(int(np.rint(w / sl)), 0) for sl in s]
    hl = [max(int(np.rint(h / sl)), 0) for sl in s]
    for l in range(nlevels):
        if wl[l] < 1 or hl[l] < 1 or (l > 0 and wl[l - 1] == 0):
            wl[l] = hl[l] = 0
    return wl, hl, np.asarray(s, np.float64).astype(np.float32)


def quotas(nfeatures, scale_factor, nlevels):
    if nlevels == 1:
        return [int(nfeatures)]
    f = 1.0 / float(scale_factor)
    nd = nfeatures * (1.0 - f) / (1.0 - math.pow(f, float(nlevels)))
    q, total = [], 0
    for _ in range(nlevels - 1):
        q.append(int(np.rint(nd)))
        total += q[-1]
        nd *= f
    q.append(max(int(nfeatures) - total, 0))
    return q


def resize_table(src, dst):
    """-> (t0, t1, a): the two clamped taps and the weight of the second, int64 [dst]"""
    d = np.arange(dst, dtype=np.float64)
    fx = (d + 0.5) * (float(src) / float(dst)) - 0.5
    i0 = np.floor(fx)
    a = np.rint((fx - i0) * 2048.0).astype(np.int64)
    i0 = i0.astype(np.int64)
    return np.clip(i0, 0, src - 1), np.clip(i0 + 1, 0, src - 1), a


def resize(img, dw, dh):
    img = np.asarray(img, np.uint8)
    sh, sw = img.shape
    if dw < 1 or dh < 1:
        return np.zeros((max(dh, 0), max(dw, 0)), np.uint8)
    x0, x1, ax = resize_table(sw, dw)
    y0, y1, ay = resize_table(sh, dh)
    I = img.astype(np.int64)
    top = (2048 - ax)[None, :] * I[y0][:, x0] + ax[None, :] * I[y0][:, x1]
    bot = (2048 - ax)[None, :] * I[y1][:, x0] + ax[None, :] * I[y1][:, x1]
    v = (2048 - ay)[:, None] * top + ay[:, None] * bot
    assert v.max(initial=0) + (1 << 21) < 2 ** 32
    return ((v + (1 << 21)) >> 22).astype(np.uint8)


def pyramid(img, scale_factor, nlevels):
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    wl, hl, _ = level_geometry(w, h, scale_factor, nlevels)
    out = [img]
    for l in range(1, nlevels):
        out.append(resize(out[-1], wl[l], hl[l]))
    return out


def harris_abc(img, x, y):
    """(a, b, c) python ints of the 7 x 7 block centred on (x, y)"""
    P = np.asarray(img, np.int64)[y - 4:y + 5, x - 4:x + 5]
    Ix = 2 * (P[1:8, 2:9] - P[1:8, 0:7]) + (P[0:7, 2:9] - P[0:7, 0:7]) + (P[2:9, 2:9] - P[2:9, 0:7])
    Iy = 2 * (P[2:9, 1:8] - P[0:7, 1:8]) + (P[2:9, 0:7] - P[0:7, 0:7]) + (P[2:9, 2:9] - P[0:7, 2:9])
    a, b, c = int((Ix * Ix).sum()), int((Iy * Iy).sum()), int((Ix * Iy).sum())
    assert max(a, b, abs(c)) < 2 ** 31
    return a, b, c


def harris_from_abc(a, b, c):
    """float32, every operation rounded on its own: ((fa * fb - fc * fc) - (0.04f * (fa + fb)) * (fa + fb)) * sc4"""
    fa, fb, fc = np.float32(a), np.float32(b), np.float32(c)
    det = np.float32(np.float32(fa * fb) - np.float32(fc * fc))
    tr = np.float32(fa + fb)
    r = np.float32(np.float32(det - np.float32(np.float32(HARRIS_K * tr) * tr)) * SC4)
    assert r.dtype == np.float32
    return r


def harris(img, x, y):
    return harris_from_abc(*harris_abc(img, x, y))


def retain(values, n):
    """keep mask: fewer than n entries are strictly greater (retainBest with its ties)"""
    v = np.asarray(values)
    if len(v) == 0:
        return np.zeros(0, bool)
    s = np.sort(v)
    greater = len(v) - np.searchsorted(s, v, side="right")
    return greater < n


def level_candidates(lvl, fast_threshold, scale32, mask, w, h):
    """-> pts int64 [n, 2] (lx, ly), scores [n] of one level image"""
    hl, wl = lvl.shape
    if min(wl, hl) < 2 * EDGE + 1:
        return np.zeros((0, 2), np.int64), np.zeros(0, np.int32)
    pts, sc = fm.cv2_keypoints(fm.score_map(lvl, fast_threshold))
    ok = (pts[:, 0] >= EDGE) & (pts[:, 0] < wl - EDGE) & (pts[:, 1] >= EDGE) & (pts[:, 1] < hl - EDGE)
    if mask is not None:
        s = np.float32(scale32)
        mx = np.minimum(np.rint(pts[:, 0].astype(np.float32) * s).astype(np.int64), w - 1)
        my = np.minimum(np.rint(pts[:, 1].astype(np.float32) * s).astype(np.int64), h - 1)
        ok &= np.asarray(mask)[my, mx] != 0
    return pts[ok], sc[ok]


def orb_np(img, mask=None, nfeatures=500, scale_factor=1.2, nlevels=8, fast_threshold=20, pattern=None):
    """-> dict(kps KP_DTYPE [n], desc u8 [n, 32], w_l, h_l, scale_l f32, quota_l, n_l (kept per level), levels (the images))"""
    assert check_params(nfeatures, scale_factor, nlevels, fast_threshold)
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape
    pat = bm.default_pattern() if pattern is None else np.asarray(pattern, np.int8).reshape(256, 4)
    wl, hl, sc = level_geometry(w, h, scale_factor, nlevels)
    q = quotas(nfeatures, scale_factor, nlevels)
    levels = pyramid(img, scale_factor, nlevels)
    rows, descs, n_l = [], [], []
    for l, lvl in enumerate(levels):
        pts, fs = level_candidates(lvl, fast_threshold, sc[l], mask, w, h)
        keep = retain(fs, 2 * q[l])
        pts = pts[keep]
        resp = np.asarray([harris(lvl, int(x), int(y)) for x, y in pts], np.float32)
        keep = retain(resp, q[l])
        pts, resp = pts[keep], resp[keep]
        order = np.lexsort((pts[:, 0], pts[:, 1], -resp.astype(np.float64))) if len(pts) else np.zeros(0, np.int64)
        pts, resp = pts[order], resp[order]
        n_l.append(len(pts))
        if len(pts):
            d, ang, fl = bm.brief_np(lvl, pts.astype(np.float32), pat)
            assert not fl.any()                  # the 31-pixel border implies the 24-pixel margin
            k = np.zeros(len(pts), KP_DTYPE)
            k["x"] = pts[:, 0].astype(np.float32) * sc[l]
            k["y"] = pts[:, 1].astype(np.float32) * sc[l]
            k["size"] = np.float32(31.0) * sc[l]
            k["angle"], k["response"], k["octave"], k["lx"], k["ly"] = ang, resp, l, pts[:, 0], pts[:, 1]
            rows.append(k)
            descs.append(d)
    kps = np.concatenate(rows) if rows else np.zeros(0, KP_DTYPE)
    desc = np.concatenate(descs) if descs else np.zeros((0, 32), np.uint8)
    return dict(kps=kps, desc=desc, w_l=wl, h_l=hl, scale_l=sc, quota_l=q, n_l=n_l, levels=levels)


def common_after_translation(ka, kb, dx, dy, wa, ha, wb, hb):
    """indices (ia, ib) of the keypoints of crop A (w x h) that must also be keypoints of crop B = A displaced by (dx, dy) (xb = xa - dx): the
    49 x 49 support (it covers FAST, its 3 x 3 neighbours, Harris and BRIEF) and the 31-pixel edge hold in both"""
    pos_b = {(int(r["lx"]), int(r["ly"])): i for i, r in enumerate(kb)}
    ia, ib = [], []
    for i, r in enumerate(ka):
        x, y = int(r["lx"]) - dx, int(r["ly"]) - dy
        if EDGE <= x < wb - EDGE and EDGE <= y < hb - EDGE:
            assert (x, y) in pos_b, (x, y)
            ia.append(i); ib.append(pos_b[(x, y)])
    return np.asarray(ia, np.int64), np.asarray(ib, np.int64)


# ---- test images ------------------------------------------------------------------------------------------------------------------------
def twin_squares(w, h, side=12, gap=40, ground=40, seed=5):
    """the same isolated textured square pasted twice on a flat ground, `gap` apart about the centre: every corner of one copy ties with its twin
    in FAST score and in Harris response (a uniform square would have no strict 3 x 3 maximum at all: its corner pixels tie with their neighbours)"""
    im = np.full((h, w), ground, np.uint8)
    sq = np.random.RandomState(seed).randint(150, 256, (side, side)).astype(np.uint8)
    y0 = h // 2 - side // 2
    for x0 in (w // 2 - gap // 2 - side // 2, w // 2 + gap // 2 - side // 2):
        im[y0:y0 + side, x0:x0 + side] = sq
    return im


def smooth_noise(w, h, seed, cell=5):
    """a random texture with structure at several scales (noise blurred by a box): corners survive a pyramid"""
    rs = np.random.RandomState(seed)
    g = rs.randint(0, 256, (h // cell + 2, w // cell + 2)).astype(np.float64)
    big = np.kron(g, np.ones((cell, cell)))[:h, :w]
    fine = rs.randint(0, 64, (h, w))
    return np.clip(0.75 * big + fine, 0, 255).astype(np.uint8)


def make_image(kind, w, h, seed=0):
    if kind == "noise":
        return bm.noise_image(w, h, seed + w * 1000 + h)
    if kind == "blocks":
        return bm.blocks_image(w, h, seed + w * 1000 + h)
    if kind == "flat":
        return bm.flat_image(w, h)
    if kind == "twin":
        return twin_squares(w, h)
    if kind == "texture":
        return smooth_noise(w, h, seed + w * 1000 + h)
    raise ValueError(kind)
