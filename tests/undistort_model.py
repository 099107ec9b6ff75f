"""numpy model of the lens undistortion (csrc/vo_undistort.hip): the definition the HIP path is pinned to, bit for bit.

It restates cv2.undistort(src, K, dist, None, newK) of OpenCV 4.4: initUndistortRectifyMap (imgproc/undistort.cpp, no rectification) to a
fixed-point map, then remap(INTER_LINEAR, BORDER_CONSTANT, 0) (imgproc/imgwarp.cpp).  One float64 map evaluation, integers behind it.

    K = (fx, fy, cx, cy), newK = (fx', fy', cx', cy') (default K), dist = (k1, k2, p1, p2, k3, k4, k5, k6), shorter forms padded with zeros

  map, float64, every operation on its own (no fused multiply-add), for output pixel (j, i):
    x = (j - cx') / fx', y = (i - cy') / fy'; x2 = x x, y2 = y y, r2 = x2 + y2, _2xy = 2 x y
    kr = (1 + ((k3 r2 + k2) r2 + k1) r2) / (1 + ((k6 r2 + k5) r2 + k4) r2)
    u = fx (x kr + p1 _2xy + p2 (r2 + 2 x2)) + cx;   v = fy (y kr + p1 (r2 + 2 y2) + p2 _2xy) + cy
  quantise, per axis: q = rint(32 u), half to even.  q not finite: outside, stored origin -2, fraction 0.  Else (q clamped to +-2^30, far
    beyond any image) origin s = q >> 5, fraction f = q & 31; outside when s is not in [-2, len]; s is stored clamped to that range.
    An output pixel with either axis outside is 0.
  sample: taps (sx, sy), (sx + 1, sy), (sx, sy + 1), (sx + 1, sy + 1), a tap outside the image reads 0 (this one rule covers remap's fast,
    partly-outside and fully-outside paths); weights (32 - fx5)(32 - fy5) 32, fx5 (32 - fy5) 32, (32 - fx5) fy5 32, fx5 fy5 32 -- exact
    integers that sum to 32768, what OpenCV's bilinear table holds for 1/32 fractions; dst = (sum + 16384) >> 15.

Known deviation from a live cv2: OpenCV walks each map row with running sums (_x += ir[0]) over an LU-inverted newK instead of the closed
form above, so a 32 u within rounding noise of a tie can quantise differently there.  This project's parity is with this restatement (the
position use_harris takes in include/vo_mi355x.h); no live-cv2 comparison is made.
"""
import numpy as np


def _k4(K):
    K = np.asarray(K, np.float64)
    if K.shape == (3, 3):
        return np.array([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    assert K.shape == (4,), K.shape
    return K


def _dist8(dist):
    d = np.asarray([] if dist is None else dist, np.float64).reshape(-1)
    assert d.size in (0, 4, 5, 8), d.size
    return np.concatenate([d, np.zeros(8 - d.size)])


def map_uv(w, h, K, dist, new_K=None):
    """the float64 map: u, v [h, w]"""
    fx, fy, cx, cy = _k4(K)
    nfx, nfy, ncx, ncy = _k4(K if new_K is None else new_K)
    k1, k2, p1, p2, k3, k4, k5, k6 = _dist8(dist)
    j = np.arange(w, dtype=np.float64)[None, :]
    i = np.arange(h, dtype=np.float64)[:, None]
    x = np.broadcast_to((j - ncx) / nfx, (h, w))
    y = np.broadcast_to((i - ncy) / nfy, (h, w))
    with np.errstate(all="ignore"):
        x2 = x * x
        y2 = y * y
        r2 = x2 + y2
        _2xy = 2.0 * x * y
        kr = (1.0 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1.0 + ((k6 * r2 + k5) * r2 + k4) * r2)
        u = fx * (x * kr + p1 * _2xy + p2 * (r2 + 2.0 * x2)) + cx
        v = fy * (y * kr + p1 * (r2 + 2.0 * y2) + p2 * _2xy) + cy
    return u, v


def _quant(u, length):
    """one axis: origin (int64, clamped to [-2, length]), fraction, outside"""
    with np.errstate(all="ignore"):
        q = np.rint(u * 32.0)
    fin = np.isfinite(q)
    iq = np.clip(np.where(fin, q, 0.0), -2.0 ** 30, 2.0 ** 30).astype(np.int64)
    s, f = iq >> 5, iq & 31
    out = ~fin | (s < -2) | (s > length)
    s = np.where(fin, np.clip(s, -2, length), -2)
    f = np.where(fin, f, 0)
    return s, f, out


def table(w, h, K, dist, new_K=None):
    """the fixed-point map: dict of sxy (h, w, 2) i16, frac (h, w) u16 = fy5 * 32 + fx5, outside (h, w) u8"""
    u, v = map_uv(w, h, K, dist, new_K)
    sx, fx5, ox = _quant(u, w)
    sy, fy5, oy = _quant(v, h)
    return dict(sxy=np.stack([sx, sy], axis=-1).astype(np.int16), frac=(fy5 * 32 + fx5).astype(np.uint16), outside=(ox | oy).astype(np.uint8))


def remap(src, tab):
    """the integer sampling of a table"""
    src = np.asarray(src)
    assert src.dtype == np.uint8 and src.ndim == 2 and src.shape == tab["outside"].shape
    h, w = src.shape
    sx, sy = tab["sxy"][..., 0].astype(np.int64), tab["sxy"][..., 1].astype(np.int64)
    fx5, fy5 = (tab["frac"] & 31).astype(np.int64), (tab["frac"] >> 5).astype(np.int64)

    def tap(xx, yy):
        ok = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
        return np.where(ok, src[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64), 0)

    acc = ((32 - fx5) * (32 - fy5) * 32 * tap(sx, sy) + fx5 * (32 - fy5) * 32 * tap(sx + 1, sy) +
           (32 - fx5) * fy5 * 32 * tap(sx, sy + 1) + fx5 * fy5 * 32 * tap(sx + 1, sy + 1))
    dst = (acc + 16384) >> 15
    return np.where(tab["outside"] != 0, 0, dst).astype(np.uint8)


def undistort(src, K, dist, new_K=None):
    """cv2.undistort(src, K, dist, None, new_K) as restated above: uint8 [h, w] -> uint8 [h, w]"""
    h, w = np.asarray(src).shape
    return remap(src, table(w, h, K, dist, new_K))


def taps_inside(tab):
    """output pixels whose four taps all lie inside the image (and that are not forced to 0)"""
    h, w = tab["outside"].shape
    sx, sy = tab["sxy"][..., 0].astype(np.int64), tab["sxy"][..., 1].astype(np.int64)
    return (tab["outside"] == 0) & (sx >= 0) & (sx + 1 < w) & (sy >= 0) & (sy + 1 < h)
