"""The definition of the oriented BRIEF descriptor (csrc/vo_brief.hip, include/vo_mi355x.h: vo_brief_*) and of the Hamming 2-NN matcher
(vo_match_hamming_knn2), in numpy.  OpenCV's learned ORB table is not part of this project, so this model -- not cv2.ORB -- is what the
kernels are pinned to, bit for bit; everything below is integer arithmetic or IEEE operations in a fixed order.

Per corner, at the integer pixel (x, y) = (rint(cx), rint(cy)) (half to even, in float32) of the image:
  margin  M = 24 = 21 (furthest rotated sample) + 3 (blur).  Described iff M <= x <= w-1-M and M <= y <= h-1-M; else flags = 1, 32 zero bytes,
          angle 0.  A row that is not finite: flags = 2 and the same zeros.
  angle   ORB's IC_Angle on the raw image: m10 = sum u I(x+u, y+v), m01 = sum v I(x+u, y+v) over |v| <= 15, |u| <= UMAX[|v|] (int32, exact).
          Both 0: c = 1, s = 0, angle = 0.  Else in float64 r = sqrt(m10*m10 + m01*m01), c = f32(m10 / r), s = f32(m01 / r);
          angle = atan2(m01, m10) in degrees in [0, 360) as float32 (reported only: it never enters the descriptor).
  blur    separable 7-tap integer Gaussian G (sum 256): horizontal sums (<= 65280: u16), vertical pass over them, S = (v + 32768) >> 16.
  tests   pattern rows (x1, y1, x2, y2) int8 in [-15, 15]; per point in float32, every operation rounded on its own: fx = x1*c - y1*s,
          fy = x1*s + y1*c, ix = rint(fx), iy = rint(fy) (half to even); bit i = S(x+ix1, y+iy1) < S(x+ix2, y+iy2) in byte i // 8 at bit i % 8.
The default pattern is tools/gen_brief_pattern.py's."""
import os
import sys

import numpy as np

M = 24
UMAX = np.array([15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3], np.int32)
G = np.array([18, 33, 49, 56, 49, 33, 18], np.int64)
INT32_MAX = 2 ** 31 - 1

_v, _u = np.mgrid[-15:16, -15:16]
DISC = np.abs(_u) <= UMAX[np.abs(_v)]                      # [31][31] by (v, u)
_U, _V = _u[DISC].astype(np.int64), _v[DISC].astype(np.int64)


def default_pattern():
    """(256, 4) int8: the generator's table"""
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import gen_brief_pattern
    return gen_brief_pattern.pattern()


def blur(img):
    """S of every pixel whose 7 x 7 support lies inside the image: [h - 6][w - 6] u8, S[i][j] belongs to pixel (j + 3, i + 3)"""
    I = np.asarray(img, np.int64)
    h, w = I.shape
    hs = sum(G[k] * I[:, k:w - 6 + k] for k in range(7))
    assert hs.max(initial=0) <= 65535
    v = sum(G[k] * hs[k:h - 6 + k, :] for k in range(7))
    return ((v + 32768) >> 16).astype(np.uint8)


def moments(img, x, y):
    """(m10, m01) of the disc around the integer pixel (x, y), python ints"""
    P = np.asarray(img, np.int64)[y - 15:y + 16, x - 15:x + 16][DISC]
    return int((_U * P).sum()), int((_V * P).sum())


def orientation(m10, m01):
    """-> (c, s) float32, angle float32 in [0, 360)"""
    if m10 == 0 and m01 == 0:
        return np.float32(1), np.float32(0), np.float32(0)
    dx, dy = np.float64(m10), np.float64(m01)
    r = np.sqrt(dx * dx + dy * dy)
    c, s = np.float32(dx / r), np.float32(dy / r)
    a = np.arctan2(dy, dx) * (180.0 / np.pi)
    if a < 0.0:
        a = a + 360.0
    a = np.float32(a)
    if a >= np.float32(360):
        a = np.float32(0)
    return c, s, a


def steer(pattern, c, s):
    """the rotated integer sample offsets (ix1, iy1, ix2, iy2), each (256,) int32"""
    p = np.asarray(pattern, np.int8).reshape(256, 4).astype(np.float32)
    c, s = np.float32(c), np.float32(s)
    out = []
    for k in (0, 2):
        px, py = p[:, k], p[:, k + 1]
        fx = (px * c).astype(np.float32) - (py * s).astype(np.float32)
        fy = (px * s).astype(np.float32) + (py * c).astype(np.float32)
        assert fx.dtype == np.float32 and fy.dtype == np.float32
        out += [np.rint(fx).astype(np.int32), np.rint(fy).astype(np.int32)]
    return out


def brief_np(img, corners, pattern=None):
    """-> desc (n, 32) u8, angle (n,) f32, flags (n,) u8 of corners (n, 2) float32 on img (h, w) u8"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    pat = default_pattern() if pattern is None else np.asarray(pattern, np.int8).reshape(256, 4)
    pts = np.asarray(corners, np.float32).reshape(-1, 2)
    n = len(pts)
    desc, angle, flags = np.zeros((n, 32), np.uint8), np.zeros(n, np.float32), np.zeros(n, np.uint8)
    S = blur(img) if h >= 7 and w >= 7 else None
    for i, (cx, cy) in enumerate(pts):
        if not (np.isfinite(cx) and np.isfinite(cy)):
            flags[i] = 2
            continue
        xr, yr = np.rint(cx), np.rint(cy)                     # float32, half to even
        if not (M <= xr <= w - 1 - M and M <= yr <= h - 1 - M):
            flags[i] = 1
            continue
        x, y = int(xr), int(yr)
        c, s, angle[i] = orientation(*moments(img, x, y))
        ix1, iy1, ix2, iy2 = steer(pat, c, s)
        assert max(np.abs(ix1).max(), np.abs(iy1).max(), np.abs(ix2).max(), np.abs(iy2).max()) <= 21
        bits = S[y + iy1 - 3, x + ix1 - 3] < S[y + iy2 - 3, x + ix2 - 3]
        desc[i] = np.packbits(bits, bitorder="little")
    return desc, angle, flags


def hamming_knn2_np(d1, d2):
    """cv2.BFMatcher(NORM_HAMMING).knnMatch(k=2): d1 (n1, nbytes), d2 (n2, nbytes) u8 -> idx (n1, 2) i32, dist (n1, 2) i32, ordered by
    (distance, train index); an empty slot is idx -1, dist INT32_MAX"""
    d1, d2 = np.asarray(d1, np.uint8), np.asarray(d2, np.uint8)
    D = np.unpackbits(d1[:, None, :] ^ d2[None, :, :], axis=2).sum(axis=2).astype(np.int64)
    n1, n2 = D.shape
    order = np.argsort(D * n2 + np.arange(n2)[None, :], axis=1, kind="stable")[:, :2]
    idx = np.full((n1, 2), -1, np.int32)
    dist = np.full((n1, 2), INT32_MAX, np.int32)
    k = order.shape[1]
    idx[:, :k] = order
    dist[:, :k] = np.take_along_axis(D, order, axis=1)
    return idx, dist


# ---- test images ------------------------------------------------------------------------------------------------------------------------
def noise_image(w, h, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w)).astype(np.uint8)


def blocks_image(w, h, seed, cell=9):
    rs = np.random.RandomState(seed)
    g = rs.randint(0, 256, (h // cell + 1, w // cell + 1)).astype(np.uint8)
    return np.kron(g, np.ones((cell, cell), np.uint8))[:h, :w].copy()


def ramp_image(w, h):
    """a diagonal ramp: the centroid lies along (1, 1), orientation near 45 degrees -- the steered samples reach radius 21"""
    y, x = np.mgrid[0:h, 0:w]
    return np.clip(x + y, 0, 255).astype(np.uint8)


def flat_image(w, h, v=77):
    return np.full((h, w), v, np.uint8)
