"""Keypoints that are NaN, infinite, beyond the int32 range or cut by the border -- TEST INFRASTRUCTURE, holds no test.

One 160 x 120 frame pair (the pyramid stops at level 1), about 24 honest points and the rows at which the tracker and the exclusion discs
could disagree with OpenCV: cvFloor and np.int32() make INT_MIN of a NaN and of every value outside [-2^31, 2^31), while a GPU's conversion
saturates (NaN -> 0, +inf -> INT_MAX).  Shared by tests/test_nonfinite_cases.py (CPU: the oracle against klt_np, the disc rasteriser) and
tests/test_gpu_nonfinite.py (the kernels against the oracle).

Every row has a kind:
  honest  an ordinary point inside the frame
  dead    a component that is NaN, infinite, beyond int32, or so large that the point is outside every level: OpenCV returns status 0,
          err 0, no level entered and p1 = p0, and draws no disc
  far     (1e6, 1e6): finite, an honest int, outside every level and every disc row
  border  inside or near the frame, so that its window or its disc is cut by the border (and -0.0, which is 0)
"""
import numpy as np

import klt_seed_model as km

W, H = 160, 120
STAMPS = ((4, 4), (4, 60))          # centres of the two painted checker corners: the detector answers near (0, 0) and near (0, 60)
RADII = (0, 7, 31)

_F = np.float32
NAN = _F(np.nan)
NAN_PAYLOAD = np.array([0xFFC00001], np.uint32).view(np.float32)[0]      # negative quiet NaN whose low 16 payload bits are not zero
INF = _F(np.inf)
P31 = _F(2147483648.0)              # 2^31: the first float np.int32() cannot hold
BELOW_P31 = _F(2147483520.0)        # the largest float below 2^31 (an honest int)
M31 = _F(-2147483648.0)             # -2^31 = INT_MIN: an honest int, and the value the out-of-range results share
BELOW_M31 = _F(-2147483904.0)       # the first float below -2^31

# (x, y, kind); the x and y roles also occur swapped
SPECIAL = [
    (NAN, 60, "dead"), (80, NAN, "dead"), (NAN, NAN, "dead"), (NAN, INF, "dead"), (INF, NAN, "dead"),
    (NAN_PAYLOAD, 60, "dead"), (80, NAN_PAYLOAD, "dead"),
    (INF, 60, "dead"), (80, -INF, "dead"), (-INF, INF, "dead"), (80, INF, "dead"), (-INF, 60, "dead"), (INF, -INF, "dead"),
    (P31, 60, "dead"), (80, P31, "dead"),
    (BELOW_P31, 60, "dead"), (80, BELOW_P31, "dead"),
    (M31, 60, "dead"), (80, M31, "dead"), (BELOW_M31, 60, "dead"), (80, BELOW_M31, "dead"),
    (1e10, 60, "dead"), (-1e10, 60, "dead"), (80, 1e10, "dead"), (80, -1e10, "dead"),
    (3e38, -3e38, "dead"), (-3e38, 3e38, "dead"),
    (1e6, 1e6, "far"),
    (-0.0, -0.0, "border"),
    (-3, 5, "border"), (-0.5, 10, "border"), (-7.9, -7.9, "border"), (W + 2, H - 1, "border"), (W - 1, H - 1, "border"),
    (5, -3, "border"), (10, -0.5, "border"), (W - 1, H + 2, "border"),
]
N_HONEST = 25


def stamp(img, cx, cy, s=6, lo=10, hi=245):
    """a 2 x 2 checker of s x s blocks around (cx, cy), cut by the frame"""
    out = img.copy()
    for j in range(-s, s):
        for i in range(-s, s):
            x, y = cx + i, cy + j
            if 0 <= x < out.shape[1] and 0 <= y < out.shape[0]:
                out[y, x] = hi if ((i >= 0) != (j >= 0)) else lo
    return out


def frames(seed=31, n=2):
    """n frames of the synthetic sequence with the two checker corners painted into each (they do not move)"""
    from vo_mi355x import synthetic as syn
    fr, _ = syn.make_sequence(n, w=W, h=H, seed=seed, margin=48)
    out = []
    for f in fr:
        for cx, cy in STAMPS:
            f = stamp(f, cx, cy)
        out.append(f)
    return np.stack(out)


def honest_points(seed=11):
    from vo_mi355x import synthetic as syn
    return syn.grid_points(N_HONEST, W, H, margin=22, seed=seed)


def points(seed=11):
    """-> p0 (n, 2) float32, kind (n,) of str: the special rows spread between the honest ones, so that special rows have honest
    neighbours in the launch grid.  The components are stored one by one as float32, so that a NaN keeps its sign and payload"""
    hon = honest_points(seed)
    order, h = [], 0
    for k in range(len(SPECIAL)):
        order.append(("s", k))
        if k % 3 != 2 and h < len(hon):
            order.append(("h", h)); h += 1
    order += [("h", i) for i in range(h, len(hon))]
    p0 = np.empty((len(order), 2), np.float32)
    kind = []
    for i, (what, k) in enumerate(order):
        x, y, name = SPECIAL[k] if what == "s" else (hon[k, 0], hon[k, 1], "honest")
        p0[i, 0] = _F(x); p0[i, 1] = _F(y)
        kind.append(name)
    assert len(p0) % 4 != 0 and len(p0) % 64 != 0
    return p0, np.array(kind)


def rotated(b, seed=11):
    """sequence b of a batch of 3: the same rows moved to other row indices (rolled by 9 b + 5 rows), another honest set; -> p0, kind"""
    p0, kind = points(seed + b)
    s = 9 * b + 5
    return np.roll(p0, s, axis=0), np.roll(kind, s)


def batch3():
    """-> frames [3, 2, H, W] (a different pair per sequence), p0 [3, n, 2], kind [3, n]"""
    fr = np.stack([frames(31 + 7 * b) for b in range(3)])
    pk = [rotated(b) for b in range(3)]
    return fr, np.stack([p for p, _ in pk]), np.stack([k for _, k in pk])


def without_border(p0, kind):
    """the rows that are not of kind 'border' (last axis of kind / last but one of p0): the set of the disc and step tests in which a
    spurious disc at the origin or on column 0 must show -- the border rows' own discs lie there"""
    keep = kind != "border"
    if p0.ndim == 3:
        n = keep.sum(-1)
        assert (n == n[0]).all()
        return np.stack([p[k] for p, k in zip(p0, keep)]), np.stack([x[k] for x, k in zip(kind, keep)])
    return p0[keep], kind[keep]


def has_nan(p):
    return np.isnan(np.asarray(p, np.float32)).any(-1)


def seed_cases():
    """the two seeded combinations -> name -> (p0, guess, kind of the SPECIAL operand per row)
    finite_guess_special_p0: p0 = points(), every guess finite (a special row's guess lies inside the frame)
    special_guess_honest_p0: every p0 honest (the honest set, repeated), the guesses = points() (a non-finite guess starts from p0;
                             a huge finite one starts outside)"""
    p0, kind = points()
    hon = honest_points()
    g = (p0 + np.array([1.5, 0.5], np.float32)).astype(np.float32)
    sp = kind != "honest"
    g[sp] = np.stack([np.linspace(30, 130, sp.sum()), np.linspace(30, 90, sp.sum())], 1).astype(np.float32)
    assert np.isfinite(g).all()
    q0 = hon[np.arange(len(p0)) % len(hon)].copy()
    q0[~sp] = p0[~sp]
    g2 = p0.copy()
    g2[~sp] += np.array([1.5, 0.5], np.float32)
    return {"finite_guess_special_p0": (p0, g, kind), "special_guess_honest_p0": (q0, g2, kind)}


def disc_mask(pts, radius, base=None):
    """the reference's exclusion mask: 255 (or base) with cv2.circle(..., 0, -1) at np.int32(pts) = km.to_int32(pts)"""
    import vo_oracle as o
    mask = np.full((H, W), 255, np.uint8) if base is None else np.ascontiguousarray(base, np.uint8).copy()
    for x, y in km.to_int32(np.asarray(pts, np.float32).reshape(-1, 2)):
        o.circle_mask(mask, (int(x), int(y)), int(radius), 0)
    return mask


def brute_disc(cx, cy, radius, hw):
    """pixels of the filled midpoint circle at the int centre (cx, cy), restated without the rasteriser's walk: row dy holds the columns
    |dx| <= hw[|dy|], hw = the half widths circle_rows(radius) reports (the dx^2 + dy^2 <= r^2 disc, widened where the outline's
    octant walk steps).  -> bool [H, W]"""
    ys, xs = np.mgrid[0:H, 0:W]
    dy = np.abs(ys - int(cy))
    inside = dy <= radius
    half = np.where(inside, np.asarray(hw)[np.minimum(dy, radius)], -1)
    return inside & (np.abs(xs - int(cx)) <= half)
