"""Full-contrast inputs for the tracker and the corner detector, and an int64 model of the tracker kernels' partial sums.

The suite's textures reach a quarter of the integer ranges that csrc/vo_klt_lk.h and k_st_eig_fused (csrc/vo_shi_tomasi.hip) argue about in
their comments.  The images here hold the values 0 and 255 only, so every derivative sits at its bound (|Scharr| = 4080, |Sobel| = 1020):
    checker2   2 x 2-pixel checkerboard                  corners everywhere: tracked, and the largest mismatch sums
    mix        left half vertical, right half horizontal stripes two pixels wide: the largest template sums; only the seam is trackable
    diag       ((x + y) // 2) % 2                         one gradient direction (aperture problem: rejected, but for three border points)
    vstripes2  vertical stripes two pixels wide           Iy = 0 everywhere: every point is rejected
    flat0, flat255                                        no gradient at all
Pairs for the tracker: the image against itself rolled by one pixel in x, by one pixel in x and y, and against its inverse 255 - image (the
gross mismatch: |I - J| = 255 at every pixel).

`lane_sums` restates the lane map of klt_lk_point -- lane = 16 r + cp owns window rows 8 r .. 8 r + 7 and columns 2 cp, 2 cp + 1; a quad is four
adjacent lanes -- on the windows that tests/klt_seed_model.py::klt_np records in its trace, in int64: per-lane, per-quad and full-window sums
of A11, A12, A22 and, per LK iteration, of b1 and b2.

`corner_response_f32` is a second, bit-exact formulation of the oracle's exact-integer eigenvalue / Harris maps; its `prefix` argument forms the
horizontal window sums the way the fused kernel does (differences of a 256-column uint32 prefix), wrapping or -- the mutant -- saturating.

Everything is deterministic and reads nothing outside the repository."""
import functools

import numpy as np
from scipy import ndimage

import klt_seed_model as km

WIN = 31
KLT_SIZES = ((128, 96), (131, 97))                 # (w, h): two pyramid levels at window 31; the second odd in both directions
ST_SIZES = ((300, 96), (259, 67))                  # wider than the 224 output columns of one workgroup of the fused kernel
SATURATED = ("checker2", "mix", "diag", "vstripes2")
IMAGES = SATURATED + ("flat0", "flat255")
PAIRS = ("roll01", "roll11", "inverse")
# cases in which no point can be tracked, and why (every other case must show both outcomes)
ONLY_REJECTED = {                                    # (`diag` is singular too, but the reflected border breaks its pattern: three border points track)
    "vstripes2": "Iy = 0 everywhere: minEig = 0",
    "flat0": "no gradient: A = 0",
    "flat255": "no gradient: A = 0",
}


def image(name, w, h):
    y, x = np.mgrid[0:h, 0:w]
    if name == "checker2":
        v = (x // 2 + y // 2) % 2
    elif name == "mix":
        v = np.where(x < w // 2, (x // 2) % 2, (y // 2) % 2)
    elif name == "diag":
        v = ((x + y) // 2) % 2
    elif name == "vstripes2":
        v = (x // 2) % 2
    elif name == "flat0":
        v = np.zeros((h, w), np.int64)
    elif name == "flat255":
        v = np.ones((h, w), np.int64)
    else:
        raise ValueError(name)
    return np.ascontiguousarray((v * 255).astype(np.uint8))


def pair(name, kind, w, h):
    """-> (previous, current) frame"""
    a = image(name, w, h)
    if kind == "roll01":
        b = np.roll(a, (0, 1), (0, 1))
    elif kind == "roll11":
        b = np.roll(a, (1, 1), (0, 1))
    elif kind == "inverse":
        b = 255 - a
    else:
        raise ValueError(kind)
    return a, np.ascontiguousarray(b)


def points(w, h, seed=0):
    """about 40 points: integer positions in all 16 phases of the period-4 patterns (the mismatch sums depend on the phase) with the first
    ones on the seam of `mix`, then the lattices k / 2, k / 128 and k / 16384, then random ones; one of each kind hangs over the border.
    A bilinear weight a b 2^14 is an exact .5 tie where one fraction is 1 / 2 and the other an odd multiple of 2^-14: four lattice points are
    placed there (two round to even downwards, two upwards); the periodic patterns then step by dyadic fractions and meet more ties on the way"""
    rng = np.random.default_rng(1000 + seed)
    cx, cy = w // 2, h // 2
    ints = [(cx - 8 + 5 * (i % 4) + i // 4, cy - 8 + 5 * (i // 4) + i % 4) for i in range(16)]       # (x % 4, y % 4) takes all 16 values
    ints += [(20, 20), (w - 21, 21), (3, h - 4)]                                                  # left half, right half of `mix`, border
    lat = []
    for den, cnt in ((2, 5), (128, 5), (16384, 4)):
        for _ in range(cnt):
            lat.append((rng.integers(16 * den, (w - 16) * den) / den, rng.integers(16 * den, (h - 16) * den) / den))
    lat += [(cx + 0.5, cy + 4 + 4097 / 16384), (cx + 2.5, cy - 5 + 4099 / 16384), (cx - 6 + 12289 / 16384, cy + 0.5), (cx + 7 + 3 / 16384, cy - 2.5)]
    lat += [(cx + 0.5, cy + 0.5), (cx - 3.5, cy + 2.0), (cx + 1 / 128, cy + 0.5 + 1 / 128), (1.5, 1.5)]
    rnd = list(zip(rng.uniform(16, w - 16, 6), rng.uniform(16, h - 16, 6))) + [(w - 2.3, h / 3.0)]
    return np.array(ints + lat + rnd, np.float32)


N_INT = 19                                          # points()[:N_INT] are the integer positions


# ---- the parameters no GPU test varied ------------------------------------------------------------------------------------------------------
THRESHOLDS = [0.0, 1e-4, 0.03, 0.1, 0.3, 1e3, np.inf, -1.0, np.nan]
MAX_COUNTS = [-5, 0, 1, 100, 101, 1000]
EPSILONS = [-1.0, 0.0, 10.0, 11.0]
CRITERIA = [(m, 0.03) for m in MAX_COUNTS] + [(30, e) for e in EPSILONS] + [(100, 0.0), (0, 0.0)]      # (max_count, epsilon)


def edges_pair():
    """the 320 x 240 seed-8 pair of tests/test_gpu_edges.py with 200 grid points"""
    from vo_mi355x import synthetic as syn
    fr, _ = syn.make_sequence(2, w=320, h=240, seed=8, margin=48)
    return fr[0], fr[1], syn.grid_points(200, 320, 240)


def own_thresholds(im0, im1, p0, count=3):
    """level-0 minEig of `count` tracked points with different values, each with its float neighbours: the status flips exactly there"""
    tr = []
    st = km.klt_np(im0, im1, p0, trace=tr)[1]
    vals = []
    for r in tr:
        if r["level"] == 0 and st[r["pt"]] and r["min_eig"] not in vals:
            vals.append(r["min_eig"])
    vals = sorted(vals)
    vals = [vals[0], vals[len(vals) // 2], vals[-1]][:count]
    out = []
    for v in vals:
        out += [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]
    return out


def sweep_pairs():
    a, b = pair("checker2", "roll01", *KLT_SIZES[0])
    return [("checker2", a, b, points(*KLT_SIZES[0])), ("edges", ) + edges_pair()]


# ---- the int64 lane model ------------------------------------------------------------------------------------------------------------------
def _lanes(prod):
    """win x win int64 products -> (64,) per-lane sums: lane = 16 r + cp, rows 8 r + s (s = 0..7), columns 2 cp and 2 cp + 1"""
    p = np.zeros((32, 32), np.int64)
    p[: prod.shape[0], : prod.shape[1]] = prod
    return p.reshape(4, 8, 16, 2).sum((1, 3)).reshape(64)


def _three(prod):
    lane = _lanes(prod)
    quad = lane.reshape(16, 4).sum(1)               # four adjacent lanes
    full = int(quad.sum())
    assert full == int(prod.sum())
    return dict(lane=lane, quad=quad, full=full)


def lane_sums(trace):
    """klt_np's trace -> one dict per (point, level): pt, level, min_eig, A11 / A12 / A22 = dict(lane, quad, full) and b1 / b2 = a list of such
    dicts, one per LK iteration; all int64"""
    out = []
    for r in trace:
        gx, gy = r["gx"], r["gy"]
        out.append(dict(pt=r["pt"], level=r["level"], min_eig=r["min_eig"],
                        A11=_three(gx * gx), A12=_three(gx * gy), A22=_three(gy * gy),
                        b1=[_three(d * gx) for d in r["diffs"]], b2=[_three(d * gy) for d in r["diffs"]]))
    return out


@functools.lru_cache(maxsize=None)
def model(name, kind, size, **kw):
    """klt_np on one case with its trace -> (p1, status, err, iters, lane sums); computed once per process"""
    w, h = size
    a, b = pair(name, kind, w, h)
    tr = []
    res = km.klt_np(a, b, points(w, h), trace=tr, **kw)
    for x in res:
        x.setflags(write=False)
    return res + (lane_sums(tr),)


def tracker_cases():
    return [(n, k, s) for n in IMAGES for k in PAIRS for s in KLT_SIZES]


# ---- the corner response, bit for bit ------------------------------------------------------------------------------------------------------
def _sobel(img):
    a = img.astype(np.int64)
    sm, df = np.array([1, 2, 1], np.int64), np.array([-1, 0, 1], np.int64)
    dx = ndimage.correlate1d(ndimage.correlate1d(a, sm, axis=0, mode="mirror"), df, axis=1, mode="mirror")
    dy = ndimage.correlate1d(ndimage.correlate1d(a, sm, axis=1, mode="mirror"), df, axis=0, mode="mirror")
    return dx, dy


def column_sums(img, block=31):
    """exact int64 sums over `block` rows (reflect-101 on the product images) of dx^2, dx dy, dy^2: (3, h, w)"""
    dx, dy = _sobel(img)
    box = np.ones(block, np.int64)
    return np.stack([ndimage.correlate1d(p, box, axis=0, mode="mirror") for p in (dx * dx, dx * dy, dy * dy)])


def window_sums(img, block=31, prefix=None):
    """exact int64 block x block sums (3, h, w).  prefix = None: a box correlation.  prefix = "wrap" / "saturate": the fused kernel's form --
    a workgroup of 256 product columns (reflected like the box filter reflects them) owns 256 - 2 R - 2 output columns, forms the inclusive
    prefix P of its column sums in uint32 and S(x) = P(x + R) - P(x - R - 1) modulo 2^32, read as int32.  "wrap" is exact whenever
    |S| < 2^31, however often P overflows; "saturate" (P clamped at the ends of its type) is the mutant."""
    V = column_sums(img, block)
    if prefix is None:
        return np.stack([ndimage.correlate1d(v, np.ones(block, np.int64), axis=1, mode="mirror") for v in V])
    R = block // 2
    h, w = img.shape
    outc = 256 - 2 * R - 2
    S = np.zeros_like(V)
    M = 1 << 32
    for x0 in range(0, w, outc):
        cols = np.arange(x0 - 1 - R, x0 - 1 - R + 256)
        cols = np.abs(cols)                                                  # reflect-101, one reflection is enough (R + 1 < w)
        cols = np.where(cols >= w, 2 * (w - 1) - cols, cols)
        cols = np.clip(cols, 0, w - 1)                                       # (threads far beyond the image: their sums are never used)
        Vt = V[:, :, cols] % M                                               # uint32 encodings (sxy may be negative)
        if prefix == "wrap":
            P = np.cumsum(Vt, axis=2) % M
        else:                                                                # clamped at the ends of the type: uint32 for the squares, int32 for dx dy
            P = np.cumsum(V[:, :, cols], axis=2)
            P = np.stack([np.clip(P[0], 0, M - 1), np.clip(P[1], -(M // 2), M // 2 - 1), np.clip(P[2], 0, M - 1)]) % M
        P = np.concatenate([np.zeros(P.shape[:2] + (1,), np.int64), P], 2)   # P[.., t + 1] = inclusive prefix of thread t
        for t in range(R + 1, 255 - R):
            xe = x0 - 1 + t - R
            if xe >= w:
                break
            s = (P[:, :, t + R + 1] - P[:, :, t - R]) % M
            S[:, :, xe] = np.where(s >= M // 2, s - M, s)
    return S


def corner_response_f32(img, block=31, harris=False, k=0.04, prefix=None):
    """the oracle's exact-integer path (cornerMinEigenVal / cornerHarris on exact window sums) in float32 numpy, expression for expression"""
    F = np.float32
    S = window_sums(img, block, prefix)
    sf = F(1.0 / (4.0 * block * 255.0))
    s2 = sf * sf
    sxx, sxy, syy = (s.astype(F) * s2 for s in S)                            # (float)sum * s2: one rounding each
    if harris:
        a, b, c = sxx, sxy, syy
        t = (a + c).astype(np.float64)
        return ((a * c - b * b).astype(np.float64) - k * t * t).astype(F)
    a, b, c = sxx * F(0.5), sxy, syy * F(0.5)
    return (a + c) - np.sqrt((a - c) * (a - c) + b * b)


def disc_mask(w, h, radius=7, seed=0):
    """the exclusion mask of re-detection: discs around about 30 points, some over the border"""
    import vo_oracle as o
    rng = np.random.default_rng(2000 + seed)
    pts = np.stack([rng.uniform(-5, w + 5, 30), rng.uniform(-5, h + 5, 30)], 1).astype(np.float32)
    m = np.full((h, w), 255, np.uint8)
    for x, y in np.int32(pts):
        o.circle_mask(m, (int(x), int(y)), radius, 0)
    return pts, m
