"""sift_model.py -- an independent model of cv2.SIFT_create(nfeatures).detect(img, mask) + compute (OpenCV 4.4), test infrastructure.

Written from Lowe 2004 and the published structure of OpenCV 4.4's SIFT; it imports nothing from oracle/ and reaches every result by another
route than oracle/sift_oracle.py and csrc/vo_sift.hip: scipy.ndimage.correlate1d(mode='mirror') for the blurs (float64) or a left-to-right tap
sum over an np.pad(mode='reflect') frame (float32), map_coordinates(order=1) for the 2x upsample, strided slicing for the decimation,
maximum_filter / minimum_filter over the 3-D DoG stack for the extrema, np.linalg.solve for the 3 x 3 step, np.bincount for both histograms,
vectorised trilinear spreading for the descriptor.  Shared with the oracle is data only: OpenCV's constants, the fastAtan2 coefficients, the
KeyPoint_LessThan order.

The whole model runs in float64 or float32 (`dtype`); the float32 run is how the rounding sensitivity of the ALGORITHM is measured without
looking at the kernel.  Every discrete decision records its margin against a bound that follows from E_DOG, the absolute error of a float32 DoG
sample: where a decision is inside its margin BOTH outcomes are followed, so a candidate ends as
  certified  kept, every decision on its way clear,
  marginal   some decision inside its margin (kept or dropped by the model itself: `own`),
  dropped    certainly no keypoint.
judge_keypoints / judge_descriptor are the verdicts the CPU test (on the oracle) and the GPU test (on the kernel) share.

Pinned conventions (tests/test_sift_model.py proves them on blobs, ramps, transposes):
  * a feature at pixel centre (cx, cy) is reported at (cx + 0.25, cy + 0.25): OpenCV 4.4's createInitialImage doubles the image with
    INTER_LINEAR (sample d of the doubled image sits at (d + 0.5) / 2 - 0.5), and keypoints are halved without the 0.25 px being taken back;
  * angle = direction of the intensity gradient (dark -> bright), degrees, measured from +x towards +y with y pointing DOWN, i.e.
    atan2(gy_down, gx) mod 360.
"""
import itertools
import math

import numpy as np
from scipy import ndimage

# ---- OpenCV's constants (data) ---------------------------------------------------------------------------------------------------------------
N_LAYERS = 3
SIGMA = 1.6
CONTRAST_THR = 0.04
EDGE_THR = 10.0
BORDER = 5
MAX_STEPS = 5
ORI_BINS = 36
ORI_SIG = 1.5
ORI_RADIUS = 3.0 * ORI_SIG
ORI_PEAK = 0.8
D_W = 4
D_BINS = 8
D_SCL = 3.0
D_MAG_THR = 0.2
D_INT = 512.0
FLT_EPS = 1.1920929e-07
ATAN_P = (0.9997878412794807, -0.3258083974640975, 0.1555786518463281, -0.04432655554792128)

# ---- measured bounds: largest |model32 - model64| over IMAGES and their transposes (test_sift_model.py::test_constants_hold measures again),
# times 4 (the kernel sums its taps in another order than the model does) --------------------------------------------------------------------
E_DOG = 3.9e-04        # DoG sample, grey levels                                      measured 9.67e-05
E_GAUSS = 4.4e-04      # Gaussian sample, grey levels                                 measured 0.000108
POS_TOL = 3.0e-03      # x, y in pixels of the keypoint's octave (first octave: 0.5)  measured 0.000725
SIZE_TOL = 4.1e-04     # relative size                                                measured 0.0001
ANG_TOL = 5.5e-04      # degrees, where no histogram sample may change bins           measured 0.000135
RESP_TOL = 7.6e-07     # response                                                     measured 1.88e-07
DESC_TOL = 4.0        # descriptor entry, units of the 0..255 output                 measured 1
# reasoning, not measurement: a sequential float32 sum of N <= (2 * 18 + 1)^2 = 1369 non-negative terms is off by at most N * 2^-24 of the sum,
# each term (exp * sqrt) by a few 2^-24 more
HIST_REL = 1.0e-4
# fastAtan2 against np.arctan2, degrees: measured 9.56e-3 in float32 (test_fast_atan2 asserts 1.5 x)
ATAN_DEV = 9.56e-3
EXCUSED_MAX = 0.05
ANG_SLACK_MAX = 5.0   # degrees: a keypoint whose histogram samples on a bin boundary could move its angle by more is marginal
SLACK_SEEN = 2.5      # degrees: the largest slack granted to a CERTIFIED keypoint of the judged images, measured 2.4934 (texture97x61; median
                      # 0.007, 90th percentile 0.2 - 0.3); test_constants_hold asserts it does not grow

E_G = math.sqrt(3.0) * E_DOG / 255.0          # |error| of the DoG gradient (each component (a - b) * 0.5 / 255)
WILD_M = 0.25                                 # an offset margin beyond this: the walk is not followed, the place is excused
MAX_NODES = 48


def key_less_than(k):
    """KeyPoint_LessThan (data): x, y ascending, size descending, angle ascending, response descending, octave descending"""
    return (k[0], k[1], -k[2], k[3], -k[4], -k[5])


# ---- images the constants are measured on and the tests run on -----------------------------------------------------------------------------
def texture(w, h, seed):
    from vo_mi355x import synthetic as syn
    return np.ascontiguousarray(np.asarray(syn.make_texture(2 * w, 2 * h, seed=seed))[:h, :w]).astype(np.uint8)


def blocks(w, h, seed):
    rng = np.random.default_rng(seed)
    return np.kron(rng.integers(0, 2, (h // 12 + 1, w // 12 + 1)) * 235 + 10, np.ones((12, 12), int))[:h, :w].astype(np.uint8)


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w)).astype(np.uint8)


IMAGES = {                                    # name -> (maker, w, h, seed, least number of certified keypoints)
    "texture161x97": (texture, 161, 97, 3, 10),
    "texture97x61": (texture, 97, 61, 32, 10),
    "blocks120x90": (blocks, 120, 90, 19, 10),
    "noise64x48": (noise, 64, 48, 12, 3),
    "texture41x33": (texture, 41, 33, 20, 3),
}


def image(name):
    """the five images, and `<name> T` for a transpose"""
    if name.endswith(" T"):
        return np.ascontiguousarray(image(name[:-2]).T)
    mk, w, h, seed, _ = IMAGES[name]
    return mk(w, h, seed)


JUDGED = list(IMAGES) + ["texture161x97 T", "texture97x61 T"]      # non-square both ways


def least_certified(name):
    return IMAGES[name[:-2] if name.endswith(" T") else name][4]


def blob_image(w, h, cx, cy, s, amp, base=None):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = (60.0 if amp > 0 else 200.0) if base is None else base          # nothing clips
    return np.clip(np.rint(base + amp * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * s * s))), 0, 255).astype(np.uint8)


def ramp_image(phi_deg, w=128, h=96, s=4.0):
    """128 + 1.2 ramp + 60 blob(s): the ramp's gradient points along phi (y down)"""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    cx, cy = (w - 1) / 2.0, (h - 1) / 2.0
    ph = math.radians(phi_deg)
    ramp = (x - cx) * math.cos(ph) + (y - cy) * math.sin(ph)
    return np.clip(np.rint(128.0 + 1.2 * ramp + 60.0 * np.exp(-((x - cx) ** 2 + (y - cy) ** 2) / (2.0 * s * s))), 0, 255).astype(np.uint8)


# ---- scale space ---------------------------------------------------------------------------------------------------------------------------
def gaussian_taps(sigma):
    """cv::getGaussianKernel(cvRound(8 sigma + 1) | 1, sigma, CV_32F): float32 taps (data of the algorithm, both dtypes use them)"""
    n = int(np.rint(sigma * 8 + 1)) | 1
    x = np.arange(n) - (n - 1) / 2.0
    t = np.exp(-x * x / (2.0 * sigma * sigma))
    return (t / t.sum()).astype(np.float32)


def layer_sigmas():
    k = 2.0 ** (1.0 / N_LAYERS)
    total = [SIGMA * k ** i for i in range(N_LAYERS + 3)]
    return [SIGMA] + [math.sqrt(total[i] ** 2 - total[i - 1] ** 2) for i in range(1, N_LAYERS + 3)], total


def upsample2(img):
    """resize to twice the size, INTER_LINEAR: sample d of the result sits at (d + 0.5) / 2 - 0.5 of the source, clamped.  Exact in float32
    (weights 1/4 and 3/4 on integers)."""
    h, w = img.shape
    yy = np.clip((np.arange(2 * h) + 0.5) / 2 - 0.5, 0, h - 1)
    xx = np.clip((np.arange(2 * w) + 0.5) / 2 - 0.5, 0, w - 1)
    return ndimage.map_coordinates(img.astype(np.float64), np.meshgrid(yy, xx, indexing="ij"), order=1, mode="nearest")


def blur(img, sigma, dtype=np.float64):
    k = gaussian_taps(sigma)
    if dtype == np.float64:
        out = ndimage.correlate1d(img, k.astype(np.float64), axis=1, mode="mirror")
        return ndimage.correlate1d(out, k.astype(np.float64), axis=0, mode="mirror")
    return blur_taps(img, k, dtype)


def blur_taps(img, k, dtype):
    """the same blur as a plain tap sum in `dtype`, taps left to right (another order than the kernel's centre-outward pairs)"""
    r = len(k) // 2
    out = img.astype(dtype)
    for axis in (1, 0):
        n = out.shape[axis]
        pad = [(0, 0), (0, 0)]
        pad[axis] = (r, r)
        p = np.pad(out, pad, mode="reflect")
        acc = np.zeros_like(out)
        for i in range(len(k)):
            acc = acc + dtype(k[i]) * np.take(p, np.arange(i, i + n), axis=axis)
        out = acc
    return out


def n_octaves(w, h):
    return int(np.rint(math.log2(min(2 * w, 2 * h)) - 2)) + 1


def pyramids(img, dtype=np.float64):
    """-> gauss[o] (6, rows, cols), dog[o] (5, rows, cols); octave 0 is the doubled image"""
    inc, _ = layer_sigmas()
    base = blur(upsample2(np.asarray(img)).astype(dtype), math.sqrt(max(SIGMA * SIGMA - 4 * 0.5 * 0.5, 0.01)), dtype)
    gauss, dog = [], []
    for o in range(n_octaves(img.shape[1], img.shape[0])):
        if o > 0:
            prev = gauss[-1][N_LAYERS]
            base = prev[0:2 * (prev.shape[0] // 2):2, 0:2 * (prev.shape[1] // 2):2]
        if min(base.shape) < 1:
            break
        layers = [base]
        for i in range(1, N_LAYERS + 3):
            layers.append(blur(layers[-1], inc[i], dtype))
        g = np.stack(layers)
        gauss.append(g)
        dog.append(g[1:] - g[:-1])
    return gauss, dog


def fast_atan2(y, x, dtype=np.float64, flip=None):
    """cv::fastAtan2's polynomial (degrees); the coefficients are OpenCV's float products.  The polynomial is 0.0095 degrees short at 45,
    so the result jumps by 0.019 degrees where |x| = |y|; `flip` takes the other side of that jump where it is set."""
    deg = np.float32(180.0 / np.pi)
    p1, p3, p5, p7 = (dtype(np.float32(c) * deg) for c in ATAN_P)
    ax, ay = np.abs(x), np.abs(y)
    swap = ay > ax
    if flip is not None:
        swap = swap ^ flip
    c = np.where(swap, ax, ay) / (np.where(swap, ay, ax) + dtype(2.220446049250313e-16))
    c2 = c * c
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    a = np.where(swap, dtype(90) - a, a)
    a = np.where(x < 0, dtype(180) - a, a)
    return np.where(y < 0, dtype(360) - a, a).astype(dtype)


# ---- candidates ----------------------------------------------------------------------------------------------------------------------------
def _candidates(S):
    """26-neighbour extrema of layers 1..3 with |v| > 1, by filters over the 3-D stack -> (layer, r, c, clear)"""
    rows, cols = S.shape[1:]
    if rows <= 2 * BORDER or cols <= 2 * BORDER:
        return []
    fp = np.ones((3, 3, 3), bool)
    fp[1, 1, 1] = False
    hi = ndimage.maximum_filter(S, footprint=fp, mode="nearest")
    lo = ndimage.minimum_filter(S, footprint=fp, mode="nearest")
    sl = (slice(1, N_LAYERS + 1), slice(BORDER, rows - BORDER), slice(BORDER, cols - BORDER))
    v, hi, lo = S[sl].astype(np.float64), hi[sl].astype(np.float64), lo[sl].astype(np.float64)
    m_ext = np.where(v > 0, v - hi, lo - v)               # v minus the best of the 26 neighbours (sign-adjusted)
    m_thr = np.abs(v) - 1.0                               # threshold floor(0.5 * 0.04 / 3 * 255) = 1
    may = (m_thr > -E_DOG) & (m_ext >= -2 * E_DOG) & (v != 0)
    own = (m_thr > 0) & (m_ext >= 0)
    clear = (m_thr > E_DOG) & (m_ext > 2 * E_DOG)
    return [(int(l) + 1, int(r) + BORDER, int(c) + BORDER, bool(clear[l, r, c]), bool(own[l, r, c])) for l, r, c in zip(*np.nonzero(may))]


def _derivs(S, l, r, c, dtype):
    img, prev, nxt = S[l], S[l - 1], S[l + 1]
    s = dtype(1.0 / 255.0)
    g = np.array([img[r, c + 1] - img[r, c - 1], img[r + 1, c] - img[r - 1, c], nxt[r, c] - prev[r, c]], dtype) * (s * dtype(0.5))
    v2 = dtype(2) * img[r, c]
    dxx = (img[r, c + 1] + img[r, c - 1] - v2) * s
    dyy = (img[r + 1, c] + img[r - 1, c] - v2) * s
    dss = (nxt[r, c] + prev[r, c] - v2) * s
    q = s * dtype(0.25)
    dxy = (img[r + 1, c + 1] - img[r + 1, c - 1] - img[r - 1, c + 1] + img[r - 1, c - 1]) * q
    dxs = (nxt[r, c + 1] - nxt[r, c - 1] - prev[r, c + 1] + prev[r, c - 1]) * q
    dys = (nxt[r + 1, c] - nxt[r - 1, c] - prev[r + 1, c] + prev[r - 1, c]) * q
    return g, np.array([[dxx, dxy, dxs], [dxy, dyy, dys], [dxs, dys, dss]], dtype)


def _why(why, cond, tag):
    """the reasons a keypoint is marginal (empty: every decision so far was clear)"""
    return why + (tag,) if cond and tag not in why else why


class _Walk:
    """one candidate's refinement, every marginal decision followed both ways"""

    def __init__(self, S, G, o, dtype):
        self.S, self.G, self.o, self.dtype = S, G, o, dtype
        self.nodes, self.wild, self.out = 0, False, []

    def step(self, l, r, c, i, marg, own):
        S, dtype = self.S, self.dtype
        rows, cols = S.shape[1:]
        self.nodes += 1
        if self.nodes > MAX_NODES:
            self.wild = True
            return
        if i >= MAX_STEPS:
            return
        g, H = _derivs(S, l, r, c, dtype)
        try:
            X = -np.linalg.solve(H, g)
            h_inv = np.linalg.inv(H.astype(np.float64))
        except np.linalg.LinAlgError:
            self.wild = True
            return
        # dx = H^-1 (dg - dH x), first order, component by component: |dg_i| <= E / 255 (two samples * 0.5), row i of dH holds one second
        # difference (4 E / 255) and two cross terms (four samples * 0.25: E / 255); this is |H^-1| (E_g + E_H |x|) without the slack of the norms
        ax = np.abs(X).astype(np.float64)
        mv = np.abs(h_inv) @ ((1.0 + 3.0 * ax + ax.sum()) * (E_DOG / 255.0))
        m = float(mv.max())
        if not np.isfinite(m) or m > WILD_M:
            self.wild = True
            return
        a = float(ax.max())
        conv = a < 0.5
        sure_conv, sure_move = bool(np.all(ax + mv < 0.5)), bool(np.any(ax - mv >= 0.5))
        if conv or not sure_move:
            self.finish(l, r, c, X, g, H, mv, _why(marg, not sure_conv, 'offset'), own and conv)
        if not conv or not sure_conv:
            if a > 2147483647 / 3:
                return
            mv_marg, mv_own = _why(marg, not sure_move, 'offset'), own and not conv
            opts = []
            for x, mx in ((float(X[2]), mv[2]), (float(X[1]), mv[1]), (float(X[0]), mv[0])):       # layer, row, column
                base = int(np.rint(x))
                o_ = [(base, True)]
                if abs(x - (math.floor(x) + 0.5)) <= mx:
                    o_.append((2 * int(math.floor(x)) + 1 - base, False))          # the other of floor(x), floor(x) + 1
                opts.append(o_)
            for (dl, el), (dr, er), (dc, ec) in itertools.product(*opts):
                e = el and er and ec
                nl, nr, nc = l + dl, r + dr, c + dc
                if nl < 1 or nl > N_LAYERS or nc < BORDER or nc >= cols - BORDER or nr < BORDER or nr >= rows - BORDER:
                    continue
                self.step(nl, nr, nc, i + 1, _why(mv_marg, len(opts[0]) + len(opts[1]) + len(opts[2]) > 3, 'step'), mv_own and e)

    def finish(self, l, r, c, X, g, H, mv, marg, own):
        S, G, o, dtype = self.S, self.G, self.o, self.dtype
        xc, xr, xi = X[0], X[1], X[2]
        contr = S[l, r, c] * dtype(1.0 / 255.0) + dtype(0.5) * (g[0] * xc + g[1] * xr + g[2] * xi)
        resp = abs(float(contr))
        e_c = E_DOG / 255.0 + 0.5 * (E_G * float(np.linalg.norm(X)) + float(np.abs(g).astype(np.float64) @ mv))
        d = resp * N_LAYERS - CONTRAST_THR
        if d < -N_LAYERS * e_c:
            return
        marg, own = _why(marg, d < N_LAYERS * e_c, 'contrast'), own and d >= 0
        dxx, dyy, dxy = float(H[0, 0]), float(H[1, 1]), float(H[0, 1])
        tr, det = dxx + dyy, dxx * dyy - dxy * dxy
        f = (EDGE_THR + 1) ** 2 * det - EDGE_THR * tr * tr          # kept iff det > 0 and tr^2 r < (r + 1)^2 det, i.e. f > 0
        d2, d1 = 4 * E_DOG / 255.0, E_DOG / 255.0
        e_f = (EDGE_THR + 1) ** 2 * ((abs(dxx) + abs(dyy)) * d2 + 2 * abs(dxy) * d1) + 4 * EDGE_THR * abs(tr) * d2
        if f <= -e_f:
            return
        marg, own = _why(marg, f <= e_f, 'edge'), own and f > 0 and det > 0
        pw = dtype(2.0) ** ((dtype(l) + xi) / dtype(N_LAYERS))
        size = float(dtype(SIGMA) * pw * dtype(2 << o))
        scl = size * 0.5 / (1 << o)
        t = ORI_RADIUS * scl
        radii = [(int(np.rint(t)), True)]
        if abs(t - (math.floor(t) + 0.5)) <= ORI_RADIUS * scl * (math.log(2.0) / N_LAYERS * mv[2] + 4 * FLT_EPS):
            radii.append((2 * int(math.floor(t)) + 1 - radii[0][0], False))
        third = int(np.rint((float(xi) + 0.5) * 255))
        for radius, e in radii:
            for p in _orientations(G[l], r, c, radius, ORI_SIG * scl, dtype):
                why = _why(_why(marg, p["tag"], p["tag"]), len(radii) > 1, 'radius')
                self.out.append(dict(x=float((dtype(c) + xc) * dtype(1 << o)) * 0.5, y=float((dtype(r) + xr) * dtype(1 << o)) * 0.5, size=size * 0.5,
                                     angle=p["angle"], response=resp, octave=((o - 1) & 255) | (l << 8) | (third << 16),
                                     o=o, l=l, r=r, c=c, j=p["j"], tie=p["tie"], radius=radius, m=float(mv.max()), slack=p["slack"], flips=p["flips"],
                                     why=why, own=own and p["own"] and e))


def _orientations(img, r, c, radius, sigma, dtype):
    """calcOrientationHist + the peak loop -> [dict(j, angle, tag ("" / "peak" / "tie"), own, slack, flips, tie)]"""
    rows, cols = img.shape
    ys = np.arange(max(r - radius, 1), min(r + radius, rows - 2) + 1)
    xs = np.arange(max(c - radius, 1), min(c + radius, cols - 2) + 1)
    if len(ys) == 0 or len(xs) == 0:
        return []
    Y, X = np.meshgrid(ys, xs, indexing="ij")
    dx = (img[Y, X + 1] - img[Y, X - 1]).ravel()
    dy = (img[Y - 1, X] - img[Y + 1, X]).ravel()
    w = np.exp(((Y - r) ** 2 + (X - c) ** 2).ravel().astype(dtype) * (dtype(-1) / (dtype(2) * dtype(sigma) * dtype(sigma))))
    ori = fast_atan2(dy, dx, dtype)
    mag = np.sqrt(dx * dx + dy * dy)
    keep = mag > 0                                        # a flat sample adds nothing to any bin
    dx, dy, w, ori, mag = dx[keep], dy[keep], w[keep], ori[keep], mag[keep]
    n = ORI_BINS
    t = ori.astype(np.float64) * (n / 360.0)
    raw = np.bincount(np.rint(t).astype(np.int64) % n, weights=(w * mag).astype(np.float64), minlength=n)
    # mass that may sit one bin further: the sample's direction is within its own error (gradient error 2 sqrt 2 E_GAUSS across it) of a bin
    # boundary.  Moving w from bin b to b +- 1 changes the [1 4 6 4 1] / 16 smoothed bins b - 3 .. b + 3 by at most 3 w / 16 each.
    d_ori = np.degrees(2.0 * math.sqrt(2.0) * E_GAUSS / np.maximum(mag.astype(np.float64), 1e-30)) + 360.0 * 4 * FLT_EPS
    near = np.abs(t - np.floor(t) - 0.5) * (360.0 / n) <= d_ori
    # ... or the gradient is within its error of a diagonal, where fastAtan2 jumps, and the jump crosses a boundary (corners of axis-aligned
    # blocks: |dx| = |dy| by symmetry, 45 degrees is a boundary, rounding decides the side)
    diag = (np.abs(np.abs(dx) - np.abs(dy)).astype(np.float64) <= 4 * E_GAUSS) & (mag > 12 * E_GAUSS)   # (smaller ones are `near` anyway)
    t2 = fast_atan2(dy, dx, dtype, flip=diag).astype(np.float64) * (n / 360.0)
    near |= np.rint(t2) != np.rint(t)
    t_lo = np.where(np.rint(t2) != np.rint(t), np.minimum(t, t2), t)
    u = np.zeros(n)
    for b, wm in zip(np.floor(t_lo[near]).astype(np.int64), (w * mag).astype(np.float64)[near]):       # boundary between bins b and b + 1
        u[np.arange(b - 2, b + 4) % n] += wm
    hist = ((np.roll(raw, 2) + np.roll(raw, -2)) / 16.0 + (np.roll(raw, 1) + np.roll(raw, -1)) * (4.0 / 16.0) + raw * (6.0 / 16.0)).astype(dtype)
    hist = hist.astype(np.float64)
    omax = float(hist.max())
    e_h = 3.0 / 16.0 * u + HIST_REL * omax                # error bound of every smoothed bin
    e_max = float(e_h.max())
    idx = np.arange(n)
    dl = (hist - np.roll(hist, 1)) / (e_h + np.roll(e_h, 1))                   # the three peak tests, in units of their error bound
    dr = (hist - np.roll(hist, -1)) / (e_h + np.roll(e_h, -1))
    dt = (hist - ORI_PEAK * omax) / (e_h + ORI_PEAK * e_max)
    out = {}
    for j in idx[(np.minimum(np.minimum(dl, dr), dt) >= -1) & (hist > 0)]:
        l, r2 = (j - 1) % n, (j + 1) % n
        hl, hj, hr = hist[l], hist[j], hist[r2]
        den = hl - 2 * hj + hr
        if den == 0:
            continue
        b = j + 0.5 * (hl - hr) / den
        b = b + n if b < 0 else (b - n if b >= n else b)
        ang = 360.0 - (360.0 / n) * b
        if abs(ang - 360.0) < FLT_EPS:
            ang = 0.0
        # what the error of the three bins can move the interpolated peak by: conditioning (1 / |den|), not a fixed epsilon
        slack = (360.0 / n) * 2.0 * max(e_h[l], e_h[j], e_h[r2]) / abs(den)
        tag = "peak" if min(dl[j], dr[j], dt[j]) <= 1 or slack > ANG_SLACK_MAX else ""
        out[int(j)] = dict(j=int(j), angle=ang, tag=tag, own=bool(hj > hl and hj > hr and hj >= ORI_PEAK * omax), slack=slack, flips=bool(max(u[l], u[j], u[r2]) > 0), tie=-1)
    # two neighbouring bins too close to call, everything else about both clear: one of the two is a peak for certain
    for j in list(out):
        k = (j + 1) % n
        if k in out and abs(dr[j]) <= 1 and min(dl[j], dt[j]) > 1 and min(dr[k], dt[k]) > 1 and max(out[j]["slack"], out[k]["slack"]) <= ANG_SLACK_MAX \
                and out[j]["tie"] < 0 and out[k]["tie"] < 0:
            out[j].update(tag="tie", tie=j)
            out[k].update(tag="tie", tie=j)
    return list(out.values())


# ---- the model -----------------------------------------------------------------------------------------------------------------------------
def detect(img, dtype=np.float64):
    """everything up to removeDuplicatedSorted -> dict(gauss, dog, raw=[keypoint dicts, sorted], zones=[(o, r, c)], n_dropped, shape)"""
    img = np.asarray(img, np.uint8)
    gauss, dog = pyramids(img, dtype)
    merged, zones, n_dropped = {}, [], 0
    for o in range(len(dog)):
        for l, r, c, clear, own in _candidates(dog[o]):
            wk = _Walk(dog[o], gauss[o], o, dtype)
            wk.step(l, r, c, 0, _why((), not clear, 'extremum'), own)
            if wk.wild:
                zones.append((o, r, c))
            n_dropped += not wk.out and not wk.wild
            for k in wk.out:
                k["cand"] = (o, l, r, c)
                key = (k["o"], k["l"], k["r"], k["c"], k["radius"], k["j"])          # the same end point reached twice is one keypoint
                if key in merged:
                    merged[key]["why"] = min(merged[key]["why"], k["why"], key=len)     # certain by one way: certain
                    merged[key]["own"] |= k["own"]
                else:
                    merged[key] = k
    raw = sorted(merged.values(), key=lambda k: key_less_than((k["x"], k["y"], k["size"], k["angle"], k["response"], k["octave"])))
    return dict(gauss=gauss, dog=dog, raw=raw, zones=zones, n_dropped=n_dropped, shape=img.shape)


def _unit(q, k):
    """the key under which keypoint k (number q of the list) counts towards the retainBest cut: alternatives share one key"""
    end = (k["o"], k["l"], k["r"], k["c"])
    if not k["why"]:
        return end + (q,)                                        # certified: itself
    if k["why"] == ("radius",):
        return end + (k["j"], "radius")                          # the two orientation radii of one peak: exactly one exists
    if k["why"] == ("tie",):
        return end + (k["radius"], k["tie"], "tie")              # the two neighbouring bins of one tie: exactly one exists
    return end + k["cand"] + (k["j"], "walk")                    # the ways one candidate's walk may end: at most one exists


def select(det, nfeatures=1000, mask=None):
    """retainBest + runByPixelsMask on a detect() result -> the model result judge_keypoints takes"""
    kps = [dict(k) for k in det["raw"]]
    if nfeatures > 0:
        own = sorted((k["response"] for k in kps if k["own"]), reverse=True)
        cut_own = own[nfeatures - 1] if len(own) > nfeatures else -np.inf
        # alternatives of which exactly one exists (see judge_keypoints), or of one candidate's walk of which at most one does, count once
        units = {}
        for q, k in enumerate(kps):
            units.setdefault(_unit(q, k), []).append(k)
        every = sorted((u[0]["response"] for u in units.values()), reverse=True)
        sure = sorted((u[0]["response"] for u in units.values() if not u[0]["why"] or len(u) == 2), reverse=True)
        cut_hi = every[nfeatures - 1] if len(every) > nfeatures else -np.inf            # the cut can be no higher than this
        cut_lo = sure[nfeatures - 1] if len(sure) > nfeatures else -np.inf              # ... and no lower than this
        kept = []
        for k in kps:
            if k["response"] < cut_lo - 2 * RESP_TOL:
                continue
            k["why"] = _why(k["why"], not k["response"] > cut_hi + 2 * RESP_TOL, "cut")
            k["own"] = k["own"] and k["response"] >= cut_own
            kept.append(k)
        kps = kept
    if mask is not None:
        kept = []
        h, w = det["shape"]
        for k in kps:
            tol = POS_TOL * (1 << k["o"]) * 0.5
            vals = {bool(mask[min(max(int(k["y"] + 0.5 + ey), 0), h - 1), min(max(int(k["x"] + 0.5 + ex), 0), w - 1)])
                    for ex in (-tol, 0.0, tol) for ey in (-tol, 0.0, tol)}
            if vals == {False}:
                continue
            k["why"] = _why(k["why"], len(vals) > 1, "mask")                              # the rounded pixel is within tolerance of the next
            k["own"] = k["own"] and bool(mask[min(int(k["y"] + 0.5), h - 1), min(int(k["x"] + 0.5), w - 1)])
            kept.append(k)
        kps = kept
    return dict(det, kps=kps)


def model(img, nfeatures=1000, mask=None, dtype=np.float64):
    return select(detect(img, dtype), nfeatures, mask)


def own_keypoints(res):
    """the model's own strict answer -> (n, 6) [x, y, size, angle, response, octave]"""
    return np.array([[k["x"], k["y"], k["size"], k["angle"], k["response"], k["octave"]] for k in res["kps"] if k["own"]], np.float64).reshape(-1, 6)


def counts(res):
    c = sum(1 for k in res["kps"] if not k["why"])            # (pairs of orientation radii, see judge_keypoints, not counted)
    return dict(certified=c, marginal=len(res["kps"]) - c, dropped=res["n_dropped"], wild=len(res["zones"]))


# ---- verdicts ------------------------------------------------------------------------------------------------------------------------------
def _ang_diff(a, b):
    return abs((a - b + 180.0) % 360.0 - 180.0)


def _close(k, row):
    """is the reported row the model keypoint k, within the tolerances"""
    oc = int(row[5])
    if (oc & 0xffff) != (k["octave"] & 0xffff) or abs(((oc >> 16) & 255) - ((k["octave"] >> 16) & 255)) > 1:
        return None
    tol = POS_TOL * (1 << k["o"]) * 0.5
    d = (abs(row[0] - k["x"]) / tol, abs(row[1] - k["y"]) / tol, abs(row[2] / k["size"] - 1.0) / SIZE_TOL, abs(row[4] - k["response"]) / RESP_TOL)
    da = _ang_diff(row[3], k["angle"])
    if max(d) > 1.0 or da > ANG_TOL + min(k["slack"], ANG_SLACK_MAX):
        return None
    return max(max(d), da / ANG_TOL)                          # the closest of several candidates is the counterpart


def judge_keypoints(res, kps):
    """the one verdict on a reported (n, 6) keypoint array against a model result.  -> dict(failures, excused (share), certified, reported)
      * every certified keypoint has exactly one counterpart (octave and layer bytes equal, third byte +-1, fields within the tolerances);
      * every reported keypoint has a certified or marginal counterpart (or lies where the model declined to follow an ill-conditioned walk);
      * the reported order is KeyPoint_LessThan."""
    kps = np.asarray(kps, np.float64).reshape(-1, 6)
    fails = []
    mk = res["kps"]
    xs = np.array([k["x"] for k in mk]) if mk else np.zeros(0)
    hits = [0] * len(mk)
    # a keypoint whose one unclear decision is the rounding of the orientation radius exists for certain, with one of two histograms: the
    # two are certified as a pair, exactly one of them has to be reported
    groups = {}
    for q, k in enumerate(mk):
        if k["why"] == ("radius",):
            groups.setdefault((k["o"], k["l"], k["r"], k["c"], k["j"]), []).append(q)
        if k["why"] == ("tie",):                            # ... or one unclear comparison of two neighbouring histogram bins
            groups.setdefault((k["o"], k["l"], k["r"], k["c"], k["radius"], "tie", k["tie"]), []).append(q)
    pairs = [g for g in groups.values() if len(g) == 2]
    pair = {q for g in pairs for q in g}
    excused = 0
    for i, row in enumerate(kps):
        best, best_d = None, None
        for q in np.nonzero(np.abs(xs - row[0]) <= POS_TOL * 4096)[0]:
            d = _close(mk[q], row)
            if d is not None and (best is None or d < best_d):
                best, best_d = int(q), d
        if best is None:
            o = ((int(row[5]) & 255) + 1) & 255
            if any(zo == o and abs(2 * row[0] / (1 << o) - zc) <= 6 and abs(2 * row[1] / (1 << o) - zr) <= 6 for zo, zr, zc in res["zones"]):
                excused += 1
            else:
                fails.append(("no counterpart", i, row.tolist()))
            continue
        hits[best] += 1
        excused += bool(mk[best]["why"]) and best not in pair
    for a, b in pairs:
        if hits[a] + hits[b] != 1:
            fails.append(("one of two alternatives: reported %d times" % (hits[a] + hits[b]), a, b))
    for q, k in enumerate(mk):
        if q in pair:
            continue
        if hits[q] > 1 or (hits[q] == 0 and not k["why"]):
            fails.append(("certified keypoint reported %d times" % hits[q], q, {a: k[a] for a in ("x", "y", "size", "angle", "response", "octave")}))
        excused += hits[q] == 0 and bool(k["why"]) and k["own"]
    keys = [key_less_than(r) for r in kps]
    if any(keys[i] > keys[i + 1] for i in range(len(keys) - 1)):
        fails.append(("order", None, None))
    n_cert = sum(1 for k in mk if not k["why"]) + len(pairs)
    return dict(failures=fails, excused=excused / max(1, len(kps), n_cert), certified=n_cert, reported=len(kps))


def descriptor(gauss, row, dtype=np.float64):
    """calcSIFTDescriptor at the fields of one keypoint row [x, y, size, angle, response, octave] -> (128 values before the final rounding,
    flagged: the window radius is within rounding of the next integer)"""
    oc = int(row[5])
    o = oc & 255
    o = o if o < 128 else o - 256
    layer = (oc >> 8) & 255
    scale = 2.0 ** -o
    img = gauss[o + 1][layer]
    rows, cols = img.shape
    T = dtype
    ori = 360.0 - row[3]
    if abs(ori - 360.0) < FLT_EPS:
        ori = 0.0
    ptx, pty, scl = row[0] * scale, row[1] * scale, row[2] * scale * 0.5
    px, py = int(np.rint(np.float32(ptx))), int(np.rint(np.float32(pty)))
    hw = D_SCL * scl
    t = hw * math.sqrt(2.0) * (D_W + 1) * 0.5
    flagged = abs(t - (math.floor(t) + 0.5)) <= 8 * FLT_EPS * t
    radius = min(int(np.rint(t)), int(math.sqrt(cols * cols + rows * rows)))
    ct, st = T(math.cos(math.radians(ori)) / hw), T(math.sin(math.radians(ori)) / hw)
    ys = np.arange(max(py - radius, 1), min(py + radius, rows - 2) + 1)
    xs = np.arange(max(px - radius, 1), min(px + radius, cols - 2) + 1)
    if len(ys) == 0 or len(xs) == 0:
        return np.zeros(128), flagged
    Y, X = np.meshgrid(ys, xs, indexing="ij")
    fi, fj = (Y - py).ravel().astype(T), (X - px).ravel().astype(T)
    c_rot, r_rot = fj * ct - fi * st, fj * st + fi * ct
    rb, cb = r_rot + T(D_W / 2 - 0.5), c_rot + T(D_W / 2 - 0.5)
    ok = (rb > -1) & (rb < D_W) & (cb > -1) & (cb < D_W)
    Y, X, rb, cb, c_rot, r_rot = Y.ravel()[ok], X.ravel()[ok], rb[ok], cb[ok], c_rot[ok], r_rot[ok]
    dx, dy = img[Y, X + 1] - img[Y, X - 1], img[Y - 1, X] - img[Y + 1, X]
    mag = np.sqrt(dx * dx + dy * dy) * np.exp((c_rot * c_rot + r_rot * r_rot) * T(-1.0 / (D_W * D_W * 0.5)))
    ob = (fast_atan2(dy, dx, T) - T(ori)) * T(D_BINS / 360.0)
    r0, c0, o0 = np.floor(rb), np.floor(cb), np.floor(ob)
    fr, fc, fo = rb - r0, cb - c0, ob - o0
    r0, c0, o0 = r0.astype(np.int64), c0.astype(np.int64), o0.astype(np.int64)
    acc = np.zeros((D_W + 2) * (D_W + 2) * D_BINS)
    for ar, wr in ((0, 1 - fr), (1, fr)):                    # trilinear spreading: 8 corners, orientation circular
        for ac, wc in ((0, 1 - fc), (1, fc)):
            for ao, wo in ((0, 1 - fo), (1, fo)):
                idx = ((r0 + 1 + ar) * (D_W + 2) + (c0 + 1 + ac)) * D_BINS + (o0 + ao) % D_BINS
                acc += np.bincount(idx, weights=(mag * wr * wc * wo).astype(np.float64), minlength=len(acc))
    dst = acc.reshape(D_W + 2, D_W + 2, D_BINS)[1:D_W + 1, 1:D_W + 1].ravel().astype(T)
    thr = np.sqrt((dst * dst).sum()) * T(D_MAG_THR)
    dst = np.minimum(dst, thr)
    dst = dst * (T(D_INT) / max(np.sqrt((dst * dst).sum()), T(FLT_EPS)))
    return np.clip(dst.astype(np.float64), 0.0, 255.0), flagged


def judge_descriptor(res, img, kp_row, desc_row):
    """the model's descriptor AT THE REPORTED keypoint fields against the 128 reported integers -> dict(ok, excused, worst)"""
    del img                                                   # the pyramid of `res` is the image's
    want, flagged = descriptor(res["gauss"], np.asarray(kp_row, np.float64))
    got = np.asarray(desc_row, np.float64)
    integral = bool(np.all(got == np.rint(got)) and got.min() >= 0 and got.max() <= 255)
    worst = float(np.max(np.abs(got - want)))
    return dict(ok=integral and (worst <= DESC_TOL + 0.5 or flagged), excused=bool(flagged and worst > DESC_TOL + 0.5), worst=worst)


def judge_all(res, img, kps, desc):
    """both verdicts over one reported result -> (keypoint verdict, descriptor failures, excused descriptors).  The verdict's `excused` is the
    ONE share the cap applies to: keypoints with a marginal counterpart and keypoints whose descriptor had to be excused, together."""
    jk = judge_keypoints(res, kps)
    bad, exc = [], 0
    for i in range(len(kps)):
        jd = judge_descriptor(res, img, kps[i], desc[i])
        exc += jd["excused"]
        if not jd["ok"]:
            bad.append((i, jd["worst"]))
    jk["excused"] += exc / max(1, len(kps), jk["certified"])
    return jk, bad, exc


# ---- measurements (model32 against model64) ------------------------------------------------------------------------------------------------
def measure(img):
    """-> dict of the largest model32 / model64 differences on one image, and the share of own keypoints that did not pair up"""
    d64, d32 = detect(img, np.float64), detect(img, np.float32)
    out = dict(dog=max(float(np.max(np.abs(a.astype(np.float64) - b))) for a, b in zip(d32["dog"], d64["dog"])),
               gauss=max(float(np.max(np.abs(a.astype(np.float64) - b))) for a, b in zip(d32["gauss"], d64["gauss"])),
               pos=0.0, size=0.0, angle=0.0, response=0.0, desc=0.0, pairs=0, unpaired=0)
    key = lambda k: (k["o"], k["l"], k["r"], k["c"], k["radius"], k["j"])
    a = {key(k): k for k in d64["raw"] if k["own"]}
    b = {key(k): k for k in d32["raw"] if k["own"]}
    for q in a.keys() & b.keys():
        p, s = a[q], b[q]
        sc = (1 << p["o"]) * 0.5
        out["pos"] = max(out["pos"], abs(p["x"] - s["x"]) / sc, abs(p["y"] - s["y"]) / sc)
        out["size"] = max(out["size"], abs(s["size"] / p["size"] - 1))
        if not p["flips"] and not s["flips"]:                # no histogram sample that may change bins: float noise alone (the rest is `slack`)
            out["angle"] = max(out["angle"], _ang_diff(p["angle"], s["angle"]))
        out["response"] = max(out["response"], abs(p["response"] - s["response"]))
        row = [p[f] for f in ("x", "y", "size", "angle", "response", "octave")]
        w64, _ = descriptor(d64["gauss"], row, np.float64)
        w32, _ = descriptor(d32["gauss"], row, np.float32)
        out["desc"] = max(out["desc"], float(np.max(np.abs(np.rint(w64) - np.rint(w32)))))
    out["pairs"] = len(a.keys() & b.keys())
    out["unpaired"] = len(a.keys() ^ b.keys())
    return out


# ---- analytic truths: images and checks shared by the CPU tests (model, oracle) and the GPU tests (kernel) ----------------------------------
BLOBS = [(88, 72, 2.0, -170), (88, 72, 3.0, 160), (88, 72, 3.0, -170), (88, 72, 5.0, 150), (128, 96, 7.0, 180), (128, 96, 7.0, -150),
         (128, 96, 10.0, 160), (128, 96, 10.0, -180)]
BLOB_OCTAVE = {3.0: 0, 7.0: 1, 10.0: 2}       # low byte of the octave field (0 = the image's own resolution)
RAMP_PHI = (0, 30, 77, 135, 200, 290)
ROLL = (16, 8)                                 # x, y: a multiple of 8 keeps every octave's sampling phase down to the fourth


def flat_margin_texture(w=160, h=120, seed=3):
    """a 97 x 61 texture faded into a flat canvas, everything at least 24 px + the roll away from the border"""
    t = texture(97, 61, seed).astype(np.float64)
    wy, wx = np.hanning(61 + 2)[1:-1], np.hanning(97 + 2)[1:-1]
    img = np.full((h, w), 128.0)
    img[24:24 + 61, 24:24 + 97] += np.minimum(1.0, 3.0 * np.outer(wy, wx)) * (t - 128.0) * 2.0
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def truth_images():
    """name -> image, every image of the analytic truths"""
    out = {}
    for w, h, s, amp in BLOBS:
        out["blob %dx%d s=%g amp=%d" % (w, h, s, amp)] = blob_image(w, h, w // 2, h // 2, s, amp)
    out["blob half"] = blob_image(88, 72, 43.5, 35.5, 3.0, 160)
    for phi in RAMP_PHI:
        out["ramp %d" % phi] = ramp_image(phi)
    t = texture(97, 61, 3)
    out["tex"] = t
    out["tex T"] = np.ascontiguousarray(t.T)
    out["tex neg"] = (255 - t).astype(np.uint8)
    m = flat_margin_texture()
    out["margin"] = m
    out["margin rolled"] = np.ascontiguousarray(np.roll(m, (ROLL[1], ROLL[0]), axis=(0, 1)))
    return out


def check_blobs(results):
    """a blob of std s centred on pixel (cx, cy): every keypoint on it sits at (cx + 0.25, cy + 0.25) +- 0.1 with size 2 s / 2^(1/6) +- 3 %
    (the DoG extremum sigma = s / sqrt k, k = 2^(1/3), size = 2 sigma), in the octave that scale belongs to"""
    cases = [("blob %dx%d s=%g amp=%d" % (w, h, s, amp), w // 2, h // 2, s) for w, h, s, amp in BLOBS] + [("blob half", 43.5, 35.5, 3.0)]
    for name, cx, cy, s in cases:
        kp = results[name][0]
        on = kp[np.hypot(kp[:, 0] - cx, kp[:, 1] - cy) < s]
        assert len(on) >= 1, (name, kp)
        assert np.all(np.abs(on[:, 0] - (cx + 0.25)) <= 0.1) and np.all(np.abs(on[:, 1] - (cy + 0.25)) <= 0.1), (name, on)
        assert np.all(np.abs(on[:, 2] / (2.0 * s / 2.0 ** (1.0 / 6.0)) - 1.0) <= 0.03), (name, on)
        if s in BLOB_OCTAVE:
            assert np.all((on[:, 5].astype(np.int64) & 255) == BLOB_OCTAVE[s]), (name, on)


def check_ramps(results):
    """blob on a linear ramp whose gradient points along phi (y down): every angle of the keypoint on the blob is phi +- 25 degrees (uint8
    quantisation makes it noisy; a mirrored or swapped convention is off by 50 degrees or more on at least three of the six)"""
    for phi in RAMP_PHI:
        kp = results["ramp %d" % phi][0]
        on = kp[np.hypot(kp[:, 0] - 63.75, kp[:, 1] - 47.75) < 1.0]
        assert len(on) >= 1, (phi, kp)
        best = on[np.argmax(on[:, 4])]
        assert max(_ang_diff(a, phi) for a in on[on[:, 4] == best[4], 3]) <= 25.0, (phi, on)       # every orientation reported for it


def pair_up(a, b, scale_tol=2.0):
    """pairs rows of two keypoint arrays that should be equal up to two float32 runs' noise (2 x the keypoint tolerances, octave and layer
    bytes equal) -> (pairs [(i, j)], share of the keypoints of either that found no partner)"""
    pairs, used = [], set()
    for i, r in enumerate(a):
        best, bd = None, None
        for j in np.nonzero(np.abs(b[:, 0] - r[0]) < 0.5)[0]:
            q = b[j]
            if j in used or (int(q[5]) & 0xffff) != (int(r[5]) & 0xffff):
                continue
            tol = scale_tol * POS_TOL * 0.5 * 2.0 ** (((int(r[5]) & 255) + 1) & 255)
            d = max(abs(q[0] - r[0]) / tol, abs(q[1] - r[1]) / tol, abs(q[2] / r[2] - 1) / (scale_tol * SIZE_TOL), _ang_diff(q[3], r[3]) / (scale_tol * ANG_TOL),
                    abs(q[4] - r[4]) / (scale_tol * RESP_TOL))
            if d <= 1 and (best is None or d < bd):
                best, bd = int(j), d
        if best is not None:
            used.add(best)
            pairs.append((i, best))
    return pairs, 1.0 - len(pairs) / max(1, max(len(a), len(b)))


# descriptor cell (i, j, k) = (row bin across the keypoint's direction, column bin along it, orientation bin relative to it).  Transposing the
# image mirrors it about the diagonal: the coordinate along the keypoint's direction is kept, the one across it and every relative angle
# change sign -> cell (i, j, k) of the transposed image's descriptor holds cell (3 - i, j, -k mod 8)
TRANSPOSE_PERM = np.array([((D_W - 1 - i) * D_W + j) * D_BINS + (-k) % D_BINS for i in range(D_W) for j in range(D_W) for k in range(D_BINS)])


def check_transpose_negation(results):
    """transposed image: (x, y, size, a) -> (y, x, size, (90 - a) mod 360), descriptor cells permuted; negated image: (x, y, size,
    (a + 180) mod 360), equal responses.  At most EXCUSED_MAX of the keypoints may fail to pair (decision flips of two float runs)."""
    (kp, desc), (kt, dt), (kn, _) = results["tex"], results["tex T"], results["tex neg"]
    assert len(kp) >= 40
    want = kp.copy()
    want[:, 0], want[:, 1], want[:, 3] = kp[:, 1], kp[:, 0], (90.0 - kp[:, 3]) % 360.0
    pairs, missed = pair_up(want, kt)
    assert missed <= EXCUSED_MAX, ("transpose", missed, len(kp), len(kt))
    worst = max(float(np.max(np.abs(desc[i][TRANSPOSE_PERM] - dt[j]))) for i, j in pairs)
    assert worst <= DESC_TOL, ("descriptor under transposition", worst)
    want = kp.copy()
    want[:, 3] = (kp[:, 3] + 180.0) % 360.0
    pairs, missed = pair_up(want, kn)
    assert missed <= EXCUSED_MAX, ("negation", missed, len(kp), len(kn))
    return worst


def check_translation(results, exact):
    """an image with flat margins rolled by ROLL: positions move by exactly that, everything else (and every descriptor) is unchanged --
    bit for bit in float32 implementations (`exact`)"""
    (kp, desc), (kr, dr) = results["margin"], results["margin rolled"]
    octs = set((kp[:, 5].astype(np.int64) & 255).tolist())
    assert len(kp) >= 20 and len(octs) >= 3, (len(kp), octs)
    assert len(kr) == len(kp)
    want = kp.copy()
    want[:, 0] += ROLL[0]
    want[:, 1] += ROLL[1]
    order = np.lexsort((want[:, 3], want[:, 1], want[:, 0]))
    order_r = np.lexsort((kr[:, 3], kr[:, 1], kr[:, 0]))
    a, b = want[order], kr[order_r]
    assert np.max(np.abs(a[:, :2] - b[:, :2])) <= 1e-5, np.max(np.abs(a[:, :2] - b[:, :2]))     # 16 + x in float32: half an ulp of ~150
    if exact:
        assert np.array_equal(a[:, 2:], b[:, 2:]) and np.array_equal(desc[order], dr[order_r])
    else:
        assert np.allclose(a[:, 2:5], b[:, 2:5], rtol=1e-9, atol=1e-9) and np.array_equal(a[:, 5], b[:, 5])
        assert np.max(np.abs(desc[order] - dr[order_r])) <= 1


def model_detect_compute(img, nfeatures=1000, mask=None):
    """the model's own strict answer in the shape of the product call -> keypoints (n, 6), descriptors (n, 128)"""
    res = model(img, nfeatures, mask)
    kp = own_keypoints(res)
    desc = np.array([np.rint(descriptor(res["gauss"], r)[0]) for r in kp]).reshape(-1, 128)
    return kp, desc


# ---- the judged cases, shared by both test files -------------------------------------------------------------------------------------------
def half_mask(shape):
    m = np.full(shape, 255, np.uint8)
    m[:, :shape[1] // 2] = 0
    return m


def cases(name):
    """-> [(label, nfeatures, mask)] judged on image `name`"""
    return [("n=0", 0, None), ("n=50", 50, None), ("n=1000", 1000, None), ("mask", 0, half_mask(image(name).shape))]


def edge_mask(det, most=8):
    """a mask whose edge passes within half a pixel of up to `most` certified keypoints: in the keypoint's own pixel row the edge is put at
    its rounded pixel, alternately just including and just excluding it -> (mask, number of such keypoints)"""
    h, w = det["shape"]
    mask = half_mask((h, w))
    rows, n = set(), 0
    for k in det["raw"]:
        py, px = int(k["y"] + 0.5), int(k["x"] + 0.5)
        if k["why"] or not k["own"] or rows & {py - 1, py, py + 1} or n >= most:
            continue
        mask[py, :] = 255
        mask[py, :px + n % 2] = 0                            # even: the pixel stays set, odd: it is the last one cleared
        rows.add(py)
        n += 1
    return mask, n


def largest_slack(res):
    """the largest angle slack (degrees) a certified keypoint of a model result is granted beyond ANG_TOL"""
    return max([min(k["slack"], ANG_SLACK_MAX) for k in res["kps"] if not k["why"]], default=0.0)
