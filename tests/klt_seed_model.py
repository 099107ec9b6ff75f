"""numpy restatement of pyramidal Lucas-Kanade with OpenCV's OPTFLOW_USE_INITIAL_FLOW: `klt_np(..., init=g)`.

Written in the style of `klt_np` of tests/test_oracle_crosscheck.py (whole-window integer arithmetic on pre-padded level arrays, exact integer
window sums, np.float32 scalars for the 2 x 2 solve in OpenCV's expression order) with the one thing the mode changes:
    at level == top (the highest level actually used):  nextPt = g * (float)(1.0 / (1 << top))   per component, float32
and the project's own rule for what OpenCV leaves undefined: a guess with a component that is not finite starts from p0.  The template
position, the propagation to the lower levels, the skips, the exits, status, err and the iteration counts are those of the unseeded tracker;
a skipped top level passes the scaled guess down as it passes prevPt down.  init=None is the unseeded tracker.

`cv_floor` and `to_int32` are OpenCV's float -> int conversions with x86's answer for NaN and values beyond int32 (INT_MIN) written out, so that
rows with such components run through the model (outside on every level) instead of raising; tests/nonfinite_cases.py holds those rows.

`predict(uv, prev)` is the constant-velocity rule of the resident predictors: g = uv + (uv - prev) in float32, g = uv where prev is missing
(NaN) or not finite."""
import numpy as np
from scipy import ndimage


def pyr_down_np(img):
    k = np.array([1, 4, 6, 4, 1], np.int64)
    a = ndimage.correlate1d(img.astype(np.int64), k, axis=1, mode="mirror")       # scipy 'mirror' = BORDER_REFLECT_101
    a = ndimage.correlate1d(a, k, axis=0, mode="mirror")
    return ((a[::2, ::2] + 128) >> 8).astype(np.uint8)


def scharr_np(img):
    a = img.astype(np.int32)
    sm, df = np.array([3, 10, 3], np.int32), np.array([-1, 0, 1], np.int32)
    ix = ndimage.correlate1d(ndimage.correlate1d(a, sm, axis=0, mode="mirror"), df, axis=1, mode="mirror")
    iy = ndimage.correlate1d(ndimage.correlate1d(a, sm, axis=1, mode="mirror"), df, axis=0, mode="mirror")
    return np.stack([ix, iy], -1).astype(np.int16)


def predict(uv, prev):
    uv, prev = np.asarray(uv, np.float32), np.asarray(prev, np.float32)
    g = uv + (uv - prev)
    bad = ~np.isfinite(prev).all(-1)
    g[bad] = uv[bad]
    return g


MUTANTS = ("int32_sums", "int32_combine", "thr_le", "half_up", "unclamped")


INT_MIN = -(1 << 31)


def cv_floor(x):
    """OpenCV's cvFloor (SSE cvtss2si): floor as a Python int; INT_MIN for NaN and for every value outside [-2^31, 2^31)"""
    x = float(x)
    if not (-2147483648.0 <= x < 2147483648.0):          # NaN fails both comparisons
        return INT_MIN
    return int(np.floor(x))


def to_int32(p):
    """np.int32(p) as x86 computes it (cvttss2si), written out: truncation toward zero; INT_MIN for NaN and for every value outside
    [-2^31, 2^31).  What the reference's disc centres np.int32(kp.uv) become.  p: any shape; -> int32 array of that shape."""
    p = np.asarray(p, np.float32)
    out = np.empty(p.shape, np.int32)
    flat, o = p.reshape(-1), out.reshape(-1)
    for i, v in enumerate(flat):
        v = float(v)
        if not (-2147483648.0 <= v < 2147483648.0):
            o[i] = INT_MIN
        else:
            o[i] = int(v)                                   # Python's int(): toward zero
    return out


def _wrap32(v):
    return ((int(v) + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def klt_np(im0, im1, p0, init=None, win=31, max_level=3, max_count=30, eps=0.03, min_eig_thr=1e-4, trace=None, mutant=None):
    """-> p1 (n, 2) f32, status (n,) u8, err (n,) f32, iters (n, max_level + 1) i32 (-1 = level skipped)
    The criteria are clamped as calcOpticalFlowPyrLK clamps them: max_count to [0, 100], eps to [0, 10].
    trace: a list that receives one dict per (point, level) whose template was formed: pt, level, min_eig (float32), Iw (the interpolated
    template, 5 fractional bits), gx, gy (the interpolated derivatives) and diffs (the difference window of every LK iteration), all int64
    win x win arrays -- what tests/range_cases.py sums lane by lane.  It changes no result.
    mutant: one of MUTANTS, a deliberately WRONG variant for tests/test_range_cases.py to catch:
      int32_sums     the window sums are accumulated in wrapping int32
      int32_combine  the sums are exact as 16-bit halves, but hi * 65536 + lo is formed in wrapping int32 (no float64 branch)
      thr_le         minEig <= threshold rejects
      half_up        the bilinear weights round half up instead of half to even
      unclamped      max_count and eps are used as given"""
    F = np.float32
    assert mutant is None or mutant in MUTANTS
    if mutant != "unclamped":
        max_count = min(max(int(max_count), 0), 100)
        eps = min(max(float(eps), 0.0), 10.0)

    def isum(x):                                   # the window sum that becomes a float
        v = int(x.sum())
        if mutant == "int32_sums":
            return _wrap32(v)
        if mutant == "int32_combine":
            return _wrap32((v >> 16) * 65536 + (v & 0xFFFF))
        return v
    p0 = np.asarray(p0, np.float32).reshape(-1, 2)
    lv0, lv1 = [im0], [im1]
    while len(lv0) <= max_level:
        h, w = lv0[-1].shape
        if (w + 1) // 2 <= win or (h + 1) // 2 <= win:
            break
        lv0.append(pyr_down_np(lv0[-1])); lv1.append(pyr_down_np(lv1[-1]))
    top = len(lv0) - 1
    pad = win + 2
    I = [np.pad(a.astype(np.int64), pad, mode="reflect") for a in lv0]
    J = [np.pad(a.astype(np.int64), pad, mode="reflect") for a in lv1]
    D = [np.pad(scharr_np(a).astype(np.int64), ((pad, pad), (pad, pad), (0, 0))) for a in lv0]
    n = len(p0)
    start = p0.copy()
    if init is not None:
        g = np.asarray(init, np.float32).reshape(-1, 2)
        assert g.shape == p0.shape
        fin = np.isfinite(g).all(-1)
        start[fin] = g[fin]                        # a guess that is not finite: the point starts from p0
    p1 = np.zeros((n, 2), np.float32)
    status = np.ones(n, np.uint8)
    err = np.zeros(n, np.float32)
    iters = np.full((n, max_level + 1), -1, np.int32)
    half, scale20, eps2 = F((win - 1) * 0.5), F(1.0 / (1 << 20)), float(eps) * float(eps)

    rnd = (lambda x: np.floor(x + F(0.5))) if mutant == "half_up" else np.rint

    def weights(a, b):
        w00 = int(rnd((F(1) - a) * (F(1) - b) * F(1 << 14)))
        w01 = int(rnd(a * (F(1) - b) * F(1 << 14)))
        w10 = int(rnd((F(1) - a) * b * F(1 << 14)))
        return w00, w01, w10, (1 << 14) - w00 - w01 - w10

    def sample(P, wts, shift):                     # P: (win + 1, win + 1[, c]) int64
        s = P[:-1, :-1] * wts[0] + P[:-1, 1:] * wts[1] + P[1:, :-1] * wts[2] + P[1:, 1:] * wts[3]
        return (s + (1 << (shift - 1))) >> shift

    def window(A, ix, iy):
        return A[iy + pad: iy + pad + win + 1, ix + pad: ix + pad + win + 1]

    def outside(ix, iy, cols, rows):               # (NaN and floats beyond the int range are INT_MIN through cv_floor: outside)
        return ix < -win or ix >= cols or iy < -win or iy >= rows

    for level in range(top, -1, -1):
        rows, cols = lv0[level].shape
        s = F(1.0 / (1 << level))
        for pt in range(n):
            prevx, prevy = F(p0[pt, 0]) * s, F(p0[pt, 1]) * s
            if level == top:
                nextx, nexty = F(start[pt, 0]) * s, F(start[pt, 1]) * s
            else:
                nextx, nexty = p1[pt, 0] * F(2), p1[pt, 1] * F(2)
            p1[pt] = (nextx, nexty)
            prevx, prevy = prevx - half, prevy - half
            ipx, ipy = cv_floor(prevx), cv_floor(prevy)
            if outside(ipx, ipy, cols, rows):
                if level == 0:
                    status[pt], err[pt] = 0, 0
                continue
            wts = weights(prevx - F(ipx), prevy - F(ipy))
            Iw = sample(window(I[level], ipx, ipy), wts, 14 - 5)
            dI = sample(window(D[level], ipx, ipy), wts, 14)
            gx, gy = dI[..., 0], dI[..., 1]
            A11, A12, A22 = F(isum(gx * gx)) * scale20, F(isum(gx * gy)) * scale20, F(isum(gy * gy)) * scale20
            det = A11 * A22 - A12 * A12
            min_eig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + F(4) * A12 * A12)) / F(2 * win * win)
            rec = None
            if trace is not None:
                rec = dict(pt=pt, level=level, min_eig=min_eig, Iw=Iw, gx=gx, gy=gy, diffs=[])
                trace.append(rec)
            low = (min_eig <= F(min_eig_thr)) if mutant == "thr_le" else (min_eig < F(min_eig_thr))
            if low or det < F(1.1920929e-07):
                if level == 0:
                    status[pt] = 0
                continue
            det = F(1) / det
            nextx, nexty = nextx - half, nexty - half
            pdx = pdy = F(0)
            j = 0
            while j < max_count:
                inx, iny = cv_floor(nextx), cv_floor(nexty)
                if outside(inx, iny, cols, rows):
                    if level == 0:
                        status[pt] = 0
                    break
                diff = sample(window(J[level], inx, iny), weights(nextx - F(inx), nexty - F(iny)), 14 - 5) - Iw
                if rec is not None:
                    rec["diffs"].append(diff)
                b1, b2 = F(isum(diff * gx)) * scale20, F(isum(diff * gy)) * scale20
                dx = (A12 * b2 - A22 * b1) * det
                dy = (A12 * b1 - A11 * b2) * det
                nextx, nexty = nextx + dx, nexty + dy
                p1[pt] = (nextx + half, nexty + half)
                if float(dx) * float(dx) + float(dy) * float(dy) <= eps2:
                    j += 1
                    break
                if j > 0 and abs(float(dx + pdx)) < 0.01 and abs(float(dy + pdy)) < 0.01:
                    p1[pt, 0] -= dx * F(0.5); p1[pt, 1] -= dy * F(0.5)
                    j += 1
                    break
                pdx, pdy = dx, dy
                j += 1
            iters[pt, level] = j
            if status[pt] and level == 0:
                nx, ny = p1[pt, 0] - half, p1[pt, 1] - half
                inx, iny = cv_floor(nx), cv_floor(ny)
                if outside(inx, iny, cols, rows):
                    status[pt] = 0
                    continue
                diff = sample(window(J[level], inx, iny), weights(nx - F(inx), ny - F(iny)), 14 - 5) - Iw
                err[pt] = F(isum(np.abs(diff))) * F(1) / F(32 * win * win)
    return p1, status, err, iters
