"""numpy restatement of sub-pixel corner refinement: `corner_subpix_np(img, corners, win, zero, max_count, eps)`.

The algorithm is OpenCV 4.4's cv2.cornerSubPix (imgproc/cornersubpix.cpp) with its getRectSubPix 8u -> 32f patch, written out operation by
operation in the order k_corner_subpix (csrc/vo_subpix.hip) evaluates it; this file is the definition the kernel is pinned to bit for bit.

    mask[i][j] = vy * vx,  v = (f32)exp((f64)(-t * t)),  t = (f32)(i - half) / (f32)half; an optional zero zone in the middle
    per corner, cT = the input, cI = cT; repeat
      S = (wh + 2) x (ww + 2) bilinear samples of the u8 image around cI in f32, coordinates clamped to the image (replicate border)
      tgx, tgy = central differences of S (f32), promoted to f64; with m = mask: gxx = tgx*tgx*m, gxy = tgx*tgy*m, gyy = tgy*tgy*m
      a, b, c, bb1, bb2 = sums over the window of gxx, gxy, gyy, gxx*px + gxy*py, gxy*px + gyy*py   (f64, in the WAVE order below)
      det = a*c - b*b;  |det| <= DBL_EPSILON^2: stop (flag 1)
      cI2 = cI + (c*bb1 - b*bb2, -b*bb1 + a*bb2) / det  rounded to f32;  err = |cI2 - cI|^2 in f32;  cI = cI2
      cI not inside [0, W) x [0, H): stop (flag 2), the iteration is not counted
      iters++;  go on while iters < max_count and err > eps^2
    afterwards: cI further than win from cT on either axis (or not a number) -> the result is cT (flag 3)
A corner with a component that is not finite, or outside [0, W) x [0, H), comes back unchanged with iters = 0 (flag 4): OpenCV asserts there.

The wave order of the sums: lane l of 64 adds its window pixels k = l, l + 64, l + 128, l + 192 (raster index k = i*ww + j) to 0.0 in
ascending k, then v = v + shfl_xor(v, off) for off = 32, 16, 8, 4, 2, 1.  order="raster" sums k = 0, 1, 2, ... instead (a test shows the
outputs do not depend on it on the test images).

Also here: the images and corner sets the tests share (rotated checkerboards with known corners, band-limited noise)."""
import numpy as np
from scipy import ndimage

F = np.float32
DBL_EPS2 = np.finfo(np.float64).eps ** 2
DEFAULTS = dict(win=(5, 5), zero=(-1, -1), max_count=40, eps=0.001)


def mask_table(win, zero=(-1, -1)):
    """[wh][ww] float32"""
    wx, wy = int(win[0]), int(win[1])
    zx, zy = int(zero[0]), int(zero[1])
    ww, wh = 2 * wx + 1, 2 * wy + 1

    def axis(n, half):
        t = (np.arange(n) - half).astype(F) / F(half)
        return np.exp((-(t * t)).astype(np.float64)).astype(F)

    m = (axis(wh, wy)[:, None] * axis(ww, wx)[None, :]).astype(F)
    if zx >= 0 and zy >= 0 and 2 * zx + 1 < ww and 2 * zy + 1 < wh:
        m[wy - zy:wy + zy + 1, wx - zx:wx + zx + 1] = 0
    return m


def _wave_sum(terms):
    """terms (n,) f64 in raster order, n <= 256 -> the butterfly's value (identical in every lane)"""
    v = np.zeros(64, np.float64)
    for base in range(0, len(terms), 64):
        chunk = terms[base:base + 64]
        v[:len(chunk)] = v[:len(chunk)] + chunk
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[lanes ^ off]
    return v[0]


def _raster_sum(terms):
    return np.cumsum(np.concatenate([[0.0], terms]))[-1]        # (cumsum adds one by one; np.sum does not)


def _patch(img, cx, cy, ww, wh):
    """(wh + 2) x (ww + 2) float32 samples around (cx, cy): getRectSubPix 8u -> 32f with a replicate border"""
    H, W = img.shape
    x0 = F(cx - F((ww + 1) * 0.5)); y0 = F(cy - F((wh + 1) * 0.5))
    ix = int(np.floor(x0)); iy = int(np.floor(y0))
    a = F(x0 - F(ix)); b = F(y0 - F(iy))
    one = F(1)
    a11 = F((one - a) * (one - b)); a12 = F(a * (one - b)); a21 = F((one - a) * b); a22 = F(a * b)
    xs0 = np.clip(ix + np.arange(ww + 2), 0, W - 1); xs1 = np.clip(ix + 1 + np.arange(ww + 2), 0, W - 1)
    ys0 = np.clip(iy + np.arange(wh + 2), 0, H - 1); ys1 = np.clip(iy + 1 + np.arange(wh + 2), 0, H - 1)
    p00 = img[np.ix_(ys0, xs0)].astype(F); p01 = img[np.ix_(ys0, xs1)].astype(F)
    p10 = img[np.ix_(ys1, xs0)].astype(F); p11 = img[np.ix_(ys1, xs1)].astype(F)
    return ((p00 * a11 + p01 * a12) + p10 * a21) + p11 * a22


def corner_subpix_np(img, corners, win=(5, 5), zero=(-1, -1), max_count=40, eps=0.001, order="wave"):
    """img (H, W) uint8, corners (n, 2) -> out (n, 2) f32, iters (n,) i32, flags (n,) u8
    flags: 0 ran to a stopping test, 1 singular, 2 left the image, 3 reverted to the input, 4 input not usable"""
    img = np.ascontiguousarray(img, np.uint8)
    H, W = img.shape
    corners = np.asarray(corners, F).reshape(-1, 2)
    wx, wy = int(win[0]), int(win[1])
    assert 1 <= wx <= 7 and 1 <= wy <= 7 and W >= 2 * wx + 5 and H >= 2 * wy + 5
    ww, wh = 2 * wx + 1, 2 * wy + 1
    max_count = min(max(int(max_count), 1), 100)
    e = F(max(float(eps), 0.0))
    eps2 = F(e * e)
    m = mask_table(win, zero).astype(np.float64).ravel()
    px = np.tile(np.arange(ww) - wx, wh).astype(np.float64)
    py = np.repeat(np.arange(wh) - wy, ww).astype(np.float64)
    total = _wave_sum if order == "wave" else _raster_sum
    out = corners.copy()
    iters = np.zeros(len(corners), np.int32)
    flags = np.zeros(len(corners), np.uint8)
    Wf, Hf = F(W), F(H)
    for n, (tx, ty) in enumerate(corners):
        if not (np.isfinite(tx) and np.isfinite(ty) and tx >= 0 and tx < Wf and ty >= 0 and ty < Hf):
            flags[n] = 4
            continue
        cx, cy = F(tx), F(ty)
        it, flag = 0, 0
        while True:
            S = _patch(img, cx, cy, ww, wh)
            tgx = (S[1:-1, 2:] - S[1:-1, :-2]).astype(np.float64).ravel()
            tgy = (S[2:, 1:-1] - S[:-2, 1:-1]).astype(np.float64).ravel()
            gxx = tgx * tgx * m; gxy = tgx * tgy * m; gyy = tgy * tgy * m
            a = total(gxx); b = total(gxy); c = total(gyy)
            bb1 = total(gxx * px + gxy * py); bb2 = total(gxy * px + gyy * py)
            det = a * c - b * b
            if abs(det) <= DBL_EPS2:
                flag = 1
                break
            scale = 1.0 / det
            with np.errstate(over="ignore"):
                nx = F(np.float64(cx) + c * scale * bb1 - b * scale * bb2)
                ny = F(np.float64(cy) - b * scale * bb1 + a * scale * bb2)
                dx = F(nx - cx); dy = F(ny - cy)
                err = F(F(dx * dx) + F(dy * dy))
            cx, cy = nx, ny
            if not (cx >= 0 and cx < Wf and cy >= 0 and cy < Hf):
                flag = 2
                break
            it += 1
            if not (it < max_count and err > eps2):
                break
        with np.errstate(invalid="ignore"):
            if not (abs(F(cx - tx)) <= F(wx) and abs(F(cy - ty)) <= F(wy)):
                cx, cy, flag = tx, ty, 3
        out[n] = (cx, cy)
        iters[n] = it
        flags[n] = flag
    return out, iters, flags


# ---- shared test images -------------------------------------------------------------------------------------------------------------
def checkerboard(w, h, square, angle, ss=8, lo=50.0, hi=200.0):
    """rotated checkerboard rendered by ss x ss supersampling (pixel (x, y) covers [x - 0.5, x + 0.5)^2) -> img (h, w) u8 and the true
    inner corners (n, 2) f64 that lie >= 8 px from the border.  Grid origin: the image centre + (0.3, -0.4)."""
    ox, oy = (w - 1) * 0.5 + 0.3, (h - 1) * 0.5 - 0.4
    ca, sa = np.cos(angle), np.sin(angle)
    sub = (np.arange(ss) + 0.5) / ss - 0.5
    xs = (np.arange(w)[:, None] + sub[None, :]).ravel() - ox
    ys = (np.arange(h)[:, None] + sub[None, :]).ravel() - oy
    X, Y = np.meshgrid(xs, ys)
    u = ca * X + sa * Y
    v = -sa * X + ca * Y
    cell = (np.floor(u / square) + np.floor(v / square)).astype(np.int64) & 1
    val = np.where(cell == 1, hi, lo).reshape(h, ss, w, ss).mean(axis=(1, 3))
    img = np.clip(np.rint(val), 0, 255).astype(np.uint8)
    r = int(np.hypot(w, h) / square) + 2
    gi, gj = np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1))
    gu, gv = gi.ravel() * float(square), gj.ravel() * float(square)
    cx = ca * gu - sa * gv + ox
    cy = sa * gu + ca * gv + oy
    ok = (cx >= 8) & (cx <= w - 1 - 8) & (cy >= 8) & (cy <= h - 1 - 8)
    return img, np.stack([cx[ok], cy[ok]], -1)


def board_starts(truth, seed):
    """integer start positions: the truth + uniform +-1.5 px, rounded"""
    rng = np.random.default_rng(seed)
    return np.rint(truth + rng.uniform(-1.5, 1.5, truth.shape)).astype(F)


def noise_image(w=320, h=240, seed=5):
    """band-limited noise: white noise through Gaussians sigma = 2 plus 1.5 x sigma = 6, mean 128, std 40"""
    rng = np.random.default_rng(seed)
    z = rng.standard_normal((h, w))
    f = ndimage.gaussian_filter(z, 2.0, mode="reflect") + 1.5 * ndimage.gaussian_filter(z, 6.0, mode="reflect")
    f = (f - f.mean()) / f.std()
    return np.clip(np.rint(128.0 + 40.0 * f), 0, 255).astype(np.uint8)


def eig_maxima(img, block=5, nms=15):
    """integer corners (n, 2) f32 at the nms x nms maxima of a min-eigenvalue map (Sobel gradients, block x block sums, reflected border).
    No margin: maxima on the image's edge rows are corners too, and they are the ones a refinement step can carry out of the image."""
    a = img.astype(np.float64)
    ix = ndimage.sobel(a, axis=1, mode="mirror"); iy = ndimage.sobel(a, axis=0, mode="mirror")
    sxx = ndimage.uniform_filter(ix * ix, block, mode="mirror")
    sxy = ndimage.uniform_filter(ix * iy, block, mode="mirror")
    syy = ndimage.uniform_filter(iy * iy, block, mode="mirror")
    eig = 0.5 * (sxx + syy) - np.sqrt(0.25 * (sxx - syy) ** 2 + sxy * sxy)
    peak = (eig == ndimage.maximum_filter(eig, nms, mode="mirror")) & (eig > 0)
    ys, xs = np.nonzero(peak)
    return np.stack([xs, ys], -1).astype(F)
