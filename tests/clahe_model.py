"""numpy model of the CLAHE contrast equalisation (csrc/vo_clahe.hip): the definition the HIP path is pinned to, bit for bit.

It restates cv2.createCLAHE(clipLimit, tileGridSize).apply(img) of OpenCV 4.4 (imgproc/clahe.cpp), 8-bit path, histSize = 256.

    clip_limit (double, OpenCV's default 40.0), tiles = (tiles_x, tiles_y) (OpenCV's default (8, 8)), image w x h uint8

  1. extension.  w % tiles_x == 0 and h % tiles_y == 0: the tiles cut the image itself.  Otherwise the image is extended on the right by
     tiles_x - w % tiles_x columns AND at the bottom by tiles_y - h % tiles_y rows, BORDER_REFLECT_101 (.. c b | a b c .. y z | y x ..,
     the edge pixel not repeated).  OpenCV applies both amounts whenever either remainder is non-zero, so an axis that divides exactly is
     still extended by a whole tiles_* pixels: 1241 x 376 with 8 x 8 tiles becomes 1248 x 384, tile 156 x 48.  (Both amounts must be smaller
     than the image side on their axis.)  tw = ext_w / tiles_x, th = ext_h / tiles_y, area = tw th.
  2. clip limit.  clip_limit > 0: clip = max((int)(clip_limit * area / 256), 1), the product in double, truncated (a quotient above `area`
     is taken as `area` before the truncation: no bin exceeds area, so nothing changes and the conversion cannot overflow).
     clip_limit == 0: no clipping (plain adaptive equalisation).
  3. per tile.  hist[256] (int32) over the tile's `area` pixels of the extended image.  When clipping: clipped = sum max(hist[i] - clip, 0),
     every bin cut to clip; batch = clipped / 256 added to every bin; residual = clipped - 256 batch; residual != 0: step =
     max(256 / residual, 1) and hist[k step] += 1 for k = 0 .. residual - 1 while k step < 256 (bin i gets the one iff i % step == 0 and
     i / step < residual).  lut_scale = (float)255 / (float)area (ONE float32 division);
     lut[i] = clamp(rint((float)sum_{j <= i} hist[j] * lut_scale), 0, 255): the int32 running sum converted to float32 (round to nearest),
     a float32 product, rint = half to even.
  4. per output pixel (x, y) of the ORIGINAL w x h image with value v, all float32, every operation on its own (no fused multiply-add):
     inv_tw = 1.0f / tw; txf = (float)x * inv_tw - 0.5f; tx1 = floor(txf); xa = txf - tx1; xa1 = 1.0f - xa; THEN tx2 = min(tx1 + 1,
     tiles_x - 1), tx1 = max(tx1, 0) (the weights are taken before the clamps).  The same in y: ty1, ty2, ya, ya1.
     res = (lut[ty1][tx1][v] xa1 + lut[ty1][tx2][v] xa) ya1 + (lut[ty2][tx1][v] xa1 + lut[ty2][tx2][v] xa) ya;
     dst = clamp(rint(res), 0, 255).

No OpenCV source or binary was at hand when this was written: parity is with this restatement (the position use_harris and vo_set_undistort
take in include/vo_mi355x.h).  tests/test_clahe_model.py compares with a live cv2 where one is importable.
"""
import numpy as np

F = np.float32


def geometry(w, h, tiles):
    """-> dict(ext_w, ext_h, tw, th, area)"""
    tx, ty = int(tiles[0]), int(tiles[1])
    assert tx >= 1 and ty >= 1
    if w % tx == 0 and h % ty == 0:
        ew, eh = w, h
    else:
        ew, eh = w + (tx - w % tx), h + (ty - h % ty)          # both, whenever either remainder is non-zero
    assert ew - w < w and eh - h < h, "reflect-101 needs an extension smaller than the image"
    tw, th = ew // tx, eh // ty
    return dict(ext_w=ew, ext_h=eh, tw=tw, th=th, area=tw * th)


def extend(img, tiles):
    """the extended image (BORDER_REFLECT_101 on the right and at the bottom)"""
    img = np.asarray(img)
    h, w = img.shape
    g = geometry(w, h, tiles)
    return np.pad(img, ((0, g["ext_h"] - h), (0, g["ext_w"] - w)), mode="reflect")     # numpy's "reflect" does not repeat the edge


def clip_value(clip_limit, area):
    """the integer clip of step 2; 0 = no clipping"""
    clip_limit = float(clip_limit)
    assert np.isfinite(clip_limit) and clip_limit >= 0
    if clip_limit == 0.0:
        return 0
    return max(int(min(clip_limit * area / 256, float(area))), 1)


def luts(img, clip_limit=40.0, tiles=(8, 8)):
    """uint8 [tiles_y][tiles_x][256]"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    h, w = img.shape
    tx, ty = int(tiles[0]), int(tiles[1])
    g = geometry(w, h, tiles)
    tw, th, area = g["tw"], g["th"], g["area"]
    t = extend(img, tiles).reshape(ty, th, tx, tw).transpose(0, 2, 1, 3).reshape(ty * tx, area).astype(np.int64)
    flat = (t + 256 * np.arange(ty * tx)[:, None]).reshape(-1)
    hist = np.bincount(flat, minlength=256 * ty * tx).reshape(ty * tx, 256).astype(np.int32)
    clip = clip_value(clip_limit, area)
    if clip > 0:
        clipped = np.maximum(hist - clip, 0).sum(axis=1, dtype=np.int32)
        hist = np.minimum(hist, clip)
        batch = clipped // 256
        residual = clipped - 256 * batch
        hist = hist + batch[:, None]
        step = np.maximum(256 // np.maximum(residual, 1), 1)
        i = np.arange(256, dtype=np.int32)[None, :]
        extra = (residual[:, None] != 0) & (i % step[:, None] == 0) & (i // step[:, None] < residual[:, None])
        hist = (hist + extra).astype(np.int32)
    lut_scale = F(255) / F(area)
    cum = np.cumsum(hist, axis=1, dtype=np.int32)
    lut = np.clip(np.rint(cum.astype(F) * lut_scale), 0, 255).astype(np.uint8)
    return lut.reshape(ty, tx, 256)


def _axis(n, tile, tiles):
    """one axis of step 4: i1, i2 (int), a, a1 (float32) for the n output coordinates"""
    inv = F(1) / F(tile)
    f = np.arange(n).astype(F) * inv - F(0.5)
    fl = np.floor(f)
    a = f - fl
    a1 = F(1) - a
    i1 = fl.astype(np.int64)
    i2 = np.minimum(i1 + 1, tiles - 1)
    i1 = np.maximum(i1, 0)
    assert a.dtype == F and a1.dtype == F
    return i1, i2, a, a1


def interpolate(img, lut, tiles):
    """step 4 with the given tables"""
    img = np.asarray(img)
    h, w = img.shape
    tx, ty = int(tiles[0]), int(tiles[1])
    g = geometry(w, h, tiles)
    x1, x2, xa, xa1 = _axis(w, g["tw"], tx)
    y1, y2, ya, ya1 = _axis(h, g["th"], ty)
    L = lut.astype(F)
    v = img.astype(np.int64)
    p11, p12 = L[y1[:, None], x1[None, :], v], L[y1[:, None], x2[None, :], v]
    p21, p22 = L[y2[:, None], x1[None, :], v], L[y2[:, None], x2[None, :], v]
    xa, xa1, ya, ya1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    res = (p11 * xa1 + p12 * xa) * ya1 + (p21 * xa1 + p22 * xa) * ya
    assert res.dtype == F
    return np.clip(np.rint(res), 0, 255).astype(np.uint8)


def clahe(img, clip_limit=40.0, tiles=(8, 8)):
    """cv2.createCLAHE(clip_limit, tiles).apply(img) as restated above: uint8 [h, w] -> uint8 [h, w]"""
    return interpolate(img, luts(img, clip_limit, tiles), tiles)
