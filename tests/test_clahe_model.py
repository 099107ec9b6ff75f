"""CPU-only: the numpy model of CLAHE (tests/clahe_model.py) is what it says it is.

The GPU tests (test_gpu_clahe.py) pin the HIP path to the model bit for bit; these pin the model: against a second restatement written as
plain loops (tile by tile and pixel by pixel, as OpenCV's two loop bodies go), against global equalisation at one tile, the extension quirk,
the tables' monotonicity and end value, and against a live cv2 where a real one is importable (the stub under oracle/ref_stub has no
createCLAHE and does not count).  No real cv2 was on the machine this was written on, so the last comparison has never run there: it is
skipped, not passed."""
import math

import numpy as np
import pytest

import clahe_model as cm

F = np.float32
# (w, h, tiles): the shapes of the GPU tests -- no extension; width remainder; height remainder; non-default tiles; one tile; 16 x 16 small tiles
SHAPES = [(96, 64, (8, 8)), (99, 64, (8, 8)), (96, 61, (8, 8)), (101, 67, (4, 3)), (101, 67, (1, 1)), (99, 67, (16, 16))]
IDS = ["%dx%d_%dx%d" % (w, h, t[0], t[1]) for w, h, t in SHAPES]
CLIPS = (0.0, 0.5, 2.0, 40.0)


def images(w, h):
    rng = np.random.default_rng(w * 1000 + h)
    yy, xx = np.mgrid[0:h, 0:w]
    return dict(zeros=np.zeros((h, w), np.uint8),
                full=np.full((h, w), 255, np.uint8),
                checker=np.where(((xx // 5) + (yy // 3)) % 2 == 0, 40, 200).astype(np.uint8),
                ramp=np.tile((np.arange(w) * 255 // (w - 1)).astype(np.uint8), (h, 1)),
                noise=rng.integers(0, 256, (h, w)).astype(np.uint8),
                narrow=rng.integers(100, 111, (h, w)).astype(np.uint8))


# ---- the second restatement: plain loops ---------------------------------------------------------------------------------------------
def _reflect101(i, n):
    return i if i < n else 2 * n - 2 - i


def loop_clahe(img, clip_limit, tiles):
    """-> (lut [ty][tx][256], dst): python ints for the integer part, numpy float32 scalars for the float part, one operation per line"""
    h, w = img.shape
    tx_n, ty_n = tiles
    if w % tx_n == 0 and h % ty_n == 0:
        ew, eh = w, h
    else:
        ew, eh = w + tx_n - w % tx_n, h + ty_n - h % ty_n
    tw, th = ew // tx_n, eh // ty_n
    area = tw * th
    clip = 0
    if clip_limit > 0:
        clip = max(int(clip_limit * area / 256), 1)
    src = img.tolist()
    lut = np.zeros((ty_n, tx_n, 256), np.uint8)
    scale = F(255) / F(area)
    for ty in range(ty_n):
        for tx in range(tx_n):
            hist = [0] * 256
            for y in range(ty * th, (ty + 1) * th):
                row = src[_reflect101(y, h)]
                for x in range(tx * tw, (tx + 1) * tw):
                    hist[row[_reflect101(x, w)]] += 1
            if clip > 0:
                clipped = 0
                for i in range(256):
                    if hist[i] > clip:
                        clipped += hist[i] - clip
                        hist[i] = clip
                batch = clipped // 256
                residual = clipped - batch * 256
                for i in range(256):
                    hist[i] += batch
                if residual != 0:
                    step = max(256 // residual, 1)
                    i = 0
                    while i < 256 and residual > 0:
                        hist[i] += 1
                        i += step
                        residual -= 1
            s = 0
            for i in range(256):
                s += hist[i]
                v = np.rint(F(s) * scale)
                lut[ty, tx, i] = min(max(int(v), 0), 255)
    dst = np.zeros((h, w), np.uint8)
    inv_tw, inv_th = F(1) / F(tw), F(1) / F(th)
    half, one = F(0.5), F(1)
    for y in range(h):
        tyf = F(y) * inv_th
        tyf = tyf - half
        ty1 = math.floor(tyf)
        ya = tyf - F(ty1)
        ya1 = one - ya
        ty2 = min(ty1 + 1, ty_n - 1)
        ty1 = max(ty1, 0)
        for x in range(w):
            txf = F(x) * inv_tw
            txf = txf - half
            tx1 = math.floor(txf)
            xa = txf - F(tx1)
            xa1 = one - xa
            tx2 = min(tx1 + 1, tx_n - 1)
            tx1 = max(tx1, 0)
            v = src[y][x]
            a = F(lut[ty1, tx1, v]) * xa1
            b = F(lut[ty1, tx2, v]) * xa
            c = F(lut[ty2, tx1, v]) * xa1
            d = F(lut[ty2, tx2, v]) * xa
            top = (a + b) * ya1
            bot = (c + d) * ya
            res = top + bot
            assert type(res) is F
            dst[y, x] = min(max(int(np.rint(res)), 0), 255)
    return lut, dst


@pytest.mark.parametrize("w,h,tiles", SHAPES, ids=IDS)
def test_model_equals_a_plain_loop_restatement(w, h, tiles):
    ims = images(w, h)
    # every image at one clip limit each way round, and the two that clipping reshapes most at every clip limit
    runs = [(k, c) for k, c in zip(("zeros", "full", "checker", "ramp"), CLIPS)] + [(k, c) for k in ("noise", "narrow") for c in CLIPS]
    for name, clip in runs:
        lut, dst = loop_clahe(ims[name], clip, tiles)
        got_lut = cm.luts(ims[name], clip, tiles)
        assert np.array_equal(got_lut, lut), (name, clip, int((got_lut != lut).sum()))
        got = cm.clahe(ims[name], clip, tiles)
        assert got.dtype == np.uint8 and np.array_equal(got, dst), (name, clip, int((got != dst).sum()))


def test_one_tile_without_clipping_is_global_equalisation():
    for w, h in ((96, 64), (101, 67)):
        for name, img in images(w, h).items():
            cum = np.cumsum(np.bincount(img.reshape(-1), minlength=256)).astype(np.int32)
            lut = np.clip(np.rint(cum.astype(F) * (F(255) / F(w * h))), 0, 255).astype(np.uint8)
            assert np.array_equal(cm.luts(img, 0.0, (1, 1))[0, 0], lut), name
            assert np.array_equal(cm.clahe(img, 0.0, (1, 1)), lut[img]), name


def test_the_extension_quirk():
    g = cm.geometry(99, 64, (8, 8))
    assert (g["tw"], g["th"], g["ext_w"], g["ext_h"]) == (13, 9, 104, 72)          # the height divides and is STILL extended, by 8 rows
    g = cm.geometry(96, 64, (8, 8))
    assert (g["tw"], g["th"], g["ext_w"], g["ext_h"]) == (12, 8, 96, 64)
    g = cm.geometry(1241, 376, (8, 8))
    assert (g["tw"], g["th"], g["ext_w"], g["ext_h"]) == (156, 48, 1248, 384)
    img = images(99, 64)["noise"]
    e = cm.extend(img, (8, 8))
    assert e.shape == (72, 104) and np.array_equal(e[:64, :99], img)
    assert np.array_equal(e[:64, 99], img[:, 97]) and np.array_equal(e[:64, 103], img[:, 93])       # .. y z | y x ..: the edge is not repeated
    assert np.array_equal(e[64, :99], img[62]) and np.array_equal(e[71, :99], img[55])
    assert e[71, 103] == img[55, 93]
    # the last tile row's table is the histogram of rows 63 .. 71 of the EXTENDED image (one real row and eight reflected ones)
    cum = np.cumsum(np.bincount(e[63:72, 0:13].reshape(-1), minlength=256)).astype(np.int32)
    assert np.array_equal(cm.luts(img, 0.0, (8, 8))[7, 0], np.clip(np.rint(cum.astype(F) * (F(255) / F(117))), 0, 255).astype(np.uint8))


@pytest.mark.parametrize("w,h,tiles", SHAPES, ids=IDS)
def test_every_table_is_monotone_and_ends_at_the_scaled_area(w, h, tiles):
    area = cm.geometry(w, h, tiles)["area"]
    end = int(np.rint(F(area) * (F(255) / F(area))))
    for name, img in images(w, h).items():
        for clip in CLIPS:
            lut = cm.luts(img, clip, tiles).astype(np.int64)
            assert np.all(np.diff(lut, axis=-1) >= 0), (name, clip)
            assert np.all(lut[..., 255] == end), (name, clip)


def test_clip_value():
    assert cm.clip_value(0.0, 35) == 0
    assert cm.clip_value(0.5, 35) == 1 and cm.clip_value(2.0, 35) == 1          # the floor of 1: 0.5 * 35 / 256 < 1
    assert cm.clip_value(40.0, 35) == 5 and cm.clip_value(40.0, 156 * 48) == 1170
    assert cm.clip_value(1e300, 35) == 35                                        # capped at area: no bin is larger


def test_the_small_tiles_reach_the_residual_path_with_a_step_above_one():
    """99 x 67 at 16 x 16: tile 7 x 5 = 35 pixels, clip 1 at clip_limit 0.5; a flat tile clips 34, residual 34, step 7"""
    img = images(99, 67)["full"]
    assert cm.geometry(99, 67, (16, 16))["area"] == 35
    lut = cm.luts(img, 0.5, (16, 16))[0, 0].astype(np.int64)
    hist = [1 if (i % 7 == 0 and i // 7 < 34) else 0 for i in range(256)]
    hist[255] += 1
    want = np.clip(np.rint(np.cumsum(hist).astype(F) * (F(255) / F(35))), 0, 255).astype(np.int64)
    assert np.array_equal(lut, want)


def test_model_equals_a_live_cv2():
    """runs only where a real OpenCV is importable; never on a machine with the stub alone"""
    cv2 = pytest.importorskip("cv2")
    if not hasattr(cv2, "createCLAHE"):
        pytest.skip("the cv2 on the path is the stub (no createCLAHE)")
    for w, h, tiles in SHAPES:
        for name, img in images(w, h).items():
            for clip in CLIPS:
                want = cv2.createCLAHE(clipLimit=clip, tileGridSize=tiles).apply(img)
                got = cm.clahe(img, clip, tiles)
                assert np.array_equal(got, want), (w, h, tiles, name, clip, int((got != want).sum()))
