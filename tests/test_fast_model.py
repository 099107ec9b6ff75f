"""CPU-only: the numpy model of the FAST-9/16 detection path (tests/fast_model.py) against two independent statements.

1. score_map against a literal brute force of the segment test: the score of a pixel is the largest threshold t' >= t at which 9 contiguous
   ring pixels are all brighter than centre + t' or all darker than centre - t' (0 if it fails at t).
2. select -- the selection behind any response map -- against the existing C oracle on ITS response: select(min_eig(img), ...) must be
   good_features(img, ...) exactly, ties, masks, min-distance grid and max_corners included.
3. cv2_keypoints against a real cv2.FastFeatureDetector where one is importable (skipped otherwise)."""
import numpy as np
import pytest

import fast_model as fm

KINDS = ("zeros", "checker", "noise", "narrow", "blocks", "extremes")


def _segment_test(I, x, y, t):
    c = int(I[y, x])
    ring = [int(I[y + dy, x + dx]) for dx, dy in fm.RING]
    for sign in (1, -1):
        flags = [(sign * (v - c)) > t for v in ring]
        for s in range(16):
            if all(flags[(s + j) % 16] for j in range(9)):
                return True
    return False


def _brute(img, t):
    h, w = img.shape
    out = np.zeros((h, w), np.int32)
    for y in range(3, h - 3):
        for x in range(3, w - 3):
            if not _segment_test(img, x, y, t):
                continue
            tp = t
            while tp + 1 <= 255 and _segment_test(img, x, y, tp + 1):
                tp += 1
            out[y, x] = tp
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_score_map_is_the_largest_passing_threshold(kind):
    img = fm.make_image(kind, 24, 17)
    seen = 0
    for t in (1, 20, 254):
        got = fm.score_map(img, t)
        assert got.dtype == np.int32 and np.array_equal(got, _brute(img, t)), (kind, t)
        assert not got[:3].any() and not got[-3:].any() and not got[:, :3].any() and not got[:, -3:].any()
        assert not got[got != 0].min(initial=255) < t                      # a score is at least the threshold
        seen += int((got > 0).sum())
    assert seen > 0 or kind == "zeros"


def test_score_map_edges():
    assert np.array_equal(fm.score_map(fm.ring_7x7(), 1), np.pad([[254]], 3))
    assert np.array_equal(fm.score_map(fm.ring_7x7(), 254), np.pad([[254]], 3))              # m = 255 > 254: the upper edge still passes
    im = fm.ring_7x7(); im[3, 3] = 1
    assert fm.score_map(im, 253)[3, 3] == 253 and not fm.score_map(im, 254).any()            # m = 254: not > 254
    for shape in ((6, 9), (9, 6), (1, 1)):
        assert not fm.score_map(np.full(shape, 9, np.uint8), 1).any()


@pytest.mark.parametrize("max_corners", [0, 5, 1000])
@pytest.mark.parametrize("min_distance", [0, 1, 7])
def test_select_equals_the_oracle_on_its_own_response(min_distance, max_corners):
    import vo_oracle as o
    w, h = 101, 67
    rng = np.random.default_rng(w * 1000 + h)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    pts = np.stack([rng.uniform(0, w, 12), rng.uniform(0, h, 12)], axis=1).astype(np.float32)
    for mask in (None, fm.disc_mask(w, h, pts, 7), fm.disc_mask(w, h, pts, 3, base=(rng.integers(0, 4, (h, w)) > 0) * np.uint8(255))):
        for quality in (0.03, 0.5):
            want, eig, n_cand = o.good_features(img, mask, maxCorners=max_corners, qualityLevel=quality, minDistance=min_distance, return_aux=True)
            assert np.array_equal(eig, o.min_eig(img))
            got = fm.select(eig, mask, max_corners, quality, min_distance)
            assert len(want) > 0 and np.array_equal(got, want), (min_distance, max_corners, quality, len(got), len(want))
            assert len(fm.candidates(eig, mask, quality)[1]) == n_cand


def test_select_orders_ties_by_descending_pixel_index():
    R = np.zeros((9, 12), np.float32)
    R[2, 3] = R[2, 9] = R[6, 5] = 7.0
    R[4, 4] = 9.0
    assert np.array_equal(fm.select(R, None, 0, 0.03, 0), [[4, 4], [5, 6], [9, 2], [3, 2]])
    assert np.array_equal(fm.select(R, None, 0, 0.03, 3), [[4, 4], [9, 2]])                  # (5, 6) and (3, 2) lie within 3 of (4, 4)
    mask = np.full(R.shape, 255, np.uint8); mask[4, 4] = 0
    assert np.array_equal(fm.select(R, mask, 2, 0.03, 0), [[5, 6], [9, 2]])                  # the mask does not zero R: (4, 4) still outranks nobody
    assert len(fm.select(np.zeros((9, 12), np.float32), None, 0, 0.03, 7)) == 0


def test_cv2_keypoints_are_the_strict_maxima_in_row_major_order():
    R = fm.score_map(fm.make_image("noise", 101, 37), 20)
    pts, sc = fm.cv2_keypoints(R)
    assert len(pts) > 20 and (sc >= 20).all()
    flat = pts[:, 1] * 101 + pts[:, 0]
    assert (np.diff(flat) > 0).all()
    for (x, y), s in zip(pts, sc):
        nb = R[y - 1:y + 2, x - 1:x + 2].copy(); nb[1, 1] = -1
        assert R[y, x] == s and (nb < s).all()
    # a checkerboard's corners tie with their neighbours nowhere or everywhere: plateaus yield no strict maximum
    flatR = np.zeros((9, 9), np.int32); flatR[4, 4] = flatR[4, 5] = 30
    assert len(fm.cv2_keypoints(flatR)[0]) == 0


def test_cv2_fast_detector_returns_the_models_keypoints():
    import live_cv2
    cv2 = live_cv2.find_real_cv2()
    if cv2 is None:
        pytest.skip("no real OpenCV importable: parity is with tests/fast_model.py")
    for kind in KINDS[1:]:
        for (w, h) in ((101, 37), (96, 64)):
            img = fm.make_image(kind, w, h)
            for t in (1, 20, 100):
                det = cv2.FastFeatureDetector_create(t, True, cv2.FAST_FEATURE_DETECTOR_TYPE_9_16)
                kps = det.detect(img)
                pts, sc = fm.cv2_keypoints(fm.score_map(img, t))
                assert [(int(k.pt[0]), int(k.pt[1]), int(k.response)) for k in kps] == [(int(x), int(y), int(s)) for (x, y), s in zip(pts, sc)], (kind, w, h, t)
