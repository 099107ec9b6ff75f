"""GPU: the loader's bilateral pre-filter fused into the level-0 kernel is bit-identical to the
oracle's cv2.bilateralFilter restatement, for pushed and resident frames, and the rest of the path sees the filtered image; a fused frame
step, captured or not, follows every change of the setting."""
import numpy as np
import pytest

import ingest_helpers as ih

pytestmark = pytest.mark.gpu


def _images():
    from vo_mi355x import synthetic as syn
    rng = np.random.default_rng(3)
    yield syn.make_sequence(1, w=321, h=123, seed=5, margin=32)[0][0]        # smooth texture: most pixels change
    yield rng.integers(0, 256, (97, 203)).astype(np.uint8)                   # noise: colour weights cut everything off
    g = np.tile(np.arange(160, dtype=np.float32), (64, 1))
    yield np.clip(g * 1.5 + rng.normal(0, 2.0, g.shape), 0, 255).astype(np.uint8)   # noisy ramp: ties at .5 exercised
    yield np.full((64, 80), 200, np.uint8)


@pytest.mark.parametrize("d,sc,ss", [(5, 1.5, 1.5), (3, 10.0, 2.0), (7, 25.0, 3.0), (-1, 4.0, 1.2)])
def test_prefilter_level0_matches_oracle(d, sc, ss):
    import vo_oracle as o
    from vo_mi355x import VoContext
    for img in _images():
        h, w = img.shape
        with VoContext(w, h, max_pts=64) as c:
            c.set_prefilter(d, sc, ss)
            c.push_frame(img)
            got, _ = c.pyramid_read(1, 0)
            ref = o.bilateral(img, d, sc, ss)
            assert np.array_equal(got, ref), (d, sc, ss, img.shape, int((got != ref).sum()))
            c.set_prefilter(0)
            c.push_frame(img)
            assert np.array_equal(c.pyramid_read(1, 0)[0], img)


def test_prefilter_feeds_pyramid_klt_and_resident_batch():
    import vo_oracle as o
    from vo_mi355x import VoContext, synthetic as syn
    w, h, n = 640, 240, 400
    fa, _ = syn.make_sequence(3, w=w, h=h, seed=31, margin=64)
    fb, _ = syn.make_sequence(3, w=w, h=h, seed=32, margin=64)
    rng = np.random.default_rng(0)
    fa = np.clip(fa.astype(np.int32) + rng.integers(-6, 7, fa.shape), 0, 255).astype(np.uint8)   # sensor-like noise
    fb = np.clip(fb.astype(np.int32) + rng.integers(-6, 7, fb.shape), 0, 255).astype(np.uint8)
    pts = syn.grid_points(n, w, h, seed=2)
    with VoContext(w, h, max_pts=512, batch=2) as c:
        c.set_prefilter()                                      # the reference's d = 5, sigmas = 1.5
        c.upload_sequence(np.stack([fa, fb]))
        c.points_upload(np.stack([pts, pts]))
        c.push_frame_resident(0)
        c.push_frame_resident(1)
        c.klt_track_resident(n)
        p1, st, err = c.points_download(n)
        for b, fr in enumerate((fa, fb)):
            f0, f1 = o.bilateral(fr[0]), o.bilateral(fr[1])
            assert (f0 != fr[0]).mean() > 0.05                 # the filter does something on this input
            lv = o.build_pyramid(f1)
            for l in range(len(lv)):
                img_l, der_l = c.pyramid_read(1, l, seq=b)
                assert np.array_equal(img_l, lv[l]) and np.array_equal(der_l, o.scharr(lv[l]))
            q1, qs, qe = o.klt(f0, f1, pts)
            assert np.array_equal(p1[b], q1) and np.array_equal(st[b], qs) and np.array_equal(err[b], qe)


@pytest.mark.parametrize("graph", [False, True], ids=["launches", "graph"])
def test_fused_steps_see_every_change_of_the_prefilter(graph):
    """a context that steps over an uploaded sequence, with graph replay or without, against one fed the same raw frames through
    frame_step_host (plain launches always), both given the same setting before each step.  A captured step holds the tap list and its
    spatial weights by value: A and B have the same 13 taps and other weights, so a captured A step replayed under B shows A's image.  C
    changes the colour table alone, which the kernel reads from device memory: a control.  Every setting sees both store parities, A twice
    (capture, then replay).  The oracle's shares of differing level-0 pixels on these frames: A / B 0.099 .. 0.101, A / C 0.863 .. 0.865."""
    import vo_oracle as o
    from vo_mi355x import synthetic as syn
    w, h, n = 320, 240, 300
    A, B, C = (5, 1.5, 1.5), (5, 1.5, 4.0), (5, 30.0, 1.5)
    plan = [A, A, A, A, B, B, C, C, None, A]
    order = [1, 2, 3, 2, 1, 2, 3, 2, 1, 2]
    frames, _ = syn.make_sequence(4, w=w, h=h, seed=21, margin=64)
    pts = syn.grid_points(n, w, h, seed=4)
    for f in (1, 2, 3):
        fa = o.bilateral(frames[f], *A)
        assert (fa != o.bilateral(frames[f], *B)).mean() > 0.05 and (fa != o.bilateral(frames[f], *C)).mean() > 0.4
    with ih.fused_pair(w, h, frames, pts, graph, False, frames[0]) as (a, b):
        def apply(s):
            for c in (a, b):
                c.set_prefilter(0) if s is None else c.set_prefilter(*s)
        ih.fused_plan(a, b, frames, order, plan, [frames[f] for f in order], n, False, apply)
