"""GPU: the SIFT kernels (csrc/vo_sift.hip) against the independent float64 model of tests/sift_model.py and against the scale-space truths,
through VoContext.sift_detect_compute only.

tests/test_gpu_sift.py shows that the kernel equals oracle/sift_oracle.py bit for bit; the kernel was written after that oracle, so a shared
misreading passes there.  Here the kernel answers to a model that reaches every result by another route and to geometry: blobs (origin, scale,
octave), ramps (angle convention), transposes (axes, descriptor layout), negatives, translations.  tests/test_sift_model.py shows on the CPU
that the oracle stays inside the very same verdicts and that they reject bent conventions.  All images of one size go through one batched
context.  Also: a batch equals single calls, and one context called with max_out large / small / large again equals fresh contexts (the reuse
of the descriptor buffers with a row stride other than max_out)."""
import numpy as np
import pytest

import sift_model as sm

pytestmark = pytest.mark.gpu


def _run(images, nfeatures=0, masks=None, max_out=None):
    """images: {name: img}; masks: {name: mask} -> {name: (kp, desc)}; every size in one batched context, one call"""
    from vo_mi355x import VoContext
    out, sizes = {}, {}
    for name, img in images.items():
        sizes.setdefault(img.shape, []).append(name)
    for (h, w), names in sizes.items():
        mk = None
        if masks is not None:
            mk = np.stack([masks.get(n, np.full((h, w), 255, np.uint8)) for n in names])
        with VoContext(w, h, max_pts=64, batch=len(names)) as c:
            res = c.sift_detect_compute(np.stack([images[n] for n in names]), mask=mk, nfeatures=nfeatures, max_out=max_out)
        out.update(zip(names, [res] if len(names) == 1 else res))
    return out


@pytest.fixture(scope="module")
def judged():
    """(name, case label) -> (model result, image, kp, desc) for the seven judged images and their four cases"""
    images = {n: sm.image(n) for n in sm.JUDGED}
    det = {n: sm.detect(im) for n, im in images.items()}
    out = {}
    for i, label in enumerate(c[0] for c in sm.cases(sm.JUDGED[0])):
        per = {n: sm.cases(n)[i] for n in images}
        masks = {n: c[2] for n, c in per.items() if c[2] is not None}
        nf = per[sm.JUDGED[0]][1]
        got = _run(images, nfeatures=nf, masks=masks or None)
        for n in images:
            out[n, label] = (sm.select(det[n], nf, per[n][2]), images[n]) + tuple(got[n])
    out["det"] = det
    return out


@pytest.fixture(scope="module")
def truth():
    return _run(sm.truth_images())


@pytest.mark.parametrize("name", sm.JUDGED)
def test_kernel_inside_the_verdicts(judged, name):
    for label, _, _ in sm.cases(name):
        res, img, kp, desc = judged[name, label]
        jk, bad, exc = sm.judge_all(res, img, kp, desc)
        print("%s %s: %d reported, %d certified, excused %.1f %%, %d descriptors excused" % (name, label, len(kp), jk["certified"], 100 * jk["excused"], exc))
        assert not jk["failures"], (label, jk["failures"][:5])
        assert not bad, (label, bad[:5])
        assert jk["excused"] <= sm.EXCUSED_MAX, (label, jk["excused"], exc)        # one share: marginal keypoints and excused descriptors
        assert jk["certified"] >= sm.least_certified(name), (label, jk["certified"])


def test_mask_edge_follows_the_rounded_pixel(judged):
    name = "texture161x97"
    det = judged["det"][name]
    mask, near = sm.edge_mask(det)
    assert near >= 3
    kp, desc = _run({name: sm.image(name)}, masks={name: mask})[name]
    jk, bad, _ = sm.judge_all(sm.select(det, 0, mask), sm.image(name), kp, desc)
    assert not jk["failures"] and not bad and jk["excused"] <= sm.EXCUSED_MAX and jk["certified"] >= sm.least_certified(name)
    px = mask[(kp[:, 1] + 0.5).astype(int), (kp[:, 0] + 0.5).astype(int)]
    assert px.all()


def test_blobs(truth):
    sm.check_blobs(truth)


def test_ramp_angle(truth):
    sm.check_ramps(truth)


def test_transpose_negation_and_descriptor_layout(truth):
    sm.check_transpose_negation(truth)


def test_translation(truth):
    sm.check_translation(truth, exact=True)


def _same(a, b):
    return a[0].shape == b[0].shape and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_batch_of_three_equals_single_calls():
    images = {"a": sm.texture(161, 97, 3), "b": sm.texture(161, 97, 4), "c": sm.blocks(161, 97, 5)}
    batch = _run(images, nfeatures=100)
    for n, im in images.items():
        assert len(batch[n][0]) >= 20
        assert _same(batch[n], _run({n: im}, nfeatures=100)[n]), n


def test_context_reuse_with_other_max_out():
    """one context: max_out large, then small (still fits), then large again -- the descriptor buffers allocated for the large call are reused
    with their own row stride while the caller's arrays have max_out rows"""
    from vo_mi355x import VoContext
    a, b = sm.texture(97, 61, 24), sm.texture(97, 61, 3)
    fresh = {}
    for cap in (4096, 128):
        with VoContext(97, 61, max_pts=64, batch=2) as c:
            fresh[cap] = c.sift_detect_compute(np.stack([a, b]), nfeatures=0, max_out=cap)
    assert 64 < max(len(k) for k, _ in fresh[4096]) <= 128
    with VoContext(97, 61, max_pts=64, batch=2) as c:
        for cap in (4096, 128, 4096):
            got = c.sift_detect_compute(np.stack([a, b]), nfeatures=0, max_out=cap)
            assert all(_same(g, f) for g, f in zip(got, fresh[cap])), cap
        got = c.sift_detect_compute(np.stack([b, a]), nfeatures=0, max_out=128)          # other content through the reused buffers
        assert _same(got[0], fresh[128][1]) and _same(got[1], fresh[128][0])
