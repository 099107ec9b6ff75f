"""GPU: k_st_select on every size class, chunk branch, conflict-list path, min_distance kind and limit instance, on purpose.

The cases come from tests/st_select_cases.py; tests/test_st_select_cases.py shows on the CPU that each lands where it claims.  Here the response
map, the candidate count and the ordered corner list are compared with the oracle (oracle.good_features) AND with the brute-force model
(tests/st_select_model.py): integers and float bit patterns, so np.array_equal everywhere, no tolerance."""
import numpy as np
import pytest

import st_select_cases as sc
import st_select_model as m

pytestmark = pytest.mark.gpu

INVALID = -1
CAPACITY = -5


def _prm(c, case):
    return c.st_params(max_corners=case["maxc"], quality_level=case["q"], min_distance=case["md"], block_size=case["block"])


def _run(cases):
    """every case through VoContext.shi_tomasi + shi_tomasi_read, one context per image"""
    from vo_mi355x import VoContext
    by_img = {}
    for case in cases:
        by_img.setdefault(case["img"], []).append(case)
    for key, group in by_img.items():
        img = sc.image(*key)
        h, w = img.shape
        with VoContext(w, h, max_pts=64) as c:
            c.push_frame(img)
            for case in group:
                ref, resp, rnc, sel = sc.reference(case)
                corners = c.shi_tomasi(None, 0, params=_prm(c, case))
                eig, mask, nc = c.shi_tomasi_read()
                assert np.array_equal(eig.view(np.uint32), resp.view(np.uint32)), (case["name"], "response map")
                assert (mask == 255).all(), case["name"]
                assert nc == rnc == sel.n_valid, (case["name"], "candidate count", nc, rnc, sel.n_valid)
                assert np.array_equal(corners, ref), (case["name"], "corners vs oracle", len(corners), len(ref))
                assert np.array_equal(corners, sel.corners), (case["name"], "corners vs brute-force model")


def test_candidate_counts_on_both_sides_of_every_size_class():
    """0, 1, 2 and n / n + 1 around 1024, 2048, 4096, 8192 (the sort's and the conflict section's classes) and 16384 (the chunk loop), each
    with the distance rule (7) and without (0.5)"""
    _run(sc.count_cases())


def test_chunk_loop_branches():
    """first chunk fills max_corners; a remainder chunk; three chunks; the radix select leaving early (distinct values) and running into the
    pixel-index bits (plateau); later-chunk candidates refused by earlier chunks' corners; no distance rule above 16384 candidates"""
    _run(sc.chunk_cases())


def test_conflict_lists_overflow_and_the_strict_distance():
    """candidates with exactly four and with more than four higher-ranked ones inside the radius (the register list and the second grid walk);
    pairs at exactly min_distance = 5 (offsets 3, 4) stay: the test is strict"""
    _run(sc.conflict_cases())


def test_fractional_huge_and_infinite_min_distance():
    """fractional distances (the cell is ceil(md), OpenCV's is lrint(md): the same corners), distances beyond the image (one corner), 1e6,
    3e9 and +inf (the host clamps the cell in double), and the coarsened grid at 320 x 240 and 640 x 480"""
    _run(sc.distance_cases())


def _single_ref(key, block, q, md, maxc):
    import vo_oracle as o
    img = sc.image(*key)
    ref, resp, rnc = o.good_features(img, None, maxCorners=maxc, qualityLevel=q, minDistance=md, blockSize=block, return_aux=True)
    sel = m.select(resp, None, maxc, q, md)
    ref = ref[:m.OUT_CAP]
    assert np.array_equal(ref, sel.corners) and rnc == sel.n_valid
    return ref, resp, rnc


def test_batch_of_three_and_reuse_after_a_chunked_call():
    """a flat image (no candidate), a chunked one (17 437 candidates, two chunks) and a small one side by side; then the same context with the
    images rotated, twice: every sequence slot runs after a chunked call in it (the raw counter is re-armed by the kernel itself)"""
    from vo_mi355x import VoContext
    w, h = sc.NOISE_A[1], sc.NOISE_A[2]
    keys = [("flat", w, h, 0), sc.NOISE_A, ("blocks", w, h, 3)]
    refs = {k: _single_ref(k, 3, 1e-3, 7.0, 0) for k in keys}
    assert refs[keys[0]][2] == 0 and refs[keys[1]][2] > sc.CHUNK and 0 < refs[keys[2]][2] < 1024
    with VoContext(w, h, max_pts=64, batch=3) as c:
        prm = c.st_params(max_corners=0, quality_level=1e-3, min_distance=7.0, block_size=3)
        for rot in range(3):
            order = keys[rot:] + keys[:rot]
            c.push_frame(np.stack([sc.image(*k) for k in order]))
            corners = c.shi_tomasi(None, 0, params=prm)
            eig, _, nc = c.shi_tomasi_read()
            for b, k in enumerate(order):
                ref, resp, rnc = refs[k]
                assert np.array_equal(eig[b].view(np.uint32), resp.view(np.uint32)) and int(nc[b]) == rnc, (rot, b)
                assert np.array_equal(corners[b], ref), (rot, b, k[0])


BAD_PARAMS = (dict(quality_level=0.0), dict(quality_level=-0.0), dict(quality_level=-0.03), dict(quality_level=float("nan")),
              dict(min_distance=-1.0), dict(min_distance=float("nan")), dict(min_distance=float("-inf")), dict(max_corners=-1))


def test_parameter_rules_on_every_entry():
    """quality_level not > 0 (NaN, -0.0), min_distance NaN or < 0, max_corners < 0: VO_E_INVALID on the synchronous call, the resident call with
    and without limits, the track table's detection, the fused step and the closed loop's creation; the context's next detection is unchanged"""
    from vo_mi355x import VoContext, VoError
    from vo_mi355x.resident import ResidentPipeline
    key = sc.BINARY
    img = sc.image(*key)
    h, w = img.shape
    ref, _, _ = _single_ref(key, 3, 1e-3, 2.5, 0)

    def refused(fn):
        with pytest.raises(VoError) as e:
            fn()
        assert e.value.code == INVALID, str(e.value)

    with VoContext(w, h, max_pts=64) as c:
        c.push_frame(img)
        good = c.st_params(max_corners=0, quality_level=1e-3, min_distance=2.5, block_size=3)
        first = c.shi_tomasi(None, 0, params=good)
        assert np.array_equal(first, ref)
        for bad in BAD_PARAMS:
            prm = c.st_params(**dict(dict(max_corners=0, quality_level=1e-3, min_distance=2.5, block_size=3), **bad))
            refused(lambda: c.shi_tomasi(None, 0, params=prm))
            assert np.array_equal(c.shi_tomasi(None, 0, params=good), ref), bad
            refused(lambda: c.shi_tomasi_resident(0, 0, params=prm))
            refused(lambda: c.shi_tomasi_resident(0, 0, params=prm, limit=5))
            refused(lambda: c.frame_step_host([img], 0, do_dlt=False, do_ba=False, do_st=True, st=prm))
            c.shi_tomasi_resident(0, 0, params=good)
            assert np.array_equal(c.shi_tomasi_fetch(), ref), bad
        # accepted: +inf and finite-but-huge distances (one corner), a quality level above 1 (no candidate)
        for md in (float("inf"), 1e300):
            one = c.shi_tomasi(None, 0, params=c.st_params(max_corners=0, quality_level=1e-3, min_distance=md, block_size=3))
            assert np.array_equal(one, ref[:1])
        assert len(c.shi_tomasi(None, 0, params=c.st_params(max_corners=0, quality_level=1.5, min_distance=2.5, block_size=3))) == 0
    with VoContext(w, h, max_pts=2048) as c:
        c.push_frame(img)
        c.tracks_seed(np.array([[20.0, 20.0]], np.float32), t=0)
        for bad in BAD_PARAMS:
            prm = c.st_params(**dict(dict(max_corners=100, quality_level=1e-3, min_distance=2.5, block_size=3), **bad))
            refused(lambda: c.tracks_detect(0, 0, params=prm, max_new=100))
        assert c.tracks_counts()[0] == 1                                              # nothing was spawned by the refused calls
        c.tracks_detect(0, 0, params=c.st_params(max_corners=100, quality_level=1e-3, min_distance=2.5, block_size=3), max_new=100)
        assert c.tracks_counts()[0] == 101
    K = np.array([[200.0, 0, w / 2], [0, 200.0, h / 2], [0, 0, 1]])
    with VoContext(w, h, max_pts=256) as c:
        for md in (-1.0, float("nan")):
            refused(lambda: ResidentPipeline(c, K, min_kp_dist=md))
        ResidentPipeline(c, K, min_kp_dist=0.0)                                        # no distance rule: accepted


def test_more_raw_candidates_than_the_list_holds_is_reported_and_the_context_goes_on():
    """the one VO_E_CAPACITY exit of the selection: > 262144 candidates appended by the NMS stage (a period-3 tile at block_size 3: the response
    is the same at every interior pixel).  n_out = 0, the status is VO_E_CAPACITY, and the next call on the same context is right."""
    import ctypes as C
    import vo_oracle as o
    from vo_mi355x import VoContext
    from vo_mi355x._lib import ptr
    img = sc.image(*sc.TILE)
    h, w = img.shape
    noise = sc.image("noise", w, h, 21)
    q, md, block, maxc = 1e-3, 7.0, 3, 500
    _, _, rnc = o.good_features(img, None, maxCorners=maxc, qualityLevel=q, minDistance=md, blockSize=block, return_aux=True)
    assert rnc > 262144
    ref, resp, rnc2 = _single_ref(("noise", w, h, 21), block, q, md, maxc)
    with VoContext(w, h, max_pts=64) as c:
        prm = c.st_params(max_corners=maxc, quality_level=q, min_distance=md, block_size=block)
        c.push_frame(img)
        out = np.full((1, maxc, 2), -1.0, np.float32)
        n_out = np.full(1, -7, np.int32)
        rc = c._L.vo_shi_tomasi(c._h, None, 0, 0, None, C.byref(prm), ptr(out, C.c_float), ptr(n_out, C.c_int32))
        assert rc == CAPACITY and n_out[0] == 0
        assert b"262144" in c._L.vo_last_error(c._h)
        c.push_frame(noise)
        corners = c.shi_tomasi(None, 0, params=prm)
        eig, _, nc = c.shi_tomasi_read()
        assert np.array_equal(eig.view(np.uint32), resp.view(np.uint32)) and nc == rnc2
        assert np.array_equal(corners, ref)


# ---- the limited detection: vo_shi_tomasi_resident_limit ----
def _limited(c, prm, limit):
    c.shi_tomasi_resident(0, 0, params=prm, limit=limit)
    return c.shi_tomasi_fetch()


@pytest.mark.parametrize("scene", [s[0] for s in sc.LIMIT_SCENES])
def test_limited_detection_is_a_prefix_of_the_unlimited_one(scene):
    """limits -3 ... 2048 and one above max_corners at max_corners 2048 (the short-chunk instance, kcap = max(256, 8 limit): both sides of
    8 limit = 256) and 2049 / 4096 (the large instance with a limit): the first min(max(limit, 0), max_corners) corners of the unlimited call"""
    from vo_mi355x import VoContext
    _, key, block, q, md = [s for s in sc.LIMIT_SCENES if s[0] == scene][0]
    img = sc.image(*key)
    h, w = img.shape
    ref, _, rnc = _single_ref(key, block, q, md, 4096)
    with VoContext(w, h, max_pts=64) as c:
        c.push_frame(img)
        for mc in sc.LIMIT_MAX_CORNERS:
            prm = c.st_params(max_corners=mc, quality_level=q, min_distance=md, block_size=block)
            c.shi_tomasi_resident(0, 0, params=prm)
            full = c.shi_tomasi_fetch()
            assert np.array_equal(full, ref[:mc]), (scene, mc, "unlimited")
            for lim in sc.LIMITS + (mc + 7,):
                got = _limited(c, prm, lim)
                want = full[:min(max(lim, 0), mc)]
                assert len(got) == len(want) and np.array_equal(got, want), (scene, mc, lim, len(got), len(want))
            # vo_tuning.st_host_limit: the limits are ignored, the unlimited list comes back
            c.set_tuning(st_host_limit=1)
            assert np.array_equal(_limited(c, prm, 5), full), (scene, mc, "st_host_limit")
            c.set_tuning(st_host_limit=0)


def test_unequal_limits_across_a_batch_of_three():
    from vo_mi355x import VoContext
    keys = [("noise", 320, 240, 9), ("binary", 320, 240, 6), ("noise", 320, 240, 10)]
    block, q, md = 3, 1e-3, 3.0
    refs = [_single_ref(k, block, q, md, 4096)[0] for k in keys]
    with VoContext(320, 240, max_pts=64, batch=3) as c:
        c.push_frame(np.stack([sc.image(*k) for k in keys]))
        for mc in sc.LIMIT_MAX_CORNERS:
            prm = c.st_params(max_corners=mc, quality_level=q, min_distance=md, block_size=block)
            for limits in ((1, 33, 513), (2048, 0, 31), (-3, 5000, 100), (512, 512, 511)):
                got = _limited(c, prm, limits)
                for b in range(3):
                    want = refs[b][:mc][:max(limits[b], 0)]
                    assert len(got[b]) == len(want) and np.array_equal(got[b], want), (mc, limits, b)
