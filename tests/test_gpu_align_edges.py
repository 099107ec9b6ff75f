"""GPU: vo_sparse_align (csrc/vo_align.hip, csrc/vo_chol6.h) at its edges, against tests/align_model.py on align_model.edge_cases() -- every
way a level can end (eps, max_iters, chi, a pivot that is not positive, points lost while the level iterates), a skipped top level above one
that runs and a run level above a skipped one, stores of four levels with even and odd sizes, levels smaller than the patch footprint,
projections exactly on the interior's edges, the tie chi == chi_prev, the host's Rodrigues / log pair at 0.5 - 2.5 rad, the count edges
of the sixteen-points-a-round loop, and a batch whose sequences leave the iteration loop at different points.
tests/test_align_model.py shows on the CPU that the model alone decides these cases and that they reach those exits and shapes.

The rule is check_case() of tests/test_gpu_align.py, unchanged: status, the pose by displacement against 4 x the model's float32 switch
(where the switch moves nothing, the kernel must move nothing), and on a decided case iters, levels_run, n_used, the mask, chi2 and flags by
equality.  Every case runs under form 1 and form 2, which must give the same bits."""
import numpy as np
import pytest

import align_model as am
from test_gpu_align import Stores, check_case, raw_align

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stores():
    s = Stores()
    yield s
    s.close()


def test_the_stores_hold_the_levels_the_model_is_given(stores):
    """four levels of 208 x 120, 211 x 123 and 67 x 43 (Stores.get asserts the sizes through level_size): the oracle's pyrDown of odd and of
    tiny levels is the store's"""
    seen = set()
    for case in am.edge_cases():
        key = am.case_store(case)
        if key in seen:
            continue
        seen.add(key)
        c = stores.get(case)
        prev, cur = am.case_frames(case)
        c.push_frame(prev); c.push_frame(cur)
        for which, img in ((0, prev), (1, cur)):
            lv = am.pyramid(img, key[2])
            for l in range(key[2]):
                assert np.array_equal(c.pyramid_read(which, l)[0], lv[l]), (key, which, l)
    assert {k[0] for k in seen} == {(208, 120), (211, 123), (67, 43)} and {k[2] for k in seen} == {2, 4}


@pytest.mark.parametrize("case", am.edge_cases(), ids=lambda c: c["name"])
def test_edge_case_against_model_in_both_forms(stores, case):
    c = stores.get(case)
    a = check_case(c, case, form=1)
    b = check_case(c, case, form=2, record=False)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and np.array_equal(a[2], b[2]) and a[3] == b[3]


def test_boundary_masks_are_the_models_exactly(stores):
    """the interior test on the line, level by level: 4 <= x is inclusive, x < w_l - 5 exclusive.  The six edge points of level l are used
    as BOUNDARY_USED says, and the whole mask is the model's"""
    for case in [c for c in am.edge_cases() if c["name"].startswith("boundary_l")]:
        l = case["params"]["min_level"]
        m64, _ = am.case_runs(case)
        rv, tv, mask, st = check_case(stores.get(case), case, record=False)
        print("%s: used %d of %d, the six on the edges %s" % (case["name"], int((mask != 0).sum()), len(mask), list(mask[16 * l:16 * l + 6])))
        assert tuple(mask[16 * l:16 * l + 6] != 0) == am.BOUNDARY_USED == tuple(m64["used"][16 * l:16 * l + 6])
        assert np.array_equal(mask != 0, m64["used"]) and m64["iters"][l] == 1 and m64["flags"] == am.END_EPS
        assert not rv.any() and not tv.any()


def test_mixed_batch_equals_each_problem_alone(stores):
    """batch = 4, one call: a four-level problem, the stripes (PIVOT), nine finite rows (no level runs) and a top level that ends by
    POINTS.  Every sequence's pose, mask and stats bytes equal the same problem run alone on a batch = 1 context (and that run the model)"""
    seqs = am.mixed_batch()
    cb = stores.get(seqs[0], batch=4)
    cb.push_frame(np.stack([am.case_frames(c)[0] for c in seqs])); cb.push_frame(np.stack([am.case_frames(c)[1] for c in seqs]))
    params = seqs[0]["params"]
    assert all(c["params"] == params and am.case_store(c) == am.case_store(seqs[0]) and c["rvec0"] is None for c in seqs)
    rc, rv, tv, mask, st = raw_align(cb, np.stack([c["K"] for c in seqs]), np.stack([c["X"] for c in seqs]), **params)
    assert rc == 0
    c1 = stores.get(seqs[0])
    for b, c in enumerate(seqs):
        one = check_case(c1, c, record=False)
        assert one[0].tobytes() == rv[b].tobytes() and one[1].tobytes() == tv[b].tobytes() and np.array_equal(one[2], mask[b]), c["name"]
        assert one[3] == bytes(st[b]), c["name"]
    print("mixed batch: status %s, flags %s, iters %s" % ([s.status for s in st], [s.flags for s in st], [list(s.iters)[:4] for s in st]))
    # the four did leave the loop at different points (the model's figures: tests/test_align_model.py asserts them on the CPU)
    models = [am.case_runs(c)[0] for c in seqs]
    assert [s.status for s in st] == [m["status"] for m in models] == [0, 0, am.VO_E_NUMERIC, 0]
    assert st[1].flags == am.END_PIVOT and st[3].iters[3] == models[3]["iters"][3] and models[3]["ends"][3] == am.END_POINTS
