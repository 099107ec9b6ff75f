"""CPU: the cases of tests/st_select_cases.py land where they claim, and the oracle's goodFeaturesToTrack (cells of lrint(min_distance), a
3 x 3 walk, as OpenCV) equals the brute-force model of tests/st_select_model.py (no grid at all) on every one of them -- the check of the
argument that integer coordinates two cells apart are at least cell + 1 > min_distance apart, fractional distances included."""
import numpy as np
import pytest

import st_select_cases as sc
import st_select_model as m

GROUPS = {"count": sc.count_cases, "chunk": sc.chunk_cases, "conflict": sc.conflict_cases, "distance": sc.distance_cases}


def _pairs_at(sel, w, h, dx, dy):
    """candidate pairs at the offset (dx, dy)"""
    img = np.zeros((h, w), bool)
    img[sel.cand_xy[:, 1], sel.cand_xy[:, 0]] = True
    return int((img & m._shifted(img, dx, dy, False)).sum())


def _row(c):
    """one line of the landing table + the assertions of the case's landing conditions"""
    ref, resp, rnc, sel = sc.reference(c)
    h, w = resp.shape
    land = c["land"]
    higher, exact_pairs, exact_kept = m.conflicts(sel, w, h, c["md"])
    hist = None if higher is None else np.bincount(np.minimum(higher, 5), minlength=6).tolist()
    print("%-22s %-9s %4dx%-4d bs %2d md %-10g mc %4d | valid %6d chunks %d corners %4d | higher-ranked inside the radius 0,1,2,3,4,>4: %s | pairs at min_distance %s (both kept %s)"
          % (c["name"], c["img"][0], w, h, c["block"], c["md"], c["maxc"], sel.n_valid, sel.n_chunks, len(sel.corners), hist, exact_pairs, exact_kept))
    assert rnc == sel.n_valid, "candidate count: oracle %d, model %d" % (rnc, sel.n_valid)
    assert np.array_equal(ref, sel.corners), "oracle != brute-force model"
    if "count" in land:
        assert sel.n_valid == land["count"]
    if "over" in land:
        assert sel.n_valid > land["over"]
    if "chunks" in land:
        assert sel.n_chunks == land["chunks"]
        if land["chunks"] > 1:                                 # the strongest 16384 did not fill the cut-off
            assert sel.yield_at[sc.CHUNK] < m.cut_off(c["maxc"])
    if land.get("later"):
        assert sel.later_rejected_by_earlier > 0 and sel.later_accepted > 0
    if "tie" in land:
        assert (sel.cand_v[sc.CHUNK - 1] == sel.cand_v[sc.CHUNK]) == land["tie"]
    if land.get("conf45"):
        assert hist[4] > 0 and hist[5] > 0
    if land.get("exact_kept"):
        assert exact_kept > 0 and float(c["md"]).is_integer()
    if "corners" in land:
        assert len(sel.corners) == land["corners"]
        if land["corners"] == 1 and sel.n_valid:
            assert np.array_equal(sel.corners[0], sel.cand_xy[0].astype(np.float32))      # the strongest candidate
    if land.get("sqrt2"):
        assert _pairs_at(sel, w, h, 1, 1) + _pairs_at(sel, w, h, 1, -1) > 0
    if land.get("unit"):
        assert _pairs_at(sel, w, h, 1, 0) + _pairs_at(sel, w, h, 0, 1) > 0
    if land.get("coarse"):
        cell = max(int(np.ceil(c["md"])), 1)
        assert ((w + cell - 1) // cell) * ((h + cell - 1) // cell) > 8192


@pytest.mark.parametrize("group", list(GROUPS))
def test_cases_land_and_the_oracle_equals_the_brute_force_model(group):
    print()
    for c in GROUPS[group]():
        _row(c)


def test_case_names_are_unique_and_every_count_target_is_there():
    names = [c["name"] for c in sc.all_cases()]
    assert len(set(names)) == len(names)
    assert set(sc.COUNT_QUALITY) == set(sc.COUNT_TARGETS)       # no target was skipped: none falls inside a run of equal values


def test_fractional_distances_tell_the_neighbour_classes_apart():
    """on the binary image 1.0 keeps horizontal neighbours, 1.4 drops them but keeps diagonal ones, 1.4142135 (< sqrt 2 in double) too,
    1.5 drops both, 2.5 also drops (2, 1) -- each step changes the list, so a cell rule that rounded the distance would show"""
    n = {md: len(sc.reference(c)[3].corners) for c in sc.distance_cases() for md in [c["md"]] if c["img"] == sc.BINARY}
    assert n[0.0] == n[0.5] == n[0.999] == n[1.0] > n[1.4] == n[1.4142135] > n[1.5] > n[2.5] > n[6.5] > n[7.3] >= n[7.5] >= n[7.999]


def test_limit_keeps_a_prefix_of_the_unlimited_list():
    import vo_oracle as o
    for name, im, block, q, md in sc.LIMIT_SCENES:
        resp = o.min_eig(sc.image(*im), block)
        for mc in sc.LIMIT_MAX_CORNERS:
            full = m.select(resp, None, mc, q, md)
            for lim in sc.LIMITS + (mc + 7,):
                got = m.select(resp, None, mc, q, md, limit=lim).corners
                assert np.array_equal(got, full.corners[:min(max(lim, 0), mc)]), (name, mc, lim)
    dense = m.select(o.min_eig(sc.image(*sc.LIMIT_SCENES[1][1]), 3), None, 4096, 1e-3, 1.0)
    assert dense.n_valid > 4096 and len(dense.corners) == 4096


def test_the_capacity_image_has_more_candidates_than_the_list_holds():
    import vo_oracle as o
    img = sc.image(*sc.TILE)
    assert img.size < 2_000_000
    _, _, rnc = o.good_features(img, None, maxCorners=10, qualityLevel=1e-3, minDistance=7, blockSize=3, return_aux=True)
    assert rnc > 262144
