"""CPU-only: what hipcc makes of the tracker that keeps the target window while LK stays in one pixel cell (gfx950 cross-compile, no GPU needed).

k_klt_track_r (csrc/vo_klt_reuse.hip) is k_klt_track around klt_lk_point<false, true>: the widened rows of the target window wait in LDS between
the samplings of one pyramid level.  The instance the launcher names must build without scratch at the occupancy it was compiled for, its LDS must
leave room for 24 one-wave workgroups per compute unit, it must not be found by the substrings that pin k_klt_track / k_klt_track_fb, and it skips
fetches, it does not add any.  (That the shipped kernels did not move is tests/test_klt_fb_build.py's and tests/test_klt_seed_build.py's business.)"""
import os
import re

import pytest

from build_helpers import CSRC, kernel_opcodes, kernel_resources

LDS_PER_CU = 160 * 1024
WORKGROUPS_PER_CU = 24          # 4 SIMDs x 6 waves, one wave per workgroup


def launched_waves():
    """the instantiation vo_klt_launch_reuse names"""
    src = open(os.path.join(CSRC, "vo_klt_reuse.hip")).read()
    body = src[src.index("void vo_klt_launch_reuse"):]
    (wv,) = set(re.findall(r"k_klt_track_r<(\d)>", body))
    return int(wv)


@pytest.fixture(scope="module")
def resources():
    return kernel_resources("vo_klt_reuse.hip")


def test_reuse_kernel_has_no_scratch_and_the_occupancy_of_its_bound(resources):
    wv = launched_waves()
    assert wv in (5, 6)
    hits = {k: v for k, v in resources.items() if "k_klt_track_rILi%dE" % wv in k}
    assert len(hits) == 1 and len(resources) == 1, sorted(resources)       # ONE instantiation, the launched one
    (r,) = hits.values()
    print(wv, r)
    assert r["ScratchSize"] == 0 and r["Occupancy"] == wv, r


def test_reuse_kernel_lds_leaves_room_for_24_workgroups(resources):
    (r,) = resources.values()
    assert 0 < r["LDS"] <= LDS_PER_CU // WORKGROUPS_PER_CU == 6826, r


def test_reuse_kernel_does_not_shadow_the_pinned_names(resources):
    """tests/test_klt_fb_build.py finds k_klt_track<4|5|6> and k_klt_track_fb by these substrings"""
    assert not [k for k in resources if "k_klt_trackILi" in k or "k_klt_track_fbILi" in k], sorted(resources)
    assert "vo_klt_reuse.hip" in open(os.path.join(CSRC, "Makefile")).read()


def test_reuse_kernel_skips_fetches_and_adds_none():
    """the template's eight row loads, one fetch in the LK loop, one in the error pass: as many buffer_load_dword as k_klt_track<6>, and the
    parked rows go through LDS as 64-bit words"""
    shipped = kernel_opcodes("vo_klt.hip", "k_klt_trackILi6E")
    got = kernel_opcodes("vo_klt_reuse.hip", "k_klt_track_rILi%dE" % launched_waves())
    print({k: (shipped.get(k, 0), got.get(k, 0)) for k in sorted(set(shipped) | set(got)) if k.startswith(("buffer_", "ds_", "v_perm"))})
    assert shipped["buffer_load_dword"] == 24
    assert got["buffer_load_dword"] <= shipped["buffer_load_dword"]
    assert got["ds_bpermute_b32"] <= shipped["ds_bpermute_b32"]
    assert not [k for k in got if k.startswith(("scratch_", "flat_"))], sorted(got)
    assert sum(v for k, v in got.items() if k.startswith("ds_read")) > 0 and sum(v for k, v in got.items() if k.startswith("ds_write")) > 0
