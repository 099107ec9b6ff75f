"""CPU-only: what hipcc makes of the tracker kernels (gfx950 cross-compile, no GPU needed).

k_klt_track (csrc/vo_klt.hip) and k_klt_track_fb (csrc/vo_klt_fb.hip: forward + backward LK in one launch) call ONE per-point LK body,
klt_lk_point (csrc/vo_klt_lk.h).  k_klt_track_fb must run without scratch at >= 5 waves per SIMD, and sharing the body must leave
k_klt_track<4|5|6> where they were: 79 / 81 VGPRs, 88 SGPRs, no scratch, occupancy 6 / 5, and -- stronger than the register pin -- the
same count of every vector, buffer, LDS and global instruction as the build of the commit before the body was shared
(tests/golden/klt_parent_opcodes.json)."""
import json
import os
import re

import pytest

from build_helpers import ROOT, kernel_opcodes, kernel_resources


def test_klt_fb_kernel_has_no_scratch_and_occupancy_5():
    res = kernel_resources("vo_klt_fb.hip")
    fb = {k: v for k, v in res.items() if "k_klt_track_fb" in k}
    assert len(fb) == 1, sorted(res)                       # ONE instantiation
    (r,) = fb.values()
    assert r["ScratchSize"] == 0 and r["Occupancy"] >= 5, r


def test_klt_track_resources_unchanged():
    res = kernel_resources("vo_klt.hip")
    want = {4: (81, 5), 5: (81, 5), 6: (79, 6)}
    for wv, (vgpr, occ) in want.items():
        (r,) = [v for k, v in res.items() if re.search(r"k_klt_trackILi%dE" % wv, k)]
        assert (r["VGPRs"], r["TotalSGPRs"], r["ScratchSize"], r["Occupancy"]) == (vgpr, 88, 0, occ), (wv, r)


@pytest.mark.parametrize("src,kernel,name", [("vo_klt.hip", "k_klt_trackILi6E", "k_klt_track<6>"),
                                             ("vo_klt_fb.hip", "k_klt_track_fbILi6E", "k_klt_track_fb<6>")])
def test_klt_vector_and_memory_opcodes_equal_the_parents(src, kernel, name):
    """every v_*, buffer_*, ds_* and global_* opcode as often as in the parent commit's build of the same kernel (a committed histogram,
    never the tree under test); scalar opcodes are reported, not asserted"""
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "klt_parent_opcodes.json")))[name]
    got = kernel_opcodes(src, kernel)
    pinned = ("v_", "buffer_", "ds_", "global_")
    assert sum(1 for k in want if k.startswith(pinned)) > 50 and any(k.startswith("buffer_load") for k in want), "fixture"
    diff = {k: (want.get(k, 0), got.get(k, 0)) for k in sorted(set(want) | set(got)) if want.get(k, 0) != got.get(k, 0)}
    scalar = {k: v for k, v in diff.items() if not k.startswith(pinned)}
    vector = {k: v for k, v in diff.items() if k.startswith(pinned)}
    assert not vector, "%s (parent, now): %s; scalar differences (not asserted): %s" % (name, vector, scalar)
