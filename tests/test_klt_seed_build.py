"""CPU-only: what hipcc makes of the seeded tracker kernels (gfx950 cross-compile, no GPU needed).

k_klt_seeded and k_klt_seeded_fb (csrc/vo_klt_seed.hip) are k_klt_track / k_klt_track_fb around klt_lk_point<true>: they must meet the bar the
project sets for k_klt_track_fb -- no scratch, at least 5 waves per SIMD -- and exist once each.  (That the unseeded kernels did not move is
tests/test_klt_fb_build.py's business.)"""
import os

import pytest

from build_helpers import CSRC, kernel_resources


@pytest.fixture(scope="module")
def resources():
    return kernel_resources("vo_klt_seed.hip")


@pytest.mark.parametrize("kernel", ["k_klt_seededILi", "k_klt_seeded_fbILi"])
def test_seeded_kernel_has_no_scratch_and_occupancy_5(resources, kernel):
    hits = {k: v for k, v in resources.items() if kernel in k}
    assert len(hits) == 1, sorted(resources)               # ONE instantiation
    (r,) = hits.values()
    print(kernel, r)
    assert r["ScratchSize"] == 0 and r["Occupancy"] >= 5, r


def test_seeded_kernels_do_not_shadow_the_pinned_names(resources):
    """tests/test_klt_fb_build.py finds k_klt_track<4|5|6> and k_klt_track_fb by substring: nothing here may match"""
    assert not [k for k in resources if "k_klt_track" in k], sorted(resources)
    assert "vo_klt_seed.hip" in open(os.path.join(CSRC, "Makefile")).read()
