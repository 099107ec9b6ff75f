"""CPU-only: what hipcc makes of the undistortion kernel (gfx950 cross-compile, no GPU needed).

k_undistort (csrc/vo_undistort.hip) must exist once, run out of registers alone (no scratch, no LDS) and be part of the library, built with
unfused arithmetic like the other units: its host half evaluates the float64 map that must equal numpy bit for bit.  Register count and
occupancy are printed and recorded in DESIGN.md; neither is asserted."""
import os
import re

import pytest

from build_helpers import CSRC, kernel_resources, makefile_flags


@pytest.fixture(scope="module")
def resources():
    return kernel_resources("vo_undistort.hip")


def test_one_kernel_without_scratch(resources):
    hits = {k: v for k, v in resources.items() if "k_undistort" in k}
    assert len(hits) == 1, sorted(resources)
    (r,) = hits.values()
    print("k_undistort", r)
    assert r["ScratchSize"] == 0, r
    assert r["LDS"] == 0, r


def test_the_library_builds_it_with_unfused_arithmetic():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bvo_undistort\.hip\b", mk, flags=re.M)
    assert "-ffp-contract=off" in makefile_flags()
