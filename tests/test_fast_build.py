"""CPU-only: what hipcc makes of the FAST response kernel (gfx950 cross-compile, no GPU needed).

k_fast_score (csrc/vo_fast.hip) must exist once, run without scratch -- its 16-pixel ring and the sliding arc minima are indexed by unrolled loop
counters only, a runtime-indexed ring would go to scratch -- and be part of the library.  Registers, LDS and occupancy are printed and recorded
in DESIGN.md; none is asserted."""
import os
import re

import pytest

from build_helpers import CSRC, kernel_resources


@pytest.fixture(scope="module")
def resources():
    return kernel_resources("vo_fast.hip")


def test_the_kernel_exists_once_and_runs_without_scratch(resources):
    hits = {k: v for k, v in resources.items() if "k_fast_score" in k}
    assert len(hits) == 1, sorted(resources)
    (r,) = hits.values()
    print("k_fast_score", r)
    assert r["ScratchSize"] == 0, r


def test_the_library_builds_it():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bvo_fast\.hip\b", mk, flags=re.M)
