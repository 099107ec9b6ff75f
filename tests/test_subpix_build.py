"""CPU-only: what hipcc makes of the sub-pixel refinement kernel (gfx950 cross-compile, no GPU needed).

k_corner_subpix (csrc/vo_subpix.hip) must exist once, keep its five float64 sums, the mask values and the patch indices in registers (no
scratch) and be part of the library.  Its register count and occupancy are printed and recorded in DESIGN.md; no occupancy is asserted:
none has been measured to matter for this kernel."""
import os
import re

import pytest

from build_helpers import CSRC, kernel_resources, makefile_flags


@pytest.fixture(scope="module")
def resources():
    return kernel_resources("vo_subpix.hip")


def test_one_kernel_without_scratch(resources):
    hits = {k: v for k, v in resources.items() if "k_corner_subpix" in k}
    assert len(hits) == 1, sorted(resources)
    (r,) = hits.values()
    print("k_corner_subpix", r)
    assert r["ScratchSize"] == 0, r
    assert r["LDS"] == 4 * 17 * 17 * 4, r              # four waves' 17 x 17 f32 patches


def test_the_library_builds_it_with_unfused_arithmetic():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bvo_subpix\.hip\b", mk, flags=re.M)
    assert "-ffp-contract=off" in makefile_flags()
