"""CPU-only: what hipcc makes of the CLAHE kernels (gfx950 cross-compile, no GPU needed).

k_clahe_lut and k_clahe_apply (csrc/vo_clahe.hip) must each exist once, run without scratch and be part of the library, built with unfused
arithmetic like the other units: the interpolation is float32 with every operation on its own and must equal numpy bit for bit.  Registers,
LDS and occupancy are printed and recorded in DESIGN.md; none is asserted."""
import os
import re

import pytest

from build_helpers import CSRC, kernel_resources, makefile_flags


@pytest.fixture(scope="module")
def resources():
    return kernel_resources("vo_clahe.hip")


@pytest.mark.parametrize("kernel", ["k_clahe_lut", "k_clahe_apply"])
def test_each_kernel_once_and_without_scratch(resources, kernel):
    hits = {k: v for k, v in resources.items() if kernel in k}
    assert len(hits) == 1, sorted(resources)
    (r,) = hits.values()
    print(kernel, r)
    assert r["ScratchSize"] == 0, r


def test_the_library_builds_it_with_unfused_arithmetic():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bvo_clahe\.hip\b", mk, flags=re.M)
    assert "-ffp-contract=off" in makefile_flags()
