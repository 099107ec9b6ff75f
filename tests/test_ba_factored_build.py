"""CPU-only: what hipcc makes of the factored bundle-adjustment kernels (csrc/vo_ba_factored.hip) -- gfx950 device-only cross-compile, no GPU.

k_ba_build_f keeps the ten Gram tiles of a window of 10 in 80 accumulator registers like k_ba_build_w: every instance must fit the 256 vector
registers of two waves per SIMD without scratch (a spill is stored and reloaded per landmark chunk), and the unit must be part of the library."""
import os
import re

import pytest

from build_helpers import CSRC, kernel_resources


@pytest.fixture(scope="module")
def resources():
    return kernel_resources("vo_ba_factored.hip")


def test_every_factored_kernel_fits_two_waves_per_simd_without_scratch(resources):
    kernels = {k: v for k, v in resources.items() if re.match(r"_Z\d+k_ba_(build|update)_fI", k)}
    assert kernels
    for k, r in kernels.items():
        assert r["ScratchSize"] == 0 and r["VGPRs"] <= 256 and r["Occupancy"] >= 2, (k, r)


def test_the_window_10_huber_instances_exist_once(resources):
    """<4, 2, 5> (windows of 9 and 10 slots, 5 lanes per landmark) with the Huber loss, which also serves the linear one"""
    assert len([k for k in resources if k.startswith("_Z12k_ba_build_fILi4ELi2ELi5ELi0EEv")]) == 1
    assert len([k for k in resources if k.startswith("_Z13k_ba_update_fILi2ELi5ELi0EEv")]) == 1


def test_static_lds_stays_small(resources):
    """the build kernel's panels are dynamic LDS of k_ba_build_w<4, 2, 5>'s size (the host passes the same byte count to both); what the kernels
    declare themselves stays a few hundred bytes (build) / under 3 KB (update: the staged cameras)"""
    (b,) = [v for k, v in resources.items() if k.startswith("_Z12k_ba_build_fILi4ELi2ELi5ELi0EEv")]
    (u,) = [v for k, v in resources.items() if k.startswith("_Z13k_ba_update_fILi2ELi5ELi0EEv")]
    assert b["LDS"] <= 512 and u["LDS"] <= 3072, (b, u)


def test_the_unit_is_part_of_the_library():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bvo_ba_factored\.hip\b", mk, flags=re.M)
