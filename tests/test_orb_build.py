"""CPU-only: what hipcc makes of the ORB kernels (csrc/vo_orb.hip) -- gfx950 cross-compile, no GPU needed.  No lane indexes a per-lane array with
a runtime value (the FAST ring, the Harris row windows and the level table are indexed by unrolled counters or read from the kernel arguments), so
every kernel must run without scratch.  Registers, LDS and occupancy are printed and recorded in DESIGN.md; only the describe kernel's, which
shares its LDS tiles with k_brief_describe, are asserted."""
import os
import re

from build_helpers import CSRC, kernel_resources

KERNELS = ("k_orb_level0", "k_orb_resize", "k_orb_score", "k_orb_nms", "k_orb_cut", "k_orb_harris", "k_orb_rank", "k_orb_describe")


def test_every_kernel_exists_once_and_runs_without_scratch():
    res = kernel_resources("vo_orb.hip")
    for name in KERNELS:
        hits = {k: v for k, v in res.items() if name in k}
        assert len(hits) == 1, (name, sorted(res))
        (r,) = hits.values()
        print(name, r)
        assert r["ScratchSize"] == 0, (name, r)
    assert len(res) == len(KERNELS), sorted(res)
    (d,) = [v for k, v in res.items() if "k_orb_describe" in k]
    # one wave per workgroup and the tiles of k_brief_describe: 49 x 49 u8 + 49 x 43 u16 + 43 x 43 u8
    assert d["LDS"] <= 9 * 1024 and d["VGPRs"] <= 64 and d["Occupancy"] >= 4, d


def test_the_shared_device_code_still_runs_without_scratch():
    for src, name in (("vo_fast.hip", "k_fast_score"), ("vo_brief.hip", "k_brief_describe")):
        (r,) = [v for k, v in kernel_resources(src).items() if name in k]
        print(name, r)
        assert r["ScratchSize"] == 0, (name, r)


def test_the_library_builds_it():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bvo_orb\.hip\b", mk, flags=re.M)
    for h in ("vo_fast_dev.h", "vo_brief_dev.h"):       # a change of the shared device code rebuilds its users
        assert re.search(r"^\$\(OBJDIR\)/%\.o:.*\b" + re.escape(h), mk, flags=re.M), h
