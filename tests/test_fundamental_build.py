"""CPU-only: what hipcc makes of the fundamental-matrix search (csrc/vo_fundamental.hip) -- gfx950 cross-compile, no GPU needed.  The scoring
kernel is the hot one (up to 768 x batch x n evaluations per round) and must run without scratch or LDS at full occupancy; the other kernels'
resources are printed, and what is asserted of them is what the build shows, with its reason."""
import os
import re

from build_helpers import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one(res, name):
    m = {k: v for k, v in res.items() if name in k}
    assert len(m) == 1, (name, sorted(res))
    return next(iter(m.values()))


def test_score_kernel_has_no_scratch_and_full_occupancy():
    res = kernel_resources("vo_fundamental.hip")
    r = _one(res, "k_f7_score")
    h = _one(kernel_resources("vo_homography.hip"), "k_h4_score")
    print("k_f7_score", r, "beside k_h4_score", h)
    # nine matrix entries, two points, two line triples, a counter and the running sum of err per lane: 56 VGPRs in this build against the
    # 46 of k_h4_score, whose loop has the same shape; 64 is the most that allows the 8 waves per SIMD that hide the point loads
    assert r["ScratchSize"] == 0 and r["LDS"] == 0 and r["VGPRs"] <= 64 and r["Occupancy"] == 8 == h["Occupancy"], (r, h)


def test_the_other_kernels_resources():
    res = kernel_resources("vo_fundamental.hip")
    for name in ("k_f7_init", "k_f7_solve", "k_f7_select", "k_f7_finish"):
        print(name, _one(res, name))
    # the minimal solve keeps its 7 x 9 system, the column order and the two null vectors in registers: every loop over them has constant
    # bounds, the pivot comes up by conditional row and column swaps and the column order is undone by selects, so nothing is indexed by a
    # run-time value (174 VGPRs in this build; 256 is the most a 64-thread workgroup's lanes can hold without spilling, and one wave per
    # workgroup needs no more than one wave per SIMD)
    s = _one(res, "k_f7_solve")
    assert s["ScratchSize"] == 0 and s["LDS"] == 0 and s["VGPRs"] <= 256, s
    # the finish kernel holds the 45 running sums of the Gram matrix per lane (90 VGPRs) beside the loop state, and the 3 x 3 Jacobi of the
    # rank-2 step in registers (unrolled, constant indices): 138 VGPRs in this build, one workgroup per sequence, so two waves per SIMD is
    # all it needs; its LDS is the partial sums and the 9 x 9 Jacobi pair
    f = _one(res, "k_f7_finish")
    assert f["ScratchSize"] == 0 and f["VGPRs"] <= 256 and f["LDS"] <= 4096, f
    # the select kernel: a count and a root per hypothesis and the models' counter in LDS (2 x 256 x 4 + 4 = 2 052 bytes in this build), one workgroup per sequence
    q = _one(res, "k_f7_select")
    assert q["ScratchSize"] == 0 and q["LDS"] <= 4096, q
    assert _one(res, "k_f7_init")["ScratchSize"] == 0


def test_the_unit_is_in_the_makefile():
    mk = open(os.path.join(ROOT, "visual-odom-pipeline_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "vo_fundamental.hip" in srcs and "vo_ransac.h" in mk
