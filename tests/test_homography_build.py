"""CPU-only: what hipcc makes of the homography search (csrc/vo_homography.hip) -- gfx950 cross-compile, no GPU needed.  The scoring kernel
is the hot one (256 x batch x n evaluations per round) and must run without scratch; the other kernels' resources are printed, and what is
asserted of them is what the build shows, with its reason."""
from build_helpers import kernel_resources


def _one(res, name):
    m = {k: v for k, v in res.items() if name in k}
    assert len(m) == 1, (name, sorted(res))
    return next(iter(m.values()))


def test_score_kernel_has_no_scratch():
    res = kernel_resources("vo_homography.hip")
    r = _one(res, "k_h4_score")
    print("k_h4_score", r)
    # nine matrix entries, two points and a counter per lane: 46 VGPRs in this build, so the full 8 waves per SIMD stay resident to hide the
    # point loads (64 is the most that allows 8); it stages nothing in LDS
    assert r["ScratchSize"] == 0 and r["VGPRs"] <= 64 and r["Occupancy"] == 8 and r["LDS"] == 0, r


def test_the_other_kernels_resources():
    res = kernel_resources("vo_homography.hip")
    for name in ("k_h4_init", "k_h4_solve", "k_h4_select", "k_h4_finish"):
        print(name, _one(res, name))
    # the minimal solve keeps its 8 x 9 system in registers: every loop over it has constant bounds and the pivot row comes up by conditional
    # swaps, so nothing is indexed by a run-time value (152 VGPRs in this build; 256 is the most a 64-thread workgroup's lanes can hold without
    # spilling, and one wave per workgroup needs no more than one wave per SIMD)
    s = _one(res, "k_h4_solve")
    assert s["ScratchSize"] == 0 and s["VGPRs"] <= 256, s
    # the finish kernel holds the 45 running sums of a reduction pass per lane (90 VGPRs) beside the loop state: 234 VGPRs in this build, one
    # workgroup per sequence, so two waves per SIMD is all it needs; its LDS is the partial sums, the 9 x 9 Jacobi pair and the LM state
    f = _one(res, "k_h4_finish")
    assert f["ScratchSize"] == 0 and f["VGPRs"] <= 256 and f["LDS"] <= 4096, f
