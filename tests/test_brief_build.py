"""CPU-only: what hipcc makes of the oriented BRIEF kernel (csrc/vo_brief.hip) and of the Hamming matcher (csrc/vo_match.hip) -- gfx950
cross-compile, no GPU needed.  Both must run without scratch: k_brief_describe indexes the sampling table it takes by value with the lane,
and k_match_hamming keeps its query in LDS so that no per-lane array is indexed by a loop counter."""
from build_helpers import kernel_resources


def test_brief_describe_has_no_scratch():
    res = {k: v for k, v in kernel_resources("vo_brief.hip").items() if "k_brief_describe" in k}
    assert len(res) == 1, sorted(res)
    (r,) = res.values()
    print("k_brief_describe", r)
    # one wave per workgroup: raw tile 49 x 49 u8 + horizontal sums 49 x 43 u16 + blurred tile 43 x 43 u8
    assert r["ScratchSize"] == 0 and r["VGPRs"] <= 64 and r["LDS"] <= 9 * 1024 and r["Occupancy"] >= 4, r


def test_hamming_matcher_has_no_scratch():
    res = kernel_resources("vo_match.hip")
    ham = {k: v for k, v in res.items() if "k_match_hammingILb0E" in k}          # the ungated instance: vo_match_hamming_knn2 and gate 0
    l2 = {k: v for k, v in res.items() if "k_match_l2" in k}
    assert len(ham) == 1 and len(l2) == 1, sorted(res)
    (r,) = ham.values()
    print("k_match_hamming<ungated>", r)
    # the train tile (36 KB) + four queries: four workgroups of four waves fit a compute unit's 160 KB
    assert r["ScratchSize"] == 0 and r["VGPRs"] <= 128 and r["LDS"] <= 40 * 1024 and r["Occupancy"] >= 4, r
    assert next(iter(l2.values()))["ScratchSize"] == 0
