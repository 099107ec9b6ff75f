"""CPU-only: what hipcc makes of the depth filter (csrc/vo_depth.hip) -- gfx950 cross-compile, no GPU needed.  The update kernel carries a
seed's float64 geometry in every lane beside the sixteen reference words of the search: it must not spill."""
import os
import re

from build_helpers import kernel_opcodes, kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_unit_is_in_the_makefile():
    mk = open(os.path.join(ROOT, "visual-odom-pipeline_amd", "csrc", "Makefile")).read()
    assert "vo_depth.hip" in re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()


def test_both_kernels_have_no_scratch():
    res = kernel_resources("vo_depth.hip")
    upd = [v for k, v in res.items() if "k_depth_update" in k]
    ini = [v for k, v in res.items() if "k_depth_seed_init" in k]
    assert len(upd) == 1 and len(ini) == 1, sorted(res)
    for name, r in sorted(res.items()):
        print(name, r)
        assert r["ScratchSize"] == 0, (name, r)
    # k_depth_update: 117 VGPRs, 78 SGPRs, 448 bytes of LDS (four patches of 112), 4 waves per SIMD; k_depth_seed_init: 18 VGPRs, no LDS.
    # Several waves per SIMD are what hides the search's loads behind another seed's arithmetic
    assert upd[0]["VGPRs"] <= 128 and upd[0]["LDS"] == 448 and upd[0]["Occupancy"] >= 4, upd[0]
    assert ini[0]["VGPRs"] <= 32 and ini[0]["LDS"] == 0, ini[0]


def test_the_search_is_byte_dot_products_on_aligned_words():
    """per candidate 48 v_dot4_u32_u8 (sum q, sum q^2, sum p q over eight rows of two words) and 16 v_alignbyte_b32 on 8 loads of three
    aligned dwords; the reference rows' own sums take 32 more dot products once per seed"""
    h = kernel_opcodes("vo_depth.hip", "k_depth_update")
    print({k: v for k, v in sorted(h.items()) if "dot4" in k or "alignbyte" in k or k.startswith("global_load") or "readfirstlane" in k})
    assert h["v_dot4_u32_u8"] == 80 and h["v_alignbyte_b32"] == 16 and h["global_load_dwordx3"] == 8
    assert h["v_readfirstlane_b32"] >= 16
    assert not any(k.startswith(("scratch_", "buffer_store", "buffer_load")) for k in h)
