"""CPU-only: what hipcc makes of the descriptor matchers, plain and guided (csrc/vo_match.hip) -- gfx950 cross-compile, no GPU needed -- and
their place in the build and the C ABI.  What is asserted of the kernels' resources is what the build shows, with its reason."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from build_helpers import kernel_resources

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one(res, name):
    m = {k: v for k, v in res.items() if name in k}
    assert len(m) == 1, (name, sorted(res))
    return next(iter(m.values()))


def _definitions(pattern):
    """the files of csrc that define what `pattern` matches, one entry per definition"""
    csrc = os.path.join(ROOT, "visual-odom-pipeline_amd", "csrc")
    return [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")) for _ in re.findall(pattern, open(os.path.join(csrc, f)).read())]


def test_the_unit_and_the_shared_header_are_in_the_makefile():
    mk = open(os.path.join(ROOT, "visual-odom-pipeline_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "vo_match.hip" in srcs and "vo_match_guided.hip" not in srcs            # one unit for the plain and the guided matchers
    deps = re.search(r"^\$\(OBJDIR\)/%\.o: (.*)$", mk, re.M).group(1).split()
    assert "vo_epi_dev.h" in deps
    # one definition of the epipolar test, included by both users
    assert _definitions(r"bool\s+f7_inlier\s*\(") == ["vo_epi_dev.h"]
    csrc = os.path.join(ROOT, "visual-odom-pipeline_amd", "csrc")
    for user in ("vo_fundamental.hip", "vo_match.hip"):
        assert '#include "vo_epi_dev.h"' in open(os.path.join(csrc, user)).read()
    # one two-best insert and one L2 row distance for the plain and the guided scans
    assert _definitions(r"void\s+knn_insert\s*\(") == ["vo_match.hip"]
    assert _definitions(r"float\s+match_l2\s*\(") == ["vo_match.hip"]


def test_kernel_resources():
    res = kernel_resources("vo_match.hip")
    for name, r in sorted(res.items()):
        print(name, r)
        assert r["ScratchSize"] == 0 and r["LDS"] <= 64 * 1024, (name, r)
    assert len(res) == 5, sorted(res)                                               # one scan per distance kind (Hamming: two instances), two accepts
    h, h0, l = _one(res, "k_match_hammingILb1E"), _one(res, "k_match_hammingILb0E"), _one(res, "k_match_l2")
    print("k_match_hamming<gated>", h, "<gate 0>", h0)
    print("k_match_l2", l)
    # Hamming with a gate: the 36 KiB descriptor tile and the four queries of the ungated instance plus two float2 position tiles of 1024
    # rows (16 KiB): 53 504 bytes, three workgroups in a CU's 160 KiB where the ungated instance has four.  The nine entries of F, the
    # query's two points and its epipolar line sit in float64 registers beside the scan (116 VGPRs in this build against 63): under 128 they
    # do not lower the three workgroups (12 waves per CU) that LDS allows.
    assert h["LDS"] == 4 * 9216 + 4 * 4 * 16 + 2 * 8 * 1024 and h["VGPRs"] <= 128 and h["Occupancy"] == 3, h
    # Hamming at gate 0, which also serves vo_match_hamming_knn2: no position tiles, no gate state, no count of admitted rows.  The bounds are
    # those held against the plain kernel k_match_hamming_knn2 this instance replaced, whose recorded values were 63 VGPRs, 37 120 B of LDS
    # and 4 workgroups per CU; this instance builds to the same three numbers.
    assert h0["LDS"] == 4 * 9216 + 4 * 4 * 16 and h0["VGPRs"] <= 72 and h0["Occupancy"] == 4, h0
    # L2, every gate and vo_match_knn2: no descriptor tile; the two position tiles and the four rings of 128 indices (18 432 bytes: eight
    # workgroups per CU).  56 VGPRs in this build: 64 is the most that keeps 8 waves per SIMD, which hide the row loads.
    assert l["LDS"] == 2 * 8 * 1024 + 4 * 4 * 128 and l["VGPRs"] <= 64 and l["Occupancy"] == 8, l
    accept = [v for k, v in res.items() if "k_match_accept" in k]
    assert len(accept) == 2 and all(r["LDS"] == 0 and r["Occupancy"] == 8 for r in accept), accept    # int32 and float distances


def test_exports_struct_size_and_abi_version(tmp_path):
    from vo_mi355x import _lib
    L = _lib.load()
    for name in ("vo_gmatch_default_params", "vo_match_guided_hamming", "vo_match_guided_l2"):
        assert name in _lib.SIGNATURES and hasattr(L, name), name
    assert ctypes.sizeof(_lib.GMatchParams) == 40
    assert L.vo_abi_version() == 4
    p = _lib.GMatchParams(gate=-1, cross_check=-1, radius=-1.0, epi_dist=-1.0, ratio=-1.0, max_dist=-1.0)
    assert L.vo_gmatch_default_params(ctypes.byref(p)) == 0
    assert (p.gate, p.cross_check, p.radius, p.epi_dist, p.ratio, p.max_dist) == (0, 0, 0.0, 0.0, 1.0, float("inf"))
    assert L.vo_gmatch_default_params(None) == -1
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    fields = ("gate", "cross_check", "radius", "epi_dist", "ratio", "max_dist")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vo_mi355x.h"\nint main(void) { printf("%zu", sizeof(vo_gmatch_params));\n' +
                   "".join('printf(" %%zu", offsetof(vo_gmatch_params, %s));\n' % f for f in fields) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [40] + [getattr(_lib.GMatchParams, f).offset for f in fields], got
