"""CPU-only: what hipcc makes of the undistortion kernel (gfx950 cross-compile, no GPU needed).

k_undistort (csrc/vo_undistort.hip) must exist once, run out of registers alone (no scratch, no LDS) and be part of the library, built with
unfused arithmetic like the other units: its host half evaluates the float64 map that must equal numpy bit for bit.  Register count and
occupancy are printed and recorded in DESIGN.md; neither is asserted."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual-odom-pipeline_amd", "csrc")


def _hipcc():
    for p in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if p and os.path.exists(p):
            return p
    pytest.skip("no hipcc")


def _flags():
    """CXXFLAGS of the Makefile, as the library is built"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^CXXFLAGS \?=(.*?)(?<!\\)\n", mk, flags=re.M | re.S)
    flags = m.group(1).replace("\\\n", " ").replace("$(ARCH)", "gfx950").split()
    return [f for f in flags if f != "-fPIC"]


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    out = subprocess.run([_hipcc()] + _flags() + ["--cuda-device-only", "-c", "vo_undistort.hip", "-o", str(tmp_path_factory.mktemp("undistort") / "k.o"),
                                                  "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1); res[cur] = {}
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur:
            res[cur][m.group(1).split()[0]] = int(m.group(2))
    return res


def test_one_kernel_without_scratch(resources):
    hits = {k: v for k, v in resources.items() if "k_undistort" in k}
    assert len(hits) == 1, sorted(resources)
    (r,) = hits.values()
    print("k_undistort", r)
    assert r["ScratchSize"] == 0, r
    assert r["LDS"] == 0, r


def test_the_library_builds_it_with_unfused_arithmetic():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^SRCS :=.*\bvo_undistort\.hip\b", mk, flags=re.M)
    assert "-ffp-contract=off" in _flags()
