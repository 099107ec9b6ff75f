"""CPU-only: what hipcc makes of the seeded tracker kernels (gfx950 cross-compile, no GPU needed).

k_klt_seeded and k_klt_seeded_fb (csrc/vo_klt_seed.hip) are k_klt_track / k_klt_track_fb around klt_lk_point<true>: they must meet the bar the
project sets for k_klt_track_fb -- no scratch, at least 5 waves per SIMD -- and exist once each.  (That the unseeded kernels did not move is
tests/test_klt_fb_build.py's business.)"""
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
    out = subprocess.run([_hipcc()] + _flags() + ["--cuda-device-only", "-c", "vo_klt_seed.hip", "-o", str(tmp_path_factory.mktemp("seed") / "k.o"),
                                                  "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    res, cur = {}, None
    for line in out.stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1); res[cur] = {}
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\d+)", line)
        if m and cur:
            res[cur][m.group(1).split()[0]] = int(m.group(2))
    return res


@pytest.mark.parametrize("kernel", ["k_klt_seededILi", "k_klt_seeded_fbILi"])
def test_seeded_kernel_has_no_scratch_and_occupancy_5(resources, kernel):
    hits = {k: v for k, v in resources.items() if kernel in k}
    assert len(hits) == 1, sorted(resources)               # ONE instantiation
    (r,) = hits.values()
    print(kernel, r)
    assert r["ScratchSize"] == 0 and r["Occupancy"] >= 5, r


def test_seeded_kernels_do_not_shadow_the_pinned_names(resources):
    """tests/test_klt_fb_build.py finds k_klt_track<4|5|6> and k_klt_track_fb by substring: nothing here may match"""
    assert not [k for k in resources if "k_klt_track" in k], sorted(resources)
    assert "vo_klt_seed.hip" in open(os.path.join(CSRC, "Makefile")).read()
