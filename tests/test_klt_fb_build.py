"""CPU-only: what hipcc makes of the tracker kernels (gfx950 cross-compile, no GPU needed).

k_klt_track_fb (csrc/vo_klt_fb.hip: forward + backward LK in one launch) must run without scratch at >= 5 waves per SIMD, and moving the LK
helpers into csrc/vo_klt_lk.h for it must leave k_klt_track<4|5|6> exactly where they were: 79 / 81 VGPRs, 88 SGPRs, no scratch, occupancy 6 / 5."""
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


def _resources(src, tmp_path):
    out = subprocess.run([_hipcc()] + _flags() + ["--cuda-device-only", "-c", src, "-o", str(tmp_path / "k.o"),
                                                  "-Rpass-analysis=kernel-resource-usage"],
                         cwd=CSRC, capture_output=True, text=True, timeout=600)
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


def test_klt_fb_kernel_has_no_scratch_and_occupancy_5(tmp_path):
    res = _resources("vo_klt_fb.hip", tmp_path)
    fb = {k: v for k, v in res.items() if "k_klt_track_fb" in k}
    assert len(fb) == 1, sorted(res)                       # ONE instantiation
    (r,) = fb.values()
    assert r["ScratchSize"] == 0 and r["Occupancy"] >= 5, r


def test_klt_track_resources_unchanged(tmp_path):
    res = _resources("vo_klt.hip", tmp_path)
    want = {4: (81, 5), 5: (81, 5), 6: (79, 6)}
    for wv, (vgpr, occ) in want.items():
        (r,) = [v for k, v in res.items() if re.search(r"k_klt_trackILi%dE" % wv, k)]
        assert (r["VGPRs"], r["TotalSGPRs"], r["ScratchSize"], r["Occupancy"]) == (vgpr, 88, 0, occ), (wv, r)
