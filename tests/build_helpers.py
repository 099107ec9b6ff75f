"""What hipcc makes of a translation unit of csrc/ (gfx950 device-only cross-compile, no GPU needed), for the CPU tests that pin a kernel's
registers, scratch, occupancy and instruction counts.  Compiled with the Makefile's own flags; every unit is compiled once per test run."""
import collections
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual-odom-pipeline_amd", "csrc")


def hipcc():
    for p in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if p and os.path.exists(p):
            return p
    pytest.skip("no hipcc")


def makefile_flags():
    """CXXFLAGS of the Makefile, as the library is built"""
    mk = open(os.path.join(CSRC, "Makefile")).read()
    m = re.search(r"^CXXFLAGS \?=(.*?)(?<!\\)\n", mk, flags=re.M | re.S)
    flags = m.group(1).replace("\\\n", " ").replace("$(ARCH)", "gfx950").split()
    return [f for f in flags if f != "-fPIC"]


@functools.lru_cache(maxsize=None)
def _device_compile(src):
    """(device assembly, the compiler's remarks) of csrc/<src>"""
    cc = hipcc()
    with tempfile.TemporaryDirectory() as td:
        asm = os.path.join(td, "k.s")
        out = subprocess.run([cc] + makefile_flags() + ["--cuda-device-only", "-S", src, "-o", asm, "-Rpass-analysis=kernel-resource-usage"],
                             cwd=CSRC, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        return open(asm).read(), out.stderr


def kernel_resources(src):
    """mangled kernel name -> {TotalSGPRs, VGPRs, ScratchSize [bytes/lane], Occupancy [waves/SIMD], LDS [bytes/block]} of csrc/<src>"""
    res, cur = {}, None
    for line in _device_compile(src)[1].splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1); res[cur] = {}
            continue
        m = re.search(r"remark:\s+(TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur:
            res[cur][m.group(1).split()[0]] = int(m.group(2))
    return res


def kernel_opcodes(src, kernel):
    """opcode -> count over the device assembly of the one kernel of csrc/<src> whose mangled name contains `kernel`"""
    lines = _device_compile(src)[0].split("\n")
    (start,) = [i for i, l in enumerate(lines) if re.match(r"_Z\w*%s\w*:" % kernel, l)]
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    h = collections.Counter()
    for l in lines[start + 1:end]:
        m = re.match(r"\s+([a-z][a-z0-9_]+)(\s|$)", l)
        if m:
            h[m.group(1)] += 1
    return h
