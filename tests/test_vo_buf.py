"""csrc/vo_buf.h on the host alone: tests/host/vo_buf_check.hip drives the owning buffer and the build-then-attach helper with a malloc / free
memory policy that counts live blocks and refuses the k-th allocation, swept over every position of a workspace's build.  It is built with
AddressSanitizer and UBSan (host code only) and run directly: a double free, a leak or a use after free ends it with a non-zero status.
No GPU, no HIP call."""
import os
import subprocess

from build_helpers import CSRC, ROOT, hipcc


def test_vo_buf_host_check(tmp_path):
    cc = hipcc()
    exe = str(tmp_path / "vo_buf_check")
    build = subprocess.run([cc, "-std=c++17", "-O1", "-g", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                            "-Xarch_host", "-fno-sanitize-recover=all", "-Wall", "-I", CSRC,
                            os.path.join(ROOT, "tests", "host", "vo_buf_check.hip"), "-o", exe],
                           capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "vo_buf_check OK" in run.stdout
    assert "Sanitizer" not in run.stderr and "runtime error" not in run.stderr, run.stderr[-4000:]
