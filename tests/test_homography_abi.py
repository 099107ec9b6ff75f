"""CPU-only: the two structures of the homography search (include/vo_mi355x.h) against their ctypes mirrors, and the default parameters."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mirrors_are_32_bytes_and_match_the_host_compiler(tmp_path):
    from vo_mi355x import _lib
    assert ctypes.sizeof(_lib.HomParams) == 32 and ctypes.sizeof(_lib.HomStats) == 32
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vo_mi355x.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(vo_hom_params), sizeof(vo_hom_stats), offsetof(vo_hom_params, refine_iters), offsetof(vo_hom_stats, n_inliers), '
                   'offsetof(vo_hom_stats, lm_iters), offsetof(vo_hom_params, max_iters)); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [ctypes.sizeof(_lib.HomParams), ctypes.sizeof(_lib.HomStats), _lib.HomParams.refine_iters.offset, _lib.HomStats.n_inliers.offset,
                   _lib.HomStats.lm_iters.offset, _lib.HomParams.max_iters.offset], got


def test_default_parameters():
    from vo_mi355x import _lib
    L = _lib.load()
    p = _lib.HomParams(threshold=-1.0, confidence=-1.0, max_iters=-1, seed=-1, refine_iters=-1, _pad=-1)
    assert L.vo_homography_default_params(ctypes.byref(p)) == 0
    assert (p.threshold, p.confidence, p.max_iters, p.refine_iters, p.seed, p._pad) == (3.0, 0.995, 2000, 10, 0, 0)
    assert L.vo_homography_default_params(None) == -1
    assert L.vo_abi_version() == 4
