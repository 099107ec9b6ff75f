"""CPU-only: the two structures of the Sim(3) search (include/vo_mi355x.h) against their ctypes mirrors, and the default parameters."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mirrors_are_32_bytes_and_match_the_host_compiler(tmp_path):
    from vo_mi355x import _lib
    assert ctypes.sizeof(_lib.Sim3Params) == 32 and ctypes.sizeof(_lib.Sim3Stats) == 32
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    pf = ("threshold", "confidence", "max_iters", "seed", "with_scale", "refit")
    sf = ("cost", "n_inliers", "hypotheses", "best", "status", "degenerate", "refit")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vo_mi355x.h"\nint main(void) { printf("%zu %zu", sizeof(vo_sim3_params), '
                   'sizeof(vo_sim3_stats));\n' + "".join('printf(" %%zu", offsetof(vo_sim3_params, %s));\n' % f for f in pf) +
                   "".join('printf(" %%zu", offsetof(vo_sim3_stats, %s));\n' % f for f in sf) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [ctypes.sizeof(_lib.Sim3Params), ctypes.sizeof(_lib.Sim3Stats)] + [getattr(_lib.Sim3Params, f).offset for f in pf] + \
        [getattr(_lib.Sim3Stats, f).offset for f in sf]
    assert got == want, (got, want)


def test_default_parameters():
    from vo_mi355x import _lib
    L = _lib.load()
    p = _lib.Sim3Params(threshold=-1.0, confidence=-1.0, max_iters=-1, seed=-1, with_scale=-1, refit=-1)
    assert L.vo_sim3_default_params(ctypes.byref(p)) == 0
    assert (p.threshold, p.confidence, p.max_iters, p.seed, p.with_scale, p.refit) == (3.0, 0.99, 1000, 0, 1, 1)
    assert L.vo_sim3_default_params(None) == -1
    assert L.vo_abi_version() == 4


def test_the_python_layers_are_exported():
    import vo_mi355x
    from vo_mi355x import Extractor, VoContext, evaluate
    assert vo_mi355x.ate is evaluate.ate and vo_mi355x.align_trajectory is evaluate.align_trajectory
    assert all(hasattr(VoContext, f) for f in ("estimate_sim3", "fit_sim3")) and hasattr(Extractor, "align_landmarks")
