"""CPU-only: the two structures of the fundamental-matrix search (include/vo_mi355x.h) against their ctypes mirrors, and the default
parameters."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mirrors_are_32_bytes_and_match_the_host_compiler(tmp_path):
    from vo_mi355x import _lib
    assert ctypes.sizeof(_lib.FundParams) == 32 and ctypes.sizeof(_lib.FundStats) == 32
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    pf = ("threshold", "confidence", "max_iters", "seed", "refit", "_pad")
    sf = ("cost", "n_inliers", "hypotheses", "best", "status", "n_roots", "models")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vo_mi355x.h"\nint main(void) { printf("%zu %zu", sizeof(vo_fund_params), '
                   'sizeof(vo_fund_stats));\n' + "".join('printf(" %%zu", offsetof(vo_fund_params, %s));\n' % f for f in pf) +
                   "".join('printf(" %%zu", offsetof(vo_fund_stats, %s));\n' % f for f in sf) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [ctypes.sizeof(_lib.FundParams), ctypes.sizeof(_lib.FundStats)] + [getattr(_lib.FundParams, f).offset for f in pf] + \
        [getattr(_lib.FundStats, f).offset for f in sf]
    assert got == want, (got, want)


def test_default_parameters():
    from vo_mi355x import _lib
    L = _lib.load()
    p = _lib.FundParams(threshold=-1.0, confidence=-1.0, max_iters=-1, seed=-1, refit=-1, _pad=-1)
    assert L.vo_fundamental_default_params(ctypes.byref(p)) == 0
    assert (p.threshold, p.confidence, p.max_iters, p.seed, p.refit, p._pad) == (3.0, 0.99, 1000, 0, 0, 0)
    assert L.vo_fundamental_default_params(None) == -1
    assert L.vo_abi_version() == 4
