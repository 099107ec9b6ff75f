"""CPU-only: the two structures of the sparse image alignment (include/vo_mi355x.h) against their ctypes mirrors, the default
parameters and the exports."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mirrors_have_no_hidden_padding_and_match_the_host_compiler(tmp_path):
    from vo_mi355x import _lib
    assert ctypes.sizeof(_lib.AlignParams) == 32 and ctypes.sizeof(_lib.AlignStats) == 56
    # no hidden padding: the fields' sizes add up to the structure's
    for T in (_lib.AlignParams, _lib.AlignStats):
        assert sum(ctypes.sizeof(t) for _, t in T._fields_) == ctypes.sizeof(T)
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    pf = ("max_level", "min_level", "max_iters", "min_points", "huber", "eps", "form", "reserved")
    sf = ("status", "n_used", "levels_run", "flags", "iters", "chi2", "zbar")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vo_mi355x.h"\nint main(void) { printf("%zu %zu", sizeof(vo_align_params), '
                   'sizeof(vo_align_stats));\n' + "".join('printf(" %%zu", offsetof(vo_align_params, %s));\n' % f for f in pf) +
                   "".join('printf(" %%zu", offsetof(vo_align_stats, %s));\n' % f for f in sf) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [ctypes.sizeof(_lib.AlignParams), ctypes.sizeof(_lib.AlignStats)] + [getattr(_lib.AlignParams, f).offset for f in pf] + \
        [getattr(_lib.AlignStats, f).offset for f in sf]
    assert got == want, (got, want)


def test_default_parameters():
    from vo_mi355x import _lib
    L = _lib.load()
    p = _lib.AlignParams(max_level=7, min_level=7, max_iters=-1, min_points=-1, huber=-1.0, eps=-1.0, form=9, reserved=9)
    assert L.vo_align_default_params(ctypes.byref(p)) == 0
    assert (p.max_level, p.min_level, p.max_iters, p.min_points, p.huber, p.form, p.reserved) == (-1, 0, 10, 10, 10.0, 0, 0)
    assert p.eps == ctypes.c_float(1e-5).value
    assert L.vo_align_default_params(None) == -1


def test_exports_are_present():
    import vo_mi355x
    from vo_mi355x import Extractor, VoContext, _lib
    L = _lib.load()
    assert hasattr(L, "vo_sparse_align") and hasattr(L, "vo_align_default_params")
    assert vo_mi355x.AlignParams is _lib.AlignParams and vo_mi355x.AlignStats is _lib.AlignStats
    assert all(hasattr(VoContext, f) for f in ("align_params", "sparse_align"))
    assert all(hasattr(Extractor, f) for f in ("align_frame", "project_landmarks"))
    import inspect
    assert inspect.signature(Extractor.extend_tracks).parameters["init"].default is None
    assert inspect.signature(Extractor.extend_landmarks).parameters["init"].default is None
