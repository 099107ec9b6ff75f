"""CPU-only: the three structures of the depth filter (include/vo_mi355x.h) against their ctypes mirrors and the host compiler, the default
parameters and the exports."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = {"vo_depth_params": ("max_steps", "max_iters", "max_score", "eps_align", "px_noise", "conv_ratio", "min_inlier", "reserved"),
          "vo_depth_seed": ("mu", "sigma2", "a", "b", "z_range", "u", "v", "ref_id", "flags"),
          "vo_depth_stats": ("counts", "converged", "diverged", "reserved")}


def test_mirrors_have_no_hidden_padding_and_match_the_host_compiler(tmp_path):
    from vo_mi355x import _lib
    import depth_model as dm
    mirrors = {"vo_depth_params": _lib.DepthParams, "vo_depth_seed": _lib.DepthSeed, "vo_depth_stats": _lib.DepthStats}
    assert [ctypes.sizeof(mirrors[k]) for k in FIELDS] == [32, 56, 40]
    for name, T in mirrors.items():
        assert sum(ctypes.sizeof(t) for _, t in T._fields_) == ctypes.sizeof(T) and tuple(f for f, _ in T._fields_) == FIELDS[name]
    # the numpy row the Python layer and the model use is the same 56 bytes
    dt = np.dtype(_lib.DEPTH_SEED_DTYPE)
    assert dt == dm.SEED and dt.itemsize == 56 and [dt.fields[f][1] for f in FIELDS["vo_depth_seed"]] == [getattr(_lib.DepthSeed, f).offset for f in FIELDS["vo_depth_seed"]]
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    src = tmp_path / "sizes.c"
    body = "".join('printf(" %%zu", sizeof(%s));\n' % n + "".join('printf(" %%zu", offsetof(%s, %s));\n' % (n, f) for f in fs) for n, fs in FIELDS.items())
    consts = 'printf(" %d %d %d %d %d %d %d %d %d %d %d", VO_DEPTH_UPDATED, VO_DEPTH_OUTLIER_NOMATCH, VO_DEPTH_OUTLIER_ALIGN, VO_DEPTH_SKIP_INVISIBLE, ' \
             'VO_DEPTH_SKIP_LONG, VO_DEPTH_SKIP_DEGENERATE, VO_DEPTH_SKIP_INACTIVE, VO_DEPTH_CONVERGED, VO_DEPTH_DIVERGED, VO_DEPTH_OBS_SHIFT, VO_PROF_DEPTH);\n'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vo_mi355x.h"\nint main(void) {\n' + body + consts + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = []
    for n, fs in FIELDS.items():
        want += [ctypes.sizeof(mirrors[n])] + [getattr(mirrors[n], f).offset for f in fs]
    want += [dm.UPDATED, dm.OUTLIER_NOMATCH, dm.OUTLIER_ALIGN, dm.SKIP_INVISIBLE, dm.SKIP_LONG, dm.SKIP_DEGENERATE, dm.SKIP_INACTIVE, dm.CONVERGED, dm.DIVERGED,
             dm.OBS_SHIFT, 28]
    assert got == want, (got, want)
    assert _lib.DEPTH_RESULTS == dm.NAMES and (_lib.DEPTH_CONVERGED, _lib.DEPTH_DIVERGED, _lib.DEPTH_OBS_SHIFT) == (dm.CONVERGED, dm.DIVERGED, dm.OBS_SHIFT)


def test_default_parameters():
    from vo_mi355x import _lib
    import depth_model as dm
    L = _lib.load()
    p = _lib.DepthParams(max_steps=-1, max_iters=-1, max_score=-1, eps_align=-1.0, px_noise=-1.0, conv_ratio=-1.0, min_inlier=-1.0, reserved=9)
    assert L.vo_depth_default_params(ctypes.byref(p)) == 0
    d = dm.DEFAULTS
    assert (p.max_steps, p.max_iters, p.max_score, p.reserved) == (d["max_steps"], d["max_iters"], d["max_score"], 0) == (128, 10, 300 * 64, 0)
    for k in ("eps_align", "px_noise", "conv_ratio", "min_inlier"):
        assert getattr(p, k) == ctypes.c_float(d[k]).value, k
    assert (d["eps_align"], d["px_noise"], d["conv_ratio"], d["min_inlier"]) == (0.03, 1.0, 200.0, 0.1)
    assert L.vo_depth_default_params(None) == -1


def test_exports_are_present():
    import vo_mi355x
    from vo_mi355x import Extractor, VoContext, _lib
    L = _lib.load()
    assert all(hasattr(L, f) for f in ("vo_depth_default_params", "vo_depth_seed_init", "vo_depth_update"))
    assert vo_mi355x.DepthParams is _lib.DepthParams and vo_mi355x.DepthSeed is _lib.DepthSeed and vo_mi355x.DepthStats is _lib.DepthStats
    assert all(n in vo_mi355x.__all__ for n in ("DepthParams", "DepthSeed", "DepthStats", "DepthSeeds"))
    assert all(hasattr(VoContext, f) for f in ("depth_params", "depth_seeds", "depth_update"))
    assert all(hasattr(Extractor, f) for f in ("init_seeds", "update_seeds", "seed_landmarks"))
    hdr = open(os.path.join(ROOT, "include", "vo_mi355x.h")).read()
    assert "tests/depth_model.py" in hdr and "VO_PROF_DEPTH = 28, VO_PROF_COUNT = 29" in hdr
