"""CPU-only: the two structures of the ORB detector (include/vo_mi355x.h) against their ctypes mirrors and the host compiler, and the defaults."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PARAM_FIELDS = ("nfeatures", "nlevels", "scale_factor", "fast_threshold", "edge_threshold", "harris_k")
KP_FIELDS = ("x", "y", "size", "angle", "response", "octave", "lx", "ly")


def test_mirrors_are_32_bytes_and_match_the_host_compiler(tmp_path):
    from vo_mi355x import _lib
    import orb_model as om
    assert ctypes.sizeof(_lib.OrbParams) == 32 and ctypes.sizeof(_lib.OrbKp) == 32
    assert _lib.ORB_KP_DTYPE.itemsize == 32 and _lib.ORB_KP_DTYPE == om.KP_DTYPE
    assert [_lib.ORB_KP_DTYPE.fields[f][1] for f in KP_FIELDS] == [getattr(_lib.OrbKp, f).offset for f in KP_FIELDS]
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vo_mi355x.h"\nint main(void) { printf("%zu %zu", sizeof(vo_orb_params), sizeof(vo_orb_kp));\n'
                   + "".join('printf(" %%zu", offsetof(vo_orb_params, %s));\n' % f for f in PARAM_FIELDS)
                   + "".join('printf(" %%zu", offsetof(vo_orb_kp, %s));\n' % f for f in KP_FIELDS) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [32, 32] + [getattr(_lib.OrbParams, f).offset for f in PARAM_FIELDS] + [getattr(_lib.OrbKp, f).offset for f in KP_FIELDS]
    assert got == want, (got, want)


def test_default_parameters():
    from vo_mi355x import _lib
    L = _lib.load()
    p = _lib.OrbParams(nfeatures=-1, nlevels=-1, scale_factor=-1.0, fast_threshold=-1, edge_threshold=-1, harris_k=-1.0, _pad=-1)
    assert L.vo_orb_default_params(ctypes.byref(p)) == 0
    assert (p.nfeatures, p.nlevels, p.scale_factor, p.fast_threshold, p.edge_threshold, p._pad) == (500, 8, 1.2, 20, 31, 0)
    assert np.float32(p.harris_k) == np.float32(0.04)
    assert L.vo_orb_default_params(None) == -1
    assert L.vo_abi_version() == 4


def test_the_calls_refuse_a_null_context():
    from vo_mi355x import _lib
    L = _lib.load()
    assert L.vo_orb_detect_compute(None, None, 0, None, None, None, 1, None, None, None) == -1
    assert L.vo_orb_levels_read(None, None, None, None, None, None) == -1
    assert L.vo_orb_level_image_read(None, 0, 0, None) == -1
