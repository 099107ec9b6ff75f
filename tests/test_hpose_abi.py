"""CPU-only: the two structures of the pose from a homography (include/vo_mi355x.h) against their ctypes mirrors, the default parameters,
and the exports."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mirrors_are_48_and_80_bytes_and_match_the_host_compiler(tmp_path):
    from vo_mi355x import _lib
    assert ctypes.sizeof(_lib.HposeParams) == 48 and ctypes.sizeof(_lib.HposeStats) == 80
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    pf = ("ratio", "threshold", "hint", "min_off", "use_hint")
    sf = ("sigma", "n_solutions", "n_distinct", "ambiguous", "status", "n_mask", "n_good", "n_off", "_pad")
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "vo_mi355x.h"\nint main(void) { printf("%zu %zu", sizeof(vo_hpose_params), '
                   'sizeof(vo_hpose_stats));\n' + "".join('printf(" %%zu", offsetof(vo_hpose_params, %s));\n' % f for f in pf) +
                   "".join('printf(" %%zu", offsetof(vo_hpose_stats, %s));\n' % f for f in sf) + 'printf("\\n"); return 0; }\n')
    exe = tmp_path / "sizes"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [48, 80] + [getattr(_lib.HposeParams, f).offset for f in pf] + [getattr(_lib.HposeStats, f).offset for f in sf]
    assert got == want, (got, want)


def test_default_parameters_and_exports():
    from vo_mi355x import _lib
    L = _lib.load()
    p = _lib.HposeParams(ratio=-1.0, threshold=-1.0, min_off=-1, use_hint=-1)
    p.hint[:] = [-1.0, -1.0, -1.0]
    assert L.vo_homography_pose_default_params(ctypes.byref(p)) == 0
    assert (p.ratio, p.threshold, list(p.hint), p.min_off, p.use_hint) == (0.75, 1.0, [0.0, 0.0, 0.0], 8, 0)
    assert L.vo_homography_pose_default_params(None) == -1
    assert L.vo_abi_version() == 4
    for name in ("vo_homography_decompose", "vo_homography_pose"):
        assert getattr(L, name) is not None
    # a null context is refused before anything else is looked at
    assert L.vo_homography_decompose(None, None, None, None, None, None, 0, None, None, None, None, None) == -1
    assert L.vo_homography_pose(None, None, None, None, 0, None, None, None, None, None, None, None, None, None) == -1
