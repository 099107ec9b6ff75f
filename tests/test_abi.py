"""CPU-only: the C-ABI library loads and exports every symbol include/vo_mi355x.h declares; host-side glue."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "vo_mi355x.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(vo_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    from vo_mi355x import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    assert len(names) >= 25
    for n in names:
        assert hasattr(L, n), "libvo_mi355x.so does not export %s" % n
    assert set(names) == set(_lib.SIGNATURES), set(names) ^ set(_lib.SIGNATURES)
    assert _lib.load().vo_abi_version() == 4


def test_the_limited_detection_is_declared_with_host_limits():
    """vo_shi_tomasi_resident_limit(ctx, n_cur, mask_radius, prm, const int32_t* limits): the resident call's arguments + one limit per sequence"""
    from vo_mi355x import _lib
    txt = open(os.path.join(ROOT, "include", "vo_mi355x.h")).read()
    assert re.search(r"int32_t vo_shi_tomasi_resident_limit\(vo_ctx\* ctx, int32_t n_cur, int32_t mask_radius, const vo_st_params\* prm, "
                     r"const int32_t\* limits\);", txt)
    res, args = _lib.SIGNATURES["vo_shi_tomasi_resident_limit"]
    assert res is ctypes.c_int32 and args[:4] == _lib.SIGNATURES["vo_shi_tomasi_resident"][1] and args[4] is ctypes.POINTER(ctypes.c_int32)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "vo_shi_tomasi_resident_limit")


def test_struct_layouts_match_header():
    from vo_mi355x import _lib
    assert ctypes.sizeof(_lib.KltParams) == 32 and ctypes.sizeof(_lib.StParams) == 40
    assert ctypes.sizeof(_lib.BaParams) == 56 and ctypes.sizeof(_lib.BaStats) == 40
    assert ctypes.sizeof(_lib.PnpParams) == 24 and ctypes.sizeof(_lib.PnpStats) == 24
    assert ctypes.sizeof(_lib.EssParams) == 32 and ctypes.sizeof(_lib.EssStats) == 24 and ctypes.sizeof(_lib.SiftKp) == 24
    L = _lib.load()
    k = _lib.KltParams(); L.vo_klt_default_params(ctypes.byref(k))
    assert (k.win, k.max_level, k.max_count) == (31, 3, 30) and abs(k.epsilon - 0.03) < 1e-15
    s = _lib.StParams(); L.vo_st_default_params(ctypes.byref(s))
    assert (s.max_corners, s.block_size) == (1000, 31) and s.quality_level == 0.03 and s.min_distance == 7.0
    assert s.use_harris == 0 and s.harris_k == 0.04          # the reference never turns the Harris response on (extractor.py:21-24)
    b = _lib.BaParams(); L.vo_ba_default_params(ctypes.byref(b))
    assert b.ftol == 1e-3 and b.xtol == 1e-3 and b.huber_delta == 1.0


def test_python_mirrors_of_the_pipe_constants_match_header():
    """resident.INFLIGHT bounds how long step_host keeps a step's images referenced: it must be the library's in-flight limit"""
    from vo_mi355x import resident
    txt = open(os.path.join(ROOT, "include", "vo_mi355x.h")).read()
    assert int(re.search(r"#define VO_PIPE_INFLIGHT (\d+)", txt).group(1)) == resident.INFLIGHT
    assert int(re.search(r"#define VO_PIPE_HIST (\d+)", txt).group(1)) == resident.HIST


def test_the_library_reads_no_tuning_from_the_environment():
    """rounds 1-5 shipped 23 getenv switches; forced forms now go through vo_set_tuning.  What is left: VO_BLOCKING_SYNC (how a host thread
    waits) and the VO_STEP_TRACE debug trace."""
    src = os.path.join(ROOT, "visual-odom-pipeline_amd", "csrc")
    found = []
    for f in sorted(os.listdir(src)):
        if f.endswith((".hip", ".h")):
            found += re.findall(r'getenv\("([A-Z_0-9]+)"\)', open(os.path.join(src, f)).read())
    assert sorted(set(found)) == ["VO_BLOCKING_SYNC", "VO_STEP_TRACE"], found
    from vo_mi355x import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "vo_mi355x.h")).read(), flags=re.S)
    body = re.search(r"typedef struct \{([^}]*)\} vo_tuning;", hdr).group(1)
    assert tuple(re.findall(r"int32_t\s+(\w+);", body)) == _lib.TUNING_FIELDS


def test_no_stage_picks_its_stream_from_swapped_context_state():
    """Enqueue functions take their stream as an argument: the ctx stream is assigned where the context is created and where it is re-created
    with a CU mask, nowhere else, and the fields that carried per-call arguments of a stage through the context are gone.
    A source scan of the pattern this code base used (`c->stream = ...` inside a function defined in column 0): a swap through another spelling of
    the context (`ctx->stream`, `std::swap`) would get past it."""
    src = os.path.join(ROOT, "visual-odom-pipeline_amd", "csrc")
    assigned_in = set()
    for f in sorted(os.listdir(src)):
        if not f.endswith((".hip", ".h")):
            continue
        txt = open(os.path.join(src, f)).read()
        for name in ("in_step", "ba_wait_before_publish", "ba_wide_event", "vo_ba_set_live"):
            assert not re.search(r"\b%s\b" % name, txt), (f, name)
        for m in re.finditer(r"c\s*->\s*stream\s*=(?!=)", txt):
            # the enclosing function: the last definition that starts in column 0 before the match
            heads = re.findall(r"^(?:extern \"C\" |static )?[A-Za-z_][\w \*:<>]*?\b(\w+)\s*\([^;{]*\)\s*\{", txt[:m.start()], flags=re.M)
            assigned_in.add(heads[-1] if heads else f)
    assert assigned_in <= {"vo_ctx_create_batched", "vo_main_stream_reserve"}, assigned_in
    assert "vo_main_stream_reserve" in assigned_in          # (the pattern still finds an assignment where there is one)


def test_no_cpu_fallback_without_a_device():
    """On a box without a GPU the product must fail loudly, not compute on the CPU."""
    from vo_mi355x import _lib, VoContext, VoError
    n = ctypes.c_int32(-1)
    rc = _lib.load().vo_device_count(ctypes.byref(n))
    if rc == 0 and n.value > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(VoError):
        VoContext(64, 64)


def test_product_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "visual-odom-pipeline_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f)).read()
                bad = re.findall(r"^\s*(?:import|from)\s+(?:\w*_oracle|cv2|oracle)\b|#include\s+\"[^\"]*oracle"
                                 r"|libvo_oracle|ref_stub/", txt, flags=re.M)
                assert not bad, (f, bad)


def test_oracle_does_not_import_the_product():
    """the checker stands on its own: nothing under oracle/ imports the package it checks (round-4 review: pipe_oracle.py took its SO(3)
    log map from vo_mi355x.so3)"""
    for dp, _, files in os.walk(os.path.join(ROOT, "oracle")):
        for f in files:
            if f.endswith((".py", ".c", ".h")):
                txt = open(os.path.join(dp, f)).read()
                bad = re.findall(r"^\s*(?:import|from)\s+vo_mi355x\b|#include\s+\"[^\"]*vo_mi355x", txt, flags=re.M)
                assert not bad, (f, bad)


def test_synthetic_generators():
    from vo_mi355x import synthetic as syn
    fr, mo = syn.make_sequence(2, w=160, h=120, margin=48)
    assert fr.dtype == np.uint8 and fr.shape == (2, 120, 160) and 100 < fr.mean() < 156 and fr.std() > 20
    p = syn.grid_points(100, 160, 120, margin=10)
    assert p.shape == (100, 2) and p.dtype == np.float32
    s = syn.make_ba_scene(50, 5)
    assert s["obs"].shape == (5, 50, 2) and not np.isnan(s["obs"]).any()
    s = syn.make_ba_scene(50, 5, visibility=0.5)
    assert np.isnan(s["obs"]).any()


def test_ctypes_mirrors_have_the_c_structs_sizes(tmp_path):
    """the structures of include/vo_mi355x.h, compiled by the host compiler, against their ctypes mirrors in vo_mi355x/_lib.py (a field added
    on one side only would make every later field read garbage)"""
    import shutil
    import subprocess
    from vo_mi355x import _lib
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler")
    pairs = [("vo_pipe_record", _lib.PipeRecord), ("vo_pipe_params", _lib.PipeParams), ("vo_klt_params", _lib.KltParams), ("vo_st_params", _lib.StParams),
             ("vo_ba_params", _lib.BaParams), ("vo_ba_stats", _lib.BaStats), ("vo_pnp_params", _lib.PnpParams), ("vo_pnp_stats", _lib.PnpStats),
             ("vo_tuning", _lib.Tuning)]
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "vo_mi355x.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n' % (
        " ".join(["%zu"] * len(pairs)), ", ".join("sizeof(%s)" % n for n, _ in pairs)))
    exe = tmp_path / "sizes"
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    for (name, mirror), size in zip(pairs, got):
        assert ctypes.sizeof(mirror) == size, (name, ctypes.sizeof(mirror), size)


def test_headline_ba_kernels_keep_their_register_budget():
    """`k_ba_build_w<4, 2, 5, huber>` / `k_ba_update_w<2, 5, huber>` (the headline's window-10 instances) must fit 256 vector registers at two waves per SIMD WITHOUT
    scratch: round 5 shipped the build kernel with 136 bytes per lane of spills (stored and reloaded per landmark chunk: 10 % of the fully active launch).
    hipcc's resource remarks of a device-only compile (cross-compiles here, no GPU)."""
    from build_helpers import kernel_resources
    res = kernel_resources("vo_ba.hip")
    seen = 0
    for mangled in ("_Z12k_ba_build_wILi4ELi2ELi5ELi0EE", "_Z13k_ba_update_wILi2ELi5ELi0EE"):
        m = [v for k, v in res.items() if k.startswith(mangled)]
        assert m, mangled
        vgprs, scratch, occ = m[0]["VGPRs"], m[0]["ScratchSize"], m[0]["Occupancy"]
        assert scratch == 0 and vgprs <= 256 and occ >= 2, (mangled, vgprs, scratch, occ)
        seen += 1
    assert seen == 2
