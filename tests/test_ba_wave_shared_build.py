"""CPU-only: what hipcc makes of the four wave-walk bundle-adjustment kernel templates (gfx950 device-only cross-compile, no GPU).

k_ba_build_w (csrc/vo_ba_wave.h) and k_ba_build_f (csrc/vo_ba_factored.hip) call ONE definition of the phases they share (the chunk
prefetch, the camera staging, the observation, the landmark factor, the Gram phase, the fold), and k_ba_update_w linearises through the
same observation, as do the trial-cost loops of both updates and the slot loop of k_ba_update_f.  Sharing the text must leave every one
of the 50 instances of the four templates where it was: registers and scratch not above, occupancy and LDS equal, and the same count of
every f64, MFMA, LDS, global, buffer and scratch instruction as the build of the commit before the phases were shared
(tests/golden/ba_wave_parent_opcodes.json: made from that commit with build_helpers, never from the tree under test).

The record, from a checkout of the parent commit (git worktree add ../parent HEAD~1; run there with tests/ on sys.path): for src in
vo_ba.hip, vo_ba_factored.hip and every k, r of kernel_resources(src) whose name matches TEMPLATE,
    h = kernel_opcodes(src, re.escape(k[2:]))
    rec[k] = {"src": src, "VGPRs": r["VGPRs"], "ScratchSize": r["ScratchSize"], "Occupancy": r["Occupancy"], "LDS": r["LDS"],
              "ops": {o: n for o, n in h.items() if PINNED.match(o)},
              "other_vector": sum of the other v_* counts, "scalar": sum of everything else}
written with json.dump(rec, f, sort_keys=True, separators=(",", ":")), one kernel per line."""
import json
import os
import re
import sys

import pytest

from build_helpers import ROOT, kernel_opcodes, kernel_resources

sys.path.insert(0, os.path.join(ROOT, "tools"))
import ba_loop_opcodes  # noqa: E402

PINNED = re.compile(r"^(v_\w+_f64|v_mfma\w*|ds_\w+|global_\w+|buffer_\w+|scratch_\w+)$")
TEMPLATE = re.compile(r"_Z\d+k_ba_(build|update)_[wf]I")
# instances per template: k_ba_build_w 8 geometries x 4 losses, k_ba_update_w 4 x 4, the factored pair once each
N_INSTANCES = {"k_ba_build_w": 32, "k_ba_update_w": 16, "k_ba_build_f": 1, "k_ba_update_f": 1}
# walk loop, per landmark chunk, of the four headline instances: (f64 vector, other vector, MFMA, LDS, global)
WALK = {"k_ba_build_wILi4ELi2ELi5ELi0E": (679, 268, 90, 80, 22), "k_ba_build_fILi4ELi2ELi5ELi0E": (451, 274, 90, 62, 22),
        "k_ba_update_wILi2ELi5ELi0E": (259, 91, 0, 6, 11), "k_ba_update_fILi2ELi5ELi0E": (229, 85, 0, 6, 11)}


@pytest.fixture(scope="module")
def parent():
    rec = json.load(open(os.path.join(ROOT, "tests", "golden", "ba_wave_parent_opcodes.json")))
    count = {t: sum(1 for k in rec if re.match(r"_Z\d+%sI" % t, k)) for t in N_INSTANCES}
    assert count == N_INSTANCES and len(rec) == 50, count
    for k, r in rec.items():
        assert r["VGPRs"] > 0 and r["Occupancy"] >= 2 and any(o.endswith("_f64") for o in r["ops"]) and all(PINNED.match(o) for o in r["ops"]), k
    return rec


@pytest.fixture(scope="module")
def now():
    return {src: {k: v for k, v in kernel_resources(src).items() if TEMPLATE.match(k)} for src in ("vo_ba.hip", "vo_ba_factored.hip")}


def test_the_instantiated_kernels_are_the_parents(parent, now):
    assert sorted(k for res in now.values() for k in res) == sorted(parent)
    for k, r in parent.items():
        assert k in now[r["src"]], k


def test_resources_of_every_instance_not_above_the_parents(parent, now):
    for k, want in sorted(parent.items()):
        r = now[want["src"]][k]
        print(k, {f: (want[f], r[f]) for f in ("VGPRs", "ScratchSize", "Occupancy", "LDS")})
        assert r["VGPRs"] <= want["VGPRs"] and r["ScratchSize"] <= want["ScratchSize"], (k, want, r)
        assert r["Occupancy"] == want["Occupancy"] and r["LDS"] == want["LDS"], (k, want, r)


def test_f64_mfma_and_memory_opcodes_of_every_instance_equal_the_parents(parent):
    """each v_*_f64, v_mfma*, ds_*, global_*, buffer_* and scratch_* opcode as often as in the parent's build of the same instance; the totals
    of the integer vector and the scalar instructions are printed, not asserted"""
    bad = {}
    for k, want in sorted(parent.items()):
        got = kernel_opcodes(want["src"], re.escape(k[2:]))
        pinned = {o: n for o, n in got.items() if PINNED.match(o)}
        diff = {o: (want["ops"].get(o, 0), pinned.get(o, 0)) for o in sorted(set(want["ops"]) | set(pinned)) if want["ops"].get(o, 0) != pinned.get(o, 0)}
        ov = sum(n for o, n in got.items() if o.startswith("v_") and not PINNED.match(o))
        sc = sum(n for o, n in got.items() if not o.startswith("v_") and not PINNED.match(o))
        print("%s: other vector %d -> %d, scalar / other %d -> %d" % (k, want["other_vector"], ov, want["scalar"], sc))
        if diff:
            bad[k] = diff
    assert not bad, "(parent, now): %s" % bad


@pytest.mark.parametrize("kernel", sorted(WALK))
def test_walk_loop_class_counts_of_the_headline_instances(kernel):
    (src, marker), = [(s, m) for s, k, m in ba_loop_opcodes.KERNELS if k == kernel]
    h = ba_loop_opcodes.loop_counts(src, kernel, marker)
    print(kernel, dict(h))
    assert tuple(h[c] for c in ("f64 vector", "other vector", "MFMA", "LDS", "global")) == WALK[kernel]
