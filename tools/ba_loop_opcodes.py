#!/usr/bin/env python3
"""Instructions per landmark chunk of the wave-private bundle-adjustment kernels, counted in the ISA of their walk loops (gfx950 device-only
cross-compile with the Makefile's flags, no GPU needed) -- the table of EXPERIMENTS.md, "Factored BA build / update".

usage: tools/ba_loop_opcodes.py            (from the repository root)

The walk loop of a kernel is taken as the innermost loop around its marker instruction (the MFMA of the build kernels, the ds_bpermute of the
update kernels): from the target of the first backward branch behind the last marker that lies in front of the first marker, to that branch.
Registers and scratch come from the compiler's resource remarks (tests/build_helpers.py)."""
import collections
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from build_helpers import _device_compile, kernel_resources  # noqa: E402

KERNELS = [("vo_ba.hip", "k_ba_build_wILi4ELi2ELi5ELi0E", "mfma"), ("vo_ba_factored.hip", "k_ba_build_fILi4ELi2ELi5ELi0E", "mfma"),
           ("vo_ba.hip", "k_ba_update_wILi2ELi5ELi0E", "ds_bpermute"), ("vo_ba_factored.hip", "k_ba_update_fILi2ELi5ELi0E", "ds_bpermute")]
CLASSES = ("f64 vector", "other vector", "MFMA", "LDS", "global", "scalar / other")


def classify(op):
    if "mfma" in op:
        return "MFMA"
    if re.match(r"v_\w+_f64", op):
        return "f64 vector"
    if op.startswith("v_"):
        return "other vector"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "global"
    return "scalar / other"


def loop_counts(src, kernel, marker):
    lines = _device_compile(src)[0].split("\n")
    (start,) = [i for i, l in enumerate(lines) if re.match(r"_Z\w*%s\w*:" % kernel, l)]
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    body = lines[start:end]
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"(\.LBB\d+_\d+):", l)] if m}
    marks = [i for i, l in enumerate(body) if marker in l]
    for i in range(marks[-1], len(body)):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", body[i])
        if m and labels.get(m.group(1), len(body)) <= marks[0]:
            first, last = labels[m.group(1)], i
            break
    else:
        raise SystemExit("no loop around %s in %s" % (marker, kernel))
    h = collections.Counter()
    for l in body[first:last + 1]:
        m = re.match(r"\s+([a-z][a-z0-9_]+)(\s|$)", l)
        if m:
            h[classify(m.group(1))] += 1
    return h


if __name__ == "__main__":
    print("%-34s %s   vector  VGPRs SGPRs scratch" % ("kernel (walk loop, per chunk)", "  ".join("%14s" % c for c in CLASSES)))
    for src, kernel, marker in KERNELS:
        h = loop_counts(src, kernel, marker)
        (r,) = [v for k, v in kernel_resources(src).items() if kernel in k]
        print("%-34s %s   %6d  %5d %5d %7d" % (kernel, "  ".join("%14d" % h[c] for c in CLASSES), h["f64 vector"] + h["other vector"],
                                                r["VGPRs"], r["TotalSGPRs"], r["ScratchSize"]))
