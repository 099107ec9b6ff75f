#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of the library, kernel by kernel.

usage: tools/device_code_diff.py OBJDIR_A OBJDIR_B    (two csrc/Makefile OBJDIRs built with the same flags)

For every object file the gfx950 code object is taken out of the .hip_fatbin section and disassembled; the instruction stream of every function symbol
(addresses and encodings stripped, so symbol order does not matter) and the set of symbols must be the same on both sides.  Exit status 1 on any difference.
A host-only refactor must leave this at "identical" for all translation units.
"""
import os, re, subprocess, sys, tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def kernels(obj):
    with tempfile.TemporaryDirectory() as td:
        fb, co = os.path.join(td, "dev.hipfb"), os.path.join(td, "dev.co")
        subprocess.run([LLVM + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, obj, os.path.join(td, "host.o")], stderr=subprocess.DEVNULL)
        if not os.path.exists(fb): return {}                                   # a unit without kernels has no such section
        subprocess.run([LLVM + "/clang-offload-bundler", "--type=o", "--targets=" + TARGET, "--input=" + fb, "--output=" + co, "--unbundle"], check=True)
        txt = subprocess.run([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    out, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s*//.*$", "", line).strip())      # (the trailing comment is the address)
    return out


def main(a, b):
    bad = 0
    for name in sorted(f for f in os.listdir(a) if f.endswith(".o")):
        ka, kb = kernels(os.path.join(a, name)), kernels(os.path.join(b, name))
        diff = sorted(set(ka) ^ set(kb)) + sorted(k for k in set(ka) & set(kb) if ka[k] != kb[k])
        print("%-20s %4d symbols, %7d instructions: %s" % (name, len(ka), sum(len(v) for v in ka.values()), "DIFFERENT " + " ".join(diff) if diff else "identical"))
        bad += len(diff)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
