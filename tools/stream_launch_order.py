#!/usr/bin/env python3
"""Which kernels go to which stream, in which order: the shipped library against lib/libvo_mi355x_b.so (csrc/Makefile: make OBJDIR=build_b OUT=...).

usage: tools/stream_launch_order.py OUTDIR [config ...]     (from the repository root; configs default to all of CONFIGS)

Every configuration is a short fixed bench run under `rocprofv3 --kernel-trace` (no counters in the same run), once per library, one host thread.
From each trace the kernel names are listed per queue / stream in dispatch order (ids renamed by first appearance; repeats folded: `name xN`,
and `{ ... } xN` for a block of lines that comes N times in a row) and written to OUTDIR/stream_launch_order_<config>.txt together with the
verdict: the lists of the two libraries are identical (then one list is written) or they are not (then both).
A change of the host path that moves a launch to another stream, drops one or reorders two shows up here; kernel times do not enter.
Stops at the first run that fails (exit status 2); exit status 1 if any configuration differs.
"""
import csv, glob, os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = "--steps 6 --warmup 2 --no-extras --no-cpu-baseline --seqs 32 --ctxs 1 --host-threads 1"
CONFIGS = {
    "frame_step_default": COMMON,
    "frame_step_side_stream_on": COMMON + " --side-stream on",
    "frame_step_side_stream_off": COMMON + " --side-stream off",
    "frame_step_graph": COMMON + " --graph",
    "closed_loop": COMMON + " --workload pipeline",
    "closed_loop_host_frames": COMMON + " --workload pipeline --pipe-host-frames",
}
LIB_B = os.path.join(ROOT, "visual-odom-pipeline_amd", "lib", "libvo_mi355x_b.so")


def trace(outdir, name, which, args):
    d = os.path.join(outdir, "trace_%s_%s" % (name, which))
    env = dict(os.environ)
    env.pop("VO_MI355X_LIB", None)
    if which == "b":
        env["VO_MI355X_LIB"] = LIB_B
    cmd = ["timeout", "-k", "10", "240", "rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "-o", "t", "--",
           sys.executable, os.path.join(ROOT, "bench.py")] + args.split()
    with open(d + ".log", "w") as log:
        rc = subprocess.call(cmd, cwd=ROOT, env=env, stdout=log, stderr=subprocess.STDOUT)
    if rc != 0:
        print("%s, library %s: exit status %d (see %s.log): nothing more is run" % (name, which, rc, d), flush=True)
        sys.exit(2)
    rows = list(csv.DictReader(open(sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[-1])))
    key = "Stream_Id" if rows and "Stream_Id" in rows[0] else "Queue_Id"
    rows.sort(key=lambda r: int(r["Dispatch_Id"] if "Dispatch_Id" in r else r["Start_Timestamp"]))
    ids, lists = {}, {}
    for r in rows:
        q = ids.setdefault(r[key], len(ids))
        n = re.sub(r"\(.*$", "", r["Kernel_Name"].replace("void ", "")).replace(" [clone .kd]", "")
        lists.setdefault(q, []).append(n)
    return key, len(rows), {q: fold(names) for q, names in lists.items()}


def fold(tok):
    """runs of a repeated block of tokens -> one token `{ block } xN` (a single name: `name xN`); passes until nothing folds, so blocks nest"""
    while True:
        out, i, changed = [], 0, False
        while i < len(tok):
            best = (1, 1)                                     # (period, repeats) that covers the most tokens from i on
            for p in range(1, min(64, (len(tok) - i) // 2) + 1):
                k = 1
                while tok[i + k * p:i + (k + 1) * p] == tok[i:i + p]:
                    k += 1
                if k > 1 and p * k > best[0] * best[1]:
                    best = (p, k)
            p, k = best
            if k == 1:
                out.append(tok[i])
            elif p == 1 and "\n" not in tok[i]:
                out.append("%s x%d" % (tok[i], k))
            else:
                out.append("{\n%s\n} x%d" % ("\n".join("  " + line for t in tok[i:i + p] for line in t.split("\n")), k))
            changed = changed or k > 1
            i += p * k
        tok = out
        if not changed:
            return tok


def main(outdir, names):
    os.makedirs(outdir, exist_ok=True)
    differ = 0
    for name in names:
        got = {w: trace(outdir, name, w, CONFIGS[name]) for w in ("a", "b")}
        same = got["a"][2] == got["b"][2]
        differ += 0 if same else 1
        with open(os.path.join(outdir, "stream_launch_order_%s.txt" % name), "w") as f:
            f.write("bench.py %s\nunder rocprofv3 --kernel-trace; kernel names per %s in dispatch order, ids by first appearance\n" % (CONFIGS[name], got["a"][0]))
            f.write("library a = the shipped build, library b = lib/libvo_mi355x_b.so (the parent commit): %s\n" % ("IDENTICAL" if same else "DIFFERENT"))
            for w in ("a",) if same else ("a", "b"):
                f.write("\n==== library %s: %d dispatches ====\n" % ("a and b alike" if same else w, got[w][1]))
                for q in sorted(got[w][2]):
                    f.write("-- %s %d --\n%s\n" % (got[w][0], q, "\n".join(got[w][2][q])))
        print("%-28s a: %5d dispatches on %d, b: %5d on %d (%s): %s" % (name, got["a"][1], len(got["a"][2]), got["b"][1], len(got["b"][2]), got["a"][0],
                                                                        "identical" if same else "DIFFERENT"), flush=True)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2:] or list(CONFIGS)))
