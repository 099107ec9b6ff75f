#!/bin/bash
# VALU instruction counters and single-stream launch time of the plain tracker with and without the kept target window (k_klt_track<6>: vo_tuning.klt_reuse = -1;
# k_klt_track_r: 1) on the same launch, 32 sequences x 2000 keypoints; counters and kernel trace in runs of their own (tools/pmc_klt_pair.sh)  -> $OUT_DIR/klt_reuse_valu.txt (OUT_DIR: default profile_out/ in the repository root)
OUT=${OUT_DIR:-$PWD/profile_out}; mkdir -p $OUT
export TMPDIR=/tmp
BENCH="$PWD/bench.py"
cd /tmp
for MODE in -1 1; do
  rm -rf $OUT/kreuse_c$MODE $OUT/kreuse_t$MODE
  timeout -k 10 400 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_LDS SQ_INSTS_VMEM_RD SQ_WAVES --output-format csv -d $OUT/kreuse_c$MODE -o c -- python3 $BENCH --full --steps 4 --warmup 2 --regions 1 --no-extras --no-cpu-baseline --seqs 32 --ctxs 1 --tune klt_reuse=$MODE > $OUT/kreuse_c$MODE.log 2>&1 || { echo "counter run $MODE failed"; exit 1; }
  timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/kreuse_t$MODE -o t -- python3 $BENCH --full --steps 20 --warmup 5 --regions 1 --no-extras --no-cpu-baseline --seqs 32 --ctxs 1 --side-stream off --tune klt_reuse=$MODE > $OUT/kreuse_t$MODE.log 2>&1 || { echo "trace run $MODE failed"; exit 1; }
done
cd - > /dev/null
python3 - <<PY > $OUT/klt_reuse_valu.txt
import csv, glob
from collections import defaultdict
print("k_klt_track<6> (klt_reuse=-1) vs k_klt_track_r<6> (klt_reuse=1), one launch = 32 sequences x 2000 keypoints, bit-identical outputs")
for mode in (-1, 1):
    f = sorted(glob.glob("$OUT/kreuse_c%d/**/*counter_collection.csv" % mode, recursive=True))[-1]
    acc = defaultdict(lambda: [0.0, 0])
    for r in csv.DictReader(open(f)):
        if "k_klt_track" in r["Kernel_Name"]:
            a = acc[r["Counter_Name"]]; a[0] += float(r["Counter_Value"]); a[1] += 1
    m = {k: v[0] / max(v[1], 1) for k, v in acc.items()}
    t = sorted(glob.glob("$OUT/kreuse_t%d/**/*kernel_stats.csv" % mode, recursive=True))[-1]
    us = [float(r["AverageNs"]) / 1e3 for r in csv.DictReader(open(t)) if "k_klt_track" in r["Name"]]
    print("klt_reuse=%2d: per keypoint SQ_INSTS_VALU %.0f, SQ_INSTS_LDS %.1f, SQ_INSTS_VMEM_RD %.1f; SQ_WAVES %.0f; %.1f us per launch (rocprofv3 --stats, single stream)"
          % (mode, m.get("SQ_INSTS_VALU", 0) / 64000.0, m.get("SQ_INSTS_LDS", 0) / 64000.0, m.get("SQ_INSTS_VMEM_RD", 0) / 64000.0, m.get("SQ_WAVES", 0), us[0] if us else -1))
PY
rm -rf $OUT/kreuse_t*/*/*kernel_trace.csv $OUT/kreuse_t*/*kernel_trace.csv
cat $OUT/klt_reuse_valu.txt
