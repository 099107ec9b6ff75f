#!/bin/bash
# A/B of two vo_tuning settings of ONE library inside ONE visit (boxes differ by a few per cent), interleaved a b b a a b ...:
#   tools/ab_tune.sh klt_reuse=-1 klt_reuse=1 [runs per side, default 6] ["bench args"]      -> $OUT_DIR/ab_tune.txt (OUT_DIR: default profile_out/ in the repository root)
# Every run has its own time limit and a failed run ends the script.  The verdict is the rule of EXPERIMENTS.md ("keep the target window"): b counts as
# a gain when its median exceeds a's by more than a's own span (max - min) in this visit and b's worst run is not below a's median.
set -o pipefail
A=${1:?tune of side a}; B=${2:?tune of side b}; N=${3:-6}
ARGS=${4:---no-extras --no-cpu-baseline}
OUT=${OUT_DIR:-$PWD/profile_out}; mkdir -p $OUT
: > $OUT/ab_tune.txt
for r in $(seq $N); do
  order="a b"; [ $((r % 2)) = 0 ] && order="b a"
  for which in $order; do
    T=$A; [ $which = b ] && T=$B
    line=$(timeout -k 10 300 python3 bench.py $ARGS --tune $T 2>/dev/null | tail -1) || { echo "side $which ($T): run failed, stopping"; exit 1; }
    python3 -c 'import json, sys; d = json.loads(sys.argv[1]); print("%s %s %.1f frames/s %.4f ms/step" % (sys.argv[2], sys.argv[3], d["value"], d["ms_per_step"]))' "$line" $which $T \
      | tee -a $OUT/ab_tune.txt || { echo "side $which ($T): no result line, stopping"; exit 1; }
  done
done
python3 - $OUT/ab_tune.txt <<'P' | tee -a $OUT/ab_tune.txt
import statistics, sys
v = {"a": [], "b": []}
for l in open(sys.argv[1]):
    f = l.split()
    if len(f) >= 3 and f[0] in v:
        v[f[0]].append(float(f[2]))
ma, mb = statistics.median(v["a"]), statistics.median(v["b"])
sa, sb = max(v["a"]) - min(v["a"]), max(v["b"]) - min(v["b"])
gain = mb - ma > sa and min(v["b"]) >= ma
print("median a %.1f (span %.1f = %.2f %%)  median b %.1f (span %.1f = %.2f %%)  b/a %+.2f %%  worst b %.1f  -> %s"
      % (ma, sa, 100 * sa / ma, mb, sb, 100 * sb / mb, 100 * (mb / ma - 1), min(v["b"]), "GAIN" if gain else "no gain"))
P
