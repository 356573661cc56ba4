#!/bin/bash
# The symboliser, one build of libdatok_gpu.so (P, the parent) against another (N): per-kernel times with three
# batches in flight, instruction counts, the kernel alone on a full chip, the bench alternated, the result arrays
# compared, and the guard workloads.  Each step is a process of its own under a time limit; the first step that
# fails ends the script.  Run from the repository root.
# usage: symbolize_ab.sh <parent .so> <new .so> <out dir> [steps: trace pmc stages bench long full dump guards]
set -o pipefail
P=$(readlink -f "$1"); N=$(readlink -f "$2"); OUT=$3; shift 3
STEPS=${*:-trace pmc stages bench long full dump guards}
mkdir -p "$OUT"
export TMPDIR=/tmp
lib() { [ "$1" = P ] && echo "$P" || echo "$N"; }
line() {  # the bench's JSON line -> its three figures
  python3 -c "
import sys, json
for l in sys.stdin:
    if l.startswith('{'):
        j = json.loads(l); print('$1', 'MB/s', j['value'], 'ms_per_step', j['ms_per_step'])
        if j.get('streams_1'):  # (--full) one batch alone: ms per kernel
            print('   streams_1', 'MB/s', j['streams_1']['value'], 'stages_ms', j['streams_1']['stages_ms'])"
}
echo "symbolize_ab.sh, steps: $STEPS.  P = the first library (the parent commit's), N = the second."
for step in $STEPS; do
  echo "==== $step"
  case $step in
  trace)  # per-kernel durations with three batches in flight (the profiler slows the bench itself: its line is not a figure)
    for v in P N; do
      d=$OUT/trace_$v; mkdir -p $d
      DATOK_GPU_LIB=$(lib $v) timeout -k 10 240 rocprofv3 --kernel-trace --stats --output-format csv -d $d -o bench -- \
        python3 bench.py --gpus 1 > $d/stdout.log 2>&1 || exit 1
      f=$(find $d -name "*kernel_stats.csv" | head -1)
      echo "-- $v"
      python3 - "$f" <<'PY' | tee $OUT/kernel_stats_$v.txt
import csv, sys
for r in csv.DictReader(open(sys.argv[1])):
    print("  %-30s calls %4s  average %9.1f ns  min %8s  max %8s" % (r["Name"].split("(")[0][:30], r["Calls"], float(r["AverageNs"]), r["MinNs"], r["MaxNs"]))
PY
      find $d -name "*kernel_trace.csv" -delete
    done ;;
  pmc)  # counters only, no tracing beside them
    for v in P N; do
      d=$OUT/pmc_$v; mkdir -p $d
      DATOK_GPU_LIB=$(lib $v) timeout -k 10 240 rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_INSTS_LDS SQ_WAVES --output-format csv -d $d -o pmc -- \
        python3 bench.py --gpus 1 --steps 6 --warmup 3 > $d/stdout.log 2>&1 || exit 1
      f=$(find $d -name "*counter_collection.csv" | head -1)
      echo "-- $v"
      python3 - "$f" <<'PY' | tee $OUT/pmc_$v.txt
import csv, sys, collections
agg = collections.defaultdict(lambda: collections.defaultdict(float)); n = collections.Counter()
for r in csv.DictReader(open(sys.argv[1])):
    k = r["Kernel_Name"].split("(")[0][:60]
    agg[k][r["Counter_Name"]] += float(r["Counter_Value"]); n[(k, r["Counter_Name"])] += 1
for k, v in agg.items():
    if "symbolize" not in k: continue
    per = {c: val / max(1, n[(k, c)]) for c, val in v.items()}
    print(k)
    for c, val in sorted(per.items()):
        print("   %-16s %14.1f per dispatch  %8.1f per wave" % (c, val, val / max(1.0, per.get("SQ_WAVES", 1.0))))
PY
      find $d -name "*.csv" -size +4M -delete
    done ;;
  stages)  # every kernel alone on a full chip
    for v in P N; do
      echo -n "$v "; DATOK_GPU_LIB=$(lib $v) timeout -k 10 120 python3 scripts/big_stages.py 2>&1 | tail -1 || exit 1
    done ;;
  bench|long)  # alternated, three fresh processes each
    extra=""; [ $step = long ] && extra="--steps 5000 --warmup 50"
    for r in 1 2 3; do for v in P N; do
      DATOK_GPU_LIB=$(lib $v) timeout -k 10 180 python3 bench.py --gpus 1 $extra 2>/dev/null | line $v || exit 1
    done; done ;;
  full)  # streams_1 and the parity gate
    DATOK_GPU_LIB=$N timeout -k 10 400 python3 bench.py --gpus 1 --full 2>$OUT/full_stderr.log | tee $OUT/full_N.json | line N || exit 1 ;;
  dump)  # the result arrays of both builds, array for array
    for v in P N; do
      DATOK_GPU_LIB=$(lib $v) timeout -k 10 180 python3 bench.py --gpus 1 --dump-outputs $OUT/dump_$v 2>/dev/null | line $v || exit 1
    done
    python3 - $OUT/dump_P $OUT/dump_N <<'PY' || exit 1
import os, sys, numpy as np
a, b = sys.argv[1:]
names = sorted(os.listdir(a))
assert names and names == sorted(os.listdir(b)), (names, os.listdir(b))
for n in names:
    x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
    assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y), n
print("dump-outputs: %d arrays equal" % len(names))
PY
    rm -rf $OUT/dump_P $OUT/dump_N ;;
  guards)  # other workloads, P N P N: N must not fall behind P by more than the two P runs differ
    for v in P N P N; do
      echo "-- tiny_docs $v"; DATOK_GPU_LIB=$(lib $v) timeout -k 10 180 python3 scripts/tiny_docs.py 2>&1 | cut -c1-170 || exit 1
    done
    for v in P N P N; do
      echo "-- robust $v"; DATOK_GPU_LIB=$(lib $v) timeout -k 10 300 python3 scripts/robust.py 2>&1 | tail -6 | cut -c1-200 || exit 1
    done
    for v in P N P; do  # (a 1.3 GB batch: the generator takes most of the minute)
      echo -n "shard (--docs 327680 --streams 1) "; DATOK_GPU_LIB=$(lib $v) timeout -k 10 300 python3 bench.py --gpus 1 --docs 327680 --streams 1 2>/dev/null | line $v || exit 1
    done
    for v in P N P N; do
      echo -n "config 4 (tokenizer_de.datok) "; DATOK_GPU_LIB=$(lib $v) timeout -k 10 180 python3 bench.py --gpus 1 --model tests/golden/models/tokenizer_de.datok 2>/dev/null | line $v || exit 1
    done ;;
  *) echo "unknown step $step"; exit 2 ;;
  esac
done
