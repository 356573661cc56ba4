#!/bin/bash
# The scan that sizes the CSR rows, one build of libdatok_gpu.so (P, the parent) against another (N): per-kernel
# times with three batches in flight, the bench alternated, streams_1, the result arrays compared, and the guard
# workloads (tiny, config3, robust, shard).  Each step is a process of its own under a time limit; the first step
# that fails ends the script.  Run from the repository root.
# usage: tail_ab.sh <parent .so> <new .so> <out dir> [steps: trace bench long full dump tiny config3 robust shard]
set -o pipefail
P=$(readlink -f "$1"); N=$(readlink -f "$2"); OUT=$3; shift 3
STEPS=${*:-trace bench long full dump tiny config3 robust shard}
mkdir -p "$OUT"
export TMPDIR=/tmp
CPUS=$(nproc); [ "$CPUS" -gt 16 ] && CPUS=16
export OMP_NUM_THREADS=$CPUS
lib() { [ "$1" = P ] && echo "$P" || echo "$N"; }
line() {  # the bench's JSON line -> its figures
  python3 -c "
import sys, json
for l in sys.stdin:
    if l.startswith('{'):
        j = json.loads(l); print('$1', 'MB/s', j['value'], 'ms_per_step', j['ms_per_step'])
        if j.get('streams_1'):  # (--full) one batch alone: ms per kernel
            print('   streams_1', 'MB/s', j['streams_1']['value'], 'stages_ms', j['streams_1']['stages_ms'])"
}
echo "tail_ab.sh, steps: $STEPS.  P = the first library (the parent commit's), N = the second."
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
  bench|long)  # alternated, three fresh processes each
    extra=""; [ $step = long ] && extra="--steps 5000 --warmup 50"
    for r in 1 2 3; do for v in P N; do
      DATOK_GPU_LIB=$(lib $v) timeout -k 10 180 python3 bench.py --gpus 1 $extra 2>/dev/null | line $v || exit 1
    done; done ;;
  full)  # streams_1 and the parity gate
    DATOK_GPU_LIB=$N timeout -k 10 400 python3 bench.py --gpus 1 --full --no-cpu-baseline 2>$OUT/full_stderr.log | tee $OUT/full_N.json | line N || exit 1 ;;
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
  tiny)  # guards, P N P N: N must not fall behind P by more than the two P runs differ.  64-byte documents: the three-launch scan
    for v in P N P N; do
      echo "-- tiny_docs $v"; DATOK_GPU_LIB=$(lib $v) timeout -k 10 180 python3 scripts/tiny_docs.py 2>&1 | cut -c1-330 || exit 1
    done ;;
  config3)  # 65 536 documents
    for v in P N P N; do
      echo -n "-- config 3 $v: "; DATOK_GPU_LIB=$(lib $v) ONLY=3 timeout -k 10 300 python3 scripts/configs.py 2>&1 | tail -1 | cut -c1-200 || exit 1
    done ;;
  robust)  # rich corpora
    for v in P N P N; do
      echo "-- robust $v"; DATOK_GPU_LIB=$(lib $v) timeout -k 10 300 python3 scripts/robust.py 2>&1 | tail -6 | cut -c1-200 || exit 1
    done ;;
  shard)  # (a 1.3 GB batch: the generator takes most of the minute)
    for v in P N P N; do
      echo -n "shard (--docs 327680 --streams 1) "; DATOK_GPU_LIB=$(lib $v) timeout -k 10 300 python3 bench.py --gpus 1 --docs 327680 --streams 1 2>/dev/null | line $v || exit 1
    done ;;
  *) echo "unknown step $step"; exit 2 ;;
  esac
done
