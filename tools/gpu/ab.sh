#!/bin/bash
# Interleaved A/B of engine builds (BK_LIB per run; "" = the in-tree library) on one leg:
#   selfplay  bench.py --workload selfplay (STEPS / WARMUP plies, default 6 / 2)   sims/s
#   leafnet   tools/leafnet_bench.py 300 256                                       k_leafnet_x3 us per launch
#   learner   bench.py --workload train (STEPS / WARMUP, default 20 / 5)           samples/s
#   legal     tools/legal_scale.py 4096                                            us per launch
# TESTS=<test file> first runs that file's GPU tests once per library. Then ROUNDS rounds (default 2),
# libraries innermost, every step under its own timeout, stopping at the first failing step; last, each
# library's median, minimum and maximum over the rounds.
# Usage: [ROUNDS=3] [TESTS=tests/test_leafnet_gpu.py] bash tools/gpu/ab.sh LEG "" blokus_rl_amd/_lib/ab/X/libblokus_hip.so ...
cd "$(dirname "$0")/../.." || exit 1
leg=$1; shift
case $leg in
  selfplay) lim=200 cmd="bench.py --workload selfplay --full --steps ${STEPS:-6} --warmup ${WARMUP:-2} --late-plies 0 --no-cpu-baseline"
            num="round(d['value']), 'step_us', round(d['search_roofline']['k_leaf_step_us'], 1)" ;;
  leafnet)  lim=120 cmd="tools/leafnet_bench.py 300 256" num="d['us_per_launch']" ;;
  learner)  lim=300 cmd="bench.py --workload train --steps ${STEPS:-20} --warmup ${WARMUP:-5} --no-cpu-baseline"
            num="round(d.get('learner', d)['value']), 'ms', round(d.get('learner', d)['ms_per_step'], 3)" ;;
  legal)    lim=120 cmd="tools/legal_scale.py 4096" num="d['us_per_launch']['4096']" ;;
  *) echo "usage: $0 selfplay|leafnet|learner|legal lib..."; exit 2 ;;
esac
OUT=${OUT:-bench_out}/ab
mkdir -p $OUT
fail() { echo "$1 failed: [$lib]"; tail -20 $2; exit 1; }
for lib in ${TESTS:+"$@"}; do
  BK_LIB=$lib timeout -k 10 300 python -u -m pytest -x -q --timeout 120 --timeout-method thread -m gpu $TESTS \
    > $OUT/tests.log 2>&1 || fail tests $OUT/tests.log
  echo "tests ok: [$lib] $(tail -1 $OUT/tests.log)"
done
: > $OUT/$leg.txt
for r in $(seq 1 ${ROUNDS:-2}); do
  for lib in "$@"; do
    BK_LIB=$lib timeout -k 10 $lim python $cmd > $OUT/$leg.json 2> $OUT/$leg.err || fail $leg $OUT/$leg.err
    python -c "import json,sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print('[%s]' % sys.argv[2], $num)" $OUT/$leg.json "$lib" >> $OUT/$leg.txt || exit 1
    tail -1 $OUT/$leg.txt
  done
done
python -c "
import statistics, sys
runs = {}
for line in open(sys.argv[1]):
    lib, x = line.split()[:2]
    runs.setdefault(lib, []).append(float(x))
for lib, x in runs.items():
    print('$leg', lib, 'median %.7g min %.7g max %.7g over %d' % (statistics.median(x), min(x), max(x), len(x)))
" $OUT/$leg.txt
