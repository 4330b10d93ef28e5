#!/bin/bash
# Self-play sims/s per tree-group schedule (BK_SIM_GROUPS x BK_SIM_RING), interleaved over
# ROUNDS rounds of the driver's command, every run's dumped outputs compared with the first leg's,
# then (TRACE=1) one kernel trace per leg read with tools/sim_groups_trace.py.
# Usage: bash tools/gpu/sim_groups_ab.sh [K:ring ...]      (default: 1:0 2:1 2:0 4:2 4:1 4:0)
cd "$(dirname "$0")/../.." || exit 1
OUT=${OUT:-bench_out}/sim_groups
DUMPS=$(mktemp -d)
mkdir -p $OUT
LEGS=${@:-1:0 2:1 2:0 4:2 4:1 4:0}
S=${STEPS:-20} W=${WARMUP:-5}
for r in $(seq 1 ${ROUNDS:-3}); do
  for leg in $LEGS; do
    k=${leg%:*} ring=${leg#*:} name=k${leg%:*}_ring${leg#*:}_r$r
    BK_SIM_GROUPS=$k BK_SIM_RING=$ring timeout -k 10 300 python bench.py --gpus 1 --steps $S --warmup $W --dump-outputs $DUMPS/$name \
      > $OUT/$name.json 2> $OUT/$name.err || { echo "failed: $name"; tail -5 $OUT/$name.err; exit 1; }
    python -c "import json,sys; d=json.loads(open(sys.argv[1]).read().strip().splitlines()[-1]); print(sys.argv[2], round(d['value']), 'ms_per_step', round(d['ms_per_step'], 3))" $OUT/$name.json $name
  done
done
python - $DUMPS <<'EOF' || exit 1
import os, sys
import numpy as np
root = sys.argv[1]
runs = sorted(os.listdir(root))
ref = runs[0]
bad = [(d, f) for d in runs[1:] for f in sorted(os.listdir(os.path.join(root, ref)))
       if not np.array_equal(np.load(os.path.join(root, ref, f)), np.load(os.path.join(root, d, f)))]
print("dumped outputs of", len(runs), "runs:", "all equal" if not bad else f"DIFFERENT {bad}")
sys.exit(1 if bad else 0)
EOF
rm -rf $DUMPS
[ "${TRACE:-0}" = "1" ] || exit 0
for leg in $LEGS; do
  k=${leg%:*} ring=${leg#*:} name=k${leg%:*}_ring${leg#*:}
  KT=$(mktemp -d)
  BK_SIM_GROUPS=$k BK_SIM_RING=$ring timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $KT -o kt --output-format csv -- \
    python bench.py --gpus 1 --steps $S --warmup $W > $OUT/kt_$name.json 2> $OUT/kt_$name.err || { echo "trace failed: $name"; tail -5 $OUT/kt_$name.err; exit 1; }
  echo -n "$name: "
  python tools/sim_groups_trace.py "$(find $KT -name '*kernel_trace.csv' | head -1)" $OUT/trace_$name.json $W $S 100 $k || exit 1
  rm -rf $KT
done
