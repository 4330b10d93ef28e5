#!/bin/bash
# The whole bench line (bench.py --full, N=1), optionally followed by the same command under
# rocprofv3 --kernel-trace --stats (PROFILE=1; the stats CSV -> $OUT/bench_kernel_stats.csv).
#   tools/gpu/bench.sh [steps] [warmup]
cd "$GRAFT_REPO_ROOT" || exit 1
export TMPDIR=/tmp
OUT=${OUT:-bench_out}  # where the outputs go
mkdir -p $OUT
S=${1:-20} W=${2:-5}
timeout -k 10 420 python bench.py --gpus 1 --steps $S --warmup $W --full > $OUT/bench.json 2> $OUT/bench.err \
  || { tail -20 $OUT/bench.err; exit 1; }
cat $OUT/bench.json
if [ "${PROFILE:-0}" = "1" ]; then
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d /tmp/bench_kt -o kt --output-format csv -- python bench.py --gpus 1 --steps $S --warmup $W --full \
    > $OUT/bench_kt.json 2> $OUT/bench_kt.err || { tail -20 $OUT/bench_kt.err; exit 1; }
  for f in $(find /tmp/bench_kt -name "*kernel_stats.csv"); do grep -q k_leaf_step_ov $f && cp $f $OUT/bench_kernel_stats.csv; done
  head -12 $OUT/bench_kernel_stats.csv | cut -c1-160
fi
