OUT=${OUT:-bench_out}; mkdir -p "$OUT"
tools/gpu/tests.sh tests/test_train_conv_gpu.py tests/test_train_bn_gpu.py tests/test_train_fc_gpu.py tests/test_learner.py tests/test_dist_gpu.py tests/test_nets.py && timeout -k 10 300 python bench.py --workload train --no-cpu-baseline > "$OUT/train.json" && python -c "
import json, sys; d=json.load(open(sys.argv[1])); print(d['value'], d['ms_per_step'], d['roofline']['kernel_ms'], d['wgrad_roofline']['kernel_ms'], d['fp32_miopen_same_batch'], d['at_reference_batch_64'])" "$OUT/train.json"
