#!/bin/bash
# fp8 suites + the ResNet-50 fp8 bench line with the tuner's log (run on the GPU box from the repo root)
OUT=${1:?usage: scripts/job_f8.sh <output dir>}
mkdir -p "$OUT"
python -m pytest tests -m gpu -q -s -k "fp8 or config4" > $OUT/r3_tf8.log 2>&1; echo "pytest rc=$?" >> $OUT/r3_tf8.log
grep -E "weights-stationary|passed|failed|Error|error|rc=" $OUT/r3_tf8.log | tail -14
python bench.py --full --model resnet50 --dtype f8 --no-secondary --cpu-sample 0 --no-hostpath > $OUT/r3_bench_f8.json 2> $OUT/r3_bench_f8.err
python - "$OUT/r3_bench_f8.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print(d["dtype"], d["value"], d["ms_per_step"], d["kernel_families_ms"])
PY
IE_PRECISION=fp8 python scripts/profile_steps.py 256 resnet50 > $OUT/r3_steps_f8.txt 2>&1; grep -E "proj|^#" $OUT/r3_steps_f8.txt
