#!/bin/bash
# fp16 weights-stationary / dense-block tests + the fp16 B=128 bench line with the tuner's log (run on the GPU box from the repo root)
OUT=${1:?usage: scripts/job_f16.sh <output dir>}
mkdir -p "$OUT"
python -m pytest tests -m gpu -q -s -k "fp16_weights_stationary or dense_block" > $OUT/r3_t3.log 2>&1; echo "pytest rc=$?" >> $OUT/r3_t3.log
grep -E "passed|failed|Error|error|rc=" $OUT/r3_t3.log | tail -6
IE_TUNE_LOG=1 python bench.py --full --dtype f16 --batch 128 --no-secondary --cpu-sample 0 --no-hostpath > $OUT/r3_bench_f16.json 2> $OUT/r3_bench_f16.err
grep -E "k=3x3|kh=3|3x3" $OUT/r3_bench_f16.err | head -30
python - "$OUT/r3_bench_f16.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print(d["value"], d["ms_per_step"], d["kernel_families_ms"])
PY
IE_PRECISION=fp16 python scripts/profile_steps.py 128 > $OUT/r3_steps_f16.txt 2>&1; grep -E "conv3x3|^#" $OUT/r3_steps_f16.txt | head -8
