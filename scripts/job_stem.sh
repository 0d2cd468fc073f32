#!/bin/bash
# stem + pool fusion: its tests, the fp8 / fp16 suites that run through it, and the three bench lines (run on the GPU box from the repo root)
OUT=${1:?usage: scripts/job_stem.sh <output dir>}
mkdir -p "$OUT"
python -m pytest tests -m gpu -q -s -k "stem or fp8 or fp16 or config" > $OUT/r3_tstem.log 2>&1; echo "pytest rc=$?" >> $OUT/r3_tstem.log
grep -E "stem \+ pool|passed|failed|Error|error|rc=" $OUT/r3_tstem.log | tail -14
IE_TUNE_LOG=1 python bench.py --full > $OUT/r3_bench_stem.json 2> $OUT/r3_bench_stem.err
grep "stem + pool" $OUT/r3_bench_stem.err | head
python - "$OUT/r3_bench_stem.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
print(d["dtype"], d["value"], d["ms_per_step"], d.get("modelinfer_images_per_s"), d["kernel_families_ms"])
for s in d["secondary"]:
    print(s["dtype"], s["value"], s["ms_per_step"], s.get("modelinfer_images_per_s"), s.get("modelinfer_uint8_images_per_s"), s["kernel_families_ms"])
PY
