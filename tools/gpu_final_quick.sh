#!/bin/bash
# Last short GPU visit of a round: the whole GPU test suite, then the bench line of the default model without the CPU leg.
#   gpurun --timeout 240 -- 'bash tools/gpu_final_quick.sh <tag>'
tag=${1:-x}; R=$(cd "$(dirname "$0")/.." && pwd); cd $R; OUT=${OUT:-$R/visit_out}; mkdir -p $OUT; export TMPDIR=/tmp
timeout 170 python -m pytest tests -m gpu -q -p no:cacheprovider -x > $OUT/pytest_gpu_$tag.log 2>&1; echo "pytest rc=$?" >> $OUT/pytest_gpu_$tag.log
tail -3 $OUT/pytest_gpu_$tag.log
timeout 80 python bench.py --full --no-cpu-baseline > $OUT/bench_$tag.json 2> $OUT/bench_$tag.err; echo "bench rc=$?"
python - <<PY
import json
try:
    d = json.load(open('$OUT/bench_$tag.json'))
    print('value', d['value'], d['ms_per_step'], 'roofline', d['roofline']['frac'], d['roofline']['avg_launch_us'], 'parity', d['parity'], 'protocol', d['fps_reference_protocol'])
except Exception as e:
    print('parse failed', e); print(open('$OUT/bench_$tag.err').read()[-800:])
PY
