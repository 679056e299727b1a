#!/bin/bash
# GPU box job for a kernel change: the GPU parity suite, one short bench line (no variants, no
# CPU baseline) and, with DIAG=1, the per-wave cycle split of the stamps build.
set -o pipefail
cd "$GRAFT_REPO_ROOT"
export OUT=${OUT:-bench_out}; mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 300 python -u -m pytest tests -x -q -m gpu --timeout 120 --timeout-method thread > $OUT/pytest_gpu.log 2>&1 || { echo "pytest failed rc=$?"; tail -40 $OUT/pytest_gpu.log; exit 1; }
tail -2 $OUT/pytest_gpu.log
NOVAR=--no-variants; [ -n "$VARIANTS" ] && NOVAR=--full
timeout -k 10 300 python bench.py --steps 5 --warmup 1 --cpu-sample 0 $NOVAR ${BENCH_ARGS} > $OUT/bench_quick.json 2> $OUT/bench_quick.err || { echo "bench failed rc=$?"; tail -30 $OUT/bench_quick.err; exit 1; }
python -c "import json; r=json.load(open('$OUT/bench_quick.json')); print('value', r['value'], 'kernel_ms', r['roofline']['kernel_ms_avg']); [print(k, v['value'], v['kernel_ms_avg']) for k, v in r.get('variants', {}).items()]"
if [ -n "$DIAG" ]; then
  timeout -k 10 300 python scripts/diag_stamps.py 4096 f64 logmap > $OUT/diag.log 2>&1 || { echo "diag failed"; tail -20 $OUT/diag.log; exit 1; }
  cat $OUT/diag.log
fi
