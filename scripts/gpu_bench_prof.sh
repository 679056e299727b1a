#!/bin/bash
# Parity tests, one full bench line, rocprofv3 kernel-trace summary; output under $OUT (default bench_out/).
set -o pipefail
cd "$GRAFT_REPO_ROOT"
export OUT=${OUT:-bench_out}; mkdir -p $OUT
export TMPDIR=/tmp
timeout -k 10 600 python -m pytest tests -x -q -m gpu > $OUT/pytest_gpu.log 2>&1 || { echo "pytest failed rc=$?"; tail -30 $OUT/pytest_gpu.log; exit 1; }
tail -3 $OUT/pytest_gpu.log
timeout -k 10 600 python bench.py --full ${BENCH_ARGS:---steps 3 --warmup 1} > $OUT/bench.json 2> $OUT/bench.err || { echo "bench failed rc=$?"; tail -30 $OUT/bench.err; exit 1; }
cat $OUT/bench.json
if [ -n "$PROF" ]; then
  timeout -k 10 600 rocprofv3 --kernel-trace --stats -d $OUT/prof -o run --output-format csv -- python3 bench.py --steps 3 --warmup 1 --cpu-sample 0 --no-variants > $OUT/prof.log 2>&1 || { echo "rocprof failed rc=$?"; tail -20 $OUT/prof.log; exit 1; }
  find $OUT/prof -name "*stats*" | head
fi
if [ -n "$DIAG" ]; then
  timeout -k 10 300 python scripts/diag_stamps.py 4096 f64 logmap > $OUT/diag.log 2>&1 && \
  timeout -k 10 300 python scripts/diag_stamps.py 4096 f64 maxlog >> $OUT/diag.log 2>&1 || { echo "diag failed"; tail -20 $OUT/diag.log; exit 1; }
  cat $OUT/diag.log
fi
if [ -n "$UBENCH" ]; then
  timeout -k 10 120 ./scripts/ubench_latency > $OUT/ubench.log 2>&1; cat $OUT/ubench.log
fi
