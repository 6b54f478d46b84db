#!/bin/bash
# SENSE tests and micro-benchmark, every GPU test, then the full bench line; logs under $1.
set -o pipefail
OUT=${1:?usage: tools/gpu_round.sh OUTDIR}
mkdir -p "$OUT"
timeout -k 10 300 python -u -m pytest tests/test_gpu_sense.py -x -q --timeout 120 --timeout-method thread > "$OUT/sense_tests.log" 2>&1 || { echo SENSE_TESTS_FAILED; tail -30 "$OUT/sense_tests.log"; exit 1; }
tail -2 "$OUT/sense_tests.log"
timeout -k 10 120 python tools/sense_bench.py > "$OUT/sense_fast.log" 2>&1 || { echo SENSE_BENCH_FAILED; tail -30 "$OUT/sense_fast.log"; exit 1; }
cat "$OUT/sense_fast.log"
DLCS_SENSE_GENERIC=1 timeout -k 10 120 python tools/sense_bench.py > "$OUT/sense_generic.log" 2>&1 || { echo SENSE_BENCH_FAILED; tail -30 "$OUT/sense_generic.log"; exit 1; }
cat "$OUT/sense_generic.log"
timeout -k 10 900 python -u -m pytest tests -x -q -m gpu --timeout 300 --timeout-method thread > "$OUT/gpu_tests.log" 2>&1 || { echo GPU_TESTS_FAILED; tail -30 "$OUT/gpu_tests.log"; exit 1; }
tail -2 "$OUT/gpu_tests.log"
timeout -k 10 600 python bench.py --full > "$OUT/bench.log" 2>&1 || { echo BENCH_FAILED; tail -30 "$OUT/bench.log"; exit 1; }
tail -1 "$OUT/bench.log"
