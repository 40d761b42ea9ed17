#!/bin/bash
# GPU box: all -m gpu tests, then one full bench line (with the WM-step secondary)
#   bash tools/gpu_all.sh TAG          (logs under $OUT_DIR, default bench_out/)
set -o pipefail
TAG=${1:-x}
OUT=${OUT_DIR:-bench_out}
mkdir -p "$OUT"
timeout -k 10 400 python -u -m pytest tests -m gpu -x -v --timeout 180 --timeout-method thread > $OUT/gpu_tests$TAG.log 2>&1 || { tail -40 $OUT/gpu_tests$TAG.log; exit 1; }
tail -3 $OUT/gpu_tests$TAG.log
timeout -k 10 300 python bench.py --full --steps 20 --warmup 3 > $OUT/bench$TAG.json 2> $OUT/bench$TAG.err || { tail -20 $OUT/bench$TAG.err; exit 1; }
cat $OUT/bench$TAG.json
