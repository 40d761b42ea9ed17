#!/bin/bash
# quick iteration on the box: GPU tests, headline bench with the live roofline (no CPU leg / secondaries),
# kernel-trace profile (bench and profile logs under $OUT_DIR, default bench_out/ in the repository root)
cd "$(dirname "$0")/.." || exit 1
export PYTHONUNBUFFERED=1
TAG=${1:-q}
shift
R=$(pwd)
OUT=$(mkdir -p "${OUT_DIR:-bench_out}" && cd "${OUT_DIR:-bench_out}" && pwd) || exit 1
bash tools/gpu_tests.sh "$@" || exit 1
timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-secondary --wm-steps 0 > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err || { tail -30 $OUT/bench_$TAG.err; exit 1; }
cat $OUT/bench_$TAG.json
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o p -- python3 $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-secondary --wm-steps 0 > $OUT/prof_$TAG.log 2>&1 || { tail -20 $OUT/prof_$TAG.log; exit 1; }
cd $R && python tools/prof_summary.py $OUT/prof_$TAG/p_results.db 30
