#!/bin/bash
# HBM-side traffic of one short bench run, per kernel: two separate PMC passes
# (FETCH_SIZE and WRITE_SIZE cannot share a pass on gfx950), kernel trace only.
#   bash tools/pmc_traffic.sh TAG [bench.py args]    (on the GPU box; results under $OUT_DIR, default bench_out/)
set -o pipefail
TAG=${1:-x}
shift
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "${OUT_DIR:-$R/bench_out}" && cd "${OUT_DIR:-$R/bench_out}" && pwd) || exit 1
cd /tmp && export TMPDIR=/tmp
for c in FETCH_SIZE WRITE_SIZE; do
  timeout -k 10 300 rocprofv3 --pmc $c --kernel-trace --output-format csv -d $OUT/pmc_$c$TAG -o p \
    -- python3 $R/bench.py --full --steps 3 --warmup 1 --no-cpu-baseline --no-secondary --wm-steps 0 "$@" > $OUT/pmc_$c$TAG.log 2>&1 \
    || { tail -20 $OUT/pmc_$c$TAG.log; exit 1; }
done
cd $R && python3 tools/pmc_traffic.py $OUT/pmc_FETCH_SIZE$TAG $OUT/pmc_WRITE_SIZE$TAG --json $OUT/traffic$TAG.json > $OUT/traffic$TAG.txt
cat $OUT/traffic$TAG.txt
