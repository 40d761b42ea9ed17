#!/bin/bash
# SQ / TCC counters of one short bench run per kernel, two passes (8 SQ counters,
# then TCC hit / miss + GRBM), kernel trace only.  Counter list first (-L).
#   bash tools/pmc_sq.sh TAG [bench.py args]    (on the GPU box; results under $OUT_DIR, default bench_out/)
set -o pipefail
TAG=${1:-x}
shift
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "${OUT_DIR:-$R/bench_out}" && cd "${OUT_DIR:-$R/bench_out}" && pwd) || exit 1
cd /tmp && export TMPDIR=/tmp
timeout -s KILL 60 rocprofv3 -L > $OUT/pmc_list$TAG.txt 2>&1 || true
P1="SQ_WAVES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_INSTS_VALU SQ_INSTS_MFMA"
P2="TCC_HIT_sum TCC_MISS_sum GRBM_GUI_ACTIVE"
i=0
for P in "$P1" "$P2"; do
  i=$((i+1))
  timeout -s KILL 240 rocprofv3 --pmc $P --kernel-trace --output-format csv -d $OUT/pmcsq$i$TAG -o p \
    -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-secondary --wm-steps 0 "$@" > $OUT/pmcsq$i$TAG.log 2>&1 \
    || { tail -20 $OUT/pmcsq$i$TAG.log; exit 1; }
done
cd $R && python3 tools/pmc_sq.py $OUT/pmcsq1$TAG $OUT/pmcsq2$TAG > $OUT/pmcsq$TAG.txt && cat $OUT/pmcsq$TAG.txt
