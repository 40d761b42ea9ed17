R=$(cd "$(dirname "$0")/.." && pwd)
OUT=$(mkdir -p "${OUT_DIR:-$R/bench_out}" && cd "${OUT_DIR:-$R/bench_out}" && pwd) || exit 1
cd /tmp && export TMPDIR=/tmp
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d $OUT/prof_bf16v5 -o p -- python3 $R/bench.py --full --steps 5 --warmup 2 --no-cpu-baseline --no-secondary --wm-steps 0 --precision bf16 > $OUT/prof_bf16v5.log 2>&1 || { tail -20 $OUT/prof_bf16v5.log; exit 1; }
cd $R && python tools/prof_summary.py $OUT/prof_bf16v5/p_results.db 12
