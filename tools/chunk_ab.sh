cd "$(dirname "$0")/.." && export PYTHONUNBUFFERED=1
OUT=${OUT_DIR:-bench_out}
mkdir -p "$OUT"
for c in 32 16 8; do
  DREAMER_WARM_CHUNK=$c timeout -k 10 200 python bench.py --full --no-cpu-baseline --no-secondary --wm-steps 0 > $OUT/chunk_$c.json 2> $OUT/chunk_$c.err || exit 1
  echo "chunk $c: $(python -c "import json;d=json.load(open('$OUT/chunk_$c.json'));print(d['value'], d['ms_per_step'])")"
done
