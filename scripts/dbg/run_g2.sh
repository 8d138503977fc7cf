python -c "from oracle.oracle import build; build()" >/dev/null 2>&1
timeout 300 python -m pytest tests/test_bench_ranks.py -m gpu -q -x 2>&1 | tail -5
OUT=${OUT:-$(mktemp -d)}; (time timeout 300 python bench.py --full --no-secondary > "$OUT/bench_ns.json" 2> "$OUT/bench_ns.err"); tail -3 "$OUT/bench_ns.err"
python - <<PY
import json
d=json.load(open("$OUT/bench_ns.json"))
print(d["value"], d["ms_per_step"])
print(d["cpu_baseline"])
PY
