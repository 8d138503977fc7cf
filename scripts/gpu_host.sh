#!/bin/bash
# host-side cost of issuing a step vs the GPU step time
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd "$ROOT"; OUT=${OUT:-$(mktemp -d)}
for i in 1 2; do
python bench.py --full --no-cpu-baseline --profile-steps 0 --steps 24 --warmup 8 > "$OUT/b$i.json" 2>/dev/null
python - <<PY
import json
d=json.load(open("$OUT/b$i.json")); print("steps 24: ms/step", d["ms_per_step"], "host enqueue ms/step", d["host_enqueue_ms_per_step"], "value", d["value"])
PY
done
