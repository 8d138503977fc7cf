#!/bin/bash
# quick GPU iteration: parity tests + default bench (+ optional extra bench args)
TAG=${1:-q}; shift
ROOT=${GRAFT_REPO_ROOT:-/root/repo}; cd "$ROOT"; OUT="$ROOT/gpurun_out/$TAG"; mkdir -p "$OUT"
python -c "from oracle.oracle import build; build()" > "$OUT/oracle_build.log" 2>&1
timeout 900 python -m pytest tests -m gpu -q > "$OUT/pytest_gpu.log" 2>&1; tail -4 "$OUT/pytest_gpu.log"; grep -E "^E  .*mismatch|Error" "$OUT/pytest_gpu.log" | head -10
timeout 600 python bench.py --full --no-cpu-baseline "$@" > "$OUT/bench.json" 2> "$OUT/bench.err"; tail -2 "$OUT/bench.err"
python - <<PY
import json
d=json.load(open("$OUT/bench.json"))
print("value", d["value"], "ms/step", d["ms_per_step"])
print({k:v["ms_per_step"] for k,v in d["kernels"].items()})
print(d["roofline"])
PY
