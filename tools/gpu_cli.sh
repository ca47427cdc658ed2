#!/bin/bash
# CLI parity tests + the bench's CLI legs (categorization pipeline, jf_occurrences) on the box.
# usage: bash tools/gpu_cli.sh <tag>
TAG=$1
OUT=${HGA_OUT:-bench_out}; mkdir -p $OUT   # HGA_OUT: output folder, relative to the repo root
timeout -k 10 400 python -u -m pytest -x -q --timeout 200 --timeout-method thread -m gpu tests/test_cli_gpu.py \
    tests/test_host.py > $OUT/pytest_cli_$TAG.log 2>&1 || { tail -20 $OUT/pytest_cli_$TAG.log; exit 1; }
tail -2 $OUT/pytest_cli_$TAG.log
timeout -k 10 300 python bench.py --full --no-scale > $OUT/bench_cli_$TAG.json 2> $OUT/bench_cli_$TAG.err \
    || { tail -5 $OUT/bench_cli_$TAG.err; exit 1; }
python3 - "$OUT/bench_cli_$TAG.json" <<'PY'
import json, sys
d = json.load(open(sys.argv[1]))
p = d["categorize"]["pipeline"]; t = d["categorize"].get("pipeline_tails", {})
print("categorization wall", p["wall_s"], p["phases_ms"])
print("tails wall", t.get("wall_s"))
print("jf", d["ingest"]["cli_jf_occurrences"]["wall_s"])
PY
