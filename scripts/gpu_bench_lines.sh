#!/bin/bash
# the secondary bench lines of the round (committed under profiles/), with every leg (--full) -> $OUT/bench_*.json
cd "$(dirname "$0")/.."
OUT="${OUT:-results}"
mkdir -p "$OUT"
export PYTHONUNBUFFERED=1
timeout 900 python bench.py --full --workload bev 2>/dev/null | grep '^{' | tail -1 > "$OUT/bench_bev.json"; cut -c1-400 "$OUT/bench_bev.json"
timeout 300 python bench.py --full --workload smpl --steps 50 2>/dev/null | grep '^{' | tail -1 > "$OUT/bench_smpl.json"; cut -c1-400 "$OUT/bench_smpl.json"
timeout 900 python bench.py --full --backbone resnet50 --no-f32-companion --no-latency 2>/dev/null | grep '^{' | tail -1 > "$OUT/bench_resnet50.json"; cut -c1-300 "$OUT/bench_resnet50.json"
timeout 900 python bench.py --full --batch 128 --no-f32-companion --no-latency --no-cpu-baseline 2>/dev/null | grep '^{' | tail -1 > "$OUT/bench_b128.json"; cut -c1-300 "$OUT/bench_b128.json"
