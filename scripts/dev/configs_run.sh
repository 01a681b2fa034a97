#!/bin/bash
# bench lines of the other BASELINE configs (one GPU) -> $LLMI_OUT_DIR/configs.jsonl (default: bench_out/)
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/../..}"
export OUT="${LLMI_OUT_DIR:-bench_out}"
mkdir -p "$OUT"
: > "$OUT/configs.jsonl"
for args in "--config gemma-3-1b" "--config gemma-3-1b --quant q8_0" "--quant q4_k_m" "--config gemma-3-27b --steps 64" \
            "--full-logits" "--prefill 2048" "--exact --steps 32 --warmup 4"; do
  timeout -k 10 400 python bench.py --full --no-cpu-baseline $args > "$OUT/cfg.log" 2>&1 || { echo "FAIL $args"; tail -3 "$OUT/cfg.log"; exit 1; }
  tail -1 "$OUT/cfg.log" >> "$OUT/configs.jsonl"
  python3 - "$args" <<'PY'
import json,os,sys
d=json.loads(open(os.path.join(os.environ["OUT"], "configs.jsonl")).read().strip().splitlines()[-1])
print(f"{sys.argv[1]:40s} {d['value']:8.1f} tok/s  prefill {d['timing_detail'].get('prefill_s')} s  {d['config']['workload'][:60]}", flush=True)
PY
done
