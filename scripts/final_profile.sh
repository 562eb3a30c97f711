#!/bin/bash
# Round-end evidence on one MI355X (repo root on the GPU box): GPU parity of the
# batched variants, the full bench line, then rocprofv3 --kernel-trace --stats
# of the plain bench (timed steps only).
# Usage: bash scripts/final_profile.sh [out-dir]
set -euo pipefail
export TMPDIR=/tmp
O=${1:-bench_out/final}
mkdir -p "$O"
timeout -k 10 500 python3 -u -m pytest tests/test_gpu_batch_variants.py tests/test_gpu_parity.py -x -q --timeout 200 --timeout-method thread > "$O/parity.log" 2>&1
timeout -k 10 600 python3 bench.py --full > "$O/bench.json" 2> "$O/bench.err"
timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d "$O/kt" -o run -- \
  python3 bench.py --steps 2 --warmup 1 > "$O/kt.log" 2>&1
