#!/bin/bash
# hipBLASLt workspace A/B: the GEMM micro-bench and the C2 step with the default workspace and with
# HIPBLASLT_WORKSPACE_SIZE=${WS_KIB:-262144} KiB, interleaved. Results in $OUT_DIR (default out/).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT="${OUT_DIR:-out}"
mkdir -p "$OUT"
for v in def big; do
  if [ $v = big ]; then export HIPBLASLT_WORKSPACE_SIZE=${WS_KIB:-262144}; else unset HIPBLASLT_WORKSPACE_SIZE; fi
  timeout -k 10 300 python scripts/gemm_bench.py | sed "s/^{/{\"ws\": \"$v\", /" >> "$OUT/ws_gemm.jsonl" || exit $?
done
for r in $(seq 1 ${ROUNDS:-2}); do
  for v in def big; do
    if [ $v = big ]; then export HIPBLASLT_WORKSPACE_SIZE=${WS_KIB:-262144}; else unset HIPBLASLT_WORKSPACE_SIZE; fi
    timeout -k 10 400 python bench.py --steps 5 --warmup 2 --full --no-cpu-baseline 2> "$OUT/ws_bench_$v$r.log" | sed "s/^{/{\"ws\": \"$v\", \"round\": $r, /" >> "$OUT/ws_bench.jsonl" || exit $?
  done
done
echo "== ws ab done"
