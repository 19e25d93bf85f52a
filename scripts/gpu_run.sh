#!/bin/bash
# One GPU session on the box: smoke -> GPU parity tests -> short bench (-> optional profile).
# Every GPU step has its own time limit; a crash / abort / timeout stops the script (a plain test
# failure, exit 1, does not). Logs and results go to $OUT_DIR (default out/).
set -u
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
OUT="${OUT_DIR:-out}"
mkdir -p "$OUT"
STAGES="${STAGES:-smoke tests bench}"
ok_or_stop() {  # $1 = exit code, $2 = step name
  local rc=$1
  echo "== $2 exit $rc" | tee -a "$OUT/status.log"
  if [ "$rc" -ne 0 ] && [ "$rc" -ne 1 ]; then echo "stopping after $2 (rc=$rc)"; exit "$rc"; fi
}
for s in $STAGES; do
  case "$s" in
    smoke)
      timeout -k 10 600 python -c "import __graft_entry__ as g; g.smoke()" > "$OUT/smoke.log" 2>&1
      ok_or_stop $? smoke ;;
    tests)
      PICO_LOSS_OUT="$OUT/loss_curve_gpu.json" timeout -k 10 1200 python -u -m pytest tests -q -m gpu --timeout 400 --timeout-method thread ${PYTEST_ARGS:-} ${PYTEST_K:+-k "$PYTEST_K"} > "$OUT/pytest_gpu.log" 2>&1
      ok_or_stop $? pytest ;;
    bench)
      # the whole record (kernels table, roofline, CPU baseline), not only the headline figure
      timeout -k 10 900 python bench.py --full ${BENCH_ARGS:-} > "$OUT/bench.json" 2> "$OUT/bench.log"
      ok_or_stop $? bench ;;
    attn)
      timeout -k 10 300 python scripts/attn_bench.py --configs ${ATTN_CONFIGS:-c2,c2_full,d128,gqa4} > "$OUT/attn_bench.jsonl" 2> "$OUT/attn_bench.log"
      ok_or_stop $? attn ;;
    gemm)
      timeout -k 10 300 python scripts/gemm_bench.py > "$OUT/gemm_default.jsonl" 2>&1
      ok_or_stop $? gemm_default
      PYTORCH_TUNABLEOP_ENABLED=1 PYTORCH_TUNABLEOP_FILENAME="$OUT/tunableop_results.csv" timeout -k 10 900 python scripts/gemm_bench.py > "$OUT/gemm_tunable.jsonl" 2>&1
      ok_or_stop $? gemm_tunable ;;
    prof)
      export TMPDIR=/tmp
      # a plain run: the trace holds the warm-up and the timed steps only
      timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d "$OUT/prof" -o run -- python3 bench.py --steps 2 --warmup 1 ${BENCH_ARGS:-} > "$OUT/prof.log" 2>&1
      ok_or_stop $? prof ;;
  esac
done
echo "== done" | tee -a "$OUT/status.log"
