#!/bin/bash
# GPU-box: parity tests -> full bench (cpu baseline + pcie) -> rocprof stats -> PMC traffic passes.
# usage: [OUT_DIR=dir] tools/round_gpu.sh TAG COMMIT [--no-pmc]   (the box has no .git: COMMIT stamps traffic.json)
# logs and results go under $OUT_DIR (default bench_out/)
set -o pipefail
TAG=$1; COMMIT=$2; shift 2
cd "$(dirname "$0")/.."
OUT=${OUT_DIR:-bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 300 python -u -m pytest tests -m gpu -x -v --timeout 120 --timeout-method thread > "$OUT/tests_$TAG.log" 2>&1 || { echo "tests failed"; tail -30 "$OUT/tests_$TAG.log"; exit 1; }
tail -2 "$OUT/tests_$TAG.log"
timeout -k 10 540 python3 bench.py --full > "$OUT/bench_$TAG.json" 2> "$OUT/bench_$TAG.err" || { echo "bench failed"; tail -20 "$OUT/bench_$TAG.err"; exit 1; }
cat "$OUT/bench_$TAG.json"
# the headline workload alone (the extras' kernels would mix into the per-kernel averages)
timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof_$TAG" -o run -f csv -- python3 bench.py --full --steps 10 --warmup 3 --no-cpu-baseline --no-extras --no-pcie > "$OUT/benchprof_$TAG.json" 2> "$OUT/benchprof_$TAG.err" || { echo "rocprof failed"; exit 1; }
for cfg in M C; do
  timeout -k 10 300 rocprofv3 --kernel-trace --stats -d "$OUT/prof_${TAG}_$cfg" -o run -f csv -- python3 bench.py --full --config $cfg --steps 5 --warmup 2 --no-cpu-baseline --no-pcie > "$OUT/benchprof_${TAG}_$cfg.json" 2> "$OUT/benchprof_${TAG}_$cfg.err" || { echo "rocprof $cfg failed"; exit 1; }
done
head -6 "$OUT/prof_$TAG/run_kernel_stats.csv" | cut -d, -f1-4
if [ "$1" != "--no-pmc" ]; then
  bash tools/traffic.sh "$OUT/traffic_$TAG.json" "$COMMIT" U Z M C || exit 1
  cat "$OUT/traffic_$TAG.json"
fi
