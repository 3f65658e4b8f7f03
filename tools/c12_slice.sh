#!/bin/bash
# configs[4]'s per-GPU slice on one GPU: 3 key ranges x 1 Mi blocks (12.7 GB of L0 input), every
# output block oracle-checked range by range; the line reports peak host RSS and wall time
# usage: [OUT_DIR=dir] tools/c12_slice.sh   (line and log under $OUT_DIR, default bench_out/)
set -o pipefail
cd "$(dirname "$0")/.."
OUT=${OUT_DIR:-bench_out}
mkdir -p "$OUT"
export TMPDIR=/tmp
timeout -k 10 500 python3 -u bench.py --full --config C --blocks 3145728 --ranges-per-gpu 3 --steps 3 --warmup 1 --no-cpu-baseline --no-pcie > "$OUT/C12g_bench.json" 2> "$OUT/C12g_bench.log"
rc=$?; tail -5 "$OUT/C12g_bench.log"; exit $rc
