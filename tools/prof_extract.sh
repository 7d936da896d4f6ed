#!/bin/bash
# kernel trace of the evidence-corpus workload (both precisions and the GEMM probe step: --full)
cd "$(dirname "$0")/.." || exit 1
OUT=${OUT:-out}/prof_ext
mkdir -p $OUT
timeout -k 10 500 rocprofv3 --kernel-trace --stats -d $OUT/trace -o run --output-format csv -- \
  python3 bench.py --workload extract --steps 3 --warmup 1 --full --no-cpu-baseline > $OUT/bench.json 2> $OUT/bench.err
