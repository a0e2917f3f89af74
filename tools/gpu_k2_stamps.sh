#!/bin/bash
# K2 phase stamps on C4 and the C5 reference legs: the -DG2N_K2_STAMPS variant (tools/exp_build.sh stamps
# "-DG2N_K2_STAMPS"); k2_stamps.json and the log under $G2N_OUT (default bench_out/ in the repository)
set -o pipefail
R=${G2N_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}; OUT=${G2N_OUT:-$R/bench_out}
cd $R && mkdir -p $OUT
G2N_LIB=$R/gfa2network_amd/_lib/exp_${1:-stamps}.so G2N_K2_STAMPS_OUT=$OUT/k2_stamps.bin \
  timeout -k 10 300 python -u bench.py --full --steps 1 --warmup 1 --no-e2e --no-cpu-baseline --no-alt > $OUT/k2_stamps.log 2>&1 || { tail -20 $OUT/k2_stamps.log; exit 1; }
python tools/k2_stamps.py $OUT/k2_stamps.bin $OUT/k2_stamps.json
rm -f $OUT/k2_stamps.bin
