#!/bin/bash
# F1 (k_sym_finish / k_sumw_finish) phase stamps: the -DG2N_F1_STAMPS variant (tools/exp_build.sh f1st
# "-DG2N_F1_STAMPS"); C4 by default, BENCH_ARGS="--workload C3 --no-c5-reference" for F1w;
# f1_stamps.json and the log under $G2N_OUT (default bench_out/ in the repository)
set -o pipefail
R=${G2N_ROOT:-$(cd "$(dirname "$0")/.." && pwd)}; OUT=${G2N_OUT:-$R/bench_out}
cd $R && mkdir -p $OUT
G2N_LIB=$R/gfa2network_amd/_lib/exp_${1:-f1st}.so G2N_F1_STAMPS_OUT=$OUT/f1_stamps.bin \
  timeout -k 10 300 python -u bench.py --full --steps 1 --warmup 1 --no-e2e --no-cpu-baseline --no-alt $BENCH_ARGS > $OUT/f1_stamps.log 2>&1 || { tail -20 $OUT/f1_stamps.log; exit 1; }
python tools/k2_stamps.py $OUT/f1_stamps.bin $OUT/f1_stamps.json f1
rm -f $OUT/f1_stamps.bin
