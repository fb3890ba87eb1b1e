#!/bin/bash
# Round-end lines of the extra bench configs (no PMC passes): rocprofv3 kernel stats of a short run,
# then the bench itself with its CPU baseline (bench.py --full).  Everything lands under $XTRL_OUT
# (default: out/ in the repository root).  Usage: tools/final_extra.sh <round tag> <config>...
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
export XTRL_OUT=${XTRL_OUT:-$R/out}
case $XTRL_OUT in /*) ;; *) XTRL_OUT=$PWD/$XTRL_OUT ;; esac
OUT=$XTRL_OUT
cd $R
tag=$1; shift
mkdir -p $OUT/final
for cfg in "$@"; do
  bash tools/gpu_check.sh prof --config $cfg > $OUT/final/prof_$cfg.txt 2>&1 || { echo "prof $cfg failed"; exit 1; }
  cp $OUT/prof_$cfg/run_kernel_stats.csv $OUT/final/${tag}_kernel_stats_$cfg.csv
  timeout -k 10 900 python bench.py --full --config $cfg > $OUT/final/bench_$cfg.log 2>&1 || { echo "bench $cfg failed"; tail -5 $OUT/final/bench_$cfg.log; exit 1; }
  tail -n 1 $OUT/final/bench_$cfg.log > $OUT/final/${tag}_bench_$cfg.json
  echo "$cfg done"
done
