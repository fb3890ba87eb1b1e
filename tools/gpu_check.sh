#!/bin/bash
# One GPU session: parity tests, then (only if they did not crash the process) bench + profile.
# Usage: tools/gpu_check.sh [tests|bench|prof|pmc|trace|all] [bench args...]
# Everything written lands under $XTRL_OUT (default: out/ in the repository root).
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
OUT=${XTRL_OUT:-$R/out}
case $OUT in /*) ;; *) OUT=$PWD/$OUT ;; esac
cd $R
mkdir -p $OUT
what=${1:-all}; shift || true
run_tests() {
  timeout -k 10 900 python -u -m pytest tests -m gpu -q -x --timeout=300 --timeout-method thread -p no:cacheprovider > $OUT/gpu_tests.log 2>&1
  rc=$?; tail -15 $OUT/gpu_tests.log
  if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "pytest rc=$rc: stopping"; exit $rc; fi
}
run_bench() {
  # the whole line: rooflines, PPO loss delta and CPU baselines (bench.py --full)
  timeout -k 10 900 python bench.py --full "$@" > $OUT/bench.log 2>&1
  rc=$?; tail -5 $OUT/bench.log
  if [ $rc -ne 0 ]; then echo "bench rc=$rc: stopping"; exit $rc; fi
}
# output suffix of a non-default bench config (--config c5 -> _c5), matching bench.py _profile()
sfx() {
  local prev=""
  for a in "$@"; do
    if [ "$prev" = "--config" ] && [ "$a" != "c3" ]; then echo "_$a"; return; fi
    prev=$a
  done
}
run_prof() {
  local S=$(sfx "$@")
  cd /tmp && export TMPDIR=/tmp
  timeout -k 10 900 rocprofv3 --kernel-trace --stats -d $OUT/prof$S -o run --output-format csv -- python3 $R/bench.py --full --steps 2 --warmup 1 --no-cpu-baseline "$@" > $OUT/prof$S.log 2>&1
  rc=$?; cd $R; tail -3 $OUT/prof$S.log
  find $OUT/prof$S -type f ! -name '*stats*' -delete
  if [ $rc -ne 0 ]; then echo "prof rc=$rc"; exit $rc; fi
}
run_pmc() {
  # HBM traffic counters, one counter group per pass (FETCH_SIZE and WRITE_SIZE do not fit together)
  local S=$(sfx "$@")
  cd /tmp && export TMPDIR=/tmp
  # one counter group per pass: HBM read bytes, HBM write bytes, MFMA busy cycles + GPU clock
  for c in FETCH_SIZE WRITE_SIZE "SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE"; do
    name=$(echo $c | cut -d' ' -f1)
    # only the two roofline kernels (many more dispatches crash the counter-collection tool)
    timeout -k 10 900 rocprofv3 --pmc $c --kernel-include-regex "k_attn_decode|k_gemm<2, 2, 1, 2, 2, true, true|k_gemm_ws<true, true" -d $OUT/pmc$S/pmc_$name -o run --output-format csv -- python3 $R/bench.py --full --steps 1 --warmup 0 --no-cpu-baseline --no-loss-delta "$@" > $OUT/pmc${S}_$name.log 2>&1
    rc=$?; tail -2 $OUT/pmc${S}_$name.log
    if [ $rc -ne 0 ]; then echo "pmc $c rc=$rc"; exit $rc; fi
  done
  cd $R && python3 tools/pmc_summary.py $OUT/pmc$S > $OUT/pmc_summary$S.txt; cat $OUT/pmc_summary$S.txt
}
run_trace() {
  # kernel trace of one update (tools/update_trace.py): per-phase totals, one minibatch, one decode step
  local cfg=${1:-c3}
  local S=$(sfx --config $cfg)
  cd /tmp && export TMPDIR=/tmp
  timeout -k 10 600 rocprofv3 --kernel-trace -d $OUT/trace$S -o run --output-format csv -- python3 $R/tools/update_trace.py run $cfg > $OUT/trace$S.log 2>&1
  rc=$?; cd $R; tail -3 $OUT/trace$S.log
  if [ $rc -ne 0 ]; then echo "trace rc=$rc"; exit $rc; fi
  python3 tools/update_trace.py show $(find $OUT/trace$S -name '*kernel_trace.csv' | head -1) > $OUT/trace_summary$S.txt
  find $OUT/trace$S -type f -name '*kernel_trace.csv' -delete
  head -80 $OUT/trace_summary$S.txt
}
case $what in
  trace) run_trace "$@" ;;
  pmc) run_pmc "$@" ;;
  tests) run_tests ;;
  bench) run_bench "$@" ;;
  prof) run_prof "$@" ;;
  all) run_tests; run_bench "$@"; run_prof "$@" ;;
esac
