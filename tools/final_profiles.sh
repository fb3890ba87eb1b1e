#!/bin/bash
# Round-end measurement of one bench config on the GPU box: rocprofv3 kernel stats and the PMC
# passes (tools/gpu_check.sh), their summaries installed as profiles/rNN_*[_cfg] so the bench line
# quotes them, then the bench itself (bench.py --full: rooflines, loss delta, CPU baseline).
# Everything kept lands in $XTRL_OUT/final/ (default: out/final/ in the repository root; copied
# into profiles/ by hand afterwards).
# Usage: tools/final_profiles.sh <round tag, e.g. r03> <config: c3 | c2 | c5>
set -u
R=$(cd "$(dirname "$0")/.." && pwd)
export XTRL_OUT=${XTRL_OUT:-$R/out}
case $XTRL_OUT in /*) ;; *) XTRL_OUT=$PWD/$XTRL_OUT ;; esac
OUT=$XTRL_OUT
cd $R
tag=$1; cfg=$2
S=""; [ "$cfg" != "c3" ] && S="_$cfg"
mkdir -p $OUT/final
bash tools/gpu_check.sh prof --config $cfg || exit $?
cp $OUT/prof$S/run_kernel_stats.csv profiles/${tag}_kernel_stats$S.csv
cp $OUT/prof$S/run_kernel_stats.csv $OUT/final/${tag}_kernel_stats$S.csv
bash tools/gpu_check.sh pmc --config $cfg || exit $?
python3 tools/pmc_summary.py $OUT/pmc$S > profiles/${tag}_pmc_traffic$S.json
cp profiles/${tag}_pmc_traffic$S.json $OUT/final/
timeout -k 10 900 python bench.py --full --config $cfg > $OUT/final/bench$S.log 2>&1
rc=$?
tail -n 1 $OUT/final/bench$S.log > $OUT/final/${tag}_bench$S.json
exit $rc
