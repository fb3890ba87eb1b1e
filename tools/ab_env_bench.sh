#!/bin/bash
# A/B of environment switches on one box: bench.py (C3 with its roofline pass, no CPU baseline / loss
# check) per setting, one JSON line each into $XTRL_OUT/ab_<tag>.log (default: out/ under the current
# directory).  Usage: tools/ab_env_bench.sh "tag:VAR=v VAR2=w" ...
OUT=${XTRL_OUT:-out}
mkdir -p $OUT
for spec in "$@"; do
  tag=${spec%%:*}; envs=${spec#*:}
  env $envs timeout -k 10 300 python bench.py --full --steps 8 --warmup 2 --no-cpu-baseline --no-loss-delta > $OUT/ab_$tag.log 2>&1
  rc=$?
  python3 -c "import json;d=json.loads(open('$OUT/ab_$tag.log').read().strip().splitlines()[-1]);print('$tag', d['value'], d['phase_ms'], d['roofline']['frac'] if d.get('roofline') else None)" || echo "$tag failed rc=$rc"
  if [ $rc -ne 0 ]; then exit $rc; fi
done
