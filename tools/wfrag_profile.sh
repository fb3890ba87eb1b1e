#!/bin/bash
# Fragment-order weight images against a worktree of the parent commit (its own Python + in-tree library,
# as tools/ab_tree.sh): for each tree one kernel trace of a C3 update (tools/update_trace.py summary and the
# per-launch table of the 64 x 256 LayerNorm-epilogue GEMMs, tools/ln_gemm_table.py), then, in runs of their
# own with no tracing, FETCH_SIZE and WRITE_SIZE of those kernels.
# Usage: tools/wfrag_profile.sh <base dir> [out dir, default $XTRL_OUT or out/]
set -u -o pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
base=$(cd "$1" && pwd)
O=${2:-${XTRL_OUT:-$R/out}}
O=$(mkdir -p "$O" && cd "$O" && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
cd "$T" && export TMPDIR=$T
for arm in base new; do
  if [ $arm = base ]; then dir=$base; else dir=$R; fi
  timeout -k 10 300 rocprofv3 --kernel-trace -d $T/tr_$arm -o run --output-format csv -- \
    python3 $dir/tools/update_trace.py run c3 > $O/wfrag_trace_$arm.log 2>&1 || { echo "trace $arm failed"; exit 1; }
  f=$(find $T/tr_$arm -name '*kernel_trace.csv' | head -1)
  python3 $R/tools/update_trace.py show $f > $O/wfrag_update_trace_$arm.txt 2>&1 || exit 1
  python3 $R/tools/ln_gemm_table.py $f > $O/wfrag_ln_table_$arm.txt 2>&1 || exit 1
  echo "== $arm"; cat $O/wfrag_ln_table_$arm.txt
done
for arm in base new; do
  if [ $arm = base ]; then dir=$base; else dir=$R; fi
  for ctr in FETCH_SIZE WRITE_SIZE; do
    timeout -k 10 300 rocprofv3 --pmc $ctr --kernel-include-regex "k_gemm_ws|k_wfrag_build" -d $T/pmc_${arm}_$ctr -o run \
      --output-format csv -- python3 $dir/tools/update_trace.py run c3 > $O/wfrag_pmc_${arm}_$ctr.log 2>&1 \
      || { echo "pmc $arm $ctr failed"; exit 1; }
  done
done
python3 - "$T" > $O/wfrag_pmc.txt <<'PY'
import csv, glob, sys
from collections import defaultdict
for arm in ('base', 'new'):
    agg = defaultdict(lambda: defaultdict(list))
    for ctr in ('FETCH_SIZE', 'WRITE_SIZE'):
        for f in glob.glob(f'{sys.argv[1]}/pmc_{arm}_{ctr}/**/*counter_collection.csv', recursive=True):
            for r in csv.DictReader(open(f)):
                if r.get('Counter_Name') != ctr:
                    continue
                name = r['Kernel_Name'].replace('xtrl::(anonymous namespace)::', '').replace('void ', '').split('(')[0]
                if 'k_wfrag_build' in name or '64, 256' in name:
                    agg[name][ctr].append(float(r['Counter_Value']))
    print(f'{arm}: per launch, KB (FETCH_SIZE and WRITE_SIZE count kilobytes); launches x mean, clusters split at 35 % gaps')
    for name, c in sorted(agg.items()):
        for ctr in ('FETCH_SIZE', 'WRITE_SIZE'):
            d = sorted(c[ctr])
            if not d:
                continue
            cl = [[d[0]]]
            for x in d[1:]:
                if x > 1.35 * max(cl[-1][-1], 1.0):
                    cl.append([])
                cl[-1].append(x)
            print(f'  {name} {ctr}: ' + ', '.join(f'{len(k)} x {sum(k) / len(k):.0f}' for k in cl))
PY
cat $O/wfrag_pmc.txt
