#!/bin/bash
# L2 traffic of the warp-specialised GEMMs in one C3 update, register-staged B against image-fed B
# (XTRL_WIMG=1): FETCH_SIZE and WRITE_SIZE, one counters-only pass each (no tracing in these runs),
# summarised per kernel into <out dir>/wimg_pmc.txt.  Usage: tools/wimg_pmc.sh [out dir, default $XTRL_OUT or out/]
R=$(cd "$(dirname "$0")/.." && pwd)
O=${1:-${XTRL_OUT:-$R/out}}
O=$(mkdir -p "$O" && cd "$O" && pwd)
cd /tmp && export TMPDIR=/tmp
for arm in 0 1; do
  for ctr in FETCH_SIZE WRITE_SIZE; do
    d=/tmp/wimg_pmc_${arm}_$ctr
    rm -rf $d
    XTRL_WIMG=$arm timeout -k 10 300 rocprofv3 --pmc $ctr --kernel-include-regex "k_gemm_ws|k_wimg_build" -d $d -o run \
      --output-format csv -- python3 $R/tools/update_trace.py run c3 > $O/wimg_pmc_${arm}_$ctr.log 2>&1
    rc=$?
    echo "XTRL_WIMG=$arm $ctr rc=$rc"
    if [ $rc -ne 0 ]; then exit $rc; fi
  done
done
python3 - > $O/wimg_pmc.txt <<'PY'
import csv, glob
from collections import defaultdict
for arm in (0, 1):
    agg = defaultdict(lambda: defaultdict(lambda: [0, 0.0]))
    for ctr in ('FETCH_SIZE', 'WRITE_SIZE'):
        for f in glob.glob(f'/tmp/wimg_pmc_{arm}_{ctr}/**/*counter_collection.csv', recursive=True):
            for r in csv.DictReader(open(f)):
                if r.get('Counter_Name') != ctr:
                    continue
                name = r['Kernel_Name'].replace('xtrl::(anonymous namespace)::', '').replace('void ', '').split('(')[0]
                a = agg[name][ctr]
                a[0] += 1
                a[1] += float(r['Counter_Value'])
    print(f'XTRL_WIMG={arm}: per launch, KB (FETCH_SIZE and WRITE_SIZE count kilobytes)')
    for name, c in sorted(agg.items()):
        f, w = c['FETCH_SIZE'], c['WRITE_SIZE']
        print(f'  {name}: launches {f[0]}, fetch {f[1] / max(f[0], 1):.0f}, write {w[1] / max(w[0], 1):.0f}')
PY
rm -rf /tmp/wimg_pmc_*
cat $O/wimg_pmc.txt
