"""Per-launch table of the 64 x 256 LayerNorm-epilogue GEMMs (and the weight-image builds) in the last update
of a `rocprofv3 --kernel-trace` CSV of tools/update_trace.py: launches, total ms and the duration clusters
behind each instantiation (one instantiation serves several K; clusters split at gaps of more than 35 %).

  python tools/ln_gemm_table.py TRACE_kernel_trace.csv
"""
import csv
import sys
from collections import defaultdict


def main(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    names = [r['Kernel_Name'] for r in rows]
    # the measured update starts at its rollout (as tools/update_trace.py)
    start = [i for i, n in enumerate(names) if 'k_rollout_begin' in n or 'k_sim_reset' in n][-1]
    agg = defaultdict(list)
    for r in rows[start:]:
        n = r['Kernel_Name'].replace('xtrl::(anonymous namespace)::', '').replace('void ', '').split('(')[0]
        if ('k_gemm_ws' in n and '64, 256' in n) or 'k_wfrag_build' in n or 'k_wimg_build' in n:
            grid = 'x'.join(r.get(f'Grid_Size_{a}', '?') for a in 'XYZ')
            agg[(n, grid)].append((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3)
    tot = 0.0
    for (n, grid), d in sorted(agg.items()):
        d.sort()
        cl = [[d[0]]]
        for x in d[1:]:
            if x > 1.35 * cl[-1][-1]:
                cl.append([])
            cl[-1].append(x)
        print(f'{n} [{grid}]: {len(d)} launches, {sum(d) / 1e3:.2f} ms')
        tot += sum(d)
        for c in cl:
            print(f'    {len(c):5d} x  mean {sum(c) / len(c):7.1f} us  min {c[0]:7.1f}  median {c[len(c) // 2]:7.1f}  '
                  f'max {c[-1]:7.1f}')
    print(f'total {tot / 1e3:.2f} ms')


if __name__ == '__main__':
    main(sys.argv[1])
