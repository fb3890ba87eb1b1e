"""Decode-attention sweep (k_attn_decode, the rollout's KV-cache attention + fused out-projection):
KV length t x live rows R at the C3 model (dh 16, H 4, d 256), where the cache read dominates.

    python tools/attn_sweep.py run [--reps 10] [--out gpurun_out/attn_sweep.json]
    python tools/attn_sweep.py summarize gpurun_out/attn_sweep.json <kernel_trace dir> [<pmc FETCH dir> <pmc WRITE dir>]

``run`` builds a C3 learner with Tmax 512, rolls out once (weights packed, caches filled), then for
every (t, R) point makes the first R slots live (alive = 1, the rest dead) and runs the multi-kernel
decode step at position t ``warm + reps`` times; HIP events around every attention launch of the
timed reps (XtrlDecodeDesc.prof_events) give the event time.  Algorithmic bytes per launch as
bench.py's DecodeAttnTimer: per live (row, head) the K and V rows 0..t-1 (2 t dh fp32) + the row's
q|k|v|gate|mix operands + the value-residual row + the K/V append + the output.  ``run --window W`` sets
XtrlDecodeDesc.attn_window (world_model['attn_max_attend_past']): the step reads the last min(t, W)
cached keys only, and the bytes count those.  ``run --kv-heads Hkv`` builds the C3 learner with
agent_kwargs kv_heads = Hkv: the cache rows, the k | v | mix operands and the value-residual row
are counted per kv head, q | gate and the output per query head.
``summarize`` assigns the k_attn_decode dispatches of a rocprofv3 --kernel-trace (and optional
--pmc FETCH_SIZE / WRITE_SIZE) run of ``run`` to the points in launch order (the points are run
in a fixed order, (warm + reps) x L dispatches each) and reports the profiler's duration and the
counters' HBM bytes per launch (reads = 2 x FETCH_SIZE, the gfx950 correction of the MI355X guide).
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / 'x-transformers-rl_amd')]

TS = (64, 128, 256, 500)
RS = (256, 1024)
WARM = 2
HBM = 8000.0


def points():
    return [(t, r) for r in RS for t in TS]


def algo_bytes(c, t, R, window=0):
    H, dh = c.heads, c.dim_head
    Hkv = getattr(c, 'kv_heads', 0) or H   # grouped-query attention: the cache rows, k, v, mix and v1 are per kv head
    if window:
        t = min(t, window)   # cached keys max(0, t - W) .. t - 1
    kv_row = 2 * dh + (1 if c.learned_mix else 0)           # the row's k | v | mix operands
    q_row = dh + (dh if c.gate_values else 0)               # q | gate
    vres = dh if c.value_residual else 0
    return 4.0 * R * (Hkv * (2 * t * dh + kv_row + vres + 2 * dh) + H * (q_row + dh))


def build_c3(cfg, kv_heads):
    """bench.build_learner's C3 learner; ``kv_heads`` > 0: the same with agent_kwargs kv_heads."""
    import bench
    if not kv_heads:
        return bench.build_learner(cfg, 0, use_graph=False)
    from xtrl_amd import Learner, SynthVecSim
    wm = dict(attn_dim_head=cfg['dim_head'], heads=cfg['heads'], depth=cfg['depth'], attn_gate_values=True,
              add_value_residual=True, learned_value_residual_mix=True)
    learner = Learner(state_dim=cfg['S'], num_actions=cfg['A'], reward_range=(-5., 5.), world_model=wm,
                      max_timesteps=cfg['T'], batch_size=cfg['batch'], num_episodes_per_update=cfg['episodes'],
                      evolutionary=cfg['evo'], evolve_every=5, evolve_after_step=10,
                      latent_gene_pool=dict(dim=32, num_genes_per_island=3, num_selected=2, tournament_size=2),
                      agent_kwargs=dict(hidden_dim=cfg['dim'], dropout=cfg['dropout'], seed=0, kv_heads=kv_heads,
                                        save_path=os.path.join(tempfile.gettempdir(), 'xtrl_attn_sweep_ppo.pt')),
                      use_graph=False)
    return learner, SynthVecSim(cfg['S'], cfg['A'], cfg['mode'], cfg['hazard_log2'])


def run(a):
    import torch
    import bench
    cfg = dict(bench.CONFIGS['c3'], T=512)
    torch.manual_seed(0)
    learner, env = build_c3(cfg, a.kv_heads)
    learner.rollout_device(env, 0, 512)      # packs the weights, fills the caches
    torch.cuda.synchronize()
    eng = learner._engine_for(env, 512)
    c = eng.c
    L = c.depth
    eng.desc.attn_window = a.window
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * 512 * L)]
    for e in ev:
        e.record()
    torch.cuda.synchronize()
    arr = (C.c_void_p * len(ev))(*[e.cuda_event for e in ev])
    out = []
    for (t, R) in points():
        ms = 0.0
        for rep in range(WARM + a.reps):
            eng.alive.zero_()
            eng.alive[:R] = 1
            eng.lens.fill_(t)
            eng.desc.prof_events = C.cast(arr, C.POINTER(C.c_void_p)) if rep >= WARM else None
            eng.step(t)
            if rep >= WARM:
                torch.cuda.synchronize()
                ms += sum(ev[2 * (t * L + l)].elapsed_time(ev[2 * (t * L + l) + 1]) for l in range(L))
        eng.desc.prof_events = None
        us = ms * 1e3 / (a.reps * L)
        b = algo_bytes(c, t, R, a.window)
        out.append(dict(t=t, rows=R, window=a.window, kv_heads=a.kv_heads or c.heads, us_event=round(us, 2), bytes=b, gbs_event=round(b / us / 1e3, 1),
                        frac_event=round(b / us / 1e3 / HBM, 4)))
        print(json.dumps(out[-1]), flush=True)
    json.dump(dict(points=out, reps=a.reps, warm=WARM, layers=L, window=a.window, kv_heads=a.kv_heads or c.heads),
              open(a.out, 'w'), indent=1)


def summarize(a):
    meta = json.load(open(a.json))
    L, per = meta['layers'], (meta['warm'] + meta['reps']) * meta['layers']
    skip = meta['warm'] * L

    def dispatches(root, csv_glob, key):
        rows = []
        for f in glob.glob(os.path.join(root, '**', csv_glob), recursive=True):
            for r in csv.DictReader(open(f)):
                if 'k_attn_decode' in r['Kernel_Name']:
                    rows.append(r)
        rows.sort(key=lambda r: int(r[key]))
        return rows

    tr = dispatches(a.trace, '*kernel_trace.csv', 'Start_Timestamp')
    need = per * len(meta['points'])
    # the warm-up rollout's dispatches come first: the sweep's are the last ``need``
    tr = tr[-need:]
    fetch = write = None
    if a.fetch:
        def counter(root, name):
            vals = [r for r in dispatches(root, '*counter_collection.csv', 'Dispatch_Id') if r['Counter_Name'] == name]
            return [float(r['Counter_Value']) * 1024.0 for r in vals][-need:]
        fetch, write = counter(a.fetch, 'FETCH_SIZE'), counter(a.write, 'WRITE_SIZE')
    res = []
    for i, p in enumerate(meta['points']):
        sl = slice(i * per + skip, (i + 1) * per)
        durs = [(int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in tr[sl]]
        us = sum(durs) / len(durs)
        q = dict(p, us_rocprof=round(us, 2), gbs_rocprof=round(p['bytes'] / us / 1e3, 1),
                 frac_rocprof=round(p['bytes'] / us / 1e3 / HBM, 4))
        if fetch:
            f = sum(fetch[sl]) / len(fetch[sl])
            w = sum(write[sl]) / len(write[sl])
            q.update(hbm_bytes_pmc=round(2 * f + w), gbs_pmc=round((2 * f + w) / us / 1e3, 1),
                     frac_pmc=round((2 * f + w) / us / 1e3 / HBM, 4))
        res.append(q)
        print(json.dumps(q))
    json.dump(dict(meta, points=res), open(a.json.replace('.json', '_summary.json'), 'w'), indent=1)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest='cmd', required=True)
    r = sub.add_parser('run')
    r.add_argument('--reps', type=int, default=10)
    r.add_argument('--window', type=int, default=0, help='sliding window (attn_max_attend_past); 0: none')
    r.add_argument('--kv-heads', type=int, default=0,
                   help='grouped-query attention (agent_kwargs kv_heads); 0: multi-head, bench.py\'s C3 learner')
    r.add_argument('--out', default=str(REPO / 'gpurun_out' / 'attn_sweep.json'))
    s = sub.add_parser('summarize')
    s.add_argument('json')
    s.add_argument('trace')
    s.add_argument('fetch', nargs='?')
    s.add_argument('write', nargs='?')
    a = ap.parse_args()
    run(a) if a.cmd == 'run' else summarize(a)
