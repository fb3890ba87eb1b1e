"""Learn-step attention with grouped-query attention: forward and backward of the xtrl_attn_*_gqa
entry points at the minibatch geometry of C3 (128 episodes x 4 heads x 128 steps) and C2 (32 x 4 x 500),
dim_head 16, dropout 0.25, ragged episode lengths, for Hkv in {H, 2, 1}.

    python tools/gqa_attn_bench.py [--out profiles/attn_gqa_kernels.json]

The Hkv values alternate inside every round (H, 2, 1, H, 2, 1, ...) so that drift hits all alike; per
point the median of ``--rounds`` timed launches-plus-synchronise after ``--warm`` warm-ups.  Backward
modes: 'pair' (dK/dV + dQ kernels), 'part' (dQ folded into the dK/dV kernel over a partial workspace) and,
at n <= 128, 'fused' — which exists for Hkv = H only: at Hkv < H that dispatch runs the pair, and the
figure says what the missing fused form costs.  Also recorded: the K + V bytes of the minibatch (what
shrinks by H / Hkv)."""
import argparse
import json
import os
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(REPO), str(REPO / 'x-transformers-rl_amd')]

GEOMETRY = dict(c3=(128, 4, 128, 16), c2=(32, 4, 500, 16))


def main():
    import torch
    from xtrl_amd import _lib as L
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=20)
    ap.add_argument('--warm', type=int, default=3)
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'attn_gqa_kernels.json'))
    a = ap.parse_args()
    lib = L.lib()
    res = []
    for name, (b, H, n, dh) in GEOMETRY.items():
        g = torch.Generator().manual_seed(0)
        lens = torch.randint(1, n + 1, (b,), generator=g).to(torch.int32)
        lens[0] = n
        lens = lens.cuda()
        q, k, v, do = (torch.randn(b, H, n, dh, generator=g).cuda() for _ in range(4))
        o, dq = torch.empty_like(q), torch.empty_like(q)
        lse, delta = (torch.empty(b, H, n, device='cuda') for _ in range(2))
        nf = int(lib.xtrl_attn_bwd_part_floats(b, H, n, dh))
        part = torch.empty(nf, device='cuda')
        kvs = {Hkv: (k[:, :Hkv].contiguous(), v[:, :Hkv].contiguous(), torch.empty(b, Hkv, n, dh, device='cuda'),
                     torch.empty(b, Hkv, n, dh, device='cuda')) for Hkv in (H, 2, 1)}
        common = (dh ** -0.5, 0.25, 1, 0, 0, 0)   # scale, p, seed, offset, sub, window

        def fwd(Hkv):
            kk, vv, _, _ = kvs[Hkv]
            L.check(lib.xtrl_attn_fwd_gqa(L.ptr(q), L.ptr(kk), L.ptr(vv), L.ptr(lens), L.ptr(o), L.ptr(lse), b, H, Hkv, n,
                                          dh, *common, L.stream()), 'fwd')

        def bwd(Hkv, mode):
            kk, vv, dk, dv = kvs[Hkv]
            os.environ['XTRL_ATTN_FUSED_BWD'] = '0' if mode == 'pair' else '1'
            if mode == 'part':
                L.check(lib.xtrl_attn_bwd_part_gqa(L.ptr(q), L.ptr(kk), L.ptr(vv), L.ptr(lens), L.ptr(o), L.ptr(lse),
                                                   L.ptr(do), L.ptr(dq), L.ptr(dk), L.ptr(dv), L.ptr(delta), L.ptr(part),
                                                   nf, b, H, Hkv, n, dh, *common, L.stream()), 'bwd_part')
            else:
                L.check(lib.xtrl_attn_bwd_gqa(L.ptr(q), L.ptr(kk), L.ptr(vv), L.ptr(lens), L.ptr(o), L.ptr(lse), L.ptr(do),
                                              L.ptr(dq), L.ptr(dk), L.ptr(dv), L.ptr(delta), b, H, Hkv, n, dh, *common,
                                              L.stream()), 'bwd')

        def timed(fn):
            torch.cuda.synchronize()
            s, e = torch.cuda.Event(True), torch.cuda.Event(True)
            s.record()
            fn()
            e.record()
            torch.cuda.synchronize()
            return s.elapsed_time(e) * 1e3

        modes = ['pair', 'part'] + (['fused'] if n <= 128 else [])
        cases = [('fwd', None)] + [('bwd', m) for m in modes]
        times = {(Hkv, c): [] for Hkv in kvs for c in cases}
        for r in range(a.warm + a.rounds):
            for c in cases:
                for Hkv in kvs:   # alternating
                    fwd(Hkv)      # (the backward reads this Hkv's o and lse)
                    us = timed((lambda: fwd(Hkv)) if c[0] == 'fwd' else (lambda: bwd(Hkv, c[1])))
                    if r >= a.warm:
                        times[(Hkv, c)].append(us)
        os.environ.pop('XTRL_ATTN_FUSED_BWD', None)
        for Hkv in kvs:
            row = dict(geometry=name, b=b, H=H, Hkv=Hkv, n=n, dh=dh, kv_bytes=2 * 4 * b * Hkv * n * dh)
            for c in cases:
                ts = times[(Hkv, c)]
                key = 'fwd_us' if c[0] == 'fwd' else f'bwd_{c[1]}_us'
                row[key] = round(statistics.median(ts), 1)
                row[key + '_minmax'] = [round(min(ts), 1), round(max(ts), 1)]
            res.append(row)
            print(json.dumps(row), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    json.dump(dict(rounds=a.rounds, warm=a.warm, dropout=0.25, points=res), open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
