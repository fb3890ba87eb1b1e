"""Grouped-query attention at the C2 and C3 geometries: rollout and learn-step time for
agent_kwargs kv_heads = Hkv in {H, 2, 1}, device events, the learners alternating in one process.

    timeout 900 python tools/gqa_bench.py [--configs c3 c2] [--steps 4] [--warmup 2]
                                          [--out profiles/attn_gqa_bench.json]

C3 / C2 (bench.py CONFIGS, restated here): LunarLander-shaped device Sim (S 8, A 4, hazard 1/64), 4 x
16-head gated value-residual policy, dropout 0.25 — C3: 1024 episodes x 128 steps, depth 4, d 256, batch
128; C2: 256 episodes x 3 genes x 500 steps, depth 2, d 128, EPO gene pool, batch 32.  The learners of a
geometry start from the same seed (their weights differ in shape, so their rollouts differ; the episodes'
lengths do not: the Sim's termination stream does not depend on the policy).  Written per variant: the
median rollout / learn-step milliseconds of the timed updates, the resident KV-cache bytes
(2 L E Hkv Tmax dh 4, read off the engine's tensors) and the algorithmic K + V bytes the decode attention
reads per env step — per live (row, kv head, layer) at step t the K and V rows of t + 1 keys — from the
last timed rollout's episode lengths.  A measurement, not a gate.
"""
import argparse
import json
import statistics
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / 'x-transformers-rl_amd')]

GEOMETRY = dict(
    c3=dict(S=8, A=4, episodes=1024, T=128, depth=4, dim=256, heads=4, dim_head=16, batch=128, hazard_log2=6,
            dropout=0.25, genes=0),
    c2=dict(S=8, A=4, episodes=256, T=500, depth=2, dim=128, heads=4, dim_head=16, batch=32, hazard_log2=6,
            dropout=0.25, genes=3))


def build(c, kv_heads, seed):
    import torch
    from xtrl_amd import Learner, SynthVecSim
    wm = dict(attn_dim_head=c['dim_head'], heads=c['heads'], depth=c['depth'], attn_gate_values=True,
              add_value_residual=True, learned_value_residual_mix=True)
    torch.manual_seed(seed)
    evo = c['genes'] > 0
    learner = Learner(state_dim=c['S'], num_actions=c['A'], reward_range=(-5., 5.), world_model=wm,
                      max_timesteps=c['T'], batch_size=c['batch'], num_episodes_per_update=c['episodes'],
                      evolutionary=evo, evolve_every=5, evolve_after_step=10,
                      latent_gene_pool=dict(dim=32, num_genes_per_island=max(c['genes'], 1), num_selected=2,
                                            tournament_size=2),
                      agent_kwargs=dict(hidden_dim=c['dim'], dropout=c['dropout'], seed=seed, kv_heads=kv_heads,
                                        save_path=str(Path(tempfile.gettempdir()) / 'xtrl_gqa_bench_ppo.pt')))
    return learner, SynthVecSim(c['S'], c['A'], 'lander', c['hazard_log2'])


def one_update(learner, env, T):
    import torch
    agent = learner.agent
    u = agent.step
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    traj, lens, genes, cum = learner.rollout_device(env, u, T)
    ev[1].record()
    fit = learner.fitness(cum, genes)
    agent.learn(traj, lens, genes, fit, update=u)
    ev[2].record()
    agent.logs = []
    return ev, lens


def kv_read_bytes(c, lens, kv_heads):
    """Algorithmic K + V bytes the decode attention reads in one rollout with these episode lengths."""
    total = sum(n * (n + 1) // 2 for n in map(int, lens))   # sum over steps t of t + 1 keys
    return 2 * total * c['dim_head'] * 4 * kv_heads * c['depth']


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--configs', nargs='+', default=['c3', 'c2'], choices=sorted(GEOMETRY))
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'attn_gqa_bench.json'))
    a = ap.parse_args()
    out = dict(steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), configs={})
    for name in a.configs:
        c = GEOMETRY[name]
        variants = {f'hkv{k}': k for k in (c['heads'], 2, 1)}
        built = {k: build(c, hkv, a.seed) for k, hkv in variants.items()}
        times = {k: [] for k in variants}
        lens_last = {}
        for step in range(a.warmup + a.steps):
            for k, (learner, env) in built.items():   # alternating: every variant sees the same machine state
                ev, lens = one_update(learner, env, c['T'])
                torch.cuda.synchronize()
                if step >= a.warmup:
                    times[k].append((ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])))
                    lens_last[k] = lens.cpu().tolist()
        res = {}
        for k, hkv in variants.items():
            learner, env = built[k]
            ro, le = [t[0] for t in times[k]], [t[1] for t in times[k]]
            lens = lens_last[k]
            steps = int(sum(lens))
            eng = learner._engine_for(env, c['T'])
            resident = sum(t.numel() * t.element_size() for kv in eng.kv for t in kv)
            kv = kv_read_bytes(c, lens, hkv)
            res[k] = dict(kv_heads=hkv, rollout_ms_median=round(statistics.median(ro), 3),
                          rollout_ms=[round(x, 3) for x in ro], learn_ms_median=round(statistics.median(le), 3),
                          learn_ms=[round(x, 3) for x in le], env_steps=steps, max_len=int(max(lens)),
                          kv_cache_resident_bytes=resident, kv_read_bytes_per_rollout=kv,
                          kv_read_bytes_per_env_step=round(kv / max(steps, 1), 1))
            print(json.dumps({name: {k: res[k]}}), flush=True)
        out['configs'][name] = dict(config=c, variants=res)
        del built
        torch.cuda.empty_cache()
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
