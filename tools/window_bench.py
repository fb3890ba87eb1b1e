"""Sliding-window attention at the C2 geometry: rollout and learn-step time with and without
world_model['attn_max_attend_past'] = 63, device events, the two learners alternating in one process.

    timeout 900 python tools/window_bench.py [--steps 4] [--warmup 2] [--window 63]
                                             [--out profiles/attn_window_c2.json]

C2 (bench.py CONFIGS['c2'], restated here): LunarLander-shaped device Sim (S 8, A 4, hazard 1/64),
256 episodes x 3 genes x 500 steps, depth-2 d = 128 4 x 16-head gated value-residual policy with an
EPO gene pool, batch 32, dropout 0.25.  Both learners start from the same seed; their rollouts differ
once a window masks a key (the episodes' lengths do not: the Sim's termination stream does not depend
on the policy).  Written: per variant the median rollout / learn-step milliseconds of the timed
updates, and the algorithmic KV-cache bytes the decode attention reads per rollout — per live (row,
head, layer) at step t the K and V rows of min(t + 1, W + 1) keys, 2 min(t + 1, W + 1) dh 4 bytes —
summed over the last timed rollout's episode lengths.  A measurement, not a gate.
"""
import argparse
import json
import statistics
import sys
import tempfile
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / 'x-transformers-rl_amd')]

C2 = dict(S=8, A=4, episodes=256, T=500, depth=2, dim=128, heads=4, dim_head=16, batch=32, hazard_log2=6,
          dropout=0.25, genes=3)


def build(window, seed):
    import torch
    from xtrl_amd import Learner, SynthVecSim
    c = C2
    wm = dict(attn_dim_head=c['dim_head'], heads=c['heads'], depth=c['depth'], attn_gate_values=True,
              add_value_residual=True, learned_value_residual_mix=True, attn_max_attend_past=window)
    torch.manual_seed(seed)
    learner = Learner(state_dim=c['S'], num_actions=c['A'], reward_range=(-5., 5.), world_model=wm,
                      max_timesteps=c['T'], batch_size=c['batch'], num_episodes_per_update=c['episodes'],
                      evolutionary=True, evolve_every=5, evolve_after_step=10,
                      latent_gene_pool=dict(dim=32, num_genes_per_island=c['genes'], num_selected=2, tournament_size=2),
                      agent_kwargs=dict(hidden_dim=c['dim'], dropout=c['dropout'], seed=seed,
                                        save_path=str(Path(tempfile.gettempdir()) / 'xtrl_window_bench_ppo.pt')))
    return learner, SynthVecSim(c['S'], c['A'], 'lander', c['hazard_log2'])


def one_update(learner, env):
    import torch
    agent = learner.agent
    u = agent.step
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    ev[0].record()
    traj, lens, genes, cum = learner.rollout_device(env, u, C2['T'])
    ev[1].record()
    fit = learner.fitness(cum, genes)
    agent.learn(traj, lens, genes, fit, update=u)
    ev[2].record()
    agent.logs = []
    return ev, lens


def kv_bytes(lens, window):
    """Algorithmic K + V bytes the decode attention reads in one rollout with these episode lengths."""
    c = C2
    total = 0
    for n in lens:
        for t in range(int(n)):
            keys = t + 1 if not window else min(t + 1, window + 1)
            total += 2 * keys * c['dim_head'] * 4
    return total * c['heads'] * c['depth']


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--window', type=int, default=63)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'attn_window_c2.json'))
    a = ap.parse_args()
    variants = {'none': None, f'w{a.window}': a.window}
    built = {k: build(w, a.seed) for k, w in variants.items()}
    times = {k: [] for k in variants}
    lens_last = {}
    for step in range(a.warmup + a.steps):
        for k, (learner, env) in built.items():   # alternating: both variants see the same machine state
            ev, lens = one_update(learner, env)
            torch.cuda.synchronize()
            if step >= a.warmup:
                times[k].append((ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])))
                lens_last[k] = lens.cpu().tolist()
    out = dict(config=C2, window=a.window, steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0),
               variants={})
    for k, w in variants.items():
        ro, le = [t[0] for t in times[k]], [t[1] for t in times[k]]
        lens = lens_last[k]
        steps = int(sum(lens))
        kv = kv_bytes(lens, w)
        out['variants'][k] = dict(window=w, rollout_ms_median=round(statistics.median(ro), 3),
                                  rollout_ms=[round(x, 3) for x in ro], learn_ms_median=round(statistics.median(le), 3),
                                  learn_ms=[round(x, 3) for x in le], env_steps=steps, max_len=int(max(lens)),
                                  kv_bytes_per_rollout=kv, kv_bytes_per_env_step=round(kv / max(steps, 1), 1))
        print(json.dumps({k: out['variants'][k]}), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
