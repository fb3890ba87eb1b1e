"""The per-head output gates at the C2 geometry: rollout and learn-step time with and without
world_model['attn_gate_value_heads'], on the gated model (attn_gate_values + the learned value-residual mix, C2's
own) and on the ungated one; device events, the learners alternating in one process.

    timeout 900 python tools/head_gate_bench.py [--steps 4] [--warmup 2] [--out profiles/attn_head_gate_c2.json]
                                                [--only VARIANT --updates N]

C2 (bench.py CONFIGS['c2'], restated as in tools/softclamp_bench.py): LunarLander-shaped device Sim (S 8, A 4, hazard
1/64), 256 episodes x 3 genes x 500 steps, depth-2 d = 128 4 x 16-head policy with an EPO gene pool, batch 32,
dropout 0.25, the padded learn step.  All learners start from the same seed; the head-gate parameters are
randomised (weight N(0, 1) / sqrt(d), bias N(0, 1)) so the gates are not all open.  The lengths of the episodes
come from the Sim's termination stream alone, so every variant's learn step sees the same padding.  What the
numbers answer: the option adds, per layer and minibatch, one row pass over [T][I] after the attention forward and
one after the out-projection's input gradient, H more columns in the projection GEMMs, and one scalar multiply
in the decode kernels' last step:
    head-gate cost = gated+head_gate - gated     (on top of the element gate: og exists already)
                   = head_gate - none            (alone: og becomes a buffer of its own)
both written per phase under "costs".  Written: per variant the median rollout / learn-step milliseconds of the
timed updates.  ``--only VARIANT --updates N``: N updates of one variant and nothing written: the workload of a
kernel trace.  A measurement, not a gate.
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


def build(gated, head_gate, seed):
    import torch
    from xtrl_amd import Learner, SynthVecSim
    c = C2
    wm = dict(attn_dim_head=c['dim_head'], heads=c['heads'], depth=c['depth'], attn_gate_value_heads=head_gate)
    if gated:
        wm.update(attn_gate_values=True, add_value_residual=True, learned_value_residual_mix=True)
    torch.manual_seed(seed)
    learner = Learner(state_dim=c['S'], num_actions=c['A'], reward_range=(-5., 5.), world_model=wm,
                      max_timesteps=c['T'], batch_size=c['batch'], num_episodes_per_update=c['episodes'],
                      evolutionary=True, evolve_every=5, evolve_after_step=10,
                      latent_gene_pool=dict(dim=32, num_genes_per_island=c['genes'], num_selected=2, tournament_size=2),
                      agent_kwargs=dict(hidden_dim=c['dim'], dropout=c['dropout'], seed=seed,
                                        save_path=str(Path(tempfile.gettempdir()) / 'xtrl_head_gate_bench_ppo.pt')))
    if head_gate:
        agent = learner.agent
        g = torch.Generator().manual_seed(seed + 1)
        with torch.no_grad():
            for name, p in agent.model.named_parameters():
                if 'to_v_head_gate' in name:
                    r = torch.randn(p.shape, generator=g)
                    p.copy_((r / p.shape[-1] ** 0.5 if p.ndim == 2 else r).to(p.device))
            agent.ema_flat.copy_(agent.flat.flat)
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


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=4)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--only', default=None)
    ap.add_argument('--updates', type=int, default=2)
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'attn_head_gate_c2.json'))
    a = ap.parse_args()
    # (attn_gate_values + value-residual mix, attn_gate_value_heads)
    variants = {'gated': (True, False), 'gated+head_gate': (True, True), 'none': (False, False),
                'head_gate': (False, True)}
    if a.only is not None:
        learner, env = build(*variants[a.only], a.seed)
        for _ in range(a.updates):
            one_update(learner, env)
        torch.cuda.synchronize()
        return
    built = {k: build(*v, a.seed) for k, v in variants.items()}
    times = {k: [] for k in variants}
    lens_last = {}
    for step in range(a.warmup + a.steps):
        for k, (learner, env) in built.items():   # alternating: every variant sees the same machine state
            ev, lens = one_update(learner, env)
            torch.cuda.synchronize()
            if step >= a.warmup:
                times[k].append((ev[0].elapsed_time(ev[1]), ev[1].elapsed_time(ev[2])))
                lens_last[k] = lens.cpu().tolist()
    out = dict(config=C2, steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), variants={})
    for k, (gated, hg) in variants.items():
        ro, le = [t[0] for t in times[k]], [t[1] for t in times[k]]
        lens = lens_last[k]
        out['variants'][k] = dict(attn_gate_values=gated, attn_gate_value_heads=hg,
                                  rollout_ms_median=round(statistics.median(ro), 3), rollout_ms=[round(x, 3) for x in ro],
                                  learn_ms_median=round(statistics.median(le), 3), learn_ms=[round(x, 3) for x in le],
                                  env_steps=int(sum(lens)), max_len=int(max(lens)))
        print(json.dumps({k: out['variants'][k]}), flush=True)
    v = out['variants']
    diff = lambda x, y: {ph: round(v[x][f'{ph}_ms_median'] - v[y][f'{ph}_ms_median'], 3) for ph in ('rollout', 'learn')}   # noqa: E731
    out['costs'] = {'head gate on the gated model (gated+head_gate - gated)': diff('gated+head_gate', 'gated'),
                    'head gate alone (head_gate - none)': diff('head_gate', 'none')}
    print(json.dumps(dict(costs=out['costs'])), flush=True)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    json.dump(out, open(a.out, 'w'), indent=1)


if __name__ == '__main__':
    main()
