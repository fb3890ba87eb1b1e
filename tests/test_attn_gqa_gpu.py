"""Grouped-query attention in the learn-step attention kernels (q [b][H][n][dh]; k, v, dk, dv
[b][Hkv][n][dh]; query head h reads kv head ops.kv_head_index(H, Hkv)[h]) on the MI355X, through the
xtrl_attn_*_gqa entry points and ops.attention: against an fp64 dense reference (multi-head attention
on the repeated k / v, whose autograd sums dk / dv per group), against the old entry points at Hkv = H,
the backward modes against each other, and the dropout stream; then the rollout, the learn step and the
deploy forward with agent_kwargs kv_heads / world_model['attn_one_kv_head'] against the GQA oracle (test_attn_gqa_cpu.gqa_init /
gqa_forward installed over the frozen oracle's Attention)."""
import os

import pytest
import torch

from oracle import ref_port as R
from oracle import thirdparty as tp

import test_gpu_parity as G
from test_attn_gqa_cpu import gqa_forward, gqa_init
from test_attn_window_gpu import attn_win_ref, problem, win_lib
from test_gpu_parity import tol

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAMES = ('o', 'lse', 'delta', 'dq', 'dk', 'dv')


def gqa_problem(b, H, Hkv, n, dh, seed):
    """problem() with k, v cut to the first Hkv heads: q, k, v, do, ragged lens (lens[0] = n, lens[-1] = 1)."""
    q, k, v, do, lens = problem(b, H, n, dh, seed)
    return q, k[:, :Hkv].contiguous(), v[:, :Hkv].contiguous(), do, lens


def gqa_lib(q, k, v, lens, do, scale, p, W, mode, seed=3, offset=1, sub=0):
    """Forward + backward through xtrl_attn_fwd_gqa / xtrl_attn_bwd_gqa / xtrl_attn_bwd_part_gqa, outputs
    pre-filled with NaN.  ``W`` None: window 0 (none).  ``mode``: 'two' (XTRL_ATTN_FUSED_BWD=0: the dK/dV +
    dQ kernel pair), 'fused' (=1 without a workspace: one launch for n <= 128 at Hkv = H; Hkv < H has no
    fused form and runs the pair) or 'part' (=1 with the dQ partial workspace, NaN-filled)."""
    from xtrl_amd import _lib as L
    lib = L.lib()
    b, H, n, dh = q.shape
    Hkv = k.shape[1]
    nan = lambda *s: torch.full(s, float('nan'), device=DEV)   # noqa: E731
    o, dq, dk, dv = nan(*q.shape), nan(*q.shape), nan(*k.shape), nan(*v.shape)
    lse, delta = nan(b, H, n), nan(b, H, n)
    win = int(W or 0)
    L.check(lib.xtrl_attn_fwd_gqa(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(lens), L.ptr(o), L.ptr(lse), b, H, Hkv, n, dh, scale,
                                  p, seed, offset, sub, win, L.stream()), 'attn_fwd_gqa')
    old = os.environ.get('XTRL_ATTN_FUSED_BWD')
    os.environ['XTRL_ATTN_FUSED_BWD'] = '0' if mode == 'two' else '1'
    try:
        if mode == 'part':
            nf = int(lib.xtrl_attn_bwd_part_floats(b, H, n, dh))
            part = nan(nf)
            L.check(lib.xtrl_attn_bwd_part_gqa(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(lens), L.ptr(o), L.ptr(lse), L.ptr(do),
                                               L.ptr(dq), L.ptr(dk), L.ptr(dv), L.ptr(delta), L.ptr(part), nf, b, H, Hkv, n,
                                               dh, scale, p, seed, offset, sub, win, L.stream()), 'attn_bwd_part_gqa')
        else:
            L.check(lib.xtrl_attn_bwd_gqa(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(lens), L.ptr(o), L.ptr(lse), L.ptr(do),
                                          L.ptr(dq), L.ptr(dk), L.ptr(dv), L.ptr(delta), b, H, Hkv, n, dh, scale, p, seed,
                                          offset, sub, win, L.stream()), 'attn_bwd_gqa')
    finally:
        if old is None:
            del os.environ['XTRL_ATTN_FUSED_BWD']
        else:
            os.environ['XTRL_ATTN_FUSED_BWD'] = old
    torch.cuda.synchronize()
    return dict(o=o, lse=lse, delta=delta, dq=dq, dk=dk, dv=dv)


def modes_of(n, dh):
    """The backward modes that exist for a shape: the pair always; at dh = 16 the partial-workspace form,
    and for n <= 128 the fused dispatch."""
    return ['two'] + (['part'] if dh == 16 else []) + (['fused'] if dh == 16 and n <= 128 else [])


def gqa_ref(q, k, v, do, lens, W, keep=None):
    """fp64 dense reference: multi-head attention on k, v repeated to H heads by the head mapping; the
    index_select's backward sums dk / dv over each kv head's query heads.  W None: no window (a band of
    n masks nothing).  Returns (o, dq, dk, dv) on the CPU."""
    from xtrl_amd import ops
    H, Hkv, n, dh = q.shape[1], k.shape[1], q.shape[2], q.shape[3]
    idx = ops.kv_head_index(H, Hkv, device=k.device)
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    ref = attn_win_ref(qd, kd[:, idx], vd[:, idx], lens, dh ** -0.5, n if W is None else W, keep)
    (ref * do.double()).sum().backward()
    return tuple(t.detach().cpu() for t in (ref, qd.grad, kd.grad, vd.grad))


def check_ref(res, ref):
    """test_attn_window_gpu.check_fp64's tolerances."""
    o, dq, dk, dv = ref
    tol(res['o'], o, 1e-5, 1e-5)
    tol(res['dq'], dq, 1e-4, 1e-5)
    tol(res['dk'], dk, 1e-4, 1e-5)
    tol(res['dv'], dv, 1e-4, 1e-5)


@pytest.mark.parametrize('b,H,Hkv,n,dh,W', [(3, 4, 2, 37, 16, None), (2, 4, 1, 70, 16, None), (2, 4, 2, 130, 16, None),
                                            (2, 4, 2, 130, 16, 10), (2, 4, 1, 200, 16, 64), (2, 6, 2, 64, 32, 7),
                                            (1, 4, 2, 70, 64, None)])
def test_gqa_forward_and_backward_against_fp64(b, H, Hkv, n, dh, W):
    """Forward + every backward mode of the shape at p = 0 against the fp64 reference, ragged lengths
    (one full episode, one of a single step), every output NaN-filled before and finite after.  W = 10 at
    n = 130 and W = 7 at n = 64 leave padded rows past the band: the uniform rows of k_attn_dead_fwd /
    k_attn_dead_bwd, whose dV part sums the group's query heads."""
    q, k, v, do, lens = gqa_problem(b, H, Hkv, n, dh, n + dh + Hkv + (W or 0))
    ref = gqa_ref(q, k, v, do, lens, W)
    for mode in modes_of(n, dh):
        res = gqa_lib(q, k, v, lens, do, dh ** -0.5, 0., W, mode)
        for name in NAMES:
            assert torch.isfinite(res[name]).all(), (mode, name)
        assert res['dk'].shape == (b, Hkv, n, dh) and res['dv'].shape == (b, Hkv, n, dh)
        check_ref(res, ref)


@pytest.mark.parametrize('W', [None, 10])
@pytest.mark.parametrize('n', [70, 130])
@pytest.mark.parametrize('p', [0., 0.25])
def test_gqa_entry_points_with_all_kv_heads_are_the_old_ones(p, n, W):
    """Hkv = H through the _gqa entry points: o, lse, D, dq, dk, dv bit-identical to xtrl_attn_fwd /
    xtrl_attn_bwd / xtrl_attn_bwd_part (and their _win forms) in every backward mode."""
    b, H, dh = 2, 4, 16
    q, k, v, do, lens = problem(b, H, n, dh, n + 3)
    for mode in modes_of(n, dh):
        old = win_lib(q, k, v, lens, do, dh ** -0.5, p, W, mode)
        new = gqa_lib(q, k, v, lens, do, dh ** -0.5, p, W, mode)
        for name in NAMES:
            assert torch.equal(old[name], new[name]), (mode, name)


@pytest.mark.parametrize('Hkv,n,W', [(2, 70, None), (1, 128, 10), (2, 130, None), (1, 200, 64)])
@pytest.mark.parametrize('p', [0., 0.25])
def test_gqa_backward_modes_agree_and_repeat(p, Hkv, n, W):
    """The backward modes under GQA: the fused dispatch (n <= 128) bit-identical to the kernel pair in
    every output, as the project requires without GQA (Hkv < H has no fused kernel: the dispatch runs
    the pair); the partial-workspace form bit-identical in dK, dV, D and within 2e-6 of the dQ scale in
    dQ (the bound of test_attention_long_backward_dq_folded_matches_two_kernel: its dQ sums key-tile
    partials).  Each mode run twice gives the same dK / dV bits: the group sum has a fixed order."""
    b, H, dh = 2, 4, 16
    q, k, v, do, lens = gqa_problem(b, H, Hkv, n, dh, n + Hkv)
    two = gqa_lib(q, k, v, lens, do, dh ** -0.5, p, W, 'two')
    for mode in modes_of(n, dh):
        res = gqa_lib(q, k, v, lens, do, dh ** -0.5, p, W, mode)
        again = gqa_lib(q, k, v, lens, do, dh ** -0.5, p, W, mode)
        assert torch.equal(res['dk'], again['dk']) and torch.equal(res['dv'], again['dv']), mode
        for name in ('o', 'lse', 'delta', 'dk', 'dv'):
            assert torch.equal(res[name], two[name]), (mode, name)
        if mode == 'part':
            scale = float(two['dq'].abs().max())
            err = float((res['dq'] - two['dq']).abs().max())
            print('dq err', err, 'scale', scale)
            assert err <= 2e-6 * scale, (err, scale)
        else:
            assert torch.equal(res['dq'], two['dq']), mode


def test_gqa_dropout_mask_is_keyed_by_the_query_head():
    """p = 0.25 at Hkv = 1: the kept probabilities are the host Philox stream's bits of the query head
    (c2 = offset + b H + h, the stream of multi-head attention with the same H) — forward and q / k / v
    gradients of ops.attention against the fp64 reference times that keep mask, with and without a
    window."""
    from xtrl_amd import ops
    from oracle import philox as P
    b, H, Hkv, n, dh, p = 2, 4, 1, 130, 16, 0.25
    g = torch.Generator().manual_seed(11)
    q, do = (torch.randn(b, H, n, dh, generator=g) for _ in range(2))
    k, v = (torch.randn(b, Hkv, n, dh, generator=g) for _ in range(2))
    lens = torch.tensor([130, 45], dtype=torch.int32)
    seed, offset, layer = 1234567, 5, 3
    keep = torch.from_numpy(P.attn_dropout_keep(b, H, n, p, seed, offset, layer)).double() / (1 - p)
    for W in (None, 10):
        ref, dq, dk, dv = gqa_ref(q, k, v, do, lens, W, keep)
        qf, kf, vf = (t.to(DEV).requires_grad_() for t in (q, k, v))
        out = ops.attention(qf, kf, vf, lens.to(DEV), dh ** -0.5, p, seed=seed, offset=offset, sub=layer, window=W or 0)
        (out * do.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        assert kf.grad.shape == k.shape and vf.grad.shape == v.shape
        tol(out, ref, 1e-5, 1e-5)
        tol(qf.grad, dq, 1e-4, 1e-5)
        tol(kf.grad, dk, 1e-4, 1e-5)
        tol(vf.grad, dv, 1e-4, 1e-5)


# ----------------------------------------------------------------------------------------------
# model level: the GQA oracle (test_attn_gqa_cpu.gqa_init / gqa_forward over the frozen Attention)
# ----------------------------------------------------------------------------------------------


def make_gqa_learner(Hkv, W=None, depth=2, gates=True, T=24, episodes=6, batch=3, seed=3, hazard=5, mode='lander',
                     dim=48, agent_extra=None, use_graph=False, with_oracle=True):
    """Learner with agent_kwargs kv_heads = Hkv — Hkv = 1 through world_model['attn_one_kv_head'] = True instead,
    so both ways in are run — (H = 4; and attn_max_attend_past = W), the device
    Sim and the oracle on the same weights (test_attn_window_gpu.make_win_learner's construction; the
    oracle takes GQA and the window from the patched Attention, which the caller installs first;
    ``with_oracle`` False: a device-only test, no oracle is built)."""
    from xtrl_amd import Learner, SynthVecSim
    S, A = 8, 4
    torch.manual_seed(seed)
    wm = dict(attn_dim_head=16, heads=4, depth=depth)
    if Hkv == 1:
        wm['attn_one_kv_head'] = True
    if gates:
        wm.update(attn_gate_values=True, add_value_residual=True, learned_value_residual_mix=True)
    if W is not None:
        wm['attn_max_attend_past'] = W
    gp = dict(dim=8, num_genes_per_island=3, num_selected=2, tournament_size=2)
    learner = Learner(state_dim=S, num_actions=A, reward_range=(-2., 2.), world_model=wm, max_timesteps=T,
                      batch_size=batch, num_episodes_per_update=episodes, evolutionary=False, latent_gene_pool=gp,
                      agent_kwargs=dict(dropout=0., seed=seed, hidden_dim=dim, reward_dropout=0.5,
                                        **(dict(kv_heads=Hkv) if Hkv != 1 else {}), **(agent_extra or {})),
                      use_graph=use_graph)
    with torch.no_grad():   # non-trivial gate / mix weights (their init is constant)
        g = torch.Generator().manual_seed(seed + 1)
        for name, p in learner.agent.model.named_parameters():
            if 'to_v_gate' in name or 'to_value_residual_mix' in name:
                p.copy_((torch.randn(p.shape, generator=g) * 0.3).to(p.device))
        learner.agent.ema_flat.copy_(learner.agent.flat.flat)
    env = SynthVecSim(S, A, mode, hazard_log2=hazard)
    if not with_oracle:
        return learner, env, None
    c = R.LearnerConfig(S, A, (-2., 2.), dim=dim, depth=depth, gate_values=gates, value_residual=gates,
                        learned_mix=gates, max_timesteps=T, batch_size=batch, num_episodes_per_update=episodes,
                        sim_mode=mode, hazard_log2=hazard, seed=seed, reward_dropout=0.5, gene_pool=gp)
    sd = {k: v.detach().cpu() for k, v in learner.agent.model.state_dict().items()}
    oracle = R.OracleLearner(c, init_state_dict=sd)
    return learner, env, oracle


def install_gqa_oracle(monkeypatch, Hkv, W=None):
    monkeypatch.setattr(tp.Attention, '__init__', gqa_init(Hkv))
    monkeypatch.setattr(tp.Attention, 'forward', gqa_forward(W))


def gqa_rollout_and_learn(monkeypatch, Hkv, T, minibatches, W=None, **kw):
    """Rollout (actions, lengths, rewards bit-exact; log-probs and logits within 1e-4: G.compare_rollout)
    and ``minibatches`` learn minibatches (loss within 1e-4 relative, gradients within 1e-4 of scale:
    G._learn_parity) against the GQA oracle; the engine's caches must have Hkv heads."""
    install_gqa_oracle(monkeypatch, Hkv, W)
    learner, env, oracle = make_gqa_learner(Hkv, W, T=T, **kw)
    assert learner.agent.cfg.kv_heads == Hkv
    traj, lens, genes, cum = learner.rollout_device(env, 0, T)
    torch.cuda.synchronize()
    eng = learner._engine_for(env, T)
    for kc, vc in eng.kv:
        assert kc.shape == vc.shape == (eng.E, Hkv, T, 16)
    assert eng.v1.shape == (eng.E, Hkv * 16)
    episodes, _ = oracle.rollout(0)
    G.compare_rollout(traj, lens, episodes)
    seen = []
    if minibatches:
        seen = G._learn_parity(learner, oracle, traj, lens, genes, learner.fitness(cum, genes), minibatches)
    return learner, lens, seen


@pytest.mark.parametrize('rows', ['1', '0'])
@pytest.mark.parametrize('Hkv', [1, 2])
def test_gqa_rollout_and_learn_match_oracle(Hkv, rows, monkeypatch):
    """H = 4, d = 48, depth 2 with gates and the learned value-residual mix (one per kv head), T = 24:
    both decode paths (the row-resident step and the multi-kernel step), then two learn minibatches."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', rows)
    _, lens, seen = gqa_rollout_and_learn(monkeypatch, Hkv, 24, 2, depth=2, gates=True, episodes=6, batch=3, hazard=5)
    assert int(lens.max()) > 10 and len(seen) == 2


def test_gqa_d256_fused_out_projection_rollout(monkeypatch):
    """d = 256, Hkv = 2, T = 40: the attention decode kernel that applies the out-projection itself (every
    wave of a row keeps its own query head's W_out rows while two waves share a kv head's cache rows)."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', '0')
    _, lens, _ = gqa_rollout_and_learn(monkeypatch, 2, 40, 0, depth=2, gates=True, episodes=6, batch=3, hazard=5, dim=256)
    assert int(lens.max()) > 7


@pytest.mark.parametrize('rows', ['1', '0'])
def test_gqa_rollout_across_the_128_key_chunk(rows, monkeypatch):
    """150 steps of the non-terminating Sim, depth 1, no gates, Hkv = 1: four waves read one kv head's
    cache past the first 128-key chunk."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', rows)
    _, lens, _ = gqa_rollout_and_learn(monkeypatch, 1, 150, 0, depth=1, gates=False, episodes=4, batch=2, mode='readme')
    assert int(lens.min()) == 150


def test_gqa_with_window_d256_rollout_and_learn(monkeypatch):
    """GQA x window: Hkv = 2, W = 7, d = 256, T = 40, two minibatches.  The padded rows past the band
    (i >= len + W) take k_attn_dead_fwd / k_attn_dead_bwd, whose dV part sums the group's query heads;
    the minibatches must really have such rows."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', '0')
    learner, lens, seen = gqa_rollout_and_learn(monkeypatch, 2, 40, 2, W=7, depth=2, gates=True, episodes=6, batch=3,
                                                hazard=5, dim=256)
    assert learner.agent.cfg.attn_window == 7 and len(seen) == 2
    n_max = max(s[0] for s in seen)
    assert int(lens.min()) + 7 < n_max, (lens.tolist(), seen)   # an episode with rows past its band in the widest minibatch


def test_gqa_long_episode_learn_matches_oracle(monkeypatch):
    """T = 140, Hkv = 1, depth 1: the learn step's attention backward takes the n > 128 form (the group
    loop in the dK/dV kernel with the dQ pass folded in, partials per query head)."""
    learner, lens, seen = gqa_rollout_and_learn(monkeypatch, 1, 140, 1, depth=1, gates=True, episodes=4, batch=2,
                                                mode='readme')
    assert seen[0][0] > 128
    assert 'dq_part' in learner.agent._train_step.cbuf


def test_gqa_packed_learn_matches_padded_step():
    """packed_learn (per-episode row ranges) with Hkv = 2 at T = 70 against the padded step: the bounds
    of test_packed_learn_matches_padded_step."""
    res = {}
    for packed in (False, True):
        learner, env, _ = make_gqa_learner(2, depth=2, gates=True, T=70, episodes=8, batch=8, seed=5, hazard=5, dim=64,
                                           agent_extra=dict(hl_reduction_mean=False, packed_learn=packed), with_oracle=False)
        agent = learner.agent
        traj, lens, genes, cum = learner.rollout_device(env, 0, 70)
        res[packed] = G._first_minibatch_state(agent, traj, lens, genes, learner.fitness(cum, genes))
        res[packed]['lens'] = lens.cpu()
    a, b = res[True], res[False]
    assert torch.equal(a['lens'], b['lens']) and torch.equal(a['idx'], b['idx'])
    lens_mb = a['lens'][a['idx']].clamp(max=a['n'])
    assert lens_mb.min() < a['n']    # padding present
    valid = (torch.arange(a['n'])[None, :] < lens_mb[:, None]).to(a['raw'].device)
    assert (a['raw'][~valid] == 0).all() and (a['values'][~valid] == 0).all()
    for k in ('raw', 'values'):
        x, y = a[k][valid], b[k][valid]
        assert float((x - y).abs().max()) <= 1e-4 * float(y.abs().max()) + 1e-6, k
    assert abs(a['loss'] - b['loss']) <= 1e-5 * abs(b['loss']) + 1e-7, (a['loss'], b['loss'])
    bad = []
    for name, (o0, o1) in learner.agent.flat.index.items():
        g0, g1 = a['grad'][o0:o1], b['grad'][o0:o1]
        own = float(g1.abs().max())
        if float((g0 - g1).abs().max()) > 1e-4 * own + 1e-7:
            bad.append((name, float((g0 - g1).abs().max()), own))
    assert not bad, bad


@pytest.mark.parametrize('p', [0., 0.25])
def test_gqa_fused_step_matches_reference_mode_autograd(p):
    """The hand-scheduled learn step against the reference-mode autograd step (model.forward_train with
    ops.attention on Hkv-head k, v) at Hkv = 2 with gates, T = 70: the bounds of
    test_fused_train_step_matches_autograd."""
    learner, env, _ = make_gqa_learner(2, depth=2, gates=True, T=70, episodes=8, batch=4, seed=9, hazard=5, dim=64,
                                       with_oracle=False)
    agent = learner.agent
    agent.cfg.dropout = p
    agent.model.cfg.dropout = p
    traj, lens, genes, cum = learner.rollout_device(env, 0, 70)
    fit = learner.fitness(cum, genes)
    agent.fused_learn = True
    a = G._first_minibatch(agent, traj, lens, genes, fit)
    agent.fused_learn = False
    b = G._first_minibatch(agent, traj, lens, genes, fit)
    assert abs(a['loss'] - b['loss']) <= 1e-5 * abs(b['loss']) + 1e-6, (a['loss'], b['loss'])
    scale = float(b['grad'].abs().max())
    for name, (s, e) in agent.flat.index.items():
        err = float((a['grad'][s:e] - b['grad'][s:e]).abs().max())
        assert err <= 1e-4 * scale + 1e-7, (name, err, scale)


def test_gqa_deploy_forward_matches_oracle_cached_decode(monkeypatch):
    """Agent.forward over 10 steps at Hkv = 1 against the GQA oracle's cached decode; the hiddens' cache
    tensors have one kv head."""
    install_gqa_oracle(monkeypatch, 1)
    learner, env, oracle = make_gqa_learner(1, depth=2, gates=True, T=24)
    agent = learner.agent
    agent.rs_mean.copy_(torch.linspace(-0.5, 0.5, 9))
    agent.rs_var.copy_(torch.linspace(0.5, 2., 9))
    rs = R.RSNormState(9)
    rs.mean, rs.var = agent.rs_mean.cpu().clone(), agent.rs_var.cpu().clone()
    m = oracle.model
    m.eval()
    g = torch.Generator().manual_seed(2)
    hiddens, cache = None, None
    for t in range(10):
        s = torch.randn(8, generator=g)
        reward = None if t % 2 == 0 else float(torch.randn((), generator=g))
        raw, hiddens = agent(s.numpy(), reward=reward, hiddens=hiddens)
        swr = rs.apply(torch.cat((s, torch.tensor([0. if reward is None else reward]))))
        with torch.no_grad():
            r, _, _, _, cache = m(swr[:-1].reshape(1, 1, -1), rewards=None if reward is None else swr[-1], cache=cache)
        tol(raw, r.reshape(-1), 1e-4, 1e-5)
    kv = [x for x in hiddens['cache'] if x.dim() == 4]
    assert kv and all(x.shape[1] == 1 and x.shape[3] == 16 for x in kv)


def test_gqa_rollout_graph_replay_equals_eager():
    """One GQA rollout (Hkv = 2, d = 48: the row-resident step's graphs) captured and replayed equals the
    eager rollout bit for bit, as test_rollout_graph_replay_equals_eager."""
    learner, env, _ = make_gqa_learner(2, depth=2, gates=True, T=16, episodes=40, batch=4, hazard=3, with_oracle=False)
    traj, lens, _, _ = learner.rollout_device(env, 0, 16)
    eager = {k: v.clone() for k, v in traj.items() if v is not None}
    learner.use_graph = True
    learner._engine = None
    for update in (0, 0):   # capture, then replay
        traj, lens2, _, _ = learner.rollout_device(env, update, 16)
    torch.cuda.synchronize()
    for k, v in eager.items():
        assert torch.equal(v, traj[k]), k
