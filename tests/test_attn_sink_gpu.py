"""Attention sinks (world_model['attn_num_mem_kv'] = M memory key / value rows per kv head,
world_model['attn_add_zero_kv'] = Z one all-zero key / value) on the MI355X: the learn-step kernels through
the xtrl_attn_*_sink entry points and ops.attention against the fp64 dense reference of
test_attn_sink_cpu.attn_sink_ref (with the window, GQA and every backward mode), against the _gqa entry
points without sinks, run to run, and with dropout against the host keep bits
(oracle.philox.attn_dropout_keep for the real columns, test_attn_sink_cpu.sink_dropout_keep for the sink
columns); then the rollout, the padded and the packed learn step, the deploy forward and the reference-mode
autograd step against the sink oracle (test_attn_sink_cpu.sink_init / sink_forward installed over the
frozen oracle's Attention)."""
import os

import pytest
import torch

from oracle import philox as P
from oracle import ref_port as R
from oracle import thirdparty as tp

import test_gpu_parity as G
from test_attn_gqa_gpu import gqa_lib, gqa_problem, modes_of
from test_attn_sink_cpu import attn_sink_ref, sink_dropout_keep, sink_forward, sink_init, visible
from test_attn_window_gpu import problem
from test_gpu_parity import tol

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAMES = ('o', 'lse', 'delta', 'dq', 'dk', 'dv')
SHAPES = [(3, 4, 4, 37, 16, None), (2, 4, 2, 70, 16, None), (2, 4, 2, 130, 16, 10), (2, 4, 1, 200, 16, 64),
          (2, 6, 2, 64, 32, 7), (1, 4, 2, 70, 64, None)]
SINKS = [(0, 1), (1, 0), (3, 1), (16, 0)]


# ----------------------------------------------------------------------------------------------
# kernel level
# ----------------------------------------------------------------------------------------------


def sink_problem(b, H, Hkv, n, dh, M, seed):
    """gqa_problem (q, k, v, do, ragged lens with lens[0] = n and lens[-1] = 1) plus mem_k, mem_v [Hkv][M][dh]
    (None at M = 0)."""
    q, k, v, do, lens = gqa_problem(b, H, Hkv, n, dh, seed)
    g = torch.Generator().manual_seed(seed + 1000)
    mem_k, mem_v = (torch.randn(Hkv, M, dh, generator=g).to(DEV) for _ in range(2)) if M else (None, None)
    return q, k, v, do, lens, mem_k, mem_v


def sink_lib(q, k, v, lens, do, scale, p, W, mode, mem_k, mem_v, Z, seed=3, offset=1, sub=0):
    """Forward + backward through xtrl_attn_fwd_sink / xtrl_attn_bwd_sink / xtrl_attn_bwd_part_sink, every
    output (and both workspaces) pre-filled with NaN.  ``mode`` as test_attn_gqa_gpu.gqa_lib: 'two', 'fused'
    or 'part'.  mem_k None: M = 0 (null sink pointers)."""
    from xtrl_amd import _lib as L
    lib = L.lib()
    b, H, n, dh = q.shape
    Hkv = k.shape[1]
    M = 0 if mem_k is None else mem_k.shape[1]
    nan = lambda *s: torch.full(s, float('nan'), device=DEV)   # noqa: E731
    o, dq, dk, dv = nan(*q.shape), nan(*q.shape), nan(*k.shape), nan(*v.shape)
    lse, delta = nan(b, H, n), nan(b, H, n)
    dmk, dmv = (nan(Hkv, M, dh), nan(Hkv, M, dh)) if M else (None, None)
    nws = int(lib.xtrl_attn_sink_ws_floats(b, H, M, dh))
    ws = nan(nws) if M else None
    win = int(W or 0)
    L.check(lib.xtrl_attn_fwd_sink(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(lens), L.ptr(o), L.ptr(lse), L.ptr(mem_k),
                                   L.ptr(mem_v), b, H, Hkv, n, dh, scale, p, seed, offset, sub, win, M, int(Z),
                                   L.stream()), 'attn_fwd_sink')
    old = os.environ.get('XTRL_ATTN_FUSED_BWD')
    os.environ['XTRL_ATTN_FUSED_BWD'] = '0' if mode == 'two' else '1'
    sink = (L.ptr(mem_k), L.ptr(mem_v), L.ptr(dmk), L.ptr(dmv), L.ptr(ws), nws)
    try:
        if mode == 'part':
            nf = int(lib.xtrl_attn_bwd_part_floats(b, H, n, dh))
            part = nan(nf)
            L.check(lib.xtrl_attn_bwd_part_sink(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(lens), L.ptr(o), L.ptr(lse),
                                                L.ptr(do), L.ptr(dq), L.ptr(dk), L.ptr(dv), L.ptr(delta), L.ptr(part),
                                                nf, *sink, b, H, Hkv, n, dh, scale, p, seed, offset, sub, win, M, int(Z),
                                                L.stream()), 'attn_bwd_part_sink')
        else:
            L.check(lib.xtrl_attn_bwd_sink(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(lens), L.ptr(o), L.ptr(lse), L.ptr(do),
                                           L.ptr(dq), L.ptr(dk), L.ptr(dv), L.ptr(delta), *sink, b, H, Hkv, n, dh,
                                           scale, p, seed, offset, sub, win, M, int(Z), L.stream()), 'attn_bwd_sink')
    finally:
        if old is None:
            del os.environ['XTRL_ATTN_FUSED_BWD']
        else:
            os.environ['XTRL_ATTN_FUSED_BWD'] = old
    torch.cuda.synchronize()
    res = dict(o=o, lse=lse, delta=delta, dq=dq, dk=dk, dv=dv)
    if M:
        res.update(dmk=dmk, dmv=dmv)
    return res


def sink_ref(q, k, v, do, lens, W, mem_k, mem_v, Z, keep=None, keep_mem=None):
    """The fp64 reference (test_attn_sink_cpu.attn_sink_ref) on k, v and the memory rows repeated to the
    query heads by ops.kv_head_index; autograd sums dk / dv / dmem over each kv head's query heads.
    Returns a dict of CPU tensors: o, lse, dq, dk, dv (and dmk, dmv)."""
    from xtrl_amd import ops
    H, Hkv, dh = q.shape[1], k.shape[1], q.shape[3]
    idx = ops.kv_head_index(H, Hkv, device=k.device)
    leaves = [t.double().requires_grad_() for t in (q, k, v)]
    mems = [t.double().requires_grad_() for t in (mem_k, mem_v)] if mem_k is not None else [None, None]
    o, lse = attn_sink_ref(leaves[0], leaves[1][:, idx], leaves[2][:, idx], lens, dh ** -0.5, W,
                           None if mems[0] is None else mems[0][idx], None if mems[1] is None else mems[1][idx], bool(Z),
                           keep, keep_mem)
    (o * do.double()).sum().backward()
    out = dict(o=o, lse=lse, dq=leaves[0].grad, dk=leaves[1].grad, dv=leaves[2].grad)
    if mems[0] is not None:
        out.update(dmk=mems[0].grad, dmv=mems[1].grad)
    return {n: t.detach().cpu() for n, t in out.items()}


def check_ref(res, ref):
    """test_attn_gqa_gpu.check_ref's tolerances; the same for dmem_k / dmem_v; lse and the row sum L = exp(lse),
    which includes the sinks."""
    tol(res['o'], ref['o'], 1e-5, 1e-5)
    tol(res['lse'], ref['lse'], 1e-5, 1e-5)
    tol(res['lse'].exp(), ref['lse'].exp(), 1e-5, 1e-5)
    for name in ('dq', 'dk', 'dv') + (('dmk', 'dmv') if 'dmk' in ref else ()):
        tol(res[name], ref[name], 1e-4, 1e-5)


@pytest.mark.parametrize('M,Z', SINKS)
@pytest.mark.parametrize('b,H,Hkv,n,dh,W', SHAPES)
def test_sink_forward_and_backward_against_fp64(b, H, Hkv, n, dh, W, M, Z):
    """Forward + every backward mode of the shape at p = 0 against the fp64 reference, ragged lengths (one
    full episode, one of a single step), every output NaN-filled before and finite after.  Under a window
    the single-step episode has padded rows past the band (i >= 1 + W): they attend the sinks alone — with
    the zero key only their o is exactly 0 — and whatever their dO, they add nothing to dK / dV."""
    q, k, v, do, lens, mem_k, mem_v = sink_problem(b, H, Hkv, n, dh, M, n + dh + Hkv + (W or 0) + M)
    ref = sink_ref(q, k, v, do, lens, W, mem_k, mem_v, Z)
    for mode in modes_of(n, dh):
        res = sink_lib(q, k, v, lens, do, dh ** -0.5, 0., W, mode, mem_k, mem_v, Z)
        for name, t in res.items():
            assert torch.isfinite(t).all(), (mode, name)
        assert res['dk'].shape == (b, Hkv, n, dh) and (M == 0 or res['dmk'].shape == (Hkv, M, dh))
        check_ref(res, ref)
        if W is not None:
            dead = ~visible(n, lens, W).any(-1)[:, 0]   # [b][n]: rows without a visible real key
            assert dead[b - 1, 1 + W:].all() and not dead[0].any()
            if M == 0:
                assert (res['o'].transpose(1, 2)[dead] == 0).all(), mode
            do2 = do.clone()
            do2.transpose(1, 2)[dead] = torch.randn(int(dead.sum()), H, dh, device=DEV)
            res2 = sink_lib(q, k, v, lens, do2, dh ** -0.5, 0., W, mode, mem_k, mem_v, Z)
            assert torch.equal(res2['dk'], res['dk']) and torch.equal(res2['dv'], res['dv']), mode


@pytest.mark.parametrize('W', [None, 10])
@pytest.mark.parametrize('n', [70, 130])
@pytest.mark.parametrize('p', [0., 0.25])
def test_sink_entry_points_without_sinks_are_the_gqa_ones(p, n, W):
    """M = 0, Z = 0 through the _sink entry points: o, lse, D, dq, dk, dv bit-identical to the _gqa entry
    points in every backward mode, at Hkv = H and Hkv < H."""
    b, H, dh = 2, 4, 16
    for Hkv in (4, 2):
        q, k, v, do, lens = gqa_problem(b, H, Hkv, n, dh, n + 3)
        for mode in modes_of(n, dh):
            old = gqa_lib(q, k, v, lens, do, dh ** -0.5, p, W, mode)
            new = sink_lib(q, k, v, lens, do, dh ** -0.5, p, W, mode, None, None, 0)
            for name in NAMES:
                assert torch.equal(old[name], new[name]), (Hkv, mode, name)


@pytest.mark.parametrize('Hkv,n,dh,W', [(2, 70, 16, None), (1, 130, 16, 10), (4, 300, 16, 64), (2, 64, 32, 7)])
@pytest.mark.parametrize('p', [0., 0.25])
def test_sink_backward_repeats_bit_for_bit(p, Hkv, n, dh, W):
    """Each backward mode run twice (M = 3, Z = 1) gives identical bits in dmem_k / dmem_v — and in every
    other output: the row, head and episode sums have a fixed order.  n = 300: more than one row chunk of
    the sink backward."""
    b, H = 3, 4
    q, k, v, do, lens, mem_k, mem_v = sink_problem(b, H, Hkv, n, dh, 3, n + Hkv)
    for mode in modes_of(n, dh):
        one = sink_lib(q, k, v, lens, do, dh ** -0.5, p, W, mode, mem_k, mem_v, 1)
        two = sink_lib(q, k, v, lens, do, dh ** -0.5, p, W, mode, mem_k, mem_v, 1)
        for name in one:
            assert torch.equal(one[name], two[name]), (mode, name)


@pytest.mark.parametrize('p', [0.25, 0.3])
@pytest.mark.parametrize('Hkv,n,W', [(2, 130, None), (1, 70, 10)])
def test_sink_dropout_against_host_keep_bits(p, Hkv, n, W):
    """Dropout with M = 3, Z = 1 (p = 0.25: byte-mode real keys; 0.3: word mode): forward and all gradients
    of ops.attention against the fp64 reference times the host keep bits — the real columns' from
    oracle.philox.attn_dropout_keep, exactly the mask of a run without sinks, the sink columns' from
    test_attn_sink_cpu.sink_dropout_keep."""
    from xtrl_amd import ops
    b, H, dh, M = 2, 4, 16, 3
    g = torch.Generator().manual_seed(11 + n)
    q, do = (torch.randn(b, H, n, dh, generator=g) for _ in range(2))
    k, v = (torch.randn(b, Hkv, n, dh, generator=g) for _ in range(2))
    mem_k, mem_v = (torch.randn(Hkv, M, dh, generator=g) for _ in range(2))
    lens = torch.tensor([n, 45], dtype=torch.int32)
    seed, offset, layer = 1234567, 5, 3
    keep = torch.from_numpy(P.attn_dropout_keep(b, H, n, p, seed, offset, layer)).double() / (1 - p)
    keep_mem = torch.from_numpy(sink_dropout_keep(b, H, n, M, p, seed, offset, layer)).double() / (1 - p)
    ref = sink_ref(q, k, v, do, lens, W, mem_k, mem_v, 1, keep, keep_mem)
    leaves = [t.to(DEV).requires_grad_() for t in (q, k, v, mem_k, mem_v)]
    out = ops.attention(*leaves[:3], lens.to(DEV), dh ** -0.5, p, seed=seed, offset=offset, sub=layer, window=W or 0,
                        mem_k=leaves[3], mem_v=leaves[4], add_zero_kv=True)
    (out * do.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    tol(out, ref['o'], 1e-5, 1e-5)
    for t, name in zip(leaves, ('dq', 'dk', 'dv', 'dmk', 'dmv')):
        assert t.grad.shape == ref[name].shape
        tol(t.grad, ref[name], 1e-4, 1e-5)


@pytest.mark.parametrize('p', [0.25, 0.3])
def test_sink_real_key_keep_bits_equal_a_run_without_sinks(p):
    """The real keys' keep bits, read off the device: with v = I (n = dh = 64) o[i][j] = keep_ij P_ij / (1 - p),
    so o != 0 is the keep mask on the visible keys.  With M = 3 (mem_v = 0, so the sinks add nothing to o)
    and Z = 1 it is the mask of the run without sinks, which is oracle.philox.attn_dropout_keep."""
    b, H, n, dh = 2, 2, 64, 64
    g = torch.Generator().manual_seed(4)
    q, k, do = (torch.randn(b, H, n, dh, generator=g).to(DEV) for _ in range(3))
    v = torch.eye(n, device=DEV).expand(b, H, n, n).contiguous()
    mem_k = torch.randn(H, 3, dh, generator=g).to(DEV)
    lens = torch.tensor([64, 40], dtype=torch.int32, device=DEV)
    plain = sink_lib(q, k, v, lens, do, dh ** -0.5, p, None, 'two', None, None, 0, seed=77, offset=2, sub=1)['o'] != 0
    sinks = sink_lib(q, k, v, lens, do, dh ** -0.5, p, None, 'two', mem_k, torch.zeros_like(mem_k), 1, seed=77, offset=2,
                     sub=1)['o'] != 0
    host = torch.from_numpy(P.attn_dropout_keep(b, H, n, p, 77, 2, 1)) & visible(n, lens.cpu(), None)
    assert torch.equal(plain.cpu(), host) and torch.equal(sinks.cpu(), host)
    assert 0.6 < float(host.sum()) / float(visible(n, lens.cpu(), None).expand(b, H, n, n).sum()) < 0.85


# ----------------------------------------------------------------------------------------------
# model level: the sink oracle (test_attn_sink_cpu.sink_init / sink_forward over the frozen Attention)
# ----------------------------------------------------------------------------------------------

CONFIGS = {'mem2+zero': (2, True), 'zero': (0, True)}   # (M, Z); both with W = 5 and kv_heads = 2
# the same three tests (rollout + learn, packed learn, fused vs autograd) at dh != 16: (M, Z, make_sink_learner
# keywords) — k_attn_decode<32|64, 0, true>, k_decode_row<32|64, ., true> and the learn step's sink kernels
GEOM_CONFIGS = {'h4x32_gqa2_mem3+zero': (3, True, dict(heads=4, dim_head=32, Hkv=2, dim=64)),
                'h2x64_kv1_zero': (0, True, dict(heads=2, dim_head=64, Hkv=1, dim=48))}
ALL_CONFIGS = list(CONFIGS) + list(GEOM_CONFIGS)


def config(cfg):
    """(M, Z, make_sink_learner keywords) of a CONFIGS or GEOM_CONFIGS entry."""
    return (*CONFIGS[cfg], {}) if cfg in CONFIGS else GEOM_CONFIGS[cfg]


def make_sink_learner(M, Z, W=5, Hkv=2, depth=2, gates=True, T=24, episodes=6, batch=3, seed=3, hazard=4, mode='lander',
                      dim=48, agent_extra=None, with_oracle=True, heads=4, dim_head=16):
    """Learner with world_model attn_num_mem_kv = M, attn_add_zero_kv = Z, attn_max_attend_past = W and
    agent_kwargs kv_heads = Hkv (``heads`` x ``dim_head``, 4 x 16 by default), the device Sim and the oracle on the same weights
    (test_attn_gqa_gpu.make_gqa_learner's construction; the oracle takes the sinks, GQA and the window from
    the patched Attention, which the caller installs first).  The Sim's terminations depend on the seed
    alone: seed 3 at hazard 2^-4 gives the lengths 22, 24, 4, 12, 24, 21 in the minibatches (24, 21, 4) and
    (12, 24, 22) — a full episode, and in both minibatches padded rows past the band of W = 5."""
    from xtrl_amd import Learner, SynthVecSim
    S, A = 8, 4
    torch.manual_seed(seed)
    wm = dict(attn_dim_head=dim_head, heads=heads, depth=depth, attn_num_mem_kv=M, attn_add_zero_kv=Z)
    if gates:
        wm.update(attn_gate_values=True, add_value_residual=True, learned_value_residual_mix=True)
    if W is not None:
        wm['attn_max_attend_past'] = W
    gp = dict(dim=8, num_genes_per_island=3, num_selected=2, tournament_size=2)
    learner = Learner(state_dim=S, num_actions=A, reward_range=(-2., 2.), world_model=wm, max_timesteps=T,
                      batch_size=batch, num_episodes_per_update=episodes, evolutionary=False, latent_gene_pool=gp,
                      agent_kwargs=dict(dropout=0., seed=seed, hidden_dim=dim, reward_dropout=0.5, kv_heads=Hkv,
                                        **(agent_extra or {})), use_graph=False)
    with torch.no_grad():   # non-trivial gate / mix weights (their init is constant)
        g = torch.Generator().manual_seed(seed + 1)
        for name, p in learner.agent.model.named_parameters():
            if 'to_v_gate' in name or 'to_value_residual_mix' in name:
                p.copy_((torch.randn(p.shape, generator=g) * 0.3).to(p.device))
        learner.agent.ema_flat.copy_(learner.agent.flat.flat)
    env = SynthVecSim(S, A, mode, hazard_log2=hazard)
    if not with_oracle:
        return learner, env, None
    c = R.LearnerConfig(S, A, (-2., 2.), dim=dim, depth=depth, heads=heads, dim_head=dim_head, gate_values=gates,
                        value_residual=gates, learned_mix=gates, max_timesteps=T, batch_size=batch, num_episodes_per_update=episodes,
                        sim_mode=mode, hazard_log2=hazard, seed=seed, reward_dropout=0.5, gene_pool=gp)
    sd = {k: v.detach().cpu() for k, v in learner.agent.model.state_dict().items()}
    oracle = R.OracleLearner(c, init_state_dict=sd)
    return learner, env, oracle


def install_sink_oracle(monkeypatch, M, Z, W=5, Hkv=2):
    monkeypatch.setattr(tp.Attention, '__init__', sink_init(Hkv, M))
    monkeypatch.setattr(tp.Attention, 'forward', sink_forward(W, Z))


def sink_rollout_and_learn(monkeypatch, M, Z, T, minibatches, packed=False, **kw):
    """Rollout (G.compare_rollout: actions, lengths, rewards bit-exact; log-probs and logits within 1e-4) and
    ``minibatches`` learn minibatches (G._learn_parity: loss within 1e-4 relative, every gradient — mem_k /
    mem_v among them — within 1e-4 of the gradient scale) against the sink oracle.  ``packed``: the packed
    learn step (per-token critic reduction on both sides)."""
    Hkv, dh = kw.get('Hkv', 2), kw.get('dim_head', 16)
    install_sink_oracle(monkeypatch, M, Z, Hkv=Hkv)
    extra = dict(hl_reduction_mean=False, packed_learn=True) if packed else None
    learner, env, oracle = make_sink_learner(M, Z, T=T, agent_extra=extra, **kw)
    cfg = learner.agent.cfg
    assert (cfg.num_mem_kv, cfg.add_zero_kv, cfg.attn_window, cfg.kv_heads, cfg.dim_head) == (M, Z, 5, Hkv, dh)
    traj, lens, genes, cum = learner.rollout_device(env, 0, T)
    torch.cuda.synchronize()
    eng = learner._engine_for(env, T)
    for kc, vc in eng.kv:   # the sinks are not cached
        assert kc.shape == vc.shape == (eng.E, Hkv, T, dh)
    episodes, _ = oracle.rollout(0)
    G.compare_rollout(traj, lens, episodes)
    seen = []
    if minibatches:
        names = [n for n, _ in oracle.model.named_parameters()]
        assert sum(n.endswith(('.1.mem_k', '.1.mem_v')) for n in names) == (4 if M else 0)   # (depth 2)
        with G._hl_reduction(not packed):
            seen = G._learn_parity(learner, oracle, traj, lens, genes, learner.fitness(cum, genes), minibatches,
                                   packed=packed)
        if M:   # the memory rows really take gradient
            for n, (lo, hi) in learner.agent.flat.index.items():
                if n.endswith(('.mem_k', '.mem_v')):
                    assert float(learner.agent.flat.grad[lo:hi].abs().max()) > 0, n
    return learner, lens, seen


@pytest.mark.parametrize('rows', ['1', '0'])
@pytest.mark.parametrize('cfg', ALL_CONFIGS)
def test_sink_rollout_and_learn_match_oracle(cfg, rows, monkeypatch):
    """H = 4, kv_heads 2, W = 5, d = 48, depth 2 with gates and the learned mix, T = 24: both decode paths (the
    row-resident step and the multi-kernel step), then two padded learn minibatches, whose padded rows past
    the band attend the sinks alone.  GEOM_CONFIGS: the same at 4 x 32 heads (kv_heads 2, M = 3, d = 64) and at
    2 x 64 heads (one kv head, the zero key alone, d = 48)."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', rows)
    M, Z, kw = config(cfg)
    learner, lens, seen = sink_rollout_and_learn(monkeypatch, M, Z, 24, 2, **kw)
    assert (learner._engine[1].rows_max > 0) == (rows == '1')
    assert int(lens.max()) > 10 and len(seen) == 2
    assert int(lens.min()) + 5 < max(s[0] for s in seen)   # an episode with rows past its band


@pytest.mark.parametrize('cfg', ALL_CONFIGS)
def test_sink_packed_learn_matches_oracle(cfg, monkeypatch):
    """The packed learn step (hl_reduction_mean=False, packed_learn=True) against the sink oracle: the row
    sums of dmem_k / dmem_v run over the valid rows."""
    M, Z, kw = config(cfg)
    learner, _, seen = sink_rollout_and_learn(monkeypatch, M, Z, 24, 2, packed=True, **kw)
    assert learner.agent.packed_learn and len(seen) == 2


def test_sink_d256_fused_out_projection_rollout(monkeypatch):
    """d = 256, T = 40, M = 2 + Z: the attention decode kernel that applies the out-projection itself."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', '0')
    _, lens, _ = sink_rollout_and_learn(monkeypatch, 2, True, 40, 0, dim=256)
    assert int(lens.max()) > 7


@pytest.mark.parametrize('cfg', list(CONFIGS))
def test_sink_deploy_forward_matches_oracle_cached_decode(cfg, monkeypatch):
    """Agent.forward over 10 steps (W = 5: the window moves past the first keys) against the sink oracle's
    cached decode; the hiddens' cache tensors hold the real keys only."""
    M, Z = CONFIGS[cfg]
    install_sink_oracle(monkeypatch, M, Z)
    learner, env, oracle = make_sink_learner(M, Z, T=24)
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
    assert kv and all(x.shape[1] == 2 and x.shape[3] == 16 for x in kv)


@pytest.mark.parametrize('p', [0., 0.25])
@pytest.mark.parametrize('cfg', ALL_CONFIGS)
def test_sink_fused_step_matches_reference_mode_autograd(cfg, p):
    """The hand-scheduled learn step against the reference-mode autograd step (model.forward_train with
    ops.attention taking the sinks) with gates, W = 5, kv_heads 2, T = 24: the bounds of
    test_fused_train_step_matches_autograd, mem_k / mem_v among the gradients."""
    M, Z, kw = config(cfg)
    learner, env, _ = make_sink_learner(M, Z, T=24, episodes=8, batch=4, seed=9, with_oracle=False, **{'dim': 64, **kw})
    agent = learner.agent
    agent.cfg.dropout = p
    agent.model.cfg.dropout = p
    traj, lens, genes, cum = learner.rollout_device(env, 0, 24)
    fit = learner.fitness(cum, genes)
    agent.fused_learn = True
    a = G._first_minibatch(agent, traj, lens, genes, fit)
    agent.fused_learn = False
    b = G._first_minibatch(agent, traj, lens, genes, fit)
    assert abs(a['loss'] - b['loss']) <= 1e-5 * abs(b['loss']) + 1e-6, (a['loss'], b['loss'])
    scale = float(b['grad'].abs().max())
    names = list(agent.flat.index)
    assert M == 0 or sum(n.endswith(('.mem_k', '.mem_v')) for n in names) == 4
    for name, (s, e) in agent.flat.index.items():
        err = float((a['grad'][s:e] - b['grad'][s:e]).abs().max())
        assert err <= 1e-4 * scale + 1e-7, (name, err, scale)
