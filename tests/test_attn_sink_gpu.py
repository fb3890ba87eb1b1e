"""Attention sinks (world_model['attn_num_mem_kv'] = M memory key / value rows per kv head,
world_model['attn_add_zero_kv'] = Z one all-zero key / value) on the MI355X: the learn-step kernels through
the xtrl_attn_*_sink entry points and ops.attention against the fp64 dense reference of
test_attn_sink_cpu.attn_sink_ref (with the window, GQA and every backward mode), against the _gqa entry
points without sinks, run to run, and with dropout against the host keep bits
(oracle.philox.attn_dropout_keep for the real columns, test_attn_sink_cpu.sink_dropout_keep for the sink
columns); then the rollout, the padded and the packed learn step, the deploy forward and the reference-mode
autograd step against the sink oracle (test_attn_sink_cpu.sink_init / sink_forward installed over the
frozen oracle's Attention)."""
import functools

import pytest
import torch

from oracle import philox as P
from oracle import thirdparty as tp

import attn_harness as AH
import test_gpu_parity as G
from attn_harness import NAMES, check_ref, modes_of, problem
from test_attn_sink_cpu import attn_sink_ref, sink_dropout_keep, sink_forward, sink_init, visible

pytestmark = pytest.mark.gpu
DEV = 'cuda'
gqa_lib = functools.partial(AH.attn_lib, abi='gqa')
sink_lib = functools.partial(AH.attn_lib, abi='sink')   # mem_k None: M = 0 (null sink pointers)
sink_ref = functools.partial(AH.fp64_ref, attn_sink_ref)   # extra = ()
SHAPES = [(3, 4, 4, 37, 16, None), (2, 4, 2, 70, 16, None), (2, 4, 2, 130, 16, 10), (2, 4, 1, 200, 16, 64),
          (2, 6, 2, 64, 32, 7), (1, 4, 2, 70, 64, None)]
SINKS = [(0, 1), (1, 0), (3, 1), (16, 0)]


# ----------------------------------------------------------------------------------------------
# kernel level
# ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('M,Z', SINKS)
@pytest.mark.parametrize('b,H,Hkv,n,dh,W', SHAPES)
def test_sink_forward_and_backward_against_fp64(b, H, Hkv, n, dh, W, M, Z):
    """Forward + every backward mode of the shape at p = 0 against the fp64 reference, ragged lengths (one
    full episode, one of a single step), every output NaN-filled before and finite after.  Under a window
    the single-step episode has padded rows past the band (i >= 1 + W): they attend the sinks alone — with
    the zero key only their o is exactly 0 — and whatever their dO, they add nothing to dK / dV."""
    q, k, v, do, lens, *mem = problem(b, H, n, dh, n + dh + Hkv + (W or 0) + M, Hkv=Hkv, M=M)
    mem_k, mem_v = mem or (None, None)
    ref = sink_ref(q, k, v, do, lens, W, (), mem_k, mem_v, Z)
    for mode in modes_of(n, dh):
        res = sink_lib(q, k, v, lens, do, dh ** -0.5, 0., mode, W=W, mem_k=mem_k, mem_v=mem_v, Z=Z)
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
            res2 = sink_lib(q, k, v, lens, do2, dh ** -0.5, 0., mode, W=W, mem_k=mem_k, mem_v=mem_v, Z=Z)
            assert torch.equal(res2['dk'], res['dk']) and torch.equal(res2['dv'], res['dv']), mode


@pytest.mark.parametrize('W', [None, 10])
@pytest.mark.parametrize('n', [70, 130])
@pytest.mark.parametrize('p', [0., 0.25])
def test_sink_entry_points_without_sinks_are_the_gqa_ones(p, n, W):
    """M = 0, Z = 0 through the _sink entry points: o, lse, D, dq, dk, dv bit-identical to the _gqa entry
    points in every backward mode, at Hkv = H and Hkv < H."""
    b, H, dh = 2, 4, 16
    for Hkv in (4, 2):
        q, k, v, do, lens = problem(b, H, n, dh, n + 3, Hkv=Hkv)
        for mode in modes_of(n, dh):
            old = gqa_lib(q, k, v, lens, do, dh ** -0.5, p, mode, W=W)
            new = sink_lib(q, k, v, lens, do, dh ** -0.5, p, mode, W=W)
            for name in NAMES:
                assert torch.equal(old[name], new[name]), (Hkv, mode, name)


@pytest.mark.parametrize('Hkv,n,dh,W', [(2, 70, 16, None), (1, 130, 16, 10), (4, 300, 16, 64), (2, 64, 32, 7)])
@pytest.mark.parametrize('p', [0., 0.25])
def test_sink_backward_repeats_bit_for_bit(p, Hkv, n, dh, W):
    """Each backward mode run twice (M = 3, Z = 1) gives identical bits in dmem_k / dmem_v — and in every
    other output: the row, head and episode sums have a fixed order.  n = 300: more than one row chunk of
    the sink backward."""
    b, H = 3, 4
    q, k, v, do, lens, mem_k, mem_v = problem(b, H, n, dh, n + Hkv, Hkv=Hkv, M=3)
    for mode in modes_of(n, dh):
        one = sink_lib(q, k, v, lens, do, dh ** -0.5, p, mode, W=W, mem_k=mem_k, mem_v=mem_v, Z=1)
        two = sink_lib(q, k, v, lens, do, dh ** -0.5, p, mode, W=W, mem_k=mem_k, mem_v=mem_v, Z=1)
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
    ref = sink_ref(q, k, v, do, lens, W, (), mem_k, mem_v, 1, keep, keep_mem)
    leaves = [t.to(DEV).requires_grad_() for t in (q, k, v, mem_k, mem_v)]
    out = ops.attention(*leaves[:3], lens.to(DEV), dh ** -0.5, p, seed=seed, offset=offset, sub=layer, window=W or 0,
                        mem_k=leaves[3], mem_v=leaves[4], add_zero_kv=True)
    (out * do.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    del ref['lse']   # (ops.attention returns none)
    res = dict(o=out)
    for t, name in zip(leaves, ('dq', 'dk', 'dv', 'dmk', 'dmv')):
        assert t.grad.shape == ref[name].shape
        res[name] = t.grad
    check_ref(res, ref)


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
    plain = sink_lib(q, k, v, lens, do, dh ** -0.5, p, 'two', seed=77, offset=2, sub=1)['o'] != 0
    sinks = sink_lib(q, k, v, lens, do, dh ** -0.5, p, 'two', mem_k=mem_k, mem_v=torch.zeros_like(mem_k), Z=1, seed=77,
                     offset=2, sub=1)['o'] != 0
    host = torch.from_numpy(P.attn_dropout_keep(b, H, n, p, 77, 2, 1)) & visible(n, lens.cpu(), None)
    assert torch.equal(plain.cpu(), host) and torch.equal(sinks.cpu(), host)
    assert 0.6 < float(host.sum()) / float(visible(n, lens.cpu(), None).expand(b, H, n, n).sum()) < 0.85


# ----------------------------------------------------------------------------------------------
# model level: the sink oracle (test_attn_sink_cpu.sink_init / sink_forward over the frozen Attention)
# ----------------------------------------------------------------------------------------------

CONFIGS = {'mem2+zero': (2, True), 'zero': (0, True)}   # (M, Z); both with W = 5 and kv_heads = 2
# the same three tests (rollout + learn, packed learn, fused vs autograd) at dh != 16: (M, Z, sink_kw
# keywords) — k_attn_decode<32|64, 0, true>, k_decode_row<32|64, ., true> and the learn step's sink kernels
GEOM_CONFIGS = {'h4x32_gqa2_mem3+zero': (3, True, dict(heads=4, dim_head=32, Hkv=2, dim=64)),
                'h2x64_kv1_zero': (0, True, dict(heads=2, dim_head=64, Hkv=1, dim=48))}
ALL_CONFIGS = list(CONFIGS) + list(GEOM_CONFIGS)


def config(cfg):
    """(M, Z, sink_kw keywords) of a CONFIGS or GEOM_CONFIGS entry."""
    return (*CONFIGS[cfg], {}) if cfg in CONFIGS else GEOM_CONFIGS[cfg]


LEARNER = dict(episodes=6, batch=3, hazard=4)   # this file's G.make_learner defaults, with T = 24


def sink_kw(M, Z, Hkv=2, **kw):
    """G.make_learner's keywords for attn_num_mem_kv = M, attn_add_zero_kv = Z, attn_max_attend_past = 5 and
    kv_heads = Hkv — through agent_kwargs whatever the count, 1 too — plus ``kw`` (heads, dim_head, dim, ...).
    The Sim's terminations depend on the seed alone: seed 3 at hazard 2^-4 (LEARNER) gives the lengths 22, 24, 4,
    12, 24, 21 in the minibatches (24, 21, 4) and (12, 24, 22) — a full episode, and in both minibatches padded
    rows past the band of W = 5."""
    return dict(window=5, num_mem_kv=M, add_zero_kv=Z, agent_extra=dict(kv_heads=Hkv), **kw)


def install_sink_oracle(monkeypatch, M, Z, W=5, Hkv=2):
    monkeypatch.setattr(tp.Attention, '__init__', sink_init(Hkv, M))
    monkeypatch.setattr(tp.Attention, 'forward', sink_forward(W, Z))


def sink_rollout_and_learn(monkeypatch, M, Z, T, minibatches, packed=False, Hkv=2, dim_head=16, **kw):
    """attn_harness.rollout_and_learn against the sink oracle (every gradient: mem_k / mem_v among them).  The
    engine caches the real keys only, the oracle has the memory rows, and they really take gradient."""
    def checks(learner, env, oracle):
        cfg = learner.agent.cfg
        assert (cfg.num_mem_kv, cfg.add_zero_kv, cfg.attn_window, cfg.kv_heads, cfg.dim_head) == (M, Z, 5, Hkv, dim_head)
        eng = learner._engine_for(env, T)
        for kc, vc in eng.kv:   # the sinks are not cached
            assert kc.shape == vc.shape == (eng.E, Hkv, T, dim_head)
        names = [n for n, _ in oracle.model.named_parameters()]
        assert sum(n.endswith(('.1.mem_k', '.1.mem_v')) for n in names) == (4 if M else 0)   # (depth 2)

    learner, lens, seen = AH.rollout_and_learn(monkeypatch, lambda mp: install_sink_oracle(mp, M, Z, Hkv=Hkv), T,
                                               minibatches, packed, checks, **LEARNER,
                                               **sink_kw(M, Z, Hkv, dim_head=dim_head, **kw))
    if M and minibatches:   # the memory rows really take gradient
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


@pytest.mark.parametrize('dim', [256, 384])
def test_sink_fused_out_projection_rollout(dim, monkeypatch):
    """d = 256 and d = 384 (the FJ = 1 and FJ = 2 forms), T = 40, M = 2 + Z: the attention decode kernel that
    applies the out-projection itself."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', '0')
    _, lens, _ = sink_rollout_and_learn(monkeypatch, 2, True, 40, 0, dim=dim)
    assert int(lens.max()) > 7


@pytest.mark.parametrize('cfg', list(CONFIGS))
def test_sink_deploy_forward_matches_oracle_cached_decode(cfg, monkeypatch):
    """Agent.forward over 10 steps (W = 5: the window moves past the first keys) against the sink oracle's
    cached decode; the hiddens' cache tensors hold the real keys only."""
    M, Z = CONFIGS[cfg]
    install_sink_oracle(monkeypatch, M, Z)
    learner, env, oracle = G.make_learner(T=24, **LEARNER, **sink_kw(M, Z))
    hiddens = G.deploy_parity(learner, oracle, 10)
    kv = [x for x in hiddens['cache'] if x.dim() == 4]
    assert kv and all(x.shape[1] == 2 and x.shape[3] == 16 for x in kv)


@pytest.mark.parametrize('p', [0., 0.25])
@pytest.mark.parametrize('cfg', ALL_CONFIGS)
def test_sink_fused_step_matches_reference_mode_autograd(cfg, p):
    """The hand-scheduled learn step against the reference-mode autograd step (model.forward_train with
    ops.attention taking the sinks) with gates, W = 5, kv_heads 2, T = 24: the bounds of
    test_fused_train_step_matches_autograd, mem_k / mem_v among the gradients."""
    M, Z, kw = config(cfg)

    def checks(learner, env, oracle):
        names = list(learner.agent.flat.index)
        assert M == 0 or sum(n.endswith(('.mem_k', '.mem_v')) for n in names) == 4

    opts = sink_kw(M, Z, **{'dim': 64, **kw})
    G._fused_vs_autograd(False, False, True, p, 24, depth=2, episodes=8, batch=4, hazard=4, dim=opts.pop('dim'),
                         checks=checks, with_oracle=False, **opts)
