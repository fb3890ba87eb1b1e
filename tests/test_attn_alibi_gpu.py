"""ALiBi (world_model['alibi_pos_bias'] / ['alibi_num_heads']) on the MI355X: the learn-step kernels through
the xtrl_attn_*_alibi entry points and ops.attention against the fp64 dense reference of
test_attn_alibi_cpu.attn_alibi_ref (with the window, GQA, the sinks and every backward mode), against the
_sink entry points with a NULL slopes pointer, run to run, with dropout against the host keep bits and on
the dead rows of a window; then the rollout (both decode paths, the second 128-key chunk, a moving window,
the fused out-projection form), the padded and the packed learn step, the deploy forward and the
reference-mode autograd step against the ALiBi oracle (test_attn_alibi_cpu.alibi_forward installed over the
frozen oracle's Attention)."""
import functools

import pytest
import torch

from oracle import philox as P

import attn_harness as AH
import test_gpu_parity as G
from attn_harness import NAMES, check_ref, modes_of, problem
from test_attn_alibi_cpu import attn_alibi_ref, install_alibi
from test_attn_sink_cpu import sink_dropout_keep

pytestmark = pytest.mark.gpu
DEV = 'cuda'
sink_lib = functools.partial(AH.attn_lib, abi='sink')
alibi_lib = functools.partial(AH.attn_lib, abi='alibi')   # slopes=None: a NULL slopes pointer
alibi_ref = functools.partial(AH.fp64_ref, attn_alibi_ref)   # extra = (slopes,)
SHAPES = [(3, 4, 4, 37, 16, None), (2, 4, 2, 70, 16, None), (2, 4, 2, 130, 16, 10), (2, 4, 1, 200, 16, 64),
          (2, 6, 2, 64, 32, 7), (1, 4, 2, 70, 64, None)]
SINKS = [(0, 0), (0, 1), (3, 1)]


# ----------------------------------------------------------------------------------------------
# kernel level
# ----------------------------------------------------------------------------------------------


def dev_slopes(H, A=None):
    from xtrl_amd import ops
    return ops.alibi_slopes(H, A).to(DEV)


@pytest.mark.parametrize('M,Z', SINKS)
@pytest.mark.parametrize('b,H,Hkv,n,dh,W', SHAPES)
def test_alibi_forward_and_backward_against_fp64(b, H, Hkv, n, dh, W, M, Z):
    """Forward + every backward mode of the shape at p = 0 against the fp64 reference (check_ref's bounds: o, lse
    1e-5 + 1e-5, gradients 1e-4 + 1e-5), ragged lengths (one full episode, one of a single step), every output
    NaN-filled before and finite after.  n = 70: a bias taken from the tile-relative column would be wrong past
    the first 64-key tile; n = 200, W = 64: the band's first tile is not tile 0; H = 6: the non-power-of-two
    slopes."""
    q, k, v, do, lens, *mem = problem(b, H, n, dh, n + dh + Hkv + (W or 0) + M, Hkv=Hkv, M=M)
    mem_k, mem_v = mem or (None, None)
    slopes = dev_slopes(H)
    ref = alibi_ref(q, k, v, do, lens, W, (slopes,), mem_k, mem_v, Z)
    for mode in modes_of(n, dh):
        res = alibi_lib(q, k, v, lens, do, dh ** -0.5, 0., mode, slopes=slopes, W=W, mem_k=mem_k, mem_v=mem_v, Z=Z)
        for name, t in res.items():
            assert torch.isfinite(t).all(), (mode, name)
        assert res['dk'].shape == (b, Hkv, n, dh) and (M == 0 or res['dmk'].shape == (Hkv, M, dh))
        check_ref(res, ref)


@pytest.mark.parametrize('M,Z', [(0, 0), (3, 1)])
def test_alibi_num_heads_leaves_the_other_heads_without_bias(M, Z):
    """alibi_num_heads = 2 of 4 (slopes 2^-4, 2^-8, 0, 0) at n = 130, W = 10, Hkv = 2: the whole result against the
    fp64 reference, and heads 2 and 3 — slope 0 — against the reference WITHOUT any bias."""
    b, H, Hkv, n, dh, W = 2, 4, 2, 130, 16, 10
    q, k, v, do, lens, *mem = problem(b, H, n, dh, 77 + M, Hkv=Hkv, M=M)
    mem_k, mem_v = mem or (None, None)
    slopes = dev_slopes(H, 2)
    assert slopes.tolist() == [2. ** -4, 2. ** -8, 0., 0.]
    ref = alibi_ref(q, k, v, do, lens, W, (slopes,), mem_k, mem_v, Z)
    plain = alibi_ref(q, k, v, do, lens, W, (torch.zeros(H),), mem_k, mem_v, Z)
    assert not torch.allclose(ref['o'][:, :2], plain['o'][:, :2], atol=1e-3)
    for mode in modes_of(n, dh):
        res = alibi_lib(q, k, v, lens, do, dh ** -0.5, 0., mode, slopes=slopes, W=W, mem_k=mem_k, mem_v=mem_v, Z=Z)
        check_ref(res, ref)
        G.tol(res['o'][:, 2:], plain['o'][:, 2:], 1e-5, 1e-5)
        G.tol(res['lse'][:, 2:], plain['lse'][:, 2:], 1e-5, 1e-5)
        G.tol(res['dq'][:, 2:], plain['dq'][:, 2:], 1e-4, 1e-5)


@pytest.mark.parametrize('W', [None, 10])
@pytest.mark.parametrize('n', [70, 130])
@pytest.mark.parametrize('p', [0., 0.25])
def test_alibi_entry_points_with_null_slopes_are_the_sink_ones(p, n, W):
    """A NULL slopes pointer through the _alibi entry points: o, lse, D, dq, dk, dv (and dmk, dmv with M = 3,
    Z = 1) bit-identical to the _sink entry points in every backward mode, at Hkv = H and Hkv < H."""
    b, H, dh = 2, 4, 16
    for Hkv, M in ((4, 0), (2, 0), (2, 3)):
        q, k, v, do, lens, *mem = problem(b, H, n, dh, n + 3, Hkv=Hkv, M=M)
        kw = dict(W=W, mem_k=mem[0], mem_v=mem[1], Z=1) if M else dict(W=W)
        for mode in modes_of(n, dh):
            old = sink_lib(q, k, v, lens, do, dh ** -0.5, p, mode, **kw)
            new = alibi_lib(q, k, v, lens, do, dh ** -0.5, p, mode, **kw)
            assert set(old) == set(new) and set(new) >= set(NAMES)
            for name in old:
                assert torch.equal(old[name], new[name]), (Hkv, M, mode, name)


@pytest.mark.parametrize('Hkv,n,W', [(4, 300, 64), (2, 70, None)])
@pytest.mark.parametrize('p', [0., 0.25])
def test_alibi_backward_repeats_bit_for_bit(p, Hkv, n, W):
    """Each backward mode run twice gives identical bits in every output (M = 3, Z = 1 along)."""
    b, H, dh = 3, 4, 16
    q, k, v, do, lens, mem_k, mem_v = problem(b, H, n, dh, n + Hkv, Hkv=Hkv, M=3)
    slopes = dev_slopes(H)
    for mode in modes_of(n, dh):
        one = alibi_lib(q, k, v, lens, do, dh ** -0.5, p, mode, slopes=slopes, W=W, mem_k=mem_k, mem_v=mem_v, Z=1)
        two = alibi_lib(q, k, v, lens, do, dh ** -0.5, p, mode, slopes=slopes, W=W, mem_k=mem_k, mem_v=mem_v, Z=1)
        for name in one:
            assert torch.isfinite(one[name]).all() and torch.equal(one[name], two[name]), (mode, name)


@pytest.mark.parametrize('p', [0.25, 0.3])
@pytest.mark.parametrize('Hkv,n,W,M', [(2, 130, None, 0), (1, 70, 10, 3)])
def test_alibi_dropout_against_host_keep_bits(p, Hkv, n, W, M):
    """Dropout (p = 0.25: byte-mode real keys; 0.3: word mode): forward and all gradients of ops.attention with
    slopes against the fp64 reference times the host keep bits — oracle.philox.attn_dropout_keep for the real
    columns, exactly the mask of a run without ALiBi, and test_attn_sink_cpu.sink_dropout_keep for the memory
    columns (M = 3 with the zero key; M = 0: no sink, every row of both episodes sees a key)."""
    from xtrl_amd import ops
    b, H, dh = 2, 4, 16
    g = torch.Generator().manual_seed(11 + n)
    q, do = (torch.randn(b, H, n, dh, generator=g) for _ in range(2))
    k, v = (torch.randn(b, Hkv, n, dh, generator=g) for _ in range(2))
    mem_k, mem_v = (torch.randn(Hkv, M, dh, generator=g) for _ in range(2)) if M else (None, None)
    lens = torch.tensor([n, 45], dtype=torch.int32)
    seed, offset, layer = 1234567, 5, 3
    slopes = ops.alibi_slopes(H)
    keep = torch.from_numpy(P.attn_dropout_keep(b, H, n, p, seed, offset, layer)).double() / (1 - p)
    keep_mem = torch.from_numpy(sink_dropout_keep(b, H, n, M, p, seed, offset, layer)).double() / (1 - p) if M else None
    ref = alibi_ref(q, k, v, do, lens, W, (slopes,), mem_k, mem_v, bool(M), keep, keep_mem)
    names = ('dq', 'dk', 'dv') + (('dmk', 'dmv') if M else ())
    leaves = [t.to(DEV).requires_grad_() for t in ((q, k, v, mem_k, mem_v) if M else (q, k, v))]
    out = ops.attention(*leaves[:3], lens.to(DEV), dh ** -0.5, p, seed=seed, offset=offset, sub=layer, window=W or 0,
                        mem_k=leaves[3] if M else None, mem_v=leaves[4] if M else None, add_zero_kv=bool(M),
                        alibi_slopes=slopes.to(DEV))
    (out * do.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    del ref['lse']   # (ops.attention returns none)
    res = dict(o=out)
    for t, name in zip(leaves, names):
        assert t.grad.shape == ref[name].shape
        res[name] = t.grad
    check_ref(res, ref)


@pytest.mark.parametrize('p', [0., 0.25])
def test_alibi_dead_rows_are_the_uniform_average(p):
    """W = 10 without sinks, padded layout: rows i >= 1 + W of the single-step episode see no key; the fill comes
    after the bias, so they attend all n positions uniformly — o is the (keep-weighted) average of v, bit for bit
    what a run with NULL slopes stores there (k_attn_dead_fwd), and dv's dead-row part is unchanged too."""
    b, H, Hkv, n, dh, W = 2, 4, 2, 130, 16, 10
    q, k, v, do, lens = problem(b, H, n, dh, 5, Hkv=Hkv)
    assert int(lens[b - 1]) == 1
    a = alibi_lib(q, k, v, lens, do, dh ** -0.5, p, 'two', slopes=dev_slopes(H), W=W)
    z = alibi_lib(q, k, v, lens, do, dh ** -0.5, p, 'two', W=W)
    dead = slice(1 + W, n)
    assert torch.equal(a['o'][b - 1, :, dead], z['o'][b - 1, :, dead])
    assert not torch.equal(a['o'][0], z['o'][0])
    if p == 0.:
        from xtrl_amd import ops
        want = v[b - 1, ops.kv_head_index(H, Hkv, device=DEV)].double().mean(1)   # [H][dh]
        G.tol(a['o'][b - 1, :, dead], want[:, None, :].expand(-1, n - 1 - W, -1).float(), 1e-5, 1e-5)
    # the single-step episode: row 0 sees key 0 alone (distance 0), rows 1 .. W see it at distance i; dk, dq of
    # the dead rows are 0 in both runs
    assert torch.equal(a['dq'][b - 1, :, dead], torch.zeros_like(a['dq'][b - 1, :, dead]))


# ----------------------------------------------------------------------------------------------
# model level: the ALiBi oracle (test_attn_alibi_cpu.alibi_forward over the frozen Attention)
# ----------------------------------------------------------------------------------------------

# (alibi_num_heads, W, M, Z, Hkv)
CONFIGS = {'plain': (None, None, 0, False, None), 'w5+zero': (None, 5, 0, True, None),
           'gqa2+mem3': (None, None, 3, False, 2), 'heads2of4': (2, None, 0, False, None)}
LEARNER = dict(episodes=6, batch=3, hazard=4)   # seed 3 at hazard 2^-4: lengths 4 .. T, ragged minibatches


def learner_kw(A, W, M, Z, Hkv, **kw):
    """G.make_learner's keywords of a CONFIGS entry (the ALiBi options themselves go in through install_alibi)."""
    return dict(window=W, num_mem_kv=M, add_zero_kv=Z, **({} if Hkv is None else dict(agent_extra=dict(kv_heads=Hkv))),
                **kw)


def alibi_rollout_and_learn(monkeypatch, cfg, T, minibatches, packed=False, heads=4, dim_head=16, **kw):
    A, W, M, Z, Hkv = CONFIGS[cfg] if isinstance(cfg, str) else cfg

    def checks(learner, env, oracle):
        c = learner.agent.cfg
        assert (c.alibi_heads, c.attn_window, c.num_mem_kv, c.add_zero_kv, c.n_kv_heads) == \
            (A or heads, W or 0, M, Z, Hkv or heads)
        eng = learner._engine_for(env, T)
        assert eng.desc.alibi_slopes and torch.equal(eng.alibi_slopes.cpu(), learner.agent.model.alibi_slopes.cpu())

    return AH.rollout_and_learn(monkeypatch, lambda mp: install_alibi(mp, heads, A, W, M, Z, Hkv), T, minibatches,
                                packed, checks, heads=heads, dim_head=dim_head, **{**LEARNER, **learner_kw(A, W, M, Z, Hkv, **kw)})


@pytest.mark.parametrize('rows', ['1', '0'])
@pytest.mark.parametrize('cfg', list(CONFIGS))
def test_alibi_rollout_and_learn_match_oracle(cfg, rows, monkeypatch):
    """Heads 4 x 16, d = 48, depth 2 with gates and the learned mix, T = 40: both decode paths (the row-resident
    step and the multi-kernel step), then two padded learn minibatches, against the ALiBi oracle — plain; W = 5
    with the zero key; kv_heads 2 with 3 memory rows; alibi_num_heads = 2."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', rows)
    learner, lens, seen = alibi_rollout_and_learn(monkeypatch, cfg, 40, 2)
    assert (learner._engine[1].rows_max > 0) == (rows == '1')
    assert int(lens.max()) > 20 and len(seen) == 2


@pytest.mark.parametrize('rows', ['1', '0'])
def test_alibi_long_rollout_second_key_chunk(rows, monkeypatch):
    """T = 140, depth 1, no window: the distances past the first 128-key chunk of k_attn_decode (and the second
    round trip of the row kernel's score loop)."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', rows)
    _, lens, _ = alibi_rollout_and_learn(monkeypatch, 'plain', 140, 0, depth=1, episodes=4, batch=2, hazard=12)
    assert int(lens.max()) > 130


@pytest.mark.parametrize('rows', ['1', '0'])
def test_alibi_windowed_rollout_measures_distance_after_the_pointer_shift(rows, monkeypatch):
    """T = 40, W = 5, no sinks: from step 6 on j_lo > 0 — the bias of the window-relative key j is slope (tw - j)."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', rows)
    _, lens, _ = alibi_rollout_and_learn(monkeypatch, (None, 5, 0, False, None), 40, 0)
    assert int(lens.max()) > 20


@pytest.mark.parametrize('dim', [256, 384])
def test_alibi_fused_out_projection_rollout(dim, monkeypatch):
    """d = 256 and d = 384 (the FJ = 1 and FJ = 2 forms), T = 40, W = 5 with the zero key: the attention decode
    kernel that applies the out-projection itself."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', '0')
    _, lens, _ = alibi_rollout_and_learn(monkeypatch, 'w5+zero', 40, 0, dim=dim)
    assert int(lens.max()) > 20


@pytest.mark.parametrize('cfg', ['plain', 'w5+zero', 'gqa2+mem3'])
def test_alibi_packed_learn_matches_oracle(cfg, monkeypatch):
    """The packed learn step: the positions i, j of the bias are per episode, not packed row numbers."""
    learner, _, seen = alibi_rollout_and_learn(monkeypatch, cfg, 40, 2, packed=True)
    assert learner.agent.packed_learn and len(seen) == 2


def test_alibi_dh32_rollout_and_learn_match_oracle(monkeypatch):
    """4 heads x 32 (d = 64), kv_heads 2, W = 5 and the zero key: the dh = 32 forms of every ALiBi kernel."""
    _, lens, seen = alibi_rollout_and_learn(monkeypatch, (None, 5, 0, True, 2), 40, 2, dim_head=32, dim=64)
    assert int(lens.max()) > 20 and len(seen) == 2


@pytest.mark.parametrize('rows', ['1', '0'])
def test_alibi_with_qk_norm_and_xpos_rollout_and_learn_match_oracle(rows, monkeypatch):
    """attn_qk_norm (scores x 10 instead of dh^-1/2: the bias is not scaled with them) and rotary_xpos under ALiBi
    with W = 5 and the zero key: rollout on both decode paths, then two padded learn minibatches."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', rows)
    wm = dict(attn_qk_norm=True, rotary_xpos=True, rotary_xpos_scale_base=8.)
    learner, lens, seen = alibi_rollout_and_learn(monkeypatch, 'w5+zero', 40, 2, wm_extra=wm)
    assert learner.agent.cfg.qk_norm and learner.agent.cfg.rotary_xpos and len(seen) == 2


@pytest.mark.parametrize('cfg', ['plain', 'w5+zero'])
def test_alibi_deploy_forward_matches_oracle_cached_decode(cfg, monkeypatch):
    """Agent.forward over 10 steps against the ALiBi oracle's cached decode (G.deploy_parity)."""
    A, W, M, Z, Hkv = CONFIGS[cfg]
    install_alibi(monkeypatch, 4, A, W, M, Z, Hkv)
    learner, env, oracle = G.make_learner(T=24, **LEARNER, **learner_kw(A, W, M, Z, Hkv))
    assert learner.agent.cfg.alibi_heads == 4
    G.deploy_parity(learner, oracle, 10)


@pytest.mark.parametrize('p', [0., 0.25])
@pytest.mark.parametrize('cfg', ['plain', 'w5+zero', 'gqa2+mem3'])
def test_alibi_fused_step_matches_reference_mode_autograd(cfg, p, monkeypatch):
    """The hand-scheduled learn step against the reference-mode autograd step (model.forward_train with
    ops.attention taking the slopes), T = 40: the bounds of test_fused_train_step_matches_autograd."""
    A, W, M, Z, Hkv = CONFIGS[cfg]
    install_alibi(monkeypatch, 4, A, W, M, Z, Hkv)

    def checks(learner, env, oracle):
        assert learner.agent.cfg.alibi_heads == 4 and learner.agent.model.alibi_slopes.is_cuda

    G._fused_vs_autograd(False, False, True, p, 40, depth=2, episodes=8, batch=4, hazard=4, dim=64, checks=checks,
                         with_oracle=False, **learner_kw(A, W, M, Z, Hkv))


def test_alibi_changes_the_rollout():
    """The feature is live: the same seed with and without alibi_pos_bias gives log-probs that differ by more
    than compare_rollout's tolerance (1e-4 relative + 1e-5) from the second step on; the first step, which has
    no past, is the same."""
    from xtrl_amd import Learner, SynthVecSim

    def run(**wm):
        torch.manual_seed(3)
        learner = Learner(state_dim=8, num_actions=4, reward_range=(-2., 2.), max_timesteps=12, batch_size=3,
                          world_model=dict(attn_dim_head=16, heads=4, depth=2, **wm), num_episodes_per_update=6,
                          agent_kwargs=dict(dropout=0., seed=3, hidden_dim=48), use_graph=False)
        traj, lens, _, _ = learner.rollout_device(SynthVecSim(8, 4, 'lander', hazard_log2=6), 0, 12)
        torch.cuda.synchronize()
        return traj['logp'].cpu(), lens.cpu()

    (a, la), (b, lb) = run(alibi_pos_bias=True), run()
    G.tol(a[:, 0], b[:, 0], 1e-4, 1e-5)
    both = (la >= 3) & (lb >= 3)
    assert both.any()
    excess = (a[both, 1:3] - b[both, 1:3]).abs() - (1e-5 + 1e-4 * b[both, 1:3].abs())
    assert float(excess.max()) > 0, float(excess.max())
