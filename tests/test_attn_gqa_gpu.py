"""Grouped-query attention in the learn-step attention kernels (q [b][H][n][dh]; k, v, dk, dv
[b][Hkv][n][dh]; query head h reads kv head ops.kv_head_index(H, Hkv)[h]) on the MI355X, through the
xtrl_attn_*_gqa entry points and ops.attention: against an fp64 dense reference (multi-head attention
on the repeated k / v, whose autograd sums dk / dv per group), against the old entry points at Hkv = H,
the backward modes against each other, and the dropout stream; then the rollout, the learn step and the
deploy forward with agent_kwargs kv_heads / world_model['attn_one_kv_head'] against the GQA oracle (test_attn_gqa_cpu.gqa_init /
gqa_forward installed over the frozen oracle's Attention)."""
import functools

import pytest
import torch

from oracle import thirdparty as tp

import attn_harness as AH
import test_gpu_parity as G
from attn_harness import NAMES, attn_win_ref, check_ref, modes_of, problem
from test_attn_gqa_cpu import gqa_forward, gqa_init

pytestmark = pytest.mark.gpu
DEV = 'cuda'
win_lib = functools.partial(AH.attn_lib, abi='win')   # W=None: the plain entry points
gqa_lib = functools.partial(AH.attn_lib, abi='gqa')   # W=None: window 0 (none)


def gqa_ref(q, k, v, do, lens, W, keep=None):
    """fp64 dense reference: multi-head attention on k, v repeated to H heads by the head mapping; the
    index_select's backward sums dk / dv over each kv head's query heads.  W None: no window (a band of
    n masks nothing).  Returns a dict of CPU tensors: o, dq, dk, dv."""
    from xtrl_amd import ops
    H, Hkv, n, dh = q.shape[1], k.shape[1], q.shape[2], q.shape[3]
    idx = ops.kv_head_index(H, Hkv, device=k.device)
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    ref = attn_win_ref(qd, kd[:, idx], vd[:, idx], lens, dh ** -0.5, n if W is None else W, keep)
    (ref * do.double()).sum().backward()
    return {name: t.detach().cpu() for name, t in dict(o=ref, dq=qd.grad, dk=kd.grad, dv=vd.grad).items()}


@pytest.mark.parametrize('b,H,Hkv,n,dh,W', [(3, 4, 2, 37, 16, None), (2, 4, 1, 70, 16, None), (2, 4, 2, 130, 16, None),
                                            (2, 4, 2, 130, 16, 10), (2, 4, 1, 200, 16, 64), (2, 6, 2, 64, 32, 7),
                                            (1, 4, 2, 70, 64, None), (1, 4, 2, 70, 64, 7)])
def test_gqa_forward_and_backward_against_fp64(b, H, Hkv, n, dh, W):
    """Forward + every backward mode of the shape at p = 0 against the fp64 reference, ragged lengths
    (one full episode, one of a single step), every output NaN-filled before and finite after.  W = 10 at
    n = 130 and W = 7 at n = 64 and n = 70 leave padded rows past the band: the uniform rows of k_attn_dead_fwd /
    k_attn_dead_bwd, whose dV part sums the group's query heads (dh = 64 at n = 70: their <64, true> forms)."""
    q, k, v, do, lens = problem(b, H, n, dh, n + dh + Hkv + (W or 0), Hkv=Hkv)
    ref = gqa_ref(q, k, v, do, lens, W)
    for mode in modes_of(n, dh):
        res = gqa_lib(q, k, v, lens, do, dh ** -0.5, 0., mode, W=W)
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
        old = win_lib(q, k, v, lens, do, dh ** -0.5, p, mode, W=W)
        new = gqa_lib(q, k, v, lens, do, dh ** -0.5, p, mode, W=W)
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
    q, k, v, do, lens = problem(b, H, n, dh, n + Hkv, Hkv=Hkv)
    two = gqa_lib(q, k, v, lens, do, dh ** -0.5, p, 'two', W=W)
    for mode in modes_of(n, dh):
        res = gqa_lib(q, k, v, lens, do, dh ** -0.5, p, mode, W=W)
        again = gqa_lib(q, k, v, lens, do, dh ** -0.5, p, mode, W=W)
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
        ref = gqa_ref(q, k, v, do, lens, W, keep)
        qf, kf, vf = (t.to(DEV).requires_grad_() for t in (q, k, v))
        out = ops.attention(qf, kf, vf, lens.to(DEV), dh ** -0.5, p, seed=seed, offset=offset, sub=layer, window=W or 0)
        (out * do.to(DEV)).sum().backward()
        torch.cuda.synchronize()
        assert kf.grad.shape == k.shape and vf.grad.shape == v.shape
        check_ref(dict(o=out, dq=qf.grad, dk=kf.grad, dv=vf.grad), ref)


# ----------------------------------------------------------------------------------------------
# model level: the GQA oracle (test_attn_gqa_cpu.gqa_init / gqa_forward over the frozen Attention)
# ----------------------------------------------------------------------------------------------


LEARNER = dict(episodes=6, batch=3, hazard=5)   # this file's G.make_learner defaults, with T = 24


def install_gqa_oracle(monkeypatch, Hkv, W=None):
    monkeypatch.setattr(tp.Attention, '__init__', gqa_init(Hkv))
    monkeypatch.setattr(tp.Attention, 'forward', gqa_forward(W))


def gqa_rollout_and_learn(monkeypatch, Hkv, T, minibatches, W=None, **kw):
    """attn_harness.rollout_and_learn against the GQA oracle (H = 4); the engine's caches must have Hkv heads."""
    def checks(learner, env, oracle):
        assert learner.agent.cfg.kv_heads == Hkv
        eng = learner._engine_for(env, T)
        for kc, vc in eng.kv:
            assert kc.shape == vc.shape == (eng.E, Hkv, T, 16)
        assert eng.v1.shape == (eng.E, Hkv * 16)

    return AH.rollout_and_learn(monkeypatch, lambda mp: install_gqa_oracle(mp, Hkv, W), T, minibatches, checks=checks,
                                kv_heads=Hkv, window=W, **{**LEARNER, **kw})


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
    G._packed_vs_padded(False, True, 70, 64, False, None, kv_heads=2, with_oracle=False)


@pytest.mark.parametrize('p', [0., 0.25])
def test_gqa_fused_step_matches_reference_mode_autograd(p):
    """The hand-scheduled learn step against the reference-mode autograd step (model.forward_train with
    ops.attention on Hkv-head k, v) at Hkv = 2 with gates, T = 70: the bounds of
    test_fused_train_step_matches_autograd."""
    G._fused_vs_autograd(False, False, True, p, 70, depth=2, episodes=8, batch=4, hazard=5, dim=64, kv_heads=2,
                         with_oracle=False)


def test_gqa_deploy_forward_matches_oracle_cached_decode(monkeypatch):
    """Agent.forward over 10 steps at Hkv = 1 against the GQA oracle's cached decode; the hiddens' cache
    tensors have one kv head."""
    install_gqa_oracle(monkeypatch, 1)
    learner, env, oracle = G.make_learner(kv_heads=1, T=24, **LEARNER)
    hiddens = G.deploy_parity(learner, oracle, 10)
    kv = [x for x in hiddens['cache'] if x.dim() == 4]
    assert kv and all(x.shape[1] == 1 and x.shape[3] == 16 for x in kv)


def test_gqa_rollout_graph_replay_equals_eager():
    """One GQA rollout (Hkv = 2, d = 48: the row-resident step's graphs) captured and replayed equals the
    eager rollout bit for bit, as test_rollout_graph_replay_equals_eager."""
    learner, env, _ = G.make_learner(kv_heads=2, T=16, episodes=40, batch=4, hazard=3, with_oracle=False)
    traj, lens, _, _ = learner.rollout_device(env, 0, 16)
    eager = {k: v.clone() for k, v in traj.items() if v is not None}
    learner.use_graph = True
    learner._engine = None
    for update in (0, 0):   # capture, then replay
        traj, lens2, _, _ = learner.rollout_device(env, update, 16)
    torch.cuda.synchronize()
    for k, v in eager.items():
        assert torch.equal(v, traj[k]), k
