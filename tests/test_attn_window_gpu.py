"""Sliding-window attention (world_model['attn_max_attend_past'] = W: query i sees key j iff
0 <= i - j <= W and j < len) on the MI355X: the windowed learn-step kernels through the C ABI against
an fp64 dense reference, and rollout / learn step / deploy against the windowed oracle
(test_attn_window_cpu.windowed_forward installed over the frozen oracle's Attention.forward)."""
import functools

import pytest
import torch

from oracle import thirdparty as tp

import attn_harness as AH
import test_gpu_parity as G
from attn_harness import attn_win_ref, check_ref, problem
from test_attn_window_cpu import windowed_forward
from test_gpu_parity import tol

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# ----------------------------------------------------------------------------------------------
# kernel level
# ----------------------------------------------------------------------------------------------

# W=None: the unwindowed entry points (xtrl_attn_fwd / xtrl_attn_bwd / xtrl_attn_bwd_part), else their _win forms
win_lib = functools.partial(AH.attn_lib, abi='win')
_REF = {}


def fp64_ref(b, H, n, dh, W):
    """o, dq, dk, dv of the fp64 reference on problem(b, H, n, dh, n + dh + W); computed once."""
    key = (b, H, n, dh, W)
    if key not in _REF:
        q, k, v, do, lens = problem(b, H, n, dh, n + dh + W)
        qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
        ref = attn_win_ref(qd, kd, vd, lens, dh ** -0.5, W)
        (ref * do.double()).sum().backward()
        out = dict(o=ref, dq=qd.grad, dk=kd.grad, dv=vd.grad)
        _REF[key] = {name: t.detach().cpu() for name, t in out.items()}
    return _REF[key]


@pytest.mark.parametrize('b,H,n,dh,W', [(3, 4, 37, 16, 5), (2, 2, 70, 16, 1), (2, 2, 130, 16, 10), (2, 2, 200, 16, 63),
                                        (2, 2, 200, 16, 64), (2, 2, 200, 16, 65), (2, 3, 64, 32, 7), (1, 2, 70, 64, 20)])
def test_window_forward_and_two_kernel_backward(b, H, n, dh, W):
    """Forward + the dK/dV and dQ kernel pair at p = 0 against the fp64 band softmax.  n = 130, W = 10:
    rows >= 75 of query tile 1 see nothing in key tile 0 (their online-softmax state stays empty
    through it) and query tile 2 skips key tile 0, whose workgroup no longer stores D for it;
    W = 63 / 64 / 65: bands ending on, at and past a tile edge."""
    q, k, v, do, lens = problem(b, H, n, dh, n + dh + W)
    res = win_lib(q, k, v, lens, do, dh ** -0.5, 0., 'two', W=W)
    assert all(torch.isfinite(t).all() for t in res.values())
    check_ref(res, fp64_ref(b, H, n, dh, W))


@pytest.mark.parametrize('W', [10, 64])
@pytest.mark.parametrize('p', [0., 0.25])
def test_window_fused_backward_matches_two_kernel(W, p):
    """k_attn_bwd_fused (n <= 128) with a window against the kernel pair: o, lse, D, dQ, dK, dV
    bit-identical (as test_attention_fused_backward_matches_two_kernel requires without one), and at
    p = 0 within tolerance of the fp64 reference — W = 10: rows 74.. of the pair (key tile 0, query
    tile 1) are masked."""
    b, H, n, dh = 4, 4, 128, 16
    q, k, v, do, lens = problem(b, H, n, dh, n + dh + W)
    two = win_lib(q, k, v, lens, do, dh ** -0.5, p, 'two', W=W)
    fus = win_lib(q, k, v, lens, do, dh ** -0.5, p, 'fused', W=W)
    for name in ('o', 'lse', 'delta', 'dv', 'dk', 'dq'):
        d = (two[name] - fus[name]).abs()
        print(name, 'max |diff|', float(d.max()), '#differing', int((d > 0).sum()))
    for name in ('o', 'lse', 'delta', 'dv', 'dk', 'dq'):
        assert torch.equal(two[name], fus[name]), name
    if p == 0.:
        check_ref(fus, fp64_ref(b, H, n, dh, W))
        check_ref(two, fp64_ref(b, H, n, dh, W))


@pytest.mark.parametrize('b,H,n,W', [(3, 4, 257, 10), (2, 4, 430, 64), (2, 4, 500, 100), (3, 2, 500, 300)])
def test_window_long_backward_dq_folded(b, H, n, W):
    """xtrl_attn_bwd_part_win (dQ folded into the dK / dV kernel, partials over the band's key tiles
    only, summed by the reduce launch over exactly those) against the windowed kernel pair at
    p = 0.25 — dV, dK, D bit-identical; dQ bit-identical on the rows one key tile visits and within
    2e-6 of the dQ scale elsewhere, the bound of test_attention_long_backward_dq_folded_matches_two_kernel
    — and against the fp64 reference at p = 0.  The workspace is NaN-filled: a partial read that no
    tile wrote shows."""
    dh = 16
    q, k, v, do, lens = problem(b, H, n, dh, n + dh + W)
    two = win_lib(q, k, v, lens, do, dh ** -0.5, 0.25, 'two', W=W)
    part = win_lib(q, k, v, lens, do, dh ** -0.5, 0.25, 'part', W=W)
    assert torch.equal(part['dv'], two['dv']) and torch.equal(part['dk'], two['dk'])
    assert torch.equal(part['delta'], two['delta'])
    assert torch.isfinite(part['dq']).all()
    i = torch.arange(n, device=DEV)
    first = (i // 64 * 64 - W).clamp(min=0) // 64
    last = torch.minimum((i // 64)[None, :], ((lens.long() - 1) // 64)[:, None])     # [b][n]
    sole = (first[None, :] == last)[:, None, :].expand(b, H, n)
    assert torch.equal(part['dq'][sole], two['dq'][sole])
    scale = float(two['dq'].abs().max())
    err = float((part['dq'] - two['dq']).abs().max())
    print('dq err', err, 'scale', scale)
    assert err <= 2e-6 * scale, (err, scale)
    assert int((~sole).sum()) > 0
    res = win_lib(q, k, v, lens, do, dh ** -0.5, 0., 'part', W=W)
    check_ref(res, fp64_ref(b, H, n, dh, W))


@pytest.mark.parametrize('b,H,n,mode', [(4, 4, 128, 'two'), (4, 4, 128, 'fused'), (2, 4, 430, 'part')])
def test_window_covering_every_key_is_bit_identical_to_no_window(b, H, n, mode):
    """W = n - 1 and W = 4 n mask nothing: the _win results equal the unwindowed entry points' bit for
    bit at p = 0.25 — the dropout stream (keyed by absolute i, j), the summation orders and the move of
    D to the diagonal workgroups leave today's results unchanged."""
    q, k, v, do, lens = problem(b, H, n, 16, n)
    base = win_lib(q, k, v, lens, do, 0.25, 0.25, mode, W=None)
    for W in (n - 1, 4 * n):
        res = win_lib(q, k, v, lens, do, 0.25, 0.25, mode, W=W)
        for name in ('o', 'lse', 'delta', 'dv', 'dk', 'dq'):
            assert torch.equal(res[name], base[name]), (W, name)


def test_window_dropout_mask_is_host_philox_stream():
    """With a window the kept probabilities are still the host Philox stream's bits at the absolute
    (i, j) (as test_attention_dropout_mask_is_host_philox_stream without one): forward and q / k / v
    gradients against the fp64 band softmax times that keep mask."""
    from xtrl_amd import ops
    from oracle import philox as P
    b, H, n, dh, W, p = 2, 2, 130, 16, 10, 0.25
    g = torch.Generator().manual_seed(9)
    q, k, v, do = (torch.randn(b, H, n, dh, generator=g) for _ in range(4))
    lens = torch.tensor([130, 45], dtype=torch.int32)
    seed, offset, scale, layer = 1234567, 5, dh ** -0.5, 3
    keep = torch.from_numpy(P.attn_dropout_keep(b, H, n, p, seed, offset, layer)).double() / (1 - p)
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    ref = attn_win_ref(qd, kd, vd, lens, scale, W, keep)
    (ref * do.double()).sum().backward()
    qf, kf, vf = (t.to(DEV).requires_grad_() for t in (q, k, v))
    out = ops.attention(qf, kf, vf, lens.to(DEV), scale, p, seed=seed, offset=offset, sub=layer, window=W)
    (out * do.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    tol(out, ref, 1e-5, 1e-5)
    tol(qf.grad, qd.grad, 1e-4, 1e-5)
    tol(kf.grad, kd.grad, 1e-4, 1e-5)
    tol(vf.grad, vd.grad, 1e-4, 1e-5)


# ----------------------------------------------------------------------------------------------
# model level: the windowed oracle
# ----------------------------------------------------------------------------------------------


LEARNER = dict(episodes=6, batch=3, hazard=5)   # this file's G.make_learner defaults, with T = 24


def rollout_and_learn(monkeypatch, W, T, minibatches, **kw):
    """attn_harness.rollout_and_learn against the windowed oracle; the Learner's descriptor must carry W."""
    def checks(learner, env, oracle):
        assert learner.agent.cfg.attn_window == W

    return AH.rollout_and_learn(monkeypatch, lambda mp: mp.setattr(tp.Attention, 'forward', windowed_forward(W)), T,
                                minibatches, checks=checks, window=W, **{**LEARNER, **kw})


@pytest.mark.parametrize('rows', ['1', '0'])
def test_window_rollout_and_learn_match_oracle(rows, monkeypatch):
    """d = 48, depth 2 with gates and the learned value-residual mix, T = 24, W = 5: most steps have a
    truncated band.  Both decode paths (the row-resident step and the multi-kernel step), then two
    learn minibatches."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', rows)
    _, lens, seen = rollout_and_learn(monkeypatch, 5, 24, 2, depth=2, gates=True, episodes=6, batch=3, hazard=5)
    assert int(lens.max()) > 10
    assert len(seen) == 2


@pytest.mark.parametrize('W', [10, 135])
@pytest.mark.parametrize('rows', ['1', '0'])
def test_window_rollout_across_the_128_key_chunk(W, rows, monkeypatch):
    """150 steps of the non-terminating Sim: W = 10, the band starts inside the second 128-key chunk;
    W = 135, it spans two chunks with a first key that is no chunk multiple."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', rows)
    _, lens, _ = rollout_and_learn(monkeypatch, W, 150, 0, depth=1, gates=False, episodes=4, batch=2, mode='readme')
    assert int(lens.min()) == 150


def test_window_d256_fused_out_projection_rollout_and_learn(monkeypatch):
    """d = 256: the attention decode kernel that applies the out-projection itself, with the one-launch
    feed-forward; T = 40, W = 7, depth 2; then two learn minibatches."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', '0')
    learner, lens, seen = rollout_and_learn(monkeypatch, 7, 40, 2, depth=2, gates=True, episodes=6, batch=3, hazard=5,
                                            dim=256)
    assert int(lens.max()) > 7 and len(seen) == 2


def test_window_long_episode_learn_matches_oracle(monkeypatch):
    """T = 140, W = 20: the learn step's attention backward takes the n > 128 form (dQ partials over
    the band's key tiles)."""
    learner, lens, seen = rollout_and_learn(monkeypatch, 20, 140, 1, depth=1, gates=True, episodes=4, batch=2,
                                            mode='readme')
    assert seen[0][0] > 128
    assert 'dq_part' in learner.agent._train_step.cbuf


def test_window_packed_learn_matches_padded_step():
    """packed_learn (per-episode row ranges) with W = 9 at T = 70 against the padded step: the bounds
    of test_packed_learn_matches_padded_step."""
    a = G._packed_vs_padded(False, True, 70, 64, False, None, window=9)
    assert a['n'] > 64    # two key tiles


def test_window_fused_step_matches_reference_mode_autograd():
    """The hand-scheduled learn step against the reference-mode autograd step (ops.attention with the
    window) at T = 70, W = 9, dropout 0.25: the bounds of test_fused_train_step_matches_autograd."""
    G._fused_vs_autograd(False, False, True, 0.25, 70, depth=2, episodes=8, batch=4, hazard=5, dim=64, window=9)


def test_window_deploy_forward_matches_oracle_cached_decode(monkeypatch):
    """Agent.forward (the deploy engine's descriptor carries the window) over 12 steps with W = 4
    against the windowed oracle's cached decode."""
    monkeypatch.setattr(tp.Attention, 'forward', windowed_forward(4))
    learner, env, oracle = G.make_learner(window=4, T=24, **LEARNER)
    G.deploy_parity(learner, oracle, 12)


def test_window_none_leaves_the_rollout_unchanged():
    """attn_max_attend_past=None is no window: the rollout equals, bit for bit, that of a Learner built
    without the key."""
    out = []
    for with_key in (True, False):
        learner, env, _ = G.make_learner(window_key=with_key, T=24, **LEARNER)
        assert learner.agent.cfg.attn_window == 0
        traj, lens, _, _ = learner.rollout_device(env, 0, 24)
        torch.cuda.synchronize()
        out.append(({k: v.clone() for k, v in traj.items() if v is not None}, lens.clone()))
    (ta, la), (tb, lb) = out
    assert torch.equal(la, lb) and ta.keys() == tb.keys()
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k
