"""Sliding-window attention (world_model['attn_max_attend_past'] = W: query i sees key j iff
0 <= i - j <= W and j < len) on the MI355X: the windowed learn-step kernels through the C ABI against
an fp64 dense reference, and rollout / learn step / deploy against the windowed oracle
(test_attn_window_cpu.windowed_forward installed over the frozen oracle's Attention.forward)."""
import os

import pytest
import torch

from oracle import ref_port as R
from oracle import thirdparty as tp

import test_gpu_parity as G
from test_attn_window_cpu import windowed_forward
from test_gpu_parity import tol

pytestmark = pytest.mark.gpu
DEV = 'cuda'


# ----------------------------------------------------------------------------------------------
# kernel level
# ----------------------------------------------------------------------------------------------


def band_mask(n, lens, W):
    """[b][1][n][n]: key j visible to query i iff j <= i, i - j <= W and j < len."""
    i = torch.arange(n, device=lens.device)
    dist = i[:, None] - i[None, :]
    return ((dist >= 0) & (dist <= W))[None, None] & (i[None, None, None, :] < lens.long()[:, None, None, None])


def attn_win_ref(q, k, v, lens, scale, W, keep=None):
    """G.attn_ref (dense softmax, masked scores filled with the finite -max as x-transformers does)
    plus the band mask.  A row whose band holds no valid key — a padded row i >= len + W — therefore
    attends all n key positions uniformly and passes no gradient to its scores (without a window no
    row of an episode with a valid key is empty, so attn_ref never meets one)."""
    n = q.shape[2]
    mask = band_mask(n, lens, W)
    s = torch.einsum('bhid,bhjd->bhij', q, k) * scale
    p = s.masked_fill(~mask, -torch.finfo(s.dtype).max).softmax(-1)
    if keep is not None:
        p = p * keep
    return torch.einsum('bhij,bhjd->bhid', p, v)


def ragged_lens(g, b, n):
    """lens[0] = n, one episode of a single step, the others random."""
    lens = torch.randint(1, n + 1, (b,), generator=g).to(torch.int32)
    lens[0] = n
    lens[b - 1] = 1
    return lens.to(DEV)


def win_lib(q, k, v, lens, do, scale, p, W, mode, seed=3, offset=1, sub=0):
    """Forward + backward through the C ABI.  ``W`` None: the unwindowed entry points (xtrl_attn_fwd /
    xtrl_attn_bwd / xtrl_attn_bwd_part), else their _win forms.  ``mode``: 'two' (the dK/dV + dQ
    kernel pair, XTRL_ATTN_FUSED_BWD=0), 'fused' (=1: one launch for n <= 128) or 'part' (the long-episode
    backward with a dQ partial workspace)."""
    from xtrl_amd import _lib as L
    lib = L.lib()
    b, H, n, dh = q.shape
    o = torch.empty_like(q)
    dq, dk, dv = (torch.full_like(q, float('nan')) for _ in range(3))
    lse, delta = (torch.empty(b, H, n, device=DEV) for _ in range(2))
    win = () if W is None else (int(W),)
    fwd = lib.xtrl_attn_fwd if W is None else lib.xtrl_attn_fwd_win
    L.check(fwd(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(lens), L.ptr(o), L.ptr(lse), b, H, n, dh, scale, p, seed, offset, sub,
                *win, L.stream()), 'attn_fwd')
    old = os.environ.get('XTRL_ATTN_FUSED_BWD')
    os.environ['XTRL_ATTN_FUSED_BWD'] = '0' if mode == 'two' else '1'
    try:
        if mode == 'part':
            nf = int(lib.xtrl_attn_bwd_part_floats(b, H, n, dh))
            part = torch.full((nf,), float('nan'), device=DEV)
            bwd = lib.xtrl_attn_bwd_part if W is None else lib.xtrl_attn_bwd_part_win
            L.check(bwd(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(lens), L.ptr(o), L.ptr(lse), L.ptr(do), L.ptr(dq), L.ptr(dk),
                        L.ptr(dv), L.ptr(delta), L.ptr(part), nf, b, H, n, dh, scale, p, seed, offset, sub, *win,
                        L.stream()), 'attn_bwd_part')
        else:
            bwd = lib.xtrl_attn_bwd if W is None else lib.xtrl_attn_bwd_win
            L.check(bwd(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(lens), L.ptr(o), L.ptr(lse), L.ptr(do), L.ptr(dq), L.ptr(dk),
                        L.ptr(dv), L.ptr(delta), b, H, n, dh, scale, p, seed, offset, sub, *win, L.stream()), 'attn_bwd')
    finally:
        if old is None:
            del os.environ['XTRL_ATTN_FUSED_BWD']
        else:
            os.environ['XTRL_ATTN_FUSED_BWD'] = old
    torch.cuda.synchronize()
    return dict(o=o, lse=lse, delta=delta, dq=dq, dk=dk, dv=dv)


def problem(b, H, n, dh, seed):
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(b, H, n, dh, generator=g).to(DEV) for _ in range(4))
    return q, k, v, do, ragged_lens(g, b, n)


_REF = {}


def fp64_ref(b, H, n, dh, W):
    """(o, dq, dk, dv) of the fp64 reference on problem(b, H, n, dh, n + dh + W); computed once."""
    key = (b, H, n, dh, W)
    if key not in _REF:
        q, k, v, do, lens = problem(b, H, n, dh, n + dh + W)
        qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
        ref = attn_win_ref(qd, kd, vd, lens, dh ** -0.5, W)
        (ref * do.double()).sum().backward()
        _REF[key] = tuple(t.detach().cpu() for t in (ref, qd.grad, kd.grad, vd.grad))
    return _REF[key]


def check_fp64(res, b, H, n, dh, W):
    o, dq, dk, dv = fp64_ref(b, H, n, dh, W)
    tol(res['o'], o, 1e-5, 1e-5)
    tol(res['dq'], dq, 1e-4, 1e-5)
    tol(res['dk'], dk, 1e-4, 1e-5)
    tol(res['dv'], dv, 1e-4, 1e-5)


@pytest.mark.parametrize('b,H,n,dh,W', [(3, 4, 37, 16, 5), (2, 2, 70, 16, 1), (2, 2, 130, 16, 10), (2, 2, 200, 16, 63),
                                        (2, 2, 200, 16, 64), (2, 2, 200, 16, 65), (2, 3, 64, 32, 7), (1, 2, 70, 64, 20)])
def test_window_forward_and_two_kernel_backward(b, H, n, dh, W):
    """Forward + the dK/dV and dQ kernel pair at p = 0 against the fp64 band softmax.  n = 130, W = 10:
    rows >= 75 of query tile 1 see nothing in key tile 0 (their online-softmax state stays empty
    through it) and query tile 2 skips key tile 0, whose workgroup no longer stores D for it;
    W = 63 / 64 / 65: bands ending on, at and past a tile edge."""
    q, k, v, do, lens = problem(b, H, n, dh, n + dh + W)
    res = win_lib(q, k, v, lens, do, dh ** -0.5, 0., W, 'two')
    assert all(torch.isfinite(t).all() for t in res.values())
    check_fp64(res, b, H, n, dh, W)


@pytest.mark.parametrize('W', [10, 64])
@pytest.mark.parametrize('p', [0., 0.25])
def test_window_fused_backward_matches_two_kernel(W, p):
    """k_attn_bwd_fused (n <= 128) with a window against the kernel pair: o, lse, D, dQ, dK, dV
    bit-identical (as test_attention_fused_backward_matches_two_kernel requires without one), and at
    p = 0 within tolerance of the fp64 reference — W = 10: rows 74.. of the pair (key tile 0, query
    tile 1) are masked."""
    b, H, n, dh = 4, 4, 128, 16
    q, k, v, do, lens = problem(b, H, n, dh, n + dh + W)
    two = win_lib(q, k, v, lens, do, dh ** -0.5, p, W, 'two')
    fus = win_lib(q, k, v, lens, do, dh ** -0.5, p, W, 'fused')
    for name in ('o', 'lse', 'delta', 'dv', 'dk', 'dq'):
        d = (two[name] - fus[name]).abs()
        print(name, 'max |diff|', float(d.max()), '#differing', int((d > 0).sum()))
    for name in ('o', 'lse', 'delta', 'dv', 'dk', 'dq'):
        assert torch.equal(two[name], fus[name]), name
    if p == 0.:
        check_fp64(fus, b, H, n, dh, W)
        check_fp64(two, b, H, n, dh, W)


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
    two = win_lib(q, k, v, lens, do, dh ** -0.5, 0.25, W, 'two')
    part = win_lib(q, k, v, lens, do, dh ** -0.5, 0.25, W, 'part')
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
    res = win_lib(q, k, v, lens, do, dh ** -0.5, 0., W, 'part')
    check_fp64(res, b, H, n, dh, W)


@pytest.mark.parametrize('b,H,n,mode', [(4, 4, 128, 'two'), (4, 4, 128, 'fused'), (2, 4, 430, 'part')])
def test_window_covering_every_key_is_bit_identical_to_no_window(b, H, n, mode):
    """W = n - 1 and W = 4 n mask nothing: the _win results equal the unwindowed entry points' bit for
    bit at p = 0.25 — the dropout stream (keyed by absolute i, j), the summation orders and the move of
    D to the diagonal workgroups leave today's results unchanged."""
    q, k, v, do, lens = problem(b, H, n, 16, n)
    base = win_lib(q, k, v, lens, do, 0.25, 0.25, None, mode)
    for W in (n - 1, 4 * n):
        res = win_lib(q, k, v, lens, do, 0.25, 0.25, W, mode)
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


def make_win_learner(W, depth=2, gates=True, T=24, episodes=6, batch=3, seed=3, hazard=5, mode='lander', dim=48,
                     agent_extra=None, with_key=True):
    """Learner with world_model['attn_max_attend_past'] = W, the device Sim and the oracle on the same
    weights (G.make_learner's construction; its option map has no entry for the window, which the
    oracle takes from the patched Attention.forward instead)."""
    from xtrl_amd import Learner, SynthVecSim
    S, A = 8, 4
    torch.manual_seed(seed)
    wm = dict(attn_dim_head=16, heads=4, depth=depth)
    if gates:
        wm.update(attn_gate_values=True, add_value_residual=True, learned_value_residual_mix=True)
    if with_key:
        wm['attn_max_attend_past'] = W
    gp = dict(dim=8, num_genes_per_island=3, num_selected=2, tournament_size=2)
    learner = Learner(state_dim=S, num_actions=A, reward_range=(-2., 2.), world_model=wm, max_timesteps=T,
                      batch_size=batch, num_episodes_per_update=episodes, evolutionary=False, latent_gene_pool=gp,
                      agent_kwargs=dict(dropout=0., seed=seed, hidden_dim=dim, reward_dropout=0.5, **(agent_extra or {})),
                      use_graph=False)
    with torch.no_grad():   # non-trivial gate / mix weights (their init is constant)
        g = torch.Generator().manual_seed(seed + 1)
        for name, p in learner.agent.model.named_parameters():
            if 'to_v_gate' in name or 'to_value_residual_mix' in name:
                p.copy_((torch.randn(p.shape, generator=g) * 0.3).to(p.device))
        learner.agent.ema_flat.copy_(learner.agent.flat.flat)
    env = SynthVecSim(S, A, mode, hazard_log2=hazard)
    c = R.LearnerConfig(S, A, (-2., 2.), dim=dim, depth=depth, gate_values=gates, value_residual=gates,
                        learned_mix=gates, max_timesteps=T, batch_size=batch, num_episodes_per_update=episodes,
                        sim_mode=mode, hazard_log2=hazard, seed=seed, reward_dropout=0.5, gene_pool=gp)
    sd = {k: v.detach().cpu() for k, v in learner.agent.model.state_dict().items()}
    oracle = R.OracleLearner(c, init_state_dict=sd)
    return learner, env, oracle


def rollout_and_learn(monkeypatch, W, T, minibatches, **kw):
    monkeypatch.setattr(tp.Attention, 'forward', windowed_forward(W))
    learner, env, oracle = make_win_learner(W, T=T, **kw)
    assert learner.agent.cfg.attn_window == W
    traj, lens, genes, cum = learner.rollout_device(env, 0, T)
    torch.cuda.synchronize()
    episodes, _ = oracle.rollout(0)
    G.compare_rollout(traj, lens, episodes)
    seen = []
    if minibatches:
        seen = G._learn_parity(learner, oracle, traj, lens, genes, learner.fitness(cum, genes), minibatches)
    return learner, lens, seen


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
    res = {}
    for packed in (False, True):
        learner, env, _ = make_win_learner(9, depth=2, gates=True, T=70, episodes=8, batch=8, seed=5, hazard=5, dim=64,
                                           agent_extra=dict(hl_reduction_mean=False, packed_learn=packed))
        agent = learner.agent
        traj, lens, genes, cum = learner.rollout_device(env, 0, 70)
        res[packed] = G._first_minibatch_state(agent, traj, lens, genes, learner.fitness(cum, genes))
        res[packed]['lens'] = lens.cpu()
    a, b = res[True], res[False]
    assert torch.equal(a['lens'], b['lens']) and torch.equal(a['idx'], b['idx'])
    lens_mb = a['lens'][a['idx']].clamp(max=a['n'])
    assert lens_mb.min() < a['n'] and a['n'] > 64    # padding present; two key tiles
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


def test_window_fused_step_matches_reference_mode_autograd():
    """The hand-scheduled learn step against the reference-mode autograd step (ops.attention with the
    window) at T = 70, W = 9, dropout 0.25: the bounds of test_fused_train_step_matches_autograd."""
    learner, env, _ = make_win_learner(9, depth=2, gates=True, T=70, episodes=8, batch=4, seed=9, hazard=5, dim=64)
    agent = learner.agent
    agent.cfg.dropout = 0.25
    agent.model.cfg.dropout = 0.25
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


def test_window_deploy_forward_matches_oracle_cached_decode(monkeypatch):
    """Agent.forward (the deploy engine's descriptor carries the window) over 12 steps with W = 4
    against the windowed oracle's cached decode."""
    monkeypatch.setattr(tp.Attention, 'forward', windowed_forward(4))
    learner, env, oracle = make_win_learner(4, depth=2, gates=True, T=24)
    agent = learner.agent
    agent.rs_mean.copy_(torch.linspace(-0.5, 0.5, 9))
    agent.rs_var.copy_(torch.linspace(0.5, 2., 9))
    rs = R.RSNormState(9)
    rs.mean, rs.var = agent.rs_mean.cpu().clone(), agent.rs_var.cpu().clone()
    m = oracle.model
    m.eval()
    g = torch.Generator().manual_seed(2)
    hiddens, cache = None, None
    for t in range(12):
        s = torch.randn(8, generator=g)
        reward = None if t % 2 == 0 else float(torch.randn((), generator=g))
        raw, hiddens = agent(s.numpy(), reward=reward, hiddens=hiddens)
        swr = rs.apply(torch.cat((s, torch.tensor([0. if reward is None else reward]))))
        with torch.no_grad():
            r, _, _, _, cache = m(swr[:-1].reshape(1, 1, -1), rewards=None if reward is None else swr[-1], cache=cache)
        tol(raw, r.reshape(-1), 1e-4, 1e-5)


def test_window_none_leaves_the_rollout_unchanged():
    """attn_max_attend_past=None is no window: the rollout equals, bit for bit, that of a Learner built
    without the key."""
    out = []
    for with_key in (True, False):
        learner, env, _ = make_win_learner(None, T=24, with_key=with_key)
        assert learner.agent.cfg.attn_window == 0
        traj, lens, _, _ = learner.rollout_device(env, 0, 24)
        torch.cuda.synchronize()
        out.append(({k: v.clone() for k, v in traj.items() if v is not None}, lens.clone()))
    (ta, la), (tb, lb) = out
    assert torch.equal(la, lb) and ta.keys() == tb.keys()
    for k in ta:
        assert torch.equal(ta[k], tb[k]), k
