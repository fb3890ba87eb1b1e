"""MI355X tests of the scalar half of the learn step at its edge shapes and branches: the fused
PPO / critic / world-model / done loss (csrc/loss.hip), HL-Gauss decode + GAE (csrc/gae.hip), the
minibatch gather and RSNorm statistics (csrc/batch.hip) and the clip / AdoptAtan2 / EMA passes
(csrc/optim.hip), each against a float64 CPU reference built from the oracle's own functions
(tests/learn_scalar_cases.py; test_learn_scalar_cpu.py settles the same inputs without a GPU).

Tolerances are those of test_gpu_parity.py's kernel-level tests.  Every device output is filled
with NaN (integers: a sentinel) before the call and must be finite after it."""
import ctypes as C_
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import learn_scalar_cases as C
import test_gpu_parity as P
from oracle import thirdparty as tp

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
tol = P.tol


def _finite(*ts):
    for t in ts:
        assert bool(torch.isfinite(t).all()), 'an output element was not written (NaN fill left) or is not finite'


# ----------------------------------------------------------------------------------------------
# fused loss
# ----------------------------------------------------------------------------------------------


def _loss_consts(c):
    from xtrl_amd import ops
    ins = C.loss_inputs(c)
    hl = C.hl_module(c.B, double=False)
    acts = ins['actions'].float() if c.cont else ins['actions'].to(torch.int32)
    return ops.LossConsts(actions=acts.to(DEV).contiguous(), old_logp=ins['old_lp'].to(DEV), returns=ins['returns'].to(DEV),
                          old_values=ins['old_values'].to(DEV), dones=ins['dones'].to(torch.uint8).to(DEV),
                          lens=ins['lens'].to(DEV), real=ins['real'].to(DEV), support=hl.support.to(DEV),
                          centers=hl.centers.to(DEV), continuous=c.cont, squash=c.squash, hl_mean=c.hl_mean,
                          sigma=float(hl.sigma), **C.HP)


def run_loss(c):
    """xtrl_loss_fwd + xtrl_loss_bwd called directly, as ops.LossFn does, on a NaN-filled token
    workspace, statistics row and gradient buffers.  Returns (stats, [d_raw, d_values, d_pred, d_done])."""
    from xtrl_amd import _lib as L
    ins = C.loss_inputs(c)
    K = _loss_consts(c)
    x = [ins[k].to(DEV).contiguous() for k in ('raw', 'values', 'pred_raw', 'done_logit')]
    b, n = c.b, c.n
    tok = torch.full((b, n, L.LOSS_TOK), NAN, device=DEV)
    stats = torch.full((L.LOSS_STATS,), NAN, device=DEV)
    grads = [torch.full_like(t, NAN) for t in x]
    d = L.LossDesc(b=b, n=n, A=c.A, B=c.B, S1=c.S1, continuous=int(c.cont), squash=int(c.squash),
                   hl_reduction_mean=int(c.hl_mean), sigma=K.sigma, **C.HP)
    fields = dict(raw_actions=x[0], values=x[1], pred_raw=x[2], done_logit=x[3],
                  actions=None if c.cont else K.actions, actions_f=K.actions if c.cont else None, old_logp=K.old_logp,
                  returns=K.returns, old_values=K.old_values, dones=K.dones, lens=K.lens, real=K.real,
                  support=K.support, centers=K.centers, tok=tok, stats=stats, d_raw_actions=grads[0], d_values=grads[1],
                  d_pred_raw=grads[2], d_done_logit=grads[3])
    for name, t in fields.items():
        if t is not None:
            assert t.is_cuda and t.is_contiguous(), name
            setattr(d, name, t.data_ptr())
    L.check(L.lib().xtrl_loss_fwd(C_.byref(d), L.stream()), 'loss_fwd')
    L.check(L.lib().xtrl_loss_bwd(C_.byref(d), 1.0, L.stream()), 'loss_bwd')
    torch.cuda.synchronize()
    return stats.cpu(), [g.cpu() for g in grads]


def check_loss(c):
    """CPU assertions of the input set (margin, direction, census, saturation), then the kernels
    against the fp64 reference: loss and the four logged means at 1e-5 / 1e-6, the four input
    gradients at 1e-4 / 1e-6."""
    from xtrl_amd import _lib as L
    C.check_case(c)
    ref = C.loss_reference(c)
    stats, grads = run_loss(c)
    LS = L.LS
    _finite(stats[:len(LS)], *grads)
    print(c.name, {k: (float(stats[LS[k]]), float(ref[k])) for k in ('loss', 'actor', 'critic', 'autoreg', 'done')},
          [float((g.double() - r).abs().max()) for g, r in zip(grads, ref['grads'])])
    for k in ('loss', 'actor', 'critic', 'autoreg', 'done'):
        tol(stats[LS[k]], ref[k], 1e-5, 1e-6)
    assert float(stats[LS['nmask']]) == float(C.loss_inputs(c)['lens'].sum())
    if c.hl_mean:
        # the whole critic gradient goes to the smaller of the two global scalars
        tol(stats[LS['L']], ref['L'], 1e-5, 1e-6)
        tol(stats[LS['Lc']], ref['Lc'], 1e-5, 1e-6)
        small, other = ('dL', 'dLc') if ref['L'] < ref['Lc'] else ('dLc', 'dL')
        assert float(stats[LS[small]]) > 0. and float(stats[LS[other]]) == 0., (small, stats[LS['dL']], stats[LS['dLc']])
    for ours, theirs in zip(grads, ref['grads']):
        tol(ours, theirs, 1e-4, 1e-6)
    return stats, grads


@pytest.mark.parametrize('case', C.SHAPE_CASES, ids=C.case_id)
def test_fused_loss_edge_shapes(case):
    """B at the lane hand-over of the HL-Gauss bin edges (63, 64, 65, 127, and 2), the 32-wide
    shuffle broadcast of the discrete logits (A = 32), the world-model c += 64 loop (S1 = 65, 70)
    and the c == lane register path (S1 <= 64), token counts that are no multiple of 4 or 16 (the
    tail waves of k_loss_tokens / k_loss_bwd), ragged lens holding both n and 1."""
    check_loss(case)


@pytest.mark.parametrize('case', C.LARGE_CASES, ids=C.case_id)
def test_fused_loss_more_than_16384_tokens(case):
    """130 x 130 tokens: 1057 block partials, so k_loss_stats' 1024-thread strided loop takes its
    second trip, and k_loss_final sums 67 partials; under both reductions of the critic."""
    stats, grads = check_loss(case)
    from xtrl_amd import _lib as L
    # every gradient here carries 1 / n_mask ~ 1e-4, so the absolute 1e-6 of the shared bound is wide
    # at this size: also hold each tensor to 1e-4 of its OWN largest gradient (grad_mismatches' rule)
    for ours, theirs in zip(grads, C.loss_reference(case)['grads']):
        assert float((ours.double() - theirs).abs().max()) <= 1e-4 * float(theirs.abs().max())
    T = C.loss_reference(case)['tokens']
    clip = C.HP['value_clip']
    zero = ((T['ret'] < T['v']) & (T['v'] < T['v_old'] - clip)) | ((T['v_old'] + clip < T['v']) & (T['v'] < T['ret']))
    assert float(stats[L.LS['kcrit']]) == float((~zero & T['mask']).sum())
    assert float(stats[L.LS['nwm']]) == float(T['mask'][:, :-1].sum()) * case.S1


@pytest.mark.parametrize('case', C.MODE_CASES, ids=C.case_id)
def test_fused_loss_modes_and_branches(case):
    """Both directions of the global critic minimum under the mean reduction, un-squashed continuous
    actions (the Gaussian entropy and its dsd_extra gradient) under both reductions, squashed
    continuous actions under the per-token reduction; each input set holds every branch of the
    census (learn_scalar_cases.branch_census) and keeps every token 1e-5 away from every kink."""
    check_loss(case)


@pytest.mark.parametrize('case', C.SAT_CASES, ids=C.case_id)
def test_fused_loss_saturation(case):
    """The restated PyTorch saturation rules, deliberately reached.
    sat_done: done logits +-30, +-120, +-800 with both labels: the BCE log clamp at -100 (reached
    by float32 rounding of the sigmoid, so the done term and d_done_logit are compared with
    R.done_loss in float32; every other term of the same call with fp64).
    sat_logits: action logits with a spread of 40: Categorical's clamp(p, eps, 1 - eps) on both
    sides, taken actions with a clamped probability, zero gradient through a clamped entry.
    sat_squash: squashed actions at exactly +-1 (the 1e-20 clamp of the squash correction; tanhf does
    return exactly 1) and at the float32 neighbours of +-1.
    Not forced, because unreachable: the var < 1e-5 clamp of the policy's standard deviation and the
    var < 1e-6 clamp of gaussian_nll_loss — var = exp(3 tanh(lv / 3)) >= e^-3."""
    _, grads = check_loss(case)
    if case.sat == 'logits':
        # tokens whose three probabilities are all clamped: the reference's gradient there is the
        # entropy's probs factor alone, and the kernel must agree to that
        ref = C.loss_reference(case)['grads'][0]
        tol(grads[0][0], ref[0], 1e-4, 1e-9)


def test_fused_loss_autograd_wrapper_equals_direct_call():
    """ops.fused_loss (the autograd Function the reference-mode learn step uses) returns what the
    direct C-ABI calls return, bit for bit."""
    from xtrl_amd import _lib as L, ops
    c = C.MODE_CASES[4]
    stats, grads = run_loss(c)
    ins = C.loss_inputs(c)
    xs = [ins[k].to(DEV).requires_grad_() for k in ('raw', 'values', 'pred_raw', 'done_logit')]
    loss, st = ops.fused_loss(*xs, _loss_consts(c))
    loss.backward()
    torch.cuda.synchronize()
    n = len(L.LS)
    assert torch.equal(st.cpu()[:n], stats[:n]) and float(loss.detach()) == float(stats[L.LS['loss']])
    for x, g in zip(xs, grads):
        assert torch.equal(x.grad.cpu(), g)


# ----------------------------------------------------------------------------------------------
# HL-Gauss decode + GAE
# ----------------------------------------------------------------------------------------------


def run_gae(c):
    """xtrl_hlgauss_gae as ops.hlgauss_gae calls it, on NaN-filled outputs."""
    from xtrl_amd import _lib as L
    ins = C.gae_inputs(c)
    E, T, B, n = c.E, c.T, c.B, c.n
    hl = C.hl_module(B, double=False)
    logits, rewards, bounds, centers = (t.to(DEV).contiguous() for t in (ins['logits'], ins['rewards'], ins['bounds'],
                                                                          hl.centers))
    boot = lens = None
    if c.boot:
        boot, lens = ins['boot'].to(DEV), ins['lens'].to(DEV)
    values = torch.full((E, n), NAN, device=DEV)
    returns = torch.full((E, n), NAN, device=DEV)
    gl = float(torch.tensor(C.GAMMA * C.LAM, dtype=torch.float32))
    L.check(L.lib().xtrl_hlgauss_gae(L.ptr(logits), T * B, L.ptr(rewards), L.ptr(bounds), T, L.ptr(centers), L.ptr(values),
                                     L.ptr(returns), E, n, B, float(C.GAMMA), gl, L.ptr(boot), L.ptr(lens), L.stream()),
            'hlgauss_gae')
    torch.cuda.synchronize()
    return values.cpu(), returns.cpu(), (logits, rewards, bounds, centers, boot, lens)


@pytest.mark.parametrize('case', C.GAE_CASES, ids=str)
def test_hlgauss_gae_edges_and_bootstrap(case):
    """B in {2, 64, 65, 127, 200} (the kernel loops over bins), n in {1, 2, 37} with n == T and
    n < T (ld_row / ld_seq), boundaries at the last step, at step 0 and on consecutive steps, and the
    truncation bootstrap: boot mixes NaN and values, lens holds n (the padding slot) and values < n.
    Past lens with a bootstrap the kernel's values deliberately hold the bootstrap value: compared
    on t < lens only; without a bootstrap every t is compared."""
    from xtrl_amd import ops
    vals, rets, dev_in = run_gae(case)
    _finite(vals, rets)
    v_ref, r_ref = C.gae_reference(case)
    if case.boot:
        m = torch.arange(case.n)[None] < C.gae_inputs(case)['lens'][:, None]
    else:
        m = torch.ones(case.E, case.n, dtype=torch.bool)
    print(case, float((vals.double() - v_ref)[m].abs().max()), float((rets.double() - r_ref)[m].abs().max()))
    tol(vals[m], v_ref[m], 1e-5, 1e-6)
    tol(rets[m], r_ref[m], 1e-5, 1e-5)
    # the torch-facing wrapper returns the same
    logits, rewards, bounds, centers, boot, lens = dev_in
    v2, r2 = ops.hlgauss_gae(logits, rewards, bounds, centers, case.n, C.GAMMA, C.LAM, boot=boot, lens=lens)
    assert torch.equal(v2.cpu(), vals) and torch.equal(r2.cpu(), rets)


@pytest.mark.parametrize('case', C.GAE_CASES, ids=str)
def test_gae_returns_bitwise_equal_float32_oracle_scan(case):
    """gae.hip's promise: the scan runs in the oracle's order with FMA contraction off, so on the
    kernel's own decoded values the float32 R.calc_gae (separate multiply and add) gives the
    kernel's returns bit for bit — with and without boundaries and bootstrap, at every t."""
    vals, rets, _ = run_gae(case)
    assert torch.equal(C.gae_f32_restatement(case, vals), rets)


# ----------------------------------------------------------------------------------------------
# minibatch gather, RSNorm update
# ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('case', C.GATHER_CASES, ids=str)
def test_minibatch_gather_matches_restatement(case):
    """train.BatchGather against Agent.learn's preparation restated in torch.  Copies are bit-equal;
    swr within 1e-6 relative of fp64; rs_m per column within 1e-5 of that column's largest |swr|
    (the reduction's shape — at most 4 sequential terms per thread, 8 tree levels, 64 sequential
    block partials, in fp32 — bounds its error by ~76 * 2^-24 = 4.5e-6 of the largest term)."""
    from xtrl_amd.train import BatchGather
    c = case
    ins, ref = C.gather_inputs(c), C.gather_reference(c)
    cfg = SimpleNamespace(state_dim=c.S, num_actions=c.A, num_bins=c.B, continuous=c.cont)
    bg = BatchGather(cfg, c.b + 1, c.n + 2, DEV)
    for t in bg.buf.values():
        t.fill_(NAN if t.is_floating_point() else (255 if t.dtype == torch.uint8 else -7))
    traj = {k: (v.to(DEV).contiguous() if v is not None else None) for k, v in ins['traj'].items()}
    out = bg(traj, ins['returns'].to(DEV), ins['lens'].to(DEV), ins['idx'].to(DEV), ins['rs_mean'].to(DEV),
             ins['rs_var'].to(DEV), c.n)
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in out.items()}
    _finite(*(v for v in out.values() if v.is_floating_point()))
    for k in ('action', 'prev_action', 'old_logp', 'returns', 'old_values', 'dones', 'lens'):
        assert out[k].shape == ref[k].shape and torch.equal(out[k], ref[k].to(out[k].dtype)), k
    np.testing.assert_allclose(out['swr'].double().numpy(), ref['swr'].numpy(), rtol=1e-6, atol=1e-12)
    err = (out['rs_m'].double() - ref['rs_m']).abs()
    assert bool((err <= 1e-5 * ref['swr_max']).all()), (err / ref['swr_max']).max()


@pytest.mark.parametrize('D', [1, 9, 64, 65])
@pytest.mark.parametrize('t', [1, 2, 1000])
def test_rsnorm_update_matches_train_call(D, t):
    """xtrl_rsnorm_update against RSNormState.train_call's formulas in fp64 (t = 1: the variance
    becomes 0; D = 65: a second block)."""
    from xtrl_amd.train import rsnorm_update
    g = torch.Generator().manual_seed(D + t)
    mean, var, m = torch.randn(D, generator=g), torch.rand(D, generator=g) + 0.1, torch.randn(D, generator=g)
    mean_d, var_d = mean.to(DEV), var.to(DEV)
    rsnorm_update(mean_d, var_d, m.to(DEV), t)
    torch.cuda.synchronize()
    mean_r, var_r = C.rsnorm_update_reference(mean, var, m, t)
    _finite(mean_d, var_d)
    tol(mean_d, mean_r, 1e-6, 1e-7)
    tol(var_d, var_r, 1e-6, 1e-7)
    if t == 1:
        assert float(var_d.abs().max()) == 0.


# ----------------------------------------------------------------------------------------------
# clip, AdoptAtan2, EMA
# ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('n', [1, 255, 131075])
def test_grad_norm_and_clip_coefficient(n):
    """xtrl_grad_norm: n = 131 075 is just past 512 x 256, so the grid-stride loop takes a second
    pass.  Norm within 1e-6 relative of fp64; below max_norm the coefficient is exactly 1."""
    from xtrl_amd import ops
    g = torch.Generator().manual_seed(n)
    base = torch.randn(n, generator=g)
    for scale, above in ((3. / math.sqrt(n), True), (0.1 / math.sqrt(n), False)):
        grad = base * scale
        norm = float(grad.double().norm())
        assert (norm > 0.5) == above
        ws = torch.full((512,), NAN, dtype=torch.float64, device=DEV)
        out = torch.full((2,), NAN, device=DEV)
        ops.grad_norm(grad.to(DEV), 0.5, ws, out)
        torch.cuda.synchronize()
        _finite(out, ws)
        assert abs(float(out[0]) - norm) <= 1e-6 * norm, (float(out[0]), norm)
        if above:
            coef = 0.5 / (norm + 1e-6)
            assert abs(float(out[1]) - coef) <= 1e-6 * coef
        else:
            assert float(out[1]) == 1.


@pytest.mark.parametrize('row', C.ADOPT_ROWS, ids=lambda r: r[0])
def test_adopt_atan2_default_chunks_option_rows(row):
    """xtrl_adopt_atan2 in the kernel's real layout — the default 2048-element chunks over segments
    of 1 .. 5000 elements: the four-elements-per-thread unroll, its clamped tail loads, a second i0
    round (segments past 1024) and a second chunk (past 2048) — for four steps including the first,
    with exact zeros in the gradients and one all-zero segment, against tp.AdoptAtan2 in float32
    (the cautious mask is a discrete decision on m g > 0, and its per-segment mean moves every
    element of a short segment, so the reference keeps the kernel's number format, as the existing
    test does).  After every step: p, the clipped gradient left in g, m, v and p_init."""
    from xtrl_amd import ops
    _, o, lr_ratio, max_norm = row
    init_lr = C.ADOPT_LR
    lr = init_lr * lr_ratio
    params = C.adopt_params()
    ref_params = [torch.nn.Parameter(p.clone()) for p in params]
    opt = tp.AdoptAtan2(ref_params, lr=init_lr, betas=(0.9, 0.99), weight_decay=o['wd'], regen_reg_rate=o['regen'],
                        cautious_factor=o['cautious'])
    opt.param_groups[0]['lr'] = lr
    offs = np.cumsum([0] + C.ADOPT_SIZES)
    flat = torch.cat(params).to(DEV)
    m, v = (torch.full_like(flat, NAN) for _ in range(2))
    pinit = torch.full_like(flat, NAN) if o['regen'] > 0 else None
    seg = torch.tensor(offs, dtype=torch.int64, device=DEV)
    chunks = ops.adopt_chunks(seg)
    assert chunks.shape[0] == 11 and int((chunks[:, 1] - chunks[:, 0]).max()) == 2048
    seg_ws = torch.full((len(C.ADOPT_SIZES),), -7, dtype=torch.int32, device=DEV)
    ws = torch.zeros(512, dtype=torch.float64, device=DEV)
    clip = torch.full((2,), NAN, device=DEV) if max_norm is not None else None
    cat = lambda ts: torch.cat([t.detach().reshape(-1) for t in ts])   # noqa: E731
    for step in range(4):
        grads = C.adopt_grads(step)
        for p, gr in zip(ref_params, grads):
            p.grad = gr.clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(ref_params, max_norm)
        opt.step()
        gflat = torch.cat(grads).to(DEV)
        if max_norm is not None:
            ops.grad_norm(gflat, max_norm, ws, clip)
        # the kernel's weight_decay is the decoupled rate the reference derives (wd / init_lr)
        ops.adopt_atan2(flat, gflat, m, v, pinit, seg, chunks, seg_ws, clip, lr=lr, init_lr=init_lr, betas=(0.9, 0.99),
                        a=1.27, b=1., weight_decay=o['wd'] / init_lr, regen_rate=o['regen'], cautious=o['cautious'],
                        first_step=step == 0)
        torch.cuda.synchronize()
        if max_norm is not None:
            assert (float(clip[1]) < 1.) == (step == 2)
        _finite(flat, gflat, m, v, *([pinit] if pinit is not None else []))
        tol(flat, cat(ref_params), 1e-5, 1e-6)
        if max_norm is None:
            assert torch.equal(gflat.cpu(), torch.cat(grads))
        else:
            tol(gflat, cat([p.grad for p in ref_params]), 1e-5, 1e-6)
        tol(m, cat([opt.state[p]['m'] for p in ref_params]), 1e-5, 1e-6)
        tol(v, cat([opt.state[p]['v'] for p in ref_params]), 1e-5, 1e-6)
        if pinit is not None:
            tol(pinit, cat([opt.state[p]['param_init'] for p in ref_params]), 1e-5, 1e-6)
    assert float((flat.cpu() - torch.cat(params)).abs().max()) > 1e-4       # the parameters did move


@pytest.mark.parametrize('w', [0.1, 0.7])
def test_ema_lerp_second_grid_stride_pass(w):
    """xtrl_ema_lerp at n = 1 048 581, past 4096 x 256 (a second grid-stride pass), on both branches
    of the two-branch lerp (w < 0.5 and w >= 0.5), against fp64 torch.lerp."""
    from xtrl_amd import ops
    n = 1048581
    g = torch.Generator().manual_seed(8)
    ema, p = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ema_d = ema.to(DEV)
    ops.ema_lerp(ema_d, p.to(DEV), w)
    torch.cuda.synchronize()
    _finite(ema_d)
    tol(ema_d, torch.lerp(ema.double(), p.double(), float(torch.tensor(w, dtype=torch.float32))), 1e-6, 1e-7)


# ----------------------------------------------------------------------------------------------
# squash_continuous=False end to end
# ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('rows', ['1', '0'], ids=['rows', 'multi'])
def test_unsquashed_continuous_rollout_and_learn_match_oracle(rows, monkeypatch):
    """Learner(squash_continuous=False): the un-squashed sample and log-prob of the decode step (both
    decode paths) against the oracle's rollout, then two learn minibatches (Gaussian entropy in the
    fused loss) against the oracle at test_ppo_loss_and_grads_identical_weights' bounds."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', rows)
    learner, env, oracle = P.make_learner(cont=True, squash=False, depth=2, gates=True, dim=48, T=12)
    assert learner.agent.cfg.squash is False and oracle.c.squash is False
    assert (learner._engine_for(env, 12).rows_max > 0) == (rows == '1')
    traj, lens, genes, cum = learner.rollout_device(env, 0, 12)
    torch.cuda.synchronize()
    episodes, _ = oracle.rollout(0)
    P.compare_rollout(traj, lens, episodes, cont=True)
    # un-squashed samples do leave (-1, 1): the rollout stores them clamped to the action range
    assert float(traj['actions_f'].abs().max()) == 1.
    seen = P._learn_parity(learner, oracle, traj, lens, genes, learner.fitness(cum, genes), 2, cont=True)
    assert len(seen) == 2
