"""Seeded inputs, fp64 references, branch census and kink-margin check for the scalar half of the
learn step: the fused PPO / critic / world-model / done loss, HL-Gauss decode + GAE, the minibatch
gather, RSNorm update, gradient clip, AdoptAtan2 and EMA kernels.

Imported by test_learn_scalar_cpu.py (which settles the inputs without a GPU: census and margin of
every loss input set) and by test_learn_scalar_gpu.py (which runs the kernels).  Everything here is
plain PyTorch on the CPU; the references are the oracle's own functions in float64."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import torch

from oracle import ref_port as R
from oracle import thirdparty as tp

# hyper-parameters of every fused-loss case (those of test_gpu_parity.test_fused_loss_matches_oracle)
HP = dict(eps_clip=0.2, value_clip=0.4, entropy_weight=0.01, w_actor=0.5, w_critic=1., w_autoreg=0.7, lo=-2., hi=2.)
MARGIN = 1e-5
F32_EPS = float(torch.finfo(torch.float32).eps)


@dataclass(frozen=True)
class LossCase:
    """One fused-loss input set.  ``census``: the set must hold every branch of branch_census.
    ``direction``: under the mean reduction, which of the two global critic scalars is the smaller
    ('L' or 'Lc'); asserted from the reference.  ``sat``: a saturation construction (None, 'done',
    'logits', 'squash')."""
    name: str
    b: int
    n: int
    A: int
    B: int
    S1: int
    cont: bool
    hl_mean: bool
    seed: int
    squash: bool = True
    census: bool = False
    direction: str = None
    sat: str = None


# §1 shapes: every B in {2, 63, 64, 65, 127}, discrete A in {1, 2, 32}, continuous A in {1, 6},
# S1 in {1, 2, 64, 65, 70}, b x n in {1 x 2, 3 x 17, 5 x 23}, each at least once
SHAPE_CASES = [
    LossCase('d_B2_A1_S1_1x2', 1, 2, 1, 2, 1, False, True, 0),
    LossCase('d_B63_A2_S2_3x17', 3, 17, 2, 63, 2, False, False, 0),
    LossCase('d_B64_A32_S64_5x23', 5, 23, 32, 64, 64, False, True, 0),
    LossCase('d_B65_A3_S65_3x17', 3, 17, 3, 65, 65, False, False, 0),
    LossCase('d_B127_A32_S70_5x23', 5, 23, 32, 127, 70, False, False, 0),
    LossCase('d_B127_A2_S6_1x2', 1, 2, 2, 127, 6, False, True, 0),
    LossCase('c_B63_A1_S1_3x17', 3, 17, 1, 63, 1, True, True, 0),
    LossCase('c_B64_A6_S65_5x23', 5, 23, 6, 64, 65, True, True, 0),
    LossCase('c_B65_A6_S2_1x2', 1, 2, 6, 65, 2, True, False, 0),
    LossCase('c_B127_A1_S64_3x17', 3, 17, 1, 127, 64, True, False, 0),
    LossCase('c_B2_A6_S70_5x23', 5, 23, 6, 2, 70, True, True, 0),
    LossCase('c_B64_A1_S2_3x17_nosquash', 3, 17, 1, 64, 2, True, False, 0, squash=False),
]

# §1 large case: 16 900 tokens -> 1057 block partials for k_loss_stats (a second trip of its
# 1024-thread strided loop) and 67 for k_loss_final
LARGE_CASES = [
    LossCase('large_mean', 130, 130, 3, 100, 6, False, True, 5, census=True, direction='L'),
    LossCase('large_token', 130, 130, 3, 100, 6, False, False, 5, census=True),
]

# §2 modes and branches at 5 x 23, B = 100, A = 3, S1 = 6, each with the full census
MODE_CASES = [
    LossCase('d_mean_L', 5, 23, 3, 100, 6, False, True, 0, census=True, direction='L'),
    LossCase('d_mean_Lc', 5, 23, 3, 100, 6, False, True, 3, census=True, direction='Lc'),
    LossCase('d_token', 5, 23, 3, 100, 6, False, False, 0, census=True),
    LossCase('c_nosquash_mean', 5, 23, 3, 100, 6, True, True, 0, squash=False, census=True),
    LossCase('c_nosquash_token', 5, 23, 3, 100, 6, True, False, 0, squash=False, census=True),
    LossCase('c_squash_token', 5, 23, 3, 100, 6, True, False, 0, census=True),
]

# §3 saturation
SAT_CASES = [
    LossCase('sat_done', 3, 17, 3, 100, 6, False, True, 0, sat='done'),
    LossCase('sat_logits', 3, 17, 3, 100, 6, False, False, 0, sat='logits'),
    LossCase('sat_squash', 3, 17, 2, 100, 6, True, True, 0, sat='squash'),
]

ALL_LOSS_CASES = SHAPE_CASES + LARGE_CASES + MODE_CASES + SAT_CASES
DONE_SAT_LOGITS = (30., -30., 120., -120., 800., -800.)


def case_id(c):
    return c.name


def hl_module(B, double=True):
    hl = tp.HLGaussLoss(HP['lo'], HP['hi'], B, clamp_to_range=True)
    return hl.double() if double else hl


def _lens(c, g):
    """Ragged episode lengths that contain both n and 1 (b = 1: the full length)."""
    if c.b == 1:
        return torch.tensor([c.n], dtype=torch.int32)
    lens = torch.randint(2, c.n + 1, (c.b,), generator=g, dtype=torch.int32)
    lens[0], lens[1] = c.n, 1
    return lens


@functools.lru_cache(maxsize=None)
def loss_inputs(c: LossCase):
    """float32 / integer CPU tensors of one case.  The value logits are drawn wide (x 3) so the
    decoded values spread over the reward range and both ``between`` clauses of the critic occur;
    the returns are drawn past +-value_clip and past [lo, hi]."""
    g = torch.Generator().manual_seed(1000 * c.seed + 17 * c.B + c.A + (7 if c.cont else 0))
    b, n, A, B, S1 = c.b, c.n, c.A, c.B, c.S1
    lens = _lens(c, g)
    raw = torch.randn(b, n, 2 * A if c.cont else A, generator=g)
    values = torch.randn(b, n, B, generator=g) * 3.
    old_values = torch.randn(b, n, B, generator=g) * 3.
    pred_raw = torch.randn(b, n, 2 * S1, generator=g)
    done_logit = torch.randn(b, n, generator=g) * 2
    returns = torch.randn(b, n, generator=g) * 1.3
    dones = torch.rand(b, n, generator=g) < 0.2
    real = torch.randn(b, n, S1, generator=g)
    if c.cont:
        if c.squash:
            actions = torch.rand(b, n, A, generator=g) * 1.8 - 0.9
        else:
            actions = torch.randn(b, n, A, generator=g) * 1.5
    else:
        actions = torch.randint(0, A, (b, n), generator=g)
    noise = torch.rand(b, n, *((A,) if c.cont else ()), generator=g) - 0.5

    if c.sat == 'done':
        # every saturating logit with both labels on the first (full-length, masked) episode
        k = 0
        for z in DONE_SAT_LOGITS:
            for label in (False, True):
                done_logit[0, k], dones[0, k] = z, label
                k += 1
        assert k <= n
    if c.sat == 'logits':
        # spread 40: [0, -40, -40] (dominant probability > 1 - eps, the others clamped at eps) and
        # [0, 0, -40]; the taken action alternates between a clamped and an unclamped entry
        for t in range(n):
            raw[0, t] = torch.tensor([0., -40., -40.]).roll(t % 3)
            actions[0, t] = (t + t // 3) % 3
        for t in range(0, lens[2].item()):
            raw[2, t] = torch.tensor([0., 0., -40.]).roll(t % 3)
            actions[2, t] = t % 3
    if c.sat == 'squash':
        # exactly +-1 (the 1e-20 clamp of the squash correction) and the float32 neighbours of +-1
        one = torch.tensor(1.)
        below = torch.nextafter(one, torch.tensor(0.))
        edge = torch.stack([one, -one, below, -below])
        for t in range(n):
            actions[0, t, 0] = edge[t % 4]
            actions[0, t, 1] = edge[(t // 4) % 4] if t % 2 else actions[0, t, 1]
    if c.cont:
        lp = R.continuous_log_prob(raw.double(), actions.double(), c.squash)
    else:
        lp = R.discrete_log_prob(raw.double(), actions)
    # old log-probs around the new ones: ratios spread over [e^-0.5, e^0.5], past both clip bounds
    old_lp = (lp + noise.double()).float()
    return dict(raw=raw, values=values, pred_raw=pred_raw, done_logit=done_logit, actions=actions, old_lp=old_lp,
                returns=returns, old_values=old_values, dones=dones, real=real, lens=lens)


def _config(c):
    return R.ModelConfig(max(c.S1 - 1, 0), c.A, 32, continuous=c.cont, squash=c.squash, reward_range=(HP['lo'], HP['hi']),
                         entropy_weight=HP['entropy_weight'], eps_clip=HP['eps_clip'], value_clip=HP['value_clip'])


@functools.lru_cache(maxsize=None)
def loss_reference(c: LossCase):
    """The fp64 reference of one case, computed once and shared: loss, the four logged means, the
    four input gradients and the per-token decision quantities of census and margin.  Combined as
    Agent.learn does (xtrl.py:939-978), from the oracle's loss functions.
    sat == 'done': the done term (value and d_done_logit) is evaluated in float32 — the -100 log
    clamp is reached by float32 rounding of the sigmoid (in float64 log(1 - sigmoid(30)) is -30),
    so float32 is the truth for that term; every other term stays fp64."""
    ins = loss_inputs(c)
    b, n, S1 = c.b, c.n, c.S1
    cfg = _config(c)
    hld = hl_module(c.B)
    prev = tp.HLGaussLoss.default_reduction
    tp.HLGaussLoss.default_reduction = 'mean' if c.hl_mean else 'none'
    try:
        leaves = [ins[k].clone().double().requires_grad_() for k in ('raw', 'values', 'pred_raw', 'done_logit')]
        r_, v_, p_, d_ = leaves
        lens = ins['lens']
        mask = torch.arange(n)[None] < lens[:, None]
        mean, lv = p_.reshape(b, n, S1, 2).unbind(-1)
        var = (torch.tanh(lv / 3.) * 3.).exp()
        wm = R.autoregressive_loss(torch.stack((mean, var)), ins['real'].double())[mask[:, :-1]]
        if c.sat == 'done':
            d32 = ins['done_logit'].clone().requires_grad_()
            dl = R.done_loss(torch.sigmoid(d32), ins['dones'])[mask]
        else:
            dl = R.done_loss(torch.sigmoid(d_), ins['dones'])[mask]
        actions = ins['actions'].double() if c.cont else ins['actions']
        old_lp, returns, old_values = ins['old_lp'].double(), ins['returns'].double(), ins['old_values'].double()
        al = R.actor_loss(cfg, hld, r_, actions, old_lp, returns, old_values, mask)
        cl = R.critic_loss(cfg, hld, v_, returns, old_values)
        ac = (al * HP['w_actor'] + cl * HP['w_critic'])[mask]
        loss = ac.mean() + (wm.mean() + dl.mean().double()) * HP['w_autoreg']
        loss.backward()
        grads = [t.grad for t in leaves]
        if c.sat == 'done':
            grads[3] = d32.grad.double()
        with torch.no_grad():
            raw64, val64 = ins['raw'].double(), ins['values'].double()
            lp = R.continuous_log_prob(raw64, actions, c.squash) if c.cont else R.discrete_log_prob(raw64, actions)
            probs = None if c.cont else R.categorical_logits(raw64)[0]
            clip = HP['value_clip']
            tokens = dict(mask=mask, ratio=(lp - old_lp).exp(), advn=R.normalize(returns - hld(old_values), mask),
                          v=hld(val64), v_old=hld(old_values), ret=returns,
                          ceu=hld(val64, returns, reduction='none'),
                          cec=hld(val64, returns.clamp(-clip, clip), reduction='none'), probs=probs)
    finally:
        tp.HLGaussLoss.default_reduction = prev
    return dict(loss=loss.detach(), actor=al.mean().detach(), critic=cl.mean().detach(), autoreg=wm.mean().detach(),
                done=dl.mean().detach().double(), grads=[g_.detach() for g_ in grads], tokens=tokens,
                L=float(tokens['ceu'].mean()), Lc=float(tokens['cec'].mean()))


def branch_census(c: LossCase):
    """How many masked tokens of the fp64 reference take each branch of the loss (for continuous
    actions the ratio branches count (token, action) pairs); 'padded' counts the tokens past their
    episode and 'last_step' the masked tokens at t = n - 1, which have no world-model term."""
    T = loss_reference(c)['tokens']
    m, r, a = T['mask'], T['ratio'], T['advn']
    lo, hi, clip = 1 - HP['eps_clip'], 1 + HP['eps_clip'], HP['value_clip']
    if r.ndim == 3:
        m3, a = m[..., None].expand_as(r), a[..., None].expand_as(r)
    else:
        m3 = m
    v, vo, ret, ceu, cec = T['v'], T['v_old'], T['ret'], T['ceu'], T['cec']
    n_ = lambda cond, mk=m: int((cond & mk).sum())   # noqa: E731
    return dict(ratio_low_adv_pos=n_((r < lo) & (a > 0), m3), ratio_low_adv_neg=n_((r < lo) & (a < 0), m3),
                ratio_high_adv_pos=n_((r > hi) & (a > 0), m3), ratio_high_adv_neg=n_((r > hi) & (a < 0), m3),
                ratio_inside=n_((r >= lo) & (r <= hi), m3),
                critic_zero_below=n_((ret < v) & (v < vo - clip)), critic_zero_above=n_((vo + clip < v) & (v < ret)),
                ret_past_value_clip=n_(ret.abs() > clip), ret_past_range=n_((ret < HP['lo']) | (ret > HP['hi'])),
                ceu_lt_cec=n_(ceu < cec), cec_lt_ceu=n_(cec < ceu), ce_tie=n_((ceu == cec) & (ret.abs() <= clip)),
                padded=int((~m).sum()), last_step=int(m[:, -1].sum()))


PER_TOKEN_ONLY = ('ceu_lt_cec', 'cec_lt_ceu', 'ce_tie')


def census_missing(c: LossCase):
    """The branches a census case does not hold (the per-token minimum's three only where the
    reduction is per token)."""
    cen = branch_census(c)
    return [k for k, v in cen.items() if v < 1 and (not c.hl_mean or k not in PER_TOKEN_ONLY)]


def kink_margin(c: LossCase):
    """Smallest distance of any token of the fp64 reference from a decision boundary: ratio vs the
    two clip bounds and normalised advantage vs 0 (masked tokens: the actor term of a padded token
    reaches no output but the logged actor mean, which is continuous in both), ret vs v and v vs
    v_old -/+ value_clip (EVERY token, padded ones included: the logged critic mean runs over all
    of them), ceu vs cec where ret lies outside +-value_clip (every token).  No token is left out."""
    T = loss_reference(c)['tokens']
    m, r, a = T['mask'], T['ratio'], T['advn']
    lo, hi, clip = 1 - HP['eps_clip'], 1 + HP['eps_clip'], HP['value_clip']
    m3 = m[..., None].expand_as(r) if r.ndim == 3 else m
    v, vo, ret = T['v'], T['v_old'], T['ret']
    out = dict(ratio=float(torch.minimum((r - lo).abs(), (r - hi).abs())[m3].min()), adv=float(a[m].abs().min()),
               ret_v=float((ret - v).abs().min()),
               v_clip=float(torch.minimum((v - (vo - clip)).abs(), (v - (vo + clip)).abs()).min()))
    outside = ret.abs() > clip
    out['ce'] = float((T['ceu'] - T['cec'])[outside].abs().min()) if outside.any() else float('inf')
    if c.hl_mean:
        out['L_Lc'] = abs(loss_reference(c)['L'] - loss_reference(c)['Lc'])
    return out


def check_case(c: LossCase):
    """The CPU-side assertions of one loss input set (run by both test files)."""
    margins = kink_margin(c)
    assert min(margins.values()) >= MARGIN, (c.name, margins)
    ref = loss_reference(c)
    if c.direction is not None:
        assert c.hl_mean
        assert (ref['L'] < ref['Lc']) == (c.direction == 'L'), (c.name, ref['L'], ref['Lc'])
    if c.census:
        assert not census_missing(c), (c.name, branch_census(c))
    if c.sat == 'logits':
        p, m = ref['tokens']['probs'], ref['tokens']['mask']
        pm = p[m]
        assert bool(((pm < 1e-12) | (pm > 1e-3)).all()), 'a probability sits near the eps clamp'
        taken = p.gather(-1, loss_inputs(c)['actions'][..., None])[..., 0][m]
        assert int((taken < 1e-12).sum()) >= 1 and int((pm > 1 - F32_EPS).sum()) >= 1
        # the gradient through a clamped entry is zero: on the tokens whose three probabilities are
        # all clamped the log-prob of the taken action has no gradient in the reference (what is left
        # of the token's gradient is the entropy's unclamped probs factor)
        raw0 = loss_inputs(c)['raw'][0].double().requires_grad_()
        R.discrete_log_prob(raw0, loss_inputs(c)['actions'][0]).sum().backward()
        assert float(raw0.grad.abs().max()) == 0. and float(ref['grads'][0][m].abs().max()) > 0.
    if c.sat == 'squash':
        a = loss_inputs(c)['actions'][0]
        below = float(torch.nextafter(torch.tensor(1.), torch.tensor(0.)))
        for x in (1., -1., below, -below):
            assert int((a == x).sum()) >= 1, x
        # at +-1 the squash correction is -log(1e-20) = 46.05..., at the neighbours -log(2^-23 - 2^-48)
        ins = loss_inputs(c)
        lp = R.continuous_log_prob(ins['raw'].double(), ins['actions'].double(), True)
        gauss = R.continuous_log_prob(ins['raw'].double(), ins['actions'].double(), False)
        corr = (lp - gauss)[0]
        assert bool(((corr[a.abs() == 1.] - 20 * math.log(10.)).abs() < 1e-9).all())
        assert bool(((corr[a.abs() == below] - 23 * math.log(2.)).abs() < 1e-6).all())
    if c.sat == 'done':
        ins = loss_inputs(c)
        seen = {(float(z), bool(y)) for z, y in zip(ins['done_logit'][0], ins['dones'][0])}
        assert all((z, y) in seen for z in DONE_SAT_LOGITS for y in (False, True))
        # the clamp is reached: a saturated, mislabelled token costs exactly 100
        assert float(R.done_loss(torch.sigmoid(torch.tensor([30., -120.])), torch.tensor([False, True])).min()) == 100.
        # ... and float64 would not reach it at +-30, so the two references differ far beyond the bound
        d64 = R.done_loss(torch.sigmoid(ins['done_logit'].double()), ins['dones'])[ref['tokens']['mask']].mean()
        assert abs(float(d64) - float(ref['done'])) > 1.


# ----------------------------------------------------------------------------------------------
# HL-Gauss decode + GAE
# ----------------------------------------------------------------------------------------------

GAMMA, LAM = 0.99, 0.95


@dataclass(frozen=True)
class GaeCase:
    B: int
    n: int
    T: int
    boot: bool
    E: int = 7


GAE_CASES = [GaeCase(2, 1, 1, False), GaeCase(64, 2, 2, True), GaeCase(65, 2, 5, False), GaeCase(127, 37, 37, True),
             GaeCase(200, 37, 40, True), GaeCase(200, 1, 3, True), GaeCase(64, 37, 40, False), GaeCase(2, 37, 37, False)]


@functools.lru_cache(maxsize=None)
def gae_inputs(c: GaeCase):
    """Boundaries at the last step, at step 0 and on consecutive steps; with a bootstrap, ``boot``
    mixes NaN (none) and values and ``lens`` holds n (the padding slot is written) and values < n."""
    g = torch.Generator().manual_seed(31 * c.B + c.n)
    E, T, B, n = c.E, c.T, c.B, c.n
    logits = torch.randn(E, T, B, generator=g) * 2.
    rewards = torch.randn(E, T, generator=g)
    bounds = (torch.rand(E, T, generator=g) < 0.1).to(torch.uint8)
    bounds[0, n - 1] = 1
    bounds[1, 0] = 1
    if n >= 5:
        bounds[2, 2:5] = 1
    bounds[3] = 0
    boot = lens = None
    if c.boot:
        boot = torch.randn(E, generator=g)
        boot[0::3] = float('nan')
        lens = torch.randint(1, n + 1, (E,), generator=g, dtype=torch.int32)
        lens[1], lens[3] = n, n            # boot[1] is a value, boot[3] NaN
        lens[2], lens[4] = max(n - 1, 1), 1
    return dict(logits=logits, rewards=rewards, bounds=bounds, boot=boot, lens=lens)


def gae_reference(c: GaeCase):
    ins = gae_inputs(c)
    n = c.n
    hl = hl_module(c.B)
    v = hl(ins['logits'][:, :n].double())
    boot = None if ins['boot'] is None else ins['boot'].double()
    r = R.calc_gae(ins['rewards'][:, :n].double(), v, (ins['bounds'][:, :n] == 0).double(), GAMMA, LAM, boot, ins['lens'])
    return v, r


def gae_f32_restatement(c: GaeCase, values_f32):
    """R.calc_gae in float32 on the kernel's own decoded values: separate multiply and add in the
    same order as the kernel's scan, so the kernel's returns must equal it bit for bit."""
    ins = gae_inputs(c)
    n = c.n
    return R.calc_gae(ins['rewards'][:, :n], values_f32, (ins['bounds'][:, :n] == 0).float(), GAMMA, LAM, ins['boot'],
                      ins['lens'])


# ----------------------------------------------------------------------------------------------
# minibatch gather + RSNorm
# ----------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class GatherCase:
    cont: bool
    S: int
    A: int
    B: int
    n: int
    Tmax: int
    N: int = 9
    b: int = 6


GATHER_CASES = [GatherCase(False, 1, 4, 2, 7, 7), GatherCase(False, 8, 4, 100, 5, 11), GatherCase(False, 63, 3, 2, 11, 11),
                GatherCase(True, 8, 1, 100, 7, 7), GatherCase(True, 63, 32, 2, 5, 11), GatherCase(True, 1, 32, 100, 11, 11)]


@functools.lru_cache(maxsize=None)
def gather_inputs(c: GatherCase):
    g = torch.Generator().manual_seed(100 * c.S + c.A + c.n)
    N, T, S, A, B, n = c.N, c.Tmax, c.S, c.A, c.B, c.n
    traj = dict(states=torch.randn(N, T, S, generator=g) * 2 + 0.5, rewards=torch.randn(N, T, generator=g),
                bounds=(torch.rand(N, T, generator=g) < 0.2).to(torch.uint8), values=torch.randn(N, T, B, generator=g))
    if c.cont:
        traj.update(actions_f=torch.randn(N, T, A, generator=g), logp=torch.randn(N, T, A, generator=g), actions=None)
    else:
        traj.update(actions=torch.randint(0, A, (N, T), generator=g, dtype=torch.int32),
                    logp=torch.randn(N, T, generator=g), actions_f=None)
    returns = torch.randn(N, n, generator=g)
    lens = torch.randint(1, n + 1, (N,), generator=g, dtype=torch.int32)
    lens[0], lens[N - 1] = n, 1
    # permuted, with a repeat, containing episode 0 and the last episode
    idx = torch.tensor([N - 1, 3, 0, 5, 3, 1], dtype=torch.int64)[:c.b]
    rs_mean = torch.randn(S + 1, generator=g) * 0.3
    rs_var = torch.rand(S + 1, generator=g) + 0.5
    rs_var[0] = 0.                       # the 1e-5 clamp of the standard deviation
    rs_var[S] = 1e-12                    # a tiny entry (sqrt = 1e-6, clamped as well)
    return dict(traj=traj, returns=returns, lens=lens, idx=idx, rs_mean=rs_mean, rs_var=rs_var)


def gather_reference(c: GatherCase):
    """Agent.learn's preparation (xtrl.py:822-924) restated in torch: index the episodes, cut to n
    steps, shift actions and rewards right by one, RSNorm with the OLD statistics (fp64), copy the
    loss inputs; rs_m is the masked column mean of the normalised rows."""
    ins = gather_inputs(c)
    tr, idx, n = ins['traj'], ins['idx'], c.n
    cut = lambda t: t[idx][:, :n]   # noqa: E731
    actions = cut(tr['actions_f'] if c.cont else tr['actions'])
    rewards = R.shift_right(cut(tr['rewards']), 0.)
    swr = torch.cat((cut(tr['states']), rewards[..., None]), dim=-1).double()
    swr = (swr - ins['rs_mean'].double()) / ins['rs_var'].double().sqrt().clamp(min=1e-5)
    lens = ins['lens'][idx]
    mask = torch.arange(n)[None] < lens[:, None]
    return dict(action=actions, prev_action=R.shift_right(actions, 0. if c.cont else -1), old_logp=cut(tr['logp']),
                returns=ins['returns'][idx], old_values=cut(tr['values']), dones=cut(tr['bounds']), lens=lens, swr=swr,
                rs_m=swr[mask].mean(0), swr_max=swr[mask].abs().amax(0))


def rsnorm_update_reference(mean, var, m, t):
    """The statistics update of RSNormState.train_call (xtrl.py:602-610) in fp64."""
    st = R.RSNormState(mean.numel(), step=t, mean=mean.double(), var=var.double())
    st.train_call(torch.zeros(1, mean.numel(), dtype=torch.float64), allreduce_mean=lambda _: m.double())
    return st.mean, st.var


# ----------------------------------------------------------------------------------------------
# AdoptAtan2
# ----------------------------------------------------------------------------------------------

ADOPT_SIZES = [1, 255, 257, 1023, 1025, 2047, 2049, 5000]
ADOPT_ZERO_SEG = 2          # this segment's gradient is all zero
ADOPT_LR = 8e-4
# option rows: (id, optimiser options, lr / init_lr, max_norm of the clip or None)
ADOPT_ROWS = [
    ('defaults', dict(cautious=0.1, regen=1e-4, wd=0.), 1., 0.5),
    ('no_cautious_count', dict(cautious=1., regen=1e-4, wd=0.), 1., 0.5),
    ('zero_cautious_factor', dict(cautious=0., regen=1e-4, wd=0.), 1., 0.5),
    ('weight_decay', dict(cautious=0.1, regen=1e-4, wd=0.01), 1., 0.5),
    ('no_regen', dict(cautious=0.1, regen=0., wd=0.), 1., 0.5),
    ('decayed_lr', dict(cautious=0.1, regen=1e-4, wd=0.), 0.5, 0.5),
    ('no_clip', dict(cautious=0.1, regen=1e-4, wd=0.), 1., None),
]


def adopt_grads(step):
    """The gradients of one step: exact zeros sprinkled in, one all-zero segment; step 2 is large,
    so its clip coefficient is below 1 (the others clip at exactly 1)."""
    g = torch.Generator().manual_seed(77 + step)
    out = []
    for k, s in enumerate(ADOPT_SIZES):
        gr = torch.randn(s, generator=g) * (3. if step == 2 else 0.002)
        gr[torch.rand(s, generator=g) < 0.1] = 0.
        if k == ADOPT_ZERO_SEG:
            gr.zero_()
        out.append(gr)
    return out


def adopt_params():
    g = torch.Generator().manual_seed(5)
    return [torch.randn(s, generator=g) for s in ADOPT_SIZES]
