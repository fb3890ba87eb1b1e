"""Seeded inputs, case tables, fp64 references and bounds for the kernels of the decode step (csrc/decode.hip), one
launch at a time through xtrl_decode_op (ABI 32) and the one-launch entries beside it (xtrl_rollout_begin,
xtrl_rollout_env_feedback, xtrl_sim_reset): compaction + embedding, attention decode with its fused out-projection
tails, the one-launch feed-forward, the three head paths with the sampling + Sim step (discrete and continuous), the
split-output projection, the small row kernels, and the row-resident step (one launch of xtrl_decode_step_rows on a
pre-filled state, against the composition of the references of the other families).

Imported by test_decode_kernels_cpu.py (which settles the bounds against the fp32 restatement and the dispatch naming
without a GPU) and by test_decode_kernels_gpu.py (which runs the kernels).  Plain PyTorch / numpy on the CPU; defines
no tests.  Region / verify / padded / guarded are learn_row_cases' own.

A case is a `DSpec`: the buffers of one call (every buffer 2-D; outputs with their prefill), the XtrlDecodeDesc /
XtrlDecodeLayer (and XtrlFractalDesc) fields as scalars or buffer names, the call (op, layer, t, args), the kernel
form the host dispatch is expected to pick, and `expect(dtype)`: the regions the call owns with their references in
`dtype` and their bounds.  expect(float64) is the reference; expect(float32) is the same arithmetic carried out in
fp32 from the same inputs (every intermediate rounded to fp32, sums taken element after element, the split-bf16
products as their six piece products): the restatement the bounds are settled against.  A case builds its own
descriptor over its own buffers; no RolloutEngine.

Layout and poison.  The live rows are a strict, non-identity subset of the slots (slot 0 is never live unless E == 1),
so row index r != slot e; live_rows entries past the count hold a stale in-range slot; the other parity's half of
live_rows / live_count must keep its bits.  Outputs are NaN before the call (in-place rows: seeded values); rows past
the live count, guard rows, cache rows other than position t and the caches of dead slots and of non-owner heads
must keep their bits.  Cache rows at positions > t and, under a window, < t - W hold NaN; rows of q|k|v and of the
other per-row inputs past the live count hold 1e30; mlp_part / heads_part hold NaN.  The weight sources handed to the
library's packers carry four padding columns of 1e30 past K; b_h2 and w_h2_t keep the zero padding the header defines.

Bounds (none is taken from the kernels).
  element-wise outputs (embedding rows, GLU, the new K / V rows, mixed values): 1e-5 + 1e-5 |ref|.  A rotated
      channel adds 2 x 2^-24 theta (|x_c| + |x_partner|), theta = t inv_freq: the fp32 product t inv_freq is itself
      rounded (at t = 257 an angle of 257 rad carries 1.5e-5 rad of rounding, more than the bound's 1e-5).
  LayerNorm rows of the embedding: the same with the absolute part times max(1, rstd[m]).
  composite outputs: C x unit, the unit a propagation of 2^-24 through the reference's own quantities (below), C four
      times the worst error of the fp32 restatement over the family's table, in those units, rounded up (the kernels sum
      in another order than the restatement: gemm_epi_cases, learn_row_cases).  A later stage takes the earlier
      stage's bound, constant included, as its input's unit.
        attention output o[h][c]:   u_o = 2^-24 (1 + s_abs) (sum_j p_j |v_jc| sigmoid(gate) + |o_c|),
            s_abs = max_j [ scale sum_i |q_i| (1 + theta_i) |k_ji| + slope (t - j) ]   (the score's own magnitude: an
            absolute score error e moves every probability by a relative e; a rotated channel counts its pair, a mixed
            value |v| + |v1|)
        fused out-projection row y = x + o W_out^T:   u_y = sum_hc (C_o u_o) |W| + 2^-24 (|x| + sum_hc |o| |W|)
        a LayerNorm of a row with unit u:   u' = rstd |g| (u + max_n u (1 + |xhat|)) + 2^-24 (|out| + |bias|)
        split-bf16 feed-forward s = res + b2 + GELU(xn W1^T + b1) W2^T:   u_h = 4 x 2^-24 (|b1| + sum |xn| |W1|)
            max(1, |gelu'|) + 2^-24 |h| (the three dropped piece products are each below 2^-24 of their term),
            u_s = sum u_h |W2| + 4 x 2^-24 sum |h| |W2| + 2^-24 (|res| + |b2| + |s|)
        projection (PROJ): 2^-24 (|bias| + sum |a| |w|) max(1, |act'|) + 2^-24 (|out| + |R|), a LayerNorm prologue
            entering through the LayerNorm rule
        heads: hidden u_h = (4 x with the split-bf16 product) 2^-24 (|b1| + sum |a| |W1|) max(1, |silu'|) + 2^-24 |h|,
            logits u_l = sum (C_h u_h) |W2| + 2^-24 (|b2| + sum |h| |W2| + |out|); with b_l the logits' bound of the row,
            logp of the sampled action 2 max b_l + 2^-24 (A + |logp|); continuous: sd's unit sd b_l / 2, the pre-tanh
            value's b_l + |z| u_sd, the action's 2 (1 - a^2) x that, logp the propagated Gaussian terms plus the
            conditioning 2 |a| / (1 - a^2) x the action's unit (and 1 - a a itself rounded: 4 x 2^-24 / (1 - a^2))
        fractal row kernels: the LayerNorm rule from 2^-24 |inputs|; sums / mean / next input add 2^-24 |terms|
  copies, integer lists, alive bytes, counters, Philox draws and the env-feedback bookkeeping: exact.

Constants and the restatement's worst error (test_decode_kernels_cpu.py::
test_fp32_restatement_within_a_quarter_of_each_bound prints them, pytest -s; worst over every case):
  family       restatement error / unit     C     restatement / bound
  attn_o       4.19  (the 'spread' regime)  17    0.25
  attn_y       0.005                        1     0.005
  attn_norm    0.009                        1     0.009  (the attention's xn / post-norm rows and the feed-forward's)
  fr_ln        0.67                         3     0.22
  mlp          0.021                        1     0.021
  proj         0.57                         3     0.19
  heads_h      0.78  (the hidden row)       4     0.19
  heads        0.19  (logits, critic)       1     0.19
  heads_lp     0.05                         1     0.05
  heads_act    0.007                        1     0.007
  row_kv       1.54  (row step: K / V / v1)  7     0.22   the row step's units are the bare-sum form at the last stage of
  row_out      1.44  (row step: logits)      6     0.24   each output (section 8): a worst-case propagation through a whole
  row_lp       0.08                          1     0.08   row grows by 1e7 and bounds nothing
Sampled action at a tie: compared exactly unless the Philox uniform lies within A x the probability bound (from the
fp64 cdf) of a cdf step; then either neighbour is accepted and logp / reward / prev_action are held to the action the
kernel took.  At most 2 % of a case's rows (TIE_CAP) may be excused; the CPU test asserts it from the reference alone
(HeadsCase.seed moves the Philox seed where a case's own draws do not pass).
  element-wise, restatement as a share of the bound: embed x 0.04, state embed 0.03, xn 0.02; new K rows 0.21 (the
  angle term at t = 257), new V rows 0.02; GLU 0.04.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch

from gemm_epi_cases import BIG, EPS24, NAN, _gen, bits, fwd_bound, ln_rows   # noqa: F401  (bits: re-exported)
from learn_row_cases import ISENT, Region, guarded, nan_out, padded, seqsum, verify   # noqa: F401  (re-exported)

OPS = ('EMBED', 'ATTN', 'MLP', 'HEADS', 'PROJ', 'GLU', 'FR_LN12', 'FR_LN3_TAIL', 'COPY_ROWS')
OP = {name: i for i, name in enumerate(OPS)}
EPI = dict(NONE=0, GELU=1, SILU=2, RELU=8)

# constants of the composite bounds: 4 x the fp32 restatement's worst error in the family's units, rounded up
# (module docstring; settled by test_decode_kernels_cpu.py before any kernel ran)
C_COMP = dict(attn_o=17., attn_y=1., attn_norm=1., fr_ln=3., mlp=1., proj=3., heads_h=4., heads=1., heads_lp=1., heads_act=1., row_kv=7., row_out=6., row_lp=1.)
EMB_MAX_E, EMB_LDS_FLOATS, EMB_AREG, MLP_HW = 8192, 8192, 8, 128


@dataclass
class DSpec:
    id: str
    op: str                       # an OPS name, or 'ENV_FEEDBACK' / 'ROLLOUT_BEGIN' / 'SIM_RESET' / 'STEP_ROWS'
    bufs: dict                    # name -> CPU tensor [R][C] as uploaded (outputs: their prefill)
    outs: tuple                   # names of the buffers the call may write
    desc: dict                    # XtrlDecodeDesc field -> scalar, or buffer name for a pointer field
    layers: list                  # per layer: XtrlDecodeLayer field -> buffer name
    t: int = 0
    layer: int = 0
    fractal: dict | None = None   # XtrlFractalDesc: scalars / buffer names, 'level': [XtrlFractalLevel dicts]
    in_: tuple = ()               # XtrlDecodeOpArgs
    out: tuple = ()
    ld: tuple = ()
    n: tuple = ()
    call: dict = field(default_factory=dict)   # arguments of the direct entries
    form: str = ''                # the kernel instantiation(s) the host dispatch is expected to launch
    expect: object = None         # dtype -> [Region]
    info: dict = field(default_factory=dict)


def rnd(g, *shape, scale=1.):
    return torch.randn(*shape, generator=g) * scale


def gain(g, d):
    return torch.rand(d, generator=g) * 0.5 + 0.75


def row(v):
    return v.reshape(1, -1)


def live_slots(E, n_live, g):
    """n_live of the E slots in increasing order, slot 0 dead (E > 1): row r is never slot r."""
    if E == 1:
        return torch.zeros(1, dtype=torch.int64)
    return (torch.randperm(E - 1, generator=g)[:n_live] + 1).sort().values


def live_bufs(E, t, slots, g):
    """live_rows [2][E] / live_count [1][2] as the step's compaction leaves them for parity t & 1: the slots, then
    stale in-range entries; the other parity holds another (stale) list."""
    rows = torch.randint(0, E, (2, E), generator=g, dtype=torch.int32)
    rows[t & 1, :len(slots)] = slots.to(torch.int32)
    cnt = torch.tensor([[3, 3]], dtype=torch.int32).clamp(max=E)
    cnt[0, t & 1] = len(slots)
    return rows, cnt


def ln_unit(u, xhat, rstd, g, out, bias=None):
    """The unit of a LayerNorm row whose input carries the unit u (module docstring)."""
    b = 0. if bias is None else bias.abs()
    return rstd[:, None] * g.abs() * (u + u.max(-1, keepdim=True).values * (1 + xhat.abs())) + EPS24 * (out.abs() + b)


def ln_bound(ref, rstd):
    """The project's LayerNorm-row bound: 1e-5 max(1, rstd[m]) + 1e-5 |ref|."""
    return 1e-5 * rstd.double().clamp_min(1.)[:, None] + 1e-5 * ref.double().abs()


def affine_ln(x, g, b, eps):
    """nn.LayerNorm in x's precision: (out, xhat, rstd)."""
    mean = x.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    xh = (x - mean) * rstd
    return xh * g + b, xh, rstd.squeeze(-1)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752))


def comp_region(buf, ref, unit, fam, **kw):
    return Region(buf, ref, C_COMP[fam] * unit.double(), fam=fam, unit=unit.double(), **kw)


# ----------------------------------------------------------------------------------------------
# the host dispatch, restated (launch_embed, attn_fused, decode_attn_form, launch_attn_decode, mlp_fused,
# launch_mlp_rows, heads_fused, decode_heads, dg_ks / dispatch_dg)
# ----------------------------------------------------------------------------------------------

def embed_form(E, d):
    nc = {1: 1, 2: 2, 3: 3, 4: 4}.get((d + 63) // 64, 8)
    return f'k_embed<{nc},true>' if E <= EMB_MAX_E else f'k_compact+k_embed<{nc},false>'


def attn_fused(H, dh, d, Tmax, w_out_t):
    lds = (H * (Tmax + 3 * dh) + H * d) * 4
    return bool(w_out_t and dh == 16 and H <= 8 and d % 4 == 0 and d <= 512 and d <= 256 * H and lds <= 160 * 1024)


def decode_attn_form(cap, alibi, sinks):
    return 'CLAMP' if cap else 'ALIBI' if alibi else 'SINK' if sinks else 'PLAIN'


FORM_FLAGS = dict(PLAIN='false,false,false', SINK='true,false,false', ALIBI='true,true,false', CLAMP='true,true,true')


def attn_kernel(H, dh, d, Tmax, w_out_t, cap, alibi, sinks):
    fj = (2 if d > 256 else 1) if attn_fused(H, dh, d, Tmax, w_out_t) else 0
    return f'k_attn_decode<{dh},{fj},{FORM_FLAGS[decode_attn_form(cap, alibi, sinks)]}>'


def dg_ks(N, K):
    return 2 if (K >= 768 and N < 512) else 1


def dgemm_kernel(N, K, epi, ln, res):
    mt, ks = (2, 1) if (N >= 512 and 32 * (((K + 15) & ~15) + 4) * 4 <= 80 * 1024) else (1, dg_ks(N, K))
    return f"k_dgemm<{mt},1,{ks},{epi},{'true' if ln else 'false'},{'true' if res else 'false'}>"


def mlp_fused(d, ff, images, xn, part_cnt, ff_glu, attn_is_fused):
    """mlp_fused of decode.hip: whether a decoder layer's feed-forward runs as the one launch."""
    return bool(not ff_glu and xn and part_cnt and images and attn_is_fused and d % 64 == 0 and d <= 256 and ff % MLP_HW == 0)


def mlp_kernel(d, fi):
    return f"k_mlp<{min(d // 64, 4)},{'true' if fi else 'false'}>"


# ----------------------------------------------------------------------------------------------
# 1. compaction + embedding (launch_embed)
# ----------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class EmbedCase:
    E: int
    d: int
    S: int
    A: int
    cont: int = 0
    t: int = 0
    state_only: int = 0
    no_reward: int = 0
    evo: int = 0
    bpin: int = 1
    ln: int = 0          # g_ln0 / xn
    rms: int = 0

    @property
    def id(self):
        return (f"embed-E{self.E}-d{self.d}-S{self.S}-A{self.A}{'c' if self.cont else ''}-t{self.t}-so{self.state_only}"
                f"-nr{self.no_reward}-evo{self.evo}-bp{self.bpin}-ln{self.ln}-rms{self.rms}")


def _embed_cases():
    out = []
    k = 0
    for d in (36, 128, 132, 256, 260, 512):
        for S in (1, 8, 17, 63):
            A, cont = [(1, 0), (8, 0), (9, 0), (32, 0), (3, 1)][k % 5]
            E = (1, 15, 16, 17, 40)[k % 5]
            out.append(EmbedCase(E, d, S, A, cont, t=k % 2, state_only=int(k % 7 == 3), no_reward=int(k % 7 == 5),
                                 evo=int(k % 3 == 1), bpin=int(k % 4 != 2), ln=int(k % 3 != 0), rms=int(k % 2 and k % 3 != 0)))
            k += 1
    for A, cont in ((1, 0), (8, 0), (9, 0), (32, 0), (6, 1)):     # every action form at both table homes, both parities
        for d in (128, 260):
            out.append(EmbedCase(17, d, 8, A, cont, t=(A + d // 4) % 2, ln=1, rms=A % 2, evo=cont))
    for E in (1, 15, 16, 17, 1025, 8192, 8200):                   # the large E at d = 36, S = 1
        out.append(EmbedCase(E, 36, 1, 4, t=E % 2, ln=int(E % 3 == 0)))
    for d in (128, 132, 256, 260):                                # k_compact + k_embed<NC, false> at every NC
        out.append(EmbedCase(8200, d, 1, 4, t=(d // 4) % 2, ln=1, rms=(d // 128) % 2))
    return out


EMBED_CASES = _embed_cases()


def embed_spec(c: EmbedCase):
    E, d, S, A, t = c.E, c.d, c.S, c.A, c.t
    g = _gen(31, E, d, S, A, c.cont, t)
    Tmax = t + 2
    in_dim = (3 if c.evo else 2) * d
    # alive bytes drawn from {0, 1, 2, 3, 4}; slot 0 dead; at most 40 live slots when E is large (small buffers' worth
    # of reference), slot E - 1 live
    al = torch.randint(0, 5, (E,), generator=g, dtype=torch.uint8)
    if E > 64:
        keep = torch.zeros(E, dtype=torch.bool)
        keep[torch.randperm(E, generator=g)[:40]] = True
        live_val = al.clone()
        dead_val = torch.where(al == 3 + (t & 1), torch.zeros_like(al), al)
        dead_val = torch.where((dead_val == 1) | (dead_val == 2), torch.zeros_like(al), dead_val)
        al = torch.where(keep, live_val, dead_val)
        al[E - 1] = 1
    if E > 1:
        al[0] = (0, 3 + ((t + 1) & 1))[E % 2]
    else:
        al[0] = 1
    live = (al == 1) | (al == 2) | (al == 3 + (t & 1))
    slots = live.nonzero().flatten()
    n = len(slots)
    al_after = torch.where(al == 3 + ((t + 1) & 1), torch.zeros_like(al), al)
    B = dict(alive=row(al).clone(), state=rnd(g, E, S), prev_reward=rnd(g, E, 1),
             rs_mean=row(rnd(g, S + 1, scale=0.3)), rs_var=row(torch.rand(S + 1, generator=g) * 1.5 + 0.5),
             w_pin=rnd(g, d, S, scale=1 / math.sqrt(S)), b_pin=row(rnd(g, d)), reward_embed=row(rnd(g, d)),
             w_se=rnd(g, d, S, scale=1 / math.sqrt(S)), b_se=row(rnd(g, d)), ln0=row(gain(g, d)))
    B['rs_var'][0, S // 2] = 0.04     # sqrt(var) = 0.2 < rs_eps: the clamp decides
    rs_eps = 0.5
    if c.cont:
        B['act_emb'] = rnd(g, d, A, scale=1 / math.sqrt(A))
        B['act_emb_b'] = row(rnd(g, d))
        B['prev_action_f'] = rnd(g, E, A)
        B['prev_action'] = torch.full((E, 1), ISENT, dtype=torch.int32)
    else:
        B['act_emb'] = rnd(g, A, d)
        B['prev_action'] = torch.randint(-1, A, (E, 1), generator=g, dtype=torch.int32)
        if n:
            B['prev_action'][slots[0]] = -1
            B['prev_action'][slots[-1]] = A - 1
    if c.evo:
        B['lat_embed'] = rnd(g, E, d)
    stale = torch.randint(0, E, (2, E), generator=g, dtype=torch.int32)
    B.update(live_rows=stale, live_count=torch.tensor([[ISENT, ISENT]], dtype=torch.int32),
             traj_states=torch.full((E * Tmax + 2, S), NAN), x=nan_out(E, d), ac_in=nan_out(E, in_dim))
    outs = ['alive', 'live_rows', 'live_count', 'traj_states', 'x', 'ac_in']
    if c.ln:
        B['xn'] = nan_out(E, d)
        outs.append('xn')
    desc = dict(E=E, S=S, A=A, B=4, d=d, L=1, H=1, dh=16, Tmax=Tmax, ff=128, in_dim=in_dim, n_qkv=48,
                continuous=c.cont, evolutionary=c.evo, state_only=c.state_only, no_reward_cond=c.no_reward,
                rs_eps=rs_eps, rms_norm=c.rms, w_pin='w_pin', b_pin='b_pin' if c.bpin else None, act_emb='act_emb',
                act_emb_b='act_emb_b' if c.cont else None, reward_embed='reward_embed', w_se='w_se', b_se='b_se',
                rs_mean='rs_mean', rs_var='rs_var', state='state', prev_action='prev_action',
                prev_action_f='prev_action_f' if c.cont else None, prev_reward='prev_reward', alive='alive',
                traj_states='traj_states', x='x', ac_in='ac_in', xn='xn' if c.ln else None, live_rows='live_rows',
                live_count='live_count', lat_embed='lat_embed' if c.evo else None)
    layers = [dict(ln_attn='ln0')]

    def expect(dt):
        st = B['state'][slots].to(dt)
        xv = torch.cat([st, B['prev_reward'][slots].to(dt)], 1)
        den = torch.sqrt(B['rs_var'].to(dt)).clamp_min(torch.tensor(rs_eps, dtype=torch.float32).to(dt))
        ns = (xv - B['rs_mean'].to(dt)) / den
        p = seqsum(ns[:, None, :S] * B['w_pin'].to(dt)[None], 2)
        se = seqsum(ns[:, None, :S] * B['w_se'].to(dt)[None], 2) + B['b_se'].to(dt)
        if c.bpin:
            p = p + B['b_pin'].to(dt)
        if c.cont:
            ak = seqsum(B['prev_action_f'][slots].to(dt)[:, None, :] * B['act_emb'].to(dt)[None], 2) + B['act_emb_b'].to(dt)
        else:
            a = B['prev_action'][slots, 0].long()
            ak = B['act_emb'].to(dt)[a.clamp_min(0)] * (a >= 0).to(dt)[:, None]
        if c.state_only:
            ak = torch.zeros_like(ak)
        rew = ns[:, S:S + 1] * B['reward_embed'].to(dt)
        if c.no_reward or c.state_only:
            rew = torch.zeros_like(rew)
        x = p + (ak + rew)
        rows_after = B['live_rows'].clone()
        rows_after[t & 1, :n] = slots.to(torch.int32)
        R = [Region('alive', row(al_after), None), Region('live_rows', rows_after[t & 1:(t & 1) + 1, :n], None, r0=t & 1),
             Region('live_count', torch.tensor([[n]], dtype=torch.int32), None, c0=t & 1),
             Region('x', x, fwd_bound(x.double())), Region('ac_in', se, fwd_bound(se.double()), c0=d)]
        for i, e in enumerate(slots.tolist()):
            R.append(Region('traj_states', B['state'][e:e + 1], None, r0=e * Tmax + t))
        if c.evo:
            R.append(Region('ac_in', B['lat_embed'][slots], None, c0=2 * d))
        if c.ln:
            xh, _, rstd = ln_rows(x, c.rms)
            xn = xh * B['ln0'].to(dt)
            R.append(Region('xn', xn, ln_bound(xn, rstd), fam='layernorm'))
        return [r for r in R if r.ref.numel()]

    return DSpec(c.id, 'EMBED', B, tuple(outs), desc, layers, t=t, n=(c.ln,), form=embed_form(E, d), expect=expect,
                 info=dict(n_live=n))


# ----------------------------------------------------------------------------------------------
# 2. attention decode (launch_attn_decode): plain / sink / ALiBi / soft-clamp forms, the fused out-projection tails
# ----------------------------------------------------------------------------------------------

HEADS = [(4, 4, 16), (4, 2, 16), (8, 1, 16), (3, 1, 32), (5, 5, 32), (1, 1, 64), (2, 2, 64), (9, 3, 16)]


def ck_of(dh):
    return 128 if dh <= 32 else 64


@dataclass(frozen=True)
class AttnCase:
    H: int
    Hkv: int
    dh: int
    t: int
    W: int = 0
    d: int = 36
    tail: str = 'att'        # 'att' (w_out_t NULL), 'x' (fused, no xn), 'xn' (fused + FF1's pre-norm), 'post0' / 'postd'
    rms: int = 0
    layer: int = 0
    vres: int = 0            # value residual (layer 0: stores v1; layer 1: learned mix)
    gate: int = 0
    qkn: int = 0
    rot: int = 0             # rotary_abs
    xpos: float = 0.
    M: int = 0               # memory rows
    zkv: int = 0
    alibi: int = 0           # 0 none, 1 every head, 2 the first half of the heads (the others slope 0)
    cap: float = 0.
    regime: str = 'o1'       # 'o1', 'spread', 'sink'

    @property
    def id(self):
        return (f'attn-H{self.H}k{self.Hkv}dh{self.dh}-t{self.t}-W{self.W}-d{self.d}-{self.tail}-rms{self.rms}-l{self.layer}'
                f'-vr{self.vres}-g{self.gate}-qkn{self.qkn}-rot{self.rot}-xp{self.xpos:g}-M{self.M}-z{self.zkv}'
                f'-al{self.alibi}-cap{self.cap:g}-{self.regime}')


def _attn_cases():
    out = []
    k = 0
    # (a) every head shape x every t x every window, not fused; the options cycle through the table
    for (H, Hkv, dh) in HEADS:
        CK = ck_of(dh)
        for t in (0, 1, CK - 1, CK, CK + 1, 2 * CK + 1):
            for W in (0, 1, 63, CK, CK + 2):
                sink = (k // 2) % 4
                out.append(AttnCase(H, Hkv, dh, t, W, layer=k % 2, vres=int(k % 3 != 0), gate=int(k % 2 == 0), qkn=int(k % 5 == 1),
                                    rot=int(k % 3 != 1), xpos=(0., 512.)[(k // 3) % 2], M=(0, 1, 16, 0)[sink],
                                    zkv=int(sink == 3 or k % 7 == 0), alibi=(0, 0, 1, 2)[k % 4],
                                    cap=(0., 0., 0., 2.5, 0., 30.)[k % 6], regime=('o1', 'o1', 'spread', 'sink')[(k // 5) % 4]))
                k += 1
    # (b) the fused tails: d x tail x norm at the chunk edges, every form
    for (H, Hkv, dh) in HEADS[:3]:
        for d in (36, 256, 260, 512):
            for tail in ('att', 'x', 'xn', 'post0', 'postd'):
                for t, W in ((0, 0), (127, 0), (129, 63), (257, 130)):
                    fr = tail.startswith('post')
                    if fr and Hkv != H:
                        continue          # (the fractal body: n_qkv = 3 I)
                    form = k % 4
                    out.append(AttnCase(H, Hkv, dh, t, W, d=d, tail=tail, rms=int(tail == 'xn' and k % 2), layer=0 if fr else k % 2,
                                        vres=0 if fr else k % 2, gate=0 if fr else int(k % 3 == 0), rot=0 if fr else int(k % 2 == 0),
                                        M=(0, 4, 0, 16)[form], zkv=int(form == 1), alibi=int(form >= 2),
                                        cap=5. if form == 3 else 0., regime=('o1', 'sink', 'o1', 'spread')[form]))
                    k += 1
    for t, W, d in ((129, 0, 36), (257, 130, 260)):     # H > 8 with w_out_t set: not fused, the output goes to att
        out.append(AttnCase(9, 3, 16, t, W, d=d, tail='attw', rot=1, M=4, alibi=1))
    return out


ATTN_CASES = _attn_cases()
ATTN_E, ATTN_LIVE = 7, 5


def attn_spec(c: AttnCase):
    H, Hkv, dh, t, d = c.H, c.Hkv, c.dh, c.t, c.d
    E, nl = ATTN_E, ATTN_LIVE
    I, Ikv = H * dh, Hkv * dh
    Tmax = t + 3
    g = _gen(37, H, Hkv, dh, t, c.W, d, len(c.tail), c.layer, c.M, c.alibi)
    mix = c.vres and c.layer > 0
    n_qkv = I + 2 * Ikv + (I if c.gate else 0) + (Hkv if c.vres else 0)
    slots = live_slots(E, nl, g)
    rows, cnt = live_bufs(E, t, slots, g)
    j_lo = max(t - c.W, 0) if c.W > 0 else 0
    rot_dim = dh // 2
    qs = dict(o1=1., spread=40., sink=1.)[c.regime]
    qkv = rnd(g, nl, n_qkv)
    qkv[:, :I] *= qs
    if c.gate:
        qkv[:, I + 2 * Ikv:I + 2 * Ikv + I] *= 2.
    if c.vres:
        qkv[:, -Hkv:] = torch.linspace(-20., 20., nl * Hkv).reshape(nl, Hkv)   # pre-sigmoid mix out to +-20
    B = dict(qkv=guarded(qkv, E - nl + 2, BIG), live_rows=rows, live_count=cnt,
             inv_freq=row(1.0 / (10000. ** (torch.arange(0, rot_dim, 2).float() / rot_dim))))
    kc = torch.full((E, Hkv, Tmax, dh), NAN)
    vc = torch.full((E, Hkv, Tmax, dh), NAN)
    kc[slots, :, j_lo:t] = rnd(g, nl, Hkv, t - j_lo, dh)
    vc[slots, :, j_lo:t] = rnd(g, nl, Hkv, t - j_lo, dh)
    B['k_cache'], B['v_cache'] = kc.reshape(-1, dh), vc.reshape(-1, dh)
    outs = ['k_cache', 'v_cache']
    layer = dict(k_cache='k_cache', v_cache='v_cache')
    desc = dict(E=E, S=4, A=4, B=4, d=d, L=2, H=H, dh=dh, Tmax=Tmax, ff=128, in_dim=2 * d, n_qkv=n_qkv, Hkv=Hkv,
                gate_values=c.gate, value_residual=c.vres, learned_mix=c.vres, rotary_abs=c.rot, rot_dim=rot_dim,
                qk_norm=c.qkn, attn_scale=8. if c.qkn else 0., xpos_base=c.xpos, rms_norm=c.rms, attn_window=c.W,
                attn_softclamp=c.cap, num_mem_kv=c.M, add_zero_kv=c.zkv, qkv='qkv', inv_freq='inv_freq',
                live_rows='live_rows', live_count='live_count')
    if c.vres:
        B['v1'] = guarded(rnd(g, nl, Ikv), E - nl + 2, NAN) if c.layer else nan_out(E, Ikv)
        desc['v1'] = 'v1'
        if c.layer == 0:
            outs.append('v1')
    if c.M:
        ms = 6. if c.regime == 'sink' else 1.
        B['mem_k'], B['mem_v'] = rnd(g, Hkv * c.M, dh, scale=ms), rnd(g, Hkv * c.M, dh)
        layer.update(mem_k='mem_k', mem_v='mem_v')
    if c.alibi:
        sl = 2. ** -(8. * (torch.arange(H).float() + 1) / H)
        if c.alibi == 2:
            sl[(H + 1) // 2:] = 0.
        B['alibi'] = row(sl)
        desc['alibi_slopes'] = 'alibi'
    fused = c.tail not in ('att', 'attw')     # 'attw': w_out_t present but the shape (H > 8) is not fused
    fr = c.tail.startswith('post')
    fractal = None
    if fused:
        B['w_out_t'] = rnd(g, I, d, scale=1 / math.sqrt(I))
        layer['w_out_t'] = 'w_out_t'
        B['ln_ff'] = row(gain(g, d))
        layer['ln_ff'] = 'ln_ff'
        xold = torch.cat([rnd(g, nl, d), rnd(g, E - nl + 2, d)])
        B['x'] = xold
        desc['x'] = 'x'
        outs.append('x')          # (the post-norm tails must leave it alone)
        if c.tail == 'xn':
            B['xn'] = nan_out(E, d)
            desc['xn'] = 'xn'
            outs.append('xn')
        if fr:
            desc.update(state_only=1)
            for nm in ('ln1_w', 'ln2_w'):
                B[nm] = row(gain(g, d))
            for nm in ('ln1_b', 'ln2_b'):
                B[nm] = row(rnd(g, d, scale=0.3))
            B.update(c0=row(rnd(g, d)), c2=guarded(rnd(g, nl, d), E - nl + 2, BIG), x2=nan_out(E, d), fdummy=torch.zeros(1, 4))
            lv = dict(ln1_w='ln1_w', ln1_b='ln1_b', ln2_w='ln2_w', ln2_b='ln2_b')
            fractal = dict(levels=2, ln_eps=1e-5, level=[lv, lv], g_init='fdummy', c0='c0', g='fdummy', c2='c2', tmp='fdummy',
                           x2='x2', mean='fdummy', allf='fdummy', hagg='fdummy')
            outs.append('x2')
    else:
        if c.tail == 'attw':
            B['w_out_t'], B['ln_ff'] = rnd(g, I, d, scale=1 / math.sqrt(I)), row(gain(g, d))
            layer.update(w_out_t='w_out_t', ln_ff='ln_ff')
        B['att'] = nan_out(E, I)
        desc['att'] = 'att'
        outs.append('att')
    lyr = 1 if (fr and c.tail == 'postd') else (0 if fr else c.layer)
    layers = [layer, layer]

    def expect(dt):
        f = lambda x: x.to(dt)   # noqa: E731
        rw = f(qkv)
        q = rw[:, :I].reshape(nl, H, dh)
        k = rw[:, I:I + Ikv].reshape(nl, Hkv, dh)
        v = rw[:, I + Ikv:I + 2 * Ikv].reshape(nl, Hkv, dh)
        R = []
        if c.vres and c.layer == 0:
            R.append(Region('v1', qkv[:, I + Ikv:I + 2 * Ikv], None))
        v_mag = v.abs()      # the new value's magnitude: a mixed value is a difference of |v| + |v1|
        if mix:
            v_mag = v_mag + f(B['v1'][:nl]).reshape(nl, Hkv, dh).abs()
            mv = rw[:, n_qkv - Hkv:].reshape(nl, Hkv, 1)
            w = 1.0 / (1.0 + torch.exp(-mv))
            v1 = f(B['v1'][:nl]).reshape(nl, Hkv, dh)
            v = torch.where(w.abs() < 0.5, v + w * (v1 - v), v1 - (v1 - v) * (1.0 - w))
        if c.qkn:
            q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
            k = k / k.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        theta = torch.zeros(dh, dtype=torch.float64)
        part = torch.arange(dh)
        part[:rot_dim] = part[:rot_dim] ^ 1
        if c.rot:
            ch = torch.arange(rot_dim)
            ang = torch.tensor(float(t), dtype=torch.float32).to(dt) * f(B['inv_freq'][0])[ch // 2]
            theta[:rot_dim] = ang.double().abs()
            cs, sn = torch.cos(ang), torch.sin(ang)
            sgn = torch.where(ch % 2 == 1, 1., -1.).to(dt)

            def rotate(x, inv):
                xr = x[..., :rot_dim]
                y = xr * cs + (sgn * xr[..., ch ^ 1]) * sn
                if c.xpos > 0:
                    base = ((ch & ~1).to(torch.float32).to(dt) + 0.4 * rot_dim) / (1.4 * rot_dim)
                    ex = torch.tensor(float(t - (t + 1) // 2), dtype=torch.float32).to(dt) / c.xpos
                    xf = base ** ex
                    y = y * (1.0 / xf if inv else xf)
                return torch.cat([y, x[..., rot_dim:]], -1)
            q, k = rotate(q, False), rotate(k, True)

        def kv_bound(x):   # the new cache rows: element-wise + the angle's own rounding
            xd = x.double()
            return fwd_bound(xd) + 2 * EPS24 * theta * (xd.abs() + xd[..., part].abs())
        for r, e in enumerate(slots.tolist()):
            for kh in range(Hkv):
                r0 = (e * Hkv + kh) * Tmax + t
                R.append(Region('k_cache', k[r, kh:kh + 1], kv_bound(k[r, kh:kh + 1]), r0=r0))
                R.append(Region('v_cache', v[r, kh:kh + 1], fwd_bound(v[r, kh:kh + 1].double()), r0=r0))
        # scores over the window's cached keys, the new key, the sinks
        kvh = torch.arange(H) % Hkv
        Kc = f(kc[slots][:, kvh, j_lo:t])                 # [nl][H][n][dh]
        Vc = f(vc[slots][:, kvh, j_lo:t])
        Kall = torch.cat([Kc, k[:, kvh, None]], 2)
        Vall = torch.cat([Vc, v[:, kvh, None]], 2)
        scale = torch.tensor(8. if c.qkn else 1.0 / math.sqrt(dh), dtype=torch.float32).to(dt)
        s = seqsum(q[:, :, None, :] * Kall, 3) * scale
        # magnitudes behind the rotated q and new k (a rotated channel is a sum of its pair), the angle's rounding on q
        q_mag = (q.abs() + (q.abs()[..., part] if c.rot else 0.)) * (1 + theta).to(dt) if c.rot else q.abs()
        k_mag = k.abs() + k.abs()[..., part] * (1 + theta).to(dt) if c.rot else k.abs()
        Kmag = torch.cat([Kc.abs(), k_mag[:, kvh, None]], 2)
        Vmag = torch.cat([Vc.abs(), v_mag[:, kvh, None]], 2)
        s_abs = seqsum(q_mag[:, :, None, :] * Kmag, 3).double() * float(scale)
        if c.alibi:
            dist = torch.arange(t - j_lo, -1, -1, dtype=torch.float32).to(dt)
            bias = f(B['alibi'][0])[None, :, None] * dist
            s = s - bias
            s_abs = s_abs + bias.double()
        if c.M:
            mk = f(B['mem_k']).reshape(Hkv, c.M, dh)[kvh]      # [H][M][dh]
            ms_ = seqsum(q[:, :, None, :] * mk[None], 3) * scale
            s_abs = torch.cat([s_abs, seqsum(q.abs()[:, :, None, :] * mk.abs()[None], 3).double() * float(scale)], 2)
            s = torch.cat([s, ms_], 2)
            mvv = f(B['mem_v']).reshape(Hkv, c.M, dh)[kvh][None].expand(nl, -1, -1, -1)
            Vall, Vmag = torch.cat([Vall, mvv], 2), torch.cat([Vmag, mvv.abs()], 2)
        if c.cap > 0:
            cap = torch.tensor(c.cap, dtype=torch.float32).to(dt)
            s = cap * torch.tanh(s * (1.0 / cap))
        if c.zkv:
            s = torch.cat([s, torch.zeros(nl, H, 1, dtype=dt)], 2)
            Vall, Vmag = (torch.cat([x, torch.zeros(nl, H, 1, dh, dtype=dt)], 2) for x in (Vall, Vmag))
        p = torch.exp(s - s.max(-1, keepdim=True).values)
        den = seqsum(p, 2)
        o = seqsum(p[..., None] * Vall, 2) / den[..., None]
        pv_abs = (seqsum(p[..., None] * Vmag, 2) / den[..., None]).double()
        gs = torch.ones_like(o)
        if c.gate:
            gs = 1.0 / (1.0 + torch.exp(-rw[:, I + 2 * Ikv:I + 2 * Ikv + I].reshape(nl, H, dh)))
            o = o * gs
        u_o = (EPS24 * (1 + s_abs.max(-1).values)[..., None] * (pv_abs * gs.double() + o.double().abs())).reshape(nl, I)
        o = o.reshape(nl, I)
        if not fused:
            R.append(comp_region('att', o, u_o, 'attn_o'))
            return R
        Wt = f(B['w_out_t'])
        parts = seqsum((o[:, :, None] * Wt[None]).reshape(nl, H, dh, d), 2)     # per head, channel after channel
        y = seqsum(torch.cat([f(B['x'][:nl])[:, None], parts], 1), 1)           # the residual, then the heads in order
        u_y = C_COMP['attn_o'] * u_o @ Wt.double().abs() + EPS24 * (B['x'][:nl].double().abs() + o.double().abs() @ Wt.double().abs())
        if c.tail in ('x', 'xn'):
            R.append(comp_region('x', y, u_y, 'attn_y'))
        if c.tail == 'xn':
            xh, _, rstd = ln_rows(y, c.rms)
            gff = f(B['ln_ff'])
            xn = xh * gff
            R.append(comp_region('xn', xn, ln_unit(C_COMP['attn_y'] * u_y, xh.double(), rstd.double(), gff.double(), xn.double()), 'attn_norm'))
        if fr:
            o1, xh1, r1 = affine_ln(y, f(B['ln1_w']), f(B['ln1_b']), 1e-5)
            u1 = ln_unit(C_COMP['attn_y'] * u_y, xh1.double(), r1.double(), B['ln1_w'].double(), o1.double(), B['ln1_b'].double())
            cx = f(B['c2'][:nl]) if lyr > 0 else f(B['c0']).expand(nl, -1)
            z = o1 + cx
            u1 = u1 + EPS24 * (o1.double().abs() + cx.double().abs())
            o2, xh2, r2 = affine_ln(z, f(B['ln2_w']), f(B['ln2_b']), 1e-5)
            u2 = ln_unit(u1, xh2.double(), r2.double(), B['ln2_w'].double(), o2.double(), B['ln2_b'].double())
            R.append(comp_region('x2', o2, u2, 'attn_norm'))
        return R

    form = attn_kernel(H, dh, d, Tmax, c.tail != 'att', c.cap > 0, c.alibi > 0, c.M > 0 or c.zkv)
    return DSpec(c.id, 'ATTN', B, tuple(outs), desc, layers, t=t, layer=lyr, fractal=fractal, form=form, expect=expect)


# ----------------------------------------------------------------------------------------------
# 3. small kernels: k_glu_rows, k_fr_ln12, k_fr_ln3_tail, k_copy_rows, k_env_feedback, k_rollout_begin, k_sim_reset
# ----------------------------------------------------------------------------------------------

SMALL_E, SMALL_LIVE = 9, 6


def base_desc(E, d, Tmax=4, **kw):
    """A descriptor that passes check_desc, with nothing but its shapes."""
    out = dict(E=E, S=4, A=4, B=4, d=d, L=1, H=4, dh=16, Tmax=Tmax, ff=128, in_dim=2 * d, n_qkv=192,
               live_rows='live_rows', live_count='live_count')
    out.update(kw)
    return out


def glu_spec(d, t):
    E, nl, ff = SMALL_E, SMALL_LIVE, d + 4
    g = _gen(41, d, t)
    slots = live_slots(E, nl, g)
    rows, cnt = live_bufs(E, t, slots, g)
    u = rnd(g, nl, 2 * ff, scale=2.)
    B = dict(live_rows=rows, live_count=cnt, hff=guarded(u, E - nl + 2, BIG), hglu=nan_out(E, ff))
    desc = base_desc(E, d, ff=ff, ff_glu=1, hff='hff', hglu='hglu')

    def expect(dt):
        ref = u[:, :ff].to(dt) * gelu(u[:, ff:].to(dt))
        return [Region('hglu', ref, fwd_bound(ref.double()))]
    return DSpec(f'glu-d{d}-t{t}', 'GLU', B, ('hglu',), desc, [dict()], t=t, form='k_glu_rows', expect=expect)


def _fractal(B, g, d, E, levels=2):
    """Level parameters and the buffers check_fractal asks for (those an op does not touch: one dummy)."""
    lvs = []
    for l in range(levels):
        q = {}
        for nm in ('ln1_w', 'ln2_w', 'ln3_w'):
            B[f'{nm}{l}'] = row(gain(g, d))
            q[nm] = f'{nm}{l}'
        for nm in ('ln1_b', 'ln2_b', 'ln3_b', 'level_emb'):
            B[f'{nm}{l}'] = row(rnd(g, d, scale=0.3))
            q[nm] = f'{nm}{l}'
        lvs.append(q)
    B['fdummy'] = torch.zeros(1, 4)
    return dict(levels=levels, ln_eps=1e-5, level=lvs, g_init='fdummy', c0='fdummy', g='fdummy', c2='fdummy', tmp='fdummy',
                x2='fdummy', mean='fdummy', allf='fdummy', hagg='fdummy')


def fr_desc(E, d, Tmax, **kw):
    return base_desc(E, d, Tmax, L=2, state_only=1, **kw)


def fr_ln12_spec(d, level, t):
    E, nl = SMALL_E, SMALL_LIVE
    g = _gen(43, d, level, t)
    slots = live_slots(E, nl, g)
    rows, cnt = live_bufs(E, t, slots, g)
    B = dict(live_rows=rows, live_count=cnt, x=guarded(rnd(g, nl, d), E - nl + 2, BIG), tmp=guarded(rnd(g, nl, d), E - nl + 2, BIG),
             c0=row(rnd(g, d)), c2=guarded(rnd(g, nl, d), E - nl + 2, BIG), x2=nan_out(E, d))
    F = _fractal(B, g, d, E)
    F.update(c0='c0', c2='c2', tmp='tmp', x2='x2')

    def expect(dt):
        f = lambda k: B[k].to(dt)   # noqa: E731
        x, o = f('x')[:nl], f('tmp')[:nl]
        v = x + o
        o1, xh1, r1 = affine_ln(v, f(f'ln1_w{level}'), f(f'ln1_b{level}'), 1e-5)
        u1 = ln_unit(EPS24 * (x.double().abs() + o.double().abs()), xh1.double(), r1.double(), B[f'ln1_w{level}'].double(),
                     o1.double(), B[f'ln1_b{level}'].double())
        cx = f('c2')[:nl] if level > 0 else f('c0').expand(nl, -1)
        z = o1 + cx
        o2, xh2, r2 = affine_ln(z, f(f'ln2_w{level}'), f(f'ln2_b{level}'), 1e-5)
        u2 = ln_unit(u1 + EPS24 * (o1.double().abs() + cx.double().abs()), xh2.double(), r2.double(),
                     B[f'ln2_w{level}'].double(), o2.double(), B[f'ln2_b{level}'].double())
        return [comp_region('x2', o2, u2, 'fr_ln')]
    return DSpec(f'fr_ln12-d{d}-l{level}-t{t}', 'FR_LN12', B, ('x2',), fr_desc(E, d, t + 2, x='x'), [dict(), dict()], t=t,
                 layer=level, fractal=F, form='k_fr_ln12', expect=expect)


def fr_tail_regions(B, dt, s3, u_s3, level, levels, t, slots, nl, d, sums_name):
    """x3 = LN3(s3), the slot's running sum, the row's running mean, the next level's input (k_fr_ln3_tail, k_mlp's FrMlp)."""
    f = lambda k: B[k].to(dt)   # noqa: E731
    x3, xh, r3 = affine_ln(s3, f(f'ln3_w{level}'), f(f'ln3_b{level}'), 1e-5)
    u3 = ln_unit(u_s3, xh.double(), r3.double(), B[f'ln3_w{level}'].double(), x3.double(), B[f'ln3_b{level}'].double())
    old = f(sums_name)[slots] if t > 0 else torch.zeros(nl, d, dtype=dt)
    sm = old + x3
    u_sm = u3 + EPS24 * (old.double().abs() + x3.double().abs())
    mean = sm / torch.tensor(float(t + 1), dtype=torch.float32).to(dt)
    R = [comp_region('mean', mean, u_sm / (t + 1) + EPS24 * mean.double().abs(), 'fr_ln')]
    for r, e in enumerate(slots.tolist()):
        R.append(comp_region(sums_name, sm[r:r + 1], u_sm[r:r + 1], 'fr_ln', r0=e))
    if level + 1 < levels:
        le = f(f'level_emb{level + 1}')
        xn = x3 + le
        R.append(comp_region('x', xn, u3 + EPS24 * (x3.double().abs() + le.double().abs()), 'fr_ln'))
    return R


def fr_ln3_spec(d, level, t):
    E, nl = SMALL_E, SMALL_LIVE
    g = _gen(47, d, level, t)
    slots = live_slots(E, nl, g)
    rows, cnt = live_bufs(E, t, slots, g)
    s3 = rnd(g, nl, d, scale=1.5)
    B = dict(live_rows=rows, live_count=cnt, tmp=guarded(s3, E - nl + 2, BIG), sums=guarded(rnd(g, E, d, scale=3.), 2, NAN),
             mean=nan_out(E, d), x=nan_out(E, d))
    F = _fractal(B, g, d, E)
    F.update(tmp='tmp', mean='mean')
    F['level'][level]['sums'] = 'sums'

    def expect(dt):
        return fr_tail_regions(B, dt, s3.to(dt), EPS24 * s3.double().abs(), level, 2, t, slots, nl, d, 'sums')
    return DSpec(f'fr_ln3_tail-d{d}-l{level}-t{t}', 'FR_LN3_TAIL', B, ('sums', 'mean', 'x'), fr_desc(E, d, t + 2, x='x'),
                 [dict(), dict()], t=t, layer=level, fractal=F, form='k_fr_ln3_tail', expect=expect)


def copy_rows_spec(d):
    E, Lv = SMALL_E, 2
    g = _gen(53, d)
    rows, cnt = live_bufs(E, 0, live_slots(E, SMALL_LIVE, g), g)
    gsrc = rnd(g, E, 2 * d)
    B = dict(live_rows=rows, live_count=cnt, g=guarded(gsrc, 2, BIG), allf=nan_out(E, (Lv + 1) * d))
    F = _fractal(B, g, d, E)
    F.update(g='g', allf='allf')

    def expect(dt):   # (every one of the E rows: the copy does not follow the live count)
        return [Region('allf', gsrc[:, :d], None, c0=Lv * d)]
    return DSpec(f'copy_rows-d{d}', 'COPY_ROWS', B, ('allf',), fr_desc(E, d, 4), [dict(), dict()], fractal=F, form='k_copy_rows',
                 expect=expect)


def small_specs():
    out = []
    for d in (36, 260, 512):
        out += [glu_spec(d, 0), glu_spec(d, 3)]
        out += [fr_ln12_spec(d, 0, 2), fr_ln12_spec(d, 1, 3)]
        out += [fr_ln3_spec(d, 0, 0), fr_ln3_spec(d, 0, 3), fr_ln3_spec(d, 1, 0), fr_ln3_spec(d, 1, 3)]
        out.append(copy_rows_spec(d))
    return out


def rng_buf(seed, update, slot_offset=0):
    return torch.tensor([[seed, update | (slot_offset << 32)]], dtype=torch.int64)


def env_feedback_spec(t, t_limit, Tmax, bootstrap, trunc_null):
    """One launch whose rows enumerate alive {0, 1, 2, 3, 4} x terminated x truncated."""
    S = 5
    combos = [(a, te, tr) for a in (0, 1, 2, 3, 4) for te in (0, 1) for tr in (0, 1)]
    E = len(combos)
    g = _gen(59, t, t_limit, Tmax, bootstrap, trunc_null)
    al = torch.tensor([c[0] for c in combos], dtype=torch.uint8)
    te = torch.tensor([c[1] for c in combos], dtype=torch.uint8)
    tr = torch.tensor([c[2] for c in combos], dtype=torch.uint8)
    B = dict(live_rows=torch.zeros(2, E, dtype=torch.int32), live_count=torch.zeros(1, 2, dtype=torch.int32), alive=row(al).clone(),
             terminated=row(te), truncated=row(tr), next_state=rnd(g, E, S), reward=rnd(g, E, 1), state=rnd(g, E, S),
             prev_reward=rnd(g, E, 1), cum_reward=rnd(g, E, 1).double() * 10, lens=torch.full((E, 1), ISENT, dtype=torch.int32),
             traj_rewards=torch.full((E, Tmax), NAN), traj_bounds=torch.full((E, Tmax), 7, dtype=torch.uint8))
    desc = base_desc(E, 36, Tmax, S=S, sim_mode=-1, alive='alive', state='state', prev_reward='prev_reward',
                     cum_reward='cum_reward', lens='lens', traj_rewards='traj_rewards', traj_bounds='traj_bounds')
    outs = ('alive', 'state', 'prev_reward', 'cum_reward', 'lens', 'traj_rewards', 'traj_bounds')

    def expect(dt):
        R = []
        after = al.clone()
        for e, (a, term, trunc) in enumerate(combos):
            trunc = trunc and not trunc_null
            if a == 2:
                after[e] = 0
            if a != 1:
                continue
            rw = B['reward'][e:e + 1]
            R += [Region('traj_rewards', rw, None, r0=e, c0=t), Region('prev_reward', rw, None, r0=e),
                  Region('traj_bounds', torch.tensor([[term]], dtype=torch.uint8), None, r0=e, c0=t),
                  Region('cum_reward', B['cum_reward'][e:e + 1] + rw.double(), None, r0=e),
                  Region('lens', torch.tensor([[t + 1]], dtype=torch.int32), None, r0=e),
                  Region('state', B['next_state'][e:e + 1], None, r0=e)]
            if term:
                after[e] = 0
            elif trunc and bootstrap and t + 1 < Tmax:
                after[e] = 2
            elif trunc or t + 1 >= t_limit:
                after[e] = 0
        R.append(Region('alive', row(after), None))
        return R
    return DSpec(f'env_feedback-t{t}-lim{t_limit}-T{Tmax}-b{bootstrap}-tn{trunc_null}', 'ENV_FEEDBACK', B, outs, desc, [dict()], t=t,
                 call=dict(next_state='next_state', reward='reward', terminated='terminated',
                           truncated=None if trunc_null else 'truncated', t_limit=t_limit, bootstrap=bootstrap),
                 form='k_env_feedback', expect=expect)


ENV_CASES = [(2, 6, 6, 1, 0), (2, 6, 6, 0, 0), (2, 6, 6, 1, 1), (4, 5, 6, 1, 0), (4, 5, 6, 0, 1), (5, 6, 6, 1, 0), (5, 6, 6, 0, 0),
             (0, 1, 2, 1, 0)]


def philox_states(seed, update, eps, t, S):
    from oracle import philox as PH
    return torch.from_numpy(np.stack([PH.philox_uniform(seed, update, int(e), t, PH.FIELD_STATE, S, normal=True) for e in eps]))


def rollout_begin_spec(E, S, cont, sim_mode, act_host, seed):
    A = 3
    g = _gen(61, E, S, cont, sim_mode + 1, act_host)
    eps = torch.randint(0, 1000, (E, 1), generator=g, dtype=torch.int32)
    ncnt = (E + 15) // 16
    B = dict(live_rows=torch.zeros(2, E, dtype=torch.int32), live_count=torch.zeros(1, 2, dtype=torch.int32),
             rng=rng_buf(seed, 5), episode_of_slot=eps, state=torch.full((E + 2, S), NAN),
             prev_action=torch.full((E + 2, 1), ISENT, dtype=torch.int32), prev_action_f=torch.full((E + 2, A), NAN),
             prev_reward=torch.full((E + 2, 1), NAN), alive=torch.full((1, E + 4), 9, dtype=torch.uint8),
             lens=torch.full((E + 2, 1), ISENT, dtype=torch.int32), cum_reward=torch.full((E + 2, 1), -7777.5, dtype=torch.float64),
             mlp_cnt=torch.full((1, ncnt + 2), 77, dtype=torch.int32),
             act_host=torch.full((E + 2, A), NAN) if cont else torch.full((E + 2, 1), ISENT, dtype=torch.int32))
    desc = base_desc(E, 36, 4, S=S, A=A, continuous=cont, sim_mode=sim_mode, rng='rng', episode_of_slot='episode_of_slot',
                     state='state', prev_action='prev_action', prev_action_f='prev_action_f', prev_reward='prev_reward',
                     alive='alive', lens='lens', cum_reward='cum_reward', mlp_cnt='mlp_cnt', act_host='act_host' if act_host else None)
    outs = ('state', 'prev_action', 'prev_action_f', 'prev_reward', 'alive', 'lens', 'cum_reward', 'mlp_cnt', 'act_host')

    def expect(dt):
        R = [Region('prev_action', torch.full((E, 1), -1, dtype=torch.int32), None), Region('prev_reward', torch.zeros(E, 1), None),
             Region('alive', torch.ones(1, E, dtype=torch.uint8), None), Region('lens', torch.zeros(E, 1, dtype=torch.int32), None),
             Region('cum_reward', torch.zeros(E, 1, dtype=torch.float64), None),
             Region('mlp_cnt', torch.zeros(1, ncnt, dtype=torch.int32), None)]
        if sim_mode >= 0:
            R.append(Region('state', philox_states(seed, 5, eps[:, 0].tolist(), 0, S), None))
        if cont:
            R.append(Region('prev_action_f', torch.zeros(E, A), None))
        if act_host:
            R.append(Region('act_host', torch.zeros(E, A) if cont else torch.full((E, 1), -1, dtype=torch.int32), None))
        return R
    return DSpec(f'rollout_begin-E{E}-S{S}-c{cont}-sim{sim_mode}-ah{act_host}', 'ROLLOUT_BEGIN', B, outs, desc, [dict()],
                 form='k_rollout_begin', expect=expect)


BEGIN_CASES = [(1, 1, 0, 1, 0, 3), (17, 8, 0, 0, 1, 2 ** 40 + 7), (300, 5, 1, 1, 1, 11), (40, 63, 1, -1, 0, 5), (257, 3, 0, -1, 1, 9)]


def sim_reset_spec(E, S, seed, update):
    g = _gen(67, E, S)
    eps = torch.randint(0, 5000, (E, 1), generator=g, dtype=torch.int32)
    B = dict(episode_of_slot=eps, state=torch.full((E + 2, S), NAN), live_rows=torch.zeros(2, E, dtype=torch.int32),
             live_count=torch.zeros(1, 2, dtype=torch.int32))

    def expect(dt):
        return [Region('state', philox_states(seed, update, eps[:, 0].tolist(), 0, S), None)]
    return DSpec(f'sim_reset-E{E}-S{S}', 'SIM_RESET', B, ('state',), base_desc(E, 36, 4, S=S), [dict()],
                 call=dict(seed=seed, update=update), form='k_sim_reset', expect=expect)


SIM_RESET_CASES = [(1, 1, 3, 0), (257, 8, 2 ** 35 + 1, 4), (40, 63, 77, 2 ** 20)]


# ----------------------------------------------------------------------------------------------
# 4. the decode projection (dproj): column split with row_map2, ReLU, the LayerNorm / RMSNorm prologue, both K splits
# ----------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class ProjCase:
    N: int
    K: int
    epi: str = 'NONE'
    ln: int = 0          # 0 none, 1 LayerNorm, 2 RMSNorm (the descriptor's rms_norm)
    ln_k: int = 0        # columns the prologue normalises (0: K)
    res: int = 0
    n_split: int = 0     # 0: no split
    nl: int = 21

    @property
    def id(self):
        return f'proj-N{self.N}-K{self.K}-{self.epi}-ln{self.ln}k{self.ln_k}-res{self.res}-split{self.n_split}-M{self.nl}'


PROJ_CASES = [ProjCase(40, 64, n_split=23), ProjCase(40, 64, n_split=1, ln=1), ProjCase(36, 1024, n_split=7),   # dg_ks 2
              ProjCase(70, 36, epi='RELU'), ProjCase(520, 36, epi='RELU', nl=33), ProjCase(100, 768, epi='RELU'),
              ProjCase(48, 128, ln=2), ProjCase(48, 132, ln=2, ln_k=64, res=1), ProjCase(600, 260, ln=2, epi='GELU', nl=33),
              ProjCase(48, 260, ln=1, epi='SILU'), ProjCase(17, 772, ln=1, ln_k=512, res=1), ProjCase(64, 16, res=1, nl=1)]


def act_and_slope(v, epi):
    if epi == 'GELU':
        return gelu(v), (0.5 * (1 + torch.erf(v * 0.70710678118654752)) + v * torch.exp(-0.5 * v * v) * 0.3989422804014327).abs()
    if epi == 'SILU':
        sg = 1.0 / (1.0 + torch.exp(-v))
        return v * sg, (sg * (1 + v * (1 - sg))).abs()
    if epi == 'RELU':
        return v.clamp_min(0.), torch.ones_like(v)
    return v, torch.ones_like(v)


def dense(a, w, bias, u_a=None):
    """a W^T + bias taken k after k in a's precision, and its unit 2^-24 (|bias| + sum |a| |w|) (+ sum u_a |w|)."""
    y = seqsum(a[:, None, :] * w[None], 2)
    unit = EPS24 * (a.double().abs() @ w.double().abs().t())
    if bias is not None:
        y = y + bias
        unit = unit + EPS24 * bias.double().abs()
    if u_a is not None:
        unit = unit + u_a @ w.double().abs().t()
    return y, unit


def proj_spec(c: ProjCase):
    N, K, nl = c.N, c.K, c.nl
    E = nl + 3
    g = _gen(71, N, K, c.ln, c.res, c.n_split, len(c.epi))
    slots = live_slots(E, nl, g)
    rows, cnt = live_bufs(E, 1, slots, g)
    lda, ldr, ldc, ldc2 = K + 8, N + 3, (c.n_split or N) + 5, (N - c.n_split) + 2 if c.n_split else 0
    ln_k = (c.ln_k or K) if c.ln else 0
    B = dict(live_rows=rows, live_count=cnt, A=guarded(padded(rnd(g, nl, K), lda), 3, BIG), W=rnd(g, N, K, scale=1 / math.sqrt(K)),
             bias=row(rnd(g, N)), gamma=row(gain(g, max(ln_k, 4))), R=guarded(padded(rnd(g, nl, N), ldr), 3, BIG),
             C=nan_out(E, ldc))
    outs = ['C']
    if c.n_split:
        B['C2'] = nan_out(E, ldc2)
        outs.append('C2')
    Wsrc = B['W']
    B['W'] = padded(Wsrc, K + 4)      # (the packer must not read past K)
    desc = base_desc(E, 36, 4, rms_norm=int(c.ln == 2))

    def expect(dt):
        a = B['A'][:nl, :K].to(dt)
        u_a = None
        if c.ln:
            xh, _, rstd = ln_rows(a[:, :ln_k], c.ln == 2)
            an = xh * B['gamma'][:, :ln_k].to(dt)
            u_n = ln_unit(EPS24 * a[:, :ln_k].double().abs(), xh.double(), rstd.double(), B['gamma'][0, :ln_k].double(), an.double())
            a = torch.cat([an, a[:, ln_k:]], 1)
            u_a = torch.cat([u_n, torch.zeros(nl, K - ln_k, dtype=torch.float64)], 1)
        v, unit = dense(a, Wsrc.to(dt), B['bias'].to(dt), u_a)
        y, slope = act_and_slope(v, c.epi)
        unit = unit * slope.double().clamp_min(1.) + EPS24 * y.double().abs()
        if c.res:
            r = B['R'][:nl, :N].to(dt)
            y = y + r
            unit = unit + EPS24 * (r.double().abs() + y.double().abs())
        if not c.n_split:
            return [comp_region('C', y, unit, 'proj')]
        R = [comp_region('C', y[:, :c.n_split], unit[:, :c.n_split], 'proj')]
        for i, e in enumerate(slots.tolist()):     # the columns past the split land in the slot's row
            R.append(comp_region('C2', y[i:i + 1, c.n_split:], unit[i:i + 1, c.n_split:], 'proj', r0=e))
        return R

    form = dgemm_kernel(N, K, 'EPI_' + c.epi, c.ln > 0, c.res > 0)
    return DSpec(c.id, 'PROJ', B, tuple(outs), desc, [dict()], t=1,
                 in_=('A', 'Wp', 'bias', 'gamma' if c.ln else None, 'R' if c.res else None, None, 'live_slots' if c.n_split else None),
                 out=('C', 'C2' if c.n_split else None), ld=(lda, ldr, ldc, ldc2), n=(K, ln_k, N, EPI[c.epi], c.n_split or N),
                 form=form, expect=expect, info=dict(pack=[('dgemm', 'W', 'Wp', N, K)], slots=slots))


# ----------------------------------------------------------------------------------------------
# 5. the one-launch feed-forward (k_mlp): both weight images, inner / last layer, the fractal tail
# ----------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class MlpCase:
    d: int
    ff: int
    nl: int
    kind: str = 'inner'     # 'inner' (C = x, Y = xn), 'last' (C NULL, Y = ac_in), 'fr0' / 'fr1' (fractal level 0 / the last)
    fi: int = 0             # the fp32 fragment images (w_ff1f / w_ff2f) instead of the split images
    rms: int = 0
    t: int = 0

    @property
    def id(self):
        return f'mlp-d{self.d}-ff{self.ff}-M{self.nl}-{self.kind}-fi{self.fi}-rms{self.rms}-t{self.t}'


def _mlp_cases():
    out = []
    k = 0
    for d in (64, 128, 192, 256):
        for ff in (128, 256, 1024):
            for nl in (1, 16, 17, 33):
                kind = ('inner', 'last', 'fr0', 'fr1')[k % 4]
                out.append(MlpCase(d, ff, nl, kind, fi=(k // 4) % 2, rms=int(kind in ('inner', 'last') and (k // 2) % 2),
                                   t=(0, 3)[(k // 3) % 2]))
                k += 1
    return out


MLP_CASES = _mlp_cases()


def split3(x):
    """x = hi + mid + lo, each the round-to-nearest bf16 of the running remainder (x6.h)."""
    h = x.bfloat16().float()
    m = (x - h).bfloat16().float()
    return h, m, (x - h) - m


def x6_dense(a, w, dt):
    """a W^T as the kernel forms it in fp32: per 32-deep k step the six largest piece products, smallest first, each
    accumulated onto the running sum (fp64: the plain product)."""
    if dt == torch.float64:
        return a.double() @ w.double().t()
    ap, wp = split3(a), split3(w)
    S = a.shape[1] // 32
    cut = lambda x: x.reshape(x.shape[0], S, 32)   # noqa: E731
    prods = torch.stack([torch.einsum('msk,nsk->smn', cut(ap[i]), cut(wp[j]))
                         for i, j in ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0))], 1)     # [S][6][M][N]
    even, odd = prods[0::2].reshape(-1, *prods.shape[2:]), prods[1::2].reshape(-1, *prods.shape[2:])
    return seqsum(even) + (seqsum(odd) if S > 1 else 0.)     # the kernel's two accumulators: even and odd k steps


def mlp_spec(c: MlpCase):
    d, ff, nl, t = c.d, c.ff, c.nl, c.t
    E = nl + 3
    g = _gen(73, d, ff, nl, len(c.kind), t)        # (not the image kind: both images see the same inputs)
    slots = live_slots(E, nl, g)
    rows, cnt = live_bufs(E, t, slots, g)
    fr = c.kind.startswith('fr')
    npan, HC = (E + 15) // 16, ff // MLP_HW
    live_pan = (nl + 15) // 16
    xin = rnd(g, nl, d)
    B = dict(live_rows=rows, live_count=cnt, W1=rnd(g, ff, d, scale=1 / math.sqrt(d)), b_ff1=row(rnd(g, ff, scale=0.5)),
             W2=rnd(g, d, ff, scale=1 / math.sqrt(ff)), b_ff2=row(rnd(g, d, scale=0.5)), w_out_t=torch.zeros(64, d),
             mlp_part=torch.full((npan * HC * 16 + 2, d), NAN), mlp_cnt=torch.zeros(1, npan + 2, dtype=torch.int32),
             gnext=row(gain(g, d)))
    W1, W2 = B['W1'], B['W2']
    B['W1'], B['W2'] = padded(W1, d + 4), padded(W2, ff + 4)      # (the packers must not read past K)
    img = ('w_ff1f', 'w_ff2f') if c.fi else ('w_ff1x', 'w_ff2x')
    layer = dict(b_ff1='b_ff1', b_ff2='b_ff2', w_out_t='w_out_t', ln_attn='gnext', **{img[0]: img[0], img[1]: img[1]})
    kindp = 'f8' if c.fi else 'x6'
    pack = [(kindp, 'W1', img[0], ff, d), (kindp, 'W2', img[1], d, ff)]
    desc = base_desc(E, d, t + 2, L=2, ff=ff, rms_norm=c.rms, mlp_part='mlp_part', mlp_cnt='mlp_cnt', ln_final='gnext')
    outs = ['mlp_part', 'mlp_cnt']
    fractal = None
    if fr:
        level = int(c.kind[2])
        B['x2'] = guarded(xin, E - nl + 2, BIG)
        B.update(sums=guarded(rnd(g, E, d, scale=3.), 2, NAN), mean=nan_out(E, d), x=nan_out(E, d))
        fractal = _fractal(B, g, d, E)
        fractal.update(x2='x2', mean='mean')
        fractal['level'][level]['sums'] = 'sums'
        desc.update(state_only=1, x='x')
        outs += ['sums', 'mean', 'x']
        lyr = level
    else:
        res = rnd(g, nl, d)
        B['x'] = torch.cat([res, rnd(g, E - nl + 2, d)])
        desc.update(x='x', xn='xn', ac_in='ac_in')
        B['ac_in'] = nan_out(E, 2 * d)
        B['xn'] = torch.cat([xin, rnd(g, E - nl + 2, d)])
        outs += ['x', 'xn', 'ac_in']
        lyr = 0 if c.kind == 'inner' else 1
    if fr:
        desc['xn'] = None

    def expect(dt):
        f = lambda k: B[k].to(dt)   # noqa: E731
        xi = xin.to(dt)
        pre = x6_dense(xin, W1, dt).to(dt) + f('b_ff1')
        h, slope = act_and_slope(pre, 'GELU')
        # (the split-bf16 product drops three piece products, each below 2^-24 of its term: 4 x 2^-24 a term)
        u_h = 4 * EPS24 * (xi.double().abs() @ W1.double().abs().t() + B['b_ff1'].double().abs()) * slope.double().clamp_min(1.) \
            + EPS24 * h.double().abs()
        hh = h.float() if dt == torch.float32 else h
        resv = xi if fr else f('x')[:nl]
        part = x6_dense(hh, W2, dt).to(dt) if dt == torch.float32 else hh @ W2.to(dt).t()
        s = (resv + f('b_ff2')) + part
        u_s = C_COMP['mlp'] * u_h @ W2.double().abs().t() + 4 * EPS24 * (h.double().abs() @ W2.double().abs().t()) \
            + EPS24 * (resv.double().abs() + B['b_ff2'].double().abs() + s.double().abs())
        R = [Region('mlp_part', None, None, shape=(live_pan * HC * 16, d)), Region('mlp_cnt', torch.zeros(1, npan, dtype=torch.int32), None)]
        if fr:
            return R + fr_tail_regions(B, dt, s, C_COMP['mlp'] * u_s, int(c.kind[2]), 2, t, slots, nl, d, 'sums')
        if c.kind == 'inner':
            R.append(comp_region('x', s, u_s, 'mlp'))
        xh, _, rstd = ln_rows(s, c.rms)
        y = xh * f('gnext')
        u_y = ln_unit(C_COMP['mlp'] * u_s, xh.double(), rstd.double(), B['gnext'][0].double(), y.double())
        R.append(comp_region('xn' if c.kind == 'inner' else 'ac_in', y, u_y, 'attn_norm'))
        return R

    assert fr or mlp_fused(d, ff, True, True, True, 0, attn_fused(4, 16, d, t + 2, True))     # (launch_mlp's own condition)
    return DSpec(c.id, 'MLP', B, tuple(outs), desc, [layer, layer], t=t, layer=lyr, fractal=fractal, form=mlp_kernel(d, c.fi),
                 expect=expect, info=dict(pack=pack))


# ----------------------------------------------------------------------------------------------
# 6. heads + sampling + Sim step, discrete actions (decode_heads): k_heads_mlp<2|3|6>, k_heads_sample<1|2>
# ----------------------------------------------------------------------------------------------

TIE_CAP = 0.02
F32_EPS = 1.1920928955078125e-07
HEADS_B = 5


@dataclass(frozen=True)
class HeadsCase:
    d: int
    evo: int
    A: int
    path: str            # 'mlp' (k_heads_mlp: w_h1x, w_h2_t, heads_part / heads_cnt) or 'hs' (projection + k_heads_sample)
    fn: int = 0          # final norm in the hidden projection's prologue ('hs' only)
    sim: int = 1         # sim_mode -1 / 0 / 1
    hz: int = 2          # hazard_log2
    last: int = 0        # t + 1 == Tmax
    ah: int = 0          # act_host set
    scale: float = 1.    # spread of the actor biases (200: the saturated softmax, the clamp to 1 - eps)
    nl: int = 21
    seed: int = 0        # Philox seed offset (moved where the reference's own tie count passes TIE_CAP)

    @property
    def id(self):
        return (f'heads-{self.path}-d{self.d}-evo{self.evo}-A{self.A}-fn{self.fn}-sim{self.sim}-hz{self.hz}-last{self.last}'
                f'-ah{self.ah}-sc{self.scale:g}-M{self.nl}-s{self.seed}')


HEADS_CASES = [
    HeadsCase(64, 0, 4, 'mlp'), HeadsCase(64, 1, 8, 'mlp', sim=0, hz=0, ah=1, nl=33), HeadsCase(128, 1, 32, 'mlp', last=1, seed=3),
    HeadsCase(64, 0, 1, 'mlp', sim=-1, ah=1, nl=16), HeadsCase(64, 0, 8, 'mlp', scale=200., nl=17),
    HeadsCase(36, 0, 4, 'hs', fn=1), HeadsCase(36, 1, 32, 'hs', sim=0, hz=0, nl=33), HeadsCase(36, 0, 9, 'hs', fn=1, sim=-1, ah=1),
    HeadsCase(192, 0, 8, 'hs', fn=1, last=1, seed=3), HeadsCase(192, 0, 32, 'hs', hz=0, ah=1, nl=17), HeadsCase(36, 0, 8, 'hs', scale=200.),
    HeadsCase(192, 0, 4, 'hs', fn=1, scale=200., nl=1),
]


def heads_kernel(c: HeadsCase):
    """decode_heads' choice, restated (heads_fused, dg_ks)."""
    in_dim, n_act = (3 if c.evo else 2) * c.d, c.A
    jh = in_dim // 64
    fused = (not c.fn and c.path == 'mlp' and in_dim % 64 == 0 and jh in (2, 3, 4, 6, 8, 12) and c.d % 32 == 0 and c.d <= 256
             and n_act <= 64 and round4(n_act + HEADS_B) <= 128)
    if fused:
        return f'k_heads_mlp<{jh}>'
    ks = dg_ks(n_act + HEADS_B, 4 * c.d)
    hidden = dgemm_kernel(4 * c.d, in_dim, 'EPI_SILU', c.fn, False)
    return hidden + (f'+k_heads_sample<{ks}>' if n_act <= 64 // ks else f"+{dgemm_kernel(n_act + HEADS_B, 4 * c.d, 'EPI_NONE', False, False)}+k_sample")


def round4(x):
    return (x + 3) & ~3


def heads_spec(c: HeadsCase):
    from oracle import philox as PH
    d, A, nl, Bn = c.d, c.A, c.nl, HEADS_B
    in_dim, na2 = (3 if c.evo else 2) * d, A + HEADS_B
    npad, E, S, t = round4(na2), nl + 3, 6, 2
    Tmax = t + 1 if c.last else t + 3
    seed, upd, soff = 2 ** 33 + 17 + d + A + 7919 * c.seed, 3, 1000
    g = _gen(79, d, c.evo, A, len(c.path), c.fn, c.sim + 1, nl)
    slots = live_slots(E, nl, g)
    rows, cnt = live_bufs(E, t, slots, g)
    al = torch.zeros(E, dtype=torch.uint8)
    al[slots] = 1
    if nl > 2:
        al[slots[1]] = 2                      # one truncation-bootstrap row
    W1 = rnd(g, 4 * d, in_dim, scale=1 / math.sqrt(in_dim))
    W2 = torch.zeros(na2, 4 * d)
    W2[:A, :2 * d] = rnd(g, A, 2 * d, scale=1 / math.sqrt(2 * d))
    W2[A:, 2 * d:] = rnd(g, Bn, 2 * d, scale=1 / math.sqrt(2 * d))
    b2 = torch.zeros(1, npad)
    b2[0, :na2] = rnd(g, na2, scale=0.5)     # (header: the padding zero)
    if c.scale > 1:
        b2[0, :A] = torch.linspace(-c.scale / 2, c.scale / 2, A)[torch.randperm(A, generator=g)]
    w2t = torch.zeros(4 * d, npad)
    w2t[:, :na2] = W2.t()
    eps = torch.randint(0, 1000, (E, 1), generator=g, dtype=torch.int32)
    acin = rnd(g, nl, in_dim)
    B = dict(live_rows=rows, live_count=cnt, alive=row(al).clone(), ac_in=guarded(acin, E - nl + 2, BIG),
             W1=padded(W1, in_dim + 4), b_h1=row(rnd(g, 4 * d, scale=0.5)), W2=padded(W2, 4 * d + 4), b_h2=b2, w_h2_t=w2t,
             ln_final=row(gain(g, d)), hff=nan_out(E, 4 * d), logits=nan_out(E, A), traj_values=torch.full((E * Tmax + 2, Bn), NAN),
             state=rnd(g, E, S), prev_action=torch.full((E, 1), ISENT, dtype=torch.int32), prev_reward=rnd(g, E, 1),
             lens=torch.full((E, 1), ISENT, dtype=torch.int32), cum_reward=rnd(g, E, 1).double() * 10,
             traj_actions=torch.full((E, Tmax), ISENT, dtype=torch.int32), traj_logp=torch.full((E, Tmax), NAN),
             traj_rewards=torch.full((E, Tmax), NAN), traj_bounds=torch.full((E, Tmax), 7, dtype=torch.uint8),
             act_host=torch.full((E, 1), ISENT, dtype=torch.int32), rng=rng_buf(seed, upd, soff), episode_of_slot=eps)
    desc = base_desc(E, d, Tmax, S=S, A=A, B=Bn, in_dim=in_dim, evolutionary=c.evo, sim_mode=c.sim, hazard_log2=c.hz,
                     ac_in='ac_in', w_h1='w_h1p', b_h1='b_h1', w_h2='w_h2p', b_h2='b_h2', ln_final='ln_final', hff='hff',
                     logits='logits', traj_values='traj_values', state='state', prev_action='prev_action', prev_reward='prev_reward',
                     alive='alive', lens='lens', cum_reward='cum_reward', traj_actions='traj_actions', traj_logp='traj_logp',
                     traj_rewards='traj_rewards', traj_bounds='traj_bounds', rng='rng', episode_of_slot='episode_of_slot',
                     act_host='act_host' if c.ah else None)
    pack = [('dgemm', 'W1', 'w_h1p', 4 * d, in_dim), ('dgemm', 'W2', 'w_h2p', na2, 4 * d)]
    outs = ['hff', 'logits', 'traj_values', 'state', 'prev_action', 'prev_reward', 'alive', 'lens', 'cum_reward', 'traj_actions',
            'traj_logp', 'traj_rewards', 'traj_bounds', 'act_host']
    if c.path == 'mlp':
        HC, npan = 4 * d // 64, (E + 15) // 16
        B.update(heads_part=torch.full((npan * HC * 16 + 2, npad), NAN), heads_cnt=torch.zeros(1, npan + 2, dtype=torch.int32))
        desc.update(w_h1x='w_h1x', w_h2_t='w_h2_t', heads_part='heads_part', heads_cnt='heads_cnt')
        pack.append(('x6', 'W1', 'w_h1x', 4 * d, in_dim))
        outs += ['heads_part', 'heads_cnt']
    info = dict(pack=pack)

    def expect(dt, taken=None):
        f = lambda k: B[k].to(dt)   # noqa: E731
        a = acin.to(dt)
        W1d, W2d = W1.to(dt), W2.to(dt)
        u_a = None
        if c.fn:
            xh, _, rstd = ln_rows(a[:, :d], 0)
            an = xh * f('ln_final')
            u_n = ln_unit(EPS24 * a[:, :d].double().abs(), xh.double(), rstd.double(), B['ln_final'][0].double(), an.double())
            a = torch.cat([an, a[:, d:]], 1)
            u_a = torch.cat([u_n, torch.zeros(nl, in_dim - d, dtype=torch.float64)], 1)
        if c.path == 'mlp':
            pre = x6_dense(acin, W1, dt).to(dt) + f('b_h1')
            u_pre = 4 * EPS24 * (a.double().abs() @ W1.double().abs().t() + B['b_h1'].double().abs())
        else:
            pre, u_pre = dense(a, W1d, f('b_h1'), u_a)
        h, slope = act_and_slope(pre, 'SILU')
        u_h = u_pre * slope.double().clamp_min(1.) + EPS24 * h.double().abs()
        out, u_l = dense(h, W2d, f('b_h2')[:, :na2], C_COMP['heads_h'] * u_h)
        u_l = u_l + EPS24 * out.double().abs()
        R = [comp_region('logits', out[:, :A], u_l[:, :A], 'heads')]
        if c.path == 'hs':
            R.append(comp_region('hff', h, u_h, 'heads_h'))
        else:
            live_pan = (nl + 15) // 16
            R += [Region('heads_part', None, None, shape=(live_pan * (4 * d // 64) * 16, npad)),
                  Region('heads_cnt', torch.zeros(1, B['heads_cnt'].shape[1] - 2, dtype=torch.int32), None)]
        bl = (C_COMP['heads'] * u_l[:, :A]).max(-1).values                      # the logits' bound, per row
        L = out[:, :A]
        ex = torch.exp(L - L.max(-1, keepdim=True).values)
        q = ex / seqsum(ex, 1)[:, None]
        p = q / seqsum(q, 1)[:, None]
        cdf = p.cumsum(1)[:, :A - 1]
        a_ref, ties, a_use, lp, u_lp = [], 0, [], [], []
        after = al.clone()
        for r, e in enumerate(slots.tolist()):
            R.append(comp_region('traj_values', out[r:r + 1, A:], u_l[r:r + 1, A:], 'heads', r0=e * Tmax + t))
            if int(al[e]) == 2:
                after[e] = 0
                a_ref.append(-1)
                continue
            u = torch.tensor(PH.philox_uniform(seed, upd, soff + e, t, PH.FIELD_SAMPLE, 1)[0]).to(dt)
            act = int((u >= cdf[r]).sum())
            # the cdf's own bound: A x the probability bound (a probability moves by a relative 2 x the logits' bound)
            delta = A * float((p[r].double() * 2 * bl[r] + 4 * EPS24).max())
            lo, hi = int((u.double() >= cdf[r].double() + delta).sum()), int((u.double() >= cdf[r].double() - delta).sum())
            a_ref.append(act)
            if lo != hi:
                ties += 1
                if taken is not None and lo <= int(taken[r]) <= hi:
                    act = int(taken[r])
            pa = p[r, act].clamp(F32_EPS, 1. - F32_EPS)
            logp = torch.log(pa)
            av = torch.tensor([[act]], dtype=torch.int32)
            R += [Region('traj_actions', av, None, r0=e, c0=t), Region('prev_action', av, None, r0=e),
                  comp_region('traj_logp', logp.reshape(1, 1), (2 * bl[r] + EPS24 * (A + logp.double().abs())).reshape(1, 1), 'heads_lp',
                              r0=e, c0=t)]
            if c.ah:
                R.append(Region('act_host', av, None, r0=e))
            if c.sim >= 0:
                ep = int(eps[e, 0])
                zr = PH.philox_uniform(seed, upd, ep, t, PH.FIELD_REWARD, 1, normal=True)[0]
                rew = np.float32(zr * PH.REWARD_FACTORS[act]) if c.sim == 1 else np.float32(zr)
                tw = int(PH.philox_u32(seed, upd, ep, t, PH.FIELD_TERM))
                term = c.sim == 1 and c.hz > 0 and (tw & ((1 << c.hz) - 1)) == 0
                rw = torch.tensor([[float(rew)]], dtype=torch.float32)
                R += [Region('state', philox_states(seed, upd, [ep], t + 1, S), None, r0=e),
                      Region('traj_rewards', rw, None, r0=e, c0=t), Region('prev_reward', rw, None, r0=e),
                      Region('traj_bounds', torch.tensor([[int(term)]], dtype=torch.uint8), None, r0=e, c0=t),
                      Region('cum_reward', B['cum_reward'][e:e + 1] + rw.double(), None, r0=e),
                      Region('lens', torch.tensor([[t + 1]], dtype=torch.int32), None, r0=e)]
                if term or t + 1 >= Tmax:
                    after[e] = 0
        R.append(Region('alive', row(after), None))
        info.update(a_ref=a_ref, ties=ties)
        return R

    return DSpec(c.id, 'HEADS', B, tuple(outs), desc, [dict()], t=t, n=(c.fn,), form=heads_kernel(c), expect=expect, info=info)


# ----------------------------------------------------------------------------------------------
# 7. heads + sampling, continuous actions: the projection + k_sample path (2 A = 64 at KS 2) and the fused paths
# ----------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class ContCase:
    d: int
    A: int
    path: str            # 'mlp' / 'hs' as HeadsCase ('hs' at d = 192, A = 32: projection + k_sample)
    squash: int = 1
    clamp: float = 0.    # has_clamp with (-clamp, clamp)
    sat: int = 0         # means of +-40: |pre-tanh| >= 30
    sim: int = 1
    ah: int = 0
    nl: int = 17

    @property
    def id(self):
        return f'headsc-{self.path}-d{self.d}-A{self.A}-sq{self.squash}-cl{self.clamp:g}-sat{self.sat}-sim{self.sim}-ah{self.ah}-M{self.nl}'


CONT_CASES = [ContCase(192, 32, 'hs', clamp=0.95, ah=1), ContCase(192, 32, 'hs', squash=0, sim=0), ContCase(192, 32, 'hs', clamp=0.9, sat=1),
              ContCase(36, 3, 'hs', clamp=0.95, sim=-1, ah=1), ContCase(64, 6, 'mlp', clamp=0.95), ContCase(64, 2, 'mlp', squash=0, ah=1, nl=33)]


def cont_kernel(c: ContCase):
    hc = HeadsCase(c.d, 0, 2 * c.A, c.path)
    return heads_kernel(hc)


def cont_spec(c: ContCase):
    from oracle import philox as PH
    d, A, nl, Bn = c.d, c.A, c.nl, HEADS_B
    n_act = 2 * A
    in_dim, na2 = 2 * d, n_act + Bn
    npad, E, S, t = round4(na2), nl + 3, 6, 2
    Tmax = t + 3
    seed, upd, soff = 2 ** 34 + 5 + d + A, 2, 500
    g = _gen(83, d, A, len(c.path), c.squash, c.sat, nl)
    slots = live_slots(E, nl, g)
    rows, cnt = live_bufs(E, t, slots, g)
    al = torch.zeros(E, dtype=torch.uint8)
    al[slots] = 1
    if nl > 2:
        al[slots[1]] = 2
    W1 = rnd(g, 4 * d, in_dim, scale=1 / math.sqrt(in_dim))
    W2 = torch.zeros(na2, 4 * d)
    W2[:n_act, :2 * d] = rnd(g, n_act, 2 * d, scale=0.5 / math.sqrt(2 * d))
    W2[n_act:, 2 * d:] = rnd(g, Bn, 2 * d, scale=1 / math.sqrt(2 * d))
    b2 = torch.zeros(1, npad)
    b2[0, :na2] = rnd(g, na2, scale=0.3)
    if c.sat:
        b2[0, 0:n_act:2] = 40. * torch.where(torch.arange(A) % 2 == 0, 1., -1.)
    w2t = torch.zeros(4 * d, npad)
    w2t[:, :na2] = W2.t()
    eps = torch.randint(0, 1000, (E, 1), generator=g, dtype=torch.int32)
    acin = rnd(g, nl, in_dim)
    B = dict(live_rows=rows, live_count=cnt, alive=row(al).clone(), ac_in=guarded(acin, E - nl + 2, BIG),
             W1=padded(W1, in_dim + 4), b_h1=row(rnd(g, 4 * d, scale=0.5)), W2=padded(W2, 4 * d + 4), b_h2=b2, w_h2_t=w2t,
             hff=nan_out(E, 4 * d), logits=nan_out(E, n_act), traj_values=torch.full((E * Tmax + 2, Bn), NAN),
             state=rnd(g, E, S), prev_action_f=torch.full((E + 2, A), NAN), prev_reward=rnd(g, E, 1),
             lens=torch.full((E, 1), ISENT, dtype=torch.int32), cum_reward=rnd(g, E, 1).double() * 10,
             traj_actions_f=torch.full((E * Tmax + 2, A), NAN), traj_logp=torch.full((E * Tmax + 2, A), NAN),
             traj_rewards=torch.full((E, Tmax), NAN), traj_bounds=torch.full((E, Tmax), 7, dtype=torch.uint8),
             act_host=torch.full((E + 2, A), NAN), rng=rng_buf(seed, upd, soff), episode_of_slot=eps)
    desc = base_desc(E, d, Tmax, S=S, A=A, B=Bn, in_dim=in_dim, continuous=1, squash=c.squash, has_clamp=int(c.clamp > 0),
                     clamp_lo=-c.clamp, clamp_hi=c.clamp, sim_mode=c.sim, hazard_log2=2,
                     ac_in='ac_in', w_h1='w_h1p', b_h1='b_h1', w_h2='w_h2p', b_h2='b_h2', hff='hff',
                     logits='logits', traj_values='traj_values', state='state', prev_action_f='prev_action_f', prev_reward='prev_reward',
                     alive='alive', lens='lens', cum_reward='cum_reward', traj_actions_f='traj_actions_f', traj_logp='traj_logp',
                     traj_rewards='traj_rewards', traj_bounds='traj_bounds', rng='rng', episode_of_slot='episode_of_slot',
                     act_host='act_host' if c.ah else None)
    pack = [('dgemm', 'W1', 'w_h1p', 4 * d, in_dim), ('dgemm', 'W2', 'w_h2p', na2, 4 * d)]
    outs = ['hff', 'logits', 'traj_values', 'state', 'prev_action_f', 'prev_reward', 'alive', 'lens', 'cum_reward', 'traj_actions_f',
            'traj_logp', 'traj_rewards', 'traj_bounds', 'act_host']
    if c.path == 'mlp':
        HC, npan = 4 * d // 64, (E + 15) // 16
        B.update(heads_part=torch.full((npan * HC * 16 + 2, npad), NAN), heads_cnt=torch.zeros(1, npan + 2, dtype=torch.int32))
        desc.update(w_h1x='w_h1x', w_h2_t='w_h2_t', heads_part='heads_part', heads_cnt='heads_cnt')
        pack.append(('x6', 'W1', 'w_h1x', 4 * d, in_dim))
        outs += ['heads_part', 'heads_cnt']

    def expect(dt):
        f = lambda k: B[k].to(dt)   # noqa: E731
        a = acin.to(dt)
        if c.path == 'mlp':
            pre = x6_dense(acin, W1, dt).to(dt) + f('b_h1')
            u_pre = 4 * EPS24 * (a.double().abs() @ W1.double().abs().t() + B['b_h1'].double().abs())
        else:
            pre, u_pre = dense(a, W1.to(dt), f('b_h1'))
        h, slope = act_and_slope(pre, 'SILU')
        u_h = u_pre * slope.double().clamp_min(1.) + EPS24 * h.double().abs()
        out, u_l = dense(h, W2.to(dt), f('b_h2')[:, :na2], C_COMP['heads_h'] * u_h)
        u_l = u_l + EPS24 * out.double().abs()
        R = [comp_region('logits', out[:, :n_act], u_l[:, :n_act], 'heads')]
        if c.path == 'hs':
            R.append(comp_region('hff', h, u_h, 'heads_h'))
        else:
            R += [Region('heads_part', None, None, shape=(((nl + 15) // 16) * (4 * d // 64) * 16, npad)),
                  Region('heads_cnt', torch.zeros(1, B['heads_cnt'].shape[1] - 2, dtype=torch.int32), None)]
        bl = C_COMP['heads'] * u_l[:, :n_act]
        after = al.clone()
        for r, e in enumerate(slots.tolist()):
            R.append(comp_region('traj_values', out[r:r + 1, n_act:], u_l[r:r + 1, n_act:], 'heads', r0=e * Tmax + t))
            if int(al[e]) == 2:
                after[e] = 0
                continue
            mean, lv = out[r, 0:n_act:2], out[r, 1:n_act:2]
            bm, bv = bl[r, 0:n_act:2], bl[r, 1:n_act:2]
            z = torch.from_numpy(PH.philox_uniform(seed, upd, soff + e, t, PH.FIELD_SAMPLE, A, normal=True)).to(dt)
            var = torch.exp(torch.tanh(lv / 3.) * 3.)
            sd = torch.sqrt(var.clamp_min(1e-5))
            sv = mean + sd * z
            sdd, zd = sd.double(), z.double().abs()
            u_sd = sdd * bv / 2 + 4 * EPS24 * sdd
            u_sv = bm + zd * u_sd + EPS24 * (mean.double().abs() + sdd * zd + sv.double().abs())
            if c.squash:
                sv = torch.tanh(sv)
                om = (1. - sv.double() ** 2)
                u_sv = 2 * u_sv * om + 4 * EPS24 * sv.double().abs()
            diff = (sv - mean)
            lp = -(diff * diff) / (2. * sd * sd) - torch.log(sd) - 0.91893853320467274
            dd = diff.double().abs()
            u_lp = dd / sdd ** 2 * (u_sv + bm) + dd ** 2 / sdd ** 3 * u_sd + u_sd / sdd
            if c.squash:
                fl = (1. - sv * sv).clamp_min(1e-20)
                lp = lp - torch.log(fl)
                # the conditioning of log(1 - a^2): 2 |a| / (1 - a^2) x the action's bound, and 1 - a a is itself rounded
                u_lp = u_lp + torch.where(fl.double() > 1e-20, (2 * sv.double().abs() * u_sv + 4 * EPS24) / fl.double(), torch.zeros_like(u_lp))
            u_lp = u_lp + 4 * EPS24 * ((dd / sdd) ** 2 + torch.log(sd).double().abs() + 1. + lp.double().abs())
            if c.clamp > 0:
                sv = sv.clamp(torch.tensor(-c.clamp, dtype=torch.float32).to(dt), torch.tensor(c.clamp, dtype=torch.float32).to(dt))
            svr, ub = sv.reshape(1, A), u_sv.reshape(1, A)
            R += [comp_region('traj_actions_f', svr, ub, 'heads_act', r0=e * Tmax + t),
                  comp_region('prev_action_f', svr, ub, 'heads_act', r0=e),
                  comp_region('traj_logp', lp.reshape(1, A), u_lp.reshape(1, A), 'heads_lp', r0=e * Tmax + t)]
            if c.ah:
                R.append(comp_region('act_host', svr, ub, 'heads_act', r0=e))
            if c.sim >= 0:
                ep = int(eps[e, 0])
                zr = PH.philox_uniform(seed, upd, ep, t, PH.FIELD_REWARD, 1, normal=True)[0]
                tw = int(PH.philox_u32(seed, upd, ep, t, PH.FIELD_TERM))
                term = c.sim == 1 and (tw & 3) == 0
                rw = torch.tensor([[float(zr)]], dtype=torch.float32)      # (continuous: no action factor)
                R += [Region('state', philox_states(seed, upd, [ep], t + 1, S), None, r0=e),
                      Region('traj_rewards', rw, None, r0=e, c0=t), Region('prev_reward', rw, None, r0=e),
                      Region('traj_bounds', torch.tensor([[int(term)]], dtype=torch.uint8), None, r0=e, c0=t),
                      Region('cum_reward', B['cum_reward'][e:e + 1] + rw.double(), None, r0=e),
                      Region('lens', torch.tensor([[t + 1]], dtype=torch.int32), None, r0=e)]
                if term:
                    after[e] = 0
        R.append(Region('alive', row(after), None))
        return R

    return DSpec(c.id, 'HEADS', B, tuple(outs), desc, [dict()], t=t, n=(0,), form=cont_kernel(c), expect=expect, info=dict(pack=pack))


# ----------------------------------------------------------------------------------------------
# 8. the row-resident step (xtrl_decode_step_rows, k_decode_row): one launch on a pre-filled state; the reference is the
#    composition of the stages above.  A worst-case propagation through the ten-odd dense stages of a row grows by 1e7 and
#    bounds nothing, so the units are the project's bare-sum form at the last stage of each output — 2^-24 (|bias| +
#    sum |a| |w| + |out|) of the q|k|v projection for the new K / V / v1 rows (a rotated channel: its pair, plus the
#    angle's rounding) and of the last Linear for the logits and critic logits — and the constants, 4 x the fp32
#    restatement's worst over the table, carry what the stages before amplify
# ----------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class RowCase:
    L: int
    d: int
    H: int
    Hkv: int
    dh: int
    t: int
    W: int = 0
    form: str = 'PLAIN'      # PLAIN / SINK / ALIBI / CLAMP
    E: int = 40
    nl: int = 9
    max_rows: int = 4
    gate: int = 0
    rms: int = 0
    seed: int = 0

    @property
    def id(self):
        return (f'rowstep-L{self.L}-d{self.d}-H{self.H}k{self.Hkv}dh{self.dh}-t{self.t}-W{self.W}-{self.form}-E{self.E}-M{self.nl}'
                f'-mr{self.max_rows}-g{self.gate}-rms{self.rms}-s{self.seed}')


def _row_cases():
    out = []
    k = 0
    forms = ('PLAIN', 'SINK', 'ALIBI', 'CLAMP')
    for t in (0, 1, 127, 128, 129, 257):
        for W in (0, 1, 63, 128, 130):
            out.append(RowCase(1 + k % 2, (36, 128)[(k // 2) % 2], 4, (4, 2)[(k // 3) % 2], 16, t, W, forms[k % 4],
                               E=(40, 65)[(k // 5) % 2], gate=k % 2, rms=int(k % 5 == 2)))
            k += 1
    for t in (63, 64, 65):
        for W in (0, 1, 63, 64, 66):
            out.append(RowCase(1 + k % 2, (36, 128)[(k // 2) % 2], (1, 2)[k % 2], (1, 2)[k % 2], 64, t, W, forms[k % 4], E=(40, 65)[k % 2]))
            k += 1
    out += [RowCase(1, 36, 4, 4, 16, 1, 0, 'PLAIN', E=1, nl=1, max_rows=1), RowCase(2, 128, 4, 2, 16, 1, 0, 'SINK', E=600, nl=100, max_rows=37),
            RowCase(2, 36, 4, 4, 16, 129, 63, 'CLAMP', E=65, nl=33, max_rows=5)]
    return out


ROW_CASES = _row_cases()
ROW_KP = {16: 2, 32: 1, 64: 1}


def row_kernel(c: RowCase):
    return f'k_decode_row<{c.dh},{ROW_KP[c.dh]},{FORM_FLAGS[c.form]}>'


def row_spec(c: RowCase):
    from oracle import philox as PH
    L, d, H, Hkv, dh, t, E, nl = c.L, c.d, c.H, c.Hkv, c.dh, c.t, c.E, c.nl
    I, Ikv, S, A, Bn, ff = H * dh, Hkv * dh, 5, 6, 5, 2 * d + 4
    vres = int(L > 1)
    n_qkv = I + 2 * Ikv + (I if c.gate else 0) + (Hkv if vres else 0)
    nq4, na2 = round4(n_qkv), A + Bn
    n2, Tmax, in_dim, rot_dim = round4(na2), t + 3, 2 * d, dh // 2
    M = 4 if c.form != 'PLAIN' else 0
    zkv = int(c.form in ('SINK', 'CLAMP'))
    alibi, cap = c.form in ('ALIBI', 'CLAMP'), 4. if c.form == 'CLAMP' else 0.
    seed, upd, soff = 2 ** 35 + 3 + t + 7919 * c.seed, 4, 200
    g = _gen(89, L, d, H, Hkv, dh, t, c.W, len(c.form), E, nl)
    slots = live_slots(E, nl, g) if E > 1 else torch.zeros(1, dtype=torch.int64)
    al = torch.zeros(E, dtype=torch.uint8)
    dead = torch.ones(E, dtype=torch.bool)
    dead[slots] = False
    al[dead] = torch.tensor([0, 3 + ((t + 1) & 1)], dtype=torch.uint8)[torch.randint(0, 2, (int(dead.sum()),), generator=g)]
    al[slots] = 1
    if nl > 3:
        al[slots[1]] = 2
        al[slots[2]] = 3 + (t & 1)
    j_lo = max(t - c.W, 0) if c.W > 0 else 0
    B = dict(alive=row(al).clone(), state=rnd(g, E, S), prev_reward=rnd(g, E, 1), rs_mean=row(rnd(g, S + 1, scale=0.3)),
             rs_var=row(torch.rand(S + 1, generator=g) + 0.5), w_pin=rnd(g, d, S, scale=1 / math.sqrt(S)), b_pin=row(rnd(g, d, scale=0.3)),
             reward_embed=row(rnd(g, d, scale=0.3)), w_se=rnd(g, d, S, scale=1 / math.sqrt(S)), b_se=row(rnd(g, d, scale=0.3)),
             act_emb=rnd(g, A, d, scale=0.5), prev_action=torch.randint(-1, A, (E, 1), generator=g, dtype=torch.int32),
             inv_freq=row(1.0 / (10000. ** (torch.arange(0, rot_dim, 2).float() / rot_dim))), ln_final=row(gain(g, d)),
             live_rows=torch.randint(0, E, (2, E), generator=g, dtype=torch.int32), live_count=torch.tensor([[ISENT, ISENT]], dtype=torch.int32),
             traj_states=torch.full((E * Tmax + 2, S), NAN), logits=nan_out(E, A), traj_values=torch.full((E * Tmax + 2, Bn), NAN),
             lens=torch.full((E, 1), ISENT, dtype=torch.int32), cum_reward=rnd(g, E, 1).double() * 10,
             traj_actions=torch.full((E, Tmax), ISENT, dtype=torch.int32), traj_logp=torch.full((E, Tmax), NAN),
             traj_rewards=torch.full((E, Tmax), NAN), traj_bounds=torch.full((E, Tmax), 7, dtype=torch.uint8),
             rng=rng_buf(seed, upd, soff), episode_of_slot=torch.randint(0, 1000, (E, 1), generator=g, dtype=torch.int32))
    Wh1 = rnd(g, 4 * d, in_dim, scale=1 / math.sqrt(in_dim))
    Wh2 = torch.zeros(na2, 4 * d)
    Wh2[:A, :2 * d] = rnd(g, A, 2 * d, scale=1 / math.sqrt(2 * d))
    Wh2[A:, 2 * d:] = rnd(g, Bn, 2 * d, scale=1 / math.sqrt(2 * d))
    bh2 = torch.zeros(1, n2)
    bh2[0, :na2] = rnd(g, na2, scale=0.5)
    w2t = torch.zeros(4 * d, n2)
    w2t[:, :na2] = Wh2.t()                                  # (header: padding columns zero)
    B.update(w_h1_t=Wh1.t().contiguous(), b_h1=row(rnd(g, 4 * d, scale=0.3)), w_h2_t=w2t, b_h2=bh2)
    if alibi:
        B['alibi'] = row(2. ** -(8. * (torch.arange(H).float() + 1) / H))
    if vres:
        B['v1'] = nan_out(E, Ikv)
    desc = base_desc(E, d, Tmax, S=S, A=A, B=Bn, L=L, H=H, dh=dh, Hkv=Hkv, ff=ff, in_dim=in_dim, n_qkv=n_qkv, gate_values=c.gate,
                     value_residual=vres, learned_mix=vres, rotary_abs=1, rot_dim=rot_dim, sim_mode=1, hazard_log2=2, rs_eps=1e-5,
                     rms_norm=c.rms, attn_window=c.W, attn_softclamp=cap, num_mem_kv=M, add_zero_kv=zkv, layers_dev=True,
                     alibi_slopes='alibi' if alibi else None, v1='v1' if vres else None)
    for k_ in ('w_pin', 'b_pin', 'act_emb', 'reward_embed', 'w_se', 'b_se', 'ln_final', 'b_h1', 'b_h2', 'inv_freq', 'rs_mean', 'rs_var',
               'state', 'prev_action', 'prev_reward', 'alive', 'lens', 'cum_reward', 'episode_of_slot', 'rng', 'traj_states', 'traj_actions',
               'traj_logp', 'traj_rewards', 'traj_bounds', 'traj_values', 'logits', 'w_h1_t', 'w_h2_t'):
        desc[k_] = k_
    layers, P = [], []
    for l in range(L):
        Wq = rnd(g, n_qkv, d, scale=1 / math.sqrt(d))
        wqt = torch.zeros(d, nq4)
        wqt[:, :n_qkv] = Wq.t()                             # (header: padding columns zero)
        bq = torch.zeros(1, nq4)
        bq[0, I + 2 * Ikv:n_qkv] = rnd(g, n_qkv - I - 2 * Ikv, scale=0.5)
        Wo, W1, W2 = rnd(g, d, I, scale=1 / math.sqrt(I)), rnd(g, ff, d, scale=1 / math.sqrt(d)), rnd(g, d, ff, scale=1 / math.sqrt(ff))
        kc, vc = torch.full((E, Hkv, Tmax, dh), NAN), torch.full((E, Hkv, Tmax, dh), NAN)
        kc[slots, :, j_lo:t] = rnd(g, nl, Hkv, t - j_lo, dh)
        vc[slots, :, j_lo:t] = rnd(g, nl, Hkv, t - j_lo, dh)
        nm = lambda s_: f'{s_}{l}'   # noqa: E731
        B.update({nm('ln_attn'): row(gain(g, d)), nm('w_qkv_t'): wqt, nm('b_qkv'): bq, nm('w_out_t'): Wo.t().contiguous(),
                  nm('ln_ff'): row(gain(g, d)), nm('w_ff1_t'): W1.t().contiguous(), nm('b_ff1'): row(rnd(g, ff, scale=0.3)),
                  nm('w_ff2_t'): W2.t().contiguous(), nm('b_ff2'): row(rnd(g, d, scale=0.3)), nm('k_cache'): kc.reshape(-1, dh),
                  nm('v_cache'): vc.reshape(-1, dh)})
        ly = {k_: nm(k_) for k_ in ('ln_attn', 'w_qkv_t', 'b_qkv', 'w_out_t', 'ln_ff', 'w_ff1_t', 'b_ff1', 'w_ff2_t', 'b_ff2', 'k_cache', 'v_cache')}
        if M:
            B[nm('mem_k')], B[nm('mem_v')] = rnd(g, Hkv * M, dh), rnd(g, Hkv * M, dh)
            ly.update(mem_k=nm('mem_k'), mem_v=nm('mem_v'))
        layers.append(ly)
        P.append(dict(Wq=Wq, bq=bq[0, :n_qkv], Wo=Wo, W1=W1, W2=W2, kc=kc, vc=vc))
    outs = ['alive', 'live_rows', 'live_count', 'traj_states', 'logits', 'traj_values', 'state', 'prev_action', 'prev_reward', 'lens',
            'cum_reward', 'traj_actions', 'traj_logp', 'traj_rewards', 'traj_bounds'] + [f'k_cache{l}' for l in range(L)] \
        + [f'v_cache{l}' for l in range(L)] + (['v1'] if vres else [])
    info = {}
    kvh = torch.arange(H) % Hkv

    def mx(x):           # a row's largest magnitude, fp64
        return x.double().abs().reshape(x.shape[0], -1).max(-1).values

    def dn(a, W, b, u):  # a W^T + b with its per-element unit: the input's unit through |W|, the sum's own rounding
        y = seqsum(a[:, None, :] * W[None], 2)
        s = a.double().abs() @ W.double().abs().t()
        if b is not None:
            y = y + b
            s = s + b.double().abs()
        return y, EPS24 * (s + y.double().abs())      # (u: unused; the sum's own 2^-24 sum |terms|)

    def lnr(x, gn, u):
        return ln_rows(x, c.rms)[0] * gn, None

    def expect(dt, taken=None):
        f = lambda k_: B[k_].to(dt)   # noqa: E731
        n = nl
        xv = torch.cat([f('state')[slots], f('prev_reward')[slots]], 1)
        ns = (xv - f('rs_mean')) / torch.sqrt(f('rs_var')).clamp_min(torch.tensor(1e-5, dtype=torch.float32).to(dt))
        p = seqsum(ns[:, None, :S] * f('w_pin')[None], 2) + f('b_pin')
        se = seqsum(ns[:, None, :S] * f('w_se')[None], 2) + f('b_se')
        a_prev = B['prev_action'][slots, 0].long()
        ak = f('act_emb')[a_prev.clamp_min(0)] * (a_prev >= 0).to(dt)[:, None]
        x = p + (ak + ns[:, S:S + 1] * f('reward_embed'))
        u = u_se = None
        R = []
        theta = torch.zeros(dh, dtype=torch.float64)
        ch = torch.arange(rot_dim)
        ang = torch.tensor(float(t), dtype=torch.float32).to(dt) * f('inv_freq')[0][ch // 2]
        theta[:rot_dim] = ang.double().abs()
        cs, sn, sgn = torch.cos(ang), torch.sin(ang), torch.where(ch % 2 == 1, 1., -1.).to(dt)
        rot = lambda z: torch.cat([z[..., :rot_dim] * cs + (sgn * z[..., :rot_dim][..., ch ^ 1]) * sn, z[..., rot_dim:]], -1)   # noqa: E731
        thm = float(theta.max())
        v1 = u_v1 = None
        scale = 1.0 / math.sqrt(dh)
        for l in range(L):
            Q = P[l]
            xn, u_n = lnr(x, f(f'ln_attn{l}'), u)
            qkv, u_q = dn(xn, Q['Wq'].to(dt), Q['bq'].to(dt), u_n)
            q = qkv[:, :I].reshape(n, H, dh)
            k = qkv[:, I:I + Ikv].reshape(n, Hkv, dh)
            v = qkv[:, I + Ikv:I + 2 * Ikv].reshape(n, Hkv, dh)
            uq, uk = u_q[:, :I].reshape(n, H, dh), u_q[:, I:I + Ikv].reshape(n, Hkv, dh)
            uv = u_q[:, I + Ikv:I + 2 * Ikv].reshape(n, Hkv, dh)
            u_v = uv
            if vres and l == 0:
                v1, u_v1 = v, uv
                R.append(Region('v1', v.reshape(n, Ikv), C_COMP['row_kv'] * uv.reshape(n, Ikv), fam='row_kv', unit=uv.reshape(n, Ikv)))
            elif vres:
                wm = 1.0 / (1.0 + torch.exp(-qkv[:, n_qkv - Hkv:].reshape(n, Hkv, 1)))
                u_v = uv + u_v1 + EPS24 * (v.double().abs() + v1.double().abs())
                v = torch.where(wm.abs() < 0.5, v + wm * (v1 - v), v1 - (v1 - v) * (1.0 - wm))
            part = torch.arange(dh)
            part[:rot_dim] = part[:rot_dim] ^ 1
            q, k = rot(q), rot(k)
            pair = lambda z: z.double().abs() + z.double().abs()[..., part]   # noqa: E731
            uq = uq + uq[..., part] + 2 * EPS24 * (theta + 1) * pair(q)              # rotated: the pair, the angle's rounding
            uk = uk + uk[..., part] + 2 * EPS24 * (theta + 1) * pair(k)
            for r_, e in enumerate(slots.tolist()):
                for kh in range(Hkv):
                    r0 = (e * Hkv + kh) * Tmax + t
                    R.append(Region(f'k_cache{l}', k[r_, kh:kh + 1], C_COMP['row_kv'] * uk[r_, kh:kh + 1], r0=r0, fam='row_kv', unit=uk[r_, kh:kh + 1]))
                    R.append(Region(f'v_cache{l}', v[r_, kh:kh + 1], C_COMP['row_kv'] * u_v[r_, kh:kh + 1], r0=r0, fam='row_kv', unit=u_v[r_, kh:kh + 1]))
            Kall = torch.cat([Q['kc'][slots][:, kvh, j_lo:t].to(dt), k[:, kvh, None]], 2)
            Vall = torch.cat([Q['vc'][slots][:, kvh, j_lo:t].to(dt), v[:, kvh, None]], 2)
            s = seqsum(q[:, :, None, :] * Kall, 3) * scale
            s_abs = (q.double().abs()[:, :, None, :] * Kall.double().abs()).sum(3) * scale
            if alibi:
                bias = f('alibi')[0][None, :, None] * torch.arange(t - j_lo, -1, -1, dtype=torch.float32).to(dt)
                s, s_abs = s - bias, s_abs + bias.double()
            if M:
                mk = f(f'mem_k{l}').reshape(Hkv, M, dh)[kvh]
                s = torch.cat([s, seqsum(q[:, :, None, :] * mk[None], 3) * scale], 2)
                s_abs = torch.cat([s_abs, (q.double().abs()[:, :, None, :] * mk.double().abs()[None]).sum(3) * scale], 2)
                Vall = torch.cat([Vall, f(f'mem_v{l}').reshape(Hkv, M, dh)[kvh][None].expand(n, -1, -1, -1)], 2)
            if cap > 0:
                s = cap * torch.tanh(s * (1.0 / cap))
            if zkv:
                s = torch.cat([s, torch.zeros(n, H, 1, dtype=dt)], 2)
                Vall = torch.cat([Vall, torch.zeros(n, H, 1, dh, dtype=dt)], 2)
            pr = torch.exp(s - s.max(-1, keepdim=True).values)
            o = seqsum(pr[..., None] * Vall, 2) / seqsum(pr, 2)[..., None]
            if c.gate:
                o = o * (1.0 / (1.0 + torch.exp(-qkv[:, I + 2 * Ikv:I + 2 * Ikv + I].reshape(n, H, dh))))
            y, u_y = dn(o.reshape(n, I), Q['Wo'].to(dt), None, None)
            x = x + y
            xn, u_n = lnr(x, f(f'ln_ff{l}'), u)
            pre, u_p = dn(xn, Q['W1'].to(dt), f(f'b_ff1{l}'), u_n)
            hh = gelu(pre)
            y, u_y = dn(hh, Q['W2'].to(dt), f(f'b_ff2{l}'), None)
            x = x + y
        xf, u_f = lnr(x, f('ln_final'), u)
        ac = torch.cat([xf, se], 1)
        pre, u_p = dn(ac, Wh1.to(dt), f('b_h1'), None)
        hid = pre / (1.0 + torch.exp(-pre))
        out, u_l = dn(hid, Wh2.to(dt), f('b_h2')[:, :na2], None)
        R.append(Region('logits', out[:, :A], C_COMP['row_out'] * u_l[:, :A], fam='row_out', unit=u_l[:, :A]))
        bl = C_COMP['row_out'] * u_l[:, :A].max(-1).values
        Lg = out[:, :A]
        ex = torch.exp(Lg - Lg.max(-1, keepdim=True).values)
        qn = ex / seqsum(ex, 1)[:, None]
        pp = qn / seqsum(qn, 1)[:, None]
        cdf = pp.cumsum(1)[:, :A - 1]
        after = torch.where(al == 3 + ((t + 1) & 1), torch.zeros_like(al), al)
        rows_after = B['live_rows'].clone()
        rows_after[t & 1, :n] = slots.to(torch.int32)
        R += [Region('live_rows', rows_after[t & 1:(t & 1) + 1, :n], None, r0=t & 1),
              Region('live_count', torch.tensor([[n]], dtype=torch.int32), None, c0=t & 1)]
        a_ref, ties = [], 0
        for r_, e in enumerate(slots.tolist()):
            R.append(Region('traj_states', B['state'][e:e + 1].clone(), None, r0=e * Tmax + t))
            R.append(Region('traj_values', out[r_:r_ + 1, A:], C_COMP['row_out'] * u_l[r_:r_ + 1, A:], r0=e * Tmax + t, fam='row_out',
                            unit=u_l[r_:r_ + 1, A:]))
            if int(al[e]) == 2:
                a_ref.append(-1)
                continue
            uu = torch.tensor(PH.philox_uniform(seed, upd, soff + e, t, PH.FIELD_SAMPLE, 1)[0]).to(dt)
            act = int((uu >= cdf[r_]).sum())
            delta = A * float((pp[r_].double() * 2 * bl[r_] + 4 * EPS24).max())
            lo, hi = int((uu.double() >= cdf[r_].double() + delta).sum()), int((uu.double() >= cdf[r_].double() - delta).sum())
            a_ref.append(act)
            if lo != hi:
                ties += 1
                if taken is not None and lo <= int(taken[r_]) <= hi:
                    act = int(taken[r_])
            logp = torch.log(pp[r_, act].clamp(F32_EPS, 1. - F32_EPS))
            av = torch.tensor([[act]], dtype=torch.int32)
            ulp = (2 * bl[r_] + EPS24 * (A + logp.double().abs())).reshape(1, 1)
            ep = int(B['episode_of_slot'][e, 0])
            zr = PH.philox_uniform(seed, upd, ep, t, PH.FIELD_REWARD, 1, normal=True)[0]
            rw = torch.tensor([[float(np.float32(zr * PH.REWARD_FACTORS[act]))]], dtype=torch.float32)
            term = (int(PH.philox_u32(seed, upd, ep, t, PH.FIELD_TERM)) & 3) == 0
            R += [Region('traj_actions', av, None, r0=e, c0=t), Region('prev_action', av, None, r0=e),
                  Region('traj_logp', logp.reshape(1, 1), C_COMP['row_lp'] * ulp, r0=e, c0=t, fam='row_lp', unit=ulp),
                  Region('state', philox_states(seed, upd, [ep], t + 1, S), None, r0=e),
                  Region('traj_rewards', rw, None, r0=e, c0=t), Region('prev_reward', rw, None, r0=e),
                  Region('traj_bounds', torch.tensor([[int(term)]], dtype=torch.uint8), None, r0=e, c0=t),
                  Region('cum_reward', B['cum_reward'][e:e + 1] + rw.double(), None, r0=e),
                  Region('lens', torch.tensor([[t + 1]], dtype=torch.int32), None, r0=e)]
            if term or t + 1 >= Tmax:
                after[e] = 3 + (t & 1)            # (the row step never turns a slot it ranks from live to dead)
        R.append(Region('alive', row(after), None))
        info.update(a_ref=a_ref, ties=ties)
        return R

    return DSpec(c.id, 'STEP_ROWS', B, tuple(outs), desc, layers, t=t, call=dict(max_rows=c.max_rows), form=row_kernel(c), expect=expect,
                 info=info)
