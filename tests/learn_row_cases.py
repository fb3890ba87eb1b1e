"""Seeded inputs, case tables and fp64 references for the row kernels of the learn step (csrc/train.hip through
xtrl_learn_rows): the embeddings, LayerNorm forward / backward, the rotary / qk-norm / value-mix pass and its
backward, the deterministic column sums and their deferred queue, the action-embedding and gene gradients, the
valid-row list with its gather / scatter, and the fractal step's row kernels.

Imported by test_learn_rows_cpu.py (which settles every closed form against torch.autograd and the oracle's
modules, the bounds against a plain fp32 restatement, the tables against a restatement of the launchers' integer
arithmetic, and the C ABI, without a GPU) and by test_learn_rows_gpu.py (which runs the kernels).  Plain PyTorch
on the CPU; defines no tests.  Inputs are fp32, a reference widens them to fp64 first.

A case is a `Spec`: the buffers of one call (inputs, and outputs with their prefill), the slots of the
XtrlRowsDesc, and `expect(dtype)`, the regions the call owns with their references in `dtype` and their bounds.
Layout.  Where a kernel takes a row stride the buffer's stride is wider than its data; every output has guard rows
(a vector: guard elements) past its last one.  Outputs are NaN before the call unless the kernel accumulates or
works in place (then: seeded non-zero values); inputs' padding columns hold 1e30.  `verify` compares every owned
element and requires every other element of an output to keep its bits.

Bounds (none is taken from the kernels):
  element-wise O(1) outputs (embeddings, normalised rows, rotated pairs, mixed values, dx rows, d mix): the
      project's |x - ref| <= 1e-5 + 1e-5 |ref|; rstd to a relative 1e-5; LayerNorm-backward rows with the absolute
      part scaled by max(1, rstd[m]) (gemm_epi_cases); the 1 / 1e-12 gradient of an all-zero head relative only.
  sums over rows, steps, episodes or chunks: C x 2^-24 x sum |terms| (an accumulated-onto old value counts as a
      term), one C per family.  Each C is four times the worst error of the sequential fp32 restatement against
      fp64 over the family's table, in units of 2^-24 sum |terms|, rounded up.
  copies and integer lists: exact.

Measured (test_learn_rows_cpu.py::test_fp32_restatement_within_a_quarter_of_each_bound prints them, pytest -s;
worst over every case of the tables):
  family       restatement error / (2^-24 sum |terms|)    C     restatement / bound
  ln_dgamma    2.60  (each term g x^ is itself rounded)   11    0.24
  colsum       1.39  (the queue's partials included)      6     0.23
  embed_grad   1.70                                       7     0.25
  latent       1.85  (d w; d lat 0.99, d b 1.49)          8     0.12 (d lat), 0.23 (d w), 0.19 (d b): d w and d b are
                                                                sums of d lat, restated with d lat's fp32 error in
  causal_mean  1.50                                       6     0.25
  element-wise outputs, restatement error as a share of the bound: embed x0 0.06, state embed 0.07, next-action
  embed 0.03, embed_ln xn 0.04, (mean, rstd) 0.03; ln_fwd y 0.06, (mean, rstd) 0.02; ln_bwd dx 0.04; latent_embed
  0.02; qkv_prep 0.03; qkv_prep_bwd 0.05; rows_axpb 0.01.
Two input families were shaped by the restatement, before any kernel ran (the bounds were not touched):
  xPos.  Base 16 runs on the padded form (n = 7) and base 512 on the packed one (n = 500, positions to 499), so the
  factor ((j + 0.4 rot) / (1.4 rot)) ^ ((pos - n // 2) / base) stays within 0.5 .. 1.9 and a rotated pair O(1)
  (prep_xpos).  Base 16 at n = 500 would span 3.4e-9 .. 3.2e8: absolute errors of the pair scale with it and the
  restatement itself left the element-wise bound.
  Zero heads.  The gradient pairs of an all-zero head have a zero odd channel, so the inverse rotation
  g0 cos + g1 sin cannot cancel (a cancelling sum has no relative accuracy and the 1 / 1e-12 gradient is held
  relative only).
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import torch

from gemm_epi_cases import BIG, EPS24, NAN, _gen, bits, fwd_bound, ln_bwd, ln_rows, round4

OPS = ('EMBED', 'LATENT_EMBED', 'LN_FWD', 'LN_BWD', 'QKV_PREP', 'QKV_PREP_BWD', 'COLSUM', 'COLSUM_FINAL',
       'COLSUM_QUEUE', 'EMBED_GRAD', 'LATENT_GRAD', 'VALID_ROWS', 'GATHER', 'SCATTER', 'CAUSAL_MEAN', 'AXPB',
       'ACTION_ROWS', 'BCAST_EP')
OP = {name: i for i, name in enumerate(OPS)}

# the constants of the sum bounds (module docstring)
C_SUM = dict(ln_dgamma=11., colsum=6., embed_grad=7., latent=8., causal_mean=6.)
ISENT = -7777   # prefill of an int32 output


def seqsum(x, dim=0):
    """The sum along `dim` taken element after element in x's precision (a plain sequential sum)."""
    return x.cumsum(dim).select(dim, -1)


def padded(t, ld, fill=BIG):
    out = torch.full((t.shape[0], ld), fill, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


def guarded(t, rows=2, fill=NAN):
    """t [R][C] with `rows` guard rows of `fill` after it."""
    return torch.cat([t, torch.full((rows, t.shape[1]), fill, dtype=t.dtype)])


def nan_out(rows, ld, guard=2):
    return torch.full((rows + guard, ld), NAN)


def vec_out(values, guard=4, fill=NAN):
    """A vector output [1][len + guard] holding `values` (its old contents) and guard elements."""
    return torch.cat([values.reshape(-1), torch.full((guard,), fill, dtype=values.dtype)]).reshape(1, -1)


@dataclass
class Region:
    buf: str
    ref: torch.Tensor | None      # [R][C] (None: owned, any value — a workspace)
    bound: torch.Tensor | None    # per element (None: exact, compared bit for bit)
    r0: int = 0
    c0: int = 0
    fam: str = 'elementwise'
    unit: torch.Tensor | None = None   # sums: 2^-24 sum |terms| per element
    shape: tuple | None = None


@dataclass
class Spec:
    id: str
    op: str
    bufs: dict                    # name -> CPU tensor as uploaded (outputs: their prefill)
    outs: tuple                   # names of the buffers the call may write
    in_: tuple = ()               # slot -> buffer name, (name, element offset) or None
    out: tuple = ()
    ld: tuple = ()
    n: tuple = ()
    f: tuple = ()
    part: str | None = None
    part_floats: int = 0
    jobs: tuple = ()              # COLSUM_QUEUE: (part buffer, (dst buffer, offset), chunks, cols)
    expect: object = None         # dtype -> [Region]
    info: dict = field(default_factory=dict)


def sum_region(buf, ref, terms_abs, fam, **kw):
    """A sum's region: bound C x 2^-24 x sum |terms|."""
    unit = EPS24 * terms_abs
    return Region(buf, ref, C_SUM[fam] * unit.double(), fam=fam, unit=unit.double(), **kw)


def verify(spec, after, regions):
    """Every owned element finite and inside its bound (exact regions: equal bits); every other element of every
    output buffer keeps its prefill bits.  Returns the worst error / bound per (family, buffer)."""
    worst = {}
    owned = {k: torch.zeros(spec.bufs[k].shape, dtype=torch.bool) for k in spec.outs}
    for r in regions:
        got_all = after[r.buf]
        if r.ref is None:
            R_, C_ = r.shape
            owned[r.buf][r.r0:r.r0 + R_, r.c0:r.c0 + C_] = True
            continue
        ref = r.ref.reshape(r.ref.shape[0], -1) if r.ref.dim() > 1 else r.ref.reshape(1, -1)
        R_, C_ = ref.shape
        got = got_all[r.r0:r.r0 + R_, r.c0:r.c0 + C_]
        owned[r.buf][r.r0:r.r0 + R_, r.c0:r.c0 + C_] = True
        what = f'{spec.id} {r.buf}[{r.r0}:, {r.c0}:]'
        if r.bound is None:
            same = bits(got) == bits(ref.to(got.dtype)) if got.dtype == torch.float32 else got == ref.to(got.dtype)
            assert bool(same.all()), f'{what}: {int((~same).sum())} elements differ (exact comparison)'
            continue
        assert bool(torch.isfinite(got).all()), f'{what}: non-finite owned elements'
        ratio = (got.double() - ref.double()).abs() / r.bound.reshape(R_, C_)
        ratio = torch.where((got.double() == ref.double()), torch.zeros_like(ratio), ratio)
        w = float(ratio.max())
        i = divmod(int(ratio.argmax()), C_)
        assert w <= 1., f'{what}: error {w:.3f} of the bound at {i}: {float(got[i])} vs {float(ref[i])}'
        key = f'{r.fam} {r.buf}'
        worst[key] = max(worst.get(key, 0.), w)
    for k in spec.outs:
        a, b = after[k], spec.bufs[k]
        same = bits(a) == bits(b) if a.dtype == torch.float32 else a == b
        assert bool(same[~owned[k]].all()), f'{spec.id} {k}: elements outside the owned regions were written'
    return worst


# ----------------------------------------------------------------------------------------------
# 1. embeddings
# ----------------------------------------------------------------------------------------------

EMB_D_BOTH, EMB_D_PLAIN = (4, 48, 192, 256), (260, 512)
# (S, A, continuous): every state width (8: the <8> instantiation), discrete and continuous action counts
EMB_SA = [(1, 1, 0), (8, 4, 0), (13, 5, 0), (32, 9, 0), (8, 32, 0), (13, 1, 1), (8, 6, 1)]


@dataclass(frozen=True)
class EmbedCase:
    ln: int
    d: int
    S: int
    A: int
    cont: int
    T: int
    evo: int
    packed: int
    rms: int
    keep: float

    @property
    def n(self):
        return 15

    @property
    def b(self):          # episodes the gene rows index (packed: 5 episodes hold the 45 listed rows)
        return 5 if self.packed else max(1, self.T // self.n)

    @property
    def in_dim(self):
        return 3 * self.d + 4

    @property
    def id(self):
        return (f"embed{'_ln' if self.ln else ''}-d{self.d}-S{self.S}-A{self.A}{'c' if self.cont else ''}-T{self.T}"
                f"-evo{self.evo}-pk{self.packed}-rms{self.rms}-keep{self.keep:g}")


def _embed_cases():
    out = []
    for ln in (0, 1):
        for di, d in enumerate(EMB_D_BOTH + (() if ln else EMB_D_PLAIN)):
            for i, (S, A, cont) in enumerate(EMB_SA):
                k = i + di
                out.append(EmbedCase(ln, d, S, A, cont, 45, k % 2, (k // 2) % 2, (i + 1) % 2 if ln else 0,
                                     float((k // 2 + i) % 2)))
        for i, (S, A, cont) in enumerate(EMB_SA[1:4]):
            out.append(EmbedCase(ln, 48, S, A, cont, 1, i % 2, 0, i % 2 if ln else 0, 1.))
    return out


EMBED_CASES = _embed_cases()


def embed_rows_list(c: EmbedCase):
    """The packed row list: 45 of the 75 rows of 5 episodes, increasing; row / n differs from t / n."""
    g = _gen(11, c.d, c.S)
    return torch.randperm(c.b * c.n, generator=g)[:c.T].sort().values.to(torch.int32)


def embed_spec(c: EmbedCase):
    T, S, A, d = c.T, c.S, c.A, c.d
    g = _gen(10, c.ln, d, S, A, c.cont, T)
    B = dict(swr=torch.randn(T, S + 1, generator=g), w_pin=torch.randn(d, S, generator=g) / math.sqrt(S),
             reward_embed=torch.randn(d, generator=g), w_se=torch.randn(d, S, generator=g) / math.sqrt(S),
             b_se=torch.randn(d, generator=g), lat_e=torch.randn(c.b, d, generator=g),
             ln_g=torch.rand(d, generator=g) * 0.5 + 0.5)
    if c.cont:
        B['act_emb'] = torch.randn(d, A, generator=g) / math.sqrt(A)
        B['act_emb_b'] = torch.randn(d, generator=g)
        B['prev_af'] = torch.randn(T, A, generator=g)
        B['next_af'] = torch.randn(T, A, generator=g)
    else:
        B['act_emb'] = torch.randn(A, d, generator=g)
        B['prev_a'] = torch.randint(-1, A, (T,), generator=g, dtype=torch.int32)
        B['next_a'] = torch.randint(-1, A, (T,), generator=g, dtype=torch.int32)
        B['prev_a'][0] = -1
        B['next_a'][T - 1] = -1
    if c.packed:
        B['rows'] = embed_rows_list(c)
    B.update(x0=nan_out(T, d), ac_in=nan_out(T, c.in_dim), ewa=nan_out(T, 2 * d))
    outs = ['x0', 'ac_in', 'ewa']
    if c.ln:
        B.update(xn=nan_out(T, d), st=nan_out(T, 2))
        outs += ['xn', 'st']
    nm = lambda k: k if k in B else None   # noqa: E731
    in_ = ('swr', 'w_pin', 'act_emb', nm('act_emb_b'), 'reward_embed', 'w_se', 'b_se', 'lat_e' if c.evo else None,
           nm('prev_af'), nm('next_af'), nm('prev_a'), nm('next_a'), 'ln_g' if c.ln else None, nm('rows'))

    def expect(dt):
        st = B['swr'][:, :S].to(dt)
        rw = B['swr'][:, S].to(dt)
        if c.cont:
            w, bb = B['act_emb'].to(dt), B['act_emb_b'].to(dt)
            ap, an = B['prev_af'].to(dt) @ w.t() + bb, B['next_af'].to(dt) @ w.t() + bb
        else:   # SafeEmbedding: a negative action embeds as zeros
            w = B['act_emb'].to(dt)
            emb = lambda a: torch.where((a >= 0)[:, None], w[a.clamp_min(0).long()], torch.zeros((), dtype=dt))   # noqa: E731
            ap, an = emb(B['prev_a']), emb(B['next_a'])
        x0 = st @ B['w_pin'].to(dt).t() + (ap + (rw[:, None] * B['reward_embed'].to(dt)) * c.keep)
        se = st @ B['w_se'].to(dt).t() + B['b_se'].to(dt)
        R = [Region('x0', x0, fwd_bound(x0.double())), Region('ac_in', se, fwd_bound(se.double()), c0=d),
             Region('ewa', an, fwd_bound(an.double()), c0=d)]
        if c.evo:
            rows = B['rows'].long() if c.packed else torch.arange(T)
            R.append(Region('ac_in', B['lat_e'][rows // c.n], None, c0=2 * d))
        if c.ln:
            xh, mean, rstd = ln_rows(x0, c.rms)
            xn = xh * B['ln_g'].to(dt)
            R += [Region('xn', xn, fwd_bound(xn.double())), Region('st', mean[:, None], fwd_bound(mean.double()[:, None])),
                  Region('st', rstd[:, None], 1e-5 * rstd.double().abs()[:, None], c0=1)]
        return R
    return Spec(c.id, 'EMBED', B, tuple(outs), in_=in_, out=('x0', 'ac_in', 'ewa', nm('xn'), nm('st')),
                n=(T, c.n, S, A, d, c.in_dim, c.cont, c.evo, c.rms, c.ln), f=(c.keep,), expect=expect)


LATENT_EMBED_CASES = [(b, G, 48) for b in (1, 9) for G in (1, 5)]


def latent_embed_spec(b, G, d):
    g = _gen(12, b, G, d)
    B = dict(latent=torch.randn(b, G, generator=g), w=torch.randn(d, G, generator=g), bias=torch.randn(d, generator=g),
             out=nan_out(b, d))

    def expect(dt):
        r = B['latent'].to(dt) @ B['w'].to(dt).t() + B['bias'].to(dt)
        return [Region('out', r, fwd_bound(r.double()))]
    return Spec(f'latent_embed-b{b}-G{G}', 'LATENT_EMBED', B, ('out',), in_=('latent', 'w', 'bias'), out=('out',),
                n=(b, G, d), expect=expect)


# ----------------------------------------------------------------------------------------------
# 2. LayerNorm forward / backward (the unfused path: d > 256 or an operand off the float4 grid)
# ----------------------------------------------------------------------------------------------

LN_DS = (4, 64, 68, 128, 192, 256, 260, 512)   # every DPL (1, 2, 4, 8) and the ragged last 64-column group
LN_TS = (1, 16, 17, 37)                        # one row; a whole 16-row block; a block and a row; three blocks
LN_ROWS = 16
# g2 (ldg2 = d + 8) | s1 | dres aliasing dx | d beta adjacent to d gamma
LN_BWD_VARIANTS = {'plain': (0, 1., 0, 0), 'g2': (1, 1., 0, 0), 's1': (0, 0.25, 0, 0), 'dres': (0, 1., 1, 0),
                   'final': (1, 0.25, 1, 0), 'beta': (0, 1., 0, 1), 'all': (1, 0.25, 1, 1)}


def ln_dpl(d):
    return 1 if d <= 64 else 2 if d <= 128 else 4 if d <= 256 else 8


def ln_fwd_spec(d, T, rms, y2):
    g = _gen(20, d, T, rms)
    x = torch.randn(T, d, generator=g) * 1.5 + 0.3
    if T >= 16:
        x[1] = 8. + torch.randn(d, generator=g)   # a row far from zero: the variance must be the centred one
        x[T - 1] = 0.                             # the padded-token row
    B = dict(x=x, gamma=torch.rand(d, generator=g) * 0.5 + 0.5, y1=nan_out(T, d + 4), st=nan_out(T, 2))
    if y2:
        B['y2'] = nan_out(T, d + 8)

    def expect(dt):
        xh, mean, rstd = ln_rows(B['x'].to(dt), rms)
        y = xh * B['gamma'].to(dt)
        R = [Region('y1', y, fwd_bound(y.double())), Region('st', mean[:, None], fwd_bound(mean.double()[:, None])),
             Region('st', rstd[:, None], 1e-5 * rstd.double().abs()[:, None], c0=1)]
        if y2:
            R.append(Region('y2', y, fwd_bound(y.double())))
        return R
    return Spec(f'ln_fwd-d{d}-T{T}-rms{rms}-y2{y2}', 'LN_FWD', B, ('y1', 'st') + (('y2',) if y2 else ()),
                in_=('x', 'gamma'), out=('y1', 'y2' if y2 else None, 'st'), ld=(d + 4, d + 8 if y2 else 0),
                n=(T, d, rms), expect=expect)


LN_FWD_CASES = [(d, T, rms, (i + j + rms) % 2) for i, d in enumerate(LN_DS) for j, T in enumerate(LN_TS)
                for rms in (0, 1)]
LN_BWD_CASES = [(d, T, rms, v) for d in LN_DS for T in LN_TS for rms in (0, 1) for v in LN_BWD_VARIANTS]


def ln_part_floats(T, d, beta):
    return -(-T // LN_ROWS) * d * (2 if beta else 1)


def ln_bwd_spec(d, T, rms, variant):
    has_g2, s1, alias, beta = LN_BWD_VARIANTS[variant]
    g = _gen(21, d, T, rms, sorted(LN_BWD_VARIANTS).index(variant))
    x = torch.randn(T, d, generator=g) * 1.5 + 0.3
    _, mean, rstd = ln_rows(x.double(), rms)
    B = dict(x=x, stats=torch.stack([mean, rstd], 1).float(), gamma=torch.rand(d, generator=g) + 0.5,
             g1=padded(torch.randn(T, d, generator=g), d + 4))
    if has_g2:
        B['g2'] = padded(torch.randn(T, d, generator=g), d + 8)
    dres = torch.randn(T, d, generator=g)
    B['dx'] = guarded(dres) if alias else nan_out(T, d)
    old = torch.randn((2 if beta else 1) * d, generator=g)
    B['dgb'] = vec_out(old)          # d gamma (| d beta), accumulated onto
    pf = ln_part_floats(T, d, beta)
    B['part'] = torch.full((1, pf + 4), NAN)

    def expect(dt):
        gv = s1 * B['g1'][:, :d].to(dt)
        gmag = gv.abs()
        if has_g2:
            gv = gv + B['g2'][:, :d].to(dt)
            gmag = gmag + B['g2'][:, :d].to(dt).abs()
        st = B['stats'].to(dt)
        dx, xh = ln_bwd(gv, B['x'].to(dt), st[:, 0], st[:, 1], B['gamma'].to(dt), rms)
        if alias:
            dx = dx + dres.to(dt)
        rs = B['stats'][:, 1].double().clamp_min(1.)[:, None]
        o = old.to(dt)
        dg = o[:d] + seqsum(gv * xh)
        R = [Region('dx', dx, 1e-5 * rs + 1e-5 * dx.double().abs(), fam='ln_bwd_rows'),
             sum_region('dgb', dg, o[:d].abs() + (gmag * xh.abs()).sum(0), 'ln_dgamma'),
             Region('part', None, None, shape=(1, pf))]
        if beta:
            R.append(sum_region('dgb', o[d:] + seqsum(gv), o[d:].abs() + gmag.sum(0), 'ln_dgamma', c0=d))
        return R
    return Spec(f'ln_bwd-d{d}-T{T}-rms{rms}-{variant}', 'LN_BWD', B, ('dx', 'dgb', 'part'),
                in_=('g1', 'g2' if has_g2 else None, 'x', 'stats', 'gamma', 'dx' if alias else None),
                out=('dx', 'dgb', ('dgb', d) if beta else None), ld=(d + 4, d + 8 if has_g2 else 0),
                n=(T, d, rms), f=(s1,), part='part', part_floats=pf, expect=expect)


# ----------------------------------------------------------------------------------------------
# 3. rotary / qk norm / xPos / value-residual mix, and the backward
# ----------------------------------------------------------------------------------------------

PREP_T = 128
PREP_GEOM = [(4, 4, 16), (4, 2, 16), (3, 1, 32), (5, 5, 32), (1, 1, 64), (8, 8, 64)]   # (H, Hkv, dh)
PREP_XPOS = (0., 16., 512.)
PREP_MIX = ('off', 'gate', 'nogate')     # mix on: with / without the gate columns between v and the mix column
MIX_PRE = (-20., -1., -1e-3, 1e-3, 1., 20.)
# backward (first_layer, accumulate, mix)
PREP_BWD_MODES = [(0, 0, 1), (0, 1, 1), (1, 1, 1), (1, 1, 0), (1, 0, 0)]


@dataclass(frozen=True)
class PrepCase:
    H: int
    Hkv: int
    dh: int
    rot: int
    packed: int
    qk_norm: int
    xpos: float
    mix: str
    first_layer: int = 0
    accumulate: int = 0
    bwd: int = 0

    @property
    def I(self):   # noqa: E743
        return self.H * self.dh

    @property
    def Ikv(self):
        return self.Hkv * self.dh

    @property
    def nq3(self):
        return self.I + 2 * self.Ikv

    @property
    def P(self):
        return self.nq3 // 2

    @property
    def b(self):
        return 2

    @property
    def n(self):
        return 500 if self.packed else 7

    @property
    def T(self):
        return 9 if self.packed else 14

    @property
    def gate(self):
        return self.mix != 'nogate'     # (mix off: the gate columns alone follow v)

    @property
    def mix_col(self):
        return -1 if self.mix == 'off' else self.nq3 + (self.I if self.gate else 0)

    @property
    def n_qkv(self):                    # the row stride: q | k | v | gate | mix | padding, kept even
        w = self.nq3 + (self.I if self.gate else 0) + (self.Hkv if self.mix != 'off' else 0)
        return w + (w % 2) + 2

    @property
    def id(self):
        s = (f"{'prep_bwd' if self.bwd else 'prep'}-H{self.H}kv{self.Hkv}dh{self.dh}-rot{self.rot}-"
             f"{'packed' if self.packed else 'padded'}-qkn{self.qk_norm}-xpos{self.xpos:g}-mix_{self.mix}")
        return s + (f'-fl{self.first_layer}acc{self.accumulate}' if self.bwd else '')


def prep_xpos(k, packed):
    """xPos off for every third case, else base 16 on the padded form (n = 7) and base 512 on the packed one
    (n = 500): the factor ((j + 0.4 rot) / (1.4 rot)) ^ ((pos - n // 2) / base) then stays within 0.5 .. 1.9 and a
    rotated pair O(1), as the element-wise bound takes it to be.  (Base 16 at n = 500 spans 3.4e-9 .. 3.2e8.)"""
    return 0. if k % 3 == 0 else (512. if packed else 16.)


def _prep_cases():
    out, i = [], 0
    for (H, Hkv, dh) in PREP_GEOM:
        for rot in (dh // 2, dh, 2 * dh):
            for packed in (0, 1):
                for qkn in (0, 1):
                    out.append(PrepCase(H, Hkv, dh, rot, packed, qkn, prep_xpos(i, packed), PREP_MIX[(i // 3 + i) % 3]))
                    i += 1
    return out


def _prep_bwd_cases():
    out, i = [], 0
    for (H, Hkv, dh) in PREP_GEOM:
        for rot in (dh // 2, dh, 2 * dh):
            for packed in (0, 1):
                for qkn in (0, 1):
                    fl, acc, mix = PREP_BWD_MODES[i % 5]
                    m = ('gate', 'nogate')[(i // 5) % 2] if mix else 'off'
                    out.append(PrepCase(H, Hkv, dh, rot, packed, qkn, prep_xpos(i // 2, packed), m, fl, acc, 1))
                    i += 1
    return out


PREP_CASES = _prep_cases()
PREP_BWD_CASES = _prep_bwd_cases()


def prep_rows(c: PrepCase):
    """Packed form: 9 rows of 2 episodes of 500 steps, positions 0 and 499 among them."""
    pos = torch.tensor([0, 1, 250, 498, 499, 0, 3, 251, 499])
    ep = torch.tensor([0, 0, 0, 0, 0, 1, 1, 1, 1])
    return (ep * c.n + pos).to(torch.int32), pos


def prep_positions(c: PrepCase):
    return prep_rows(c)[1] if c.packed else torch.arange(c.T) % c.n


def prep_inputs(c: PrepCase):
    T, I, Ikv, dh = c.T, c.I, c.Ikv, c.dh
    g = _gen(30, c.H, c.Hkv, dh, c.rot, c.packed, c.qk_norm, c.bwd)
    row = torch.randn(T, c.n_qkv, generator=g)
    w = c.nq3 + (I if c.gate else 0) + (c.Hkv if c.mix != 'off' else 0)
    row[:, w:] = BIG
    if c.qk_norm:                       # one all-zero head of q and one of k
        row[T // 2, dh * (c.H - 1):dh * c.H] = 0.
        row[T - 1, I:I + dh] = 0.
    if c.mix != 'off':                  # pre-activations on both sides of the lerp switch (sigmoid = 0.5 at 0)
        k = torch.arange(T * c.Hkv).reshape(T, c.Hkv)
        row[:, c.mix_col:c.mix_col + c.Hkv] = torch.tensor(MIX_PRE)[k % len(MIX_PRE)]
    ldv = c.nq3 + 4
    vfirst = torch.full((T, ldv), BIG)
    vfirst[:, I + Ikv:c.nq3] = torch.randn(T, Ikv, generator=g)
    inv_freq = (1.0 / (10000. ** (torch.arange(0, c.rot, 2).float() / c.rot))).float()
    B = dict(proj=row, vfirst=vfirst, inv_freq=inv_freq)
    if c.packed:
        B['rows'] = prep_rows(c)[0]
    return B, g


def rotary_tables(c: PrepCase, dt):
    """cos, sin [T][dh / 2] and the xPos factor [T][dh / 2] (1 where off) of the rotated pairs; pairs at or past
    rot_dim / 2 are not rotated (cos 1, sin 0).  The angle is the fp32 product pos * inv_freq and the xPos
    exponent the fp32 quotient (pos - n // 2) / base, as x-transformers forms them, widened to `dt`."""
    pos = prep_positions(c)
    hp = c.dh // 2
    inv = (1.0 / (10000. ** (torch.arange(0, c.rot, 2).float() / c.rot))).float()
    npair = min(hp, c.rot // 2)
    ang = (pos.float()[:, None] * inv[None, :npair]).to(dt)
    cos, sin = torch.ones(len(pos), hp, dtype=dt), torch.zeros(len(pos), hp, dtype=dt)
    cos[:, :npair], sin[:, :npair] = ang.cos(), ang.sin()
    xf = torch.ones(len(pos), hp, dtype=dt)
    if c.xpos > 0.:
        j = torch.arange(0, 2 * npair, 2).to(dt)
        sc = (j + 0.4 * c.rot) / (1.4 * c.rot)
        power = ((pos - c.n // 2).float() / torch.tensor(c.xpos)).to(dt)
        xf[:, :npair] = sc[None, :] ** power[:, None]
    return cos, sin, xf


def head_norms(x, dh):
    """x [T][H dh] -> the heads' l2 norms [T][H]."""
    return x.reshape(x.shape[0], -1, dh).norm(dim=-1)


def prep_forward(c: PrepCase, proj, vfirst, dt):
    """qkv [T][nq3] of the forward in `dt` (proj, vfirst: the buffers of prep_inputs)."""
    T, I, Ikv, dh = c.T, c.I, c.Ikv, c.dh
    cos, sin, xf = rotary_tables(c, dt)
    out = []
    for seg, (c0, w) in enumerate(((0, I), (I, Ikv))):
        x = proj[:, c0:c0 + w].to(dt).reshape(T, -1, dh)
        if c.qk_norm:   # F.normalize: x / max(||x||, 1e-12)
            x = x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
        x = x.reshape(T, -1, dh // 2, 2)
        a, b_ = x[..., 0], x[..., 1]
        s = (xf if seg == 0 else 1.0 / xf)[:, None, :]
        ya = (a * cos[:, None] - b_ * sin[:, None]) * s
        yb = (b_ * cos[:, None] + a * sin[:, None]) * s
        out.append(torch.stack([ya, yb], -1).reshape(T, w))
    v = proj[:, I + Ikv:c.nq3].to(dt)
    if c.mix != 'off':
        m = torch.sigmoid(proj[:, c.mix_col:c.mix_col + c.Hkv].to(dt)).repeat_interleave(dh, 1)
        vf = vfirst[:, I + Ikv:c.nq3].to(dt)
        v = v + m * (vf - v)
    out.append(v)
    return torch.cat(out, 1)


def prep_spec(c: PrepCase):
    B, _ = prep_inputs(c)
    B['qkv'] = nan_out(c.T, c.nq3)

    def expect(dt):
        r = prep_forward(c, B['proj'], B['vfirst'], dt)
        return [Region('qkv', r, fwd_bound(r.double()))]
    return Spec(c.id, 'QKV_PREP', B, ('qkv',), in_=('proj', 'vfirst' if c.mix != 'off' else None, 'inv_freq',
                                                   'rows' if c.packed else None), out=('qkv',),
                ld=(c.n_qkv, c.nq3 + 4), n=(c.T, c.n, c.b, c.H, c.Hkv, c.dh, c.rot, c.mix_col, c.qk_norm),
                f=(c.xpos,), expect=expect)


def prep_backward(c: PrepCase, proj, vfirst, gq3, dvf_old, dt):
    """Closed form of the backward: (d q | d k | d v [T][nq3], dvfirst [T][Ikv] or None, d mix [T][Hkv] or None,
    zero-head mask [T][nq3]) from the gradient gq3 w.r.t. the forward's output."""
    T, I, Ikv, dh = c.T, c.I, c.Ikv, c.dh
    cos, sin, xf = rotary_tables(c, dt)
    out, zero = [], []
    for seg, (c0, w) in enumerate(((0, I), (I, Ikv))):
        gy = gq3[:, c0:c0 + w].to(dt).reshape(T, -1, dh // 2, 2)
        s = (xf if seg == 0 else 1.0 / xf)[:, None, :]
        g0, g1 = gy[..., 0] * s, gy[..., 1] * s
        ga = g0 * cos[:, None] + g1 * sin[:, None]
        gb = g1 * cos[:, None] - g0 * sin[:, None]
        gx = torch.stack([ga, gb], -1).reshape(T, -1, dh)
        z = torch.zeros(T, w // dh, dtype=torch.bool)
        if c.qk_norm:   # x^ = x / ||x||: dx = (g - x^ (x^ . g)) / ||x||; below the clamp of F.normalize dx = g / 1e-12
            x = proj[:, c0:c0 + w].to(dt).reshape(T, -1, dh)
            r = x.norm(dim=-1, keepdim=True)
            nrm = r.clamp_min(1e-12)
            xh = x / nrm
            z = (r < 1e-12).squeeze(-1)
            gx = torch.where(r >= 1e-12, (gx - xh * (xh * gx).sum(-1, keepdim=True)) / nrm, gx / nrm)
        out.append(gx.reshape(T, w))
        zero.append(z.repeat_interleave(dh, 1))
    gv = gq3[:, I + Ikv:].to(dt)
    old = dvf_old.to(dt)
    dvf = dmix = None
    if c.mix != 'off':
        m = torch.sigmoid(proj[:, c.mix_col:c.mix_col + c.Hkv].to(dt))
        me = m.repeat_interleave(dh, 1)
        v, vf = proj[:, I + Ikv:c.nq3].to(dt), vfirst[:, I + Ikv:c.nq3].to(dt)
        dmix = (gv * (vf - v)).reshape(T, -1, dh).sum(-1) * m * (1 - m)
        dvf = gv * me + (old if c.accumulate else 0.)
        gv = gv * (1 - me)
    elif c.first_layer and c.accumulate:
        gv = gv + old
    out.append(gv)
    zero.append(torch.zeros(T, Ikv, dtype=torch.bool))
    return torch.cat(out, 1), dvf, dmix, torch.cat(zero, 1)


def prep_bwd_spec(c: PrepCase):
    B, g = prep_inputs(c)
    T = c.T
    dproj = torch.randn(T, c.n_qkv, generator=g)       # gate and mix columns: values the kernel must keep / replace
    w = c.nq3 + (c.I if c.gate else 0) + (c.Hkv if c.mix != 'off' else 0)
    dproj[:, w:] = BIG
    if c.qk_norm:   # the all-zero heads: the odd channel of each gradient pair is zero, so the inverse rotation adds
        # nothing to nothing (a cancelling g0 cos + g1 sin has no relative accuracy for the relative-only bound to hold)
        dproj[T // 2, c.dh * (c.H - 1) + 1:c.dh * c.H:2] = 0.
        dproj[T - 1, c.I + 1:c.I + c.dh:2] = 0.
    gq3 = dproj[:, :c.nq3].clone()
    dvf_old = torch.randn(T, c.Ikv, generator=g)
    B['dproj'], B['dvfirst'] = guarded(dproj), guarded(dvf_old)

    def expect(dt):
        d3, dvf, dmix, zero = prep_backward(c, B['proj'], B['vfirst'], gq3, dvf_old, dt)
        bound = fwd_bound(d3.double())
        bound[zero] = 1e-5 * d3.double().abs()[zero]   # the 1 / 1e-12 gradient of an all-zero head: relative only
        mix_on = c.mix != 'off'
        if not mix_on and not (c.first_layer and c.accumulate):   # d v is not touched: the input bits stay
            R = [Region('dproj', d3[:, :c.I + c.Ikv], bound[:, :c.I + c.Ikv])]
        else:
            R = [Region('dproj', d3, bound)]
        if mix_on:
            R += [Region('dvfirst', dvf, fwd_bound(dvf.double())),
                  Region('dproj', dmix, fwd_bound(dmix.double()), c0=c.mix_col)]
        return R
    return Spec(c.id, 'QKV_PREP_BWD', B, ('dproj', 'dvfirst'),
                in_=('proj', 'vfirst' if c.mix != 'off' else None, 'inv_freq', 'rows' if c.packed else None),
                out=('dproj', 'dvfirst'), ld=(c.n_qkv, c.nq3 + 4),
                n=(c.T, c.n, c.b, c.H, c.Hkv, c.dh, c.rot, c.mix_col, c.qk_norm, c.first_layer, c.accumulate),
                f=(c.xpos,), expect=expect, info=dict(gq3=gq3, dvf_old=dvf_old))


# ----------------------------------------------------------------------------------------------
# 4. column sums and their deferred queue
# ----------------------------------------------------------------------------------------------

CS_COLS, CS_G, MAX_JOBS = 16, 64, 16
COLSUM_CASES = ([(r, c, w) for r in (1, 15, 17, 4112) for c in (1, 16, 17, 300) for w in (0, 1)]
                + [(16400, c, w) for c in (1, 16, 17) for w in (0, 1)])


def colsum_chunks(rows):
    """(chunks, chunk_rows) of colsum (train.hip): 16-row partials, at most 1024 of them."""
    chunks = min(1024, max(1, rows // 16))
    chunk_rows = -(-rows // chunks)
    return -(-rows // chunk_rows), chunk_rows


def colsum_spec(rows, cols, weighted):
    g = _gen(40, rows, cols, weighted)
    src = torch.randn(rows, cols, generator=g)
    old = torch.randn(cols, generator=g)
    B = dict(src=padded(src, cols + 3), dst=vec_out(old))
    if weighted:
        B['rw'] = padded(torch.randn(rows, 1, generator=g), 3)
    pf = colsum_chunks(rows)[0] * cols
    B['part'] = torch.full((1, pf + 4), NAN)

    def expect(dt):
        t = src.to(dt)
        if weighted:
            t = t * (B['rw'][:, :1].to(dt) * 0.5)
        o = old.to(dt)
        return [sum_region('dst', o + seqsum(t), o.abs() + t.abs().sum(0), 'colsum'),
                Region('part', None, None, shape=(1, pf))]
    return Spec(f'colsum-r{rows}-c{cols}-w{weighted}', 'COLSUM', B, ('dst', 'part'),
                in_=('src', 'rw' if weighted else None), out=('dst',), ld=(cols + 3, 3 if weighted else 0),
                n=(rows, cols), f=(0.5,), part='part', part_floats=pf, expect=expect)


# (name, [(chunks, cols)], workspace floats): one flush; the 17th job forces a flush; the third job forces one
QUEUE_CASES = [('one_flush', [(1, 4), (5, 300), (300, 17)], 1 << 16),
               ('slots_full', [(3, 5 + j) for j in range(17)], 1 << 16),
               ('space_full', [(1, 4), (5, 300), (300, 17)], 300 * 17)]


def queue_flushes(jobs, cap):
    """The launches of ColsumQueue over `jobs` (take_or_flush, then the final flush), restated: a list of the job
    index lists each k_colsum_final_multi launch finishes."""
    launches, cur, used = [], [], 0
    for j, (chunks, cols) in enumerate(jobs):
        need = chunks * cols
        if len(cur) == MAX_JOBS or used + need > cap:
            assert cur, 'a job larger than the workspace'
            launches.append(cur)
            cur, used = [], 0
        assert used + need <= cap
        cur.append(j)
        used += round4(need)
    if cur:
        launches.append(cur)
    return launches


def queue_spec(name, jobs, cap):
    g = _gen(41, len(jobs), cap)
    B = dict(ws=torch.full((1, cap + 4), NAN))
    outs, J, parts, olds = ['ws'], [], [], []
    off = 0
    total = sum(c for _, c in jobs)
    for j, (chunks, cols) in enumerate(jobs):
        B[f'p{j}'] = torch.randn(chunks, cols, generator=g)
        olds.append(torch.randn(cols, generator=g))
        J.append((f'p{j}', ('dst', off), chunks, cols))
        off += cols
    B['dst'] = vec_out(torch.cat(olds))   # the jobs' destinations side by side, guard after the last
    assert off == total

    def expect(dt):
        R, o = [Region('ws', None, None, shape=(1, cap))], 0
        for j, (chunks, cols) in enumerate(jobs):
            p, old = B[f'p{j}'].to(dt), olds[j].to(dt)
            R.append(sum_region('dst', old + seqsum(p), old.abs() + p.abs().sum(0), 'colsum', c0=o))
            o += cols
        return R
    return Spec(f'colsum_queue-{name}', 'COLSUM_QUEUE', B, ('ws', 'dst'), part='ws', part_floats=cap, jobs=tuple(J),
                expect=expect, info=dict(jobs=jobs, olds=olds))


def colsum_final_spec(part, old):
    """k_colsum_final alone on the partials `part` [chunks][cols] (the queue's bit-exact reference)."""
    chunks, cols = part.shape
    B = dict(part=part.clone(), dst=vec_out(old))
    return Spec(f'colsum_final-{chunks}x{cols}', 'COLSUM_FINAL', B, ('dst',), in_=('part',), out=('dst',),
                n=(chunks, cols), expect=lambda dt: [])


# ----------------------------------------------------------------------------------------------
# 5. action-embedding gradient, gene gradients
# ----------------------------------------------------------------------------------------------

EMBED_GRAD_CASES = ([(A, d, T, prev, 0) for A in (1, 4, 5, 8, 9, 32) for d in (48, 260) for T in (1, 37, 300)
                     for prev in (0, 1)]
                    + [(5, 48, 300, 1, 1), (32, 260, 300, 0, 1)])   # the workspace, not T / 16, caps the chunk count


def embed_grad_chunks(T, A, d, part_floats):
    """(chunks, chunk_rows, MAXA) of Backward::embed_grad."""
    chunks = min(min(1024, max(1, T // 16)), max(1, part_floats // (A * d)))
    chunk_rows = -(-T // chunks)
    return -(-T // chunk_rows), chunk_rows, 4 if A <= 4 else 8 if A <= 8 else 32


def embed_grad_spec(A, d, T, prev, capped):
    g = _gen(50, A, d, T, prev, capped)
    g1, g2 = torch.randn(T, d, generator=g), torch.randn(T, d, generator=g)
    pa = torch.randint(-1, A, (T,), generator=g, dtype=torch.int32)
    na = torch.randint(-1, A, (T,), generator=g, dtype=torch.int32)
    na[0] = -1
    old = torch.randn(A, d, generator=g)
    pf = 5 * A * d if capped else max(1, T // 16) * A * d
    B = dict(g2=padded(g2, 2 * d + 4), next=na, dst=vec_out(old), part=torch.full((1, pf + 4), NAN))
    if prev:
        B.update(g1=padded(g1, d + 4), prev=pa)

    def expect(dt):
        oh = lambda a: (a.long()[:, None] == torch.arange(A)[None, :]).to(dt)   # noqa: E731  [T][A]; -1: no row
        # terms in row order: row r adds g1[r] to prev[r]'s row, then g2[r] to next[r]'s
        t = oh(na)[:, :, None] * g2.to(dt)[:, None, :]
        mag = t.abs().sum(0)
        if prev:
            tp = oh(pa)[:, :, None] * g1.to(dt)[:, None, :]
            t = torch.stack([tp, t], 1).reshape(2 * T, A, d)
            mag = mag + tp.abs().sum(0)
        o = old.to(dt)
        return [sum_region('dst', (o + seqsum(t)).reshape(1, -1), (o.abs() + mag).reshape(1, -1), 'embed_grad'),
                Region('part', None, None, shape=(1, pf))]
    return Spec(f'embed_grad-A{A}-d{d}-T{T}-prev{prev}-cap{capped}', 'EMBED_GRAD', B, ('dst', 'part'),
                in_=('g1' if prev else None, 'prev' if prev else None, 'g2', 'next'), out=('dst',),
                ld=(d + 4 if prev else 0, 2 * d + 4), n=(T, d, A), part='part', part_floats=pf, expect=expect)


LATENT_GRAD_CASES = ([(b, n, d, G, 0) for b in (1, 3, 9) for n in (1, 7, 17, 130) for d in (48, 100) for G in (1, 5)]
                     + [(b, n, d, 5 if (b + n) % 2 else 1, 1) for b in (3, 9) for n in (7, 17, 130) for d in (48, 100)])


def latent_ep_off(b, n):
    """Packed episodes: lengths n, 0 (one empty episode), then 1 .. n cycling."""
    lens = [n, 0] + [1 + (7 * e) % n for e in range(b - 2)]
    return torch.tensor([0] + lens).cumsum(0).to(torch.int32)


def latent_grad_spec(b, n, d, G, packed):
    g = _gen(51, b, n, d, G, packed)
    ep = latent_ep_off(b, n) if packed else torch.arange(b + 1, dtype=torch.int32) * n
    T = int(ep[-1])
    ld, off = 3 * d + 4, 2 * d
    dac = torch.full((T, ld), BIG)
    dac[:, off:off + d] = torch.randn(T, d, generator=g)
    latent = torch.randn(b, G, generator=g)
    old_w, old_b = torch.randn(d, G, generator=g), torch.randn(d, generator=g)
    pf = b * d
    B = dict(dac=dac, latent=latent, dw=vec_out(old_w), db=vec_out(old_b), part=torch.full((1, pf + 4), NAN))
    if packed:
        B['ep_off'] = ep

    def expect(dt):
        x = dac[:, off:off + d].to(dt)
        z = torch.zeros(1, d, dtype=dt)
        seg = [x[int(ep[e]):int(ep[e + 1])] for e in range(b)]
        dlat = torch.stack([seqsum(torch.cat([z, s])) for s in seg])            # [b][d]
        mag = torch.stack([s.abs().sum(0) for s in seg])
        lt = latent.to(dt)
        dw = old_w.to(dt) + seqsum(dlat[:, :, None] * lt[:, None, :])
        dbv = old_b.to(dt) + seqsum(dlat)
        return [sum_region('part', dlat.reshape(1, -1), mag.reshape(1, -1), 'latent'),
                sum_region('dw', dw.reshape(1, -1),
                           (old_w.to(dt).abs() + (mag[:, :, None] * lt.abs()[:, None, :]).sum(0)).reshape(1, -1), 'latent'),
                sum_region('db', dbv.reshape(1, -1), (old_b.to(dt).abs() + mag.sum(0)).reshape(1, -1), 'latent')]
    return Spec(f'latent_grad-b{b}-n{n}-d{d}-G{G}-pk{packed}', 'LATENT_GRAD', B, ('part', 'dw', 'db'),
                in_=('dac', 'ep_off' if packed else None, 'latent'), out=('dw', 'db'), ld=(ld,), n=(off, b, n, d, G),
                part='part', part_floats=pf, expect=expect)


# ----------------------------------------------------------------------------------------------
# 6. the valid-row list, gather, scatter
# ----------------------------------------------------------------------------------------------

VALID_BN = [(1, 1), (3, 17), (5, 300)]


def valid_lens(b, n, k):
    """lens holding 0, n, a value above n and a negative one where b allows (k: the pattern)."""
    if b == 1:
        return torch.tensor([[1], [0], [5]][k % 3], dtype=torch.int32)
    base = [n, 0, n + 4, -3, max(1, n // 2)]
    return torch.tensor([base[(e + k) % 5] for e in range(b)], dtype=torch.int32)


def valid_reference(lens, b, n, Tv):
    """(vrows [Tv], vinv [b n], ep_off [b + 1]) of k_valid_rows' documented contract: lens clamped to [0, n];
    the valid rows e n + t in order; entries at or past Tv are not listed and scatter as padding (-1); list slots
    past the true count read row 0."""
    cl = lens.clamp(0, n).tolist()
    vrows = torch.zeros(Tv, dtype=torch.int32)
    vinv = torch.full((b * n,), -1, dtype=torch.int32)
    j, off = 0, [0]
    for e in range(b):
        for t in range(cl[e]):
            if j < Tv:
                vrows[j] = e * n + t
                vinv[e * n + t] = j
            j += 1
        off.append(min(j, Tv))
    return vrows, vinv, torch.tensor(off, dtype=torch.int32)


def _valid_cases():
    out = []
    for (b, n) in VALID_BN:
        for k in range(3 if b == 1 else 2):
            count = int(valid_lens(b, n, k).clamp(0, n).sum())
            for dTv in (0, -3, 2):
                Tv = count + dTv
                if 0 <= Tv <= b * n:
                    out.append((b, n, k, Tv, (k + dTv) % 2))
    return out


VALID_CASES = _valid_cases()   # (b, n, lens pattern, Tv, ep_off given)


def valid_rows_spec(b, n, k, Tv, ep):
    lens = valid_lens(b, n, k)
    B = dict(lens=lens, vrows=torch.full((1, Tv + 4), ISENT, dtype=torch.int32),
             vinv=torch.full((1, b * n + 4), ISENT, dtype=torch.int32))
    if ep:
        B['ep_off'] = torch.full((1, b + 1 + 4), ISENT, dtype=torch.int32)

    def expect(dt):
        vr, vi, eo = valid_reference(lens, b, n, Tv)
        R = [Region('vinv', vi.reshape(1, -1), None)]
        if Tv:
            R.append(Region('vrows', vr.reshape(1, -1), None))
        if ep:
            R.append(Region('ep_off', eo.reshape(1, -1), None))
        return R
    return Spec(f'valid_rows-b{b}-n{n}-k{k}-Tv{Tv}-ep{ep}', 'VALID_ROWS', B,
                ('vrows', 'vinv') + (('ep_off',) if ep else ()), in_=('lens',),
                out=('vrows', 'vinv', 'ep_off' if ep else None), n=(b, n, Tv), expect=expect)


# (cols, offset of the source pointer in floats): <4> needs cols, strides and both pointers on the float4 grid
MOVE_FORMS = [(8, 0), (8, 1), (6, 0)]
MOVE_CASES = [(b, n, cols, o) for (b, n) in VALID_BN[1:] for (cols, o) in MOVE_FORMS]


def move_is_vec4(cols, lds, ldd, src_off):
    return cols % 4 == 0 and lds % 4 == 0 and ldd % 4 == 0 and src_off % 4 == 0


def move_spec(kind, b, n, cols, src_off):
    """gather: dst[i] = src[vrows[i]]; scatter: dst[r] = vinv[r] >= 0 ? src[vinv[r]] : 0.  The row lists are the
    reference lists of the (b, n) valid-row case with Tv three below the count (overflow rows scatter as padding)."""
    lens = valid_lens(b, n, 0)
    count = int(lens.clamp(0, n).sum())
    Tv = count - 3
    vrows, vinv, _ = valid_reference(lens, b, n, Tv)
    g = _gen(60, b, n, cols, src_off, kind == 'gather')
    lds = ldd = cols + 4
    src_rows, idx, out_rows = (b * n, vrows, Tv) if kind == 'gather' else (Tv, vinv, b * n)
    flat = torch.full((src_rows * lds + 4,), BIG)
    body = flat[src_off:src_off + src_rows * lds].view(src_rows, lds)
    body[:, :cols] = torch.randn(src_rows, cols, generator=g)
    B = dict(src=flat.reshape(1, -1), idx=idx, dst=nan_out(out_rows, ldd))

    def expect(dt):
        data = body[:, :cols]
        if kind == 'gather':
            ref = data[idx.long()]
        else:
            ref = torch.where((idx >= 0)[:, None], data[idx.clamp_min(0).long()], torch.zeros(()))
        return [Region('dst', ref, None)]
    return Spec(f'{kind}-b{b}-n{n}-c{cols}-off{src_off}', kind.upper(), B, ('dst',), in_=(('src', src_off), 'idx'),
                out=('dst',), ld=(lds, ldd), n=(out_rows if kind == 'scatter' else Tv, cols), expect=expect,
                info=dict(vec4=move_is_vec4(cols, lds, ldd, src_off)))


# ----------------------------------------------------------------------------------------------
# 7. the fractal step's row kernels
# ----------------------------------------------------------------------------------------------

CM_G = 16
CAUSAL_CASES = [(n, d, rev, add) for n in (1, 15, 17, 130) for d in (48, 100) for rev in (0, 1) for add in (0, 1)
                if rev or not add]


def causal_mean_spec(n, d, rev, add, b=2):
    g = _gen(70, n, d, rev, add)
    T = b * n
    src = torch.randn(T, d, generator=g)
    B = dict(src=padded(src, d + 4), dst=nan_out(T, d + 12))
    if add:
        B['add'] = padded(torch.randn(T, d, generator=g), d + 8)

    def expect(dt):
        x = src.to(dt).reshape(b, n, d)
        cnt = torch.arange(1, n + 1).to(dt)[None, :, None]
        if not rev:        # dst[e, t] = sum_{s <= t} src[e, s] / (t + 1)
            ref = x.cumsum(1) / cnt
            mag = x.abs().cumsum(1) / cnt
        else:              # dst[e, s] = add[e, s] + sum_{t >= s} src[e, t] / (t + 1)
            y = x / cnt
            ref = y.flip(1).cumsum(1).flip(1)
            mag = y.abs().flip(1).cumsum(1).flip(1)
            if add:
                a = B['add'][:, :d].to(dt).reshape(b, n, d)
                ref, mag = ref + a, mag + a.abs()
        return [sum_region('dst', ref.reshape(T, d), mag.reshape(T, d), 'causal_mean')]
    return Spec(f'causal_mean-n{n}-d{d}-rev{rev}-add{add}', 'CAUSAL_MEAN', B, ('dst',),
                in_=('src', 'add' if add else None), out=('dst',), ld=(d + 4, d + 8 if add else 0, d + 12),
                n=(b, n, d, rev), expect=expect)


def action_rows_spec(rows=37, d=48, A=5):
    g = _gen(71, rows, d, A)
    act = torch.randint(0, A, (rows,), generator=g, dtype=torch.int32)
    act[0], act[3], act[rows - 1], act[7] = -1, A, A + 4, A - 1   # SafeEmbedding: out of range on either side -> 0
    W = torch.randn(A, d, generator=g)
    B = dict(act=act, W=W, out=nan_out(rows, 2 * d))

    def expect(dt):
        ok = (act >= 0) & (act < A)
        return [Region('out', torch.where(ok[:, None], W[act.clamp(0, A - 1).long()], torch.zeros(())), None, c0=d)]
    # (as the step calls it: the destination is the ewa row's second half)
    return Spec('action_rows', 'ACTION_ROWS', B, ('out',), in_=('act', 'W'), out=(('out', d),), ld=(2 * d,), n=(rows, d, A),
                expect=expect)


AXPB_CASES = [(0, 0), (1, 1), (1, 0)]   # (a has rows (else lda = 0: one row broadcast), b given)


def rows_axpb_spec(a_rows, has_b, rows=37, cols=50):
    g = _gen(72, a_rows, has_b)
    a = torch.randn(rows if a_rows else 1, cols, generator=g)
    B = dict(a=padded(a, cols + 4), dst=nan_out(rows, cols + 8))
    if has_b:
        B['b'] = padded(torch.randn(rows, cols, generator=g), cols + 6)

    def expect(dt):
        r = 0.5 * a.to(dt).expand(rows, cols)
        if has_b:
            r = r + B['b'][:, :cols].to(dt)
        return [Region('dst', r, fwd_bound(r.double()))]
    return Spec(f'rows_axpb-a{a_rows}-b{has_b}', 'AXPB', B, ('dst',), in_=('a', 'b' if has_b else None), out=('dst',),
                ld=(cols + 4 if a_rows else 0, cols + 6 if has_b else 0, cols + 8), n=(rows, cols), f=(0.5,),
                expect=expect)


def rows_bcast_spec(b=3, n=15, d=48):
    g = _gen(73, b, n, d)
    src = torch.randn(b, d, generator=g)
    B = dict(src=src, dst=nan_out(b * n, 3 * d + 4))
    # (as the step calls it: the destination is the ac_in row's third d-column block)
    return Spec('rows_bcast_ep', 'BCAST_EP', B, ('dst',), in_=('src',), out=(('dst', 2 * d),), ld=(3 * d + 4,),
                n=(b * n, n, d),
                expect=lambda dt: [Region('dst', src[torch.arange(b * n) // n], None, c0=2 * d)])


def all_specs():
    """Every case of every table (the queue's bit-exact twin launches aside), for the tests that sweep them all."""
    for c in EMBED_CASES:
        yield embed_spec(c)
    for a in LATENT_EMBED_CASES:
        yield latent_embed_spec(*a)
    for a in LN_FWD_CASES:
        yield ln_fwd_spec(*a)
    for a in LN_BWD_CASES:
        yield ln_bwd_spec(*a)
    for c in PREP_CASES:
        yield prep_spec(c)
    for c in PREP_BWD_CASES:
        yield prep_bwd_spec(c)
    for a in COLSUM_CASES:
        yield colsum_spec(*a)
    for a in QUEUE_CASES:
        yield queue_spec(*a)
    for a in EMBED_GRAD_CASES:
        yield embed_grad_spec(*a)
    for a in LATENT_GRAD_CASES:
        yield latent_grad_spec(*a)
    for a in VALID_CASES:
        yield valid_rows_spec(*a)
    for a in MOVE_CASES:
        yield move_spec('gather', *a)
        yield move_spec('scatter', *a)
    for a in CAUSAL_CASES:
        yield causal_mean_spec(*a)
    yield action_rows_spec()
    for a in AXPB_CASES:
        yield rows_axpb_spec(*a)
    yield rows_bcast_spec()
