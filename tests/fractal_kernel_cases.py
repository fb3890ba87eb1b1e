"""Seeded inputs, case tables and fp64 references for the kernels of the fractal encoder's forward:
the bidirectional / token-major attention forward (xtrl_attn_fwd_tokens), the row kernels of
csrc/fractal.hip (rows_add, add_layernorm, seq_mean, safe_embed, wm_post) and the forms of
xtrl_gemm_f32 that only the fractal forward uses.

Imported by test_fractal_kernels_cpu.py (which settles the references against the oracle's own
functions and the case tables against the edges they are there for, without a GPU) and by
test_fractal_kernels_gpu.py (which runs the kernels).  Everything here is plain PyTorch on the CPU
and defines no tests.  Inputs are fp32; a reference widens them to fp64 first.  The padding columns
of an input whose row stride is wider than its data hold NaN: a kernel that reads them shows."""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch

from oracle import ref_port as R

NAN = float('nan')


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def padded(t, ld, fill=NAN):
    """[M][ld] with t [M][D] in its first D columns and ``fill`` in the rest."""
    M, D = t.shape
    out = torch.full((M, ld), fill, dtype=t.dtype)
    out[:, :D] = t
    return out


# ----------------------------------------------------------------------------------------------
# 1. attention forward on token-major operands
# ----------------------------------------------------------------------------------------------


@dataclass(frozen=True)
class AttnCase:
    """q, k, v: the column slices [0, I), [I, 2I), [2I, 3I) (I = H dh) of one [b n][ld] buffer, ld = 3 I + pad;
    o [b n][I + pad]."""
    b: int
    H: int
    n: int
    dh: int
    lens: tuple
    pad: int = 0
    causal: bool = False

    @property
    def I(self):   # noqa: E743
        return self.H * self.dh

    @property
    def ld(self):
        return 3 * self.I + self.pad

    @property
    def ldo(self):
        return self.I + self.pad


ATTN_CASES = [
    AttnCase(2, 2, 1, 16, (1, 1)),            # the rollout shape: one key, o = v
    AttnCase(3, 2, 64, 16, (64, 1, 37)),      # one full tile
    AttnCase(3, 2, 65, 16, (65, 64, 1)),      # a second key tile of one key; one skipped at len = 64; a second query tile of one row
    AttnCase(3, 3, 130, 32, (130, 65, 128)),  # three key tiles; odd H
    AttnCase(2, 2, 130, 64, (130, 63)),       # three key tiles at dh = 64
    AttnCase(2, 4, 70, 16, (70, 5), pad=4),   # padded rows: ld = 3 H dh + 4, ldo = H dh + 4
]
ATTN_CAUSAL_CASE = AttnCase(2, 2, 130, 16, (130, 40), causal=True)
TK = 64   # the key / query tile of k_attn_fwd


def attn_id(c):
    return f'b{c.b}_H{c.H}_n{c.n}_dh{c.dh}_pad{c.pad}' + ('_causal' if c.causal else '')


def attn_inputs(c):
    """buf [b n][ld] fp32 (padding NaN) and lens int32 [b]."""
    g = _gen(1, c.b, c.H, c.n, c.dh, c.pad)
    buf = padded(torch.randn(c.b * c.n, 3 * c.I, generator=g), c.ld)
    return buf, torch.tensor(c.lens, dtype=torch.int32)


def attn_heads(c, buf):
    """q, k, v [b][H][n][dh] views of the buffer's column slices."""
    I = c.I   # noqa: E741
    return tuple(buf[:, j * I:(j + 1) * I].reshape(c.b, c.n, c.H, c.dh).transpose(1, 2) for j in range(3))


def attn_ref(q, k, v, lens, scale, causal=False):
    """fp64 dense softmax of q, k, v [b][H][n][dh] with the key-padding mask j < lens[b] (and j <= i when
    ``causal``), lens >= 1.  Every row is computed, the padded ones i >= len too: they attend the len valid keys.
    Returns o [b][H][n][dh] and lse [b][H][n]."""
    assert int(lens.min()) >= 1
    n = q.shape[2]
    q, k, v = q.double(), k.double(), v.double()
    s = torch.einsum('bhid,bhjd->bhij', q, k) * scale
    j = torch.arange(n)
    mask = (j[None, :] < lens.long()[:, None])[:, None, None, :].expand(-1, 1, n, -1)
    if causal:
        mask = mask & (j[None, :] <= j[:, None])[None, None]
    s = s.masked_fill(~mask, -math.inf)
    return torch.einsum('bhij,bhjd->bhid', s.softmax(-1), v), s.logsumexp(-1)


def attn_reference(c):
    buf, lens = attn_inputs(c)
    q, k, v = attn_heads(c, buf)
    return attn_ref(q, k, v, lens, c.dh ** -0.5, c.causal)


def tokens_of(o):
    """[b][H][n][dh] -> token-major [b n][H dh]."""
    b, H, n, dh = o.shape
    return o.transpose(1, 2).reshape(b * n, H * dh)


# ----------------------------------------------------------------------------------------------
# 2. row kernels
# ----------------------------------------------------------------------------------------------

ROWS_ADD_CASES = [(1, 48), (5, 64), (7, 65), (4, 256)]   # (M, D); ldx = D + 3, ldy = D + 5


def rows_add_inputs(M, D):
    g = _gen(2, M, D)
    return torch.randn(M, D, generator=g), torch.randn(D, generator=g)


def rows_add_ref(x, v, M):
    """The fp32 sum itself, [M][D] (x None: v on every row)."""
    return x + v if x is not None else v[None].repeat(M, 1)


@dataclass(frozen=True)
class LNCase:
    """``r``: 'given' (one residual row per row, r_rep = 1), 'rep' (r_rep rows share one residual row;
    ceil(M / r_rep) rows), None (NULL).  ``kind``: 'randn', 'offset' (rows drawn as N(16, 1): a one-pass
    E[x^2] - mean^2 variance is 1.6e-4 from fp64 there, a two-pass one 2e-6) or 'const' (row 2 is constant:
    variance 0, the output is beta)."""
    M: int
    D: int
    r: str = 'given'
    r_rep: int = 1
    beta: bool = True
    eps: float = 1e-5
    kind: str = 'randn'


LN_MAX_D = 1024
LN_CASES = [
    LNCase(1, 48), LNCase(5, 64, eps=1e-3), LNCase(9, 65), LNCase(5, 256), LNCase(1, 1000, eps=1e-3), LNCase(9, 1000),
    LNCase(5, 1024), LNCase(1, 1024, eps=1e-3),
    LNCase(9, 65, r='rep', r_rep=3), LNCase(7, 1000, r='rep', r_rep=3), LNCase(7, 48, r='rep', r_rep=3, eps=1e-3),
    LNCase(5, 48, r=None), LNCase(1, 1024, r=None), LNCase(9, 256, r=None, eps=1e-3),
    LNCase(5, 65, beta=False), LNCase(9, 256, r=None, beta=False), LNCase(5, 1024, r='rep', r_rep=3, beta=False),
    LNCase(5, 1024, r=None, kind='offset'),
    LNCase(5, 65, r=None, kind='const'),
]
LN_CONST_ROW, LN_CONST = 2, 0.75   # (65 x 0.75 and its quotient by 65 are exact in fp32)


def ln_id(c):
    return f'M{c.M}_D{c.D}_r{c.r}{c.r_rep}_{"beta" if c.beta else "nobeta"}_eps{c.eps:g}_{c.kind}'


def ln_inputs(c):
    """x [M][D], r [ceil(M / r_rep)][D] or None, gamma [D], beta [D] or None."""
    g = _gen(3, c.M, c.D, c.r_rep, c.beta, c.kind == 'offset')
    x = torch.randn(c.M, c.D, generator=g)
    if c.kind == 'offset':
        x = x + 16.
    elif c.kind == 'const':
        x[LN_CONST_ROW] = LN_CONST
    r = torch.randn(-(-c.M // c.r_rep), c.D, generator=g) if c.r else None
    gamma = torch.rand(c.D, generator=g) + 0.5
    beta = torch.randn(c.D, generator=g) if c.beta else None
    return x, r, gamma, beta


def ln_ref(x, r, r_rep, gamma, beta, eps):
    """fp64 LayerNorm (biased variance, eps inside the root) of the fp32-rounded sum x + r[m // r_rep]."""
    s = x if r is None else x + r[torch.arange(x.shape[0]) // r_rep]
    assert s.dtype == torch.float32
    s = s.double()
    mean = s.mean(-1, keepdim=True)
    var = ((s - mean) ** 2).mean(-1, keepdim=True)
    y = (s - mean) / (var + eps).sqrt() * gamma.double()
    return y if beta is None else y + beta.double()


def ln_reference(c):
    x, r, gamma, beta = ln_inputs(c)
    return ln_ref(x, r, c.r_rep, gamma, beta, c.eps)


SEQ_MEAN_CASES = [(1, 1, 48), (3, 23, 300), (2, 70, 257)]   # (B, n, D); y a column slice, ldy = 2 D + 4


def seq_mean_inputs(B, n, D):
    return torch.randn(B * n, D, generator=_gen(4, B, n, D))


def seq_mean_ref(x, B, n):
    """fp64 mean over the n rows of each sequence, and the bound of a sequential fp32 sum and its division:
    n 2^-24 mean_i |x_i| per element."""
    xd = x.double().reshape(B, n, -1)
    return xd.mean(1), n * 2.0 ** -24 * xd.abs().mean(1)


SAFE_EMBED_ACTIONS = (-1, 0, 4, 2, -1, 4, 1)   # M = 7 rows over a table of A = 5 rows: the last row twice
SAFE_EMBED_A = 5
SAFE_EMBED_DS = [48, 65]


def safe_embed_inputs(D):
    return torch.randn(SAFE_EMBED_A, D, generator=_gen(5, D)), torch.tensor(SAFE_EMBED_ACTIONS, dtype=torch.int32)


def safe_embed_ref(table, actions):
    """The table row, or 0 for a negative action (no arithmetic: exact in any precision)."""
    out = torch.zeros(len(actions), table.shape[1], dtype=table.dtype)
    for m, a in enumerate(actions.tolist()):
        if a >= 0:
            out[m] = table[a]
    return out


WM_POST_CASES = [(1, 1), (5, 9), (300, 3)]   # (M, P); ldr = 2 P + 2
WM_LOGVAR_EDGES = (0., 30., -30., 100., -100.)
WM_DONE_EDGES = (0., 88., -88., 104., -104.)
WM_DONE_MODES = ('ldd1', 'ldd3', 'none')


def wm_post_inputs(M, P):
    """raw [M][2 P] interleaved (mean, log-variance) with the log-variances at scale 4 and done logits [M] at
    scale 6; the edge values go to the first elements (as many as fit)."""
    g = _gen(6, M, P)
    raw = torch.randn(M, P, 2, generator=g)
    raw[..., 1] *= 4.
    lv = raw[..., 1].reshape(-1)
    k = min(len(WM_LOGVAR_EDGES), M * P)
    lv[:k] = torch.tensor(WM_LOGVAR_EDGES[:k])
    raw[..., 1] = lv.reshape(M, P)
    logit = torch.randn(M, generator=g) * 6.
    k = min(len(WM_DONE_EDGES), M)
    logit[:k] = torch.tensor(WM_DONE_EDGES[:k])
    return raw.reshape(M, 2 * P), logit


def wm_post_ref(raw, logit):
    """The oracle's Continuous.mean_variance (ref_port.continuous_params) and sigmoid in fp64:
    mean_var [2][M][P], done [M]."""
    mean, var = R.continuous_params(raw.double())
    return torch.stack((mean, var)), torch.sigmoid(logit.double())


# ----------------------------------------------------------------------------------------------
# 3. GEMM forms of the fractal forward
# ----------------------------------------------------------------------------------------------

GEMM_SHAPES = [(1, 5, 8), (37, 100, 96), (130, 257, 48)]   # (M, N, K)
GEMM_FORMS = ('relu', 'gelu', 'out_slice', 'bias_residual_alias', 'x_slice')
GEMM_X_PAD, GEMM_X_FILL = 4, 1e30


def gemm_inputs(M, N, K):
    """x [M][K], w [N][K] (scaled by K^-1/2), bias [N], residual [M][N]."""
    g = _gen(7, M, N, K)
    return (torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g),
            torch.randn(M, N, generator=g))


def gemm_ref(form, x, w, bias, res):
    y = x.double() @ w.double().T + bias.double()
    if form == 'relu':
        return torch.relu(y)
    if form == 'gelu':
        return torch.nn.functional.gelu(y)
    if form == 'bias_residual_alias':
        return y + res.double()
    assert form in ('out_slice', 'x_slice'), form
    return y
