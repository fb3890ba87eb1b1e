"""Seeded inputs, case tables, the dispatch restatement and fp64 references for the epilogues of the fp32 GEMM
(csrc/gemm.hip through xtrl_gemm_epi), and for the four direct entries beside it that no test called
(xtrl_gemm_ex with bias and beta, xtrl_linear_gelu_drop, xtrl_glu_drop_fwd / _bwd, xtrl_layernorm_f32).

Imported by test_gemm_epi_cpu.py (which settles every closed form against torch.autograd, the case tables against
the (combination, path, epilogue form) pairs gemm_run can reach, and the bounds against a plain fp32 restatement,
without a GPU) and by test_gemm_epi_gpu.py (which runs the kernels).  Plain PyTorch on the CPU; defines no tests.
Inputs are fp32, a reference widens them to fp64 first.

Layout of every case.  An output has a row stride wider than its data and guard rows past M (a partial buffer one
guard row past its last row tile), all NaN before the call: owned elements must come back finite and inside their
bound, everything else still NaN bit for bit.  The padding columns of A and B past K hold 1e30
(test_gemm_ragged_extent_padded_rows): a kernel that lets them into a product shows.

Bounds (none is taken from the kernels):
  forward values  C, aux_out, ln_y1, ln_y2, the mean of ln_stats: an O(1) function of an O(1) pre-activation
      (weights scaled 1 / sqrt K as in test_gemm_f32), held to that test's |x - ref| <= 1e-5 + 1e-5 |ref|; rstd to a
      relative 1e-5.
  bare products   7 x 2^-24 x sum_k |a b|  (test_gemm_large_tile_split_bf16_accuracy).
  LayerNorm-backward rows  the gradient is linear in the GEMM output with coefficients of size rstd[m], so the
      absolute part scales with the row: 1e-5 max(1, rstd[m]) + 1e-5 |ref|.  The chained second LayerNorm takes
      the first one's output, error included, through coefficients of size rstd2[m]:
      1e-5 max(1, rstd[m]) max(1, rstd2[m]) + 1e-5 |ref|.
  partial sums    ln_part[t][n] = sum over the rows of tile t of g x^:  PART_C x 2^-24 x sum_rows |g| |x^| for the
      sum itself (the style of fractal_kernel_cases.seq_mean_ref) plus the error g carries in,
      sum_rows |x^| x 7 x 2^-24 x |gscale| sum_k |dy w|; ln_part_b the same with x^ = 1; the chained pair the same
      with g = C and the row bound of C as the carried error.  Where g = gscale v + ln_gpre, |g| stands for
      |gscale v| + |ln_gpre|: the add rounds at the size of its operands, which a cancelling sum does not show.

Measured (test_gemm_epi_cpu.py::test_fp32_restatement_within_a_quarter_of_each_bound prints them, pytest -s: the
formulas below evaluated in plain fp32 torch on the CPU against fp64, worst over every case of the tables):
  forward values            C 0.18 of the bound, aux_out 0.11; RES_LN: C 0.18, ln_y1 0.19, ln_y2 0.19, mean 0.015,
                            rstd 0.022
  LayerNorm-backward rows   0.18 of the bound (EPI_LN_BWD), 0.14 (EPI_LN_BWD2), 0.14 (the chained output)
  partial sums, the GEMM output given exactly (fp64 product rounded to fp32): 3.42 x 2^-24 x sum |g| |x^|
  -> PART_C = 14 (4 x 3.42, rounded up: a wave tree against a sequential sum, the MFMA accumulation order); with
     it those sums sit at 0.14 of their bound or less, the chained pair's at 0.06.
  partial sums with the fp32 product too: 0.29 of the bound.  That share of the bound is the project's product
     figure, 7 x 2^-24 sum |a b|, of which the BLAS's summation alone takes up to 2.5 and the native fp32 MFMA path
     3 - 5 (test_gemm_large_tile_split_bf16_accuracy); the ratio does not move with the inputs' scale, so the
     quarter rule is held on the sums with the product given exactly, and the full restatement inside the bound.
  Two input families were rescaled to stay inside a quarter (the bounds were not touched): A of the K = 512 shape
  is drawn at half scale (a 512-deep fp32 product reached 0.25 of the forward bound at unit scale), and the gains
  of the RES_LN cases lie in [0.5, 1] (the N(16, 1) row reached 0.27 with gains up to 1.5).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from functools import lru_cache

import torch

NAN = float('nan')
BIG = 1e30
EPS24 = 2.0 ** -24
PART_C = 14.0

EPI = dict(NONE=0, GELU=1, SILU=2, GELU_DROP=3, SILU_SAVE=4, MUL_AUX=5, DGATE=7, RELU=8, RES_LN=9, LN_BWD=10,
           MASK_POS=11, LN_BWD2=12)
EPI_NAME = {v: k for k, v in EPI.items()}
LN_EPIS = (EPI['RES_LN'], EPI['LN_BWD'], EPI['LN_BWD2'])
AUX_IN_EPIS = (EPI['MUL_AUX'], EPI['DGATE'], EPI['MASK_POS'])
AUX_OUT_EPIS = (EPI['GELU_DROP'], EPI['SILU_SAVE'], EPI['DGATE'])

# (trans_a, trans_b, epi, LN prologue, residual): the instantiations of gemm_run's table
COMBOS = [
    (0, 0, EPI['NONE'], False, False), (0, 0, EPI['NONE'], False, True), (0, 0, EPI['NONE'], True, False),
    (0, 0, EPI['GELU'], True, False), (0, 0, EPI['GELU'], False, False), (0, 0, EPI['SILU'], False, False),
    (0, 0, EPI['RELU'], False, False), (0, 0, EPI['GELU_DROP'], False, False), (0, 0, EPI['SILU_SAVE'], False, False),
    (0, 1, EPI['NONE'], False, False), (0, 1, EPI['NONE'], False, True), (0, 1, EPI['MASK_POS'], False, False),
    (0, 1, EPI['MUL_AUX'], False, False), (0, 1, EPI['DGATE'], False, False),
    (1, 1, EPI['NONE'], False, False),
]


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def round4(x):
    return (x + 3) & ~3


def bits(t):
    return t.contiguous().view(torch.int32)


def padded(t, fill):
    """t [R][D] in the first D columns of [R][round4(D) + 4], `fill` in the rest."""
    out = torch.full((t.shape[0], round4(t.shape[1]) + 4), fill, dtype=t.dtype)
    out[:, :t.shape[1]] = t
    return out


# ----------------------------------------------------------------------------------------------
# 1. the dispatch, restated (gemm_run, dispatch_geom, ws_ok, ln_gemm_run; split-bf16 products on, no images)
# ----------------------------------------------------------------------------------------------

PATHS = ('scalar64', 'tall_wk2', 'x6_128', 'ws128', 'tile64', 'small_wk2', 'wk4')


def operands_vec(M, N, K, ta, tb, lda, ldb):
    """gemm_run's `vec` for 16-byte aligned bases: float4 staging of both operands."""
    return (lda % 4 == 0 and ldb % 4 == 0 and lda >= round4(M if ta else K) and ldb >= round4(N if tb else K))


def ws_ok(M, N, K, ta, ln):
    if ln or not (K % 32 == 0 or ta):
        return False
    wgs = ((N + 127) // 128) * ((M + 127) // 128)
    return wgs <= 256 and K >= (64 if ta else 512)


def expected_path(M, N, K, trans_a, trans_b, epi, ln, vec):
    """The geometry path of dispatch_geom (one of PATHS; 'tile64' is the 64 x 64 tile in either product form), or
    'ln128' / 'ln256' for the LayerNorm epilogues.  vec: gemm_run's vec_k (EwCase.vec)."""
    if epi in LN_EPIS:
        return 'ln128' if N <= 128 else 'ln256'
    tiles128 = ((M + 127) // 128) * ((N + 127) // 128)
    tiles64 = ((M + 63) // 64) * ((N + 63) // 64)
    if not vec:
        return 'scalar64'
    if not trans_a and N <= 32 and M >= 4096:
        return 'tall_wk2'
    if tiles128 >= 192 and K > 64:
        if epi != EPI['DGATE'] and not ln and ws_ok(M, N, K, trans_a, ln) and K % 32 == 0:
            return 'ws128'
        return 'x6_128'
    if tiles64 >= 256 and K <= 512:
        return 'tile64'
    return 'small_wk2' if K <= 256 else 'wk4'


def _b(x):
    return 'true' if x else 'false'


def expected_kernel(M, N, K, trans_a, trans_b, epi, ln, vec, res):
    """The kernel instantiation as a profiler prints it, up to its last non-defaulted template argument."""
    path = expected_path(M, N, K, trans_a, trans_b, epi, ln, vec)
    ta, tb = _b(trans_a), _b(trans_b)
    if path in ('ln128', 'ln256'):
        kt = K % 32 != 0 or epi != EPI['RES_LN']   # the backward epilogues always take the masked-tail kernel
        tile = '128, 128' if path == 'ln128' else '64, 256'
        return f'k_gemm_ws<false, {tb}, {epi}, {_b(res)}, {tile}, {_b(kt)}'
    if path == 'ws128':
        return f'k_gemm_ws<{ta}, {tb}, {epi}, {_b(res)}, 128, 128, false'
    x6 = path == 'x6_128' or (path == 'tile64' and not trans_a and not trans_b and epi != EPI['DGATE'])
    geom = {'scalar64': '2, 2, 1, 1, 1', 'tall_wk2': '2, 1, 2, 1, 1', 'x6_128': '2, 2, 1, 2, 2',
            'tile64': '2, 2, 1, 1, 1', 'small_wk2': '2, 1, 2, 1, 1', 'wk4': '1, 1, 4, 1, 1'}[path]
    return f'k_gemm<{geom}, {ta}, {tb}, {epi}, {_b(ln)}, {_b(res)}, {_b(vec)}, {_b(x6)}>'


def gemm_ln_rows(N):
    return 128 if N <= 128 else 64


# ----------------------------------------------------------------------------------------------
# 2. element-wise epilogues: one shape per path, every extent ragged against its tile
# ----------------------------------------------------------------------------------------------

# path -> (M, N of the row-vector form, K); the scalar form runs N - 1 columns of the same operands
# (scalar64: N + 1, the table's 37), which keeps the path and leaves a column quad cut short
PATH_SHAPE = {
    'scalar64': (70, 36, 31),       # lda = 33: operands not float4
    'tall_wk2': (4100, 20, 40),     # N <= 32, M >= 4096, A "N"
    'x6_128': (3080, 1000, 72),     # 25 x 8 = 200 tiles >= 192; last row tile 8 rows, last column tile 104
    'ws128': (3080, 1000, 512),     # 200 workgroups <= 256, K >= 512, K % 32 == 0
    'tile64': (1030, 1000, 72),     # 72 tiles of 128, 272 of 64
    'small_wk2': (70, 100, 72),     # K <= 256
    'wk4': (70, 100, 260),          # K > 256
}
BETAS = (0., 1., -0.5)
DROP_PS = (0., 0.1, 0.25)           # none, word mode, byte mode (64 / 256)
DROP_SEED, DROP_OFFSET, DROP_LAYER = 0x1234567887654321, 77, 3


@dataclass(frozen=True)
class EwCase:
    combo: tuple
    path: str
    form: str          # 'v4': the row-vector epilogue; 'scalar': the scalar one
    M: int
    N: int
    K: int
    beta: float
    bias: bool
    bias_col0: int
    act_cols: int      # 0: every column
    p: float
    ln_rms: int

    @property
    def ta(self):
        return self.combo[0]

    @property
    def tb(self):
        return self.combo[1]

    @property
    def epi(self):
        return self.combo[2]

    @property
    def ln(self):
        return self.combo[3]

    @property
    def res(self):
        return self.combo[4]

    @property
    def nfull(self):   # columns of the shared operands
        return PATH_SHAPE[self.path][1] + (1 if self.path == 'scalar64' else 0)

    @property
    def lda(self):
        if self.path == 'scalar64':
            return (self.M if self.ta else self.K) + 2            # 33 for A "N": odd
        return round4(self.M if self.ta else self.K) + 4

    @property
    def ldb(self):
        if self.path == 'scalar64':
            return (self.nfull if self.tb else self.K) + 2
        return round4(self.nfull if self.tb else self.K) + 4

    @property
    def ldo(self):     # row stride of C, R, the aux operands: a multiple of 4 only in the row-vector form
        return self.N + 4 if self.form == 'v4' else self.N + 4 + (1 if (self.N + 4) % 2 == 0 else 0)

    @property
    def epi_v4(self):  # epi_v4_ok (16-byte aligned bases)
        return self.N % 4 == 0 and self.ldo % 4 == 0

    @property
    def vec(self):     # gemm_run's vec_k: GELU + dropout has no scalar epilogue on the float4 kernels
        v = operands_vec(self.M, self.N, self.K, self.ta, self.tb, self.lda, self.ldb)
        return v and (self.epi != EPI['GELU_DROP'] or self.epi_v4)

    @property
    def id(self):
        ta, tb, epi, ln, res = self.combo
        return (f"{'T' if ta else 'N'}{'T' if tb else 'N'}-{EPI_NAME[epi]}{'-ln' if ln else ''}{'-res' if res else ''}"
                f'-{self.path}-{self.form}')


def _ew_cases():
    out = []
    i = 0
    for combo in COMBOS:
        ta, tb, epi, ln, res = combo
        for path in PATHS:
            M, N, K = PATH_SHAPE[path]
            for form in ('v4', 'scalar'):
                n = N if form == 'v4' else (N + 1 if path == 'scalar64' else N - 1)
                has_bias = tb == 0                       # the forward layouts; the dgrad / wgrad callers pass none
                c = EwCase(combo, path, form, M, n, K, BETAS[i % 3], has_bias,
                           3 if (has_bias and path in ('scalar64', 'small_wk2', 'ws128')) else 0,
                           (n - 4 if form == 'v4' else n - 1) if epi == EPI['SILU_SAVE'] else 0,
                           DROP_PS[i % 3] if epi == EPI['GELU_DROP'] else 0., 1 if (ln and form == 'scalar') else 0)
                i += 1
                # keep a case only where the table's shape lands on the path it is there for (a path this
                # combination cannot take — tall_wk2 for A "T", ws128 for the gate or the LN prologue, the scalar
                # epilogue of GELU + dropout on a float4 kernel — drops out here, not by a list kept by hand)
                if expected_path(c.M, c.N, c.K, ta, tb, epi, ln, c.vec) == path and c.epi_v4 == (form == 'v4'):
                    out.append(c)
    return out


# (ordered by path and layout: consecutive cases share their cached operands and fp64 product)
EW_CASES = sorted(_ew_cases(), key=lambda c: (PATHS.index(c.path), c.ta, c.tb, c.ln, c.ln_rms))


@lru_cache(maxsize=4)
def _ew_operands(path, ta, tb):
    """A, B in their storage layouts (padding 1e30), shared by every case of one path and layout."""
    M, _, K = PATH_SHAPE[path]
    probe = EwCase((ta, tb, 0, False, False), path, 'v4', M, PATH_SHAPE[path][1], K, 0., False, 0, 0, 0., 0)
    N, lda, ldb = probe.nfull, probe.lda, probe.ldb
    g = _gen(1, M, N, K, ta, tb)
    a = torch.randn(M, K, generator=g)
    if K >= 512:   # (rescaled: at unit scale the fp32 restatement of a 512-deep product passes a quarter of the bound)
        a *= 0.5
    b = torch.randn(K, N, generator=g) / math.sqrt(K)          # B[k][n]
    A = torch.full((K, lda) if ta else (M, lda), BIG)
    if ta:
        A[:, :M] = a.t()
    else:
        A[:, :K] = a
    B = torch.full((K, ldb) if tb else (N, ldb), BIG)
    if tb:
        B[:, :N] = b
    else:
        B[:, :K] = b.t()
    gamma = torch.rand(K, generator=g) + 0.5
    return a, b, A, B, gamma


def ln_rows(x, rms, eps=1e-5):
    """(normalised rows, mean, rstd) of x-transformers' LayerNorm (no affine) or RMSNorm, in x's precision."""
    n = x.shape[-1]
    if rms:
        mean = torch.zeros_like(x[..., :1])
        rstd = math.sqrt(n) / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    else:
        mean = x.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    return (x - mean) * rstd, mean.squeeze(-1), rstd.squeeze(-1)


@lru_cache(maxsize=4)
def _ew_product(path, ta, tb, ln, rms, dtype):
    a, b, _, _, gamma = _ew_operands(path, ta, tb)
    a, b = a.to(dtype), b.to(dtype)
    if ln:
        a = ln_rows(a, rms)[0] * gamma.to(dtype)
    return a @ b


def ew_inputs(c: EwCase):
    """The CPU tensors of one case: A, B (storage layouts), gamma, bias, R, C0 (the prefill: NaN where beta = 0),
    aux_in, aux_in2; outputs are [M + 2][ldo]."""
    _, _, A, B, gamma = _ew_operands(c.path, c.ta, c.tb)
    g = _gen(2, c.M, c.N, c.K, c.epi, c.form == 'v4')
    rows, ld = c.M + 2, c.ldo
    d = dict(A=A, B=B, gamma=gamma if c.ln else None)
    d['bias'] = torch.randn(c.N - c.bias_col0, generator=g) if c.bias else None
    d['R'] = torch.randn(c.M, ld, generator=g) if c.res else None
    c0 = torch.full((rows, ld), NAN)
    if c.beta != 0.:
        c0[:c.M, :c.N] = torch.randn(c.M, c.N, generator=g)
    d['C0'] = c0
    if c.epi in AUX_IN_EPIS:
        aux = torch.randn(c.M, ld, generator=g)
        if c.epi == EPI['MASK_POS']:   # exact zeros of both signs: neither is positive
            flat = aux.view(-1)
            flat[::7] = 0.0
            flat[3::11] = -0.0
        d['aux_in'] = aux
    else:
        d['aux_in'] = None
    d['aux_in2'] = torch.randn(c.M, ld, generator=g) if c.epi == EPI['DGATE'] else None
    return d


def gelu_and_deriv(v):
    """torch's GELU (erf form) and its derivative Phi(v) + v phi(v), in v's precision."""
    cdf = 0.5 * (1.0 + torch.erf(v / math.sqrt(2.0)))
    return v * cdf, cdf + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


def silu_and_deriv(v):
    s = torch.sigmoid(v)
    return v * s, s * (1.0 + v * (1.0 - s))


def epilogue_ref(epi, v, *, keep=None, p=0., act_cols=0, aux_in=None, aux_in2=None):
    """(C before residual / beta, aux_out or None) of an element-wise epilogue at pre-activation v [M][N]."""
    N = v.shape[1]
    aux = None
    if epi == EPI['GELU']:
        v = gelu_and_deriv(v)[0]
    elif epi == EPI['SILU']:
        v = silu_and_deriv(v)[0]
    elif epi == EPI['RELU']:
        v = v.clamp_min(0.)
    elif epi == EPI['GELU_DROP']:
        v, aux = gelu_and_deriv(v)
        if p > 0.:
            k = keep.to(v.dtype) / (1.0 - p)
            v, aux = v * k, aux * k
    elif epi == EPI['SILU_SAVE']:
        act = torch.arange(N) < (act_cols if act_cols > 0 else N)
        s, ds = silu_and_deriv(v)
        v, aux = torch.where(act, s, v), torch.where(act, ds, torch.ones_like(v))
    elif epi == EPI['MUL_AUX']:
        v = v * aux_in
    elif epi == EPI['MASK_POS']:
        v = torch.where(aux_in > 0, v, torch.zeros_like(v))
    elif epi == EPI['DGATE']:
        s = torch.sigmoid(aux_in2)
        v, aux = v * s, v * aux_in * s * (1.0 - s)
    return v, aux


def ew_reference(c: EwCase, d, keep=None, dtype=torch.float64):
    """(C, aux_out) [M][N] of one case in `dtype` (fp64: the reference; fp32: the restatement)."""
    cv = lambda t: None if t is None else t[:c.M, :c.N].to(dtype)   # noqa: E731
    v = _ew_product(c.path, c.ta, c.tb, c.ln, c.ln_rms, dtype)[:, :c.N].clone()
    if c.bias:
        v[:, c.bias_col0:] += d['bias'].to(dtype)
    v, aux = epilogue_ref(c.epi, v, keep=keep, p=c.p, act_cols=c.act_cols, aux_in=cv(d['aux_in']),
                          aux_in2=cv(d['aux_in2']))
    if c.res:
        v = v + cv(d['R'])
    if c.beta != 0.:
        v = c.beta * cv(d['C0']) + v
    return v, aux


def fwd_bound(ref):
    """The project's forward bound, tol(x, ref, 1e-5, 1e-5), per element."""
    return 1e-5 + 1e-5 * ref.abs()


def dot_scale(a, b):
    return a.abs() @ b.abs()


# ----------------------------------------------------------------------------------------------
# 3. LayerNorm epilogues
# ----------------------------------------------------------------------------------------------

LN_NARROW = [(N, M) for N in (128, 64, 36) for M in (1, 128, 130)]   # 128-row tiles, N <= 128
LN_WIDE = [(N, M) for N in (256, 200, 132) for M in (1, 64, 70)]     # 64 x 256 tiles
LN_NM = LN_NARROW + LN_WIDE
LN_KS = (32, 36, 96, 260)   # one slab; a slab and a tail; an odd slab count; nine slabs and a tail
LN_VARIANTS = {
    # bias / ln_b / ln_y2 (ln_ld2 = N + 8) / ln_b2; the all-zero row needs no bias; ln_ld1 = N + 4 throughout
    EPI['RES_LN']: {'bias': dict(bias=True, ln_b=False, y2=False, b2=False, zero_row=False),
                    'beta_y2': dict(bias=False, ln_b=True, y2=True, b2=True, zero_row=True),
                    'all': dict(bias=True, ln_b=True, y2=True, b2=False, zero_row=False)},
    EPI['LN_BWD']: {'none': dict(dres='none'), 'sep': dict(dres='sep'), 'alias': dict(dres='alias')},
    # chain: only without ln_rms (the chained LayerNorm is always the mean form; train.hip calls ln_rms = 1 alone)
    EPI['LN_BWD2']: {'bare': dict(gpre=None, gscale=1., part_b=False, pstride=False, chain=False),
                     'side': dict(gpre=0, gscale=0.5, part_b=True, pstride=True, chain=True),
                     'ldg2': dict(gpre=2, gscale=1., part_b=True, pstride=False, chain=True)},
}


@dataclass(frozen=True)
class LnCase:
    epi: int
    N: int
    M: int
    K: int
    rms: int
    variant: str

    @property
    def opt(self):
        o = dict(LN_VARIANTS[self.epi][self.variant])
        if self.epi == EPI['LN_BWD2'] and self.rms:
            o['chain'] = False
        return o

    @property
    def tb(self):
        return 0 if self.epi == EPI['RES_LN'] else 1

    @property
    def tiles(self):
        return -(-self.M // gemm_ln_rows(self.N))

    @property
    def id(self):
        return f'{EPI_NAME[self.epi]}-N{self.N}-M{self.M}-K{self.K}-rms{self.rms}-{self.variant}'


def ln_cases(epi, N, M):
    return [LnCase(epi, N, M, K, rms, v) for K in LN_KS for rms in (0, 1) for v in LN_VARIANTS[epi]]


LN_CASES = [c for epi in LN_EPIS for (N, M) in LN_NM for c in ln_cases(epi, N, M)]


def _stats32(x, rms):
    """(mean, rstd) of the rows of x as the fp32 pair a forward stored: what the backward kernels read."""
    _, mean, rstd = ln_rows(x.double(), rms)
    return torch.stack([mean, rstd], 1).float()


def ln_inputs(c: LnCase):
    """CPU tensors of one LayerNorm-epilogue case.  A [M][K + 4], B in its layout, both padded with 1e30."""
    M, N, K, o = c.M, c.N, c.K, c.opt
    g = _gen(3, c.epi, N, M, K, c.rms, sorted(LN_VARIANTS[c.epi]).index(c.variant))
    a = torch.randn(M, K, generator=g)
    b = torch.randn(K, N, generator=g) / math.sqrt(K)
    d = dict(opt=o)
    d['ln_g'] = torch.rand(N, generator=g) + 0.5
    if c.epi == EPI['RES_LN']:
        # (rescaled to [0.5, 1]: with gains up to 1.5 the fp32 restatement of the N(16, 1) row passes a quarter of
        # the bound: x - mean rounds at the size of x, 16)
        d['ln_g'] = d['ln_g'] * 0.5 + 0.25
        r = torch.randn(M, N, generator=g)
        big = 0
        if o['zero_row']:            # the padded-token row: A row zero, no bias, R row zero
            a[M - 1] = 0.
            r[M - 1] = 0.
            big = 0 if M > 1 else None
        if big is not None:          # one row drawn N(16, 1): through the residual, its GEMM part zero
            a[big] = 0.
            r[big] = 16. + torch.randn(N, generator=g)
        d['R'] = torch.full((M, N + 4), NAN)
        d['R'][:, :N] = r
        d['bias'] = torch.randn(N, generator=g) if o['bias'] else None
        d['ln_b'] = torch.randn(N, generator=g) if o['ln_b'] else None
        d['ln_b2'] = torch.randn(N, generator=g) if o['b2'] else None
    else:
        x = torch.randn(M, N, generator=g) * 1.5 + 0.3
        d['ln_x'] = x
        d['ln_stats'] = _stats32(x, c.rms)
        if c.epi == EPI['LN_BWD']:
            d['ln_dres'] = torch.randn(M, N, generator=g) if o['dres'] != 'none' else None
        else:
            if o['gpre'] is None:
                d['ln_gpre'] = None
            else:
                ldg = N if o['gpre'] == 0 else 2 * N
                d['ln_gpre'] = torch.full((M, ldg), NAN)
                d['ln_gpre'][:, :N] = torch.randn(M, N, generator=g)
            if o['chain']:
                x2 = torch.randn(M, N, generator=g) * 0.7 - 0.2
                d['ln2_x'], d['ln2_stats'] = x2, _stats32(x2, 0)
                d['ln2_g'] = torch.rand(N, generator=g) + 0.5
    A = torch.full((M, K + 4), BIG)
    A[:, :K] = a
    if c.tb:
        B = torch.full((K, N + 4), BIG)
        B[:, :N] = b
    else:
        B = torch.full((N, K + 4), BIG)
        B[:, :K] = b.t()
    d.update(a=a, b=b, A=A, B=B)
    return d


def ln_bwd(g, x, mean, rstd, gamma, rms):
    """(dx, x^) of y = LN(x) gamma given g = dL/dy, in g's precision, from the forward's (mean, rstd):
    dx = rstd (g gamma - mean_n(g gamma) - x^ mean_n(g gamma x^)); RMSNorm has no mean_n(g gamma) term."""
    xh = (x - mean[:, None]) * rstd[:, None]
    gm = g * gamma
    ma = 0. if rms else gm.mean(1, keepdim=True)
    mb = (gm * xh).mean(1, keepdim=True)
    return rstd[:, None] * (gm - ma - xh * mb), xh


def tile_sums(t, rows):
    """[ceil(M / rows)][N]: the sums of t over each row tile."""
    M = t.shape[0]
    return torch.stack([t[i:i + rows].sum(0) for i in range(0, M, rows)])


def ln_reference(c: LnCase, d, dtype=torch.float64, v=None):
    """Outputs of one LayerNorm-epilogue case in `dtype` as a dict, with 'terms' for the partial sums' bounds
    (name -> the summed term).  v: the GEMM output to use (default: a . b in `dtype`)."""
    o, N = c.opt, c.N
    cv = lambda t: None if t is None else t.to(dtype)   # noqa: E731
    if v is None:
        v = d['a'].to(dtype) @ d['b'].to(dtype)
    gam = d['ln_g'].to(dtype)
    out = {}
    if c.epi == EPI['RES_LN']:
        x = v
        if d['bias'] is not None:
            x = x + cv(d['bias'])
        x = x + cv(d['R'][:, :N])
        xh, mean, rstd = ln_rows(x, c.rms)
        y = xh * gam
        if d['ln_b'] is not None:
            y = y + cv(d['ln_b'])
        out.update(C=x, ln_y1=y, mean=mean, rstd=rstd)
        if o['y2']:
            out['ln_y2'] = y + cv(d['ln_b2']) if d['ln_b2'] is not None else y
        return out
    rows = gemm_ln_rows(N)
    st = d['ln_stats'].to(dtype)
    g = gmag = v
    if c.epi == EPI['LN_BWD2']:
        g = g * o['gscale']
        gmag = g.abs()
        if d['ln_gpre'] is not None:
            gmag = gmag + cv(d['ln_gpre'][:, :N]).abs()   # |g| before the add can cancel: what its rounding scales with
            g = g + cv(d['ln_gpre'][:, :N])
    dx, xh = ln_bwd(g, cv(d['ln_x']), st[:, 0], st[:, 1], gam, c.rms)
    terms = {'ln_part': g * xh}
    if c.epi == EPI['LN_BWD']:
        if d['ln_dres'] is not None:
            dx = dx + cv(d['ln_dres'])
    else:
        if o['part_b']:
            terms['ln_part_b'] = g
        if o['chain']:
            st2 = d['ln2_stats'].to(dtype)
            dx2, xh2 = ln_bwd(dx, cv(d['ln2_x']), st2[:, 0], st2[:, 1], cv(d['ln2_g']), 0)
            out['ln2_out'] = dx2
            terms['ln2_part'] = dx * xh2
            terms['ln2_part_b'] = dx
            out['xh2'] = xh2
    out['C'] = dx
    out['xh'] = xh
    out['gmag'] = gmag.abs()
    out['terms'] = terms
    for k, t in terms.items():
        out[k] = tile_sums(t, rows)
    return out


def ln_bounds(c: LnCase, d, ref):
    """Per-element bounds of the outputs of a backward case from its fp64 reference `ref` (module docstring)."""
    o, rows = c.opt, gemm_ln_rows(c.N)
    rs = d['ln_stats'][:, 1].double().clamp_min(1.)[:, None]
    gs = abs(o['gscale']) if c.epi == EPI['LN_BWD2'] else 1.
    gerr = 7 * EPS24 * gs * dot_scale(d['a'].double(), d['b'].double())          # the product's error in g
    bc = 1e-5 * rs + 1e-5 * ref['C'].abs()
    bnd = {'C': bc}
    t = ref['terms']
    bnd['ln_part'] = (PART_C * EPS24 * tile_sums(ref['gmag'] * ref['xh'].abs(), rows)
                      + tile_sums(ref['xh'].abs() * gerr, rows))
    if 'ln_part_b' in t:
        bnd['ln_part_b'] = PART_C * EPS24 * tile_sums(ref['gmag'], rows) + tile_sums(gerr, rows)
    if 'ln2_out' in ref:
        rs2 = d['ln2_stats'][:, 1].double().clamp_min(1.)[:, None]
        bnd['ln2_out'] = 1e-5 * rs * rs2 + 1e-5 * ref['ln2_out'].abs()
        bnd['ln2_part'] = (PART_C * EPS24 * tile_sums(t['ln2_part'].abs(), rows)
                           + tile_sums(ref['xh2'].abs() * bc, rows))
        bnd['ln2_part_b'] = PART_C * EPS24 * tile_sums(t['ln2_part_b'].abs(), rows) + tile_sums(bc, rows)
    return bnd


def ln_fwd_bounds(ref):
    b = {k: fwd_bound(ref[k]) for k in ('C', 'ln_y1', 'ln_y2', 'mean') if k in ref}
    b['rstd'] = 1e-5 * ref['rstd'].abs()
    return b


# ----------------------------------------------------------------------------------------------
# 4. the direct entries: gated feed-forward (xtrl_glu_drop_fwd / _bwd), LayerNorm rows (xtrl_layernorm_f32)
# ----------------------------------------------------------------------------------------------

GLU_CASES = [(7, 37), (70, 100)]   # (M, ff): M ff is no multiple of 256; ldu = 2 ff + 5, ldh = ff + 2, lddu = 2 ff + 3


def glu_inputs(M, ff):
    g = _gen(5, M, ff)
    u = torch.full((M, 2 * ff + 5), NAN)
    u[:, :2 * ff] = torch.randn(M, 2 * ff, generator=g)
    dh = torch.full((M, ff + 2), NAN)
    dh[:, :ff] = torch.randn(M, ff, generator=g)
    return u, dh


def glu_fwd_ref(u, ff, keep, p):
    """h = drop(value gelu(gate)): value = u[:, :ff], gate = u[:, ff : 2 ff] (x-transformers GLU)."""
    a, gate = u[:, :ff], u[:, ff:2 * ff]
    return a * gelu_and_deriv(gate)[0] * keep.to(u.dtype) / (1.0 - p)


def glu_bwd_ref(dh, u, ff, keep, p):
    """du [M][2 ff] of glu_fwd_ref, closed form."""
    a, gate = u[:, :ff], u[:, ff:2 * ff]
    ge, dge = gelu_and_deriv(gate)
    dk = dh * keep.to(u.dtype) / (1.0 - p)
    return torch.cat([dk * ge, dk * a * dge], 1)


LAYERNORM_DS = (4, 48, 256, 320, 512)
LAYERNORM_MS = (1, 70)


def layernorm_inputs(M, D):
    """x [M][D + 4] (padding NaN) with the zero row (last) and the N(16, 1) row (first; M = 1: that row alone)."""
    g = _gen(6, M, D)
    x = torch.randn(M, D, generator=g)
    x[0] = 16. + torch.randn(D, generator=g)
    if M > 1:
        x[M - 1] = 0.
    xp = torch.full((M, D + 4), NAN)
    xp[:, :D] = x
    return xp, torch.rand(D, generator=g) + 0.5
