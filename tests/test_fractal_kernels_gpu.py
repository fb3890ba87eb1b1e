"""MI355X tests of the kernels of the fractal encoder's forward, one kernel at a time through the C ABI
against the fp64 references of fractal_kernel_cases.py (test_fractal_kernels_cpu.py settles those
references and the case tables without a GPU): the bidirectional / token-major attention forward
(xtrl_attn_fwd_tokens, csrc/attn.hip), the row kernels of csrc/fractal.hip and the forms of
xtrl_gemm_f32 (csrc/gemm.hip) that only the fractal forward uses.

Every output buffer holds NaN before the call.  After it every element the kernel owns is finite and
every element it does not own — the padding columns of a row stride wider than the data, the
neighbouring column slices — still holds its NaN.  A refused call leaves every output NaN.  Unless a
test says otherwise the bound is the project's own for forward values, tol(x, ref, 1e-5, 1e-5)
against fp64.

Which test of this file first reaches which kernel or path (the whole-model tests of test_fractal.py
reach the same kernels at their own shapes, behind a bound of 1e-4 of a whole output's largest element):

attention (csrc/attn.hip, k_attn_fwd<DH> with a.causal = 0 through xtrl_attn_fwd_tokens)
  one key, one row (the rollout shape)                        test_attn_tokens_against_fp64[b2_H2_n1_dh16_pad0]
  one full tile; an episode of one key                        test_attn_tokens_against_fp64[b3_H2_n64_dh16_pad0]
  a second key tile of one key, a masked key in it, a second
    key tile skipped (len <= 64 < n), a second query tile     test_attn_tokens_against_fp64[b3_H2_n65_dh16_pad0]
  three key tiles at dh = 32, H = 3                           test_attn_tokens_against_fp64[b3_H3_n130_dh32_pad0]
  three key tiles at dh = 64                                  test_attn_tokens_against_fp64[b2_H2_n130_dh64_pad0]
  row strides other than 3 H dh / H dh                        test_attn_tokens_against_fp64[b2_H4_n70_dh16_pad4]
  causal = 1 through the token-major entry                    test_attn_tokens_causal_is_the_head_major_forward
  the stride check of the entry point                         test_attn_tokens_refuses_unequal_row_strides
row kernels (csrc/fractal.hip)
  k_rows_add (x given / NULL, D off the 64-lane grid)         test_rows_add
  k_add_layernorm: D = 48 .. 1024 (one to sixteen floats
    per lane), r_rep = 3, r / beta NULL, variance 0           test_add_layernorm_against_fp64
  k_seq_mean: the second column block (D > 256), a column
    slice as output                                           test_seq_mean
  k_safe_embed: the last table row, negative actions          test_safe_embed
  k_wm_post: saturated log-variances and done logits, a
    second 256-thread block, ldd = 1 / 3 / no done head       test_wm_post
GEMM (csrc/gemm.hip, xtrl_gemm_f32)
  EPI_RELU; EPI_GELU without the LayerNorm prologue           test_gemm_fractal_forms[relu-*] / [gelu-*]
  out a column slice of a wider buffer                        test_gemm_fractal_forms[out_slice-*]
  bias + residual aliasing out                                test_gemm_fractal_forms[bias_residual_alias-*]
  X a column slice with a wider row stride                    test_gemm_fractal_forms[x_slice-*]"""
import pytest
import torch

import attn_harness as AH
import fractal_kernel_cases as C
import test_gpu_parity as G

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN = float('nan')
tol = G.tol


def nan(*shape):
    return torch.full(shape, NAN, device=DEV)


def owned(t, what):
    assert bool(torch.isfinite(t).all()), f'{what}: an element the kernel owns was not written (NaN left) or is not finite'


def untouched(t, what):
    assert bool(torch.isnan(t).all()), f'{what}: an element the kernel does not own was written'


def call(name, *args):
    """The C ABI function ``name`` on the current stream, synchronised; returns its code (0: OK)."""
    from xtrl_amd import _lib as L
    rc = getattr(L.lib(), name)(*[L.ptr(a) if torch.is_tensor(a) or a is None else a for a in args], L.stream())
    torch.cuda.synchronize()
    return rc


def ok(name, *args):
    from xtrl_amd import _lib as L
    L.check(call(name, *args), name)


# ----------------------------------------------------------------------------------------------
# 1. attention forward on token-major operands
# ----------------------------------------------------------------------------------------------


def run_attn(c, **kw):
    buf, lens = C.attn_inputs(c)
    return AH.attn_tokens_lib(buf.to(DEV), lens.to(DEV), c.b, c.H, c.n, c.dh, c.dh ** -0.5, causal=c.causal, ldo=c.ldo,
                              **kw)


def check_attn(c, res):
    """o (its H dh data columns) and lse written everywhere and within the bound of the fp64 reference — the padded
    rows i >= len too; the padding columns of o untouched."""
    o_ref, lse_ref = C.attn_reference(c)
    o, lse = res['o'], res['lse']
    owned(o[:, :c.I], 'o')
    owned(lse, 'lse')
    untouched(o[:, c.I:], 'o padding')
    err = (o[:, :c.I].double().cpu() - C.tokens_of(o_ref)).abs().max()
    print(C.attn_id(c), 'max |o - ref|', float(err), 'max |lse - ref|', float((lse.double().cpu() - lse_ref).abs().max()))
    tol(o[:, :c.I], C.tokens_of(o_ref), 1e-5, 1e-5)
    tol(lse, lse_ref, 1e-5, 1e-5)
    tol(lse.exp(), lse_ref.exp(), 1e-5, 1e-5)


@pytest.mark.parametrize('case', C.ATTN_CASES, ids=C.attn_id)
def test_attn_tokens_against_fp64(case):
    res = run_attn(case)
    check_attn(case, res)
    if case.n == 1:   # one key: the softmax is 1 and o is v
        buf, _ = C.attn_inputs(case)
        assert torch.equal(res['o'].cpu(), buf[:, 2 * case.I:3 * case.I])


def test_attn_tokens_causal_is_the_head_major_forward():
    """causal = 1 through the token-major entry: within the bound of the fp64 causal reference, and bit-identical
    to xtrl_attn_fwd on [b][H][n][dh] copies of the same data (both are k_attn_fwd<16>, with other strides)."""
    c = C.ATTN_CAUSAL_CASE
    res = run_attn(c)
    check_attn(c, res)
    buf, lens = C.attn_inputs(c)
    q, k, v = (t.contiguous().to(DEV) for t in C.attn_heads(c, buf))
    o, lse = nan(*q.shape), nan(c.b, c.H, c.n)
    ok('xtrl_attn_fwd', q, k, v, lens.to(DEV), o, lse, c.b, c.H, c.n, c.dh, c.dh ** -0.5, 0., 0, 0, 0)
    owned(o, 'xtrl_attn_fwd o')
    assert torch.equal(C.tokens_of(o), res['o']) and torch.equal(lse, res['lse'])


def test_attn_tokens_refuses_unequal_row_strides():
    c = C.ATTN_CASES[5]
    with pytest.raises(RuntimeError, match='share one row stride'):
        run_attn(c, ldk=c.ld + 4)
    res = AH.attn_tokens_lib.last
    untouched(res['o'], 'o')
    untouched(res['lse'], 'lse')


# ----------------------------------------------------------------------------------------------
# 2. row kernels
# ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('with_x', [True, False], ids=['x', 'nox'])
@pytest.mark.parametrize('M,D', C.ROWS_ADD_CASES)
def test_rows_add(M, D, with_x):
    """y = x + v (x NULL: v) with ldx = D + 3, ldy = D + 5: bit-equal to the fp32 sum, the padding untouched."""
    x, v = C.rows_add_inputs(M, D)
    xd = C.padded(x, D + 3).to(DEV) if with_x else None
    y = nan(M, D + 5)
    ok('xtrl_rows_add', xd, D + 3, v.to(DEV), y, D + 5, M, D)
    owned(y[:, :D], 'y')
    untouched(y[:, D:], 'y padding')
    assert torch.equal(y[:, :D].cpu(), C.rows_add_ref(x if with_x else None, v, M))


def test_rows_add_of_no_rows_writes_nothing():
    x, v = C.rows_add_inputs(4, 65)
    y = nan(4, 70)
    ok('xtrl_rows_add', C.padded(x, 68).to(DEV), 68, v.to(DEV), y, 70, 0, 65)
    untouched(y, 'y')


def run_layernorm(c):
    """xtrl_add_layernorm with ldx = D + 1, ldr = D + 2, ldy = D + 3; returns y [M][D + 3]."""
    x, r, gamma, beta = C.ln_inputs(c)
    y = nan(c.M, c.D + 3)
    ok('xtrl_add_layernorm', C.padded(x, c.D + 1).to(DEV), c.D + 1, None if r is None else C.padded(r, c.D + 2).to(DEV),
       c.D + 2, c.r_rep, gamma.to(DEV), None if beta is None else beta.to(DEV), y, c.D + 3, c.M, c.D, c.eps)
    return y


@pytest.mark.parametrize('case', C.LN_CASES, ids=C.ln_id)
def test_add_layernorm_against_fp64(case):
    """y = LayerNorm(x + r[m / r_rep]) gamma + beta against the fp64 LayerNorm of the fp32-rounded sum.  The offset
    case (rows N(16, 1) at D = 1024) holds a one-pass variance apart at this bound; the constant row (variance 0)
    gives beta itself."""
    c = case
    y = run_layernorm(c)
    owned(y[:, :c.D], 'y')
    untouched(y[:, c.D:], 'y padding')
    ref = C.ln_reference(c)
    print(C.ln_id(c), 'max |y - ref|', float((y[:, :c.D].double().cpu() - ref).abs().max()))
    tol(y[:, :c.D], ref, 1e-5, 1e-5)
    if c.kind == 'const':
        beta = C.ln_inputs(c)[3]
        assert torch.equal(y[C.LN_CONST_ROW, :c.D].cpu(), beta)


def test_add_layernorm_refuses_a_row_past_its_registers():
    D = C.LN_MAX_D + 1
    x, g = torch.randn(2, D).to(DEV), torch.ones(D).to(DEV)
    y = nan(2, D)
    assert call('xtrl_add_layernorm', x, D, None, 0, 1, g, None, y, D, 2, D, 1e-5) != 0
    untouched(y, 'y')


@pytest.mark.parametrize('B,n,D', C.SEQ_MEAN_CASES)
def test_seq_mean(B, n, D):
    """y[b] = mean over the n rows of sequence b, written into the right-hand column slice of a [B][2 D + 4] buffer:
    each element within n 2^-24 mean_i |x_i| of fp64 (a sequential fp32 sum and its division); at n = 1 x itself."""
    x = C.seq_mean_inputs(B, n, D)
    ldx, ldy = D + 3, 2 * D + 4
    y = nan(B, ldy)
    ok('xtrl_seq_mean', C.padded(x, ldx).to(DEV), ldx, B, n, D, y[:, D:], ldy)
    owned(y[:, D:2 * D], 'y')
    untouched(y[:, :D], 'the column slice before y')
    untouched(y[:, 2 * D:], 'y padding')
    got = y[:, D:2 * D].cpu()
    if n == 1:
        assert torch.equal(got, x)
        return
    ref, bound = C.seq_mean_ref(x, B, n)
    err = (got.double() - ref).abs()
    print('seq_mean', (B, n, D), 'max err / bound', float((err / bound).max()))
    assert bool((err <= bound).all()), float((err / bound).max())


@pytest.mark.parametrize('D', C.SAFE_EMBED_DS)
def test_safe_embed(D):
    """The table row of each action — the last row among them — or 0 for a negative one, bit-equal, written into
    the right half of a [M][2 D] buffer."""
    table, actions = C.safe_embed_inputs(D)
    M = len(actions)
    y = nan(M, 2 * D)
    ok('xtrl_safe_embed', actions.to(DEV), M, table.to(DEV), D, y[:, D:], 2 * D)
    owned(y[:, D:], 'y')
    untouched(y[:, :D], 'the left half')
    assert torch.equal(y[:, D:].cpu(), C.safe_embed_ref(table, actions))


def run_wm_post(M, P, mode):
    """xtrl_wm_post with ldr = 2 P + 2 and the done head of ``mode``: 'ldd1' / 'ldd3' (done logits at stride 1 / 3)
    or 'none' (both pointers NULL).  Returns mean_var [2][M][P] and done [M] (None without the head)."""
    raw, logit = C.wm_post_inputs(M, P)
    mv = nan(2, M, P)
    ldd = dict(ldd1=1, ldd3=3, none=0)[mode]
    lg = C.padded(logit[:, None], ldd).to(DEV) if ldd else None
    done = nan(M) if ldd else None
    ok('xtrl_wm_post', C.padded(raw, 2 * P + 2).to(DEV), 2 * P + 2, M, P, mv, lg, ldd, done)
    return mv, done


@pytest.mark.parametrize('mode', C.WM_DONE_MODES)
@pytest.mark.parametrize('M,P', C.WM_POST_CASES)
def test_wm_post(M, P, mode):
    """mean bit-equal to the input, variance exp(3 tanh(lv / 3)) and done = sigmoid(logit) within the common bound
    of the oracle's fp64 values, at log-variances 0, +-30, +-100 and done logits 0, +-88, +-104 (the sigmoid at
    -104 is below fp32's range: the absolute part of the bound covers it)."""
    raw, logit = C.wm_post_inputs(M, P)
    ref_mv, ref_done = C.wm_post_ref(raw, logit)
    mv, done = run_wm_post(M, P, mode)
    owned(mv, 'mean_var')
    assert torch.equal(mv[0].cpu(), raw[:, 0::2])
    tol(mv[1], ref_mv[1], 1e-5, 1e-5)
    if mode != 'none':
        owned(done, 'done')
        tol(done, ref_done, 1e-5, 1e-5)


def test_wm_post_refuses_done_without_its_logits():
    M, P = 5, 9
    raw, _ = C.wm_post_inputs(M, P)
    mv, done = nan(2, M, P), nan(M)
    assert call('xtrl_wm_post', C.padded(raw, 2 * P + 2).to(DEV), 2 * P + 2, M, P, mv, None, 1, done) != 0
    untouched(mv, 'mean_var')
    untouched(done, 'done')


# ----------------------------------------------------------------------------------------------
# 3. GEMM forms of the fractal forward
# ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('M,N,K', C.GEMM_SHAPES)
@pytest.mark.parametrize('form', C.GEMM_FORMS)
def test_gemm_fractal_forms(form, M, N, K):
    """xtrl_gemm_f32 as the fractal forward calls it, at test_gemm_f32's bound against fp64: bias + ReLU and bias +
    GELU without a LayerNorm prologue; an output that is the middle of three column slices of a [M][3 N] buffer
    (the neighbours untouched); bias + a residual that aliases the output; X a column slice of a [M][K + 4]
    buffer whose padding holds 1e30."""
    from xtrl_amd import _lib as L, ops
    x, w, b, res = C.gemm_inputs(M, N, K)
    ref = C.gemm_ref(form, x, w, b, res)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    if form == 'out_slice':
        big = nan(M, 3 * N)
        out = ops.gemm(xd, wd, bd, out=big[:, N:2 * N])
        torch.cuda.synchronize()
        untouched(big[:, :N], 'the slice before out')
        untouched(big[:, 2 * N:], 'the slice after out')
    elif form == 'bias_residual_alias':
        r2 = res.to(DEV)
        out = ops.gemm(xd, wd, bd, residual=r2, out=r2)
    elif form == 'x_slice':
        xb = C.padded(x, K + C.GEMM_X_PAD, C.GEMM_X_FILL).to(DEV)
        out = nan(M, N)
        ops.gemm(xb[:, :K], wd, bd, out=out)
    else:
        out = nan(M, N)
        ops.gemm(xd, wd, bd, act=dict(relu=L.ACT_RELU, gelu=L.ACT_GELU)[form], out=out)
    torch.cuda.synchronize()
    owned(out, 'out')
    tol(out, ref, 1e-5, 1e-5)
    if form == 'relu':
        assert bool((out.cpu()[ref == 0.] == 0.).all())
