"""Kernel-level fp64 tests of the fp32 GEMM's epilogues (csrc/gemm.hip through xtrl_gemm_epi), over the tables of
tests/gemm_epi_cases.py: every (layout, epilogue, LN prologue, residual) combination of gemm_run on every geometry
path it can take, in the row-vector and the scalar epilogue form, and the LayerNorm epilogues over both tile
families, K tails and one-row last tiles.  Then the direct entries no test called: xtrl_gemm_ex with bias and beta,
xtrl_linear_gelu_drop, xtrl_glu_drop_fwd / _bwd and xtrl_layernorm_f32.

Every output is NaN before the call; owned elements must come back finite and inside their bound (module docstring
of gemm_epi_cases), padding columns and guard rows still NaN bit for bit.  Each test prints its worst error as a
fraction of the bound (pytest -s)."""
import ctypes as C
import math
from functools import lru_cache

import pytest
import torch

import gemm_epi_cases as GC
from gemm_epi_cases import EPI, NAN

pytestmark = pytest.mark.gpu
DEV = 'cuda'
NAN_BITS = int(GC.bits(torch.tensor([NAN]))[0])


def dev(t):
    return None if t is None else t.to(DEV)


def nan_buf(rows, ld):
    return torch.full((rows, ld), NAN, device=DEV)


class Checked:
    """One output buffer [rows][ld]: regions checked against their references, the rest against the NaN prefill."""

    def __init__(self, name, buf):
        self.name, self.buf = name, buf.cpu()
        self.owned = torch.zeros(self.buf.shape, dtype=torch.bool)

    def region(self, ref, bound, col0=0, what=None):
        what = what or self.name
        ref = ref.reshape(ref.shape[0], -1)
        M, N = ref.shape
        got = self.buf[:M, col0:col0 + N]
        self.owned[:M, col0:col0 + N] = True
        assert bool(torch.isfinite(got).all()), f'{what}: non-finite owned elements'
        ratio = (got.double() - ref).abs() / bound.reshape(M, -1)
        worst = float(ratio.max())
        assert worst <= 1., (f'{what}: error {worst:.3f} of the bound at {divmod(int(ratio.argmax()), N)}: '
                             f'{float(got.reshape(-1)[ratio.argmax()])} vs {float(ref.reshape(-1)[ratio.argmax()])}')
        return worst

    def rest_untouched(self):
        assert bool((GC.bits(self.buf)[~self.owned] == NAN_BITS).all()), f'{self.name}: padding or guard rows written'


def keep_bits(M, N, p):
    """The keep bits of the feed-forward dropout stream (xtrl_ff_dropout_mask, tied to the host Philox stream by
    test_ff_dropout_mask_is_host_philox_stream)."""
    from xtrl_amd import _lib as L
    if p == 0.:
        return torch.ones(M, N, dtype=torch.bool)
    mask = torch.zeros(M, N, dtype=torch.uint8, device=DEV)
    L.check(L.lib().xtrl_ff_dropout_mask(L.ptr(mask), M, N, p, GC.DROP_SEED, GC.DROP_OFFSET, GC.DROP_LAYER, L.stream()),
            'ff_dropout_mask')
    keep = mask.cpu().bool()
    assert 0.5 * (1 - p) < float(keep.float().mean()) <= 1.
    return keep


def gemm_epi(ta, tb, epi, **kw):
    from xtrl_amd import _lib as L
    d = L.GemmDesc(ln_gscale=1.)
    for k, v in kw.items():
        setattr(d, k, v.data_ptr() if torch.is_tensor(v) else v)
    rc = L.lib().xtrl_gemm_epi(C.byref(d), ta, tb, epi, L.stream())
    torch.cuda.synchronize()
    return rc


# ----------------------------------------------------------------------------------------------
# element-wise epilogues on every geometry path
# ----------------------------------------------------------------------------------------------


@lru_cache(maxsize=2)
def _dev_operands(path, ta, tb):
    _, _, A, B, gamma = GC._ew_operands(path, ta, tb)
    return A.to(DEV), B.to(DEV), gamma.to(DEV)


@pytest.mark.parametrize('c', GC.EW_CASES, ids=lambda c: c.id)
def test_elementwise_epilogue(c):
    from xtrl_amd import _lib as L
    d = GC.ew_inputs(c)
    A, B, gamma = _dev_operands(c.path, c.ta, c.tb)
    keep = keep_bits(c.M, c.N, c.p) if c.epi == EPI['GELU_DROP'] else None
    Cb = d['C0'].to(DEV)
    aux_out = nan_buf(c.M + 2, c.ldo) if c.epi in GC.AUX_OUT_EPIS else None
    hold = {k: dev(d[k]) for k in ('bias', 'R', 'aux_in', 'aux_in2')}
    kw = dict(A=A, B=B, C=Cb, lda=c.lda, ldb=c.ldb, ldc=c.ldo, M=c.M, N=c.N, K=c.K, beta=c.beta,
              bias_col0=c.bias_col0, act_cols=c.act_cols, ln_rms=c.ln_rms)
    if c.ln:
        kw['gamma'] = gamma
    if c.bias:
        kw['bias'] = hold['bias']
    if c.res:
        kw.update(R=hold['R'], ldr=c.ldo)
    if hold['aux_in'] is not None:
        kw.update(aux_in=hold['aux_in'], ld_aux_in=c.ldo)
    if hold['aux_in2'] is not None:
        kw.update(aux_in2=hold['aux_in2'], ld_aux_in2=c.ldo)
    if aux_out is not None:
        kw.update(aux_out=aux_out, ld_aux_out=c.ldo)
    if c.epi == EPI['GELU_DROP']:
        kw.update(drop_p=c.p, drop_seed=GC.DROP_SEED, drop_offset=GC.DROP_OFFSET, drop_layer=GC.DROP_LAYER)
    rc = gemm_epi(c.ta, c.tb, c.epi, **kw)
    assert rc == 0, L.load().xtrl_last_error().decode()
    ref, aux_ref = GC.ew_reference(c, d, keep)
    out = Checked('C', Cb)
    worst = {'C': out.region(ref, GC.fwd_bound(ref))}
    out.rest_untouched()
    if aux_out is not None:
        ao = Checked('aux_out', aux_out)
        worst['aux_out'] = ao.region(aux_ref, GC.fwd_bound(aux_ref))
        ao.rest_untouched()
        if c.epi == EPI['GELU_DROP'] and c.p > 0. and c.beta == 0.:   # dropped elements exactly 0 in both outputs
            assert float(out.buf[:c.M, :c.N][~keep].abs().max()) == 0.
        if c.epi == EPI['GELU_DROP'] and c.p > 0.:
            assert float(ao.buf[:c.M, :c.N][~keep].abs().max()) == 0.
    print(f' [{c.M}x{c.N}x{c.K} beta {c.beta:g}] worst / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()),
          end='')


# ----------------------------------------------------------------------------------------------
# LayerNorm epilogues
# ----------------------------------------------------------------------------------------------


def _run_ln_case(c, worst):
    from xtrl_amd import _lib as L
    d = GC.ln_inputs(c)
    o, M, N, K = c.opt, c.M, c.N, c.K
    hold = {k: dev(v) for k, v in d.items() if torch.is_tensor(v)}
    kw = dict(A=hold['A'], B=hold['B'], lda=K + 4, ldb=(N if c.tb else K) + 4, M=M, N=N, K=K, ln_rms=c.rms,
              ln_g=hold['ln_g'])
    T = c.tiles
    bufs = {}
    if c.epi == EPI['RES_LN']:
        bufs = dict(C=nan_buf(M + 2, N + 4), ln_y1=nan_buf(M + 2, N + 4), ln_stats=nan_buf(M + 2, 2))
        kw.update(R=hold['R'], ldr=N + 4, C=bufs['C'], ldc=N + 4, ln_y1=bufs['ln_y1'], ln_ld1=N + 4,
                  ln_stats=bufs['ln_stats'])
        if o['y2']:
            bufs['ln_y2'] = nan_buf(M + 2, N + 8)
            kw.update(ln_y2=bufs['ln_y2'], ln_ld2=N + 8)
        for k in ('bias', 'ln_b', 'ln_b2'):
            if d[k] is not None:
                kw[k] = hold[k]
    else:
        kw.update(ln_x=hold['ln_x'], ln_stats=hold['ln_stats'])
        alias = c.epi == EPI['LN_BWD'] and o['dres'] == 'alias'
        ldc = N if (alias or c.epi == EPI['LN_BWD2']) else N + 4
        bufs['C'] = nan_buf(M + 2, ldc)
        if alias:   # ln_dres is C itself (ldc == N): the residual gradient updated in place
            bufs['C'][:M] = hold['ln_dres']
            kw['ln_dres'] = bufs['C']
        elif c.epi == EPI['LN_BWD'] and o['dres'] == 'sep':
            kw['ln_dres'] = hold['ln_dres']
        kw.update(C=bufs['C'], ldc=ldc)
        if c.epi == EPI['LN_BWD']:
            bufs['ln_part'] = nan_buf(T + 1, N)
            kw['ln_part'] = bufs['ln_part']
        else:
            names = ['ln_part'] + (['ln_part_b'] if o['part_b'] else []) + (['ln2_part', 'ln2_part_b'] if o['chain'] else [])
            kw['ln_gscale'] = o['gscale']
            if d['ln_gpre'] is not None:
                kw.update(ln_gpre=hold['ln_gpre'], ln_ldg=0 if o['gpre'] == 0 else 2 * N)
            if o['pstride']:   # the four partial sets of one row tile side by side
                bufs['parts'] = nan_buf(T + 1, 4 * N)
                kw['ln_pstride'] = 4 * N
                for i, k in enumerate(('ln_part', 'ln_part_b', 'ln2_part', 'ln2_part_b')):
                    if k in names:
                        kw[k] = bufs['parts'].data_ptr() + 4 * N * i
            else:
                for k in names:
                    bufs[k] = nan_buf(T + 1, N)
                    kw[k] = bufs[k]
            if o['chain']:
                bufs['ln2_out'] = nan_buf(M + 2, N)
                kw.update(ln2_out=bufs['ln2_out'], ln2_g=hold['ln2_g'], ln2_x=hold['ln2_x'], ln2_stats=hold['ln2_stats'])
    rc = gemm_epi(0, c.tb, c.epi, **kw)
    assert rc == 0, (c.id, L.load().xtrl_last_error().decode())
    ref = GC.ln_reference(c, d)
    chk = {k: Checked(f'{c.id} {k}', b) for k, b in bufs.items()}

    def note(k, r):
        worst[k] = max(worst.get(k, 0.), r)

    if c.epi == EPI['RES_LN']:
        bnd = GC.ln_fwd_bounds(ref)
        for k in ('C', 'ln_y1', 'ln_y2'):
            if k in chk:
                note(k, chk[k].region(ref[k], bnd[k]))
        note('mean', chk['ln_stats'].region(ref['mean'][:, None], bnd['mean'][:, None], 0, f'{c.id} mean'))
        note('rstd', chk['ln_stats'].region(ref['rstd'][:, None], bnd['rstd'][:, None], 1, f'{c.id} rstd'))
        if o['zero_row']:   # the padded-token row: mean 0, rstd = 1 / sqrt(eps), y = beta
            m = M - 1
            st = chk['ln_stats'].buf[m]
            assert float(st[0]) == 0. and float(chk['C'].buf[m, :N].abs().max()) == 0.
            if not c.rms:
                assert abs(float(st[1]) - 1e-5 ** -0.5) <= 1e-5 * 1e-5 ** -0.5
            assert torch.equal(chk['ln_y1'].buf[m, :N], d['ln_b'])
    else:
        bnd = GC.ln_bounds(c, d, ref)
        note('C', chk['C'].region(ref['C'], bnd['C']))
        if 'ln2_out' in ref:
            note('ln2_out', chk['ln2_out'].region(ref['ln2_out'], bnd['ln2_out']))
        for i, k in enumerate(('ln_part', 'ln_part_b', 'ln2_part', 'ln2_part_b')):
            if k in ref:
                if 'parts' in chk:
                    note(k, chk['parts'].region(ref[k], bnd[k], N * i, f'{c.id} {k}'))
                else:
                    note(k, chk[k].region(ref[k], bnd[k]))
    for ck in chk.values():
        ck.rest_untouched()


@pytest.mark.parametrize('N,M', GC.LN_NM)
@pytest.mark.parametrize('epi', ['RES_LN', 'LN_BWD', 'LN_BWD2'])
def test_layernorm_epilogue(epi, N, M):
    """K in {32, 36, 96, 260} x both ln_rms values x the epilogue's argument variants at one (N, M)."""
    worst = {}
    cases = GC.ln_cases(EPI[epi], N, M)
    for c in cases:
        _run_ln_case(c, worst)
    print(f' [{len(cases)} cases] worst / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()), end='')


def test_refusals_leave_outputs_untouched():
    """EPI_RES_LN with N = 260, EPI_RES_LN without ln_stats, EPI_DGATE without aux_in2: nonzero, nothing written."""
    M, K = 8, 32
    for what in ('wide', 'nostats', 'nogate'):
        N = 260 if what == 'wide' else 64
        a, b = torch.randn(M, K, device=DEV), torch.randn(max(N, K), max(N, K), device=DEV)
        r, g = torch.randn(M, N, device=DEV), torch.ones(N, device=DEV)
        outs = [nan_buf(M, N) for _ in range(3)]
        stats = nan_buf(M, 2)
        if what == 'nogate':
            rc = gemm_epi(0, 1, EPI['DGATE'], A=a, B=b, C=outs[0], lda=K, ldb=max(N, K), ldc=N, M=M, N=N, K=K,
                          aux_in=r, ld_aux_in=N, aux_out=outs[1], ld_aux_out=N)
        else:
            kw = dict(A=a, B=b, C=outs[0], R=r, lda=K, ldb=max(N, K), ldr=N, ldc=N, M=M, N=N, K=K, ln_g=g, ln_y1=outs[1],
                      ln_ld1=N, ln_y2=outs[2], ln_ld2=N)
            if what == 'wide':
                kw['ln_stats'] = stats
            rc = gemm_epi(0, 0, EPI['RES_LN'], **kw)
        assert rc != 0, what
        for t in outs + [stats]:
            assert bool((GC.bits(t.cpu()) == NAN_BITS).all()), what


# ----------------------------------------------------------------------------------------------
# the direct entries
# ----------------------------------------------------------------------------------------------


@lru_cache(maxsize=2)
def _ex_operands(M, N, K):
    g = GC._gen(8, M, N, K)
    a, b = torch.randn(M, K, generator=g), torch.randn(K, N, generator=g) / math.sqrt(K)
    return a, b, a.double() @ b.double(), GC.dot_scale(a.double(), b.double())


@pytest.mark.parametrize('beta', GC.BETAS)
@pytest.mark.parametrize('ta,tb', [(0, 0), (0, 1), (1, 1)])
@pytest.mark.parametrize('M,N,K', [(70, 99, 72), (1030, 1000, 72)])
def test_gemm_ex_bias_and_beta(M, N, K, ta, tb, beta):
    """C = beta C + A . B + bias through xtrl_gemm_ex.  Bound: the bare-product figure 7 x 2^-24 over the absolute
    sum of everything added into an element, sum_k |a b| + |bias| + |beta C|.  beta = 0 never reads the NaN prefill."""
    from xtrl_amd import _lib as L
    a, b, prod, scale = _ex_operands(M, N, K)
    g = GC._gen(9, M, N, K, ta, tb)
    bias = torch.randn(N, generator=g)
    ldc = N + 4
    c0 = torch.full((M + 2, ldc), NAN)
    if beta != 0.:
        c0[:M, :N] = torch.randn(M, N, generator=g)
    A = GC.padded(a.t() if ta else a, GC.BIG)
    B = GC.padded(b if tb else b.t(), GC.BIG)
    Ad, Bd, Cd, bd = A.to(DEV), B.to(DEV), c0.to(DEV), bias.to(DEV)
    L.check(L.lib().xtrl_gemm_ex(ta, tb, L.ptr(Ad), A.shape[1], L.ptr(Bd), B.shape[1], L.ptr(bd), L.ptr(Cd), ldc, M, N, K,
                                 beta, L.stream()), 'gemm_ex')
    torch.cuda.synchronize()
    ref, sc = prod + bias.double(), scale + bias.double().abs()
    if beta != 0.:
        ref, sc = ref + beta * c0[:M, :N].double(), sc + abs(beta) * c0[:M, :N].double().abs()
    out = Checked('C', Cd)
    worst = out.region(ref, 7 * GC.EPS24 * sc)
    out.rest_untouched()
    print(f' worst / bound: {worst:.3f}', end='')


@pytest.mark.parametrize('p', GC.DROP_PS)
@pytest.mark.parametrize('N', [100, 99])
def test_linear_gelu_drop(N, p):
    """Y = drop(gelu(X W^T + b)), deriv = drop(gelu'): N % 4 == 0 and not, no dropout / word mode / byte mode."""
    from xtrl_amd import _lib as L
    M, K = 70, 72
    g = GC._gen(10, N)
    x, w = torch.randn(M, K + 4, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K)
    bias = torch.randn(N, generator=g)
    x[:, K:] = GC.BIG
    ld = N + 4
    y, dv = nan_buf(M + 2, ld), nan_buf(M + 2, ld)
    xd, wd, bd = x.to(DEV), w.to(DEV), bias.to(DEV)
    L.check(L.lib().xtrl_linear_gelu_drop(L.ptr(xd), K + 4, L.ptr(wd), L.ptr(bd), L.ptr(y), ld, L.ptr(dv), ld, M, N, K, p,
                                          GC.DROP_SEED, GC.DROP_OFFSET, GC.DROP_LAYER, L.stream()), 'linear_gelu_drop')
    torch.cuda.synchronize()
    keep = keep_bits(M, N, p)
    ref, dref = GC.epilogue_ref(EPI['GELU_DROP'], x[:, :K].double() @ w.double().t() + bias.double(), keep=keep, p=p)
    cy, cd = Checked('Y', y), Checked('deriv', dv)
    worst = cy.region(ref, GC.fwd_bound(ref)), cd.region(dref, GC.fwd_bound(dref))
    cy.rest_untouched()
    cd.rest_untouched()
    if p > 0.:
        assert float(cy.buf[:M, :N][~keep].abs().max()) == 0. and float(cd.buf[:M, :N][~keep].abs().max()) == 0.
    print(f' worst / bound: Y {worst[0]:.3f}, deriv {worst[1]:.3f}', end='')


@pytest.mark.parametrize('p', GC.DROP_PS)
@pytest.mark.parametrize('M,ff', GC.GLU_CASES)
def test_glu_drop_forward_and_backward(M, ff, p):
    """h = drop(value gelu(gate)) and du from dh, with ldu > 2 ff, ldh > ff, lddu > 2 ff and M ff no multiple of the
    256-thread block; the keep bits are xtrl_ff_dropout_mask's."""
    from xtrl_amd import _lib as L
    assert (M * ff) % 256
    u, dh = GC.glu_inputs(M, ff)
    ud, dhd = u.to(DEV), dh.to(DEV)
    h, du = nan_buf(M + 1, ff + 2), nan_buf(M + 1, 2 * ff + 3)
    args = (p, GC.DROP_SEED, GC.DROP_OFFSET, GC.DROP_LAYER, L.stream())
    L.check(L.lib().xtrl_glu_drop_fwd(L.ptr(ud), u.shape[1], L.ptr(h), ff + 2, M, ff, *args), 'glu_drop_fwd')
    L.check(L.lib().xtrl_glu_drop_bwd(L.ptr(dhd), dh.shape[1], L.ptr(ud), u.shape[1], L.ptr(du), 2 * ff + 3, M, ff, *args),
            'glu_drop_bwd')
    torch.cuda.synchronize()
    keep = keep_bits(M, ff, p)
    u64 = u[:, :2 * ff].double()
    href, duref = GC.glu_fwd_ref(u64, ff, keep, p), GC.glu_bwd_ref(dh[:, :ff].double(), u64, ff, keep, p)
    ch, cdu = Checked('h', h), Checked('du', du)
    worst = ch.region(href, GC.fwd_bound(href)), cdu.region(duref, GC.fwd_bound(duref))
    ch.rest_untouched()
    cdu.rest_untouched()
    if p > 0.:   # the kernels' own keep bits are the mask's: dropped elements are exact zeros, kept ones are not
        assert torch.equal(ch.buf[:M, :ff] != 0., keep)
        assert float(cdu.buf[:M, :ff][~keep].abs().max()) == 0. and float(cdu.buf[:M, ff:2 * ff][~keep].abs().max()) == 0.
    print(f' worst / bound: h {worst[0]:.3f}, du {worst[1]:.3f}', end='')


@pytest.mark.parametrize('M', GC.LAYERNORM_MS)
@pytest.mark.parametrize('D', GC.LAYERNORM_DS)
def test_layernorm_rows(D, M):
    """xtrl_layernorm_f32 with ldx, ldy > D: the N(16, 1) row, the zero row (y = 0), padding untouched."""
    from xtrl_amd import _lib as L
    x, gamma = GC.layernorm_inputs(M, D)
    xd, gd = x.to(DEV), gamma.to(DEV)
    y = nan_buf(M + 1, D + 8)
    L.check(L.lib().xtrl_layernorm_f32(L.ptr(xd), D + 4, L.ptr(gd), L.ptr(y), D + 8, M, D, L.stream()), 'layernorm_f32')
    torch.cuda.synchronize()
    ref = GC.ln_rows(x[:, :D].double(), 0)[0] * gamma.double()
    cy = Checked('y', y)
    worst = cy.region(ref, GC.fwd_bound(ref))
    cy.rest_untouched()
    if M > 1:
        assert float(cy.buf[M - 1, :D].abs().max()) == 0.
    print(f' worst / bound: {worst:.3f}', end='')
