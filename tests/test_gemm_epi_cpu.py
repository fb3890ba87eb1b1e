"""The GEMM epilogue tests' references, case tables and bounds, settled without a GPU (tests/gemm_epi_cases.py):
every closed form against torch.autograd in fp64, the bounds against a plain fp32 restatement of the same formulas,
the case tables against the (combination, path, epilogue form) triples gemm_run can reach, and the C ABI of the
entry the GPU tests drive (XtrlGemmDesc / xtrl_gemm_epi, ABI 30)."""
import ctypes
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import gemm_epi_cases as GC
from gemm_epi_cases import EPI

REPO = Path(__file__).resolve().parent.parent
D = torch.float64


def close(a, b, tol=1e-10):
    assert a.shape == b.shape
    assert float((a - b).abs().max()) <= tol * max(1., float(b.abs().max())), float((a - b).abs().max())


def _g(*k):
    return GC._gen(99, *k)


# ----------------------------------------------------------------------------------------------
# closed forms vs autograd
# ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('rms', [0, 1])
@pytest.mark.parametrize('M,N', [(1, 36), (70, 132)])
def test_norm_forward_is_torch_layer_norm_or_normalize(M, N, rms):
    x = torch.randn(M, N, generator=_g(M, N), dtype=D) * 2 + 0.5
    xh, mean, rstd = GC.ln_rows(x, rms)
    if rms:   # x-transformers RMSNorm: F.normalize(x, dim = -1) * sqrt(dim)
        close(xh, F.normalize(x, dim=-1) * N ** 0.5)
        assert float(mean.abs().max()) == 0.
    else:
        close(xh, F.layer_norm(x, (N,), eps=1e-5))
        close(mean, x.mean(1))
    close(xh, (x - mean[:, None]) * rstd[:, None])


@pytest.mark.parametrize('rms', [0, 1])
@pytest.mark.parametrize('M,N', [(1, 36), (130, 64), (70, 200)])
def test_norm_backward_closed_form_is_autograd(M, N, rms):
    """dx, d gamma (the sum of the row-tile partials) and d beta of y = LN(x) gamma + beta."""
    g_ = _g(M, N, rms)
    x = (torch.randn(M, N, generator=g_, dtype=D) * 1.5 + 0.3).requires_grad_()
    gamma = (torch.rand(N, generator=g_, dtype=D) + 0.5).requires_grad_()
    beta = torch.randn(N, generator=g_, dtype=D).requires_grad_()
    up = torch.randn(M, N, generator=g_, dtype=D)
    xh, mean, rstd = GC.ln_rows(x, rms)
    ((xh * gamma + beta) * up).sum().backward()
    dx, xh_c = GC.ln_bwd(up, x.detach(), mean.detach(), rstd.detach(), gamma.detach(), rms)
    close(dx, x.grad)
    rows = GC.gemm_ln_rows(N)
    close(GC.tile_sums(up * xh_c, rows).sum(0), gamma.grad)
    close(GC.tile_sums(up, rows).sum(0), beta.grad)
    assert GC.tile_sums(up, rows).shape[0] == -(-M // rows)


def _f64_case(c):
    d = GC.ln_inputs(c)
    return c, {k: (v.double() if torch.is_tensor(v) else v) for k, v in d.items()}


def test_ln_bwd_reference_is_autograd():
    """EPI_LN_BWD through ln_reference: the x-transformers LayerNorm's input gradient plus the residual gradient."""
    for rms in (0, 1):
        c, d = _f64_case(GC.LnCase(EPI['LN_BWD'], 132, 70, 36, rms, 'sep'))
        x = d['ln_x'].clone().requires_grad_()
        xh, mean, rstd = GC.ln_rows(x, rms)
        d['ln_stats'] = torch.stack([mean, rstd], 1).detach()
        up = d['a'] @ d['b']
        ((xh * d['ln_g']) * up).sum().backward()
        ref = GC.ln_reference(c, d)
        close(ref['C'], x.grad + d['ln_dres'])
        close(ref['ln_part'].sum(0), (up * xh.detach()).sum(0))


def test_post_norm_chain_reference_is_autograd():
    """EPI_LN_BWD2 with the chain: y = LN1(LN2(x2) g2 + b2) g1 + b1 (two nn.LayerNorm whose residual path has no
    other branch), upstream gscale v + gpre: the gradients of x1, x2 and both (weight, bias) pairs."""
    c, d = _f64_case(GC.LnCase(EPI['LN_BWD2'], 64, 130, 36, 0, 'side'))
    g_ = _g(7)
    x2 = d['ln2_x'].clone().requires_grad_()
    w2, b2 = d['ln2_g'].clone().requires_grad_(), torch.randn(64, generator=g_, dtype=D).requires_grad_()
    w1, b1 = d['ln_g'].clone().requires_grad_(), torch.randn(64, generator=g_, dtype=D).requires_grad_()
    x1 = F.layer_norm(x2, (64,), w2, b2, 1e-5)
    x1.retain_grad()
    y = F.layer_norm(x1, (64,), w1, b1, 1e-5)
    up = c.opt['gscale'] * (d['a'] @ d['b']) + d['ln_gpre'][:, :64]
    (y * up).sum().backward()
    d['ln_x'] = x1.detach()
    for k, x in (('ln_stats', x1), ('ln2_stats', x2)):
        _, mean, rstd = GC.ln_rows(x.detach(), 0)
        d[k] = torch.stack([mean, rstd], 1)
    ref = GC.ln_reference(c, d)
    close(ref['C'], x1.grad)
    close(ref['ln2_out'], x2.grad)
    for k, p in (('ln_part', w1), ('ln_part_b', b1), ('ln2_part', w2), ('ln2_part_b', b2)):
        assert ref[k].shape == (2, 64)
        close(ref[k].sum(0), p.grad)


def test_residual_layernorm_reference_is_torch():
    for rms in (0, 1):
        c, d = _f64_case(GC.LnCase(EPI['RES_LN'], 36, 130, 36, rms, 'beta_y2'))
        ref = GC.ln_reference(c, d)
        x = d['a'] @ d['b'] + d['R'][:, :36]
        close(ref['C'], x)
        n = F.normalize(x, dim=-1) * 6. if rms else F.layer_norm(x, (36,), eps=1e-5)
        close(ref['ln_y1'], n * d['ln_g'] + d['ln_b'])
        close(ref['ln_y2'], ref['ln_y1'] + d['ln_b2'])
        # the padded-token row
        assert float(ref['C'][129].abs().max()) == 0. and float(ref['mean'][129]) == 0.
        assert torch.equal(ref['ln_y1'][129], d['ln_b'])
        if not rms:
            assert abs(float(ref['rstd'][129]) - 1e-5 ** -0.5) < 1e-9
        assert abs(float(ref['C'][0].mean()) - 16.) < 1.


def test_activation_derivatives_are_autograd():
    v = (torch.randn(50, 37, generator=_g(1), dtype=D) * 3).requires_grad_()
    for fn, ref in ((F.gelu, GC.gelu_and_deriv), (F.silu, GC.silu_and_deriv)):
        v.grad = None
        y = fn(v)
        y.sum().backward()
        f, df = ref(v.detach())
        close(f, y.detach())
        close(df, v.grad)


def test_epilogue_references_are_autograd():
    g_ = _g(2)
    v = (torch.randn(40, 21, generator=g_, dtype=D) * 2).requires_grad_()
    keep = torch.rand(40, 21, generator=g_) > 0.25
    # GELU + dropout: C = keep gelu(v) / (1 - p); aux_out its derivative; dropped elements exactly 0 in both
    c, aux = GC.epilogue_ref(EPI['GELU_DROP'], v, keep=keep, p=0.25)
    close(c.detach(), F.gelu(v.detach()) * keep / 0.75)
    c.sum().backward()
    close(aux.detach(), v.grad)
    assert float(c.detach()[~keep].abs().max()) == 0. and float(aux.detach()[~keep].abs().max()) == 0.
    # SiLU on the first act_cols columns, identity after
    v.grad = None
    c, aux = GC.epilogue_ref(EPI['SILU_SAVE'], v, act_cols=20)
    close(c.detach(), torch.cat([F.silu(v.detach()[:, :20]), v.detach()[:, 20:]], 1))
    c.sum().backward()
    close(aux.detach(), v.grad)
    assert float((aux.detach()[:, 20] - 1.).abs().max()) == 0.
    # the value gate og = o sigmoid(gate): with v = d og, C = d o and aux_out = d gate (aux_in = o, aux_in2 = gate)
    o = torch.randn(40, 21, generator=g_, dtype=D).requires_grad_()
    gate = torch.randn(40, 21, generator=g_, dtype=D).requires_grad_()
    (o * torch.sigmoid(gate) * v.detach()).sum().backward()
    c, aux = GC.epilogue_ref(EPI['DGATE'], v.detach(), aux_in=o.detach(), aux_in2=gate.detach())
    close(c, o.grad)
    close(aux, gate.grad)
    # a ReLU's backward from its output, zeros of both signs masked; the saved-derivative multiply
    out = torch.tensor([[1.5, 0.0, -0.0, 2.0]], dtype=D)
    c, _ = GC.epilogue_ref(EPI['MASK_POS'], torch.full((1, 4), 3., dtype=D), aux_in=out)
    assert c.tolist() == [[3., 0., 0., 3.]]
    c, _ = GC.epilogue_ref(EPI['MUL_AUX'], v.detach(), aux_in=o.detach())
    close(c, v.detach() * o.detach())


def test_glu_references_are_autograd():
    u, dh = GC.glu_inputs(7, 37)
    u = u[:, :74].double().requires_grad_()
    dh = dh[:, :37].double()
    keep = torch.rand(7, 37, generator=_g(3)) > 0.1
    h = GC.glu_fwd_ref(u, 37, keep, 0.1)
    close(h.detach(), u.detach()[:, :37] * F.gelu(u.detach()[:, 37:]) * keep / 0.9)
    (h * dh).sum().backward()
    close(GC.glu_bwd_ref(dh, u.detach(), 37, keep, 0.1), u.grad)


# ----------------------------------------------------------------------------------------------
# the bounds against the fp32 restatement
# ----------------------------------------------------------------------------------------------


def test_fp32_restatement_within_a_quarter_of_each_bound():
    """The same formulas in plain fp32 torch stay inside a quarter of every bound (the measured ratios and the
    constant they give are in the module docstring of gemm_epi_cases; run with -s to see them)."""
    worst = {}

    def note(key, err, bnd):
        r = float((err / bnd).max())
        worst[key] = max(worst.get(key, 0.), r)

    for c in GC.EW_CASES:
        if c.M > 2000 and c.combo != GC.COMBOS[0] and c.epi not in GC.AUX_OUT_EPIS:
            continue   # (the large shapes once per output kind: their restatement differs only in the shared product)
        d = GC.ew_inputs(c)
        keep = torch.rand(c.M, c.N, generator=_g(c.M, c.N)) > c.p
        r64, a64 = GC.ew_reference(c, d, keep)
        r32, a32 = GC.ew_reference(c, d, keep, torch.float32)
        note('forward C', (r32.double() - r64).abs(), GC.fwd_bound(r64))
        if a64 is not None:
            note('forward aux_out', (a32.double() - a64).abs(), GC.fwd_bound(a64))
    part_unit = part_full = 0.
    for c in GC.LN_CASES:
        d = GC.ln_inputs(c)
        r64 = GC.ln_reference(c, d)
        r32 = GC.ln_reference(c, d, torch.float32)
        name = GC.EPI_NAME[c.epi]
        if c.epi == EPI['RES_LN']:
            for k, b in GC.ln_fwd_bounds(r64).items():
                note(f'{name} {k}', (r32[k].double() - r64[k]).abs(), b)
            continue
        bnd = GC.ln_bounds(c, d, r64)
        # the partial sums: with the GEMM output given exactly (the fp64 product rounded to fp32) the quarter rule
        # holds and their error in units of 2^-24 sum |term| gives PART_C.  With the fp32 product the restatement
        # must stay inside the bound, but not a quarter of it: that share of the bound is the project's
        # 7 x 2^-24 sum |a b| of a product, of which the BLAS's own summation takes up to 2.5 (the native fp32 MFMA
        # path 3 - 5, test_gemm_large_tile_split_bf16_accuracy), and the ratio does not move with the inputs' scale
        rx = GC.ln_reference(c, d, torch.float32, v=(d['a'].double() @ d['b'].double()).float())
        for k, b in bnd.items():
            if 'part' in k and not k.startswith('ln2'):
                note(f'{name} {k}', (rx[k].double() - r64[k]).abs(), b)
                full = float(((r32[k].double() - r64[k]).abs() / b).max())
                part_full = max(part_full, full)
            else:
                note(f'{name} {k}', (r32[k].double() - r64[k]).abs(), b)
        for k, w in (('ln_part', r64['xh'].abs()), ('ln_part_b', 1.)):
            if k in r64['terms']:
                unit = GC.EPS24 * GC.tile_sums(r64['gmag'] * w, GC.gemm_ln_rows(c.N))
                part_unit = max(part_unit, float(((rx[k].double() - r64[k]).abs() / unit).max()))
    for k, r in sorted(worst.items()):
        print(f'\n  fp32 restatement / bound  {k:24s} {r:.3f}', end='')
    print(f'\n  partial sums, exact GEMM output: {part_unit:.2f} x 2^-24 x sum |term|  (PART_C = {GC.PART_C:g})')
    print(f'  partial sums, fp32 product: {part_full:.3f} of the bound')
    assert 4 * part_unit <= GC.PART_C and part_full < 1.
    bad = {k: r for k, r in worst.items() if r > 0.25}
    assert not bad, bad


# ----------------------------------------------------------------------------------------------
# the case tables against the dispatch
# ----------------------------------------------------------------------------------------------


def _reachable():
    """(combination, path, form) triples gemm_run can reach, from the `if constexpr` exclusions of dispatch_geom:
    A "T" never takes the tall-narrow path; the gate epilogue and the LN prologue never take the warp-specialised
    kernel; GELU + dropout has its scalar epilogue only on the scalar-load kernel.  Each combination has one form of
    the 64 x 64 tile (split-bf16 for "N" x "N" without the gate, native fp32 otherwise)."""
    out = set()
    for combo in GC.COMBOS:
        ta, tb, epi, ln, res = combo
        for path in GC.PATHS:
            if path == 'tall_wk2' and ta:
                continue
            if path == 'ws128' and (epi == EPI['DGATE'] or ln):
                continue
            for form in ('v4', 'scalar'):
                if form == 'scalar' and epi == EPI['GELU_DROP'] and path != 'scalar64':
                    continue
                out.add((combo, path, form))
    return out


def test_case_table_reaches_every_combination_path_and_form():
    got = {(c.combo, c.path, c.form) for c in GC.EW_CASES}
    assert len(got) == len(GC.EW_CASES)
    assert got == _reachable()
    assert len(got) == 196        # 101 (combination, path) pairs, 95 of them in both epilogue forms
    assert len({(c.combo, c.path) for c in GC.EW_CASES}) == 101
    for c in GC.EW_CASES:
        assert GC.expected_path(c.M, c.N, c.K, c.ta, c.tb, c.epi, c.ln, c.vec) == c.path, c.id
        assert c.epi_v4 == (c.form == 'v4'), c.id
        M, N, K = GC.PATH_SHAPE[c.path]
        assert (c.M, c.K) == (M, K) and abs(c.N - N) <= 1
        # every extent ragged against its tile
        bm, bn = {'scalar64': (64, 64), 'tall_wk2': (64, 32), 'x6_128': (128, 128), 'ws128': (128, 128),
                  'tile64': (64, 64), 'small_wk2': (64, 32), 'wk4': (32, 32)}[c.path]
        assert c.M % bm and c.N % bn, c.id
    # every epilogue sees every beta and a bias offset where it takes a bias; GELU + dropout every p
    for epi in {c.epi for c in GC.EW_CASES}:
        mine = [c for c in GC.EW_CASES if c.epi == epi]
        assert {c.beta for c in mine} == set(GC.BETAS), epi
        if any(c.bias for c in mine):
            assert any(c.bias_col0 > 0 for c in mine), epi
    assert {c.p for c in GC.EW_CASES if c.epi == EPI['GELU_DROP']} == set(GC.DROP_PS)
    # both forms of the 64 x 64 tile, and the instantiation names the reach trace is compared with
    names = {GC.expected_kernel(c.M, c.N, c.K, c.ta, c.tb, c.epi, c.ln, c.vec, c.res) for c in GC.EW_CASES}
    assert 'k_gemm<2, 2, 1, 1, 1, false, false, 4, false, false, true, true>' in names
    assert 'k_gemm<2, 2, 1, 1, 1, false, true, 7, false, false, true, false>' in names
    assert 'k_gemm_ws<true, true, 0, false, 128, 128, false' in names
    assert 'k_gemm<2, 2, 1, 2, 2, false, true, 7, false, false, true, true>' in names


def test_layernorm_case_table():
    assert len(GC.LN_CASES) == 3 * 18 * 4 * 2 * 3
    names = {GC.expected_kernel(c.M, c.N, c.K, 0, c.tb, c.epi, False, True, c.epi == EPI['RES_LN'])
             for c in GC.LN_CASES}
    assert names == {f'k_gemm_ws<false, false, 9, true, {t}, {kt}' for t in ('128, 128', '64, 256')
                     for kt in ('true', 'false')} | \
        {f'k_gemm_ws<false, true, {e}, false, {t}, true' for e in (10, 12) for t in ('128, 128', '64, 256')}
    for N, M in GC.LN_NM:
        rows = GC.gemm_ln_rows(N)
        assert rows == (128 if N <= 128 else 64) and N % 4 == 0 and N <= 256
    assert {M % GC.gemm_ln_rows(N) for N, M in GC.LN_NM} == {0, 1, 2, 6}   # whole tiles, one row, a short last tile
    assert {K % 32 for K in GC.LN_KS} == {0, 4} and {-(-K // 32) for K in GC.LN_KS} == {1, 2, 3, 9}
    chain = [c for c in GC.LN_CASES if c.opt.get('chain')]
    assert chain and all(c.rms == 0 for c in chain)
    assert any(c.rms == 1 and c.epi == EPI['LN_BWD2'] for c in GC.LN_CASES)


# ----------------------------------------------------------------------------------------------
# the C ABI
# ----------------------------------------------------------------------------------------------


def test_gemm_epi_abi():
    from xtrl_amd import _lib
    text = (REPO / 'include' / 'xtrl_hip.h').read_text()
    abi = int(re.search(r'#define XTRL_ABI_VERSION (\d+)', text).group(1))
    assert abi == _lib.ABI_VERSION >= 30
    lib = _lib.load()
    assert lib.xtrl_abi_version() == abi
    assert int(lib.xtrl_struct_size(b'XtrlGemmDesc')) == ctypes.sizeof(_lib.GemmDesc)
    for name, val in EPI.items():
        assert int(re.search(r'#define XTRL_EPI_%s (\d+)' % name, text).group(1)) == val == getattr(_lib, f'EPI_{name}')
    # the enum the defines mirror (static_asserts in csrc/gemm.hip hold the two together at compile time)
    enum = re.search(r'enum GemmEpi : int \{(.*?)\};', (REPO / 'x-transformers-rl_amd' / 'csrc' / 'kernels.h').read_text(),
                     re.S).group(1)
    assert {m.group(1): int(m.group(2)) for m in re.finditer(r'EPI_(\w+) = (\d+)', enum)} == EPI
    # the descriptor's fields, in the header's order
    body = re.search(r'typedef struct XtrlGemmDesc \{(.*?)\n\} XtrlGemmDesc;', text, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = [n.strip(' *') for decl in body.split(';') if decl.strip()
              for n in decl.strip().split(None, 1)[1].replace('float*', '').replace('float ', '').split(',')]
    assert fields == [n for n, _ in _lib.GemmDesc._fields_]
    # internal arguments stay out of it
    for name in ('kspan', 'c_split', 'rowsum', 't_dev', 'row_mask', 'wimg', 'wfrag', 'xcd_remap'):
        assert not any(name in f for f in fields), name


def test_gemm_epi_refusals_reach_no_kernel():
    """The argument checks are host code ahead of any launch: reachable without a GPU (the operands are never
    read).  The GPU tests repeat them with NaN-filled outputs."""
    from xtrl_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 4)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def desc(**kw):
        d = _lib.GemmDesc(A=p, B=p, C=p, R=p, lda=64, ldb=64, ldr=64, ldc=64, M=4, N=64, K=64, ln_g=p, ln_stats=p,
                          ln_y1=p, ln_ld1=64, ln_gscale=1.)
        for k, v in kw.items():
            setattr(d, k, v)
        return d
    assert lib.xtrl_gemm_epi(None, 0, 0, 0, None) == 1
    d = desc(N=260, ldb=64, ldc=260, ldr=260, ln_ld1=260)
    assert lib.xtrl_gemm_epi(ctypes.byref(d), 0, 0, EPI['RES_LN'], None) == 1
    assert 'N=260' in lib.xtrl_last_error().decode()
    d = desc(ln_stats=None)
    assert lib.xtrl_gemm_epi(ctypes.byref(d), 0, 0, EPI['RES_LN'], None) == 1
    d = desc(R=None, aux_in=p, aux_out=p, ld_aux_in=64, ld_aux_out=64)
    assert lib.xtrl_gemm_epi(ctypes.byref(d), 0, 1, EPI['DGATE'], None) == 1
    assert 'aux_in2' in lib.xtrl_last_error().decode()
    d = desc(R=None)
    assert lib.xtrl_gemm_epi(ctypes.byref(d), 1, 0, EPI['NONE'], None) == 1    # no such combination
    assert 'unsupported combination' in lib.xtrl_last_error().decode()
    d = desc(drop_p=1.0)
    assert lib.xtrl_gemm_epi(ctypes.byref(d), 0, 0, EPI['GELU_DROP'], None) == 1
