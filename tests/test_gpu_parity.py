"""MI355X parity tests: every HIP kernel through the C ABI vs the oracle / an fp64 torch reference.

Tolerances: integer / index / mask outputs bit-exact; fp32 outputs within 1e-4 relative (BASELINE
north_star), tighter where the computation is short."""
import contextlib
import itertools
import math

import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fractal_ref as FR
from oracle import ref_port as R
from oracle import thirdparty as tp

import attn_harness as AH

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def tol(a, b, rtol=1e-4, atol=1e-5):
    a = a.detach().double().cpu() if torch.is_tensor(a) else torch.as_tensor(a).double()
    b = b.detach().double().cpu() if torch.is_tensor(b) else torch.as_tensor(b).double()
    np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=rtol, atol=atol)


def grad_mismatches(gpu_g, named_params, rtol=1e-4, atol=1e-7):
    """Per-parameter-tensor gradient check: |g_gpu - g_ref| <= rtol * max|g_ref of THAT tensor| + atol
    for every element — a tensor whose gradients are small next to the model's largest ones is held
    to its own scale.  Returns (worst err / own scale, [(name, err, own scale)] of the tensors that fail)."""
    worst, bad = 0., []
    for name, p in named_params:
        if p.grad is None:
            continue
        own = float(p.grad.abs().max())
        err = float((gpu_g[name] - p.grad).abs().max())
        if own > 0:
            worst = max(worst, err / own)
        if err > rtol * own + atol:
            bad.append((name, err, own))
    return worst, bad


# ----------------------------------------------------------------------------------------------
# GEMM (decode projections, FF, heads)
# ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('M,N,K', [(1, 5, 8), (37, 100, 96), (64, 64, 64), (130, 257, 48), (1024, 1024, 256),
                                   (515, 4, 512),
                                   # learn-step geometry rules: narrow outputs over many rows (64x32/WK2),
                                   # K = 64 over 16384 rows (64x64 instead of 128x128)
                                   (4100, 18, 256), (4096, 4, 512), (16384, 256, 64)])
@pytest.mark.parametrize('mode', ['plain', 'ln_gelu', 'silu', 'residual', 'ln'])
def test_gemm_f32(M, N, K, mode):
    from xtrl_amd import _lib as L, ops
    g = torch.Generator(device='cpu').manual_seed(M * 7 + N)
    x = torch.randn(M, K, generator=g).to(DEV)
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    gam = (torch.rand(K, generator=g) + 0.5).to(DEV)
    res = torch.randn(M, N, generator=g).to(DEV)
    xd, wd = x.double(), w.double()
    if mode == 'plain':
        out, ref = ops.gemm(x, w, b), xd @ wd.T + b.double()
    elif mode == 'silu':
        out, ref = ops.gemm(x, w, b, act=L.ACT_SILU), torch.nn.functional.silu(xd @ wd.T + b.double())
    elif mode == 'residual':
        r2 = res.clone()
        out = ops.gemm(x, w, None, residual=r2, out=r2)
        ref = xd @ wd.T + res.double()
    else:
        xn = torch.nn.functional.layer_norm(xd, (K,), eps=1e-5) * gam.double()
        if mode == 'ln':
            out, ref = ops.gemm(x, w, b, ln_gamma=gam), xn @ wd.T + b.double()
        else:
            out, ref = ops.gemm(x, w, b, ln_gamma=gam, act=L.ACT_GELU), torch.nn.functional.gelu(xn @ wd.T + b.double())
    torch.cuda.synchronize()
    tol(out, ref, 1e-5, 1e-5)


@pytest.mark.parametrize('M,N,K,live', [(1, 5, 8, 1), (37, 260, 256, 30), (1024, 1024, 256, 1024), (1024, 256, 1024, 700),
                                        (300, 256, 64, 300), (130, 100, 512, 77), (64, 1024, 768, 50), (40, 48, 48, 40),
                                        (33, 192, 96, 33), (1000, 512, 384, 999)])
@pytest.mark.parametrize('mode', ['plain', 'ln_gelu', 'ln_silu_part', 'residual', 'scatter'])
def test_dgemm_decode_projection(M, N, K, live, mode):
    """xtrl_dgemm (the rollout's projections over compacted live rows) vs an fp64 torch reference:
    LayerNorm prologue over the first ln_k columns, GELU / SiLU, residual, row scatter, and the
    device live-row count (rows >= live are not written)."""
    import ctypes as C
    from xtrl_amd import _lib as L
    g = torch.Generator(device='cpu').manual_seed(M * 3 + N + K)
    x = torch.randn(M, K, generator=g).to(DEV) + 0.5
    w = (torch.randn(N, K, generator=g) / math.sqrt(K)).to(DEV)
    b = torch.randn(N, generator=g).to(DEV)
    gam = (torch.rand(K, generator=g) + 0.5).to(DEV)
    res = torch.randn(M, N, generator=g).to(DEV)
    m_dev = torch.tensor([live], dtype=torch.int32, device=DEV)
    xd, wd, bd = x.double(), w.double(), b.double()
    ln_k = min(K, 512) if mode == 'ln_gelu' else (K // 2 if mode == 'ln_silu_part' else 0)   # (ln_k <= 512)
    ln_k -= ln_k % 4
    if ln_k:
        xd = xd.clone()
        xd[:, :ln_k] = torch.nn.functional.layer_norm(xd[:, :ln_k], (ln_k,), eps=1e-5) * gam[:ln_k].double()
    ref = xd @ wd.T + bd
    if mode == 'ln_gelu':
        ref = torch.nn.functional.gelu(ref)
    elif mode == 'ln_silu_part':
        ref = torch.nn.functional.silu(ref)
    elif mode == 'residual':
        ref = ref + res.double()
    act = {'ln_gelu': 1, 'ln_silu_part': 2}.get(mode, 0)
    sentinel = -7.0
    rows_out = M + 5 if mode == 'scatter' else M
    out = torch.full((rows_out, N), sentinel, device=DEV)
    row_map = None
    if mode == 'scatter':
        row_map = torch.randperm(rows_out, generator=g)[:M].to(torch.int32).to(DEV)
    if mode == 'residual':
        out[:M] = res
    wp = torch.empty(L.lib().xtrl_dgemm_packed_floats(N, K), device=DEV)
    L.check(L.lib().xtrl_dgemm_pack(L.ptr(w), K, N, K, L.ptr(wp), L.stream()), 'dgemm_pack')
    rc = L.lib().xtrl_dgemm(L.ptr(x), K, L.ptr(wp), L.ptr(b), L.ptr(gam) if ln_k else None, ln_k,
                            L.ptr(out) if mode == 'residual' else None, N, L.ptr(out), N,
                            L.ptr(row_map) if row_map is not None else None, L.ptr(m_dev), M, N, K, act, L.stream())
    L.check(rc, 'dgemm')
    torch.cuda.synchronize()
    if mode == 'scatter':
        got = out[row_map[:live].long()]
        untouched = torch.ones(rows_out, dtype=torch.bool, device=DEV)
        untouched[row_map[:live].long()] = False
        assert bool((out[untouched] == sentinel).all())
    else:
        got = out[:live]
        if mode != 'residual':
            assert bool((out[live:] == sentinel).all())
        else:
            assert torch.equal(out[live:], res[live:])
    tol(got, ref[:live], 2e-5, 2e-5)


@pytest.mark.parametrize('N,K', [(1024, 256), (256, 1024), (20, 64)])
def test_dgemm_pack_x6_pieces_are_exact(N, K):
    """xtrl_dgemm_pack_x6: hi + mid + lo reproduce every fp32 weight exactly, each piece sits in the
    16x16x32 bf16 fragment slot the fused feed-forward kernel reads, zero past N."""
    from xtrl_amd import _lib as L
    g = torch.Generator().manual_seed(N + K)
    w = (torch.randn(N, K, generator=g) * torch.exp(torch.randn(N, K, generator=g))).to(DEV)
    out = torch.zeros(int(L.lib().xtrl_dgemm_packed_x6_elems(N, K)), dtype=torch.int16, device=DEV)
    L.check(L.lib().xtrl_dgemm_pack_x6(L.ptr(w), K, N, K, L.ptr(out), L.stream()), 'dgemm_pack_x6')
    torch.cuda.synchronize()
    Np = (N + 15) // 16 * 16
    bits = out.view(3, Np // 16, K // 32, 4, 16, 8).cpu().to(torch.int32) & 0xFFFF   # piece, tile, step, q, row, j
    f = (bits << 16).view(torch.float32)
    pieces = f.permute(0, 1, 4, 2, 3, 5).reshape(3, Np, K)   # [piece][n][k = 32 step + 8 q + j]
    # the smallest piece first, as the kernel's products: exact because the pieces do not overlap
    total = (pieces[2] + pieces[1]) + pieces[0]
    assert torch.equal(total[:N], w.cpu())
    assert float(total[N:].abs().sum()) == 0.
    assert bool((pieces[0][:N].abs() >= pieces[1][:N].abs()).all())


def _dot_scale(a, b):
    """sum_k |a[m, k] b[k, n]| (the scale of an fp32 dot product's rounding error)."""
    return a.abs() @ b.abs()


@pytest.mark.parametrize('layout', ['NN', 'NT', 'TT', 'TT32'])
def test_gemm_large_tile_split_bf16_accuracy(layout):
    """The large-tile geometry computes fp32 products as six bf16 piece products (csrc/gemm.hip,
    X6).  Its error against fp64 must stay at the native fp32 level: max |C - C64| / sum|a b| below
    7 x 2^-24 (native f32 MFMA: 3-5 x 2^-24 at these K; a two-piece bf16x3 split would sit near
    2^-17).  Ragged M / N / K exercise the masked tail slabs and clamped tiles."""
    from xtrl_amd import ops
    g = torch.Generator(device='cpu').manual_seed(11)
    M, N, K = 4100, 772, 260
    scale = torch.exp2(torch.randint(-4, 4, (M, 1), generator=g).double())
    a = (torch.randn(M, K, generator=g, dtype=torch.float64) * scale).float()
    b = torch.randn(K, N, generator=g, dtype=torch.float64).float() * 0.1
    ad, bd = a.double(), b.double()
    out = torch.empty(M, N, device=DEV)
    if layout == 'NN':     # A [M][K], B as an nn.Linear weight [N][K]
        ops.gemm_ex(a.to(DEV), b.t().contiguous().to(DEV), 0, 0, M, N, K, out)
        ref, sc = ad @ bd, _dot_scale(ad, bd)
    elif layout == 'NT':   # A [M][K], B [K][N] (input-gradient GEMM)
        ops.gemm_ex(a.to(DEV), b.to(DEV), 0, 1, M, N, K, out)
        ref, sc = ad @ bd, _dot_scale(ad, bd)
    else:                  # weight gradient: dW[N][K'] = dY^T X over M tokens (split over tokens); TT32: a
        # token count that is a multiple of 32 (the native-f32 LDS-DMA ring kernel), ragged feature tiles
        if layout == 'TT32':
            a = a[:4096, :260].contiguous()
            M = 4096
        nk = (260, 1000) if layout == 'TT32' else (256, 1024)
        dy, x = a[:, :nk[0]].contiguous(), torch.randn(M, nk[1], generator=g).float()
        dw = torch.zeros(dy.shape[1], x.shape[1], device=DEV)
        ws = torch.empty(32 << 20, device=DEV)
        ops.wgrad(dy.to(DEV), x.to(DEV), dw, ws, beta=0.)
        out = dw
        ref, sc = dy.double().t() @ x.double(), _dot_scale(dy.double().t(), x.double())
    torch.cuda.synchronize()
    err = ((out.double().cpu() - ref).abs() / sc).max().item()
    assert err < 7 * 2.0 ** -24, f'{layout}: max error {err / 2.0 ** -24:.2f} x 2^-24 of sum |a b|'


@pytest.mark.parametrize('K', [257, 18, 3])
def test_gemm_ragged_extent_padded_rows(K):
    """Operands whose contiguous extent is not a multiple of 4 but whose rows are padded to one
    (the world-model head's d + 1 columns in a d + 4 row) take the float4 path: quads straddling
    the extent read in-bounds padding that the tail mask zeroes (K) or the epilogue discards."""
    from xtrl_amd import ops
    g = torch.Generator(device='cpu').manual_seed(K)
    M, N, ld = 4100, 260, (K + 3) // 4 * 4 + 4
    a = torch.randn(M, ld, generator=g)
    a[:, K:] = 1e30                                   # garbage in the padding columns
    b = torch.randn(K, N, generator=g)
    out = torch.empty(M, N, device=DEV)
    ops.gemm_ex(a.to(DEV)[:, :K], b.to(DEV), 0, 1, M, N, K, out)   # dgrad layout, K ragged
    ad, bd = a[:, :K].double(), b.double()
    torch.cuda.synchronize()
    assert float(((out.double().cpu() - ad @ bd).abs() / _dot_scale(ad, bd)).max()) < 1e-6
    # weight gradient with a ragged output dimension N' = K: dW[K][N] = dY[:, :K]^T X
    x = torch.randn(M, N, generator=g).double()
    dw = torch.zeros(K, N, device=DEV)
    ws = torch.empty(32 << 20, device=DEV)
    ops.wgrad(a.to(DEV)[:, :K], x.float().to(DEV), dw, ws, beta=0.)
    torch.cuda.synchronize()
    assert float(((dw.double().cpu() - ad.t() @ x).abs() / _dot_scale(ad.t(), x)).max()) < 1e-6


@pytest.mark.parametrize('N,K,ldy,ldx,M,bias,m0', [
    (256, 8, 256, 9, 16384, False, 0),     # project_in over [states | reward] rows (tall, S 8)
    (256, 8, 517, 9, 16384, True, 0),      # to_state_embed, dY a column slice of the head input grad
    (18, 256, 18, 260, 7001, True, 0),     # to_pred.2: 2 (S + 1) outputs (wide, two lanes per index)
    (4, 500, 4, 500, 4100, True, 0),       # action-logit shaped (wide, float4-aligned operands)
    (300, 5, 301, 7, 77, True, 3),         # ragged: tall with two indices per lane, a short token range
    (3, 31, 5, 33, 1000, False, 0),        # every extent off the float4 grid
])
def test_wgrad_skinny(N, K, ldy, ldx, M, bias, m0):
    """Skinny weight gradients (k_wgrad_skinny: one side <= 32 wide with the bias column, the other
    <= 512) against fp64: dW accumulates (beta 1) onto its old value, db[n - m0] += sum_m dY[m][n]
    for n >= m0.  Bound: 2^-20 of sum |dy x| (fp32 FMAs over a 64-token span, then the fixed
    reduction tree)."""
    from xtrl_amd import _lib as L
    g = torch.Generator(device='cpu').manual_seed(N * 1000 + K)
    dy = torch.randn(M, ldy, generator=g)
    x = torch.randn(M, ldx, generator=g)
    dw0 = torch.randn(N, K, generator=g)
    db0 = torch.randn(N - m0, generator=g)
    dw, db = dw0.to(DEV), db0.to(DEV)
    ws = torch.empty(32 << 20, device=DEV)
    dyd, xd = dy.to(DEV), x.to(DEV)
    if bias:
        rc = L.lib().xtrl_gemm_wgrad_db(L.ptr(dyd), ldy, L.ptr(xd), ldx, L.ptr(dw), K, M, N, K, 1., L.ptr(ws),
                                        ws.numel(), L.ptr(db), m0, L.stream())
    else:
        rc = L.lib().xtrl_gemm_wgrad(L.ptr(dyd), ldy, L.ptr(xd), ldx, L.ptr(dw), K, M, N, K, 1., L.ptr(ws),
                                     ws.numel(), L.stream())
    L.check(rc, 'gemm_wgrad')
    torch.cuda.synchronize()
    a, b = dy[:, :N].double().t(), x[:, :K].double()
    ref = dw0.double() + a @ b
    err = ((dw.double().cpu() - ref).abs() / (_dot_scale(a, b) + dw0.double().abs())).max().item()
    assert err < 2.0 ** -20, f'dW: {err / 2.0 ** -24:.1f} x 2^-24'
    if bias:
        rb = db0.double() + a.sum(1)[m0:]
        eb = ((db.double().cpu() - rb).abs() / (a.abs().sum(1)[m0:] + db0.double().abs())).max().item()
        assert eb < 2.0 ** -20, f'db: {eb / 2.0 ** -24:.1f} x 2^-24'
    else:
        assert torch.equal(db.cpu(), db0)


# ----------------------------------------------------------------------------------------------
# training attention
# ----------------------------------------------------------------------------------------------


def attn_ref(q, k, v, lens, scale):
    b, H, n, dh = q.shape
    s = torch.einsum('bhid,bhjd->bhij', q, k) * scale
    i = torch.arange(n, device=q.device)
    mask = (i[None, :] <= i[:, None])[None, None] & (i[None, None, None, :] < lens[:, None, None, None])
    s = s.masked_fill(~mask, -torch.finfo(s.dtype).max)
    return torch.einsum('bhij,bhjd->bhid', s.softmax(-1), v)


@pytest.mark.parametrize('b,H,n,dh', [(3, 4, 37, 16), (2, 2, 130, 16), (2, 3, 64, 32), (1, 2, 70, 64), (4, 4, 128, 16),
                                      # more than two key tiles at dh = 32 / 64 (n > 128: the long-episode backward dispatch)
                                      (2, 2, 130, 32), (1, 2, 257, 32), (2, 2, 130, 64), (1, 2, 200, 64)])
def test_attention_fwd_bwd(b, H, n, dh):
    """dh != 16 at n > 128: also through the C ABI with every output filled with NaN before the call — all
    finite afterwards, and within the same bounds."""
    from xtrl_amd import ops
    g = torch.Generator().manual_seed(n + dh)
    q, k, v, do = (torch.randn(b, H, n, dh, generator=g).to(DEV) for _ in range(4))
    lens = torch.randint(1, n + 1, (b,), generator=g).to(torch.int32)
    lens[0] = n
    lens = lens.to(DEV)
    scale = dh ** -0.5
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    ref = attn_ref(qd, kd, vd, lens, scale)
    (ref * do.double()).sum().backward()
    qf, kf, vf = (t.clone().requires_grad_() for t in (q, k, v))
    out = ops.attention(qf, kf, vf, lens, scale)
    (out * do).sum().backward()
    torch.cuda.synchronize()
    tol(out, ref, 1e-5, 1e-5)
    tol(qf.grad, qd.grad, 1e-4, 1e-5)
    tol(kf.grad, kd.grad, 1e-4, 1e-5)
    tol(vf.grad, vd.grad, 1e-4, 1e-5)
    if dh != 16 and n > 128:
        res = AH.attn_lib(q, k, v, lens, do, scale, 0., 'two', 'plain')
        for name, t in res.items():
            assert torch.isfinite(t).all(), name
        tol(res['o'], ref, 1e-5, 1e-5)
        for name, r in (('dq', qd.grad), ('dk', kd.grad), ('dv', vd.grad)):
            tol(res[name], r, 1e-4, 1e-5)


@pytest.mark.parametrize('b,H,n,p', [(3, 4, 37, 0.), (4, 4, 128, 0.), (4, 4, 128, 0.25), (2, 2, 10, 0.25),
                                     (3, 2, 100, 0.1), (5, 4, 65, 0.25)])
def test_attention_fused_backward_matches_two_kernel(b, H, n, p):
    """The fused short-episode backward (k_attn_bwd_fused: one workgroup per (episode, head), P and dS
    formed once per (key tile, query tile) pair) against the dK/dV + dQ kernel pair on the same
    inputs: byte-mode (p = 0.25) and word-mode (p = 0.1) dropout, n not a multiple of 64, ragged
    lens < n.  dV, dK, dQ and D bit-identical."""
    g = torch.Generator().manual_seed(n + int(100 * p))
    q, k, v, do = (torch.randn(b, H, n, 16, generator=g).to(DEV) for _ in range(4))
    lens = torch.randint(1, n + 1, (b,), generator=g).to(torch.int32)
    lens[0] = n
    lens = lens.to(DEV)
    two = AH.attn_lib(q, k, v, lens, do, 0.25, p, 'two', 'plain')
    fus = AH.attn_lib(q, k, v, lens, do, 0.25, p, 'fused', 'plain')
    report = {}
    for name in ('o', 'lse', 'delta', 'dv', 'dk', 'dq'):
        d = (two[name] - fus[name]).abs()
        report[name] = (float(d.max()), int((d > 0).sum()))
    print('fused vs two-kernel (max |diff|, #differing):', report)
    for name in ('o', 'lse', 'delta', 'dv', 'dk', 'dq'):
        assert torch.equal(two[name], fus[name]), (name, report)


@pytest.mark.parametrize('b,H,n,p', [(3, 4, 257, 0.25), (2, 4, 430, 0.25), (3, 2, 500, 0.1), (2, 4, 500, 0.)])
def test_attention_long_backward_dq_folded_matches_two_kernel(b, H, n, p):
    """Long episodes (n > 128, C2's padded widths): the dK / dV kernel with the dQ pass folded in
    (xtrl_attn_bwd_part: dQ from the same P / dS per (key tile, query tile) pair, per-key-tile partials
    for rows with several contributing key tiles, summed in key-tile order) against the dK/dV + dQ
    kernel pair.  dV, dK and D bit-identical; dQ bit-identical on the rows with one contributing key
    tile (query tile 0, episodes of <= 64 steps) and within fp32 summation rounding elsewhere.  Lens
    ragged: one full-length episode, the others random (some <= 64: single-key-tile rows past 64)."""
    from xtrl_amd import _lib as L
    g = torch.Generator().manual_seed(n + int(100 * p))
    q, k, v, do = (torch.randn(b, H, n, 16, generator=g).to(DEV) for _ in range(4))
    lens = torch.randint(1, n + 1, (b,), generator=g).to(torch.int32)
    lens[0] = n
    if b > 2:
        lens[2] = 40
    lens = lens.to(DEV)
    two = AH.attn_lib(q, k, v, lens, do, 0.25, p, 'two', 'plain')
    lib = L.lib()
    nf = int(lib.xtrl_attn_bwd_part_floats(b, H, n, 16))
    assert nf == -(-n // 64) * b * H * n * 16
    part = torch.full((nf,), float('nan'), device=DEV)
    dq, dk, dv = (torch.full_like(q, float('nan')) for _ in range(3))
    delta = torch.empty(b, H, n, device=DEV)
    L.check(lib.xtrl_attn_bwd_part(L.ptr(q), L.ptr(k), L.ptr(v), L.ptr(lens), L.ptr(two['o']), L.ptr(two['lse']),
                                   L.ptr(do), L.ptr(dq), L.ptr(dk), L.ptr(dv), L.ptr(delta), L.ptr(part), nf, b, H, n,
                                   16, 0.25, p, 3, 1, 0, L.stream()), 'attn_bwd_part')
    torch.cuda.synchronize()
    assert torch.equal(dv, two['dv']) and torch.equal(dk, two['dk']) and torch.equal(delta, two['delta'])
    i = torch.arange(n, device=DEV)
    sole = torch.minimum((i // 64)[None, :], ((lens.long() - 1) // 64)[:, None]) == 0     # [b][n]
    sole = sole[:, None, :].expand(b, H, n)
    assert torch.equal(dq[sole], two['dq'][sole])
    assert torch.isfinite(dq).all()
    scale = float(two['dq'].abs().max())
    err = float((dq - two['dq']).abs().max())
    assert err <= 2e-6 * scale, (err, scale)
    assert int((~sole).sum()) > 0


def test_attention_dropout_consistent():
    """Same seed -> same mask; the backward differentiates exactly the forward's dropped product."""
    from xtrl_amd import ops
    g = torch.Generator().manual_seed(5)
    b, H, n, dh = 2, 2, 50, 16
    q, k, v = (torch.randn(b, H, n, dh, generator=g).to(DEV) for _ in range(3))
    lens = torch.tensor([50, 31], dtype=torch.int32, device=DEV)
    o1 = ops.attention(q, k, v, lens, 0.25, 0.25, seed=11, offset=3)
    o2 = ops.attention(q, k, v, lens, 0.25, 0.25, seed=11, offset=3)
    o3 = ops.attention(q, k, v, lens, 0.25, 0.25, seed=12, offset=3)
    assert torch.equal(o1, o2) and not torch.equal(o1, o3)
    # directional derivative check in v (output is linear in v given the mask)
    dv = torch.randn_like(v)
    vv = v.clone().requires_grad_()
    w = torch.randn_like(o1)
    (ops.attention(q, k, vv, lens, 0.25, 0.25, seed=11, offset=3) * w).sum().backward()
    fd = ((ops.attention(q, k, v + dv, lens, 0.25, 0.25, seed=11, offset=3) - o1) * w).sum()
    tol((vv.grad * dv).sum(), fd, 1e-4, 1e-4)
    # expectation: dropout keeps ~75 %
    o0 = ops.attention(q, k, torch.ones_like(v), lens, 0.25, 0.25, seed=7, offset=0)
    assert abs(float(o0.mean()) - 1.0) < 0.05


@pytest.mark.parametrize('p', [0.25, 0.1])
def test_attention_dropout_mask_is_host_philox_stream(p):
    """The kept attention probabilities are exactly the host Philox stream's (oracle/philox.py
    attn_dropout_keep): byte mode at p = 0.25 (one block per 4 query rows x 4 keys 16 apart), word mode
    at p = 0.1 (word (i & 3) of the block of (i >> 2, j)).  Forward against a double reference that
    applies that mask after the softmax, and q / k / v gradients against its autograd (the backward
    kernels draw the same bits, grouped differently: dealt out by a quad transpose in dK / dV).  The
    word-mode mask is also rebuilt here from the raw stream, independently of attn_dropout_keep."""
    from xtrl_amd import ops
    from oracle import philox as P
    g = torch.Generator().manual_seed(9)
    b, H, n, dh = 2, 2, 70, 16
    q, k, v, do = (torch.randn(b, H, n, dh, generator=g) for _ in range(4))
    lens = torch.tensor([70, 45], dtype=torch.int32)
    seed, offset, scale, layer = 1234567, 5, dh ** -0.5, 3
    keep = P.attn_dropout_keep(b, H, n, p, seed, offset, layer)
    if not float(p * 256).is_integer():
        thresh = np.uint32(min(int(p * 2 ** 32), 2 ** 32 - 1))
        i, j = np.arange(n)[:, None], np.arange(n)[None, :]
        for bb in range(b):
            for hh in range(H):
                words = P.philox4x32(i >> 2, j, offset + bb * H + hh, P._c3(P.FIELD_DROPOUT, layer), seed)
                ref_keep = np.choose(np.broadcast_to(i & 3, (n, n)), [np.broadcast_to(w, (n, n)) for w in words]) >= thresh
                assert (keep[bb, hh] == ref_keep).all()
    assert abs(keep.mean() - (1 - p)) < 0.02
    keep_t = torch.from_numpy(keep).double() / (1 - p)
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    s = torch.einsum('bhid,bhjd->bhij', qd, kd) * scale
    ii = torch.arange(n)
    valid = (ii[None, :] <= ii[:, None])[None, None] & (ii[None, None, None, :] < lens.long()[:, None, None, None])
    ref = torch.einsum('bhij,bhjd->bhid', s.masked_fill(~valid, float('-inf')).softmax(-1) * keep_t, vd)
    (ref * do.double()).sum().backward()
    qf, kf, vf = (t.to(DEV).requires_grad_() for t in (q, k, v))
    out = ops.attention(qf, kf, vf, lens.to(DEV), scale, p, seed=seed, offset=offset, sub=layer)
    (out * do.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    tol(out, ref, 1e-5, 1e-5)
    tol(qf.grad, qd.grad, 1e-4, 1e-5)
    tol(kf.grad, kd.grad, 1e-4, 1e-5)
    tol(vf.grad, vd.grad, 1e-4, 1e-5)


@pytest.mark.parametrize('p', [0.25, 0.1])
@pytest.mark.parametrize('dh', [32, 64])
def test_attention_dropout_dh32_64_against_host_keep_bits(dh, p):
    """Dropout at dh = 32 / 64 over three key tiles (n = 130; p = 0.25: byte mode, 0.1: word mode): the forward
    and the q / k / v gradients of ops.attention against the fp64 softmax times the host keep bits
    (oracle.philox.attn_dropout_keep), at the bounds of test_attn_sink_gpu.test_sink_dropout_against_host_keep_bits
    (o 1e-5 + 1e-5, gradients 1e-4 + 1e-5); and through the C ABI with every output NaN-filled before the
    calls: all finite afterwards, within the same bounds."""
    from xtrl_amd import ops
    from oracle import philox as P
    g = torch.Generator().manual_seed(13 + dh)
    b, H, n = 2, 2, 130
    q, k, v, do = (torch.randn(b, H, n, dh, generator=g) for _ in range(4))
    lens = torch.tensor([n, 77], dtype=torch.int32)
    seed, offset, scale, layer = 1234567, 5, dh ** -0.5, 3
    keep = P.attn_dropout_keep(b, H, n, p, seed, offset, layer)
    assert abs(keep.mean() - (1 - p)) < 0.02
    keep_t = torch.from_numpy(keep).double() / (1 - p)
    qd, kd, vd = (t.double().requires_grad_() for t in (q, k, v))
    s = torch.einsum('bhid,bhjd->bhij', qd, kd) * scale
    ii = torch.arange(n)
    valid = (ii[None, :] <= ii[:, None])[None, None] & (ii[None, None, None, :] < lens.long()[:, None, None, None])
    ref = torch.einsum('bhij,bhjd->bhid', s.masked_fill(~valid, float('-inf')).softmax(-1) * keep_t, vd)
    (ref * do.double()).sum().backward()
    qf, kf, vf = (t.to(DEV).requires_grad_() for t in (q, k, v))
    out = ops.attention(qf, kf, vf, lens.to(DEV), scale, p, seed=seed, offset=offset, sub=layer)
    (out * do.to(DEV)).sum().backward()
    res = AH.attn_lib(q.to(DEV), k.to(DEV), v.to(DEV), lens.to(DEV), do.to(DEV), scale, p, 'two', 'plain', seed=seed,
                      offset=offset, sub=layer)
    torch.cuda.synchronize()
    for name, t in list(res.items()) + [('out', out), ('qg', qf.grad), ('kg', kf.grad), ('vg', vf.grad)]:
        assert torch.isfinite(t).all(), name
    for o_, gq, gk, gv in ((out, qf.grad, kf.grad, vf.grad), (res['o'], res['dq'], res['dk'], res['dv'])):
        tol(o_, ref, 1e-5, 1e-5)
        tol(gq, qd.grad, 1e-4, 1e-5)
        tol(gk, kd.grad, 1e-4, 1e-5)
        tol(gv, vd.grad, 1e-4, 1e-5)


@pytest.mark.parametrize('p,layer', [(0.25, 0), (0.1, 0), (0.25, 5), (0.1, 2)])
def test_ff_dropout_mask_is_host_philox_stream(p, layer):
    """FF dropout keep mask (xtrl_ff_dropout_mask, the bits the GELU_DROP GEMM epilogue draws) equals
    the host Philox stream (oracle/philox.py).  p a multiple of 1/256 (byte mode): keep(m, n) = byte
    (m & 3) of word ((m >> 3) & 3) of philox4x32(n, 2 (m >> 5) + ((m >> 2) & 1), off, FIELD_FF_DROPOUT
    sub 2 layer + 1; seed) >= 256 p; else (word mode): word (m & 3) of philox4x32(n, m >> 2, off,
    FIELD_FF_DROPOUT sub 2 layer; seed) >= p 2^32.  Keep fraction ~ 1 - p."""
    from xtrl_amd.train import ff_dropout_mask
    from oracle import philox as P
    M, N, seed, off = 200, 70, 987654321, 11
    got = ff_dropout_mask(M, N, p, seed, off, DEV, layer=layer).cpu().numpy().astype(bool)
    m, n = np.arange(M)[:, None], np.arange(N)[None, :]
    m, n = np.broadcast_to(m, (M, N)), np.broadcast_to(n, (M, N))
    if float(p * 256).is_integer():
        words = P.philox4x32(n, ((m >> 5) << 1) | ((m >> 2) & 1), off, P._c3(P.FIELD_FF_DROPOUT, 2 * layer + 1), seed)
        w = np.choose((m >> 3) & 3, words)
        want = ((w >> (8 * (m & 3))) & 0xFF) >= int(p * 256)
    else:
        words = P.philox4x32(n, m >> 2, off, P._c3(P.FIELD_FF_DROPOUT, 2 * layer), seed)
        want = np.choose(m & 3, words) >= np.uint32(min(int(p * 2 ** 32), 2 ** 32 - 1))
    np.testing.assert_array_equal(got, want)
    assert abs(got.mean() - (1 - p)) < 0.02


# ----------------------------------------------------------------------------------------------
# rollout (decode step, sampling, synthetic Sim) vs the oracle's batch-1 reference loop
# ----------------------------------------------------------------------------------------------


def make_learner(S=8, A=4, depth=2, gates=True, evo=False, cont=False, T=12, episodes=8, batch=4, seed=3,
                 hazard=3, mode='lander', dim=48, reward_dropout=0.5, gene_dim=8, agent_extra=None, fractal_levels=None,
                 ff_mult=4, genes=3, shard_by_gene=False, ff_no_bias=False, ff_glu=False, wm_extra=None, squash=True,
                 heads=4, dim_head=16, device=None, window=None, window_key=True, kv_heads=None, num_mem_kv=0,
                 add_zero_kv=False, use_graph=False, with_oracle=True):
    """``heads``, ``dim_head``: the attention geometry (world_model heads / attn_dim_head and the oracle's
    LearnerConfig fields).  ``device``: 'cpu' builds the Learner without a GPU (the same initial weights:
    test_geometry_cpu settles the cases' inputs from the oracle alone).
    ``window``, ``num_mem_kv``, ``add_zero_kv``: world_model attn_max_attend_past (``window_key`` False: the key
    is left out), attn_num_mem_kv and attn_add_zero_kv; ``kv_heads``: 1 goes in as world_model['attn_one_kv_head'],
    any other count as agent_kwargs kv_heads, so both ways in are run.  These go to the Learner alone: the oracle
    takes them from the Attention the caller has patched over the frozen one (attn_harness.rollout_and_learn).
    ``with_oracle`` False: a device-only test, the third result is None.
    ``fractal_levels``: the causal fractal policy body (policy_body='fractal') on both sides.
    ``squash``: squash_continuous of the Learner / squash of the oracle (tanh-squashed continuous actions).
    ``ff_mult``: the feed-forward width through world_model['ff_mult'] (x-transformers' FeedForward mult).
    ``wm_extra``: further world_model options (attn_qk_norm, attn_qk_norm_scale, rotary_xpos,
    rotary_xpos_scale_base), given to the oracle's Decoder as well."""
    from xtrl_amd import Learner, SynthVecSim
    torch.manual_seed(seed)
    factory = None
    if fractal_levels is not None:
        assert not gates
        agent_extra = dict(agent_extra or {}, policy_body='fractal', fractal_levels=fractal_levels)
        factory = lambda mc: FR.OracleFractalPolicy(mc, fractal_levels)   # noqa: E731
    wm = dict(attn_dim_head=dim_head, heads=heads, depth=depth)
    if ff_mult != 4:
        wm['ff_mult'] = ff_mult
    if ff_no_bias:
        wm['ff_no_bias'] = True
    if ff_glu:
        wm['ff_glu'] = True
    if gates:
        wm.update(attn_gate_values=True, add_value_residual=True, learned_value_residual_mix=True)
    wm.update(wm_extra or {}, attn_num_mem_kv=num_mem_kv, attn_add_zero_kv=add_zero_kv)
    if window_key:
        wm['attn_max_attend_past'] = window
    if kv_heads == 1:
        wm['attn_one_kv_head'] = True
    elif kv_heads is not None:
        agent_extra = dict(agent_extra or {}, kv_heads=kv_heads)
    names = dict(attn_qk_norm='qk_norm', attn_qk_norm_scale='qk_norm_scale', rotary_xpos='rotary_xpos',
                 rotary_xpos_scale_base='xpos_scale_base', use_rmsnorm='rms_norm')
    oracle_extra = {names[k]: v for k, v in (wm_extra or {}).items()}
    gp = dict(dim=gene_dim, num_genes_per_island=genes, num_selected=2, tournament_size=2)
    learner = Learner(state_dim=S, num_actions=A, reward_range=(-2., 2.), world_model=wm, max_timesteps=T,
                      batch_size=batch, num_episodes_per_update=episodes, evolutionary=evo, evolve_every=1,
                      evolve_after_step=0, latent_gene_pool=gp, continuous_actions=cont, squash_continuous=squash,
                      continuous_actions_clamp=(-1., 1.) if cont else None,
                      agent_kwargs=dict(dropout=0., seed=seed, hidden_dim=dim, reward_dropout=reward_dropout,
                                        **(agent_extra or {})),
                      use_graph=use_graph, shard_by_gene=shard_by_gene,
                      **(dict(accelerate_kwargs=dict(device=device)) if device is not None else {}))
    with torch.no_grad():   # non-trivial gate / mix weights (their init is constant)
        g = torch.Generator().manual_seed(seed + 1)
        for name, p in learner.agent.model.named_parameters():
            if 'to_v_gate' in name or 'to_value_residual_mix' in name:
                p.copy_((torch.randn(p.shape, generator=g) * 0.3).to(p.device))
        learner.agent.ema_flat.copy_(learner.agent.flat.flat)
    env = SynthVecSim(S, A, mode, hazard_log2=hazard)
    if not with_oracle:
        return learner, env, None
    c = R.LearnerConfig(S, A, (-2., 2.), dim=dim, depth=depth, heads=heads, dim_head=dim_head, gate_values=gates,
                        value_residual=gates, learned_mix=gates, continuous=cont, squash=squash,
                        clamp=(-1., 1.) if cont else None, evolutionary=evo, evolve_every=1, evolve_after_step=0, gene_pool=gp, max_timesteps=T, batch_size=batch,
                        num_episodes_per_update=episodes, sim_mode=mode, hazard_log2=hazard, seed=seed,
                        reward_dropout=reward_dropout, ff_mult=ff_mult, ff_no_bias=ff_no_bias, ff_glu=ff_glu,
                        **oracle_extra)
    sd = {k: v.detach().cpu() for k, v in learner.agent.model.state_dict().items()}
    genes = learner.agent.gene_pool.genes.clone() if evo else None
    oracle = R.OracleLearner(c, init_state_dict=sd, genes=genes, model_factory=factory)
    return learner, env, oracle


@contextlib.contextmanager
def _loss_kinks(force=None):
    """While the oracle computes a minibatch loss: the elements sitting on a kink of the losses —
    a PPO ratio within 1e-5 of 1 -/+ eps_clip (xtrl.py:413-444: there min(r A, clip(r) A) has the
    one-sided slopes A and 0) and a critic token whose value lies within 1e-5 of the return or of
    v_old -/+ value_clip (xtrl.py:446-477: the clipped-value loss switches between 0 and the HL-Gauss
    term).  The two implementations' last bits may put such an element on different sides.
    ``force``: dict(actor=[k...], critic=[k...]), one k in {0, 1} per kinked element in the order
    found: the element takes that branch (actor: slope k A at the same value; critic: k times the
    HL-Gauss term) — so the GPU gradient can be matched against every branch assignment of the
    kinked elements instead of skipping the minibatch's gradients."""
    out = {'distance': float('inf'), 'n_actor': 0, 'n_critic': 0}
    orig_a, orig_c = R.actor_loss, R.critic_loss

    def actor(cfg, hl, raw, actions, old_lp, returns, old_values, mask):
        natural = orig_a(cfg, hl, raw, actions, old_lp, returns, old_values, mask)
        lp = R.continuous_log_prob(raw, actions, cfg.squash) if cfg.continuous else R.discrete_log_prob(raw, actions)
        r = (lp - old_lp).exp()
        m = mask.reshape(*mask.shape, *((1,) * (r.ndim - mask.ndim))).expand_as(r).bool()
        d = torch.minimum((r - (1 - cfg.eps_clip)).abs(), (r - (1 + cfg.eps_clip)).abs()).detach()
        kink = (d < 1e-5) & m
        if m.any():
            out['distance'] = min(out['distance'], float(d[m].min()))
            out['ratio'] = float(d[m].min())
        out['n_actor'] = int(kink.sum())
        if force is None or not kink.any():
            return natural
        # R.actor_loss restated with the kinked elements' surrogate forced to slope k A (same value)
        if cfg.continuous:
            ent = -lp if cfg.squash else R.continuous_entropy(raw)
        else:
            ent = R.discrete_entropy(raw)
        clipped = r.clamp(1 - cfg.eps_clip, 1 + cfg.eps_clip)
        adv = returns - hl(old_values).detach()
        if cfg.normalize_advantages:
            adv = R.normalize(adv, mask)
        adv = adv.reshape(*adv.shape, *((1,) * (r.ndim - adv.ndim)))
        surr = torch.min(r * adv, clipped * adv)
        k = torch.zeros_like(r)
        k[kink] = torch.as_tensor(force['actor'], dtype=r.dtype)
        surr = torch.where(kink, surr.detach() + (r - r.detach()) * adv * k, surr)
        loss = -surr - cfg.entropy_weight * ent
        return loss.reshape(*loss.shape[:2], -1).sum(-1)

    def critic(cfg, hl, values, returns, old_values):
        natural = orig_c(cfg, hl, values, returns, old_values)
        v, v_old = hl(values).detach(), hl(old_values).detach()
        d = torch.stack([(v - returns).abs(), (v - (v_old - cfg.value_clip)).abs(),
                         (v - (v_old + cfg.value_clip)).abs()]).min(0).values
        out['distance'] = min(out['distance'], float(d.min()))
        out['value'] = float(d.min())
        kink = d < 1e-5
        out['n_critic'] = int(kink.sum())
        if force is None or not kink.any():
            return natural
        clip = cfg.value_clip
        full = torch.min(hl(values, returns), hl(values, returns.clamp(-clip, clip)))
        k = torch.zeros(natural.shape, dtype=natural.dtype)
        k[kink] = torch.as_tensor(force['critic'], dtype=natural.dtype)
        return torch.where(kink, k * full, natural)

    R.actor_loss, R.critic_loss = actor, critic
    try:
        yield out
    finally:
        R.actor_loss, R.critic_loss = orig_a, orig_c


def compare_rollout(traj, lens, episodes, cont=False, rows=None, prefix=None):
    """Device trajectory rows vs the oracle's episodes (rows[i] <-> episodes[i]; default row i).
    ``prefix``: the oracle ran at most ``prefix`` steps — compare the first min(len, prefix) steps."""
    lens = lens.cpu().numpy()
    if rows is not None:
        traj = {k: (v[torch.as_tensor(rows, device=v.device)] if v is not None else None) for k, v in traj.items()}
        lens = lens[np.asarray(rows)]
    for i, ep in enumerate(episodes):
        n = ep['len']
        if prefix is not None:
            assert min(int(lens[i]), prefix) == n, (i, lens[i], n)
            traj_i = {k: (v[i:i + 1, :n] if v is not None else None) for k, v in traj.items()}
            compare_rollout(traj_i, torch.tensor([n]), [ep], cont)
            continue
        assert lens[i] == n, (i, lens[i], n)
        mem = ep['mem']
        states = torch.stack([m[0] for m in mem])
        np.testing.assert_array_equal(traj['states'][i, :n].cpu().numpy(), states.numpy())
        if cont:
            tol(traj['actions_f'][i, :n], torch.stack([m[1] for m in mem]), 1e-4, 1e-5)
            tol(traj['logp'][i, :n], torch.stack([m[2] for m in mem]), 1e-4, 1e-4)
        else:
            np.testing.assert_array_equal(traj['actions'][i, :n].cpu().numpy(), np.array([int(m[1]) for m in mem]))
            tol(traj['logp'][i, :n], torch.stack([m[2] for m in mem]), 1e-4, 1e-5)
        rw = torch.stack([m[3] for m in mem])
        if not cont:
            np.testing.assert_array_equal(traj['rewards'][i, :n].cpu().numpy(), rw.numpy())
        np.testing.assert_array_equal(traj['bounds'][i, :n].cpu().numpy().astype(bool),
                                      torch.stack([m[4] for m in mem]).numpy())
        tol(traj['values'][i, :n], torch.stack([m[5] for m in mem]), 1e-4, 1e-4)
        # padding past the episode is zero, as pad_sequence leaves it (xtrl.py:837)
        assert float(traj['values'][i, n:].abs().sum()) == 0.


@pytest.fixture(params=['rows', 'multi'])
def decode_path(request, monkeypatch):
    """The decode step the rollout takes at these sizes (d <= 128, few rows): the row-resident step
    (xtrl_decode_step_rows, one workgroup per live row) or the multi-kernel step (XTRL_DECODE_ROWS=0)."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', '1' if request.param == 'rows' else '0')
    return request.param


@pytest.mark.parametrize('depth,gates,evo', [(1, False, False), (2, True, False), (2, True, True), (3, True, True)])
def test_rollout_matches_oracle(depth, gates, evo, decode_path):
    learner, env, oracle = make_learner(depth=depth, gates=gates, evo=evo)
    assert (learner._engine_for(env, 12).rows_max > 0) == (decode_path == 'rows')
    traj, lens, _, cum = learner.rollout_device(env, 0, 12)
    torch.cuda.synchronize()
    episodes, fitness = oracle.rollout(0)
    compare_rollout(traj, lens, episodes)
    if evo:
        tol(learner.fitness(cum, torch.tensor([g for _, g in learner.episode_genes])), fitness, 1e-5, 1e-5)


@pytest.mark.parametrize('variant', ['mlp_f32_images', 'heads_one_launch', 'two_gemm_ff'])
def test_rollout_opt_in_decode_variants_match_oracle(variant, monkeypatch):
    """The opt-in decode kernels against the oracle on the multi-kernel step (d = 128, EPO latents in
    the heads' input: in_dim = 384): the one-launch feed-forward on fp32 fragment images
    (XTRL_MLP_IMG=f32, split per fragment in the kernel), the one-launch heads (XTRL_DECODE_HEADS=1:
    hidden layer + SiLU + last Linear + sampling, k_heads_mlp) and the two-GEMM feed-forward
    (XTRL_DECODE_MLP=0)."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', '0')
    monkeypatch.setenv({'mlp_f32_images': 'XTRL_MLP_IMG', 'heads_one_launch': 'XTRL_DECODE_HEADS',
                        'two_gemm_ff': 'XTRL_DECODE_MLP'}[variant],
                       {'mlp_f32_images': 'f32', 'heads_one_launch': '1', 'two_gemm_ff': '0'}[variant])
    learner, env, oracle = make_learner(depth=2, gates=True, evo=True, dim=128, episodes=12)
    eng = learner._engine_for(env, 12)
    if variant == 'mlp_f32_images':
        assert 'w_ff1f' in eng.wl[0] and 'w_ff1x' not in eng.wl[0]
    if variant == 'heads_one_launch':
        assert eng.desc.heads_part
    traj, lens, _, cum = learner.rollout_device(env, 0, 12)
    torch.cuda.synchronize()
    episodes, fitness = oracle.rollout(0)
    compare_rollout(traj, lens, episodes)


@pytest.mark.parametrize('ff', [4, 2])
def test_rollout_d256_matches_oracle(ff):
    """The C3 width (d = 256, 4 x 16 heads; the decode embedding kernel's fused layer-0 pre-norm, the
    decode GEMM geometries of that shape) reproduces the oracle's batch-1 rollout; ff = 2: the one-launch
    feed-forward kernel at world_model['ff_mult'] = 2 (4 hidden-unit workgroups per row panel instead of 8)."""
    learner, env, oracle = make_learner(depth=2, gates=True, dim=256, episodes=20, ff_mult=ff)
    traj, lens, _, _ = learner.rollout_device(env, 0, 12)
    torch.cuda.synchronize()
    episodes, _ = oracle.rollout(0)
    compare_rollout(traj, lens, episodes)


def test_rollout_continuous_matches_oracle(decode_path):
    learner, env, oracle = make_learner(cont=True, gates=True)
    traj, lens, _, _ = learner.rollout_device(env, 0, 12)
    torch.cuda.synchronize()
    episodes, _ = oracle.rollout(0)
    compare_rollout(traj, lens, episodes, cont=True)


@pytest.mark.parametrize('dim', [48, 256])
def test_rollout_graph_replay_equals_eager(dim, decode_path):
    """dim 256: the one-launch feed-forward kernel (its per-panel arrival counters reset in-graph).
    dim 48 (rows): the row-resident step's graphs."""
    learner, env, _ = make_learner(depth=2, T=16, episodes=40, dim=dim)
    traj, lens, _, _ = learner.rollout_device(env, 0, 16)
    eager = {k: v.clone() for k, v in traj.items() if v is not None}
    learner.use_graph = True
    learner._engine = None
    for update in (0, 0):   # capture, then replay
        traj, lens2, _, _ = learner.rollout_device(env, update, 16)
    torch.cuda.synchronize()
    for k, v in eager.items():
        assert torch.equal(v, traj[k]), k


def test_row_step_oversubscribed_grid_matches_multi_kernel_and_oracle(monkeypatch):
    """The row-resident step with far more workgroups than the chip holds at once (2048 rows, one
    workgroup each, from step 0), so most workgroups start after others have already stepped and
    ended their rows within the same launch: every workgroup must still rank the rows live at the
    step's start (the alive byte's ended-at-step marker; a row skipped or stepped twice would shift
    every later row).  Lengths, terminations and the Sim's states (independent of the actions) are
    bit-identical to the multi-kernel step for all 2048 rows; actions / log-probs / values match the
    oracle's batch-1 loop for every row's first 4 steps and 16 whole episodes."""
    E, T = 2048, 12
    learner, env, oracle = make_learner(depth=2, T=T, episodes=E, batch=64, hazard=2)
    eng = learner._engine_for(env, T)
    assert eng.rows_max > 0
    monkeypatch.setattr(eng, 'rows_max', E)   # every step row-resident, grid = E workgroups
    traj, lens, _, _ = learner.rollout_device(env, 0, T)
    torch.cuda.synchronize()
    rows_out = {k: v.clone() for k, v in traj.items() if v is not None}
    rows_lens = lens.clone()
    # the ended-at-step markers (3 / 4) of the last row step are cleared at the rollout's end
    assert set(eng.alive.cpu().tolist()) <= {0, 1}
    monkeypatch.setattr(eng, 'rows_max', 0)   # the multi-kernel step
    traj, lens, _, _ = learner.rollout_device(env, 0, T)
    torch.cuda.synchronize()
    assert torch.equal(rows_lens, lens)
    for k in ('states', 'bounds'):
        assert torch.equal(rows_out[k], traj[k]), k
    assert int((lens < T).sum()) > E // 2          # most episodes ended inside a row-step launch
    episodes, _ = oracle.rollout(0, max_timesteps=4)
    compare_rollout(rows_out, rows_lens, episodes, prefix=4)
    longest = torch.argsort(rows_lens.cpu(), descending=True, stable=True)[:8].tolist()
    rows = sorted(set(longest + [int(x) for x in torch.linspace(7, E - 9, 8).round().long().tolist()]))
    episodes, _ = oracle.rollout(0, slots=rows)
    compare_rollout(rows_out, rows_lens, episodes, rows=rows)


# ---- the causal fractal policy body (oracle/fractal_ref.OracleFractalPolicy) ------------


@pytest.mark.parametrize('levels,evo,cont,dim', [(1, False, False, 48), (2, False, False, 48), (3, True, False, 64),
                                                 (2, False, True, 48), (2, True, False, 256)])
def test_fractal_rollout_matches_oracle(levels, evo, cont, dim):
    """xtrl_fractal_decode_step (per level: K/V cache, running level means, per-step global state)
    reproduces the oracle's batch-1 streaming rollout: identical actions and states, logp / values
    within 1e-4."""
    learner, env, oracle = make_learner(depth=levels, gates=False, evo=evo, cont=cont, dim=dim, fractal_levels=levels,
                                        episodes=12 if dim == 256 else 8)
    traj, lens, _, cum = learner.rollout_device(env, 0, 12)
    torch.cuda.synchronize()
    episodes, fitness = oracle.rollout(0)
    compare_rollout(traj, lens, episodes, cont=cont)
    if evo:
        tol(learner.fitness(cum, torch.tensor([g for _, g in learner.episode_genes])), fitness, 1e-5, 1e-5)


def test_fractal_rollout_graph_replay_equals_eager():
    learner, env, _ = make_learner(depth=2, gates=False, T=16, episodes=16, fractal_levels=2)
    traj, _, _, _ = learner.rollout_device(env, 0, 16)
    eager = {k: v.clone() for k, v in traj.items() if v is not None}
    learner.use_graph = True
    learner._engine = None
    for update in (0, 0):   # capture, then replay
        traj, _, _, _ = learner.rollout_device(env, update, 16)
    torch.cuda.synchronize()
    for k, v in eager.items():
        assert torch.equal(v, traj[k]), k


def test_fractal_forward_train_ragged_matches_oracle():
    """The learn-step forward (cumulative-mean form, flash attention with key padding) equals the
    oracle's streaming form position by position on ragged episodes; gradients of a random
    functional of every output agree within 1e-4 of the gradient scale."""
    learner, _, oracle = make_learner(depth=3, gates=False, dim=64, fractal_levels=3, evo=True)
    agent = learner.agent
    model, om = agent.model, oracle.model
    g = torch.Generator().manual_seed(11)
    b, n, S = 5, 23, 8
    state = torch.randn(b, n, S, generator=g)
    lens = torch.tensor([23, 1, 7, 16, 22], dtype=torch.int32)
    nxt = torch.randint(-1, 4, (b, n), generator=g)
    lat = F.normalize(torch.randn(b, 8, generator=g), dim=-1)
    model.eval()
    om.eval()
    agent.flat.zero_grad()
    outs = model.forward_train(state.cuda(), None, None, nxt.cuda(), lat.cuda(), lens.cuda())
    mask = (torch.arange(n)[None] < lens[:, None].long())
    ref = om(state, next_actions=nxt, latent_gene=lat, mask=mask)
    for name, a, r in zip(('raw_actions', 'values'), outs[:2], ref[:2]):
        a = a.detach().cpu()[mask]
        r = r.detach()[mask]
        assert float((a - r).abs().max()) <= 1e-4 * float(r.abs().max()) + 1e-6, name
    w = [torch.randn(o.shape, generator=g) * mask.reshape(b, n, *([1] * (o.ndim - 2))) for o in outs]
    sum((o * wi.cuda()).sum() for o, wi in zip(outs, w)).backward()
    # oracle side: the same functional of (raw_actions, values, pred_raw, done_logit)
    om.zero_grad()
    ref = om(state, next_actions=nxt, latent_gene=lat, mask=mask)
    (sum((o * wi).sum() for o, wi in zip((ref[0], ref[1]) + _oracle_wm_raw(om, state, nxt, mask), w))).backward()
    gpu_g = dict(zip(agent.flat.names, (p.grad.detach().cpu() for p in agent.flat.params)))
    worst, bad = grad_mismatches(gpu_g, om.named_parameters())
    assert not bad, bad


def _oracle_wm_raw(om, state, nxt, mask):
    """(pred_raw, done_logit) of the oracle fractal policy — the world-model heads before the
    mean / variance split and the sigmoid (forward_train's outputs 3 and 4)."""
    cache = dict(t=0, k=[None] * om.levels, v=[None] * om.levels, sums=[None] * om.levels)
    feats = torch.stack([om._step(state[:, i], cache, mask[:, :i + 1]) for i in range(state.shape[1])], dim=1)
    ewa = torch.cat((feats, om.embed_actions(nxt)), dim=-1)
    return om.to_pred(ewa), om.to_pred_done(ewa)[..., 0]


# ----------------------------------------------------------------------------------------------
# GAE + HL-Gauss value decode
# ----------------------------------------------------------------------------------------------


def test_hlgauss_gae_matches_oracle():
    from xtrl_amd import ops
    g = torch.Generator().manual_seed(9)
    E, T, B, n = 33, 40, 100, 37
    logits = torch.randn(E, T, B, generator=g)
    rewards = torch.randn(E, T, generator=g)
    bounds = (torch.rand(E, T, generator=g) < 0.1).to(torch.uint8)
    hl = tp.HLGaussLoss(-2., 2., B, clamp_to_range=True)
    vals, rets = ops.hlgauss_gae(logits.to(DEV), rewards.to(DEV), bounds.to(DEV), hl.centers.to(DEV), n, 0.99, 0.95)
    torch.cuda.synchronize()
    v_ref = hl(logits[:, :n])
    r_ref = R.calc_gae(rewards[:, :n], v_ref, (bounds[:, :n] == 0).float(), 0.99, 0.95)
    tol(vals, v_ref, 1e-5, 1e-6)
    tol(rets, r_ref, 1e-5, 1e-5)


# ----------------------------------------------------------------------------------------------
# fused loss forward / backward vs autograd through the oracle's loss restatement
# ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('cont,hl_mean', [(False, True), (True, True), (False, False)])
def test_fused_loss_matches_oracle(cont, hl_mean):
    from xtrl_amd import ops
    g = torch.Generator().manual_seed(21 + cont)
    b, n, A, B, S1 = 5, 23, 3, 100, 6
    lens = torch.tensor([23, 17, 1, 9, 22], dtype=torch.int32)
    raw = torch.randn(b, n, 2 * A if cont else A, generator=g)
    values = torch.randn(b, n, B, generator=g)
    pred_raw = torch.randn(b, n, 2 * S1, generator=g)
    done_logit = torch.randn(b, n, generator=g) * 2
    if cont:
        actions = torch.rand(b, n, A, generator=g) * 1.8 - 0.9
        old_lp = torch.randn(b, n, A, generator=g) * 0.3 - 1.
    else:
        actions = torch.randint(0, A, (b, n), generator=g)
        old_lp = torch.log(torch.rand(b, n, generator=g) * 0.8 + 0.1)
    returns = torch.randn(b, n, generator=g)
    old_values = torch.randn(b, n, B, generator=g)
    dones = torch.rand(b, n, generator=g) < 0.2
    real = torch.randn(b, n, S1, generator=g)
    lo, hi = -2., 2.
    cfg = R.ModelConfig(S1 - 1, A, 32, continuous=cont, squash=True, reward_range=(lo, hi))
    hl = tp.HLGaussLoss(lo, hi, B, clamp_to_range=True)
    hl_prev = tp.HLGaussLoss.default_reduction
    tp.HLGaussLoss.default_reduction = 'mean' if hl_mean else 'none'
    try:
        ins = [t.clone().double().requires_grad_() for t in (raw, values, pred_raw, done_logit)]
        r_, v_, p_, d_ = ins
        mask = torch.arange(n)[None] < lens[:, None]
        mean, lv = p_.reshape(b, n, S1, 2).unbind(-1)
        var = (torch.tanh(lv / 3.) * 3.).exp()
        wm = R.autoregressive_loss(torch.stack((mean, var)), real.double())[mask[:, :-1]]
        dl = R.done_loss(torch.sigmoid(d_), dones)[mask]
        hld = tp.HLGaussLoss(lo, hi, B, clamp_to_range=True).double()
        al = R.actor_loss(cfg, hld, r_, actions.double() if cont else actions, old_lp.double(), returns.double(),
                          old_values.double(), mask)
        cl = R.critic_loss(cfg, hld, v_, returns.double(), old_values.double())
        ac = (al * 0.5 + cl * 1.)[mask]
        ref = ac.mean() + (wm.mean() + dl.mean()) * 0.7
        ref.backward()
    finally:
        tp.HLGaussLoss.default_reduction = hl_prev
    K = ops.LossConsts(actions=(actions.float() if cont else actions.to(torch.int32)).to(DEV).contiguous(),
                       old_logp=old_lp.to(DEV), returns=returns.to(DEV), old_values=old_values.to(DEV),
                       dones=dones.to(torch.uint8).to(DEV), lens=lens.to(DEV), real=real.to(DEV),
                       support=hl.support.to(DEV), centers=hl.centers.to(DEV), continuous=cont, squash=True,
                       hl_mean=hl_mean, eps_clip=0.2, value_clip=0.4, entropy_weight=0.01, w_actor=0.5, w_critic=1.,
                       w_autoreg=0.7, lo=lo, hi=hi, sigma=float(hl.sigma))
    outs = [t.clone().to(DEV).requires_grad_() for t in (raw, values, pred_raw, done_logit)]
    loss, stats = ops.fused_loss(*outs, K)
    loss.backward()
    torch.cuda.synchronize()
    tol(loss, ref, 1e-5, 1e-6)
    tol(stats[1], al.mean(), 1e-5, 1e-6)
    tol(stats[2], cl.mean(), 1e-5, 1e-6)
    tol(stats[3], wm.mean(), 1e-5, 1e-6)
    tol(stats[4], dl.mean(), 1e-5, 1e-6)
    for ours, theirs in zip(outs, ins):
        tol(ours.grad, theirs.grad, 1e-4, 1e-6)


# ----------------------------------------------------------------------------------------------
# optimiser path vs the restated AdoptAtan2 / clip_grad_norm_
# ----------------------------------------------------------------------------------------------


def test_adopt_atan2_and_clip_match_oracle():
    from xtrl_amd import ops
    g = torch.Generator().manual_seed(4)
    shapes = [(7, 5), (13,), (3, 4, 2), (1,)]
    params = [torch.randn(s, generator=g) for s in shapes]
    ref_params = [torch.nn.Parameter(p.clone()) for p in params]
    opt = tp.AdoptAtan2(ref_params, lr=8e-4, betas=(0.9, 0.99), regen_reg_rate=1e-4, cautious_factor=0.1)
    sizes = [p.numel() for p in params]
    offs = np.cumsum([0] + sizes)
    flat = torch.cat([p.reshape(-1) for p in params]).to(DEV)
    m, v, pinit = (torch.zeros_like(flat) for _ in range(3))
    seg = torch.tensor(offs, dtype=torch.int64, device=DEV)
    seg_ws = torch.zeros(len(shapes), dtype=torch.int32, device=DEV)
    ws = torch.zeros(512, dtype=torch.float64, device=DEV)
    clip = torch.zeros(2, device=DEV)
    for step in range(4):
        grads = [torch.randn(s, generator=g) * (3. if step == 2 else 0.05) for s in shapes]
        for p, gr in zip(ref_params, grads):
            p.grad = gr.clone()
        torch.nn.utils.clip_grad_norm_(ref_params, 0.5)
        opt.step()
        gflat = torch.cat([gr.reshape(-1) for gr in grads]).to(DEV)
        ops.grad_norm(gflat, 0.5, ws, clip)
        ops.adopt_atan2(flat, gflat, m, v, pinit, seg, ops.adopt_chunks(seg, chunk=8), seg_ws, clip, lr=8e-4, init_lr=8e-4, betas=(0.9, 0.99),
                        a=1.27, b=1., weight_decay=0., regen_rate=1e-4, cautious=0.1, first_step=step == 0)
        torch.cuda.synchronize()
        tol(flat, torch.cat([p.detach().reshape(-1) for p in ref_params]), 1e-5, 1e-6)


# ----------------------------------------------------------------------------------------------
# end to end: rollout + learn (two updates) vs the oracle Learner
# ----------------------------------------------------------------------------------------------


def gpu_episodes(traj, lens, genes, cont=False):
    """The device trajectory as the reference's per-episode Memory lists (xtrl.py:67-81)."""
    out = []
    lens_c = lens.cpu()
    for i, gene in enumerate(genes):
        n = int(lens_c[i])
        acts = traj['actions_f'][i, :n].cpu() if cont else traj['actions'][i, :n].cpu().long()
        mem = list(zip(traj['states'][i, :n].cpu(), acts, traj['logp'][i, :n].cpu(), traj['rewards'][i, :n].cpu(),
                       traj['bounds'][i, :n].cpu().bool(), traj['values'][i, :n].cpu()))
        out.append(dict(mem=mem, len=n, gene=gene))
    return out


def oracle_minibatch_tensors(episodes):
    """Agent.learn's data preparation (xtrl.py:822-852) on the oracle side."""
    from torch.nn.utils.rnn import pad_sequence
    cols = list(zip(*[tuple(map(torch.stack, zip(*ep['mem']))) for ep in episodes]))
    states, actions, old_lp, rewards, bounds, values = (pad_sequence(list(col), batch_first=True) for col in cols)
    lens = torch.tensor([ep['len'] for ep in episodes])
    genes = torch.tensor([ep['gene'] for ep in episodes])
    return states, actions, old_lp, rewards, bounds, values, lens, genes


@pytest.mark.parametrize('evo,gates,cont,frac,ff', [(False, False, False, None, 4), (True, True, False, None, 4),
                                                     (False, True, True, None, 4), (False, False, False, 2, 4),
                                                     (True, False, True, 3, 4), (False, True, False, None, 2),
                                                     (False, True, False, None, 3), (False, False, False, 2, 3)])
def test_ppo_loss_and_grads_identical_weights(evo, gates, cont, frac, ff):
    """BASELINE metric 'PPO loss delta vs CPU ref': for every minibatch of two learning updates the
    oracle recomputes loss and gradients with the GPU's current weights / RSNorm / genes on the
    same minibatch; loss within 1e-4 relative, every gradient tensor within 1e-4 of its OWN largest
    gradient (+ 1e-7); a minibatch with elements on a loss kink matches for some branch of each.
    ff != 4: world_model['ff_mult'] (feed-forward width 2d / 3d; 3d = 144 is not a multiple of the
    decode feed-forward kernel's column tile, so the rollout takes its two-GEMM path)."""
    learner, env, oracle = make_learner(depth=2, gates=gates, evo=evo, cont=cont, T=10, episodes=6, batch=2, seed=5,
                                        hazard=2, fractal_levels=frac, ff_mult=ff)
    agent = learner.agent
    c = oracle.c
    worst = [0.]
    kinked = []
    for u in range(2):
        traj, lens, genes, cum = learner.rollout_device(env, u, 10)
        episodes, fitness = oracle.rollout(u)      # oracle rollout under its own (drifting) weights
        gpu_eps = []
        lens_c = lens.cpu()
        for i in range(len(episodes)):          # rebuild the episodes from the GPU trajectory
            n = int(lens_c[i])
            acts = traj['actions_f'][i, :n].cpu() if cont else traj['actions'][i, :n].cpu().long()
            mem = list(zip(traj['states'][i, :n].cpu(), acts, traj['logp'][i, :n].cpu(), traj['rewards'][i, :n].cpu(),
                           traj['bounds'][i, :n].cpu().bool(), traj['values'][i, :n].cpu()))
            gpu_eps.append(dict(mem=mem, len=n, gene=episodes[i]['gene']))
        states, actions, old_lp, rewards, bounds, values, elens, egenes = oracle_minibatch_tensors(gpu_eps)
        returns = R.calc_gae(rewards, oracle.model.hl(values), (~bounds).float(), c.gamma, c.lam)
        rs = R.RSNormState(c.state_dim + 1)
        rs.mean, rs.var = agent.rs_mean.cpu().clone(), agent.rs_var.cpu().clone()
        fit = learner.fitness(cum, genes)

        def probe(epoch, mbi, idx, loss, stats):
            idx = idx.cpu()
            sd = {k: v.detach().cpu() for k, v in agent.model.state_dict().items()}
            oracle.model.load_state_dict(sd)
            oracle.model.train()
            oracle.model.zero_grad()
            mb = R.Minibatch(states[idx], actions[idx], rewards[idx], old_lp[idx], returns[idx], values[idx], bounds[idx],
                             egenes[idx], elens[idx])
            latent = R.l2norm(agent.gene_pool.genes[mb.gene_ids]) if evo else None
            keep = R.reward_coin(c.seed, u, epoch, mbi, c.reward_dropout)
            with _loss_kinks() as kinks:
                ref_loss, _, _, _ = R.minibatch_loss(oracle.model, rs, mb, latent, c.weights, keep)
            ref_loss.backward()
            l_gpu, l_ref = float(loss.detach()), float(ref_loss.detach())
            assert abs(l_gpu - l_ref) <= 1e-4 * abs(l_ref) + 1e-6, (u, epoch, mbi, l_gpu, l_ref)
            gpu_g = dict(zip(agent.flat.names, (p.grad.detach().cpu() for p in agent.flat.params)))
            w, bad = grad_mismatches(gpu_g, oracle.model.named_parameters())
            na, nc = kinks['n_actor'], kinks['n_critic']
            if bad and na + nc:
                # elements on a loss kink: the GPU gradient must equal the oracle's for SOME side of
                # each kinked element — every gradient tensor compared at the per-tensor bound
                assert na + nc <= 4, (u, epoch, mbi, kinks)
                for combo in itertools.product((0., 1.), repeat=na + nc):
                    oracle.model.zero_grad()
                    with _loss_kinks(dict(actor=combo[:na], critic=combo[na:])):
                        R.minibatch_loss(oracle.model, rs, mb, latent, c.weights, keep)[0].backward()
                    w, bad_k = grad_mismatches(gpu_g, oracle.model.named_parameters())
                    if not bad_k:
                        kinked.append((u, epoch, mbi, na, nc, combo))
                        break
                else:
                    raise AssertionError(('no branch assignment of the kinked elements matches', u, epoch, mbi,
                                          kinks, sorted(bad, key=lambda x: -x[1] / max(x[2], 1e-30))[:8]))
            else:
                assert not bad, (u, epoch, mbi, sorted(bad, key=lambda x: -x[1] / max(x[2], 1e-30))[:8], len(bad))
            worst[0] = max(worst[0], w)

        agent.learn(traj, lens, genes, fit, update=u, probe=probe)
    print(f'worst gradient error / own tensor scale: {worst[0]:.2e}; minibatches on a loss kink (resolved branch): '
          f'{kinked}')


@pytest.mark.parametrize('evo,gates,frac', [(False, False, None), (True, True, None), (False, False, 2),
                                             (True, False, 2)])
def test_learner_two_updates_match_oracle(evo, gates, frac):
    """Free-running: both sides train on their own.  The first update matches at 1e-4; later
    minibatches may drift because AdoptAtan2's cautious mask (sign of m*g) is discontinuous, so a
    1e-7 gradient difference can flip an element's step size 10x (documented in DESIGN.md).  Every
    step of the same runs is checked tightly by test_optimizer_step_in_learner_matches_restatement
    (teacher-forced) and every minibatch's loss / gradients by test_ppo_loss_and_grads_identical_weights."""
    learner, env, oracle = make_learner(depth=2, gates=gates, evo=evo, T=10, episodes=6, batch=2, seed=5, hazard=2,
                                        fractal_levels=frac)
    agent = learner.agent
    keys = ('loss', 'actor_loss', 'critic_loss', 'autoreg_loss', 'pred_done_loss')
    for u in range(2):
        traj, lens, genes, cum = learner.rollout_device(env, u, 10)
        episodes, fitness = oracle.rollout(u)
        compare_rollout(traj, lens, episodes)
        fit = learner.fitness(cum, genes)
        agent.learn(traj, lens, genes, fit, update=u)
        oracle.learn(episodes, fitness, u)
        ours = np.array([[lg[k] for k in keys] for lg in agent.pop_logs()])
        theirs = np.array([[lg[k] for k in keys] for lg in oracle.logs])
        oracle.logs = []
        if u == 0:
            np.testing.assert_allclose(ours, theirs, rtol=1e-4, atol=1e-5)
        else:
            np.testing.assert_allclose(ours[:3], theirs[:3], rtol=1e-4, atol=1e-5)
            np.testing.assert_allclose(ours, theirs, rtol=5e-2, atol=5e-3)


@pytest.mark.parametrize('evo,gates,frac', [(False, True, None), (True, False, None), (False, False, 2)])
def test_optimizer_step_in_learner_matches_restatement(evo, gates, frac):
    """Teacher-forced clip + AdoptAtan2 inside the Learner: for every minibatch of two updates the
    step is recomputed on the host from the GPU's own pre-step weights, gradient and optimiser state
    (the arithmetic of oracle/thirdparty.AdoptAtan2 and torch's clip_grad_norm_), so nothing drifts
    and every step is checked tightly — where test_learner_two_updates_match_oracle, free-running,
    allows 5e-2 after three minibatches.  The cautious mask where(m g > 0, 1, c) is discontinuous in
    m, so it is taken from the GPU's updated m (itself checked at 2e-6); the clip coefficient at 1e-6;
    the weight change at 1e-4 of itself + 4 ulp of the weight; v at 2e-6."""
    learner, env, oracle = make_learner(depth=2, gates=gates, evo=evo, T=10, episodes=6, batch=2, seed=5, hazard=2,
                                        fractal_levels=frac)
    agent = learner.agent
    o = agent.opt_cfg
    seg = agent.flat.seg.cpu().tolist()
    snap, checked = {}, []

    def probe(epoch, mbi, idx, loss, stats):
        torch.cuda.synchronize()
        snap.update(p=agent.flat.flat.cpu().clone(), g=agent.flat.grad.cpu().clone(), m=agent.opt_m.cpu().clone(),
                    v=agent.opt_v.cpu().clone(), first=agent.opt_first,
                    pi=agent.opt_p_init.cpu().clone() if agent.opt_p_init is not None else None)

    def probe_step(epoch, mbi):
        torch.cuda.synchronize()
        p1, m1, v1 = agent.flat.flat.cpu(), agent.opt_m.cpu(), agent.opt_v.cpu()
        g0 = snap['g']
        norm = float(g0.double().pow(2).sum().sqrt())
        coef = float(agent.clip_out[1])
        assert abs(coef - min(1., agent.max_grad_norm / (norm + 1e-6))) <= 1e-6 * coef, (epoch, mbi, coef, norm)
        g = g0 * coef
        pp = snap['p'].clone()
        if o['regen_rate'] > 0 and not snap['first']:
            pp = torch.lerp(pp, snap['pi'], o['lr'] / o['init_lr'] * o['regen_rate'])
        if snap['first']:
            tol(m1, torch.zeros_like(m1), 0., 0.)
            tol(v1, g * g, 2e-6, 1e-12)
            tol(p1, pp, 0., 1e-7)
            checked.append((epoch, mbi, 'first'))
            return
        u = torch.atan2(g, o['b'] * snap['v'].sqrt())
        m = torch.lerp(snap['m'], u, 1. - o['betas'][0])
        tol(m1, m, 2e-6, 1e-7)
        tol(v1, torch.lerp(snap['v'], g * g, 1. - o['betas'][1]), 2e-6, 1e-12)
        delta = torch.empty_like(p1)
        cf = o['cautious']
        for a0, b0 in zip(seg[:-1], seg[1:]):
            mm, gg = m1[a0:b0], g[a0:b0]
            align = (mm * gg) > 0
            k = int(align.sum())
            mean = (k + cf * (b0 - a0 - k)) / (b0 - a0) if cf < 1. else 1.
            scale = torch.where(align, torch.ones_like(mm), torch.full_like(mm, cf)) / max(mean, 1e-5) \
                if cf < 1. else torch.ones_like(mm)
            delta[a0:b0] = -o['lr'] * (mm * scale * o['a'])
        got = p1 - pp
        ulp = torch.maximum(pp.abs(), p1.abs()) * 2. ** -23
        bad = (got - delta).abs() > 1e-4 * delta.abs() + 4 * ulp
        assert not bad.any(), (epoch, mbi, int(bad.sum()), float((got - delta).abs().max()))
        checked.append((epoch, mbi))

    for u in range(2):
        traj, lens, genes, cum = learner.rollout_device(env, u, 10)
        agent.learn(traj, lens, genes, learner.fitness(cum, genes), update=u, probe=probe, probe_step=probe_step)
    assert len(checked) >= 8 and checked[0][-1] == 'first', checked


@pytest.mark.parametrize('name', ['learner_readme', 'learner_lander_evo'])
def test_learner_replays_reference_learner_fixture(golden, name):
    """The device Learner against the REFERENCE's own Learner run (tests/golden/make_golden.py
    gen_learner executes x_transformers_rl.py:1174-1380 — rollout, Agent.learn, EMA, EPO — with the
    shared sampling / reward-coin / minibatch-order / evolve-seed protocol patched in): the same
    initial weights (reference state_dict names, strict load) and genes, then two updates.
    Rollouts: lengths, actions, terminations, states and rewards bit-exact, log-probs and critic
    logits within 1e-4, per-gene fitness within 1e-5.  Logs: update 0's minibatches within 1e-4;
    update 1's first three within 1e-4 and all within the free-running drift bound of
    test_learner_two_updates_match_oracle (5e-2: AdoptAtan2's cautious mask).  Final online / EMA
    weights: 99 % of the elements within 1e-5 of the reference's, every element within 16 lr (one
    full step per optimiser step: a flipped cautious-mask bit moves an element by at most that);
    RSNorm statistics within 1e-5, final genes within 1e-5 (README config: no EPO)."""
    from xtrl_amd import Learner, SynthVecSim
    g = golden(name)
    seed, S, A, Tm, depth, gates, evo, episodes, batch, updates, hz, gdim = (int(x) for x in g['cfg'])
    wm = dict(attn_dim_head=16, heads=4, depth=depth)
    if gates:
        wm.update(attn_gate_values=True, add_value_residual=True, learned_value_residual_mix=True)
    gp = dict(dim=gdim, num_genes_per_island=3, num_selected=2, tournament_size=2)
    learner = Learner(state_dim=S, num_actions=A, reward_range=(-2., 2.), world_model=wm, max_timesteps=Tm,
                      batch_size=batch, num_episodes_per_update=episodes, evolutionary=bool(evo), evolve_every=1,
                      evolve_after_step=0, latent_gene_pool=gp,
                      agent_kwargs=dict(dropout=0., seed=seed, reward_dropout=float(g['reward_dropout'])),
                      use_graph=False)
    agent = learner.agent
    sd = {k[5:]: torch.from_numpy(g[k]) for k in g.files if k.startswith('init.')}
    with torch.no_grad():
        agent.model.load_state_dict(sd, strict=True)
        agent.ema_flat.copy_(agent.flat.flat)
        if evo:
            agent.gene_pool.genes.copy_(torch.from_numpy(g['init_genes']).to(agent.gene_pool.genes.device))
    env = SynthVecSim(S, A, str(g['mode']), hazard_log2=hz)
    keys = list(g['log_keys'])
    n_mb = g['logs'].shape[0] // updates
    for u in range(updates):
        traj, lens, genes, cum = learner.rollout_device(env, u, Tm)
        torch.cuda.synchronize()
        lens_c = lens.cpu().numpy()
        np.testing.assert_array_equal(lens_c, g[f'u{u}.lens'])
        n = int(lens_c.max())
        np.testing.assert_array_equal(traj['actions'][:, :n].cpu().numpy(), g[f'u{u}.actions'])
        np.testing.assert_array_equal(traj['states'][:, :n].cpu().numpy(), g[f'u{u}.states'])
        np.testing.assert_array_equal(traj['rewards'][:, :n].cpu().numpy(), g[f'u{u}.rewards'])
        np.testing.assert_array_equal(traj['bounds'][:, :n].cpu().numpy().astype(bool), g[f'u{u}.bounds'])
        tol(traj['logp'][:, :n], torch.from_numpy(g[f'u{u}.logp']), 1e-4, 1e-5)
        tol(traj['values'][:, :n], torch.from_numpy(g[f'u{u}.values']), 1e-4, 1e-4)
        np.testing.assert_array_equal(genes.cpu().numpy(), g[f'u{u}.genes'])
        fit = learner.fitness(cum, genes)
        if evo:
            tol(fit, torch.from_numpy(g[f'u{u}.fitness']), 1e-5, 1e-5)
        agent.learn(traj, lens, genes, fit, update=u)
        ours = np.array([[lg[k] for k in keys] for lg in agent.pop_logs()])
        ref = g['logs'][u * n_mb:(u + 1) * n_mb]
        assert ours.shape == ref.shape
        if u == 0:
            np.testing.assert_allclose(ours, ref, rtol=1e-4, atol=1e-5)
        else:
            np.testing.assert_allclose(ours[:3], ref[:3], rtol=1e-4, atol=1e-5)
            np.testing.assert_allclose(ours, ref, rtol=5e-2, atol=5e-3)
    lr = 8e-4
    steps = updates * n_mb
    worst, off = 0., 0
    for pre, model in (('final.', agent.model), ('ema.', agent.ema_model)):
        for k, p in model.state_dict().items():
            ref = torch.from_numpy(g[pre + k])
            d = (p.detach().cpu() - ref).abs()
            worst = max(worst, float(d.max()))
            off += int((d > 1e-5 + 1e-5 * ref.abs()).sum())
            assert float(d.max()) <= steps * lr, (pre + k, float(d.max()))
            assert float((d > 1e-5 + 1e-5 * ref.abs()).float().mean()) <= 0.01, (pre + k, float(d.max()))
    print(f'{name}: final weights max |delta| {worst:.2e}, {off} elements beyond 1e-5')
    tol(agent.rs_mean, torch.from_numpy(g['rs_mean']), 1e-5, 1e-6)
    tol(agent.rs_var, torch.from_numpy(g['rs_var']), 1e-5, 1e-6)
    assert agent.rs_step == int(g['rs_step'])
    if evo:
        tol(agent.gene_pool.genes, torch.from_numpy(g['final_genes']), 1e-5, 1e-6)


# ----------------------------------------------------------------------------------------------
# the reference's own test contract (tests/test_x_transformers_rl.py:4-53) on the host-env path
# ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('evolutionary', (False, True))
@pytest.mark.parametrize('continuous_actions', (False, True))
def test_e2e_reference_contract(evolutionary, continuous_actions, tmp_path):
    from xtrl_amd import Learner

    class Sim:
        def reset(self, seed=None):
            return np.random.randn(5)

        def step(self, actions):
            return np.random.randn(5), np.random.randn(1), False

    learner = Learner(state_dim=5, num_actions=2, reward_range=(-1., 1.), max_timesteps=10, batch_size=2,
                      num_episodes_per_update=2, continuous_actions=continuous_actions, evolutionary=evolutionary,
                      latent_gene_pool=dict(dim=32, num_genes_per_island=3, num_selected=2, tournament_size=2),
                      world_model=dict(attn_dim_head=16, heads=4, depth=1),
                      agent_kwargs=dict(save_path=str(tmp_path / 'ppo.pt')))
    learner(Sim(), 1)
    agent = learner.agent
    hiddens = None
    actions, hiddens = agent(np.random.randn(5), hiddens=hiddens)
    actions, hiddens = agent(np.random.randn(5), hiddens=hiddens)
    assert actions.shape == ((4,) if continuous_actions else (2,))
    assert torch.isfinite(actions).all()
    assert (tmp_path / 'ppo.pt').exists()


@pytest.mark.parametrize('frac,dim', [(None, 48), (2, 48), (None, 256)])
def test_deploy_forward_matches_oracle_cached_decode(frac, dim):
    """Agent.forward (online model, KV cache — and for the fractal body the level running sums —
    threaded through hiddens) vs the oracle module; dim 256: the one-launch feed-forward at E = 1."""
    learner, env, oracle = make_learner(depth=2, gates=frac is None, fractal_levels=frac, dim=dim)
    deploy_parity(learner, oracle, 4)


def deploy_parity(learner, oracle, steps, S=8):
    """Agent.forward for ``steps`` steps (E = 1, the cache threaded through hiddens; non-trivial RSNorm
    statistics, a reward on every second step) against the oracle module's cached decode: the actor's raw
    outputs within 1e-4 + 1e-5.  Returns the last hiddens."""
    agent = learner.agent
    agent.rs_mean.copy_(torch.linspace(-0.5, 0.5, S + 1))
    agent.rs_var.copy_(torch.linspace(0.5, 2., S + 1))
    rs = R.RSNormState(S + 1)
    rs.mean, rs.var = agent.rs_mean.cpu().clone(), agent.rs_var.cpu().clone()
    m = oracle.model
    m.eval()
    g = torch.Generator().manual_seed(2)
    hiddens, cache = None, None
    for t in range(steps):
        s = torch.randn(S, generator=g)
        reward = None if t % 2 == 0 else float(torch.randn((), generator=g))
        raw, hiddens = agent(s.numpy(), reward=reward, hiddens=hiddens)
        swr = rs.apply(torch.cat((s, torch.tensor([0. if reward is None else reward]))))
        with torch.no_grad():
            r, _, _, _, cache = m(swr[:-1].reshape(1, 1, -1), rewards=None if reward is None else swr[-1],
                                  cache=cache)
        tol(raw, r.reshape(-1), 1e-4, 1e-5)
    return hiddens


class _Captured(Exception):
    pass


def _first_minibatch(agent, traj, lens, genes, fit):
    """Loss and flat gradient of the first minibatch of agent.learn (weights left untouched)."""
    out = {}

    def probe(epoch, mbi, idx, loss, stats):
        out['loss'] = float(loss.detach())
        out['grad'] = agent.flat.grad.detach().clone()
        raise _Captured()

    with pytest.raises(_Captured):
        agent.learn(traj, lens, genes, fit, update=0, probe=probe)
    agent.step = 0
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('cont,evo,gates,p,T', [(False, False, True, 0.0, 70), (False, True, True, 0.25, 70),
                                               (True, False, False, 0.1, 40), (False, True, False, 0.25, 130)])
def test_fused_train_step_matches_autograd(cont, evo, gates, p, T):
    """The hand-scheduled learn step (xtrl_train_forward/backward) against the reference-mode
    autograd step (model.forward_train + fused loss + loss.backward) on identical weights and
    minibatch, dropout on (the same counter-based masks): loss within 1e-5 relative, every
    gradient within 1e-4 of the gradient scale.  n > 64 exercises multi-tile attention."""
    _fused_vs_autograd(cont, evo, gates, p, T, depth=3, episodes=8, batch=4, hazard=5, dim=64)


@pytest.mark.gpu
def test_fused_train_step_large_tiles_matches_autograd():
    """As above at a size where the forward, input-gradient and weight-gradient GEMMs take the
    large-tile split-bf16 geometry (96 episodes x 131 tokens, d 128, ff 512) with every fused
    epilogue (LayerNorm prologue, GELU + dropout, SiLU save, residual, GELU' and gate backward)."""
    _fused_vs_autograd(False, False, True, 0.25, 130, depth=2, episodes=96, batch=96, hazard=9, dim=128)


@pytest.mark.gpu
def test_ff_glu_fused_train_step_matches_autograd():
    """ff_glu: the fused learn step (GLU projection GEMM + k_glu_fwd / k_glu_bwd) against the
    reference-mode autograd step (xlinear + ops.glu_drop) with dropout on, at large-tile sizes."""
    _fused_vs_autograd(False, True, True, 0.25, 70, depth=2, episodes=16, batch=16, hazard=6, dim=128, ff_glu=True)


def _fused_vs_autograd(cont, evo, gates, p, T, depth, episodes, batch, hazard, dim, fractal=None, ff_glu=False,
                       checks=None, **geom):
    """``geom``: further make_learner keywords (S, A, heads, dim_head, ff_mult, squash: test_geometry_gpu; window,
    kv_heads, num_mem_kv, add_zero_kv, with_oracle: the attention files); ``checks(learner, env, oracle)``: the
    caller's own assertions on what was built."""
    learner, env, oracle = make_learner(depth=depth, gates=gates, evo=evo, cont=cont, T=T, episodes=episodes,
                                        batch=batch, seed=9, hazard=hazard, dim=dim, fractal_levels=fractal,
                                        ff_glu=ff_glu, **geom)
    if checks is not None:
        checks(learner, env, oracle)
    agent = learner.agent
    agent.cfg.dropout = p
    agent.model.cfg.dropout = p
    traj, lens, genes, cum = learner.rollout_device(env, 0, T)
    fit = learner.fitness(cum, genes)
    agent.fused_learn = True
    a = _first_minibatch(agent, traj, lens, genes, fit)
    agent.fused_learn = False
    b = _first_minibatch(agent, traj, lens, genes, fit)
    assert abs(a['loss'] - b['loss']) <= 1e-5 * abs(b['loss']) + 1e-6, (a['loss'], b['loss'])
    scale = float(b['grad'].abs().max())
    for name, (s, e) in agent.flat.index.items():
        err = float((a['grad'][s:e] - b['grad'][s:e]).abs().max())
        assert err <= 1e-4 * scale + 1e-7, (name, err, scale)
    return lens.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize('cont,evo,p,T,levels,dim', [(False, True, 0.25, 70, 2, 64), (True, False, 0.1, 40, 3, 64),
                                                     (False, False, 0.0, 130, 1, 48), (False, True, 0.25, 100, 2, 256)])
def test_fractal_fused_train_step_matches_autograd(cont, evo, p, T, levels, dim):
    """The hand-scheduled fractal learn step (xtrl_fractal_train_forward/backward: LayerNorm with
    bias in the GEMM epilogues, causal running means as scans, dropout from the shared Philox
    streams) against the reference-mode autograd step (FractalPolicyActorCritic.forward_train +
    fused loss + loss.backward) on identical weights, minibatch and masks: loss within 1e-5
    relative, every gradient within 1e-4 of the gradient scale."""
    _fused_vs_autograd(cont, evo, False, p, T, depth=levels, episodes=8, batch=4, hazard=5, dim=dim, fractal=levels)


# ----------------------------------------------------------------------------------------------
# BASELINE configurations (C2, C3) against the oracle: rollout, then the learn step's loss and
# every gradient on identical weights, at the configs' model shapes and sequence lengths
# ----------------------------------------------------------------------------------------------


def _config_parity(depth, dim, T, hazard, evo, episodes, batch, gene_dim=8, max_minibatches=2, fractal=None):
    """Rollout of the device Learner vs the oracle's batch-1 loop (actions / lengths / rewards /
    done masks bit-exact, log-probs and critic logits within 1e-4), then the first
    ``max_minibatches`` minibatches of Agent.learn: loss within 1e-4 relative and every gradient
    within 1e-4 of the gradient scale against the oracle on the GPU's weights and minibatch."""
    learner, env, oracle = make_learner(depth=depth, gates=fractal is None, evo=evo, T=T, episodes=episodes,
                                        batch=batch, seed=4, hazard=hazard, dim=dim, gene_dim=gene_dim,
                                        fractal_levels=fractal)
    traj, lens, genes, cum = learner.rollout_device(env, 0, T)
    torch.cuda.synchronize()
    episodes_o, fitness = oracle.rollout(0)
    compare_rollout(traj, lens, episodes_o)
    fit = learner.fitness(cum, genes)
    if evo:
        tol(fit, fitness, 1e-5, 1e-5)
    seen = _learn_parity(learner, oracle, traj, lens, genes, fit, max_minibatches)
    return seen, lens


def _learn_parity(learner, oracle, traj, lens, genes, fit, max_minibatches, dropout=0., packed=False, cont=False):
    """The first ``max_minibatches`` minibatches of Agent.learn against the oracle on the GPU's
    current weights, RSNorm, genes and minibatch (rebuilt from the device trajectory as
    xtrl.py:822-852 does): loss within 1e-4 relative, every gradient within 1e-4 of the gradient
    scale.  ``dropout`` > 0: the learn step runs with attention / FF dropout and the oracle applies
    the same keep masks (oracle.philox.attn_dropout_keep / ff_dropout_keep) in its training forward.
    ``cont``: continuous actions (the episodes are rebuilt from the trajectory's float actions)."""
    agent = learner.agent
    c = oracle.c
    evo = agent.evolutionary
    agent.cfg.dropout = dropout
    agent.model.cfg.dropout = dropout
    gene_list = genes.cpu().tolist()
    states, actions, old_lp, rewards, bounds, values, elens, egenes = oracle_minibatch_tensors(
        gpu_episodes(traj, lens, gene_list, cont))
    returns = R.calc_gae(rewards, oracle.model.hl(values), (~bounds).float(), c.gamma, c.lam)
    rs = R.RSNormState(c.state_dim + 1)
    rs.mean, rs.var = agent.rs_mean.cpu().clone(), agent.rs_var.cpu().clone()
    N = len(gene_list)
    n_mb_epoch = (N + agent.batch_size - 1) // agent.batch_size
    seen = []

    def probe(epoch, mbi, idx, loss, stats):
        idx = idx.cpu()
        oracle.model.load_state_dict({k: v.detach().cpu() for k, v in agent.model.state_dict().items()})
        oracle.model.train()
        oracle.model.zero_grad()
        ordinal = epoch * n_mb_epoch + mbi        # Agent.learn's dropout counters for this minibatch
        if dropout > 0.:     # (the decoder's dropout streams; the fractal oracle body runs dropout-free)
            R.install_philox_dropout(oracle.model, dropout, agent.seed * 1000003 + 0,
                                     ordinal * agent.batch_size * agent.cfg.heads, ordinal,
                                     packed_lens=elens[idx].tolist() if packed else None)
        mb = R.Minibatch(states[idx], actions[idx], rewards[idx], old_lp[idx], returns[idx], values[idx], bounds[idx],
                         egenes[idx], elens[idx])
        latent = R.l2norm(agent.gene_pool.genes[mb.gene_ids]) if evo else None
        keep = R.reward_coin(c.seed, 0, epoch, mbi, c.reward_dropout)
        ref_loss, _, _, _ = R.minibatch_loss(oracle.model, rs, mb, latent, c.weights, keep)
        ref_loss.backward()
        l_gpu, l_ref = float(loss.detach()), float(ref_loss.detach())
        assert abs(l_gpu - l_ref) <= 1e-4 * abs(l_ref) + 1e-6, (epoch, mbi, l_gpu, l_ref)
        gpu_g = dict(zip(agent.flat.names, (p.grad.detach().cpu() for p in agent.flat.params)))
        worst, bad = grad_mismatches(gpu_g, oracle.model.named_parameters())
        assert not bad, (epoch, mbi, sorted(bad, key=lambda x: -x[1] / max(x[2], 1e-30))[:8], len(bad))
        seen.append((int(states.shape[1]), l_gpu, worst, int(idx.numel())))   # padded n = the learn step's width
        if len(seen) >= max_minibatches:
            raise _Captured()

    with pytest.raises(_Captured):
        agent.learn(traj, lens, genes, fit, update=0, probe=probe)
    print('minibatches (n, loss, worst grad err / scale, episodes):', seen)
    return seen


@pytest.mark.parametrize('dim,gates', [(48, True), (256, False)])
def test_ff_no_bias_rollout_and_learn_match_oracle(dim, gates):
    """world_model['ff_no_bias'] (x-transformers FeedForward without biases): the rollout (the decode
    feed-forward kernel on zero packed biases) and the fused learn step (bias pointers absent: no bias
    epilogue, no bias gradient) against the oracle's bias-free FeedForward."""
    learner, env, oracle = make_learner(depth=2, gates=gates, T=24, episodes=6, batch=3, seed=6, hazard=3, dim=dim,
                                        ff_no_bias=True)
    names = [n for n, _ in learner.agent.model.named_parameters()]
    assert not any(n.endswith(('ff.0.0.bias', 'ff.2.bias')) for n in names)
    traj, lens, genes, cum = learner.rollout_device(env, 0, 24)
    torch.cuda.synchronize()
    episodes_o, _ = oracle.rollout(0)
    compare_rollout(traj, lens, episodes_o)
    seen = _learn_parity(learner, oracle, traj, lens, genes, learner.fitness(cum, genes), 2)
    assert len(seen) == 2


@pytest.mark.gpu
@pytest.mark.parametrize('dim,gates,no_bias,dropout', [(64, True, False, 0.25), (128, False, True, 0.)])
def test_ff_glu_rollout_and_learn_match_oracle(dim, gates, no_bias, dropout):
    """world_model['ff_glu'] (x-transformers FeedForward glu: the GLU projection [2 ff][d], value *
    gelu(gate), then the dropout): the rollout (GLU projection GEMM + k_glu_rows, the multi-kernel decode
    step) and the fused learn step (GLU projection GEMM, k_glu_fwd / k_glu_bwd with the feed-forward
    dropout stream, gradients of the [2 ff] projection) against the oracle's GLU FeedForward; with
    ff_no_bias the GLU projection keeps its bias (x-transformers GLU), the last Linear has none."""
    learner, env, oracle = make_learner(depth=2, gates=gates, T=24, episodes=6, batch=3, seed=8, hazard=3, dim=dim,
                                        ff_glu=True, ff_no_bias=no_bias)
    names = [n for n, _ in learner.agent.model.named_parameters()]
    assert any(n.endswith('ff.0.proj.weight') for n in names) and any(n.endswith('ff.0.proj.bias') for n in names)
    traj, lens, genes, cum = learner.rollout_device(env, 0, 24)
    torch.cuda.synchronize()
    episodes_o, _ = oracle.rollout(0)
    compare_rollout(traj, lens, episodes_o)
    seen = _learn_parity(learner, oracle, traj, lens, genes, learner.fitness(cum, genes), 2, dropout=dropout)
    assert len(seen) == 2


@pytest.mark.parametrize('opts', [dict(attn_qk_norm=True), dict(rotary_xpos=True, rotary_xpos_scale_base=16.),
                                  dict(attn_qk_norm=True, attn_qk_norm_scale=6., rotary_xpos=True)],
                         ids=['qk_norm', 'xpos', 'qk_norm_scale6_xpos'])
def test_world_model_qk_norm_xpos_rollout_and_learn_match_oracle(opts, decode_path):
    """world_model['attn_qk_norm'] (q, k l2-normalised per head before the rotary, scores x
    qk_norm_scale) and world_model['rotary_xpos'] (the xPos scale of the rotary channels: q times,
    k divided by ((j + 0.4 rot) / (1.4 rot)) ^ ((pos - n // 2) / scale_base); a small scale base so
    the factors are far from 1 at T = 24): the rollout (decode attention of both decode paths; the
    reference's cached decode rotates at position 0, where xPos is the identity) and the fused learn
    step (k_qkv_prep / k_qkv_prep_bwd with the l2-norm and xPos terms, the attention scale) against
    the oracle's restated x-transformers Attention / RotaryEmbedding."""
    learner, env, oracle = make_learner(depth=2, gates=True, T=24, episodes=6, batch=3, seed=6, hazard=5,
                                        wm_extra=opts)
    c = learner.agent.cfg
    assert c.qk_norm == bool(opts.get('attn_qk_norm')) and c.rotary_xpos == bool(opts.get('rotary_xpos'))
    traj, lens, genes, cum = learner.rollout_device(env, 0, 24)
    torch.cuda.synchronize()
    episodes_o, _ = oracle.rollout(0)
    compare_rollout(traj, lens, episodes_o)
    assert int(lens.max()) > 10
    seen = _learn_parity(learner, oracle, traj, lens, genes, learner.fitness(cum, genes), 2)
    assert len(seen) == 2


@pytest.mark.parametrize('dim,T', [(48, 24), (256, 40)])
def test_world_model_rmsnorm_rollout_and_learn_match_oracle(dim, T, decode_path):
    """world_model['use_rmsnorm'] (x-transformers RMSNorm, F.normalize(x) sqrt(d) g, parameter .g,
    for every pre-norm and the final norm): the rollout — the embedding's layer-0 norm, the fused
    attention's FF norm, k_mlp's next norm (d 256), the decode GEMM prologues, the row-resident step's
    norms (d 48) — and the fused learn step (the norm epilogues of the GEMMs completing their rows and
    their backward, the embedding's pre-norm, the final norm) against the oracle's restated RMSNorm."""
    learner, env, oracle = make_learner(depth=2, gates=True, T=T, episodes=6, batch=3, seed=8, hazard=4, dim=dim,
                                        wm_extra=dict(use_rmsnorm=True))
    names = [n for n, _ in learner.agent.model.named_parameters()]
    assert 'transformer.attn_layers.final_norm.g' in names and not any(n.endswith('.gamma') for n in names)
    traj, lens, genes, cum = learner.rollout_device(env, 0, T)
    torch.cuda.synchronize()
    episodes_o, _ = oracle.rollout(0)
    compare_rollout(traj, lens, episodes_o)
    seen = _learn_parity(learner, oracle, traj, lens, genes, learner.fitness(cum, genes), 2)
    assert len(seen) == 2


def test_rotary_absolute_rollout_with_xpos_matches_oracle(monkeypatch):
    """The decision-log alternative rotary_abs_rollout=True (absolute positions in the cached
    decode) with rotary_xpos and attn_qk_norm: the decode kernels' rotation at position t with the
    xPos factor of a t + 1 long input, against the oracle's Decoder in 'absolute' rollout mode."""
    monkeypatch.setattr(tp.XT, 'rollout_rotary', 'absolute')
    learner, env, oracle = make_learner(depth=2, gates=True, T=16, episodes=6, batch=3, seed=7, hazard=4,
                                        wm_extra=dict(rotary_xpos=True, rotary_xpos_scale_base=8., attn_qk_norm=True),
                                        agent_extra=dict(rotary_abs_rollout=True))
    traj, lens, _, _ = learner.rollout_device(env, 0, 16)
    torch.cuda.synchronize()
    episodes_o, _ = oracle.rollout(0)
    compare_rollout(traj, lens, episodes_o)
    assert int(lens.max()) > 8


def test_c3_shape_rollout_and_learn_match_oracle():
    """C3 model (depth 4, d 256, 4 x 16 heads, gated values + learned value-residual mix) at its
    sequence length (T = 128, termination hazard 1/64), 16 episodes in minibatches of 8."""
    seen, lens = _config_parity(depth=4, dim=256, T=128, hazard=6, evo=False, episodes=16, batch=8)
    assert len(seen) == 2 and int(lens.max()) > 64     # multi-tile training attention


# ---- the bench's own geometry (bench.py CONFIGS): the kernels and grids the timed run uses ------------


def _bench_learner(cfg, agent_extra=None):
    """make_learner at a bench.py configuration (model, episodes per update, minibatch, T, hazard)."""
    from bench import CONFIGS
    c = CONFIGS[cfg]
    return make_learner(depth=c['depth'], gates=c['gates'], evo=c['evo'], T=c['T'], episodes=c['episodes'],
                        batch=c['batch'], seed=4, hazard=c['hazard_log2'], dim=c['dim'], gene_dim=32,
                        genes=c.get('genes', 3), fractal_levels=c.get('fractal'), agent_extra=agent_extra)


@contextlib.contextmanager
def _hl_reduction(mean):
    """The oracle's HL-Gauss reduction (thirdparty.HLGaussLoss.default_reduction) for one test."""
    prev = tp.HLGaussLoss.default_reduction
    tp.HLGaussLoss.default_reduction = 'mean' if mean else 'none'
    try:
        yield
    finally:
        tp.HLGaussLoss.default_reduction = prev


def _first_minibatch_state(agent, traj, lens, genes, fit):
    """Loss, flat gradient and the per-token outputs of the first minibatch of agent.learn."""
    out = {}

    def probe(epoch, mbi, idx, loss, stats):
        ts = agent._train_step
        b, n = ts.D.b, ts.D.n
        out.update(loss=float(loss.detach()), grad=agent.flat.grad.detach().clone(), n=n, idx=idx.cpu(),
                   raw=ts.buf['raw'][:b * n].view(b, n, -1).clone(), values=ts.buf['values'][:b * n].view(b, n, -1).clone())
        raise _Captured()

    with pytest.raises(_Captured):
        agent.learn(traj, lens, genes, fit, update=0, probe=probe)
    agent.step = 0
    return out


@pytest.mark.parametrize('evo,gates,T,dim,cont,wm', [
    (True, True, 40, 64, False, None), (False, True, 150, 48, False, None), (True, False, 130, 64, False, None),
    (False, True, 40, 64, True, None),                                            # continuous actions
    (True, True, 40, 64, False, dict(ff_glu=True, attn_qk_norm=True, rotary_xpos=True)),
    (False, False, 70, 64, False, dict(use_rmsnorm=True))])
def test_packed_learn_matches_padded_step(evo, gates, T, dim, cont, wm):
    """The packed learn step (Agent(packed_learn=True): only the minibatch's valid tokens, episode after
    episode — packed inputs, per-episode attention row ranges, rotary positions from the row list, the
    latent broadcast and gradient per episode range) against the padded fused step on the same
    weights and minibatch, both with the per-token critic reduction and dropout 0: the loss, the
    actor / critic outputs on the valid tokens (zeros on the padding for the packed step) and every
    gradient tensor within 1e-4 of its own scale.  T 150: key tiles past 128 (the long-episode
    attention backward with per-episode rows)."""
    _packed_vs_padded(evo, gates, T, dim, cont, wm)


def _packed_vs_padded(evo, gates, T, dim, cont, wm, depth=2, **geom):
    """The body of test_packed_learn_matches_padded_step; ``depth`` and ``geom`` (S, A, heads, dim_head, ...;
    window, kv_heads, with_oracle): further make_learner keywords (test_geometry_gpu, the attention files).
    Returns the packed step's first-minibatch state (its padded width ``n`` among it)."""
    res = {}
    glu = bool((wm or {}).get('ff_glu', False))
    extra = {k: v for k, v in (wm or {}).items() if k != 'ff_glu'} or None
    for packed in (False, True):
        learner, env, _ = make_learner(depth=depth, gates=gates, evo=evo, T=T, episodes=8, batch=8, seed=5, hazard=5,
                                       dim=dim, cont=cont, ff_glu=glu, wm_extra=extra,
                                       agent_extra=dict(hl_reduction_mean=False, packed_learn=packed), **geom)
        agent = learner.agent
        traj, lens, genes, cum = learner.rollout_device(env, 0, T)
        res[packed] = _first_minibatch_state(agent, traj, lens, genes, learner.fitness(cum, genes))
        res[packed]['lens'] = lens.cpu()
    a, b = res[True], res[False]
    assert torch.equal(a['lens'], b['lens']) and torch.equal(a['idx'], b['idx'])
    lens_mb = a['lens'][a['idx']].clamp(max=a['n'])
    assert lens_mb.min() < a['n']    # padding present
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
    return a


@pytest.mark.parametrize('cfg', ['c3', 'c2'])
def test_packed_learn_bench_minibatch_matches_oracle(cfg):
    """The packed learn step at the bench geometry (C3: 128 episodes x 128 steps per minibatch, depth 4,
    d 256; C2: 32 x ~430, 3-gene EPO, long-episode attention backward) with the per-token critic reduction
    and dropout 0.25, against the oracle on the padded minibatch: the attention keep masks are the padded
    step's (keyed by episode and position), the FF masks are numbered over the packed rows (the oracle's
    PhiloxFFDropout(packed_lens)); loss at 1e-4 relative, every gradient at 1e-4 of its scale, two
    minibatches."""
    learner, env, oracle = _bench_learner(cfg, agent_extra=dict(hl_reduction_mean=False, packed_learn=True))
    T = 128 if cfg == 'c3' else 500
    traj, lens, genes, cum = learner.rollout_device(env, 0, T)
    with _hl_reduction(False):
        seen = _learn_parity(learner, oracle, traj, lens, genes, learner.fitness(cum, genes), 2, dropout=0.25,
                             packed=True)
    assert len(seen) == 2


def _full_width_rollout(cfg):
    """The bench rollout of ``cfg`` at full width through the captured hipGraph vs the oracle's
    batch-1 loop: every (episode, gene) pair's first 4 steps, and 16 whole episodes (the longest ones
    and a spread of slots) over the full KV-cache length."""
    learner, env, oracle = _bench_learner(cfg)
    learner.use_graph = True
    learner._engine = None
    traj, lens, genes, cum = learner.rollout_device(env, 0, 128)
    torch.cuda.synchronize()
    assert len(learner.episode_genes) == 1024
    episodes, fitness = oracle.rollout(0, max_timesteps=4)
    compare_rollout(traj, lens, episodes, prefix=4)
    lens_c = lens.cpu()
    longest = torch.argsort(lens_c, descending=True, stable=True)[:8].tolist()
    spread = [int(x) for x in torch.linspace(5, 1019, 8).round().long().tolist()]
    rows = sorted(set(longest + spread))
    episodes, _ = oracle.rollout(0, slots=rows)
    compare_rollout(traj, lens, episodes, rows=rows)
    assert int(lens_c.max()) == 128 and int((lens_c == 128).sum()) > 50
    return learner, traj, lens, genes, cum


def test_c2_full_width_rollout_matches_oracle():
    """The C2 bench rollout at full width: 768 (episode, gene) pairs (256 episodes x 3 genes, 32-dim
    genes), T = 500, depth 2, d 128, through the captured graphs — the multi-kernel step while more
    than rows_max rows are live, then the row-resident step for the long tail (chunks after the live
    count fell to rows_max) — against the oracle's batch-1 loop: every pair's first 4 steps, and 16
    whole episodes (the longest ones, which run deep into the row-resident tail, and a spread)."""
    learner, env, oracle = _bench_learner('c2')
    learner.use_graph = True
    learner._engine = None
    traj, lens, genes, cum = learner.rollout_device(env, 0, 500)
    torch.cuda.synchronize()
    eng = learner._engine[1]
    assert len(learner.episode_genes) == 768 and eng.rows_max > 0 and eng.chunks_rows > 2
    episodes, fitness = oracle.rollout(0, max_timesteps=4)
    compare_rollout(traj, lens, episodes, prefix=4)
    lens_c = lens.cpu()
    longest = torch.argsort(lens_c, descending=True, stable=True)[:8].tolist()
    spread = [int(x) for x in torch.linspace(3, 764, 8).round().long().tolist()]
    rows = sorted(set(longest + spread))
    episodes, _ = oracle.rollout(0, slots=rows)
    compare_rollout(traj, lens, episodes, rows=rows)
    assert int(lens_c.max()) > 300


def test_c5_full_width_fractal_rollout_matches_oracle():
    """The C5 bench rollout at full width: 1024 (episode, gene) pairs of EPO population 8, the
    fractal policy body (4 levels, d 256) — 37 launches per step through the captured hipGraph,
    k_mlp's fractal last arriver (LN3, running level means, next level input) and the split-output
    global-state / level-projection GEMM at up to 1024 live rows — against the streaming oracle;
    the per-gene fitness sums against the oracle's sequential ones."""
    learner, traj, lens, genes, cum = _full_width_rollout('c5')
    assert sorted(set(genes.cpu().tolist())) == list(range(8))


def test_c5_bench_minibatch_learn_matches_oracle():
    """The C5 learn step as the bench runs it — 1024 pairs, minibatches of 128 episodes x 128
    steps, 4 fractal levels at d 256, 8 genes of 32 dims, the hand-scheduled fractal train step —
    against the streaming fractal oracle on identical weights and minibatch (dropout 0: the fractal
    oracle body is dropout-free): loss at 1e-4 relative and every gradient at 1e-4 of the gradient
    scale, for two minibatches (the second after one optimiser step)."""
    learner, env, oracle = _bench_learner('c5')
    traj, lens, genes, cum = learner.rollout_device(env, 0, 128)
    seen = _learn_parity(learner, oracle, traj, lens, genes, learner.fitness(cum, genes), 2)
    assert [s[0] for s in seen] == [128, 128] and all(s[3] == 128 for s in seen)


def test_c3_full_width_rollout_matches_oracle():
    """The C3 bench rollout at full width — 1024 episodes x 128 steps through the captured
    hipGraph: 64 k_mlp panels meeting through the counter hand-off and the fused attention /
    out-projection at up to 1024 live rows — against the oracle's batch-1 loop: every episode's
    first 4 steps, and 16 whole episodes (the longest ones and a spread of slots) over the full
    KV-cache length."""
    learner, env, oracle = _bench_learner('c3')
    learner.use_graph = True
    learner._engine = None
    traj, lens, _, _ = learner.rollout_device(env, 0, 128)
    torch.cuda.synchronize()
    assert len(learner.episode_genes) == 1024
    episodes, _ = oracle.rollout(0, max_timesteps=4)
    compare_rollout(traj, lens, episodes, prefix=4)
    lens_c = lens.cpu()
    longest = torch.argsort(lens_c, descending=True, stable=True)[:8].tolist()
    spread = [int(x) for x in torch.linspace(5, 1019, 8).round().long().tolist()]
    rows = sorted(set(longest + spread))
    episodes, _ = oracle.rollout(0, slots=rows)
    compare_rollout(traj, lens, episodes, rows=rows)
    assert int(lens_c.max()) == 128 and int((lens_c == 128).sum()) > 50


@pytest.mark.parametrize('dropout', [0., 0.25])
def test_c3_bench_minibatch_learn_matches_oracle(dropout):
    """The C3 learn step exactly as the bench runs it — 1024 episodes per update, minibatches of
    128 episodes x 128 steps = 16384 tokens, depth 4, d 256, gated values + value residual, the
    fused step (X6 large-tile / warp-specialised GEMMs, split-K weight gradients on the side
    stream) — against the oracle on identical weights and minibatch: loss at 1e-4 relative and
    every gradient at 1e-4 of the gradient scale, for two minibatches (the second after one
    optimiser step).  Dropout 0.25: the oracle draws the GPU's attention / FF keep masks from the
    host Philox stream."""
    learner, env, oracle = _bench_learner('c3')
    traj, lens, genes, cum = learner.rollout_device(env, 0, 128)
    seen = _learn_parity(learner, oracle, traj, lens, genes, learner.fitness(cum, genes), 2, dropout=dropout)
    assert [s[0] for s in seen] == [128, 128] and all(s[3] == 128 for s in seen)


def test_c2_bench_minibatch_learn_matches_oracle():
    """C2 as the bench runs it: 256 episodes x 3 genes (EPO, 32-dim genes) at T = 500, minibatches
    of 32 episodes x ~430 steps, depth 2, d 128, dropout 0.25 — loss and every gradient against
    the oracle with the GPU's dropout masks, two minibatches."""
    learner, env, oracle = _bench_learner('c2')
    traj, lens, genes, cum = learner.rollout_device(env, 0, 500)
    seen = _learn_parity(learner, oracle, traj, lens, genes, learner.fitness(cum, genes), 2, dropout=0.25)
    assert len(seen) == 2 and seen[0][0] > 300 and all(s[3] == 32 for s in seen)


def test_c5_shape_fractal_rollout_and_learn_match_oracle():
    """C5 policy (the fractal body: 4 levels, d 256, 4 x 16 heads, causal per timestep) with EPO
    genes at T = 128: the fractal decode step and the learn step against the streaming oracle."""
    seen, lens = _config_parity(depth=4, dim=256, T=128, hazard=6, evo=True, episodes=4, batch=4, fractal=4)
    assert len(seen) == 2 and int(lens.max()) > 64


def test_c2_shape_rollout_and_learn_match_oracle():
    """C2 model (train_lander defaults: depth 2, d 128, 3-gene EPO with 32-dim genes) at T = 500:
    the decode attention over caches up to 500 keys and the training attention over 8 key tiles
    (hazard 2^-9 so most episodes run long)."""
    seen, lens = _config_parity(depth=2, dim=128, T=500, hazard=9, evo=True, episodes=2, batch=2, gene_dim=32)
    assert int(lens.max()) > 256


def test_c3_full_minibatch_fused_matches_reference_mode():
    """The C3 learn step at its real minibatch (128 episodes x 128 steps = 16384 tokens, dropout
    0.25): the fused step — X6 large-tile GEMMs, the warp-specialised kernel, split-K weight
    gradients over 192 workgroups on the side stream — against the reference-mode autograd step on
    identical weights, minibatch and dropout masks."""
    _fused_vs_autograd(False, False, True, 0.25, 128, depth=4, episodes=128, batch=128, hazard=6, dim=256)


def test_c5_full_minibatch_fractal_fused_matches_reference_mode():
    """The C5 learn step at its bench minibatch (128 episodes x 128 steps, 4 levels, d 256, 4 x 16
    heads, EPO genes, dropout 0.25): the fused fractal step against the reference-mode autograd step."""
    _fused_vs_autograd(False, True, False, 0.25, 128, depth=4, episodes=128, batch=128, hazard=6, dim=256, fractal=4)


def test_ema_schedule_and_model_copy_back_match_oracle():
    """Agent EMA (xtrl.py:747-753, ema-pytorch restated) against oracle/thirdparty.EMA fed the same
    online weights: copies before ``update_after_step``, the lerp with the warm-up decay after it
    (k_ema on the flat buffer), and the online-model copy-back every ``update_model_with_ema_every``
    steps — with ema_kwargs small enough that 40 optimiser steps cover all three."""
    # update_model_with_ema_every not a multiple of update_every: the copy-back also runs on steps
    # where the EMA itself does not update (ema-pytorch order)
    ek = dict(update_after_step=6, update_every=2, update_model_with_ema_every=15)
    learner, _, _ = make_learner(depth=1, gates=False, agent_extra=dict(ema_kwargs=ek))
    agent = learner.agent
    online = torch.nn.Module()
    online.p = torch.nn.Parameter(agent.flat.flat.detach().cpu().clone())
    ema = tp.EMA(online, beta=agent.ema_beta, **ek)
    snaps = []
    orig = agent._ema_update

    def hooked():
        snaps.append(agent.flat.flat.detach().cpu().clone())
        orig()

    agent._ema_update = hooked
    g = torch.Generator().manual_seed(21)
    lerped = copied_back = 0
    for i in range(40):
        agent.flat.grad.copy_(torch.randn(agent.flat.n, generator=g).to(DEV) * 0.1)
        agent.optimizer_step()
        with torch.no_grad():
            online.p.copy_(snaps[-1])
        before = ema.ema_model.p.detach().clone()
        ema.update()
        lerped += int(ema.initted.item() and not torch.equal(before, ema.ema_model.p))
        tol(agent.ema_flat, ema.ema_model.p, 1e-6, 1e-7)
        tol(agent.flat.flat, online.p, 1e-6, 1e-7)
        copied_back += int(torch.equal(online.p.detach(), ema.ema_model.p.detach()) and ema.initted.item())
    assert agent.ema_step == 40 and lerped >= 10 and copied_back >= 2


# ----------------------------------------------------------------------------------------------
# host environments (xtrl.py:1232-1341): the reference's scalar contract and a vectorised env,
# 3 / 4 / 5-tuple step returns, truncation with the GAE bootstrap
# ----------------------------------------------------------------------------------------------


class HostLander:
    """numpy host env, deterministic per episode id (the seed when reset gets one, else the count
    of resets): N(0,1) states, reward N(0,1) (1 + 0.1 a), termination hazard, truncation at
    ``limit`` steps (TimeLimit).  ``ret`` = 3: (s, r, terminated); 4: (s, r, terminated, info) with
    a truthy info on truncation (old gym; the reference reads it as truncated, quirk B8);
    5: (s, r, terminated, truncated, info), reset -> (s, info)."""

    def __init__(self, S=8, ret=5, hazard=0.08, limit=None, base=1000):
        self.S, self.ret, self.hazard, self.limit, self.base = S, ret, hazard, limit, base
        self.count = 0

    def reset(self, seed=None):
        eid = self.count if seed is None else int(seed)
        self.count += 1
        self.rng = np.random.RandomState(self.base + eid)
        self.t = 0
        s = self.rng.randn(self.S)
        return (s, {}) if self.ret == 5 else s

    def step(self, action):
        a = float(np.sum(action)) if isinstance(action, list) else int(action)
        self.t += 1
        s = self.rng.randn(self.S)
        r = self.rng.randn() * (1 + 0.1 * a)
        term = bool(self.rng.rand() < self.hazard)
        trunc = self.limit is not None and self.t >= self.limit
        if self.ret == 3:
            return s, r, term
        if self.ret == 4:
            return s, r, term, ({'TimeLimit.truncated': True} if trunc else {})
        return s, r, term, trunc, {}


class HostLanderVec:
    """W HostLander sub-envs behind the batched contract; wave w's sub-env i plays episode id
    w W + i (the reset count of the scalar env running the same pairs one by one)."""

    def __init__(self, W, **kw):
        self.num_envs = W
        self.envs = [HostLander(**kw) for _ in range(W)]
        self.wave = 0

    def reset(self, seed=None):
        out = [e.reset(seed=seed[i] if seed is not None else self.wave * self.num_envs + i)
               for i, e in enumerate(self.envs)]
        self.wave += 1
        states = np.stack([o[0] if isinstance(o, tuple) else o for o in out])
        return (states, {}) if self.envs[0].ret == 5 else states

    def step(self, actions):
        outs = [e.step(actions[i].tolist() if np.ndim(actions) > 1 else int(actions[i]))
                for i, e in enumerate(self.envs)]
        cols = list(zip(*outs))
        res = [np.stack(cols[0]), np.array(cols[1]), np.array(cols[2])]
        if len(cols) >= 4:
            res.append(list(cols[3]) if isinstance(cols[3][0], dict) else np.array(cols[3]))
        return tuple(res)


def _compare_host(learner, oracle, env_gpu, env_cpu, T, seeds=None):
    traj, lens, genes, cum = learner.rollout_host(env_gpu, 0, T, seeds)
    torch.cuda.synchronize()
    episodes, fitness = oracle.rollout_env(env_cpu, 0, T, seeds)
    compare_rollout(traj, lens, episodes)
    hl = oracle.model.hl
    boot = traj['boot'].cpu()
    for i, ep in enumerate(episodes):
        if ep['boot'] is None:
            assert torch.isnan(boot[i]), i
        else:
            tol(boot[i], hl(ep['boot'][None])[0], 1e-4, 1e-5)
    return traj, lens, genes, cum, episodes, fitness


@pytest.mark.parametrize('ret,limit', [(3, None), (4, 5), (5, 5), (5, None), (5, 9), (4, 9)])
def test_host_env_scalar_contract_matches_oracle(ret, limit, decode_path):
    """The reference's scalar env (batch 1, pairs one by one) through the device decode: states,
    actions, log-probs, rewards, is_boundary = terminated, critic logits and lengths as the
    oracle's reference loop; truncated episodes carry the next state's value (bootstrap) — limit 9 =
    max_timesteps: the truncation lands on the last allowed step and still bootstraps."""
    learner, _, oracle = make_learner(depth=2, gates=True, T=9, episodes=6, batch=2)
    _, lens, _, _, episodes, _ = _compare_host(learner, oracle, HostLander(ret=ret, limit=limit),
                                               HostLander(ret=ret, limit=limit), 9)
    if limit is not None:
        assert any(ep['boot'] is not None for ep in episodes)     # some episodes truncated


class SlowHostLander(HostLander):
    """HostLander whose env step sleeps ``pause`` seconds at step ``at`` of every ``every``-th episode."""

    def __init__(self, at, pause, every=2, **kw):
        super().__init__(**kw)
        self.at, self.pause, self.every = at, pause, every

    def step(self, action):
        if self.t == self.at and (self.count - 1) % self.every == 0:
            time.sleep(self.pause)
        return super().step(action)


@pytest.mark.parametrize('ret,limit', [(5, None), (5, 5), (4, 9), (3, None)])
def test_host_env_gated_step_equals_ungated(ret, limit, monkeypatch):
    """The gated scalar-env loop (xtrl_host_row_step: decode launches queued ahead, each waiting on the
    device for the host's go and applying the previous env results itself) against the launch-per-step
    loop (XTRL_HOST_GATE=0): every trajectory tensor, length, return and bootstrap value bit-identical,
    with truncation bootstraps (limit 5 / 9) and old-gym returns."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', '1')
    runs = []
    for gate in ('1', '0'):
        monkeypatch.setenv('XTRL_HOST_GATE', gate)
        learner, _, _ = make_learner(depth=2, gates=True, T=9, episodes=6, batch=2)
        eng_w = learner._engine_for_host(1, 9)
        assert eng_w.rows_max > 0
        traj, lens, _, cum = learner.rollout_host(HostLander(ret=ret, limit=limit), 0, 9)
        torch.cuda.synchronize()
        runs.append((traj, lens.cpu(), cum.clone()))
    (a, la, ca), (b, lb, cb) = runs
    assert torch.equal(la, lb) and torch.equal(ca, cb)
    for k in a:
        if a[k] is None:
            assert b[k] is None
        else:
            assert torch.equal(torch.nan_to_num(a[k], nan=-7.), torch.nan_to_num(b[k], nan=-7.)), k


class RaisingHostLander(HostLander):
    """HostLander whose env step raises (once) at the first step ``at`` of any episode."""

    def __init__(self, at, **kw):
        super().__init__(**kw)
        self.at, self.raised = at, False

    def step(self, action):
        if self.t == self.at and not self.raised:
            self.raised = True
            raise ValueError('env failure')
        return super().step(action)


def test_host_env_gated_step_env_exception_releases_queued_steps(monkeypatch):
    """An env step that raises inside the gated loop: the exception reaches the caller at once, the
    queued decode launches are released (cancel word) instead of waiting out the device timeout, and
    the same learner then rolls out again and matches the oracle."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', '1')
    monkeypatch.setenv('XTRL_HOST_GATE', '1')
    learner, _, oracle = make_learner(depth=2, gates=True, T=9, episodes=6, batch=2)
    t0 = time.perf_counter()
    with pytest.raises(ValueError, match='env failure'):
        learner.rollout_host(RaisingHostLander(at=1), 0, 9)
    torch.cuda.synchronize()
    assert time.perf_counter() - t0 < 2.0   # (not the 4 s device wait of each queued step)
    _compare_host(learner, oracle, HostLander(), HostLander(), 9)


def test_host_env_gated_step_device_timeout_resumes_ungated(monkeypatch):
    """A host env step slower than the device's wait (XTRL_HOST_GATE_WAIT_MS=30, a 0.25 s step in
    every other episode): the queued step reports that it gave up, the wave resumes on the
    launch-per-step loop from that step (the previous results fed back first) — the rollout still
    reproduces the oracle's reference loop, bootstraps included."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', '1')
    monkeypatch.setenv('XTRL_HOST_GATE', '1')
    monkeypatch.setenv('XTRL_HOST_GATE_WAIT_MS', '30')
    learner, _, oracle = make_learner(depth=2, gates=True, T=9, episodes=6, batch=2)
    _compare_host(learner, oracle, SlowHostLander(at=2, pause=0.25, limit=5), HostLander(limit=5), 9)


@pytest.mark.parametrize('frac,dim', [(None, 48), (2, 48), (None, 256)])
def test_host_env_vectorised_waves_match_oracle(frac, dim, decode_path):
    """A vectorised env of 4 sub-envs over 2 genes x 5 episodes (10 pairs: waves of 4, 4, 2 — the
    last one partial), evolutionary with per-episode reset seeds, truncation at 6 steps (the
    truncation bootstrap step included); decoder and fractal policy bodies (dim 256: the decoder's
    one-launch feed-forward writing the final norm into the 3d-wide heads' input row)."""
    learner, _, oracle = make_learner(depth=2, gates=frac is None, evo=True, T=8, episodes=5, batch=5,
                                      fractal_levels=frac, dim=dim)
    seeds = torch.randint(0, 10 ** 7, (5,), generator=torch.Generator().manual_seed(3))
    _, _, genes, cum, episodes, fitness = _compare_host(learner, oracle, HostLanderVec(4, limit=6),
                                                        HostLander(limit=6), 8, seeds)
    tol(learner.fitness(cum, genes), fitness, 1e-5, 1e-5)


@pytest.mark.parametrize('frac', [None, 2])
def test_host_env_vectorised_truncation_at_max_timesteps(frac):
    """TimeLimit equal to max_timesteps on a vectorised env: every episode that reaches the last
    step is truncated there and bootstraps from the next state's value (xtrl.py:1323-1336 take
    the bootstrap on any truncated, not terminated step)."""
    learner, _, oracle = make_learner(depth=2, gates=frac is None, T=7, episodes=6, batch=3, fractal_levels=frac)
    traj, lens, _, _, episodes, _ = _compare_host(learner, oracle, HostLanderVec(4, limit=7, hazard=0.05),
                                                  HostLander(limit=7, hazard=0.05), 7)
    assert any(ep['boot'] is not None and ep['len'] == 7 for ep in episodes)
    assert bool(torch.isfinite(traj['boot'].cpu()[lens.cpu() == 7]).all())


def test_host_env_learn_with_truncation_bootstrap_matches_oracle():
    """One learning update on a truncating host env: GAE reads the bootstrap value at each
    truncated episode's end (xtrl.py:1323-1336 intent); every minibatch's losses match the
    oracle's learn at 1e-4."""
    learner, _, oracle = make_learner(depth=2, gates=True, T=9, episodes=6, batch=2, seed=5)
    agent = learner.agent
    traj, lens, genes, cum, episodes, fitness = _compare_host(learner, oracle, HostLander(limit=4),
                                                              HostLander(limit=4), 9)
    assert int(torch.isfinite(traj['boot']).sum()) > 0
    agent.learn(traj, lens, genes, None, update=0)
    oracle.learn(episodes, fitness, 0)
    keys = ('loss', 'actor_loss', 'critic_loss', 'autoreg_loss', 'pred_done_loss')
    ours = np.array([[lg[k] for k in keys] for lg in agent.pop_logs()])
    theirs = np.array([[lg[k] for k in keys] for lg in oracle.logs])
    np.testing.assert_allclose(ours, theirs, rtol=1e-4, atol=1e-5)


def test_learner_call_runs_batched_vector_env():
    """train_lander.py's loop (learner(env, n)) on a vectorised env: two updates, finite weights."""
    learner, _, _ = make_learner(depth=1, gates=False, T=8, episodes=8, batch=4)
    learner(HostLanderVec(8, ret=5, limit=6), 2)
    assert learner.agent.step == 2 and torch.isfinite(learner.agent.flat.flat).all()


@pytest.mark.parametrize('fractal', (None, 2))
def test_compact_world_model_heads_match_full_rows(fractal):
    """The world-model heads on the valid rows only (XtrlTrainDesc.Tv = sum(min(lens, n)): the row
    list, the gather, the compact GEMMs and the scatter back) against the same fused step over every
    row (Tv = 0), on a first minibatch with ragged episode lengths: pred and done agree on the valid
    rows and are exactly zero on the padding, the loss agrees, and every gradient tensor — the heads'
    to_pred / to_pred_done weights included — is within 1e-4 of its own scale."""
    learner, env, _ = make_learner(depth=2, gates=fractal is None, T=40, episodes=8, batch=8, hazard=4, dim=64,
                                   fractal_levels=fractal)
    agent = learner.agent
    traj, lens, genes, cum = learner.rollout_device(env, 0, 40)
    fit = learner.fitness(cum, genes)
    lens_h = lens.cpu()
    assert lens_h.min() < lens_h.max(), lens_h   # ragged: the minibatch has padding
    out = {}
    for compact in (True, False):
        agent.heads_compact = compact
        got = {}

        def probe(epoch, mbi, idx, loss, stats, got=got):
            ts = agent._train_step
            b, n = ts.D.b, ts.D.n
            got.update(loss=float(loss.detach()), grad=agent.flat.grad.detach().clone(), n=n,
                       lens=lens_h[idx.cpu()].clamp(max=n), Tv=ts.D.Tv,
                       pred=ts.buf['pred'][:b * n].view(b, n, -1).clone(), done=ts.buf['done'][:b * n].view(b, n).clone())
            raise _Captured()

        with pytest.raises(_Captured):
            agent.learn(traj, lens, genes, fit, update=0, probe=probe)
        agent.step = 0
        out[compact] = got
    cp, fu = out[True], out[False]
    assert cp['Tv'] == int(cp['lens'].sum()) > 0 and fu['Tv'] == 0
    valid = (torch.arange(cp['n'])[None, :] < cp['lens'][:, None]).to(cp['pred'].device)
    assert (cp['pred'][~valid] == 0).all() and (cp['done'][~valid] == 0).all()
    for k in ('pred', 'done'):
        a, b = cp[k][valid], fu[k][valid]
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max()) + 1e-7, k
    assert abs(cp['loss'] - fu['loss']) <= 1e-5 * abs(fu['loss'])
    bad = []
    for name, (a0, a1) in agent.flat.index.items():
        g0, g1 = cp['grad'][a0:a1], fu['grad'][a0:a1]
        own = float(g1.abs().max())
        if float((g0 - g1).abs().max()) > 1e-4 * own + 1e-7:
            bad.append((name, float((g0 - g1).abs().max()), own))
    assert not bad, bad
    assert any('to_pred' in n for n in agent.flat.index)
