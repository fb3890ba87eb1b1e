"""The learn-step row-kernel tests' references, case tables and bounds, settled without a GPU
(tests/learn_row_cases.py): every closed form against torch.autograd in fp64 on the forward reference, the forward
references against the oracle's own modules, the bounds against a plain fp32 restatement, the tables against a
restatement of the launchers' integer arithmetic, and the C ABI of the entry the GPU tests drive (XtrlRowsDesc /
xtrl_learn_rows, ABI 31) with the refusals that return before any launch."""
import ctypes
import re
from pathlib import Path

import pytest
import torch
import torch.nn.functional as F

import learn_row_cases as LC
from gemm_epi_cases import _gen, ln_rows
from oracle import thirdparty as TP

REPO = Path(__file__).resolve().parent.parent
D = torch.float64


def close(a, b, tol=1e-9):
    assert a.shape == b.shape, (a.shape, b.shape)
    err = float((a - b).abs().max())
    assert err <= tol * max(1., float(b.abs().max())), err


def regions(spec, dt=D):
    return {(r.buf, r.c0): r.ref for r in spec.expect(dt) if r.ref is not None}


# ----------------------------------------------------------------------------------------------
# closed forms vs autograd
# ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('rms', [0, 1])
@pytest.mark.parametrize('variant', sorted(LC.LN_BWD_VARIANTS))
@pytest.mark.parametrize('d,T', [(4, 1), (68, 17), (260, 37)])
def test_ln_backward_reference_is_autograd(d, T, rms, variant):
    """dx (+ dres), d gamma and d beta (onto their old values) of y = LN(x) gamma + beta for g = s1 g1 + g2.  The
    reference reads the fp32 (mean, rstd) a forward stored; autograd recomputes them: 1e-6."""
    has_g2, s1, alias, beta = LC.LN_BWD_VARIANTS[variant]
    spec = LC.ln_bwd_spec(d, T, rms, variant)
    B = spec.bufs
    x = B['x'].double().requires_grad_()
    gamma = B['gamma'].double().requires_grad_()
    b_ = torch.zeros(d, dtype=D, requires_grad=True)
    g = s1 * B['g1'][:, :d].double() + (B['g2'][:, :d].double() if has_g2 else 0.)
    ((ln_rows(x, rms)[0] * gamma + b_) * g).sum().backward()
    R = regions(spec)
    old = B['dgb'][0].double()
    close(R[('dx', 0)], x.grad + (B['dx'][:T].double() if alias else 0.), 1e-6)
    close(R[('dgb', 0)], old[:d] + gamma.grad, 1e-6)
    if beta:
        close(R[('dgb', d)], old[d:2 * d] + b_.grad, 1e-6)
    else:
        assert ('dgb', d) not in R


@pytest.mark.parametrize('c', LC.PREP_BWD_CASES[::3] + [c for c in LC.PREP_BWD_CASES if c.qk_norm and c.xpos][:4],
                         ids=lambda c: c.id)
def test_qkv_prep_backward_reference_is_autograd(c):
    """d q | d k (inverse rotation, xPos, the normalise backward with F.normalize's zero-head rule), d v, dvfirst
    and d mix of the forward reference, for every (first_layer, accumulate, mix) mode."""
    spec = LC.prep_bwd_spec(c)
    B, gq3, old = spec.bufs, spec.info['gq3'].double(), spec.info['dvf_old'].double()
    proj = B['proj'].double().clone()
    proj[proj.abs() > 1e29] = 0.            # (the 1e30 padding: never read, zeroed so autograd stays finite)
    proj.requires_grad_()
    vf = B['vfirst'].double().clone()
    vf[vf.abs() > 1e29] = 0.
    vf.requires_grad_()
    (LC.prep_forward(c, proj, vf, D) * gq3).sum().backward()
    d3, dvf, dmix, zero = LC.prep_backward(c, B['proj'], B['vfirst'], spec.info['gq3'], spec.info['dvf_old'], D)
    want = proj.grad[:, :c.nq3].clone()
    if c.mix == 'off' and c.first_layer and c.accumulate:
        want[:, c.I + c.Ikv:] += old
    scale = d3.abs().clamp_min(1.)
    assert float(((d3 - want).abs() / scale).max()) < 1e-9
    if c.mix != 'off':
        close(dvf, vf.grad[:, c.I + c.Ikv:c.nq3] + (old if c.accumulate else 0.))
        close(dmix, proj.grad[:, c.mix_col:c.mix_col + c.Hkv])
    else:
        assert dvf is None and dmix is None
    if c.qk_norm:   # the all-zero heads take g / 1e-12 (the clamp of F.normalize passes no gradient to the norm)
        assert int(zero.sum()) == 2 * c.dh
        assert float(d3[zero].abs().max()) > 1e3
    # the regions: d v keeps its input bits where the kernel does not touch it
    R = regions(spec)
    touched = c.mix != 'off' or (c.first_layer and c.accumulate)
    assert R[('dproj', 0)].shape[1] == (c.nq3 if touched else c.I + c.Ikv)


@pytest.mark.parametrize('n,d', [(1, 48), (17, 100), (130, 48)])
def test_causal_mean_reverse_reference_is_autograd_of_the_forward(n, d):
    fwd, rev = LC.causal_mean_spec(n, d, 0, 0), LC.causal_mean_spec(n, d, 1, 1)
    x = fwd.bufs['src'][:, :d].double().requires_grad_()
    y = (x.reshape(2, n, d).cumsum(1) / torch.arange(1, n + 1, dtype=D)[None, :, None]).reshape(2 * n, d)
    close(regions(fwd)[('dst', 0)], y.detach())
    up = rev.bufs['src'][:, :d].double()
    (y * up).sum().backward()
    close(regions(rev)[('dst', 0)], x.grad + rev.bufs['add'][:, :d].double())


@pytest.mark.parametrize('a', [(5, 48, 37, 1, 0), (32, 260, 37, 0, 0), (1, 48, 1, 1, 0), (5, 48, 300, 1, 1)], ids=str)
def test_embed_grad_reference_is_the_gradient_of_the_embed_reference(a):
    A, d, T, prev, _ = a
    spec = LC.embed_grad_spec(*a)
    B = spec.bufs
    W = torch.zeros(A, d, dtype=D, requires_grad=True)
    emb = lambda idx: torch.where((idx >= 0)[:, None], W[idx.clamp_min(0).long()], torch.zeros((), dtype=D))   # noqa: E731
    loss = (emb(B['next']) * B['g2'][:, :d].double()).sum()
    if prev:
        loss = loss + (emb(B['prev']) * B['g1'][:, :d].double()).sum()
    loss.backward()
    close(regions(spec)[('dst', 0)].reshape(A, d), B['dst'][0, :A * d].double().reshape(A, d) + W.grad)


@pytest.mark.parametrize('a', [(1, 1, 48, 1, 0), (3, 17, 100, 5, 0), (9, 130, 48, 5, 1), (3, 7, 48, 1, 1)], ids=str)
def test_latent_grad_reference_is_the_gradient_of_the_gene_embedding(a):
    b, n, d, G, packed = a
    spec = LC.latent_grad_spec(*a)
    B = spec.bufs
    ep = B['ep_off'] if packed else torch.arange(b + 1) * n
    gene = torch.repeat_interleave(torch.arange(b), (ep[1:] - ep[:-1]).long())
    w = torch.zeros(d, G, dtype=D, requires_grad=True)
    bias = torch.zeros(d, dtype=D, requires_grad=True)
    lat_e = B['latent'].double() @ w.t() + bias
    (lat_e[gene] * B['dac'][:, 2 * d:3 * d].double()).sum().backward()
    R = regions(spec)
    close(R[('dw', 0)].reshape(d, G), B['dw'][0, :d * G].double().reshape(d, G) + w.grad)
    close(R[('db', 0)].reshape(d), B['db'][0, :d].double() + bias.grad)


# ----------------------------------------------------------------------------------------------
# forward references vs the oracle's modules
# ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('a', [a for a in LC.LN_FWD_CASES if a[1] in (1, 37)][::3], ids=str)
def test_ln_forward_reference_is_the_oracle_norm(a):
    d, T, rms, y2 = a
    spec = LC.ln_fwd_spec(*a)
    mod = (TP.RMSNorm(d) if rms else TP.LayerNorm(d)).double()
    with torch.no_grad():
        (mod.g if rms else mod.gamma).copy_(spec.bufs['gamma'].double())
        want = mod(spec.bufs['x'].double())
    close(regions(spec)[('y1', 0)], want)


@pytest.mark.parametrize('c', [c for c in LC.EMBED_CASES if c.ln][::5], ids=lambda c: c.id)
def test_embed_ln_reference_is_the_oracle_norm_of_x0(c):
    spec = LC.embed_spec(c)
    R = regions(spec)
    mod = (TP.RMSNorm(c.d) if c.rms else TP.LayerNorm(c.d)).double()
    with torch.no_grad():
        (mod.g if c.rms else mod.gamma).copy_(spec.bufs['ln_g'].double())
        close(R[('xn', 0)], mod(R[('x0', 0)]))


@pytest.mark.parametrize('c', [c for c in LC.PREP_CASES if not c.packed], ids=lambda c: c.id)
def test_qkv_prep_forward_reference_is_the_oracle_attention_prologue(c):
    """F.normalize, RotaryEmbedding (+ xpos), apply_rotary and lerp of oracle.thirdparty on the padded cases
    (positions 0 .. n - 1, so the oracle's max_pos // 2 is n // 2).  The oracle's angle and xPos factor are fp32
    (as x-transformers'), widened here; the factor's fp32 power is held to 2e-6 of the result."""
    B = LC.prep_inputs(c)[0]
    ref = LC.prep_forward(c, B['proj'], B['vfirst'], D)
    rope = TP.RotaryEmbedding(c.rot, use_xpos=c.xpos > 0., scale_base=c.xpos or 512.)
    pos = torch.arange(c.n)
    keep = min(c.rot, c.dh)
    freqs = rope(pos)[:, :keep].double().repeat(c.b, 1)
    xp = rope.xpos(pos)
    xp = 1. if xp is None else xp[:, :keep].double().repeat(c.b, 1)
    proj = B['proj'].double()
    q = proj[:, :c.I].reshape(c.T, c.H, c.dh)
    k = proj[:, c.I:c.I + c.Ikv].reshape(c.T, c.Hkv, c.dh)
    if c.qk_norm:
        q, k = F.normalize(q, dim=-1), F.normalize(k, dim=-1)
    un = lambda t: t if not torch.is_tensor(t) else t[:, None, :]   # noqa: E731
    q = TP.apply_rotary(q, un(freqs), un(xp))
    k = TP.apply_rotary(k, un(freqs), un(xp) ** -1.)
    v = proj[:, c.I + c.Ikv:c.nq3]
    if c.mix != 'off':
        m = torch.sigmoid(proj[:, c.mix_col:c.mix_col + c.Hkv]).repeat_interleave(c.dh, 1)
        v = v.lerp(B['vfirst'][:, c.I + c.Ikv:c.nq3].double(), m)
    want = torch.cat([q.reshape(c.T, -1), k.reshape(c.T, -1), v], 1)
    assert float(((ref - want).abs() / want.abs().clamp_min(1.)).max()) < 2e-6


# ----------------------------------------------------------------------------------------------
# bounds: the fp32 restatement
# ----------------------------------------------------------------------------------------------


def test_fp32_restatement_within_a_quarter_of_each_bound():
    """Every case's formulas in plain fp32 torch (sums: sequential) against fp64: each sum family's worst error in
    units of 2^-24 sum |terms| times four is at most its constant, and every output of every case sits inside a
    quarter of its bound.  The restatement also goes through `verify` as the kernels' outputs will."""
    share, unit = {}, {}
    for spec in LC.all_specs():
        r64, r32 = spec.expect(D), spec.expect(torch.float32)
        after = {k: spec.bufs[k].clone() for k in spec.outs}
        for a, b in zip(r64, r32):
            if a.ref is None:
                continue
            ref = b.ref.reshape(b.ref.shape[0], -1) if b.ref.dim() > 1 else b.ref.reshape(1, -1)
            R, C = ref.shape
            after[a.buf][a.r0:a.r0 + R, a.c0:a.c0 + C] = ref.to(after[a.buf].dtype)
            if a.bound is None:
                continue
            err = (ref.double() - a.ref.double().reshape(R, C)).abs()
            key = f'{spec.op} {a.fam} {a.buf}'
            share[key] = max(share.get(key, 0.), float((err / a.bound.reshape(R, C)).nan_to_num(0.).max()))
            if a.unit is not None:
                unit[a.fam] = max(unit.get(a.fam, 0.), float((err / a.unit.reshape(R, C)).nan_to_num(0.).max()))
        LC.verify(spec, after, r64)
    for k, v in sorted(share.items()):
        print(f'\n  fp32 restatement / bound  {k:40s} {v:.3f}', end='')
    for k, v in sorted(unit.items()):
        print(f'\n  {k:12s} {v:.2f} x 2^-24 x sum |terms|   (C = {LC.C_SUM[k]:g})', end='')
    assert set(unit) == set(LC.C_SUM)
    for k, v in unit.items():
        assert 4 * v <= LC.C_SUM[k] < 4 * v + 1.5, (k, v)     # four times the measured, rounded up (not more)
    bad = {k: v for k, v in share.items() if v > 0.25}
    assert not bad, bad


def test_verify_rejects_a_wrong_element_and_a_written_guard():
    spec = LC.colsum_spec(17, 17, 1)
    r64 = spec.expect(D)
    good = {k: spec.bufs[k].clone() for k in spec.outs}
    good['dst'][0, :17] = r64[0].ref.float()
    LC.verify(spec, good, r64)
    for where, value in (((0, 3), float(r64[0].ref[3]) + 1e-3), ((0, 18), 0.), ((0, 2), float('inf'))):
        bad = {k: v.clone() for k, v in good.items()}
        bad['dst'][where] = value
        with pytest.raises(AssertionError):
            LC.verify(spec, bad, r64)
    bad = {k: v.clone() for k, v in good.items()}
    bad['part'][0, spec.part_floats] = 0.       # one float past the workspace
    with pytest.raises(AssertionError):
        LC.verify(spec, bad, r64)


# ----------------------------------------------------------------------------------------------
# input conditions and the launchers' integer arithmetic
# ----------------------------------------------------------------------------------------------


def test_tables_reach_the_branches_they_are_there_for():
    # embeddings: both kernels at every d they take, every S (8: the <8> instantiation), the action counts, -1 among
    # the actions, evolutionary x packed, two 32-token blocks with a ragged last 8-token batch, one token
    for ln, ds in ((0, LC.EMB_D_BOTH + LC.EMB_D_PLAIN), (1, LC.EMB_D_BOTH)):
        mine = [c for c in LC.EMBED_CASES if c.ln == ln]
        assert {c.d for c in mine} == set(ds) and max(ds) <= (256 if ln else 512)
        assert {c.S for c in mine} == {1, 8, 13, 32}
        assert {c.A for c in mine if not c.cont} == {1, 4, 5, 9, 32} and {c.A for c in mine if c.cont} == {1, 6}
        assert {(c.evo, c.packed) for c in mine} == {(0, 0), (0, 1), (1, 0), (1, 1)}
        assert {c.keep for c in mine} == {0., 1.} and {c.T for c in mine} == {1, 45}
        assert {c.rms for c in mine} == ({0, 1} if ln else {0})
        assert all(c.in_dim > 3 * c.d for c in mine)
    assert -(-45 // 32) == 2 and 45 % 8 == 5
    c = next(c for c in LC.EMBED_CASES if c.packed and c.evo)
    rows = LC.embed_rows_list(c).long()
    assert bool(((rows // c.n) != (torch.arange(c.T) // c.n)).any()) and int(rows.max()) < c.b * c.n
    spec = LC.embed_spec(next(c for c in LC.EMBED_CASES if not c.cont and c.T == 45))
    assert int(spec.bufs['prev_a'].min()) == -1 and int(spec.bufs['next_a'].min()) == -1
    # LayerNorm: every DPL instantiation, a ragged last 64-column group, one block / a block and a row / three
    assert {LC.ln_dpl(d) for d in LC.LN_DS} == {1, 2, 4, 8} and any(d % 64 for d in LC.LN_DS) and max(LC.LN_DS) == 512
    assert {-(-T // LC.LN_ROWS) for T in LC.LN_TS} == {1, 2, 3} and {T % LC.LN_ROWS for T in LC.LN_TS} == {0, 1, 5}
    assert {(d, T, rms, v) for d, T, rms, v in LC.LN_BWD_CASES} == \
        {(d, T, rms, v) for d in LC.LN_DS for T in LC.LN_TS for rms in (0, 1) for v in LC.LN_BWD_VARIANTS}
    assert {a[3] for a in LC.LN_FWD_CASES} == {0, 1}
    # rotary / mix: pair counts (a ragged second block, one block with idle lanes, six full blocks), rot_dim on
    # both sides of dh, both forms, positions to 499
    for cases in (LC.PREP_CASES, LC.PREP_BWD_CASES):
        assert {80, 240, 768} <= {c.P for c in cases}
        assert {(c.rot < c.dh, c.rot == c.dh, c.rot > c.dh) for c in cases} == {(1, 0, 0), (0, 1, 0), (0, 0, 1)}
        assert {c.dh for c in cases} == {16, 32, 64} and {c.packed for c in cases} == {0, 1}
        assert {c.xpos for c in cases} == set(LC.PREP_XPOS) and {c.qk_norm for c in cases} == {0, 1}
        assert {(c.qk_norm, c.xpos > 0, c.mix != 'off') for c in cases} == {(a, b, m) for a in (0, 1) for b in (0, 1)
                                                                              for m in (0, 1)}
    # xPos: base 16 on the padded form, 512 on the packed one; the factor stays O(1)
    for c in LC.PREP_CASES + LC.PREP_BWD_CASES:
        assert c.xpos == (0. if c.xpos == 0. else (512. if c.packed else 16.))
        xf = LC.rotary_tables(c, D)[2]
        assert 0.5 < float(xf.min()) and float(xf.max()) < 1.9
        assert c.xpos == 0. or float(xf.max()) > 1.05
    assert {c.mix for c in LC.PREP_CASES} == set(LC.PREP_MIX)
    assert {(c.first_layer, c.accumulate, int(c.mix != 'off')) for c in LC.PREP_BWD_CASES} == set(LC.PREP_BWD_MODES)
    assert {c.mix for c in LC.PREP_BWD_CASES} == set(LC.PREP_MIX)
    pk = next(c for c in LC.PREP_CASES if c.packed)
    assert int(LC.prep_positions(pk).max()) == 499 == pk.n - 1 and int(LC.prep_rows(pk)[0].max()) == 999
    # gather / scatter forms, valid-row lens
    assert {LC.move_spec('gather', *a).info['vec4'] for a in LC.MOVE_CASES} == {True, False}
    lens = torch.cat([LC.valid_lens(b, n, k) for (b, n, k, _, _) in LC.VALID_CASES if b == 5])
    assert {0, 300, 304, -3} <= set(lens.tolist())
    assert {ep for *_, ep in LC.VALID_CASES} == {0, 1}
    assert any(Tv == int(LC.valid_lens(b, n, k).clamp(0, n).sum()) - 3 for (b, n, k, Tv, _) in LC.VALID_CASES)
    # causal mean: one step per group, 16 groups and a tail, nine steps per group
    assert {-(-n // LC.CM_G) for n, *_ in LC.CAUSAL_CASES} == {1, 2, 9}


@pytest.mark.parametrize('c', [c for c in LC.PREP_CASES + LC.PREP_BWD_CASES if c.qk_norm or c.mix != 'off'][::4],
                         ids=lambda c: c.id)
def test_prep_inputs_hold_the_zero_heads_and_both_sides_of_the_lerp_switch(c):
    B = LC.prep_inputs(c)[0]
    if c.qk_norm:
        nq = LC.head_norms(B['proj'][:, :c.I].double(), c.dh)
        nk = LC.head_norms(B['proj'][:, c.I:c.I + c.Ikv].double(), c.dh)
        assert int((nq == 0).sum()) == 1 and int((nk == 0).sum()) == 1
        assert float(nq[nq > 0].min()) > 1e-3 and float(nk[nk > 0].min()) > 1e-3
    if c.mix != 'off':
        m = torch.sigmoid(B['proj'][:, c.mix_col:c.mix_col + c.Hkv])
        assert set(B['proj'][:, c.mix_col:c.mix_col + c.Hkv].unique().tolist()) == \
            set(torch.tensor(LC.MIX_PRE).tolist())
        assert bool((m.abs() < 0.5).any()) and bool((m.abs() >= 0.5).any())
        assert c.mix_col == c.nq3 + (c.I if c.mix == 'gate' else 0) and c.mix_col + c.Hkv <= c.n_qkv


def test_colsum_and_queue_arithmetic():
    assert LC.colsum_chunks(4112) == (257, 16) and 257 > 3 * LC.CS_G          # the final kernel's four-chain loop
    assert min(1024, 16400 // 16) == 1024 and LC.colsum_chunks(16400)[1] == 17   # the 1024-chunk cap: 17-row chunks
    assert LC.colsum_chunks(1) == (1, 1) and LC.colsum_chunks(15) == (1, 15) and LC.colsum_chunks(17) == (1, 17)
    assert max(r * c for r, c, _ in LC.COLSUM_CASES) <= 4112 * 300 and (16400, 17, 1) in LC.COLSUM_CASES
    name, jobs, cap = LC.QUEUE_CASES[0]
    assert LC.queue_flushes(jobs, cap) == [[0, 1, 2]]
    name, jobs, cap = LC.QUEUE_CASES[1]
    assert len(jobs) == 17 and LC.queue_flushes(jobs, cap) == [list(range(16)), [16]]   # the slots are full
    name, jobs, cap = LC.QUEUE_CASES[2]
    assert LC.queue_flushes(jobs, cap) == [[0, 1], [2]] and max(a * b for a, b in jobs) == cap   # the workspace is
    # embed_grad: every MAXA instantiation; the capped cases' chunk count comes from the workspace
    assert {LC.embed_grad_chunks(T, A, d, 1 << 30)[2] for A, d, T, *_ in LC.EMBED_GRAD_CASES} == {4, 8, 32}
    for A, d, T, prev, capped in LC.EMBED_GRAD_CASES:
        spec = LC.embed_grad_spec(A, d, T, prev, capped)
        chunks, chunk_rows, _ = LC.embed_grad_chunks(T, A, d, spec.part_floats)
        assert chunks * A * d <= spec.part_floats
        if capped:
            assert chunks == 5 < T // 16 and chunk_rows == 60
        else:
            assert chunks == LC.colsum_chunks(T)[0]
    # latent grad: nine steps per group at n = 130 (one 8-wide batch and a tail); an empty packed episode
    assert -(-130 // 16) == 9
    ep = LC.latent_ep_off(3, 17)
    assert 0 in (ep[1:] - ep[:-1]).tolist() and any(p for *_, p in LC.LATENT_GRAD_CASES)


# ----------------------------------------------------------------------------------------------
# the C ABI and the refusals
# ----------------------------------------------------------------------------------------------


def test_learn_rows_abi():
    from xtrl_amd import _lib
    text = (REPO / 'include' / 'xtrl_hip.h').read_text()
    abi = int(re.search(r'#define XTRL_ABI_VERSION (\d+)', text).group(1))
    assert abi == _lib.ABI_VERSION >= 31
    lib = _lib.load()
    assert lib.xtrl_abi_version() == abi and hasattr(lib, 'xtrl_learn_rows')
    assert int(lib.xtrl_struct_size(b'XtrlRowsDesc')) == ctypes.sizeof(_lib.RowsDesc)
    assert int(lib.xtrl_struct_size(b'XtrlColsumJob')) == ctypes.sizeof(_lib.ColsumJob)
    ops = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define XTRL_ROWS_(\w+) (\d+)', text)}
    assert ops == LC.OP == _lib.ROWS
    body = re.search(r'typedef struct XtrlRowsDesc \{(.*?)\n\} XtrlRowsDesc;', text, re.S).group(1)
    fields = re.findall(r'(\w+)(?:\[(\d+)\])?;', body)
    assert [n for n, _ in fields] == [n.rstrip('_') for n, _ in _lib.RowsDesc._fields_]
    sizes = {n: int(k) for n, k in fields if k}
    assert sizes == {'in': 16, 'out': 6, 'ld': 4, 'n': 12, 'f': 2}
    for spec in (LC.embed_spec(LC.EMBED_CASES[0]), LC.prep_bwd_spec(LC.PREP_BWD_CASES[0])):   # the widest users
        assert len(spec.in_) <= 16 and len(spec.out) <= 6 and len(spec.ld) <= 4 and len(spec.n) <= 12


def test_learn_rows_refusals_reach_no_kernel():
    """The argument checks are host code ahead of any launch: reachable without a GPU (a NULL stream, operands never
    read)."""
    from xtrl_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value

    def call(op, in_=(), out=(), ld=(), n=(), f=(), part_floats=0, jobs=()):
        d = _lib.RowsDesc()
        for i in in_:
            d.in_[i] = p
        for i in out:
            d.out[i] = p
        for i, v in enumerate(ld):
            d.ld[i] = v
        for i, v in enumerate(n):
            d.n[i] = v
        for i, v in enumerate(f):
            d.f[i] = v
        d.part, d.part_floats = p, part_floats
        arr = (_lib.ColsumJob * max(1, len(jobs)))()
        for j, (chunks, cols) in enumerate(jobs):
            arr[j].part, arr[j].dst, arr[j].chunks, arr[j].cols = p, p, chunks, cols
        if jobs:
            d.jobs, d.n_jobs = arr, len(jobs)
        rc = lib.xtrl_learn_rows(ctypes.byref(d), LC.OP[op] if isinstance(op, str) else op, None)
        return rc, lib.xtrl_last_error().decode()
    assert lib.xtrl_learn_rows(None, 0, None) == 1 and 'null descriptor' in lib.xtrl_last_error().decode()
    rc, msg = call(99)
    assert rc == 1 and 'unknown op 99' in msg
    rc, msg = call(-1)
    assert rc == 1 and 'unknown op' in msg
    rc, msg = call('LN_FWD', in_=(0, 1), out=(0, 2), ld=(516, 0), n=(4, 516, 0))
    assert rc == 1 and 'd = 516' in msg
    rc, msg = call('LN_BWD', in_=(0, 2, 3, 4), out=(0, 1), ld=(516, 0), n=(4, 516, 0), f=(1.,), part_floats=1 << 20)
    assert rc == 1 and 'd = 516' in msg
    rc, msg = call('LN_BWD', in_=(0, 2, 3, 4), out=(0, 1), ld=(64, 0), n=(40, 64, 0), f=(1.,), part_floats=2 * 64)
    assert rc == 1 and 'workspace too small' in msg      # three 16-row blocks need 3 x 64
    # d beta not adjacent to d gamma
    d = _lib.RowsDesc()
    for i in (0, 2, 3, 4):
        d.in_[i] = p
    d.out[0], d.out[1], d.out[2] = p, p, p + 4 * 8
    d.ld[0], d.n[0], d.n[1], d.f[0], d.part, d.part_floats = 4, 4, 4, 1., p, 64
    assert lib.xtrl_learn_rows(ctypes.byref(d), LC.OP['LN_BWD'], None) == 1
    assert 'must be adjacent' in lib.xtrl_last_error().decode()
    # embed_ln past the width one workgroup holds; too many discrete actions; too wide a state
    emb = dict(in_=(0, 1, 2, 4, 5, 6, 10, 11, 12), out=(0, 1, 2, 3, 4), f=(1.,))
    rc, msg = call('EMBED', n=(4, 2, 8, 4, 260, 784, 0, 0, 0, 1), **emb)
    assert rc == 1 and 'embed_ln needs d <= 256' in msg
    rc, msg = call('EMBED', n=(4, 2, 8, 4, 516, 2000, 0, 0, 0, 0), **emb)
    assert rc == 1 and 'd = 516' in msg
    rc, msg = call('EMBED', n=(4, 2, 8, 33, 48, 148, 0, 0, 0, 0), **emb)
    assert rc == 1 and '33 discrete actions' in msg
    rc, msg = call('EMBED', n=(4, 2, 33, 4, 48, 148, 0, 0, 0, 0), **emb)
    assert rc == 1 and 'state_dim 33' in msg
    for dh in (8, 24, 128):
        for op in ('QKV_PREP', 'QKV_PREP_BWD'):
            rc, msg = call(op, in_=(0, 2), out=(0, 1), ld=(3 * dh + 2, 3 * dh + 4),
                           n=(4, 2, 2, 1, 1, dh, dh, -1, 0, 0, 0))
            assert rc == 1 and f'dh = {dh}' in msg
    rc, msg = call('QKV_PREP', in_=(0, 2, 3), out=(0,), ld=(50, 52), n=(70000, 500, 2, 1, 1, 16, 16, -1, 0))
    assert rc == 1 and 'exceed the grid' in msg
    rc, msg = call('COLSUM', in_=(0,), out=(0,), ld=(20, 0), n=(4112, 17), f=(1.,), part_floats=257 * 17 - 1)
    assert rc == 1 and 'workspace too small' in msg
    rc, msg = call('EMBED_GRAD', in_=(2, 3), out=(0,), ld=(0, 100), n=(37, 48, 5), part_floats=5 * 48 - 1)
    assert rc == 1 and 'workspace too small' in msg
    rc, msg = call('LATENT_GRAD', in_=(0, 2), out=(0, 1), ld=(148,), n=(96, 3, 7, 48, 5), part_floats=3 * 48 - 1)
    assert rc == 1 and 'workspace too small' in msg
    rc, msg = call('COLSUM_QUEUE', part_floats=100, jobs=((1, 4), (11, 10)))
    assert rc == 1 and 'job 1 (11 x 10) exceeds the workspace' in msg
    rc, msg = call('VALID_ROWS', in_=(0,), out=(0, 1), n=(4097, 2, 3))
    assert rc == 1 and 'b = 4097' in msg
