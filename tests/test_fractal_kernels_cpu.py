"""CPU companion of test_fractal_kernels_gpu.py: settles the fp64 references of
fractal_kernel_cases.py against the oracle's own functions (fractal_ref._attention with a key mask,
torch.nn.LayerNorm, ref_port.safe_embed, ref_port.continuous_params) and the case tables against the
edges they are there for, without a GPU."""
import math

import pytest
import torch

import fractal_kernel_cases as C
from oracle import fractal_ref as FR
from oracle import ref_port as R


# ----------------------------------------------------------------------------------------------
# attention
# ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('case', C.ATTN_CASES[:3] + C.ATTN_CASES[5:], ids=C.attn_id)
def test_attention_reference_is_the_oracles_attention_with_a_key_mask(case):
    """fractal_ref._attention on the buffer's rows with selection matrices for to_q / to_k / to_v and the
    identity for to_out is the same softmax; its masked scores take the finite fill, which at lens >= 1 gives
    the same probabilities as -inf."""
    c = case
    buf, lens = C.attn_inputs(c)
    I = c.I   # noqa: E741
    x = buf[:, :3 * I].double().reshape(c.b, c.n, 3 * I)
    eye = torch.eye(3 * I, dtype=torch.float64)
    sd = {'a.to_q.weight': eye[:I], 'a.to_k.weight': eye[I:2 * I], 'a.to_v.weight': eye[2 * I:],
          'a.to_out.weight': torch.eye(I, dtype=torch.float64)}
    key_mask = torch.arange(c.n)[None, :] < lens.long()[:, None]
    theirs = FR._attention(x, x, sd, 'a', c.H, c.dh, key_mask)
    o, lse = C.attn_reference(c)
    assert lse.shape == (c.b, c.H, c.n) and bool(torch.isfinite(o).all()) and bool(torch.isfinite(lse).all())
    torch.testing.assert_close(C.tokens_of(o).reshape(c.b, c.n, I), theirs, rtol=1e-12, atol=1e-14)


def test_attention_reference_rows_past_len_attend_the_valid_keys_and_causal_masks_the_future():
    c = C.ATTN_CASES[2]
    buf, lens = C.attn_inputs(c)
    q, k, v = C.attn_heads(c, buf)
    o, _ = C.attn_ref(q, k, v, lens, 0.25)
    # the episode of one step: every row, the padded ones included, is that key's value
    assert lens[2] == 1 and torch.equal(o[2], v[2, :, :1].double().expand(-1, c.n, -1))
    # changing a masked key or value changes nothing
    k2, v2 = k.clone(), v.clone()
    k2[1, :, 64], v2[1, :, 64] = 7., -7.
    assert lens[1] == 64 and torch.equal(C.attn_ref(q, k2, v2, lens, 0.25)[0], o)
    oc, _ = C.attn_ref(q, k, v, lens, 0.25, causal=True)
    assert torch.equal(oc[:, :, 0], v[:, :, 0].double())           # row 0 sees key 0 alone
    assert torch.equal(oc[0, :, c.n - 1], o[0, :, c.n - 1])        # the last row of a full episode sees all keys
    assert not torch.equal(oc[0, :, 1], o[0, :, 1])


def test_attention_cases_hold_the_edges():
    cs = C.ATTN_CASES
    assert [(c.b, c.H, c.n, c.dh, c.lens) for c in cs] == [
        (2, 2, 1, 16, (1, 1)), (3, 2, 64, 16, (64, 1, 37)), (3, 2, 65, 16, (65, 64, 1)),
        (3, 3, 130, 32, (130, 65, 128)), (2, 2, 130, 64, (130, 63)), (2, 4, 70, 16, (70, 5))]
    assert all(min(c.lens) >= 1 and max(c.lens) == c.n and len(c.lens) == c.b for c in cs + [C.ATTN_CAUSAL_CASE])
    # a masked key in a second key tile; a second key tile skipped (len <= 64 < n); more than one tile at dh = 32, 64
    assert any(c.n > C.TK and any(C.TK < ln < c.n for ln in c.lens) for c in cs)
    assert any(c.n > C.TK and any(ln <= C.TK for ln in c.lens) for c in cs)
    assert {c.dh for c in cs if c.n > 2 * C.TK} >= {32, 64}
    assert any(c.n % C.TK == 1 for c in cs) and any(c.H % 2 for c in cs)
    pads = [c for c in cs if c.pad]
    assert pads and all(c.ld == 3 * c.I + 4 and c.ldo == c.I + 4 for c in pads)
    cc = C.ATTN_CAUSAL_CASE
    assert (cc.b, cc.H, cc.n, cc.dh, cc.lens, cc.causal) == (2, 2, 130, 16, (130, 40), True)
    for c in cs:
        buf, _ = C.attn_inputs(c)
        assert buf.shape == (c.b * c.n, c.ld) and bool(torch.isfinite(buf[:, :3 * c.I]).all())
        assert bool(torch.isnan(buf[:, 3 * c.I:]).all())


# ----------------------------------------------------------------------------------------------
# row kernels
# ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('case', C.LN_CASES, ids=C.ln_id)
def test_layernorm_reference_is_torch_layernorm_in_fp64(case):
    c = case
    x, r, gamma, beta = C.ln_inputs(c)
    ln = torch.nn.LayerNorm(c.D, eps=c.eps, elementwise_affine=True, bias=c.beta, dtype=torch.float64)
    with torch.no_grad():
        ln.weight.copy_(gamma.double())
        if c.beta:
            ln.bias.copy_(beta.double())
        s = x if r is None else x + r.repeat_interleave(c.r_rep, 0)[:c.M]
        theirs = ln(s.double())
    ours = C.ln_reference(c)
    assert r is None or r.shape[0] == -(-c.M // c.r_rep)
    torch.testing.assert_close(ours, theirs, rtol=1e-12, atol=1e-13)
    if c.kind == 'const':
        want = beta.double() if c.beta else torch.zeros(c.D, dtype=torch.float64)
        assert torch.equal(ours[C.LN_CONST_ROW], want)
        # the constant's row sum and mean are exact in fp32
        assert float(x[C.LN_CONST_ROW].sum()) == C.LN_CONST * c.D and float(x[C.LN_CONST_ROW].sum() / c.D) == C.LN_CONST


def test_layernorm_offset_case_tells_one_pass_from_two_pass_at_the_common_bound():
    """Rows N(16, 1) at D = 1024: an fp32 two-pass LayerNorm stays inside 1e-5 + 1e-5 |ref| of fp64, the
    one-pass E[x^2] - mean^2 form does not."""
    c = next(c for c in C.LN_CASES if c.kind == 'offset')
    assert (c.D, c.r) == (1024, None)
    x, _, gamma, beta = C.ln_inputs(c)
    ref = C.ln_reference(c)
    mean = x.mean(-1, keepdim=True)
    two = (x - mean) / (((x - mean) ** 2).mean(-1, keepdim=True) + c.eps).sqrt() * gamma + beta
    one = (x - mean) / (((x * x).mean(-1, keepdim=True) - mean * mean) + c.eps).sqrt() * gamma + beta
    bound = 1e-5 + 1e-5 * ref.abs()
    assert bool(((two.double() - ref).abs() <= bound).all())
    assert bool(((one.double() - ref).abs() > bound).any())


def test_layernorm_cases_hold_the_edges():
    cs = C.LN_CASES
    assert {c.D for c in cs} == {48, 64, 65, 256, 1000, 1024} and {c.M for c in cs} >= {1, 5, 9}
    assert max(c.D for c in cs) == C.LN_MAX_D
    given = [c for c in cs if c.r == 'given' and c.beta and c.kind == 'randn']
    assert {c.D for c in given} == {48, 64, 65, 256, 1000, 1024} and {c.M for c in given} == {1, 5, 9}
    rep = [c for c in cs if c.r == 'rep']
    assert all(c.r_rep == 3 for c in rep) and {c.M for c in rep} >= {7, 9}   # M = 7: the last residual row serves one row
    assert any(c.r is None for c in cs) and any(not c.beta for c in cs) and {c.eps for c in cs} == {1e-5, 1e-3}
    assert any(c.r is None and not c.beta for c in cs)
    assert {c.kind for c in cs} == {'randn', 'offset', 'const'}
    assert all(c.r_rep == 1 for c in cs if c.r != 'rep')


def test_row_kernel_cases_hold_the_edges():
    assert C.ROWS_ADD_CASES == [(1, 48), (5, 64), (7, 65), (4, 256)]
    x, v = C.rows_add_inputs(7, 65)
    assert torch.equal(C.rows_add_ref(None, v, 7), v[None].expand(7, -1)) and torch.equal(C.rows_add_ref(x, v, 7), x + v)
    assert C.SEQ_MEAN_CASES == [(1, 1, 48), (3, 23, 300), (2, 70, 257)]
    assert any(D > 256 for _, _, D in C.SEQ_MEAN_CASES) and any(n == 1 for _, n, _ in C.SEQ_MEAN_CASES)
    assert C.WM_POST_CASES == [(1, 1), (5, 9), (300, 3)] and 300 * 3 > 256
    assert C.SAFE_EMBED_ACTIONS == (-1, 0, 4, 2, -1, 4, 1) and max(C.SAFE_EMBED_ACTIONS) == C.SAFE_EMBED_A - 1
    assert C.SAFE_EMBED_DS == [48, 65]
    assert C.GEMM_SHAPES == [(1, 5, 8), (37, 100, 96), (130, 257, 48)] and len(C.GEMM_FORMS) == 5


def test_seq_mean_bound_holds_a_sequential_fp32_sum_with_room():
    """At n = 70 a sequential fp32 sum and its division sit well inside n 2^-24 mean |x|; at n = 1 the mean is x."""
    B, n, D = C.SEQ_MEAN_CASES[2]
    x = C.seq_mean_inputs(B, n, D)
    ref, bound = C.seq_mean_ref(x, B, n)
    s = torch.zeros(B, D)
    for i in range(n):
        s = s + x.reshape(B, n, D)[:, i]
    err = ((s / n).double() - ref).abs()
    assert bool((err <= bound).all()) and float((bound / err.clamp(min=1e-30)).min()) > 4.
    x1 = C.seq_mean_inputs(1, 1, 48)
    assert torch.equal(C.seq_mean_ref(x1, 1, 1)[0], x1.double())


@pytest.mark.parametrize('D', C.SAFE_EMBED_DS)
def test_safe_embed_reference_is_the_oracles(D):
    table, actions = C.safe_embed_inputs(D)
    ours = C.safe_embed_ref(table, actions)
    assert torch.equal(ours, R.safe_embed(table, actions.long()))
    assert torch.equal(ours[2], table[C.SAFE_EMBED_A - 1]) and float(ours[0].abs().max()) == 0.


@pytest.mark.parametrize('M,P', C.WM_POST_CASES)
def test_wm_post_reference_is_the_oracles_mean_variance(M, P):
    raw, logit = C.wm_post_inputs(M, P)
    mv, done = C.wm_post_ref(raw, logit)
    mean, var = R.continuous_params(raw.double())
    assert mv.shape == (2, M, P) and torch.equal(mv[0], mean) and torch.equal(mv[1], var)
    assert torch.equal(mv[0].float(), raw[:, 0::2])                  # the mean is the input itself
    assert torch.equal(done, torch.sigmoid(logit.double())) and bool(torch.isfinite(mv).all())
    lv = raw[:, 1::2].reshape(-1).tolist()
    k = min(M * P, len(C.WM_LOGVAR_EDGES))
    assert lv[:k] == list(C.WM_LOGVAR_EDGES[:k]) and logit.tolist()[:min(M, 5)] == list(C.WM_DONE_EDGES[:min(M, 5)])
    if M * P >= 5:
        # saturated log-variances: exp(+-3) to the last bit of fp64's tanh
        assert abs(float(mv[1].reshape(-1)[3]) - math.exp(3.)) < 1e-12 and abs(float(mv[1].reshape(-1)[4]) - math.exp(-3.)) < 1e-12
        # the sigmoid at -104 is below fp32's smallest subnormal: the absolute part of the bound covers it
        assert 0. < float(done[4]) < 2.0 ** -149 and float(done[3]) == 1.


def test_wm_post_edges_are_all_present_in_the_larger_cases():
    assert C.WM_LOGVAR_EDGES == (0., 30., -30., 100., -100.) and C.WM_DONE_EDGES == (0., 88., -88., 104., -104.)
    for M, P in C.WM_POST_CASES[1:]:
        raw, logit = C.wm_post_inputs(M, P)
        assert set(C.WM_LOGVAR_EDGES) <= set(raw[:, 1::2].reshape(-1).tolist())
        assert set(C.WM_DONE_EDGES) <= set(logit.tolist())
        assert 2. < float(raw[:, 1::2].std()) and 3. < float(logit.std())


@pytest.mark.parametrize('form', C.GEMM_FORMS)
def test_gemm_reference_forms(form):
    x, w, b, res = C.gemm_inputs(37, 100, 96)
    ref = C.gemm_ref(form, x, w, b, res)
    lin = torch.nn.functional.linear(x.double(), w.double(), b.double())
    want = dict(relu=lin.clamp(min=0.), gelu=0.5 * lin * (1. + torch.erf(lin / math.sqrt(2.))),
                bias_residual_alias=lin + res.double()).get(form, lin)
    torch.testing.assert_close(ref, want, rtol=1e-12, atol=1e-13)
    if form == 'relu':
        assert bool((lin < 0).any()) and bool((lin > 0).any())
