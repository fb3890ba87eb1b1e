"""Logit soft-clamp (world_model['attn_softclamp_logits'], world_model['attn_logit_softclamp_value']) without a
GPU: the dense fp64 reference the GPU tests compare against (attn_softclamp_ref = test_attn_alibi_cpu.
attn_alibi_ref with the clamp on the real and the memory columns), the soft-clamp oracle (softclamp_forward =
test_attn_alibi_cpu.alibi_forward plus the clamp, installed over the frozen oracle's Attention.forward), the
option handling of the Learner, the checkpoint interchange with a model without the option and the C ABI's
declarations of the xtrl_attn_*_softclamp entry points.

Semantics (restated from x-transformers' Attend.forward, parity unpinned): with c the clamp value, the score of
query head h, query position i and real key position j is
    x_ij = scale q_i . k_j - slope[h] (i - j)        (the ALiBi term only with ALiBi)
    s_ij = c tanh(x_ij / c)
applied after the bias and before every mask fill; the memory columns are clamped too (no bias); the zero
key's score 0 stays 0."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import thirdparty as tp

from test_attn_alibi_cpu import alibi_forward, attn_alibi_ref
from test_attn_sink_cpu import sink_init, visible

ROOT = Path(__file__).resolve().parents[1]


# ----------------------------------------------------------------------------------------------
# the dense reference
# ----------------------------------------------------------------------------------------------


def attn_softclamp_ref(q, k, v, lens, scale, W, slopes, c, mem_k=None, mem_v=None, zero_kv=False, keep=None,
                       keep_mem=None, fill=float('-inf')):
    """test_attn_alibi_cpu.attn_alibi_ref with s = c tanh(x / c) on the real columns (after the bias) and on the
    memory columns, before the fill, in the dtype of its arguments.  ``slopes`` [H] or None (no bias).  The zero
    key's score is 0.  Returns (o [b][H][n][dh], lse [b][H][n])."""
    b, H, n, dh = q.shape
    i = torch.arange(n, device=q.device)
    dist = (i[:, None] - i[None, :]).to(q.dtype)
    s = torch.einsum('bhid,bhjd->bhij', q, k) * scale
    if slopes is not None:
        s = s - slopes.to(q.dtype)[None, :, None, None] * dist[None, None]
    s = c * torch.tanh(s / c)
    cols = [s.masked_fill(~visible(n, lens, W), fill)]
    M = 0 if mem_k is None else mem_k.shape[1]
    if M:
        sm = torch.einsum('bhid,hmd->bhim', q, mem_k) * scale
        cols.append(c * torch.tanh(sm / c))
    if zero_kv:
        cols.append(torch.zeros(b, H, n, 1, dtype=q.dtype, device=q.device))
    s = torch.cat(cols, dim=-1)
    lse = torch.logsumexp(s, dim=-1)
    p = s.softmax(-1)
    pr, pm = p[..., :n], p[..., n:n + M]
    if keep is not None:
        pr = pr * keep
    o = torch.einsum('bhij,bhjd->bhid', pr, v)
    if M:
        if keep_mem is not None:
            pm = pm * keep_mem
        o = o + torch.einsum('bhim,hmd->bhid', pm, mem_v)
    return o, lse


# ----------------------------------------------------------------------------------------------
# the soft-clamp oracle: test_attn_alibi_cpu.alibi_forward plus the clamp
# ----------------------------------------------------------------------------------------------


def softclamp_forward(W=None, zero_kv=False, slopes=None, c=None):
    """alibi_forward(W, zero_kv, slopes) with sim = c tanh(sim / c) after the ALiBi bias and before the causal,
    window and padding fills, and the same clamp on the memory columns; the zero key's 0 is not touched.
    ``slopes`` None: no bias.  ``c`` None: alibi_forward itself."""
    if c is None:
        return alibi_forward(W, zero_kv, slopes)
    c = float(c)

    def forward(self, x, freqs, key_mask=None, cache_kv=None, value_residual=None, xpos=None):
        b, n, _ = x.shape
        h, dh = self.heads, self.dim_head
        hkv = getattr(self, 'kv_heads', h)
        split = lambda t, heads: t.reshape(b, n, heads, dh).permute(0, 2, 1, 3)   # noqa: E731
        q, k, v = split(self.to_q(x), h), split(self.to_k(x), hkv), split(self.to_v(x), hkv)
        orig_v = v
        if value_residual is not None and self.to_value_residual_mix is not None:
            mix = self.to_value_residual_mix(x)
            if tp.XT.value_residual_lerp == 'toward_first':
                v = v.lerp(value_residual, mix)
            else:
                v = value_residual.lerp(v, mix)
        scale = dh ** -0.5
        if self.qk_norm:
            q, k = F.normalize(q, dim=-1), F.normalize(k, dim=-1)
            scale = self.qk_norm_scale
        if freqs is not None:
            xq, xk = (1., 1.) if xpos is None else (xpos, xpos ** -1.)
            q, k = tp.apply_rotary(q, freqs, xq), tp.apply_rotary(k, freqs, xk)
        if cache_kv is not None:
            k = torch.cat((cache_kv[0], k), dim=-2)
            v = torch.cat((cache_kv[1], v), dim=-2)
        rep = h // hkv
        kr, vr = (k, v) if rep == 1 else (k.repeat(1, rep, 1, 1), v.repeat(1, rep, 1, 1))
        i, j = q.shape[-2], k.shape[-2]
        sim = torch.einsum('bhid,bhjd->bhij', q, kr) * scale
        dist = torch.arange(j - i, j, device=x.device)[:, None] - torch.arange(j, device=x.device)[None, :]
        if slopes is not None:
            sim = sim - slopes.to(sim)[None, :, None, None] * dist.abs().to(sim)[None, None]
        sim = c * torch.tanh(sim / c)
        neg = -torch.finfo(sim.dtype).max
        causal = torch.ones((i, j), dtype=torch.bool, device=x.device).triu(j - i + 1)
        sim = sim.masked_fill(causal, neg)
        if W is not None:
            sim = sim.masked_fill(dist > W, neg)
        if key_mask is not None:
            sim = sim.masked_fill(~key_mask[:, None, None, :], neg)
        mem_k = getattr(self, 'mem_k', None)
        M = 0 if mem_k is None else mem_k.shape[1]
        cols = [sim]
        if M:
            sm = torch.einsum('bhid,hmd->bhim', q, mem_k.repeat(rep, 1, 1)) * scale
            cols.append(c * torch.tanh(sm / c))
        if zero_kv:
            cols.append(sim.new_zeros(b, h, i, 1))
        attn = self.attn_dropout(torch.cat(cols, dim=-1).softmax(dim=-1, dtype=torch.float32))
        out = torch.einsum('bhij,bhjd->bhid', attn[..., :j], vr)
        if M:
            out = out + torch.einsum('bhim,hmd->bhid', attn[..., j:j + M], self.mem_v.repeat(rep, 1, 1))
        out = out.permute(0, 2, 1, 3).reshape(b, n, h * dh)
        if self.to_v_gate is not None:
            out = out * self.to_v_gate(x).sigmoid()
        return self.to_out(out), (k, v), orig_v

    return forward


def install_softclamp(monkeypatch, heads, c, alibi=False, alibi_heads=None, W=None, M=0, Z=False, Hkv=None):
    """The soft-clamp oracle over the frozen Attention (with the sink / GQA constructor when M or Hkv ask for it)
    and the options into every Learner built afterwards: test_gpu_parity.make_learner takes no soft-clamp
    keyword and imports ``xtrl_amd.Learner`` when called, so that name is wrapped to add attn_softclamp_logits
    and attn_logit_softclamp_value (and the ALiBi options with ``alibi``) to the world_model it is given.
    ``c`` None: the same model and oracle without the clamp.  Returns the fp32 slopes [heads], or None without
    ALiBi."""
    import xtrl_amd
    from xtrl_amd import ops
    slopes = ops.alibi_slopes(heads, alibi_heads) if alibi else None
    if M or Hkv is not None:
        monkeypatch.setattr(tp.Attention, '__init__', sink_init(Hkv or heads, M))
    monkeypatch.setattr(tp.Attention, 'forward', softclamp_forward(W, Z, slopes, c))
    real = xtrl_amd.Learner

    def learner(*args, world_model, **kw):
        extra = {} if c is None else dict(attn_softclamp_logits=True, attn_logit_softclamp_value=float(c))
        if alibi:
            extra.update(alibi_pos_bias=True, **({} if alibi_heads is None else dict(alibi_num_heads=alibi_heads)))
        return real(*args, world_model=dict(world_model, **extra), **kw)

    monkeypatch.setattr(xtrl_amd, 'Learner', learner)
    return slopes


# ----------------------------------------------------------------------------------------------
# tests
# ----------------------------------------------------------------------------------------------


def _problem(seed, b=2, H=4, n=9, dh=4, M=2):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(b, H, n, dh, generator=g, dtype=torch.float64) for _ in range(3))
    mem_k, mem_v = (torch.randn(H, M, dh, generator=g, dtype=torch.float64) for _ in range(2))
    return q, k, v, mem_k, mem_v, torch.tensor([n, 4], dtype=torch.int32)


SLOPES = torch.tensor([.25, .0625, .015625, 0.], dtype=torch.float64)


@pytest.mark.parametrize('W', [None, 3])
def test_reference_with_a_huge_value_is_the_alibi_reference(W):
    """c = 1e6: c tanh(x / c) = x (1 - (x / c)^2 / 3 + ...), a relative change of 1e-11 at |x| = 5."""
    q, k, v, mem_k, mem_v, lens = _problem(1)
    a = attn_softclamp_ref(q, k, v, lens, 0.5, W, SLOPES, 1e6, mem_k, mem_v, True)
    b = attn_alibi_ref(q, k, v, lens, 0.5, W, SLOPES, mem_k, mem_v, True)
    torch.testing.assert_close(a[0], b[0], rtol=1e-9, atol=1e-9)
    torch.testing.assert_close(a[1], b[1], rtol=1e-9, atol=1e-9)
    z = attn_softclamp_ref(q, k, v, lens, 0.5, W, None, 1e6, mem_k, mem_v, True)
    y = attn_alibi_ref(q, k, v, lens, 0.5, W, torch.zeros(4, dtype=torch.float64), mem_k, mem_v, True)
    torch.testing.assert_close(z[0], y[0], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize('W', [None, 3])
def test_reference_with_a_small_value_bounds_every_score(W):
    """c = 0.5 changes the output, and every unmasked score (real and memory columns) lies in (-c, c): with
    v = I and no sinks o is P itself, and lse + log P recovers the scores."""
    q, k, v, mem_k, mem_v, lens = _problem(2)
    c = 0.5
    q = q * 3
    a = attn_softclamp_ref(q, k, v, lens, 0.5, W, SLOPES, c, mem_k, mem_v, True)
    b = attn_alibi_ref(q, k, v, lens, 0.5, W, SLOPES, mem_k, mem_v, True)
    assert float((a[0] - b[0]).abs().max()) > 1e-2
    n = q.shape[2]
    eye = torch.eye(n, dtype=torch.float64).expand(2, 4, n, n)
    qq = torch.cat((q, torch.zeros(2, 4, n, n - q.shape[3], dtype=torch.float64)), dim=-1)
    kk = torch.cat((k, torch.zeros(2, 4, n, n - k.shape[3], dtype=torch.float64)), dim=-1)
    p, lse = attn_softclamp_ref(qq, kk, eye, lens, 0.5, W, SLOPES, c)
    vis = visible(n, lens, W).expand(2, 4, n, n)
    live = vis.any(-1)
    s = (p.log() + lse[..., None])[vis]
    assert s.numel() > 0 and bool((s.abs() < c).all())
    raw = (torch.einsum('bhid,bhjd->bhij', q, k) * 0.5)[vis]
    assert bool((raw.abs() > c).any())   # (the clamp had something to bound)
    # the memory columns: rows whose only columns are the M memory columns (no visible key never happens for
    # live rows, so take lse against the reference's own formula)
    sm = c * torch.tanh(torch.einsum('bhid,hmd->bhim', q, mem_k) * 0.5 / c)
    assert bool((sm.abs() < c).all())
    _, lse_m = attn_softclamp_ref(q, k, v, lens, 0.5, W, SLOPES, c, mem_k, mem_v, False)
    _, lse_0 = attn_softclamp_ref(q, k, v, lens, 0.5, W, SLOPES, c)
    torch.testing.assert_close(torch.logaddexp(lse_0, torch.logsumexp(sm, -1))[live], lse_m[live])


@pytest.mark.parametrize('W', [None, 3])
def test_reference_gradient_is_the_hand_formula(W):
    """autograd's dq through the reference equals scale (P o (dP - D) o (1 - t^2)) K with t = tanh(x / c)."""
    q, k, v, _, _, lens = _problem(3)
    c, scale = 0.75, 0.5
    q = (q * 2).requires_grad_()
    o, _ = attn_softclamp_ref(q, k, v, lens, scale, W, SLOPES, c)
    g = torch.Generator().manual_seed(4)
    do = torch.randn(o.shape, generator=g, dtype=torch.float64)
    live = visible(q.shape[2], lens, W).any(-1).expand(2, 4, -1)[..., None]
    do = do * live
    (dq,) = torch.autograd.grad((o * do).sum(), q)
    with torch.no_grad():
        n = q.shape[2]
        i = torch.arange(n)
        x = torch.einsum('bhid,bhjd->bhij', q, k) * scale - SLOPES[None, :, None, None] * (i[:, None] - i[None, :])
        t = torch.tanh(x / c)
        vis = visible(n, lens, W)
        p = (c * t).masked_fill(~vis, float('-inf')).softmax(-1)
        p = torch.where(vis.any(-1, keepdim=True), p, torch.zeros_like(p))
        dp = torch.einsum('bhid,bhjd->bhij', do, v)
        D = (do * torch.einsum('bhij,bhjd->bhid', p, v)).sum(-1, keepdim=True)
        dx = p * (dp - D) * (1 - t * t)
        want = torch.einsum('bhij,bhjd->bhid', dx, k) * scale
        nofactor = torch.einsum('bhij,bhjd->bhid', p * (dp - D), k) * scale
    torch.testing.assert_close(torch.where(live, dq, torch.zeros_like(dq)), want * live, rtol=1e-10, atol=1e-12)
    assert float((want - nofactor).abs().max()) > 1e-2   # (the factor matters at this c)


def _module(Hkv, M, seed=0):
    torch.manual_seed(seed)
    m = tp.Attention.__new__(tp.Attention)
    sink_init(Hkv, M)(m, 24, 4, 8, dropout=0., gate_values=True, learned_value_residual_mix=False)
    return m.eval()


def test_softclamp_oracle_without_a_value_is_the_alibi_oracle():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 9, 24, generator=g) * 4
    key_mask = torch.arange(9)[None, :] < torch.tensor([9, 3])[:, None]
    m = _module(2, 3)
    sl = torch.tensor([.25, .0625, 0., 0.])
    with torch.no_grad():
        a = alibi_forward(2, True, sl)(m, x, None, key_mask=key_mask)
        b = softclamp_forward(2, True, sl, None)(m, x, None, key_mask=key_mask)
        big = softclamp_forward(2, True, sl, 1e4)(m, x, None, key_mask=key_mask)
        small = softclamp_forward(2, True, sl, 0.25)(m, x, None, key_mask=key_mask)
        a0 = alibi_forward(2, True, None)(m, x, None, key_mask=key_mask)
        big0 = softclamp_forward(2, True, None, 1e4)(m, x, None, key_mask=key_mask)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0]) and torch.equal(a[2], b[2])
    torch.testing.assert_close(a[0], big[0], rtol=1e-4, atol=1e-5)
    torch.testing.assert_close(a0[0], big0[0], rtol=1e-4, atol=1e-5)
    assert float((a[0] - small[0]).abs().max()) > 1e-3


@pytest.mark.parametrize('Hkv,M,Z', [(4, 0, False), (2, 3, True)])
def test_softclamp_oracle_cached_decode_equals_full_sequence(Hkv, M, Z, monkeypatch):
    """The clamp is elementwise, so the oracle's cached single-token calls give the full-sequence forward at
    every position (rollout_rotary = 'absolute'), with ALiBi under the clamp."""
    from xtrl_amd import ops
    monkeypatch.setattr(tp.XT, 'rollout_rotary', 'absolute')
    monkeypatch.setattr(tp.Attention, '__init__', sink_init(Hkv, M))
    monkeypatch.setattr(tp.Attention, 'forward', softclamp_forward(None, Z, ops.alibi_slopes(4, 3), 0.05))
    torch.manual_seed(2)
    dec = tp.Decoder(24, 2, heads=4, attn_dim_head=8, rotary_pos_emb=True, attn_gate_values=True,
                     add_value_residual=True, learned_value_residual_mix=True).eval()
    n = 11
    x = torch.randn(2, n, 24, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        full, _ = dec(x)
        cache = None
        for t in range(n):
            out, cache = dec(x[:, t:t + 1], cache=cache)
            torch.testing.assert_close(out[:, 0], full[:, t], rtol=1e-5, atol=1e-5)
        monkeypatch.setattr(tp.Attention, 'forward', softclamp_forward(None, Z, ops.alibi_slopes(4, 3), None))
        assert float((dec(x)[0] - full).abs().max()) > 1e-3   # the clamp matters


BASE = dict(attn_dim_head=16, heads=4, depth=2, attn_gate_values=True, add_value_residual=True,
            learned_value_residual_mix=True)


def _kw(**agent):
    return dict(num_episodes_per_update=2, batch_size=2, accelerate_kwargs=dict(device='cpu'), use_graph=False,
                agent_kwargs=dict(hidden_dim=48, **agent))


def test_softclamp_option_handling():
    """attn_softclamp_logits=True sets ModelConfig.softclamp = attn_logit_softclamp_value (default 50); the
    defaults build today's model; bad values, and a value without the switch, are refused by name; the fractal
    body refuses."""
    from xtrl_amd import Learner
    from xtrl_amd.learner import XT_DEFAULTS
    assert XT_DEFAULTS['attn_softclamp_logits'] is False and XT_DEFAULTS['attn_logit_softclamp_value'] == 50.
    shapes = lambda learner: {k: tuple(v.shape) for k, v in learner.agent.model.state_dict().items()}   # noqa: E731
    mk = lambda **wm: Learner(5, 2, (-1., 1.), world_model=dict(BASE, **wm), **_kw())   # noqa: E731
    plain = mk()
    assert plain.agent.cfg.softclamp == 0.
    a = mk(attn_softclamp_logits=True)
    assert a.agent.cfg.softclamp == 50. and isinstance(a.agent.cfg.softclamp, float)
    assert shapes(a) == shapes(plain) and list(a.agent.model.state_dict()) == list(plain.agent.model.state_dict())
    for val, want in ((50., 50.), (50, 50.), (5, 5.), (2.5, 2.5), (np.float32(0.5), 0.5), (np.int64(3), 3.), (1e-3, 1e-3)):
        x = mk(attn_softclamp_logits=True, attn_logit_softclamp_value=val)
        assert x.agent.cfg.softclamp == want and isinstance(x.agent.cfg.softclamp, float), val
    # attn_flash stays an ignored implementation switch
    assert mk(attn_softclamp_logits=True, attn_flash=True).agent.cfg.softclamp == 50.
    # composes with the other attention options
    c = Learner(5, 2, (-1., 1.), world_model=dict(BASE, attn_softclamp_logits=True, attn_logit_softclamp_value=7.,
                                                  alibi_pos_bias=True, attn_max_attend_past=5, attn_num_mem_kv=2,
                                                  attn_add_zero_kv=True, rotary_xpos=True),
                **_kw(kv_heads=2))
    assert (c.agent.cfg.softclamp, c.agent.cfg.alibi_heads, c.agent.cfg.attn_window, c.agent.cfg.kv_heads,
            c.agent.cfg.num_mem_kv) == (7., 4, 5, 2, 2)
    qn = mk(attn_softclamp_logits=True, attn_logit_softclamp_value=5, attn_qk_norm=True)
    assert qn.agent.cfg.softclamp == 5. and qn.agent.cfg.qk_norm
    # the defaults are today's model
    for wm in (dict(attn_softclamp_logits=False), dict(attn_logit_softclamp_value=50.),
               dict(attn_logit_softclamp_value=50), dict(attn_softclamp_logits=False, attn_logit_softclamp_value=50.)):
        d = mk(**wm)
        assert d.agent.cfg.softclamp == 0. and shapes(d) == shapes(plain)
    # a value without the switch
    for wm in (dict(attn_logit_softclamp_value=30.), dict(attn_softclamp_logits=False, attn_logit_softclamp_value=5)):
        with pytest.raises(ValueError, match='attn_logit_softclamp_value.*attn_softclamp_logits=True'):
            mk(**wm)
    # the value: a finite real > 0, not a bool
    for bad in (0, 0., -1, -50., float('inf'), float('-inf'), float('nan'), True, False, '50', None, (50.,)):
        with pytest.raises(ValueError, match='attn_logit_softclamp_value') as ei:
            mk(attn_softclamp_logits=True, attn_logit_softclamp_value=bad)
        assert repr(bad) in str(ei.value), bad
    for bad in ('yes', 2, None, 1.5, 50.):
        with pytest.raises(ValueError, match='attn_softclamp_logits'):
            mk(attn_softclamp_logits=bad)
    fbase = dict(attn_dim_head=16, heads=4, depth=1)
    with pytest.raises(NotImplementedError, match='soft-clamp'):
        Learner(5, 2, (-1., 1.), world_model=dict(fbase, attn_softclamp_logits=True), **_kw(policy_body='fractal'))
    Learner(5, 2, (-1., 1.), world_model=dict(fbase, attn_softclamp_logits=False, attn_logit_softclamp_value=50.),
            **_kw(policy_body='fractal'))


def test_softclamp_checkpoint_interchanges_with_a_model_without(tmp_path):
    """A checkpoint saved with the option loads into a model without it and back: the clamp has no state."""
    from xtrl_amd import Learner
    kw = _kw(save_path=str(tmp_path / 'ppo.pt'))
    torch.manual_seed(0)
    a = Learner(5, 2, (-1., 1.), world_model=dict(BASE, attn_softclamp_logits=True, attn_logit_softclamp_value=5.),
                **kw).agent
    torch.manual_seed(1)
    b = Learner(5, 2, (-1., 1.), world_model=dict(BASE), **kw).agent
    assert list(a.model.state_dict()) == list(b.model.state_dict())
    assert not torch.equal(a.flat.flat, b.flat.flat)
    a.save()
    assert not any('clamp' in k for k in torch.load(str(tmp_path / 'ppo.pt'), weights_only=True)['model'])
    b.load()
    assert torch.equal(a.flat.flat, b.flat.flat) and b.cfg.softclamp == 0.
    with torch.no_grad():
        b.flat.flat.mul_(0.5)
    b.save()
    a.load()
    assert torch.equal(a.flat.flat, b.flat.flat) and a.cfg.softclamp == 5.


def test_softclamp_entry_points_are_declared_bound_and_exported():
    """include/xtrl_hip.h declares the three _softclamp entry points — the _alibi signatures plus ``float
    softclamp`` after the slopes; the ctypes table binds them with one float more than _alibi; the library
    exports them; the ABI number agrees in the header, the binding and the library; both descriptors carry the
    field."""
    from xtrl_amd import _lib
    text = (ROOT / 'include' / 'xtrl_hip.h').read_text()
    names = ('xtrl_attn_fwd_softclamp', 'xtrl_attn_bwd_softclamp', 'xtrl_attn_bwd_part_softclamp')
    for name in names:
        m = re.search(r'int %s\(([^;]*)\);' % name, text)
        assert m, name
        args = ' '.join(m.group(1).split())
        s = re.search(r'int %s\(([^;]*)\);' % name.replace('_softclamp', '_alibi'), text)
        alibi_args = ' '.join(s.group(1).split())
        assert args == alibi_args.replace('const float* alibi_slopes, void* stream',
                                          'const float* alibi_slopes, float softclamp, void* stream'), (name, args)
        res, sig = _lib.SIGNATURES[name]
        ares, asig = _lib.SIGNATURES[name.replace('_softclamp', '_alibi')]
        assert res == ares and sig == asig[:-1] + [_lib.F32, _lib.P] and len(sig) == args.count(',') + 1, name
    abi = int(re.search(r'#define XTRL_ABI_VERSION (\d+)', text).group(1))
    assert abi == _lib.ABI_VERSION >= 29
    lib = _lib.load()
    assert lib.xtrl_abi_version() == abi
    for name in names:
        assert getattr(lib, name) is not None, name
    for desc, cname in ((_lib.DecodeDesc, 'XtrlDecodeDesc'), (_lib.TrainDesc, 'XtrlTrainDesc')):
        assert dict(desc._fields_)['attn_softclamp'] is _lib.F32
        body = re.search(r'typedef struct %s \{(.*?)\n\} %s;' % (cname, cname), text, re.S)
        assert body is not None and 'float attn_softclamp;' in body.group(1), cname
        assert int(lib.xtrl_struct_size(cname.encode())) == ctypes.sizeof(desc), cname


@pytest.mark.parametrize('bad,shown', [(-1., '-1'), (-1e-30, '-1e-30'), (float('nan'), 'nan'), (float('inf'), 'inf'),
                                       (float('-inf'), '-inf')])
def test_softclamp_value_check_names_the_value(bad, shown):
    """The argument check of the entry points is host code that runs before any operand is read or any kernel
    launched, so it is reachable without a GPU: a negative or non-finite value is XTRL_E_ARG with the value in
    the message; the largest finite floats pass it (the call then stops at the next check, the null operands)."""
    from xtrl_amd import _lib
    lib = _lib.load()
    call = lambda c: lib.xtrl_attn_fwd_softclamp(None, None, None, 1, None, None, None, None, 1, 4, 4, 8, 16, 0.25, 0.,   # noqa: E731
                                                 0, 0, 0, 0, 0, 0, None, c, None)
    assert call(bad) == 1
    msg = lib.xtrl_last_error().decode()
    assert f'softclamp {shown} ' in msg.replace('-nan', 'nan'), msg
    for fine in (3.2e38, 3.4028234e38, 1e-38):
        assert call(fine) == 1
        assert 'softclamp' not in lib.xtrl_last_error().decode(), lib.xtrl_last_error().decode()
