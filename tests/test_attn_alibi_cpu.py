"""ALiBi (world_model['alibi_pos_bias'], world_model['alibi_num_heads']) without a GPU: the slope table, the
dense fp64 reference the GPU tests compare against (attn_alibi_ref = test_attn_sink_cpu.attn_sink_ref with
the distance penalty on the real columns), the ALiBi oracle (alibi_forward = test_attn_sink_cpu.sink_forward
plus the bias, installed over the frozen oracle's Attention.forward), the option handling of the Learner, the
checkpoint interchange with a model without ALiBi and the C ABI's declarations of the xtrl_attn_*_alibi
entry points.

Semantics: the score of query head h, query position i and real key position j (positions inside the
episode) is scale q_i . k_j - slope[h] (i - j), added before any mask fill; memory columns and the zero key
take no bias; slope[h] = 0 for the heads past alibi_num_heads."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import thirdparty as tp

from test_attn_sink_cpu import attn_sink_ref, sink_forward, sink_init, visible

ROOT = Path(__file__).resolve().parents[1]


# ----------------------------------------------------------------------------------------------
# the dense reference
# ----------------------------------------------------------------------------------------------


def attn_alibi_ref(q, k, v, lens, scale, W, slopes, mem_k=None, mem_v=None, zero_kv=False, keep=None, keep_mem=None,
                   fill=float('-inf')):
    """test_attn_sink_cpu.attn_sink_ref with - slopes[h] (i - j) on the real columns only, in the dtype of its
    arguments.  ``slopes`` [H] in that dtype: the tests pass the fp32 slopes widened to fp64, so the slope
    rounding is no part of any error.  Masked real scores are ``fill``, put in after the bias: -inf (exact zeros:
    every row then needs a visible key or a sink), or x-transformers' finite -max of the dtype, under which a
    row without a visible key and without sinks attends all n positions uniformly (every filled score is the
    same number, whatever the bias was).  Returns (o [b][H][n][dh], lse [b][H][n])."""
    b, H, n, dh = q.shape
    i = torch.arange(n, device=q.device)
    dist = (i[:, None] - i[None, :]).to(q.dtype)
    s = torch.einsum('bhid,bhjd->bhij', q, k) * scale - slopes.to(q.dtype)[None, :, None, None] * dist[None, None]
    cols = [s.masked_fill(~visible(n, lens, W), fill)]
    M = 0 if mem_k is None else mem_k.shape[1]
    if M:
        cols.append(torch.einsum('bhid,hmd->bhim', q, mem_k) * scale)
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
# the ALiBi oracle: test_attn_sink_cpu.sink_forward plus the bias
# ----------------------------------------------------------------------------------------------


def alibi_forward(W=None, zero_kv=False, slopes=None):
    """sink_forward(W, zero_kv) with x-transformers' AlibiPositionalBias added to the real columns before any
    mask fill: bias[h][i][j] = - slopes[h] |arange(j - i, j)[i] - arange(j)[j]|, i the query count and j the
    key count of the call — so the cached single-token call (i = 1, j = cache length + 1) measures the distance
    to the last key.  The memory columns and the zero key take no bias (x-transformers pads the bias with
    zeros on the memory side).  ``slopes`` [heads] fp32, or None: sink_forward itself, bit for bit."""
    base = sink_forward(W, zero_kv)
    if slopes is None:
        return base

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
        sim = sim - slopes.to(sim)[None, :, None, None] * dist.abs().to(sim)[None, None]
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
            cols.append(torch.einsum('bhid,hmd->bhim', q, mem_k.repeat(rep, 1, 1)) * scale)
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


def install_alibi(monkeypatch, heads, alibi_heads=None, W=None, M=0, Z=False, Hkv=None):
    """The ALiBi oracle over the frozen Attention (with the sink / GQA constructor when M or Hkv ask for it) and
    the options into every Learner built afterwards: test_gpu_parity.make_learner takes no ALiBi keyword and
    imports ``xtrl_amd.Learner`` when called, so that name is wrapped to add alibi_pos_bias (and
    alibi_num_heads) to the world_model it is given.  Returns the fp32 slopes [heads]."""
    import xtrl_amd
    from xtrl_amd import ops
    slopes = ops.alibi_slopes(heads, alibi_heads)
    if M or Hkv is not None:
        monkeypatch.setattr(tp.Attention, '__init__', sink_init(Hkv or heads, M))
    monkeypatch.setattr(tp.Attention, 'forward', alibi_forward(W, Z, slopes))
    real = xtrl_amd.Learner

    def learner(*args, world_model, **kw):
        extra = dict(alibi_pos_bias=True, **({} if alibi_heads is None else dict(alibi_num_heads=alibi_heads)))
        return real(*args, world_model=dict(world_model, **extra), **kw)

    monkeypatch.setattr(xtrl_amd, 'Learner', learner)
    return slopes


# ----------------------------------------------------------------------------------------------
# tests
# ----------------------------------------------------------------------------------------------


def test_alibi_slope_table():
    """The pinned slopes, exactly, as fp32 (every one a power of two or 0: exact in fp32)."""
    from xtrl_amd import ops
    p = lambda *e: torch.tensor([0. if x is None else 2. ** -x for x in e], dtype=torch.float32)   # noqa: E731
    for (heads, A), want in (((4, None), p(2, 4, 6, 8)), ((8, None), p(1, 2, 3, 4, 5, 6, 7, 8)),
                             ((6, None), p(2, 4, 6, 8, 1, 3)), ((4, 2), p(4, 8, None, None)), ((4, 4), p(2, 4, 6, 8))):
        got = ops.alibi_slopes(heads, A)
        assert got.dtype == torch.float32 and got.shape == (heads,)
        assert torch.equal(got, want), (heads, A, got)
    # a non-power-of-two geometric ratio: fp64 on the host, rounded once to fp32
    got = ops.alibi_slopes(16)
    want = torch.tensor([2. ** (-0.5 * (k + 1)) for k in range(16)], dtype=torch.float64).to(torch.float32)
    assert torch.equal(got, want)
    # 3 heads: pow2(2) + pow2(4)[0::2][:1]
    assert torch.equal(ops.alibi_slopes(3), p(4, 8, 2))


def _problem(seed, b=2, H=4, n=9, dh=4, M=2):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(b, H, n, dh, generator=g, dtype=torch.float64) for _ in range(3))
    mem_k, mem_v = (torch.randn(H, M, dh, generator=g, dtype=torch.float64) for _ in range(2))
    return q, k, v, mem_k, mem_v, torch.tensor([n, 4], dtype=torch.int32)


@pytest.mark.parametrize('W', [None, 3])
def test_reference_with_zero_slopes_is_the_sink_reference(W):
    q, k, v, mem_k, mem_v, lens = _problem(1)
    a = attn_alibi_ref(q, k, v, lens, 0.5, W, torch.zeros(4, dtype=torch.float64), mem_k, mem_v, True)
    b = attn_sink_ref(q, k, v, lens, 0.5, W, mem_k, mem_v, True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize('W', [None, 3])
def test_reference_with_zero_queries_decays_with_distance(W):
    """q = 0: the probabilities of row i over its visible keys are proportional to exp(-slope (i - j)); with
    v = I they are o itself.  The zero key (score 0, bias 0) takes its share of the denominator."""
    from xtrl_amd import ops
    b, H, n = 2, 4, 8
    slopes = ops.alibi_slopes(H, 3).double()
    v = torch.eye(n, dtype=torch.float64).expand(b, H, n, n)
    lens = torch.tensor([8, 3], dtype=torch.int32)
    for Z in (False, True):
        o, lse = attn_alibi_ref(torch.zeros(b, H, n, n, dtype=torch.float64), v, v, lens, 0.5, W, slopes, zero_kv=Z)
        vis = visible(n, lens, W)
        for e in range(b):
            for h in range(H):
                for i in range(n):
                    js = [j for j in range(n) if vis[e, 0, i, j]]
                    if not js and not Z:
                        continue
                    w = torch.tensor([float(np.exp(-float(slopes[h]) * (i - j))) for j in js], dtype=torch.float64)
                    den = w.sum() + float(Z)
                    want = torch.zeros(n, dtype=torch.float64)
                    want[js] = w / den
                    torch.testing.assert_close(o[e, h, i], want)
                    torch.testing.assert_close(lse[e, h, i], den.log())
        # head 3 has slope 0: the sink reference
        ref = attn_sink_ref(torch.zeros(b, H, n, n, dtype=torch.float64), v, v, lens, 0.5, W, zero_kv=Z)[0]
        live = vis.any(-1)[:, 0] | Z
        assert torch.equal(o[:, 3][live], ref[:, 3][live])


def _module(Hkv, M, seed=0):
    torch.manual_seed(seed)
    m = tp.Attention.__new__(tp.Attention)
    sink_init(Hkv, M)(m, 24, 4, 8, dropout=0., gate_values=True, learned_value_residual_mix=False)
    return m.eval()


def test_alibi_oracle_without_slopes_is_the_sink_oracle():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 9, 24, generator=g)
    key_mask = torch.arange(9)[None, :] < torch.tensor([9, 3])[:, None]
    m = _module(2, 3)
    assert alibi_forward(2, True, None) is not None
    with torch.no_grad():
        a = sink_forward(2, True)(m, x, None, key_mask=key_mask)
        b = alibi_forward(2, True, None)(m, x, None, key_mask=key_mask)
        z = alibi_forward(2, True, torch.zeros(4))(m, x, None, key_mask=key_mask)
        s = alibi_forward(2, True, torch.tensor([.25, .0625, 0., 0.]))(m, x, None, key_mask=key_mask)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0]) and torch.equal(a[2], b[2])
    assert torch.equal(a[0], z[0])          # zero slopes subtract exact zeros
    assert not torch.equal(a[0], s[0])      # slopes change it


@pytest.mark.parametrize('Hkv,M,Z', [(4, 0, False), (2, 3, True)])
def test_alibi_oracle_cached_decode_equals_full_sequence(Hkv, M, Z, monkeypatch):
    """With slopes, the oracle's Decoder fed one token at a time with its cache gives the full-sequence
    forward at every position — in its rollout_rotary = 'absolute' mode (the rotary positions of the two then
    agree as well), gates and the learned value-residual mix on, no window.  Without the distances to the
    LAST key (arange(j - i, j) against arange(j)) the single-token call would see distance 0 everywhere."""
    from xtrl_amd import ops
    monkeypatch.setattr(tp.XT, 'rollout_rotary', 'absolute')
    monkeypatch.setattr(tp.Attention, '__init__', sink_init(Hkv, M))
    monkeypatch.setattr(tp.Attention, 'forward', alibi_forward(None, Z, ops.alibi_slopes(4, 3)))
    torch.manual_seed(2)
    dec = tp.Decoder(24, 2, heads=4, attn_dim_head=8, rotary_pos_emb=True, attn_gate_values=True,
                     add_value_residual=True, learned_value_residual_mix=True).eval()
    with torch.no_grad():
        for name, p in dec.named_parameters():
            if 'to_v_gate' in name or 'to_value_residual_mix' in name:
                p.copy_(torch.randn_like(p) * 0.3)
    n = 11
    x = torch.randn(2, n, 24, generator=torch.Generator().manual_seed(3))
    with torch.no_grad():
        full, _ = dec(x)
        cache = None
        for t in range(n):
            out, cache = dec(x[:, t:t + 1], cache=cache)
            torch.testing.assert_close(out[:, 0], full[:, t], rtol=1e-5, atol=1e-5)
        monkeypatch.setattr(tp.Attention, 'forward', alibi_forward(None, Z, None))   # the bias matters
        assert float((dec(x)[0] - full).abs().max()) > 1e-3
    assert cache.cache_length == n and cache.attn_intermediates[0].cached_kv[0].shape == (2, Hkv, n, 8)


BASE = dict(attn_dim_head=16, heads=4, depth=2, attn_gate_values=True, add_value_residual=True,
            learned_value_residual_mix=True)


def _kw(**agent):
    return dict(num_episodes_per_update=2, batch_size=2, accelerate_kwargs=dict(device='cpu'), use_graph=False,
                agent_kwargs=dict(hidden_dim=48, **agent))


def test_alibi_option_handling():
    """alibi_pos_bias=True sets ModelConfig.alibi_heads = heads (alibi_num_heads = A: A) and the non-persistent
    slopes buffer; the defaults build today's model; bad values are refused by name; alibi_learned and the
    fractal body refuse."""
    from xtrl_amd import Learner, ops
    from xtrl_amd.learner import XT_DEFAULTS
    assert XT_DEFAULTS['alibi_pos_bias'] is False and XT_DEFAULTS['alibi_num_heads'] is None
    assert XT_DEFAULTS['alibi_learned'] is False
    shapes = lambda learner: {k: tuple(v.shape) for k, v in learner.agent.model.state_dict().items()}   # noqa: E731
    plain = Learner(5, 2, (-1., 1.), world_model=dict(BASE), **_kw())
    assert plain.agent.cfg.alibi_heads == 0 and plain.agent.model.alibi_slopes is None
    a = Learner(5, 2, (-1., 1.), world_model=dict(BASE, alibi_pos_bias=True), **_kw())
    assert a.agent.cfg.alibi_heads == 4
    assert torch.equal(a.agent.model.alibi_slopes, ops.alibi_slopes(4)) and a.agent.model.alibi_slopes.dtype == torch.float32
    assert torch.equal(a.agent.ema_model.alibi_slopes, ops.alibi_slopes(4))
    assert shapes(a) == shapes(plain) and 'alibi_slopes' not in a.agent.model.state_dict()
    for A in (1, 2, 4):
        x = Learner(5, 2, (-1., 1.), world_model=dict(BASE, alibi_pos_bias=True, alibi_num_heads=A), **_kw())
        assert x.agent.cfg.alibi_heads == A and torch.equal(x.agent.model.alibi_slopes, ops.alibi_slopes(4, A))
    n = Learner(5, 2, (-1., 1.), world_model=dict(BASE, alibi_pos_bias=True, alibi_num_heads=None), **_kw())
    assert n.agent.cfg.alibi_heads == 4
    # composes with the other attention options
    c = Learner(5, 2, (-1., 1.), world_model=dict(BASE, alibi_pos_bias=True, attn_max_attend_past=5, attn_num_mem_kv=2,
                                                  attn_add_zero_kv=True, rotary_xpos=True, attn_qk_norm=False),
                **_kw(kv_heads=2))
    assert (c.agent.cfg.alibi_heads, c.agent.cfg.attn_window, c.agent.cfg.kv_heads, c.agent.cfg.num_mem_kv) == (4, 5, 2, 2)
    # the defaults are today's model
    for wm in (dict(alibi_pos_bias=False), dict(alibi_num_heads=None), dict(alibi_learned=False),
               dict(alibi_pos_bias=False, alibi_num_heads=None, alibi_learned=False)):
        d = Learner(5, 2, (-1., 1.), world_model=dict(BASE, **wm), **_kw())
        assert d.agent.cfg.alibi_heads == 0 and shapes(d) == shapes(plain)
    for wm in (dict(alibi_num_heads=2), dict(alibi_num_heads=4), dict(alibi_pos_bias=False, alibi_num_heads=2)):
        with pytest.raises(ValueError, match='alibi_num_heads'):
            Learner(5, 2, (-1., 1.), world_model=dict(BASE, **wm), **_kw())
    for bad in (0, 5, -1, 2.0, True, '2'):
        with pytest.raises(ValueError, match='alibi_num_heads'):
            Learner(5, 2, (-1., 1.), world_model=dict(BASE, alibi_pos_bias=True, alibi_num_heads=bad), **_kw())
    for bad in ('yes', 2, None, 1.5):
        with pytest.raises(ValueError, match='alibi_pos_bias'):
            Learner(5, 2, (-1., 1.), world_model=dict(BASE, alibi_pos_bias=bad), **_kw())
    for wm in (dict(alibi_learned=True), dict(alibi_pos_bias=True, alibi_learned=True)):
        with pytest.raises(NotImplementedError, match='alibi_learned'):
            Learner(5, 2, (-1., 1.), world_model=dict(BASE, **wm), **_kw())
    fbase = dict(attn_dim_head=16, heads=4, depth=1)
    with pytest.raises(NotImplementedError, match='ALiBi'):
        Learner(5, 2, (-1., 1.), world_model=dict(fbase, alibi_pos_bias=True), **_kw(policy_body='fractal'))
    Learner(5, 2, (-1., 1.), world_model=dict(fbase, alibi_pos_bias=False, alibi_num_heads=None, alibi_learned=False),
            **_kw(policy_body='fractal'))


def test_alibi_checkpoint_interchanges_with_a_model_without(tmp_path):
    """A checkpoint saved with ALiBi loads into a model without it and back: the slopes are no state."""
    from xtrl_amd import Learner, ops
    kw = _kw(save_path=str(tmp_path / 'ppo.pt'))
    torch.manual_seed(0)
    a = Learner(5, 2, (-1., 1.), world_model=dict(BASE, alibi_pos_bias=True, alibi_num_heads=3), **kw).agent
    torch.manual_seed(1)
    b = Learner(5, 2, (-1., 1.), world_model=dict(BASE), **kw).agent
    assert list(a.model.state_dict()) == list(b.model.state_dict())
    assert not torch.equal(a.flat.flat, b.flat.flat)
    a.save()
    assert not any('alibi' in k for k in torch.load(str(tmp_path / 'ppo.pt'), weights_only=True)['model'])
    b.load()
    assert torch.equal(a.flat.flat, b.flat.flat) and b.model.alibi_slopes is None
    with torch.no_grad():
        b.flat.flat.mul_(0.5)
    b.save()
    a.load()
    assert torch.equal(a.flat.flat, b.flat.flat) and torch.equal(a.model.alibi_slopes, ops.alibi_slopes(4, 3))


def test_alibi_entry_points_are_declared_bound_and_exported():
    """include/xtrl_hip.h declares the three _alibi entry points — the _sink signatures plus the slopes before
    the stream; the ctypes table binds them with one argument more than _sink; the library exports them; the
    ABI number agrees in the header, the binding and the library; the descriptors carry the field."""
    from xtrl_amd import _lib
    text = (ROOT / 'include' / 'xtrl_hip.h').read_text()
    for name in ('xtrl_attn_fwd_alibi', 'xtrl_attn_bwd_alibi', 'xtrl_attn_bwd_part_alibi'):
        m = re.search(r'int %s\(([^;]*)\);' % name, text)
        assert m, name
        args = ' '.join(m.group(1).split())
        s = re.search(r'int %s\(([^;]*)\);' % name.replace('_alibi', '_sink'), text)
        sink_args = ' '.join(s.group(1).split())
        assert args == sink_args.replace('void* stream', 'const float* alibi_slopes, void* stream'), (name, args)
        res, sig = _lib.SIGNATURES[name]
        sres, ssig = _lib.SIGNATURES[name.replace('_alibi', '_sink')]
        assert res == sres and sig == ssig[:-1] + [_lib.P, _lib.P] and len(sig) == args.count(',') + 1, name
    abi = int(re.search(r'#define XTRL_ABI_VERSION (\d+)', text).group(1))
    assert abi == _lib.ABI_VERSION >= 27
    lib = _lib.load()
    assert lib.xtrl_abi_version() == abi
    for name in ('xtrl_attn_fwd_alibi', 'xtrl_attn_bwd_alibi', 'xtrl_attn_bwd_part_alibi'):
        assert getattr(lib, name) is not None, name
    for desc, cname in ((_lib.DecodeDesc, 'XtrlDecodeDesc'), (_lib.TrainDesc, 'XtrlTrainDesc')):
        assert dict(desc._fields_)['alibi_slopes'] is _lib.P
        body = re.search(r'typedef struct[^;]*?\{((?:[^{}]|\{[^{}]*\})*)\}\s*%s;' % cname, text, re.S)
        assert 'const float* alibi_slopes;' in text and (body is None or 'alibi_slopes' in body.group(1)), cname
