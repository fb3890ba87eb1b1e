"""Grouped-query attention (agent_kwargs kv_heads / world_model['attn_one_kv_head']) without a GPU: the GQA
oracle the GPU tests compare against (gqa_init / gqa_forward installed over the frozen oracle's
Attention), checked against the frozen oracle at Hkv = H and against the frozen multi-head oracle on
replicated weights; the head mapping (query head h reads kv head h % Hkv, the restatement of
x-transformers' repeat 'b kvh n d -> b (r kvh) n d') pinned against that repeat; the option handling of
the Learner; and the C ABI's declarations of the xtrl_attn_*_gqa entry points."""
import re
from pathlib import Path

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import thirdparty as tp

ROOT = Path(__file__).resolve().parents[1]
_FROZEN_INIT, _FROZEN_FORWARD = tp.Attention.__init__, tp.Attention.forward


def gqa_init(Hkv):
    """oracle.thirdparty.Attention.__init__ with ``Hkv`` kv heads: to_k / to_v are Linear(dim, Hkv dim_head)
    and the learned value-residual mix Linear(dim, Hkv) — the state-dict keys of the frozen oracle with
    the shapes of the device model.  Install with monkeypatch.setattr(tp.Attention, '__init__', gqa_init(Hkv))
    together with gqa_forward."""

    def __init__(self, dim, heads, dim_head, *args, **kw):
        _FROZEN_INIT(self, dim, heads, dim_head, *args, **kw)
        assert heads % Hkv == 0
        self.kv_heads = Hkv
        self.to_k = nn.Linear(dim, Hkv * dim_head, bias=False)
        self.to_v = nn.Linear(dim, Hkv * dim_head, bias=False)
        if self.to_value_residual_mix is not None:
            self.to_value_residual_mix = nn.Sequential(nn.Linear(dim, Hkv), nn.Sigmoid(), tp._Rearrange())
            nn.init.zeros_(self.to_value_residual_mix[0].weight)
            nn.init.zeros_(self.to_value_residual_mix[0].bias)

    return __init__


def gqa_forward(W=None):
    """oracle.thirdparty.Attention.forward for a module built by gqa_init (a frozen one counts as Hkv = H):
    k, v, the value residual, the mix, qk norm, the rotary and the cache all have Hkv heads; after the cache
    concatenation k and v are repeated to H heads as x-transformers does, 'b kvh n d -> b (r kvh) n d' (a
    tile of the head axis — stated here with Tensor.repeat, independently of ops.kv_head_index).  ``W``: the
    sliding window of test_attn_window_cpu.windowed_forward on top (None: none)."""

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
        kr, vr = (k, v) if hkv == h else (k.repeat(1, h // hkv, 1, 1), v.repeat(1, h // hkv, 1, 1))
        i, j = q.shape[-2], k.shape[-2]
        sim = torch.einsum('bhid,bhjd->bhij', q, kr) * scale
        neg = -torch.finfo(sim.dtype).max
        causal = torch.ones((i, j), dtype=torch.bool, device=x.device).triu(j - i + 1)
        sim = sim.masked_fill(causal, neg)
        if W is not None:
            dist = (torch.arange(i, device=x.device) + j - i)[:, None] - torch.arange(j, device=x.device)[None, :]
            sim = sim.masked_fill(dist > W, neg)
        if key_mask is not None:
            sim = sim.masked_fill(~key_mask[:, None, None, :], neg)
        attn = self.attn_dropout(sim.softmax(dim=-1, dtype=torch.float32))
        out = torch.einsum('bhij,bhjd->bhid', attn, vr)
        out = out.permute(0, 2, 1, 3).reshape(b, n, h * dh)
        if self.to_v_gate is not None:
            out = out * self.to_v_gate(x).sigmoid()
        return self.to_out(out), (k, v), orig_v

    return forward


def _attention(Hkv=None, seed=0, dim=24, heads=4, dim_head=8):
    """A gated Attention with the learned mix and random weights: frozen (Hkv None) or built by gqa_init."""
    torch.manual_seed(seed)
    m = tp.Attention.__new__(tp.Attention)
    init = _FROZEN_INIT if Hkv is None else gqa_init(Hkv)
    init(m, dim, heads, dim_head, dropout=0., gate_values=True, learned_value_residual_mix=True)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn_like(p) * 0.3)
    return m.eval()


def _same(a, b):
    return (torch.equal(a[0], b[0]) and torch.equal(a[1][0], b[1][0]) and torch.equal(a[1][1], b[1][1])
            and torch.equal(a[2], b[2]))


def test_gqa_oracle_with_all_kv_heads_equals_frozen_oracle():
    """Hkv = H (a module built by gqa_init(H), and a frozen module): output, cache and orig_v equal the
    frozen forward's bit for bit — full sequences with a key mask and the value residual, and one cached
    token."""
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 9, 24, generator=g)
    vres = torch.randn(2, 4, 9, 8, generator=g)
    key_mask = torch.arange(9)[None, :] < torch.tensor([9, 4])[:, None]
    x1 = torch.randn(2, 1, 24, generator=g)
    cache = (torch.randn(2, 4, 7, 8, generator=g), torch.randn(2, 4, 7, 8, generator=g))
    fwd = gqa_forward()
    for m in (_attention(4), _attention(None)):
        with torch.no_grad():
            for kw in (dict(key_mask=key_mask), dict(key_mask=key_mask, value_residual=vres), dict()):
                assert _same(_FROZEN_FORWARD(m, x, None, **kw), fwd(m, x, None, **kw))
            assert _same(_FROZEN_FORWARD(m, x1, None, cache_kv=cache), fwd(m, x1, None, cache_kv=cache))


@pytest.mark.parametrize('Hkv', [1, 2])
def test_gqa_oracle_equals_frozen_mha_oracle_on_replicated_weights(Hkv):
    """H = 4: the GQA oracle equals the frozen multi-head oracle whose to_k / to_v / mix rows and whose
    value-residual heads are the GQA ones replicated by ops.kv_head_index (the project's one Python
    statement of the mapping; the oracle repeats with Tensor.repeat) — outputs within fp32 assert_close
    defaults (the projections are differently shaped GEMMs), and the GQA weight gradients equal to the
    per-group sums of the multi-head ones."""
    from xtrl_amd import ops
    H, dh, dim = 4, 8, 24
    idx = ops.kv_head_index(H, Hkv)
    gm, mm = _attention(Hkv, seed=3), _attention(None, seed=3)
    rows = lambda w: w.reshape(Hkv, -1, *w.shape[1:])[idx].reshape(-1, *w.shape[1:])   # noqa: E731
    with torch.no_grad():
        for name in ('to_q', 'to_out', 'to_v_gate'):
            getattr(mm, name).load_state_dict(getattr(gm, name).state_dict())
        mm.to_k.weight.copy_(rows(gm.to_k.weight))
        mm.to_v.weight.copy_(rows(gm.to_v.weight))
        mm.to_value_residual_mix[0].weight.copy_(gm.to_value_residual_mix[0].weight[idx])
        mm.to_value_residual_mix[0].bias.copy_(gm.to_value_residual_mix[0].bias[idx])
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 9, dim, generator=g)
    vres = torch.randn(2, Hkv, 9, dh, generator=g)
    key_mask = torch.arange(9)[None, :] < torch.tensor([9, 5])[:, None]
    w_out = torch.randn(2, 9, dim, generator=g)
    out_g, (kg, vg), ov_g = gqa_forward()(gm, x, None, key_mask=key_mask, value_residual=vres)
    out_m, (km, vm), ov_m = _FROZEN_FORWARD(mm, x, None, key_mask=key_mask, value_residual=vres[:, idx])
    torch.testing.assert_close(out_g, out_m)
    torch.testing.assert_close(kg[:, idx], km)
    torch.testing.assert_close(vg[:, idx], vm)
    torch.testing.assert_close(ov_g[:, idx], ov_m)
    assert kg.shape == (2, Hkv, 9, dh) and ov_g.shape == (2, Hkv, 9, dh)
    (out_g * w_out).sum().backward()
    (out_m * w_out).sum().backward()

    def group_sum(gr):   # [H * r][...] multi-head gradient rows -> [Hkv * r][...] per-group sums
        per = gr.reshape(H, -1, *gr.shape[1:])
        return torch.zeros(Hkv, *per.shape[1:]).index_add_(0, idx, per).reshape(-1, *gr.shape[1:])

    torch.testing.assert_close(gm.to_k.weight.grad, group_sum(mm.to_k.weight.grad))
    torch.testing.assert_close(gm.to_v.weight.grad, group_sum(mm.to_v.weight.grad))
    torch.testing.assert_close(gm.to_value_residual_mix[0].weight.grad, group_sum(mm.to_value_residual_mix[0].weight.grad))
    torch.testing.assert_close(gm.to_value_residual_mix[0].bias.grad, group_sum(mm.to_value_residual_mix[0].bias.grad))
    torch.testing.assert_close(gm.to_q.weight.grad, mm.to_q.weight.grad)
    torch.testing.assert_close(gm.to_out.weight.grad, mm.to_out.weight.grad)


def test_kv_heads_option_handling():
    """The kv head count is the Agent's ``kv_heads`` argument (agent_kwargs=dict(kv_heads=Hkv)) or
    world_model['attn_one_kv_head'] = True: kv_heads = Hkv shrinks to_k / to_v / the mix and sets
    ModelConfig.kv_heads; attn_one_kv_head is kv_heads = 1; kv_heads = heads and None build today's state dict;
    bad values and both options together are refused by name; the fractal body refuses Hkv < heads and takes the
    defaults.  world_model['attn_kv_heads'] itself stays refused with NotImplementedError, as
    test_host_cpu.test_world_model_options_defaults_accepted_others_named requires of it: that x-transformers
    spelling of the option is not available here, and the refusal names the two that are."""
    from xtrl_amd import Learner
    base_kw = dict(num_episodes_per_update=2, batch_size=2, accelerate_kwargs=dict(device='cpu'), use_graph=False)
    kw = lambda **agent: dict(base_kw, agent_kwargs=dict(hidden_dim=48, **agent))   # noqa: E731
    base = dict(attn_dim_head=16, heads=4, depth=2, attn_gate_values=True, add_value_residual=True,
                learned_value_residual_mix=True)
    shapes = lambda learner: {k: tuple(v.shape) for k, v in learner.agent.model.state_dict().items()}   # noqa: E731
    plain = Learner(5, 2, (-1., 1.), world_model=dict(base), **kw())
    assert plain.agent.cfg.kv_heads == 0 and plain.agent.cfg.kv_inner == 64
    pre = 'transformer.attn_layers.layers.'
    for Hkv in (1, 2):
        a = Learner(5, 2, (-1., 1.), world_model=dict(base), **kw(kv_heads=Hkv))
        sa = shapes(a)
        assert a.agent.cfg.kv_heads == Hkv and a.agent.cfg.kv_inner == 16 * Hkv
        assert list(sa) == list(shapes(plain))
        assert sa[pre + '0.1.to_k.weight'] == sa[pre + '0.1.to_v.weight'] == (16 * Hkv, 48)
        assert sa[pre + '2.1.to_k.weight'] == (16 * Hkv, 48) and sa[pre + '0.1.to_q.weight'] == (64, 48)
        assert sa[pre + '0.1.to_v_gate.weight'] == (64, 48) and sa[pre + '0.1.to_out.weight'] == (48, 64)
        assert sa[pre + '2.1.to_value_residual_mix.0.weight'] == (Hkv, 48)
        assert sa[pre + '2.1.to_value_residual_mix.0.bias'] == (Hkv,)
    one = Learner(5, 2, (-1., 1.), world_model=dict(base, attn_one_kv_head=True), **kw())
    assert one.agent.cfg.kv_heads == 1
    assert shapes(one) == shapes(Learner(5, 2, (-1., 1.), world_model=dict(base), **kw(kv_heads=1)))
    for wm, agent in ((dict(), dict(kv_heads=4)), (dict(), dict(kv_heads=None)), (dict(attn_one_kv_head=False), dict()),
                      (dict(attn_kv_heads=None), dict())):
        n = Learner(5, 2, (-1., 1.), world_model=dict(base, **wm), **kw(**agent))
        assert n.agent.cfg.kv_heads == 0 and shapes(n) == shapes(plain)
    for bad in (0, 3, 2.5, True, 8):
        with pytest.raises(ValueError, match='kv_heads'):
            Learner(5, 2, (-1., 1.), world_model=dict(base), **kw(kv_heads=bad))
    with pytest.raises(ValueError, match='attn_one_kv_head'):
        Learner(5, 2, (-1., 1.), world_model=dict(base, attn_one_kv_head=True), **kw(kv_heads=2))
    for value in (1, 2, 4):   # the x-transformers spelling stays a refused world_model option, named with the way in
        with pytest.raises(NotImplementedError, match='attn_kv_heads.*kv_heads=Hkv'):
            Learner(5, 2, (-1., 1.), world_model=dict(base, attn_kv_heads=value), **kw())
    fbase = dict(attn_dim_head=16, heads=4, depth=1)
    for wm, agent in ((dict(), dict(kv_heads=2)), (dict(attn_one_kv_head=True), dict())):
        with pytest.raises(NotImplementedError, match='kv_heads'):
            Learner(5, 2, (-1., 1.), world_model=dict(fbase, **wm), **kw(policy_body='fractal', **agent))
    Learner(5, 2, (-1., 1.), world_model=dict(fbase, attn_kv_heads=None, attn_one_kv_head=False),
            **kw(policy_body='fractal'))
    Learner(5, 2, (-1., 1.), world_model=dict(fbase), **kw(policy_body='fractal', kv_heads=4))


@pytest.mark.parametrize('H,Hkv', [(4, 1), (4, 2), (6, 2), (6, 3), (4, 4)])
def test_kv_head_index_is_the_tiled_repeat(H, Hkv):
    """ops.kv_head_index: k[:, idx] equals k tiled H / Hkv times along the head axis — the (r kvh)
    ordering of the repeat, in which consecutive query heads read different kv heads — and its autograd
    sums a kv head's gradient over exactly the query heads mapped to it."""
    from xtrl_amd import ops
    idx = ops.kv_head_index(H, Hkv)
    assert idx.shape == (H,) and idx.dtype == torch.int64
    g = torch.Generator().manual_seed(H + Hkv)
    k = torch.randn(2, Hkv, 5, 3, generator=g, requires_grad=True)
    rep = k[:, idx]
    assert torch.equal(rep, k.repeat(1, H // Hkv, 1, 1))
    w = torch.randn(2, H, 5, 3, generator=g)
    (rep * w).sum().backward()
    want = torch.stack([sum(w[:, h] for h in range(H) if int(idx[h]) == kvh) for kvh in range(Hkv)], dim=1)
    torch.testing.assert_close(k.grad, want)
    assert all(0 <= int(i) < Hkv for i in idx) and sorted(set(idx.tolist())) == list(range(Hkv))


def test_gqa_entry_points_are_declared_and_bound():
    """include/xtrl_hip.h declares the three _gqa entry points with Hkv after H and the window before the
    stream, and the ctypes table binds them with one more int than the _win forms."""
    from xtrl_amd import _lib
    text = (ROOT / 'include' / 'xtrl_hip.h').read_text()
    for name in ('xtrl_attn_fwd_gqa', 'xtrl_attn_bwd_gqa', 'xtrl_attn_bwd_part_gqa'):
        m = re.search(r'int %s\(([^;]*)\);' % name, text)
        assert m, name
        args = ' '.join(m.group(1).split())
        assert 'int H, int Hkv, int n, int dh' in args and args.endswith('int window, void* stream'), (name, args)
        res, sig = _lib.SIGNATURES[name]
        wres, wsig = _lib.SIGNATURES[name.replace('_gqa', '_win')]
        assert res == wres and len(sig) == len(wsig) + 1 and len(sig) == args.count(',') + 1, name
    assert _lib.ABI_VERSION == int(re.search(r'#define XTRL_ABI_VERSION (\d+)', text).group(1)) >= 23
