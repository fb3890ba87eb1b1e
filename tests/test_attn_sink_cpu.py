"""Attention sinks (world_model['attn_num_mem_kv'] = M learned memory key / value rows per kv head,
world_model['attn_add_zero_kv'] one all-zero key / value) without a GPU: the dense fp64 reference and the
host statement of the sink keep bits that the GPU tests compare against, the sink oracle (sink_init /
sink_forward installed over the frozen oracle's Attention), the option handling of the Learner, the
checkpoint round trip and the C ABI's declarations of the xtrl_attn_*_sink entry points.

Semantics (V(i) = {j : j <= i, j < len, i - j <= W} the real keys row i sees; g the kv head of head h):
  L_i = sum_{j in V(i)} exp(s_ij) + sum_m exp(scale q_i . mem_k[g, m]) + Z,   lse_i = log L_i
  o_i = sum_j keep_ij P_ij v_j + sum_m keep'_im P_im mem_v[g, m]
The sinks are visible to every row, padded rows included; a row with V(i) empty attends them alone."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle import philox as P
from oracle import thirdparty as tp

from test_attn_gqa_cpu import gqa_init

ROOT = Path(__file__).resolve().parents[1]


# ----------------------------------------------------------------------------------------------
# the dense reference and the sink keep bits
# ----------------------------------------------------------------------------------------------


def visible(n, lens, W):
    """bool [b][1][n][n]: real key j visible to query i iff j <= i, j < len and (W not None) i - j <= W."""
    i = torch.arange(n, device=lens.device)
    dist = i[:, None] - i[None, :]
    band = dist >= 0 if W is None else (dist >= 0) & (dist <= W)
    return band[None, None] & (i[None, None, None, :] < lens.long()[:, None, None, None])


def attn_sink_ref(q, k, v, lens, scale, W, mem_k=None, mem_v=None, zero_kv=False, keep=None, keep_mem=None):
    """Dense softmax attention with sinks, in the dtype of its arguments (the tests call it in fp64).
    q, k, v [b][H][n][dh] (k, v already repeated to the query heads), mem_k, mem_v [H][M][dh] (the kv
    head's rows of each query head) or None, ``keep`` [b][H][n][n] / ``keep_mem`` [b][H][n][M] the dropout
    keep factors (bit / (1 - p)) or None.  Masked real scores are -inf — exact zeros, the limit of
    x-transformers' finite fill whenever a sink is present — so at least one sink (or a visible key in
    every row) is required.  Returns (o [b][H][n][dh], lse [b][H][n])."""
    b, H, n, dh = q.shape
    s = torch.einsum('bhid,bhjd->bhij', q, k) * scale
    cols = [s.masked_fill(~visible(n, lens, W), float('-inf'))]
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


def sink_dropout_keep(b, H, n, M, p, seed, offset, layer):
    """bool [b][H][n][M]: the keep bit of memory column m at query row i of (episode e, head h) — word
    (i & 3) of philox4x32(i >> 2, 0x80000000 | m, offset + e H + h, c3; seed) >= p 2^32, with c3 the c3 of the
    call's real keys (oracle.philox.attn_dropout_keep): FIELD_DROPOUT << 24 | layer, and bit 23 set when
    256 p is an integer (byte mode).  c1 has bit 31 set: a real key's c1 (j, or 16 (j >> 6) + (j & 15)) never
    has, so the two streams share no counter and the real keys' bits do not depend on M."""
    n4 = (n + 3) // 4
    c2 = (np.uint64(offset) + np.arange(b * H, dtype=np.uint64))[:, None, None]
    sub = layer | (1 << 23) if float(p * 256).is_integer() else layer
    words = P.philox4x32(np.arange(n4)[None, :, None], (0x80000000 | np.arange(M, dtype=np.uint64))[None, None, :], c2,
                         P._c3(P.FIELD_DROPOUT, sub), seed)
    w = np.stack(words, axis=2).reshape(b * H, 4 * n4, M)[:, :n]     # row i = 4 (i >> 2) + (i & 3)
    return (w >= P._thresh32(p)).reshape(b, H, n, M)


# ----------------------------------------------------------------------------------------------
# the sink oracle: oracle.thirdparty.Attention with memory key / values and the zero key
# ----------------------------------------------------------------------------------------------


def sink_init(Hkv, M):
    """test_attn_gqa_cpu.gqa_init(Hkv) plus the parameters mem_k, mem_v [Hkv][M][dim_head] (randn, as
    x-transformers initialises them; M = 0: none) — the state-dict names and shapes of the device model."""
    base = gqa_init(Hkv)

    def __init__(self, dim, heads, dim_head, *args, **kw):
        base(self, dim, heads, dim_head, *args, **kw)
        if M > 0:
            self.mem_k = nn.Parameter(torch.randn(Hkv, M, dim_head))
            self.mem_v = nn.Parameter(torch.randn(Hkv, M, dim_head))

    return __init__


def sink_forward(W=None, zero_kv=False):
    """test_attn_gqa_cpu.gqa_forward(W) with the sinks as x-transformers has them: the memory rows (no
    rotary, no value residual, not cached) and the zero key are extra key / value columns that no mask
    touches — the causal, window and key-padding fills apply to the real columns only — inside the one
    softmax, finite fill and all.  The returned cache holds the real keys only."""

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
        neg = -torch.finfo(sim.dtype).max
        causal = torch.ones((i, j), dtype=torch.bool, device=x.device).triu(j - i + 1)
        sim = sim.masked_fill(causal, neg)
        if W is not None:
            dist = (torch.arange(i, device=x.device) + j - i)[:, None] - torch.arange(j, device=x.device)[None, :]
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


# ----------------------------------------------------------------------------------------------
# tests
# ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('M,Z', [(0, True), (3, False), (2, True)])
@pytest.mark.parametrize('W', [None, 2])
def test_reference_with_zero_queries_is_uniform_over_visible_keys_and_sinks(W, M, Z):
    """q = 0: every score is 0, so each probability of row i is 1 / (|V(i)| + M + Z): lse = log of that
    count and o_i = (sum_{j in V(i)} v_j + sum_m mem_v[m]) / count.  lens = (6, 2), n = 6, W = 2: rows 4 and 5
    of the second episode are padded rows past the band, V(i) empty — they attend the sinks alone, and with
    the zero key only their output is exactly 0."""
    b, H, n, dh = 2, 2, 6, 4
    g = torch.Generator().manual_seed(5)
    k, v = (torch.randn(b, H, n, dh, generator=g, dtype=torch.float64) for _ in range(2))
    mem_k, mem_v = (torch.randn(H, M, dh, generator=g, dtype=torch.float64) for _ in range(2)) if M else (None, None)
    lens = torch.tensor([6, 2], dtype=torch.int32)
    o, lse = attn_sink_ref(torch.zeros(b, H, n, dh, dtype=torch.float64), k, v, lens, 0.5, W, mem_k, mem_v, Z)
    for e in range(b):
        for i in range(n):
            V = [j for j in range(n) if j <= i and j < int(lens[e]) and (W is None or i - j <= W)]
            cnt = len(V) + M + int(Z)
            for h in range(H):
                want = sum((v[e, h, j] for j in V), torch.zeros(dh, dtype=torch.float64))
                if M:
                    want = want + mem_v[h].sum(0)
                torch.testing.assert_close(o[e, h, i], want / cnt)
                torch.testing.assert_close(lse[e, h, i], torch.tensor(float(np.log(cnt)), dtype=torch.float64))
    if W == 2 and M == 0:
        assert (o[1, :, 4:] == 0).all()   # V empty, the zero key alone


def test_reference_without_masked_rows_matches_plain_softmax_plus_columns():
    """Against an independent statement: the sinks as extra key / value rows prepended to k and v (the memory
    rows, then a zero row — x-transformers' own construction) under a mask that leaves them visible."""
    b, H, n, dh, M = 2, 3, 7, 4, 2
    g = torch.Generator().manual_seed(2)
    q, k, v = (torch.randn(b, H, n, dh, generator=g, dtype=torch.float64) for _ in range(3))
    mem_k, mem_v = (torch.randn(H, M, dh, generator=g, dtype=torch.float64) for _ in range(2))
    lens = torch.tensor([7, 3], dtype=torch.int32)
    o, lse = attn_sink_ref(q, k, v, lens, 0.5, 3, mem_k, mem_v, True)
    zero = torch.zeros(b, H, 1, dh, dtype=torch.float64)
    k2 = torch.cat((mem_k[None].expand(b, -1, -1, -1), zero, k), dim=2)
    v2 = torch.cat((mem_v[None].expand(b, -1, -1, -1), zero, v), dim=2)
    s = torch.einsum('bhid,bhjd->bhij', q, k2) * 0.5
    mask = F.pad(visible(n, lens, 3).expand(b, H, n, n), (M + 1, 0), value=True)
    s = s.masked_fill(~mask, -torch.finfo(s.dtype).max)
    torch.testing.assert_close(o, torch.einsum('bhij,bhjd->bhid', s.softmax(-1), v2))
    torch.testing.assert_close(lse, torch.logsumexp(s, -1))


def test_sink_keep_bits_host_statement():
    """The sink columns' keep bits: a deterministic stream of rate 1 - p per (row, column), disjoint from
    the real keys' counters (bit 31 of c1), keyed by the query head and the layer like theirs, the same
    words in byte mode and word mode up to the c3 flag."""
    b, H, n, M, seed, off, layer = 2, 4, 70, 16, 1234567, 5, 3
    k25 = sink_dropout_keep(b, H, n, M, 0.25, seed, off, layer)
    assert k25.shape == (b, H, n, M) and k25.dtype == np.bool_
    assert np.array_equal(k25, sink_dropout_keep(b, H, n, M, 0.25, seed, off, layer))
    assert abs(k25.mean() - 0.75) < 0.02
    # one word per (i, m): word (i & 3) of the block of rows 4 (i >> 2) .. + 3, restated element by element
    for (e, h, i, m) in ((0, 0, 0, 0), (1, 3, 69, 15), (0, 2, 34, 7)):
        w = P.philox4x32(i >> 2, 0x80000000 | m, off + e * H + h, (P.FIELD_DROPOUT << 24) | layer | (1 << 23), seed)
        assert bool(k25[e, h, i, m]) == bool(int(w[i & 3]) >= int(0.25 * 2 ** 32))
    # p = 0.3 is word mode for the real keys: the sink stream takes that call's c3 (no byte flag)
    k30 = sink_dropout_keep(b, H, n, M, 0.3, seed, off, layer)
    w = P.philox4x32(5 >> 2, 0x80000000 | 2, off + 1 * H + 1, (P.FIELD_DROPOUT << 24) | layer, seed)
    assert bool(k30[1, 1, 5, 2]) == bool(int(w[5 & 3]) >= int(0.3 * 2 ** 32))
    # the head, the layer and the offset key the stream; fewer columns are a prefix (column m's bits do not
    # depend on M), and the real keys' mask is what it is without sinks (its function takes no M)
    assert not np.array_equal(k25[:, 0], k25[:, 1])
    assert not np.array_equal(k25, sink_dropout_keep(b, H, n, M, 0.25, seed, off, layer + 1))
    assert np.array_equal(k25[0, 1], sink_dropout_keep(b, H, n, M, 0.25, seed, off + 1, layer)[0, 0])
    assert np.array_equal(k25[..., :3], sink_dropout_keep(b, H, n, 3, 0.25, seed, off, layer))
    # no real key of either mode reaches c1 >= 2^31
    assert 16 * ((2 ** 31 - 1) >> 6) + 15 < 2 ** 31


def test_sink_oracle_without_sinks_is_the_gqa_oracle_and_sinks_change_it():
    """sink_forward over a module without memory rows and zero_kv False is gqa_forward bit for bit; with
    sinks the full-sequence forward and the cached decode of the last token agree (the sinks are not in
    the cache), and a padded row past the window gives exactly to_out(0) under the zero key alone."""
    from test_attn_gqa_cpu import gqa_forward
    torch.manual_seed(0)

    def build(M):
        m = tp.Attention.__new__(tp.Attention)
        sink_init(2, M)(m, 24, 4, 8, dropout=0., gate_values=False, learned_value_residual_mix=False)
        return m.eval()

    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 9, 24, generator=g)
    key_mask = torch.arange(9)[None, :] < torch.tensor([9, 3])[:, None]
    m0 = build(0)
    with torch.no_grad():
        a, b_ = gqa_forward(2)(m0, x, None, key_mask=key_mask), sink_forward(2)(m0, x, None, key_mask=key_mask)
        assert torch.equal(a[0], b_[0]) and torch.equal(a[1][0], b_[1][0])
        z = sink_forward(2, True)(m0, x, None, key_mask=key_mask)[0]
        assert not torch.equal(z[0], a[0][0])
        assert (z[1, 6:] == 0).all()   # len 3, W 2: rows >= 5 see no real key; no bias in to_out
        m3 = build(3)
        assert m3.mem_k.shape == m3.mem_v.shape == (2, 3, 8)
        full, (k, v), _ = sink_forward(4, True)(m3, x, None)
        assert k.shape == (2, 2, 9, 8)   # the cache holds the real keys only
        last, _, _ = sink_forward(4, True)(m3, x[:, 8:], None, cache_kv=(k[:, :, :8], v[:, :, :8]))
        torch.testing.assert_close(last[:, 0], full[:, 8])


def test_sink_option_handling():
    """attn_num_mem_kv = M builds mem_k / mem_v [Hkv][M][dh] beside to_q in every attention block (kv_heads None
    and 2) and sets ModelConfig.num_mem_kv; attn_add_zero_kv sets ModelConfig.add_zero_kv and adds no
    parameter; the defaults build today's state dict; bad values are refused by name; attn_num_mem_kv with
    attn_qk_norm is refused naming both (the zero key with qk norm is fine); the fractal body refuses both
    options and takes them at their defaults."""
    from xtrl_amd import Learner
    base_kw = dict(num_episodes_per_update=2, batch_size=2, accelerate_kwargs=dict(device='cpu'), use_graph=False)
    kw = lambda **agent: dict(base_kw, agent_kwargs=dict(hidden_dim=48, **agent))   # noqa: E731
    base = dict(attn_dim_head=16, heads=4, depth=2, attn_gate_values=True, add_value_residual=True,
                learned_value_residual_mix=True)
    shapes = lambda learner: {k: tuple(v.shape) for k, v in learner.agent.model.state_dict().items()}   # noqa: E731
    plain = Learner(5, 2, (-1., 1.), world_model=dict(base), **kw())
    assert plain.agent.cfg.num_mem_kv == 0 and plain.agent.cfg.add_zero_kv is False
    pre = 'transformer.attn_layers.layers.'
    for kvh, Hkv in ((None, 4), (2, 2)):
        a = Learner(5, 2, (-1., 1.), world_model=dict(base, attn_num_mem_kv=4), **kw(kv_heads=kvh))
        sa = shapes(a)
        assert a.agent.cfg.num_mem_kv == 4 and a.agent.cfg.add_zero_kv is False
        for li in (0, 2):
            assert sa[f'{pre}{li}.1.mem_k'] == sa[f'{pre}{li}.1.mem_v'] == (Hkv, 4, 16)
        ref = shapes(Learner(5, 2, (-1., 1.), world_model=dict(base), **kw(kv_heads=kvh)))
        assert {k: s for k, s in sa.items() if not k.endswith(('.mem_k', '.mem_v'))} == ref
        assert len(sa) == len(ref) + 4
        # parameters of the flat buffer, in their block's gradient bucket, 16-byte aligned, randn-initialised
        agent = a.agent
        names = agent.model.flat_buckets_names()
        for li, bucket in ((0, names[2]), (1, names[1])):
            flat_names = [n for g in bucket for n in g]
            assert f'{pre}{2 * li}.1.mem_k' in flat_names and f'{pre}{2 * li}.1.mem_v' in flat_names
        for n in (f'{pre}0.1.mem_k', f'{pre}2.1.mem_v'):
            lo, hi = agent.flat.index[n]
            assert lo % 4 == 0 and hi - lo == Hkv * 4 * 16
            assert 0.5 < float(agent.flat.flat[lo:hi].std()) < 1.5
            assert torch.equal(agent.ema_flat[lo:hi], agent.flat.flat[lo:hi])
    z = Learner(5, 2, (-1., 1.), world_model=dict(base, attn_add_zero_kv=True), **kw())
    assert z.agent.cfg.add_zero_kv is True and z.agent.cfg.num_mem_kv == 0 and shapes(z) == shapes(plain)
    both = Learner(5, 2, (-1., 1.), world_model=dict(base, attn_add_zero_kv=True, attn_num_mem_kv=16,
                                                     attn_max_attend_past=5), **kw(kv_heads=2))
    assert (both.agent.cfg.num_mem_kv, both.agent.cfg.add_zero_kv, both.agent.cfg.attn_window) == (16, True, 5)
    for wm in (dict(attn_num_mem_kv=0), dict(attn_add_zero_kv=False), dict(attn_num_mem_kv=0, attn_add_zero_kv=False)):
        n = Learner(5, 2, (-1., 1.), world_model=dict(base, **wm), **kw())
        assert n.agent.cfg.num_mem_kv == 0 and n.agent.cfg.add_zero_kv is False and shapes(n) == shapes(plain)
    for bad in (-1, 17, 2.5, True, '4', None):
        with pytest.raises(ValueError, match='attn_num_mem_kv'):
            Learner(5, 2, (-1., 1.), world_model=dict(base, attn_num_mem_kv=bad), **kw())
    for bad in (1, 'yes', None, 1.0):
        with pytest.raises(ValueError, match='attn_add_zero_kv'):
            Learner(5, 2, (-1., 1.), world_model=dict(base, attn_add_zero_kv=bad), **kw())
    with pytest.raises(NotImplementedError, match='attn_num_mem_kv.*attn_qk_norm'):
        Learner(5, 2, (-1., 1.), world_model=dict(base, attn_num_mem_kv=2, attn_qk_norm=True), **kw())
    qz = Learner(5, 2, (-1., 1.), world_model=dict(base, attn_add_zero_kv=True, attn_qk_norm=True), **kw())
    assert qz.agent.cfg.add_zero_kv is True and qz.agent.cfg.qk_norm is True
    fbase = dict(attn_dim_head=16, heads=4, depth=1)
    for wm in (dict(attn_num_mem_kv=2), dict(attn_add_zero_kv=True)):
        with pytest.raises(NotImplementedError, match='attention sinks'):
            Learner(5, 2, (-1., 1.), world_model=dict(fbase, **wm), **kw(policy_body='fractal'))
    Learner(5, 2, (-1., 1.), world_model=dict(fbase, attn_num_mem_kv=0, attn_add_zero_kv=False),
            **kw(policy_body='fractal'))


def test_sink_checkpoint_roundtrip(tmp_path):
    """Agent.save / load and save_checkpoint / load_checkpoint keep mem_k / mem_v: the state dict holds them
    under x-transformers' names, and a second agent restores them (weights, EMA and moments) bit for bit."""
    from xtrl_amd import Learner
    kw = dict(world_model=dict(attn_dim_head=16, heads=4, depth=2, attn_num_mem_kv=3, attn_add_zero_kv=True),
              num_episodes_per_update=4, batch_size=2, accelerate_kwargs=dict(device='cpu'),
              agent_kwargs=dict(hidden_dim=16, kv_heads=2, save_path=str(tmp_path / 'ppo.pt')), use_graph=False)
    torch.manual_seed(0)
    a = Learner(5, 2, (-1., 1.), **kw).agent
    with torch.no_grad():
        a.opt_m.normal_()
        a.ema_flat.normal_()
    names = [f'transformer.attn_layers.layers.{li}.1.{p}' for li in (0, 2) for p in ('mem_k', 'mem_v')]
    a.save()
    data = torch.load(str(tmp_path / 'ppo.pt'), weights_only=True)
    for n in names:
        assert data['model'][n].shape == (2, 3, 16)
    torch.manual_seed(1)
    b = Learner(5, 2, (-1., 1.), **kw).agent
    sd_a, sd_b = a.model.state_dict(), b.model.state_dict()
    assert not torch.equal(sd_a[names[0]], sd_b[names[0]])
    b.load()
    for n in names:
        assert torch.equal(sd_a[n], b.model.state_dict()[n])
        lo, hi = b.flat.index[n]
        assert torch.equal(b.flat.flat[lo:hi], sd_a[n].reshape(-1))
    a.save_checkpoint()
    torch.manual_seed(2)
    c = Learner(5, 2, (-1., 1.), **kw).agent
    c.load_checkpoint()
    assert torch.equal(c.flat.flat, a.flat.flat) and torch.equal(c.ema_flat, a.ema_flat) and torch.equal(c.opt_m, a.opt_m)
    saved = torch.load(str(tmp_path / 'ppo.pt'), weights_only=True)
    assert all(n in saved['ema_flat'] and n in saved['opt_m'] for n in names)


def test_sink_entry_points_are_declared_bound_and_exported():
    """include/xtrl_hip.h declares the three _sink entry points — the _gqa signatures plus the sink operands,
    num_mem_kv and add_zero_kv before the stream — and the workspace size; the ctypes table binds them with
    the declared number of arguments; the library exports them, at ABI 25; the descriptors carry the
    fields."""
    from xtrl_amd import _lib
    text = (ROOT / 'include' / 'xtrl_hip.h').read_text()
    extra = dict(xtrl_attn_fwd_sink=4, xtrl_attn_bwd_sink=8, xtrl_attn_bwd_part_sink=8)
    for name, more in extra.items():
        m = re.search(r'int %s\(([^;]*)\);' % name, text)
        assert m, name
        args = ' '.join(m.group(1).split())
        assert 'const float* mem_k, const float* mem_v' in args, (name, args)
        assert 'int b, int H, int Hkv, int n, int dh' in args, (name, args)
        assert args.endswith('int window, int num_mem_kv, int add_zero_kv, void* stream'), (name, args)
        if 'bwd' in name:
            assert 'float* dmem_k, float* dmem_v, float* sink_ws, int64_t sink_ws_floats' in args, (name, args)
        res, sig = _lib.SIGNATURES[name]
        gres, gsig = _lib.SIGNATURES[name.replace('_sink', '_gqa')]
        assert res == gres and len(sig) == len(gsig) + more and len(sig) == args.count(',') + 1, name
    assert re.search(r'int64_t xtrl_attn_sink_ws_floats\(int b, int H, int num_mem_kv, int dh\);', text)
    assert _lib.ABI_VERSION == int(re.search(r'#define XTRL_ABI_VERSION (\d+)', text).group(1)) >= 25
    lib = _lib.load()
    assert lib.xtrl_abi_version() == _lib.ABI_VERSION
    for name in list(extra) + ['xtrl_attn_sink_ws_floats']:
        assert getattr(lib, name) is not None, name
    assert lib.xtrl_attn_sink_ws_floats(3, 4, 5, 16) >= 2 * 3 * 4 * 5 * 16
    assert lib.xtrl_attn_sink_ws_floats(3, 4, 0, 16) == 0
    fields = lambda s: [n for n, _ in s._fields_]   # noqa: E731
    assert fields(_lib.DecodeLayer)[-2:] == ['mem_k', 'mem_v'] and fields(_lib.TrainLayer)[-2:] == ['mem_k', 'mem_v']
    assert fields(_lib.DecodeDesc)[-2:] == ['num_mem_kv', 'add_zero_kv']
    assert fields(_lib.TrainDesc)[-4:] == ['num_mem_kv', 'add_zero_kv', 'sink_ws', 'sink_ws_floats']
