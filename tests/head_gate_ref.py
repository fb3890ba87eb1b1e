"""Per-head output gates (world_model['attn_gate_value_heads']): what the CPU and the GPU tests share.  The patched
oracle — HeadGateAttention, a subclass of the frozen oracle's Attention with ``to_v_head_gate`` = Linear(dim, heads)
(weight 0, bias 10, as x-transformers initialises it) whose forward applies sigmoid(to_v_head_gate(x)) to each
head's attention output before the heads are merged, then the element-wise to_v_gate gate — installed over
``oracle.thirdparty.Attention`` by install_head_gate, the way attn_harness.rollout_and_learn expects; the
randomisation of the gate parameters the model-level tests use; and the fp64 references of the learn step's two
row kernels (xtrl_head_gate_fwd / xtrl_head_gate_bwd) with the bounds the GPU tests hold them to.

Semantics (x-transformers Attention.forward, restated): with o[t, h, :] the output of softmax . V, the sinks
included,
    og[t, h, c] = o[t, h, c] sigmoid(x[t] . W_hg[h] + b_hg[h]) (sigmoid(x[t] . W_g[h dh + c] + b_g[h dh + c]))
one gate per query head whatever kv_heads is.

A plain module that defines no tests."""
import torch
import torch.nn.functional as F
from torch import nn

from oracle import thirdparty as tp

from test_attn_sink_cpu import sink_init

FROZEN = tp.Attention   # the frozen oracle's class, taken before anything is patched over the name


# ----------------------------------------------------------------------------------------------
# the patched oracle
# ----------------------------------------------------------------------------------------------


def head_gate_attention(W=None, zero_kv=False, slopes=None, c=None, Hkv=None, M=0, gated=True, heads=None):
    """The subclass of the frozen Attention with the per-head gate and, as the option files' oracles have them,
    the window ``W``, the zero key, ALiBi ``slopes`` [heads], the soft-clamp value ``c``, ``Hkv`` kv heads and ``M``
    memory rows (test_attn_softclamp_cpu.softclamp_forward's scores; ``heads``: the query head count, needed with
    ``M`` when ``Hkv`` is None).  ``gated`` False: the same class without
    the gate's parameter and multiply — the unpatched oracle of that configuration."""
    base_init = sink_init(Hkv or heads, M) if (M or Hkv is not None) else FROZEN.__init__

    class HeadGateAttention(FROZEN):
        def __init__(self, dim, heads, dim_head, *args, **kw):
            base_init(self, dim, heads, dim_head, *args, **kw)
            self.to_v_head_gate = None
            if gated:
                self.to_v_head_gate = nn.Linear(dim, heads)
                nn.init.constant_(self.to_v_head_gate.weight, 0.)
                nn.init.constant_(self.to_v_head_gate.bias, 10.)

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
            if c is not None:
                sim = c * torch.tanh(sim / c)
            neg = -torch.finfo(sim.dtype).max
            causal = torch.ones((i, j), dtype=torch.bool, device=x.device).triu(j - i + 1)
            sim = sim.masked_fill(causal, neg)
            if W is not None:
                sim = sim.masked_fill(dist > W, neg)
            if key_mask is not None:
                sim = sim.masked_fill(~key_mask[:, None, None, :], neg)
            mem_k = getattr(self, 'mem_k', None)
            Mm = 0 if mem_k is None else mem_k.shape[1]
            cols = [sim]
            if Mm:
                sm = torch.einsum('bhid,hmd->bhim', q, mem_k.repeat(rep, 1, 1)) * scale
                cols.append(sm if c is None else c * torch.tanh(sm / c))
            if zero_kv:
                cols.append(sim.new_zeros(b, h, i, 1))
            attn = self.attn_dropout(torch.cat(cols, dim=-1).softmax(dim=-1, dtype=torch.float32))
            out = torch.einsum('bhij,bhjd->bhid', attn[..., :j], vr)
            if Mm:
                out = out + torch.einsum('bhim,hmd->bhid', attn[..., j:j + Mm], self.mem_v.repeat(rep, 1, 1))
            if self.to_v_head_gate is not None:   # 'b n h -> b h n 1', before the heads are merged
                out = out * self.to_v_head_gate(x).permute(0, 2, 1).unsqueeze(-1).sigmoid()
            out = out.permute(0, 2, 1, 3).reshape(b, n, h * dh)
            if self.to_v_gate is not None:
                out = out * self.to_v_gate(x).sigmoid()
            return self.to_out(out), (k, v), orig_v

    return HeadGateAttention


def randomise_head_gates(model, seed=77):
    """to_v_head_gate.weight ~ N(0, 1) / sqrt(d), .bias ~ N(0, 1) in every attention block of ``model`` (a device
    model or an oracle), from one CPU generator: the initial weight 0, bias 10 leaves every gate within 5e-5 of
    open, which a kernel that ignores the gate would pass."""
    g = torch.Generator().manual_seed(seed)
    n = 0
    with torch.no_grad():
        for name, p in model.named_parameters():
            if 'to_v_head_gate' in name:
                r = torch.randn(p.shape, generator=g)
                p.copy_((r / p.shape[-1] ** 0.5 if p.ndim == 2 else r).to(p.device))
                n += 1
    assert n > 0, 'the model has no to_v_head_gate'
    return model


def install_head_gate(monkeypatch, heads, W=None, M=0, Z=False, Hkv=None, alibi=False, c=None, on=True):
    """HeadGateAttention over the frozen Attention and the option into every Learner built afterwards:
    test_gpu_parity.make_learner takes no head-gate keyword and imports ``xtrl_amd.Learner`` when called, so that
    name is wrapped to add attn_gate_value_heads (and ALiBi / the soft-clamp with ``alibi`` / ``c``) to the
    world_model it is given and to randomise the new Learner's gate parameters (randomise_head_gates) before
    make_learner copies the weights to the EMA model and the oracle.  ``on`` False: the same model and oracle
    without the option."""
    import xtrl_amd
    from xtrl_amd import ops
    slopes = ops.alibi_slopes(heads, None) if alibi else None
    monkeypatch.setattr(tp, 'Attention', head_gate_attention(W, Z, slopes, c, Hkv, M, gated=on, heads=heads))
    real = xtrl_amd.Learner

    def learner(*args, world_model, **kw):
        extra = dict(attn_gate_value_heads=True) if on else {}
        if c is not None:
            extra.update(attn_softclamp_logits=True, attn_logit_softclamp_value=float(c))
        if alibi:
            extra.update(alibi_pos_bias=True)
        made = real(*args, world_model=dict(world_model, **extra), **kw)
        if on:
            randomise_head_gates(made.agent.model)
        return made

    monkeypatch.setattr(xtrl_amd, 'Learner', learner)
    return slopes


def force_gates_open(model):
    """Context manager: every to_v_head_gate of ``model`` at weight 0, bias +40 (sigmoid(40) rounds to 1 in fp32
    and in fp64 differs from 1 by 4e-18), restored on exit — the model without the gate."""
    import contextlib

    @contextlib.contextmanager
    def cm():
        saved = {n: p.detach().clone() for n, p in model.named_parameters() if 'to_v_head_gate' in n}
        assert saved
        with torch.no_grad():
            for n, p in model.named_parameters():
                if n in saved:
                    p.fill_(40. if n.endswith('bias') else 0.)
        try:
            yield
        finally:
            with torch.no_grad():
                for n, p in model.named_parameters():
                    if n in saved:
                        p.copy_(saved[n])

    return cm()


# ----------------------------------------------------------------------------------------------
# the row kernels: problem, fp64 references, fp32 restatement, bounds
# ----------------------------------------------------------------------------------------------

SPECIAL_LOGITS = (0., 30., -30., 100., -100.)   # gate logits every problem holds: s = 1/2, ~1, ~0, 1, 0
SENTINEL = -7.25                                 # the columns of proj / dproj no kernel owns


def row_problem(T, H, dh, n_qkv, elem_gate, seed, gap=0):
    """One launch's operands on the CPU, fp32: o, C [T][I] ~ N(0, 1); proj [T][n_qkv] = SENTINEL except the head-gate
    logits at its last H columns (N(0, 2), the first entries of the flattened [T][H] SPECIAL_LOGITS); dproj
    [T][n_qkv] = SENTINEL except, with ``elem_gate``, the element gate's I columns at gate_col = n_qkv - H - gap - I
    (N(0, 1): what the DGATE epilogue wrote; ``gap``: sentinel columns between them and the head gates', where
    the mix's sit).  Returns a dict."""
    I = H * dh   # noqa: E741
    hg_col = n_qkv - H
    gate_col = hg_col - gap - I if elem_gate else -1
    assert hg_col >= (I + gap if elem_gate else 0)
    g = torch.Generator().manual_seed(seed)
    o, C = torch.randn(T, I, generator=g), torch.randn(T, I, generator=g)
    logits = torch.randn(T, H, generator=g) * 2.
    flat = logits.view(-1)
    k = min(flat.numel(), len(SPECIAL_LOGITS))
    flat[:k] = torch.tensor(SPECIAL_LOGITS[:k])
    proj = torch.full((T, n_qkv), SENTINEL)
    proj[:, hg_col:] = logits
    dproj = torch.full((T, n_qkv), SENTINEL)
    if elem_gate:
        dproj[:, gate_col:gate_col + I] = torch.randn(T, I, generator=g)
    return dict(T=T, H=H, dh=dh, n_qkv=n_qkv, hg_col=hg_col, gate_col=gate_col, o=o, C=C, proj=proj, dproj=dproj)


def ref_fwd(src, proj, H, dh, hg_col, dtype=torch.float64):
    """og = src sigmoid(proj[:, hg_col + h]) in ``dtype``."""
    T = src.shape[0]
    s = torch.sigmoid(proj[:, hg_col:hg_col + H].to(dtype))
    return (src.to(dtype).view(T, H, dh) * s[:, :, None]).reshape(T, H * dh)


def ref_bwd(C, o, proj, dproj, H, dh, hg_col, gate_col, dtype=torch.float64):
    """The backward row pass in ``dtype``: (dog, dproj, sum_abs) with dog = C s, dproj's head-gate columns
    (sum_c C o) s (1 - s), its element-gate columns times s, every other column as given; sum_abs [T][H] =
    sum_c |C o| s (1 - s), the scale of the gate gradient's bound."""
    T = C.shape[0]
    I = H * dh   # noqa: E741
    s = torch.sigmoid(proj[:, hg_col:hg_col + H].to(dtype))
    Ch, oh = C.to(dtype).view(T, H, dh), o.to(dtype).view(T, H, dh)
    out = dproj.to(dtype).clone()
    out[:, hg_col:hg_col + H] = (Ch * oh).sum(-1) * s * (1 - s)
    if gate_col >= 0:
        out[:, gate_col:gate_col + I] = (out[:, gate_col:gate_col + I].view(T, H, dh) * s[:, :, None]).reshape(T, I)
    return (Ch * s[:, :, None]).reshape(T, I), out, (Ch * oh).abs().sum(-1) * s * (1 - s)


# The bounds of the GPU tests against the fp64 references (settled without a GPU by test_attn_head_gate_cpu.
# test_fp32_restatement_fits_a_quarter_of_the_bounds): the gate gradient within GRAD_REL sum_c |C o| s (1 - s) +
# GRAD_ABS (a sum of up to 64 fp32 terms: 64 x 2^-24 = 3.8e-6 relative to the sum of their magnitudes), the
# element outputs within ELEM_REL |x| + ELEM_ABS
GRAD_REL, GRAD_ABS = 1e-5, 1e-7
ELEM_REL, ELEM_ABS = 1e-5, 1e-6


def bwd_excess(dog, dproj, ref, p, scale=1.):
    """The worst ratio error / bound of a backward result (fp32 tensors) against ref_bwd's fp64 triple, per kind:
    dict(grad, dog, egate) (egate only with an element gate).  ``scale``: the fraction of the bounds to hold."""
    rdog, rdp, sabs = ref
    hg, gc, I = p['hg_col'], p['gate_col'], p['H'] * p['dh']   # noqa: E741
    out = dict(
        grad=float(((dproj[:, hg:hg + p['H']].double() - rdp[:, hg:hg + p['H']]).abs()
                    / (scale * (GRAD_REL * sabs + GRAD_ABS))).max()),
        dog=float(((dog.double() - rdog).abs() / (scale * (ELEM_REL * rdog.abs() + ELEM_ABS))).max()))
    if gc >= 0:
        e = rdp[:, gc:gc + I]
        out['egate'] = float(((dproj[:, gc:gc + I].double() - e).abs() / (scale * (ELEM_REL * e.abs() + ELEM_ABS))).max())
    return out
