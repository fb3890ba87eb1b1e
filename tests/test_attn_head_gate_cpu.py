"""Per-head output gates (world_model['attn_gate_value_heads']) without a GPU: the option's handling and the
fractal body's refusal; the new parameters' names, shapes, initial values and their place in the flat buffer
and the fused projection view; the strict state-dict round trip with the patched oracle (head_gate_ref.
HeadGateAttention); model.forward_train's gate arithmetic against that oracle with the GEMM and attention
launches replaced by their dense CPU statements; the patched oracle with its gates forced open against the
unpatched one; the C ABI (version, descriptors, the two test entries and the checks they make before any
launch); and the bounds the GPU tests hold the row kernels to, settled on an fp32 restatement."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_port as R
from oracle import thirdparty as tp

import head_gate_ref as HG

ROOT = Path(__file__).resolve().parents[1]
BASE = dict(attn_dim_head=16, heads=4, depth=2, attn_gate_values=True, add_value_residual=True,
            learned_value_residual_mix=True)
PRE = 'transformer.attn_layers.layers.'


def _kw(**agent):
    return dict(num_episodes_per_update=2, batch_size=2, accelerate_kwargs=dict(device='cpu'), use_graph=False,
                agent_kwargs=dict(hidden_dim=48, **agent))


def _learner(wm=None, **agent):
    from xtrl_amd import Learner
    return Learner(5, 2, (-1., 1.), world_model=dict(BASE, **(wm or {})), **_kw(**agent))


def test_head_gate_option_handling():
    """attn_gate_value_heads=True sets ModelConfig.gate_value_heads; False, the x-transformers default, builds
    today's model; a non-bool is refused by name; the fractal body refuses the option by name."""
    from xtrl_amd import Learner
    from xtrl_amd.learner import XT_DEFAULTS
    assert XT_DEFAULTS['attn_gate_value_heads'] is False
    plain, on = _learner(), _learner(dict(attn_gate_value_heads=True))
    assert plain.agent.cfg.gate_value_heads is False and on.agent.cfg.gate_value_heads is True
    off = _learner(dict(attn_gate_value_heads=False))
    assert list(off.agent.model.state_dict()) == list(plain.agent.model.state_dict())
    assert _learner(dict(attn_gate_value_heads=np.bool_(True))).agent.cfg.gate_value_heads is True
    for bad in ('yes', 1, 2, None, 1.5, (True,)):
        with pytest.raises(ValueError, match='attn_gate_value_heads'):
            _learner(dict(attn_gate_value_heads=bad))
    # composes with the other attention options
    c = _learner(dict(attn_gate_value_heads=True, attn_softclamp_logits=True, alibi_pos_bias=True,
                      attn_max_attend_past=5, attn_num_mem_kv=2, attn_add_zero_kv=True), kv_heads=2).agent.cfg
    assert (c.gate_value_heads, c.softclamp, c.alibi_heads, c.attn_window, c.kv_heads, c.num_mem_kv) == \
        (True, 50., 4, 5, 2, 2)
    fbase = dict(attn_dim_head=16, heads=4, depth=1)
    with pytest.raises(NotImplementedError, match='attn_gate_value_heads'):
        Learner(5, 2, (-1., 1.), world_model=dict(fbase, attn_gate_value_heads=True), **_kw(policy_body='fractal'))
    Learner(5, 2, (-1., 1.), world_model=dict(fbase, attn_gate_value_heads=False), **_kw(policy_body='fractal'))


@pytest.mark.parametrize('gates,kv_heads,heads', [(True, None, 4), (False, None, 4), (True, 1, 3), (False, 1, 3)])
def test_head_gate_parameters_and_flat_layout(gates, kv_heads, heads):
    """to_v_head_gate = Linear(d, heads) per attention block, weight 0 and bias 10, whatever kv_heads is; its
    weight closes the fused projection view (the last H rows), its bias the projection's bias span; every
    earlier row, the mix's column among them, sits where it does without the option."""
    from xtrl_amd import Learner
    wm = dict(attn_dim_head=16, heads=heads, depth=3)
    if gates:
        wm.update(attn_gate_values=True, add_value_residual=True, learned_value_residual_mix=True)
    mk = lambda **o: Learner(5, 2, (-1., 1.), world_model=dict(wm, **o), **_kw(kv_heads=kv_heads)).agent   # noqa: E731
    a, plain = mk(attn_gate_value_heads=True), mk()
    d, H, I = 48, heads, heads * 16   # noqa: E741
    Hkv = kv_heads or heads
    sd = a.model.state_dict()
    new = [k for k in sd if k not in plain.model.state_dict()]
    assert new == [f'{PRE}{2 * li}.1.to_v_head_gate.{p}' for li in range(3) for p in ('weight', 'bias')]
    a.model.bind_flat(a.flat, a.gemm_ws)
    plain.model.bind_flat(plain.flat, plain.gemm_ws)
    for li in range(3):
        w, b = sd[f'{PRE}{2 * li}.1.to_v_head_gate.weight'], sd[f'{PRE}{2 * li}.1.to_v_head_gate.bias']
        assert tuple(w.shape) == (H, d) and tuple(b.shape) == (H,)
        assert torch.equal(w, torch.zeros(H, d)) and torch.equal(b, torch.full((H,), 10.))
        P, Q = a.model._proj[li], plain.model._proj[li]
        mix = gates and li > 0
        n_qkv = I + 2 * Hkv * 16 + (I if gates else 0) + (Hkv if mix else 0) + H
        assert tuple(P['w'].shape) == (n_qkv, d) and P['w'].is_contiguous() and tuple(Q['w'].shape) == (n_qkv - H, d)
        assert P['hg_col'] == n_qkv - H and P['mix_col'] == Q['mix_col'] == I + 2 * Hkv * 16 + (I if gates else 0)
        blk = a.model.blocks()[li][0][1]
        assert P['w'][-H:].data_ptr() == blk.to_v_head_gate.weight.data_ptr()
        assert P['b'][-H:].data_ptr() == blk.to_v_head_gate.bias.data_ptr()
        assert P['b'].numel() == (I if gates else 0) + (Hkv if mix else 0) + H
        if mix:
            assert P['w'][P['mix_col']:P['mix_col'] + Hkv].data_ptr() == blk.to_value_residual_mix[0].weight.data_ptr()
        assert P['w'][:1].data_ptr() == blk.to_q.weight.data_ptr()


def _oracle_for(agent, T, monkeypatch, gated=True, **cfg):
    """The oracle model of ``agent``'s configuration with HeadGateAttention installed, weights from the agent
    (strict load)."""
    monkeypatch.setattr(tp, 'Attention', HG.head_gate_attention(Hkv=cfg.pop('Hkv', None), gated=gated))
    c = agent.cfg
    m = R.OracleWMAC(R.ModelConfig(c.state_dim, c.num_actions, dim=c.dim, depth=c.depth, heads=c.heads,
                                   dim_head=c.dim_head, max_timesteps=T, reward_range=c.reward_range,
                                   gate_values=c.gate_values, value_residual=c.value_residual,
                                   learned_mix=c.learned_mix))
    return m.eval()


def test_head_gate_state_dict_round_trip_with_the_patched_oracle(monkeypatch):
    """The device model's state dict loads strictly into the patched oracle and back: the names and shapes are
    x-transformers' (…to_v_head_gate.weight / .bias)."""
    agent = _learner(dict(attn_gate_value_heads=True)).agent
    HG.randomise_head_gates(agent.model)
    oracle = _oracle_for(agent, 8, monkeypatch)
    sd = {k: v.detach().clone() for k, v in agent.model.state_dict().items()}
    res = oracle.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    back = oracle.state_dict()
    assert list(back) == list(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    with torch.no_grad():
        for v in back.values():
            v.mul_(0.5)
    agent.model.load_state_dict(back, strict=True)
    assert all(torch.equal(agent.model.state_dict()[k], sd[k] * 0.5) for k in sd)
    # without the subclass the frozen oracle refuses the new names
    monkeypatch.setattr(tp, 'Attention', HG.FROZEN)
    with pytest.raises(RuntimeError, match='to_v_head_gate'):
        _oracle_for_frozen(agent).load_state_dict(sd, strict=True)


def _oracle_for_frozen(agent):
    c = agent.cfg
    return R.OracleWMAC(R.ModelConfig(c.state_dim, c.num_actions, dim=c.dim, depth=c.depth, heads=c.heads,
                                      dim_head=c.dim_head, max_timesteps=8, reward_range=c.reward_range,
                                      gate_values=c.gate_values, value_residual=c.value_residual,
                                      learned_mix=c.learned_mix))


def _cpu_ops(monkeypatch):
    """model.forward_train's launches as their dense CPU statements (p = 0, no window, no sinks): the projection,
    column offsets, gates and merges of forward_train itself are what runs."""
    from xtrl_amd import ops

    def attention(q, k, v, lens, scale, *a, **kw):
        assert not kw.get('window') and kw.get('mem_k') is None and not kw.get('add_zero_kv') and \
            kw.get('alibi_slopes') is None and not kw.get('softclamp')
        n, rep = q.shape[2], q.shape[1] // k.shape[1]
        k, v = k.repeat(1, rep, 1, 1), v.repeat(1, rep, 1, 1)
        sim = torch.einsum('bhid,bhjd->bhij', q, k) * scale
        neg = -torch.finfo(sim.dtype).max
        sim = sim.masked_fill(torch.ones(n, n, dtype=torch.bool).triu(1), neg)
        sim = sim.masked_fill(~(torch.arange(n)[None, :] < lens[:, None])[:, None, None, :], neg)
        return torch.einsum('bhij,bhjd->bhid', sim.softmax(-1), v)

    monkeypatch.setattr(ops, 'xlinear', lambda x, w, b, wg, bg, ws, bg_off=0: F.linear(x, w, b))
    monkeypatch.setattr(ops, 'attention', attention)
    monkeypatch.setattr(ops, 'linear_gelu_drop', lambda x, w, b, wg, bg, ws, p, seed, off, layer: F.gelu(F.linear(x, w, b)))


def _forward_pair(agent, oracle, seed=5, b=3, n=7):
    """(device model's forward_train raw actions and critic logits, the oracle's) on one random minibatch."""
    g = torch.Generator().manual_seed(seed)
    S, A = agent.cfg.state_dim, agent.cfg.num_actions
    state, rewards = torch.randn(b, n, S, generator=g), torch.randn(b, n, generator=g)
    actions = torch.randint(-1, A, (b, n), generator=g)
    nxt = torch.randint(0, A, (b, n), generator=g)
    lens = torch.tensor([n, 3, 1][:b], dtype=torch.int32)
    with torch.no_grad():
        agent.model.eval()
        raw, values, _, _ = agent.model.forward_train(state, actions, rewards, nxt, None, lens)
        oraw, ovalues, _, _, _ = oracle(state, actions=actions, rewards=rewards, next_actions=nxt,
                                        mask=torch.arange(n)[None, :] < lens[:, None])
    valid = (torch.arange(n)[None, :] < lens[:, None])
    return (raw[valid], values[valid]), (oraw[valid], ovalues[valid])


@pytest.mark.parametrize('gates,kv_heads,heads', [(True, None, 4), (False, None, 4), (True, 1, 3)])
def test_forward_train_applies_the_gate_as_the_patched_oracle(gates, kv_heads, heads, monkeypatch):
    """Randomised gate weights (N(0, 1) / sqrt(d), bias N(0, 1)): the reference-mode forward equals the patched
    oracle within 1e-4 + 1e-5, and the oracle with its gates forced open is far from both — with the element
    gate and the learned mix, without them, and with one kv head under three query heads."""
    from xtrl_amd import Learner
    wm = dict(attn_dim_head=16, heads=heads, depth=2, attn_gate_value_heads=True)
    if gates:
        wm.update(attn_gate_values=True, add_value_residual=True, learned_value_residual_mix=True)
    torch.manual_seed(0)
    agent = Learner(5, 2, (-1., 1.), world_model=wm, **_kw(kv_heads=kv_heads, dropout=0.)).agent
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():   # non-trivial element gates and mixes too (their init is constant)
        for name, p in agent.model.named_parameters():
            if 'to_v_gate' in name or 'to_value_residual_mix' in name:
                p.copy_(torch.randn(p.shape, generator=g) * 0.3)
    HG.randomise_head_gates(agent.model)
    oracle = _oracle_for(agent, 8, monkeypatch, Hkv=kv_heads)
    oracle.load_state_dict({k: v.detach().clone() for k, v in agent.model.state_dict().items()}, strict=True)
    _cpu_ops(monkeypatch)
    got, want = _forward_pair(agent, oracle)
    for a, b in zip(got, want):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5)
    with HG.force_gates_open(oracle):
        _, opened = _forward_pair(agent, oracle)
    excess = max(float(((a - b).abs() - 100 * (1e-5 + 1e-4 * b.abs())).max()) for a, b in zip(opened, want))
    assert excess > 0, excess


def test_patched_oracle_with_open_gates_is_the_unpatched_oracle(monkeypatch):
    """Gate logits forced to +40 (weight 0, bias 40: sigmoid rounds to 1 in fp32): the patched oracle is the
    oracle of the same configuration without the gate, bit for bit; with the randomised gates it is not."""
    agent = _learner(dict(attn_gate_value_heads=True), dropout=0.).agent
    HG.randomise_head_gates(agent.model)
    sd = {k: v.detach().clone() for k, v in agent.model.state_dict().items()}
    g = torch.Generator().manual_seed(3)
    state = torch.randn(2, 6, 5, generator=g)
    # (one installed class at a time: the oracle's Decoder finds its attention blocks by the installed name)
    plain = _oracle_for(agent, 8, monkeypatch, gated=False)
    plain.load_state_dict({k: v for k, v in sd.items() if 'to_v_head_gate' not in k}, strict=True)
    with torch.no_grad():
        want = plain(state)
    patched = _oracle_for(agent, 8, monkeypatch)
    patched.load_state_dict(sd, strict=True)
    with torch.no_grad():
        with HG.force_gates_open(patched):
            got = patched(state)
        live = patched(state)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert float((live[0] - want[0]).abs().max()) > 1e-3
    # and the ungated subclass is the frozen class's arithmetic
    monkeypatch.setattr(tp, 'Attention', HG.FROZEN)
    froz = _oracle_for_frozen(agent).eval()
    froz.load_state_dict({k: v for k, v in sd.items() if 'to_v_head_gate' not in k}, strict=True)
    with torch.no_grad():
        f = froz(state)
    torch.testing.assert_close(f[0], want[0], rtol=1e-6, atol=1e-6)


# ----------------------------------------------------------------------------------------------
# C ABI
# ----------------------------------------------------------------------------------------------


def test_head_gate_abi_is_declared_bound_and_exported():
    """ABI 33 in the header, the binding and the library; both descriptors carry ``int head_gate`` and their
    sizes and field lists agree with the header; the two test entries are declared, bound with one ctypes
    argument per C argument, and exported; no XTRL_ROWS_* / XTRL_DECODE_* op was added for them."""
    from xtrl_amd import _lib
    text = (ROOT / 'include' / 'xtrl_hip.h').read_text()
    abi = int(re.search(r'#define XTRL_ABI_VERSION (\d+)', text).group(1))
    assert abi == _lib.ABI_VERSION == 33
    lib = _lib.load()
    assert lib.xtrl_abi_version() == 33
    for desc, cname in ((_lib.DecodeDesc, 'XtrlDecodeDesc'), (_lib.TrainDesc, 'XtrlTrainDesc')):
        assert dict(desc._fields_)['head_gate'] is _lib.I32
        body = re.search(r'typedef struct %s \{(.*?)\n\} %s;' % (cname, cname), text, re.S).group(1)
        body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
        assert re.search(r'\bint head_gate;', body), cname
        names = re.findall(r'(\w+)\s*(?:,|;)', re.sub(r'\[[^\]]*\]', '', body))
        assert names == [n for n, _ in desc._fields_], cname
        assert int(lib.xtrl_struct_size(cname.encode())) == ctypes.sizeof(desc), cname
    for name, nargs in (('xtrl_head_gate_fwd', 11), ('xtrl_head_gate_bwd', 14)):
        m = re.search(r'int %s\(([^;]*)\);' % name, text)
        assert m and m.group(1).count(',') + 1 == nargs, name
        res, sig = _lib.SIGNATURES[name]
        assert res is _lib.I32 and len(sig) == nargs and sig[-1] is _lib.P, name
        assert getattr(lib, name) is not None
    assert 'HEAD_GATE' not in ' '.join(_lib.ROWS_OPS + _lib.DECODE_OPS)
    assert not re.search(r'#define XTRL_(ROWS|DECODE)_\w*GATE', text)


def test_head_gate_entries_refuse_before_any_launch():
    """The argument checks are host code in front of the launch, so they are reachable without a GPU: every
    refusal is XTRL_E_ARG with a message that names the entry; a fine call with T = 0 launches nothing and
    returns 0."""
    from xtrl_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    p = ctypes.c_void_p((base + 15) & ~15)        # a 16-byte aligned, non-null address (never read: T = 0 or refused)
    off = ctypes.c_void_p(p.value + 4)
    fwd = lambda **o: lib.xtrl_head_gate_fwd(*[{**dict(src=p, ld_src=64, proj=p, ld_proj=70, og=p, ld_og=64, T=0, H=4,   # noqa: E731
                                                       dh=16, hg_col=66, stream=None), **o}[k]
                                               for k in ('src', 'ld_src', 'proj', 'ld_proj', 'og', 'ld_og', 'T', 'H', 'dh',
                                                         'hg_col', 'stream')])
    bwd = lambda **o: lib.xtrl_head_gate_bwd(*[{**dict(dog=p, ld_dog=64, o=p, ld_o=64, proj=p, ld_proj=134, dproj=p,   # noqa: E731
                                                       ld_dproj=134, T=0, H=4, dh=16, hg_col=130, gate_col=64,
                                                       stream=None), **o}[k]
                                               for k in ('dog', 'ld_dog', 'o', 'ld_o', 'proj', 'ld_proj', 'dproj', 'ld_dproj',
                                                         'T', 'H', 'dh', 'hg_col', 'gate_col', 'stream')])
    assert fwd() == 0 and bwd() == 0 and bwd(gate_col=-1) == 0
    refused = [(fwd, dict(dh=8)), (fwd, dict(dh=48)), (fwd, dict(dh=128)), (bwd, dict(dh=24)),
               (fwd, dict(src=None)), (fwd, dict(proj=None)), (fwd, dict(og=None)),
               (bwd, dict(dog=None)), (bwd, dict(o=None)), (bwd, dict(proj=None)), (bwd, dict(dproj=None)),
               (fwd, dict(T=2 ** 30, H=4)), (bwd, dict(T=2 ** 30, H=4)), (fwd, dict(T=-1)), (fwd, dict(H=0)),
               (fwd, dict(ld_src=60)), (fwd, dict(ld_og=66)), (fwd, dict(src=off)), (bwd, dict(o=off)),
               (fwd, dict(hg_col=67)), (fwd, dict(hg_col=-1)), (bwd, dict(ld_dproj=133)),
               (bwd, dict(gate_col=-2)), (bwd, dict(gate_col=71)), (bwd, dict(gate_col=128, ld_dproj=200, ld_proj=200))]
    for call, o in refused:
        T = o.get('T', 5)   # a launch would follow: the refusal must come first
        assert call(**{**o, 'T': T}) == 1, o
        msg = lib.xtrl_last_error().decode()
        assert msg.startswith('head_gate_fwd' if call is fwd else 'head_gate_bwd'), (o, msg)
    assert 'beyond the grid' in (fwd(T=2 ** 30, H=4), lib.xtrl_last_error().decode())[1]


# ----------------------------------------------------------------------------------------------
# the row kernels' bounds
# ----------------------------------------------------------------------------------------------


def _fp32_bwd(p):
    """The backward kernel's arithmetic restated in fp32 on the CPU: per (token, head) dh / 4 partial sums of four
    products each, combined pairwise (the lane group's butterfly); s (1 - s) formed as sigmoid(x) sigmoid(-x), as
    the kernel does — with 1 - s in fp32 a nearly open gate (x = 8: 1 - s = 3e-4) alone is off by 2e-4 relative,
    twenty times the bound."""
    T, H, dh = p['T'], p['H'], p['dh']
    I, hg, gc = H * dh, p['hg_col'], p['gate_col']   # noqa: E741
    x = p['proj'][:, hg:hg + H]
    s, s1 = 1. / (1. + torch.exp(-x)), 1. / (1. + torch.exp(x))   # sigmoid(x), sigmoid(-x) = 1 - s without the cancellation
    C, o = p['C'].view(T, H, dh // 4, 4), p['o'].view(T, H, dh // 4, 4)
    pr = C * o
    part = (pr[..., 0] + pr[..., 1]) + (pr[..., 2] + pr[..., 3])
    while part.shape[-1] > 1:
        part = part[..., 0::2] + part[..., 1::2]
    dproj = p['dproj'].clone()
    dproj[:, hg:hg + H] = part[..., 0] * s * s1
    if gc >= 0:
        dproj[:, gc:gc + I] = (dproj[:, gc:gc + I].view(T, H, dh) * s[:, :, None]).reshape(T, I)
    return (p['C'].view(T, H, dh) * s[:, :, None]).reshape(T, I), dproj


@pytest.mark.parametrize('H,dh', [(1, 16), (3, 16), (4, 16), (5, 32), (9, 16), (2, 64)])
@pytest.mark.parametrize('elem_gate', [False, True])
def test_fp32_restatement_fits_a_quarter_of_the_bounds(H, dh, elem_gate):
    """The GPU bounds (head_gate_ref.GRAD_REL / GRAD_ABS, ELEM_REL / ELEM_ABS) hold with a factor 4 to spare for
    an fp32 restatement of the backward at T = 257, every column outside the kernel's own comes back bit for
    bit, and the special logits (0, +-30, +-100) give a gradient that is exactly 0 or finite, never NaN."""
    I = H * dh   # noqa: E741
    p = HG.row_problem(257, H, dh, I + 2 * dh + (I if elem_gate else 0) + 1 + H, elem_gate, seed=H * dh)
    dog, dproj = _fp32_bwd(p)
    ref = HG.ref_bwd(p['C'], p['o'], p['proj'], p['dproj'], H, dh, p['hg_col'], p['gate_col'])
    worst = HG.bwd_excess(dog, dproj, ref, p, scale=0.25)
    print(f'head-gate fp32 restatement H={H} dh={dh} gate={elem_gate}: error / (bound / 4) = {worst}')
    assert all(v <= 1. for v in worst.values()), worst
    own = torch.zeros(p['n_qkv'], dtype=torch.bool)
    own[p['hg_col']:] = True
    if elem_gate:
        own[p['gate_col']:p['gate_col'] + I] = True
    assert torch.equal(dproj[:, ~own], p['dproj'][:, ~own])
    g = dproj[:, p['hg_col']:].reshape(-1)[:len(HG.SPECIAL_LOGITS)]
    assert torch.isfinite(dproj).all() and torch.isfinite(dog).all()
    for v, logit in zip(g.tolist(), HG.SPECIAL_LOGITS):
        if abs(logit) >= 100.:
            assert v == 0., (logit, v)
    og = HG.ref_fwd(p['o'], p['proj'], H, dh, p['hg_col'], dtype=torch.float32)
    ref_og = HG.ref_fwd(p['o'], p['proj'], H, dh, p['hg_col'])
    assert float(((og.double() - ref_og).abs() / (0.25 * (HG.ELEM_REL * ref_og.abs() + HG.ELEM_ABS))).max()) <= 1.
