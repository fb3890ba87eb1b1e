"""Logit soft-clamp (world_model['attn_softclamp_logits'] / ['attn_logit_softclamp_value']) on the MI355X: the
learn-step kernels through the xtrl_attn_*_softclamp entry points and ops.attention against the fp64 dense
reference of test_attn_softclamp_cpu.attn_softclamp_ref (with the window, GQA, the sinks, with and without ALiBi
and in every backward mode; a saturated and a near-linear regime), against the _alibi entry points at
softclamp = 0, run to run, with dropout against the host keep bits, on the dead rows of a window and on the
values the C ABI refuses; then the rollout (both decode paths, the second 128-key chunk, a moving window, the
fused out-projection form), the padded and the packed learn step, the deploy forward and the reference-mode
autograd step against the soft-clamp oracle (test_attn_softclamp_cpu.softclamp_forward installed over the frozen
oracle's Attention)."""
import functools

import pytest
import torch

from oracle import philox as P

import attn_harness as AH
import test_gpu_parity as G
from attn_harness import NAMES, check_ref, modes_of, problem
from test_attn_alibi_gpu import SHAPES, SINKS, alibi_lib, dev_slopes
from test_attn_softclamp_cpu import attn_softclamp_ref, install_softclamp
from test_attn_sink_cpu import sink_dropout_keep, visible

pytestmark = pytest.mark.gpu
DEV = 'cuda'
# (c, the factor on q — and on mem_k): c = 2 with q x 4 — about 30 % of the visible scores saturated (|x / c| > 2),
# about 12 % linear (|x / c| < 0.3) — and the default c = 50 on unscaled scores, the near-linear regime
REGIMES = {'c2-q4': (2., 4.), 'c50': (50., 1.)}
softclamp_lib = functools.partial(AH.attn_lib, abi='softclamp')   # slopes=None: a NULL pointer; c=0.: off
softclamp_ref = functools.partial(AH.fp64_ref, attn_softclamp_ref)   # extra = (slopes or None, c)


# ----------------------------------------------------------------------------------------------
# kernel level
# ----------------------------------------------------------------------------------------------


@pytest.mark.parametrize('regime', list(REGIMES))
@pytest.mark.parametrize('alibi', [False, True])
@pytest.mark.parametrize('M,Z', SINKS)
@pytest.mark.parametrize('b,H,Hkv,n,dh,W', SHAPES)
def test_softclamp_forward_and_backward_against_fp64(b, H, Hkv, n, dh, W, M, Z, alibi, regime):
    """Forward + every backward mode of the shape at p = 0 against the fp64 reference (check_ref's bounds
    unchanged: o, lse 1e-5 + 1e-5, gradients 1e-4 + 1e-5), ragged lengths, every output NaN-filled before and
    finite after, with and without slopes.  n = 37 / 70 / 130: a partial tile, two and three key tiles; n = 200,
    W = 64: the band's first tile is not tile 0; H = 6 x 32 and dh = 64: the other head sizes; Hkv = 4, 2, 1: the kv
    head mappings.  'c2-q4' (c = 2, q and the memory keys x 4): saturated and linear scores side by side — a
    kernel without the 1 - t^2 factor, or with the clamp on the wrong side of the bias, is off by orders of
    magnitude; 'c50': the default on unscaled scores, where a cancelling tanh shows in lse."""
    c, f = REGIMES[regime]
    q, k, v, do, lens, *mem = problem(b, H, n, dh, n + dh + Hkv + (W or 0) + M, Hkv=Hkv, M=M)
    q = q * f
    mem_k, mem_v = mem or (None, None)
    if M:
        mem_k = mem_k * f
    slopes = dev_slopes(H) if alibi else None
    ref = softclamp_ref(q, k, v, do, lens, W, (slopes, c), mem_k, mem_v, Z)
    for mode in modes_of(n, dh):
        res = softclamp_lib(q, k, v, lens, do, dh ** -0.5, 0., mode, slopes=slopes, c=c, W=W, mem_k=mem_k, mem_v=mem_v, Z=Z)
        for name, t in res.items():
            assert torch.isfinite(t).all(), (mode, name)
        assert res['dk'].shape == (b, Hkv, n, dh) and (M == 0 or res['dmk'].shape == (Hkv, M, dh))
        for name in ref:
            err = float((res[name].double().cpu() - ref[name]).abs().max())
            print(f'softclamp {regime} alibi={int(alibi)} M={M} Z={Z} n={n} dh={dh} {mode} {name}: max err {err:.3e}')
        check_ref(res, ref)


def test_softclamp_reference_regimes_bite():
    """The 'c2-q4' inputs do what the test above relies on: more than 20 % of the visible scores saturated
    (|x / c| > 2), more than 5 % linear (|x / c| < 0.3), and the clamp moves o by far more than check_ref's bound."""
    b, H, Hkv, n, dh, W = SHAPES[1]
    c, f = REGIMES['c2-q4']
    q, k, v, do, lens = problem(b, H, n, dh, n + dh + Hkv, Hkv=Hkv)
    from xtrl_amd import ops
    kk = k[:, ops.kv_head_index(H, Hkv, device=DEV)].double()
    x = torch.einsum('bhid,bhjd->bhij', q.double() * f, kk) * dh ** -0.5
    y = (x / c).abs()[visible(n, lens, W).expand(b, H, n, n)]
    assert float((y > 2).double().mean()) > 0.2 and float((y < 0.3).double().mean()) > 0.05
    on = softclamp_ref(q * f, k, v, do, lens, W, (None, c))
    off = softclamp_ref(q * f, k, v, do, lens, W, (None, 1e9))
    assert float((on['o'] - off['o']).abs().max()) > 1e-2 and float((on['dq'] - off['dq']).abs().max()) > 1e-2


@pytest.mark.parametrize('W', [None, 10])
@pytest.mark.parametrize('n', [70, 130])
@pytest.mark.parametrize('p', [0., 0.25])
def test_softclamp_entry_points_at_zero_are_the_alibi_ones(p, n, W):
    """softclamp = 0 through the _softclamp entry points: o, lse, D, dq, dk, dv (and dmk, dmv with M = 3, Z = 1)
    bit-identical to the _alibi entry points in every backward mode, with slopes and with NULL, at Hkv = H and
    Hkv < H."""
    b, H, dh = 2, 4, 16
    for Hkv, M in ((4, 0), (2, 0), (2, 3)):
        q, k, v, do, lens, *mem = problem(b, H, n, dh, n + 3, Hkv=Hkv, M=M)
        kw = dict(W=W, mem_k=mem[0], mem_v=mem[1], Z=1) if M else dict(W=W)
        for slopes in (dev_slopes(H), None):
            for mode in modes_of(n, dh):
                old = alibi_lib(q, k, v, lens, do, dh ** -0.5, p, mode, slopes=slopes, **kw)
                new = softclamp_lib(q, k, v, lens, do, dh ** -0.5, p, mode, slopes=slopes, c=0., **kw)
                assert set(old) == set(new) and set(new) >= set(NAMES)
                for name in old:
                    assert torch.equal(old[name], new[name]), (Hkv, M, slopes is None, mode, name)


@pytest.mark.parametrize('Hkv,n,W', [(4, 300, 64), (2, 70, None)])
@pytest.mark.parametrize('p', [0., 0.25])
def test_softclamp_backward_repeats_bit_for_bit(p, Hkv, n, W):
    """Each backward mode run twice gives identical bits in every output (slopes, M = 3, Z = 1 along)."""
    b, H, dh = 3, 4, 16
    q, k, v, do, lens, mem_k, mem_v = problem(b, H, n, dh, n + Hkv, Hkv=Hkv, M=3)
    slopes = dev_slopes(H)
    for mode in modes_of(n, dh):
        one = softclamp_lib(q * 4, k, v, lens, do, dh ** -0.5, p, mode, slopes=slopes, c=2., W=W, mem_k=mem_k, mem_v=mem_v, Z=1)
        two = softclamp_lib(q * 4, k, v, lens, do, dh ** -0.5, p, mode, slopes=slopes, c=2., W=W, mem_k=mem_k, mem_v=mem_v, Z=1)
        for name in one:
            assert torch.isfinite(one[name]).all() and torch.equal(one[name], two[name]), (mode, name)


@pytest.mark.parametrize('p', [0.25, 0.3])
@pytest.mark.parametrize('Hkv,n,W,M', [(2, 130, None, 0), (1, 70, 10, 3)])
def test_softclamp_dropout_against_host_keep_bits(p, Hkv, n, W, M):
    """Dropout (p = 0.25: byte-mode real keys; 0.3: word mode): forward and all gradients of ops.attention with
    slopes and c = 2 (q x 4) against the fp64 reference times the host keep bits — oracle.philox.
    attn_dropout_keep for the real columns and test_attn_sink_cpu.sink_dropout_keep for the memory columns,
    exactly the masks of a run without the clamp."""
    from xtrl_amd import ops
    b, H, dh, c = 2, 4, 16, 2.
    g = torch.Generator().manual_seed(11 + n)
    q, do = (torch.randn(b, H, n, dh, generator=g) for _ in range(2))
    q = q * 4
    k, v = (torch.randn(b, Hkv, n, dh, generator=g) for _ in range(2))
    mem_k, mem_v = (torch.randn(Hkv, M, dh, generator=g) for _ in range(2)) if M else (None, None)
    lens = torch.tensor([n, 45], dtype=torch.int32)
    seed, offset, layer = 1234567, 5, 3
    slopes = ops.alibi_slopes(H)
    keep = torch.from_numpy(P.attn_dropout_keep(b, H, n, p, seed, offset, layer)).double() / (1 - p)
    keep_mem = torch.from_numpy(sink_dropout_keep(b, H, n, M, p, seed, offset, layer)).double() / (1 - p) if M else None
    ref = softclamp_ref(q, k, v, do, lens, W, (slopes, c), mem_k, mem_v, bool(M), keep, keep_mem)
    names = ('dq', 'dk', 'dv') + (('dmk', 'dmv') if M else ())
    leaves = [t.to(DEV).requires_grad_() for t in ((q, k, v, mem_k, mem_v) if M else (q, k, v))]
    out = ops.attention(*leaves[:3], lens.to(DEV), dh ** -0.5, p, seed=seed, offset=offset, sub=layer, window=W or 0,
                        mem_k=leaves[3] if M else None, mem_v=leaves[4] if M else None, add_zero_kv=bool(M),
                        alibi_slopes=slopes.to(DEV), softclamp=c)
    (out * do.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    del ref['lse']   # (ops.attention returns none)
    res = dict(o=out)
    for t, name in zip(leaves, names):
        assert t.grad.shape == ref[name].shape
        res[name] = t.grad
    check_ref(res, ref)


@pytest.mark.parametrize('p', [0., 0.25])
def test_softclamp_dead_rows_are_the_uniform_average(p):
    """W = 10 without sinks, padded layout: rows i >= 1 + W of the single-step episode see no key; the fill comes
    after the clamp, so they attend all n positions uniformly — o is bit for bit what a run without the clamp
    stores there (k_attn_dead_fwd) — and they pass no gradient: dq of those rows is 0, dk of the episode's padded
    keys too."""
    b, H, Hkv, n, dh, W = 2, 4, 2, 130, 16, 10
    q, k, v, do, lens = problem(b, H, n, dh, 5, Hkv=Hkv)
    assert int(lens[b - 1]) == 1
    a = softclamp_lib(q * 4, k, v, lens, do, dh ** -0.5, p, 'two', c=2., W=W)
    z = softclamp_lib(q * 4, k, v, lens, do, dh ** -0.5, p, 'two', c=0., W=W)
    dead = slice(1 + W, n)
    assert torch.equal(a['o'][b - 1, :, dead], z['o'][b - 1, :, dead])
    assert not torch.equal(a['o'][0], z['o'][0])
    if p == 0.:
        from xtrl_amd import ops
        want = v[b - 1, ops.kv_head_index(H, Hkv, device=DEV)].double().mean(1)   # [H][dh]
        G.tol(a['o'][b - 1, :, dead], want[:, None, :].expand(-1, n - 1 - W, -1).float(), 1e-5, 1e-5)
    assert torch.equal(a['dq'][b - 1, :, dead], torch.zeros_like(a['dq'][b - 1, :, dead]))
    assert torch.equal(a['dk'][b - 1, :, 1:], torch.zeros_like(a['dk'][b - 1, :, 1:]))
    assert torch.equal(a['lse'][b - 1, :, dead], torch.zeros_like(a['lse'][b - 1, :, dead]))


@pytest.mark.parametrize('bad', [-1., -1e-30, float('nan'), float('inf'), float('-inf')])
def test_softclamp_c_abi_refuses_a_negative_or_non_finite_value(bad):
    """softclamp < 0, NaN or infinite: XTRL_E_ARG with the value in the message from each of the three entry
    points, and no kernel ran — every NaN-filled output still holds NaN."""
    from xtrl_amd import _lib as L
    b, H, Hkv, n, dh = 2, 4, 2, 37, 16
    q, k, v, do, lens = problem(b, H, n, dh, 7, Hkv=Hkv)
    with pytest.raises(RuntimeError, match='softclamp') as ei:
        softclamp_lib(q, k, v, lens, do, dh ** -0.5, 0., 'two', c=bad)
    want = {-1.: 'softclamp -1 ', -1e-30: 'softclamp -1e-30 ', float('inf'): 'softclamp inf ', float('-inf'): 'softclamp -inf '}
    msg = str(ei.value).lower()
    assert ('nan' in msg) if bad != bad else (want[bad] in msg), msg
    for t in AH.attn_lib.last.values():
        assert torch.isnan(t).all()
    lib = L.lib()
    nan = lambda *s: torch.full(s, float('nan'), device=DEV)   # noqa: E731
    o, lse, dq, dk, dv, delta = nan(*q.shape), nan(b, H, n), nan(*q.shape), nan(*k.shape), nan(*v.shape), nan(b, H, n)
    io = tuple(L.ptr(t) for t in (q, k, v, lens, q, lse, do, dq, dk, dv, delta))   # (o: any finite tensor)
    tail = (b, H, Hkv, n, dh, dh ** -0.5, 0., 3, 1, 0, 0, 0, 0, None, bad, L.stream())
    nf = int(lib.xtrl_attn_bwd_part_floats(b, H, n, dh))
    part = nan(nf)
    assert lib.xtrl_attn_bwd_softclamp(*io, None, None, None, None, None, 0, *tail) == 1
    assert 'softclamp' in lib.xtrl_last_error().decode()
    assert lib.xtrl_attn_bwd_part_softclamp(*io, L.ptr(part), nf, None, None, None, None, None, 0, *tail) == 1
    torch.cuda.synchronize()
    for t in (o, dq, dk, dv, delta, part):
        assert torch.isnan(t).all()


# ----------------------------------------------------------------------------------------------
# model level: the soft-clamp oracle (test_attn_softclamp_cpu.softclamp_forward over the frozen Attention)
# ----------------------------------------------------------------------------------------------

# (ALiBi, W, M, Z, Hkv)
CONFIGS = {'plain': (False, None, 0, False, None), 'w5+zero': (False, 5, 0, True, None),
           'gqa2+mem3': (False, None, 3, False, 2), 'alibi': (True, None, 0, False, None),
           'alibi+w5+zero': (True, 5, 0, True, None)}
LEARNER = dict(episodes=6, batch=3, hazard=4)   # seed 3 at hazard 2^-4: lengths 4 .. T, ragged minibatches
# A freshly initialised model's scores are a few tenths at most: c = 0.25 bites (on the CPU oracle it moves the
# rollout's log-probs past compare_rollout's bound by 3.7e-3 or more in every case below); attn_qk_norm's scores
# reach +-10: c = 5.  test_softclamp_changes_the_rollout asserts it on the device for every entry of CASES
C = 0.25
# every model-level configuration the tests below run: name -> (CONFIGS key or tuple, c, T, rows (None: both decode
# paths), further keywords of G.make_learner).  Each parity test takes its configuration from here, and
# test_softclamp_changes_the_rollout runs every one of them with and without the option
CASES = {
    **{name: (name, C, 40, None, {}) for name in CONFIGS},
    'long': ('alibi', C, 140, None, dict(depth=1, episodes=4, batch=2, hazard=12)),
    'alibi+w5': ((True, 5, 0, False, None), C, 40, None, {}),
    'd256': ('w5+zero', C, 40, '0', dict(dim=256)),
    'd384': ('w5+zero', C, 40, '0', dict(dim=384)),
    'dh32': ((False, 5, 0, True, 2), C, 40, None, dict(dim_head=32, dim=64)),
    'dh64': ((True, 5, 3, True, None), C, 40, None, dict(heads=2, dim_head=64, dim=48)),
    'qknorm+xpos': ('w5+zero', 5., 40, None, dict(wm_extra=dict(attn_qk_norm=True, rotary_xpos=True,
                                                                 rotary_xpos_scale_base=8.))),
}


def learner_kw(alibi, W, M, Z, Hkv, **kw):
    """G.make_learner's keywords of a CONFIGS entry (the soft-clamp and ALiBi options go in through
    install_softclamp)."""
    return dict(window=W, num_mem_kv=M, add_zero_kv=Z, **({} if Hkv is None else dict(agent_extra=dict(kv_heads=Hkv))),
                **kw)


def case_of(name):
    """A CASES entry resolved: (ALiBi, W, M, Z, Hkv), c, T, rows, heads, G.make_learner's keywords."""
    cfg, c, T, rows, kw = CASES[name]
    cfg = CONFIGS[cfg] if isinstance(cfg, str) else cfg
    kw = {**LEARNER, **learner_kw(*cfg, **kw)}
    return cfg, c, T, rows, kw.get('heads', 4), kw


def softclamp_rollout_and_learn(monkeypatch, name, minibatches, packed=False):
    """attn_harness.rollout_and_learn of the CASES entry ``name`` against the soft-clamp oracle."""
    (alibi, W, M, Z, Hkv), c, T, _, heads, kw = case_of(name)

    def checks(learner, env, oracle):
        cf = learner.agent.cfg
        assert (cf.softclamp, cf.alibi_heads, cf.attn_window, cf.num_mem_kv, cf.add_zero_kv, cf.n_kv_heads) == \
            (c, heads if alibi else 0, W or 0, M, Z, Hkv or heads)
        eng = learner._engine_for(env, T)
        assert eng.desc.attn_softclamp == c and bool(eng.desc.alibi_slopes) == alibi

    return AH.rollout_and_learn(monkeypatch, lambda mp: install_softclamp(mp, heads, c, alibi, None, W, M, Z, Hkv), T,
                                minibatches, packed, checks, **kw)


@pytest.mark.parametrize('rows', ['1', '0'])
@pytest.mark.parametrize('cfg', list(CONFIGS))
def test_softclamp_rollout_and_learn_match_oracle(cfg, rows, monkeypatch):
    """Heads 4 x 16, d = 48, depth 2 with gates and the learned mix, T = 40, c = 0.25: both decode paths (the
    row-resident step and the multi-kernel step), then two padded learn minibatches, against the soft-clamp
    oracle — plain; W = 5 with the zero key; kv_heads 2 with 3 memory rows; ALiBi; ALiBi with W = 5 and the zero
    key."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', rows)
    learner, lens, seen = softclamp_rollout_and_learn(monkeypatch, cfg, 2)
    assert (learner._engine[1].rows_max > 0) == (rows == '1')
    assert int(lens.max()) > 20 and len(seen) == 2


@pytest.mark.parametrize('rows', ['1', '0'])
def test_softclamp_long_rollout_second_key_chunk(rows, monkeypatch):
    """T = 140, depth 1, ALiBi, no window: the keys past the first 128-key chunk of k_attn_decode (and the second
    round trip of the row kernel's score loop)."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', rows)
    _, lens, _ = softclamp_rollout_and_learn(monkeypatch, 'long', 0)
    assert int(lens.max()) > 130


@pytest.mark.parametrize('rows', ['1', '0'])
def test_softclamp_windowed_rollout_past_the_pointer_shift(rows, monkeypatch):
    """T = 40, W = 5, ALiBi, no sinks: from step 6 on j_lo > 0."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', rows)
    _, lens, _ = softclamp_rollout_and_learn(monkeypatch, 'alibi+w5', 0)
    assert int(lens.max()) > 20


@pytest.mark.parametrize('name', ['d256', 'd384'])
def test_softclamp_fused_out_projection_rollout(name, monkeypatch):
    """d = 256 and d = 384 (the FJ = 1 and FJ = 2 forms), T = 40, W = 5 with the zero key: the attention decode
    kernel that applies the out-projection itself."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', '0')
    _, lens, _ = softclamp_rollout_and_learn(monkeypatch, name, 0)
    assert int(lens.max()) > 20


@pytest.mark.parametrize('cfg', ['plain', 'gqa2+mem3', 'alibi+w5+zero'])
def test_softclamp_packed_learn_matches_oracle(cfg, monkeypatch):
    """The packed learn step on three of the configs."""
    learner, _, seen = softclamp_rollout_and_learn(monkeypatch, cfg, 2, packed=True)
    assert learner.agent.packed_learn and len(seen) == 2


def test_softclamp_dh32_rollout_and_learn_match_oracle(monkeypatch):
    """4 heads x 32 (d = 64), kv_heads 2, W = 5 and the zero key: the dh = 32 forms of every soft-clamp kernel."""
    _, lens, seen = softclamp_rollout_and_learn(monkeypatch, 'dh32', 2)
    assert int(lens.max()) > 20 and len(seen) == 2


@pytest.mark.parametrize('rows', ['1', '0'])
def test_softclamp_dh64_rollout_and_learn_match_oracle(rows, monkeypatch):
    """2 heads x 64 (d = 48), ALiBi, W = 5, 3 memory rows and the zero key: the dh = 64 forms of every soft-clamp
    kernel, on both decode paths."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', rows)
    learner, lens, seen = softclamp_rollout_and_learn(monkeypatch, 'dh64', 2)
    assert (learner._engine[1].rows_max > 0) == (rows == '1')
    assert int(lens.max()) > 20 and len(seen) == 2


@pytest.mark.parametrize('rows', ['1', '0'])
def test_softclamp_with_qk_norm_and_xpos_rollout_and_learn_match_oracle(rows, monkeypatch):
    """attn_qk_norm (scores q . k x 10 of unit vectors: up to +-10) with attn_logit_softclamp_value = 5, so |x / c|
    reaches 2, and rotary_xpos, with W = 5 and the zero key: rollout on both decode paths, then two padded learn
    minibatches."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', rows)
    learner, lens, seen = softclamp_rollout_and_learn(monkeypatch, 'qknorm+xpos', 2)
    assert learner.agent.cfg.qk_norm and learner.agent.cfg.rotary_xpos and len(seen) == 2


@pytest.mark.parametrize('cfg', ['plain', 'alibi+w5+zero'])
def test_softclamp_deploy_forward_matches_oracle_cached_decode(cfg, monkeypatch):
    """Agent.forward over 10 steps against the soft-clamp oracle's cached decode (G.deploy_parity)."""
    alibi, W, M, Z, Hkv = CONFIGS[cfg]
    install_softclamp(monkeypatch, 4, C, alibi, None, W, M, Z, Hkv)
    learner, env, oracle = G.make_learner(T=24, **LEARNER, **learner_kw(alibi, W, M, Z, Hkv))
    assert learner.agent.cfg.softclamp == C
    G.deploy_parity(learner, oracle, 10)


@pytest.mark.parametrize('p', [0., 0.25])
@pytest.mark.parametrize('cfg', ['plain', 'gqa2+mem3', 'alibi+w5+zero'])
def test_softclamp_fused_step_matches_reference_mode_autograd(cfg, p, monkeypatch):
    """The hand-scheduled learn step against the reference-mode autograd step (fused_learn=False: model.
    forward_train with ops.attention taking the value), T = 40: the bounds of
    test_fused_train_step_matches_autograd."""
    alibi, W, M, Z, Hkv = CONFIGS[cfg]
    install_softclamp(monkeypatch, 4, C, alibi, None, W, M, Z, Hkv)

    def checks(learner, env, oracle):
        assert learner.agent.cfg.softclamp == C

    G._fused_vs_autograd(False, False, True, p, 40, depth=2, episodes=8, batch=4, hazard=4, dim=64, checks=checks,
                         with_oracle=False, **learner_kw(alibi, W, M, Z, Hkv))


@pytest.mark.parametrize('name', list(CASES))
def test_softclamp_changes_the_rollout(name):
    """The feature is live on the device in every model-level configuration the parity tests run (CASES: the same
    G.make_learner keywords, value, T and decode path): the same seed with and without the option gives
    log-probs that differ by more than compare_rollout's tolerance (1e-4 relative + 1e-5) over the steps both
    runs share.  Without this a parity test whose value does not bite would pass with the clamp left out."""
    (alibi, W, M, Z, Hkv), c, T, rows, heads, kw = case_of(name)

    def run(value):
        with pytest.MonkeyPatch.context() as mp:
            if rows is not None:
                mp.setenv('XTRL_DECODE_ROWS', rows)
            install_softclamp(mp, heads, value, alibi, None, W, M, Z, Hkv)
            learner, env, _ = G.make_learner(T=T, with_oracle=False, **kw)
            assert learner.agent.cfg.softclamp == (value or 0.)
            traj, lens, _, _ = learner.rollout_device(env, 0, T)
            torch.cuda.synchronize()
            return traj['logp'].cpu(), traj['actions'].cpu(), lens.cpu()

    (a, aa, la), (b, ab, lb) = run(c), run(None)
    # the steps both runs share: up to the first step at which their sampled actions differ (the rewards, an
    # input of the next step, follow the actions), within both lengths
    worst = 0.
    for e in range(a.shape[0]):
        n = int(min(la[e], lb[e]))
        same = (aa[e, :n] == ab[e, :n]).long().cumprod(0)
        m = min(n, int(same.sum()) + 1)
        worst = max(worst, float(((a[e, :m] - b[e, :m]).abs() - (1e-5 + 1e-4 * b[e, :m].abs())).max()))
    print(f'softclamp bite {name}: log-prob excess over the bound {worst:.3e}')
    assert worst > 0, worst
