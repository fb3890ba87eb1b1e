"""Per-head output gates (world_model['attn_gate_value_heads']) on the MI355X: the learn step's two row kernels
through xtrl_head_gate_fwd / xtrl_head_gate_bwd against the fp64 references of head_gate_ref (outputs NaN before
the call, every column of proj / dproj the kernel does not own bit-identical after it, row strides with n_qkv % 4
in {0, 1, 3}, the vector and the scalar form of the element gate's columns, gate logits 0, +-30, +-100); then, with
randomised gate weights and the patched oracle (head_gate_ref.HeadGateAttention): the rollout on both decode
kernels and with the fused out-projection tails, the padded and the packed learn step, the reference-mode
autograd step and the deploy forward.  Every model-level case first asserts, on the CPU, that the patched
oracle's logits differ from the same oracle's with its gates forced open by more than 100 x the comparison
tolerance: a kernel that ignores the gate cannot pass.

Bounds (head_gate_ref, settled by test_attn_head_gate_cpu.test_fp32_restatement_fits_a_quarter_of_the_bounds):
the gate gradient within 1e-5 sum_c |C o| s (1 - s) + 1e-7, the element outputs within 1e-5 |x| + 1e-6."""
import pytest
import torch

import attn_harness as AH
import head_gate_ref as HG
import test_gpu_parity as G

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPES = [(1, 16), (3, 16), (4, 16), (5, 32), (9, 16), (2, 64)]   # (H, dh): one lane group, odd head counts, 4 / 8 / 16 lanes
TS = [1, 15, 17, 257]   # one token; a partial block; past one block of 64 / 32 / 16 groups; many blocks with a tail


# ----------------------------------------------------------------------------------------------
# kernel level
# ----------------------------------------------------------------------------------------------


def _variants(H, dh, elem_gate):
    """(n_qkv, gap, vector form expected) of one shape: a row of ``front`` leading sentinel columns | the element
    gate's I (opt) | ``gap`` sentinel columns | H head gates, with n_qkv % 4 = 0 twice (the element gate's columns
    16-byte aligned: the float4 form; one column off: scalar accesses on an aligned stride), 1 and 3."""
    I = H * dh if elem_gate else 0   # noqa: E741
    out = []
    for res, front in ((0, 8), (0, 9), (1, 8), (3, 10)):
        gap = (res - (front + I + H)) % 4
        out.append((front + I + gap + H, gap, bool(elem_gate and res == 0 and front % 4 == 0)))
    assert [n % 4 for n, _, _ in out] == [0, 0, 1, 3], out
    return out


def _run_fwd(p, src, og):
    from xtrl_amd import _lib as L
    I = p['H'] * p['dh']   # noqa: E741
    proj = p['proj'].to(DEV)
    rc = L.lib().xtrl_head_gate_fwd(L.ptr(src), I, L.ptr(proj), p['n_qkv'], L.ptr(og), I, p['T'], p['H'], p['dh'],
                                    p['hg_col'], L.stream())
    torch.cuda.synchronize()
    return rc, proj.cpu()


@pytest.mark.parametrize('elem_gate', [False, True])
@pytest.mark.parametrize('T', TS)
@pytest.mark.parametrize('H,dh', SHAPES)
def test_head_gate_forward_against_fp64(H, dh, T, elem_gate):
    """og = src sigmoid(logit) within 1e-5 |x| + 1e-6 of the fp64 reference: out of place from o into an og that
    holds NaN (no element gate), in place on og (with one: the attention kernel wrote it), at every row stride of
    _variants; proj comes back bit for bit; a logit of -100 gives exactly 0, +100 exactly the input."""
    for n_qkv, gap, _ in _variants(H, dh, elem_gate):
        p = HG.row_problem(T, H, dh, n_qkv, elem_gate, seed=T + H * dh + n_qkv, gap=gap)
        ref = HG.ref_fwd(p['o'], p['proj'], H, dh, p['hg_col'])
        if elem_gate:
            og = p['o'].to(DEV)
            src = og
        else:
            src, og = p['o'].to(DEV), torch.full((T, H * dh), float('nan'), device=DEV)
        rc, proj = _run_fwd(p, src, og)
        assert rc == 0
        got = og.cpu()
        assert torch.isfinite(got).all()
        excess = float(((got.double() - ref).abs() / (HG.ELEM_REL * ref.abs() + HG.ELEM_ABS)).max())
        print(f'head_gate_fwd H={H} dh={dh} T={T} n_qkv={n_qkv}: error / bound {excess:.3f}')
        assert excess <= 1., (n_qkv, excess)
        assert torch.equal(proj, p['proj'])
        if not elem_gate:
            assert torch.equal(src.cpu(), p['o'])
        logits = p['proj'][:, p['hg_col']:].reshape(-1)
        g3 = got.view(T * H, dh)
        for i in range(min(T * H, len(HG.SPECIAL_LOGITS))):
            if logits[i] == -100.:
                assert (g3[i] == 0).all()
            if logits[i] == 100.:
                assert torch.equal(g3[i], p['o'].view(T * H, dh)[i])


@pytest.mark.parametrize('elem_gate', [False, True])
@pytest.mark.parametrize('T', TS)
@pytest.mark.parametrize('H,dh', SHAPES)
def test_head_gate_backward_against_fp64(H, dh, T, elem_gate):
    """The backward row pass against the fp64 reference at every row stride of _variants: dproj's head-gate
    columns hold NaN before the call and the gate gradient after it (within 1e-5 sum |C o| s (1 - s) + 1e-7; at
    logits +-100 exactly 0, never NaN), dog = C s in place and the element gate's columns times s (1e-5 |x| +
    1e-6), o and proj untouched, every other column of dproj bit-identical to its sentinel."""
    from xtrl_amd import _lib as L
    I = H * dh   # noqa: E741
    for n_qkv, gap, vec in _variants(H, dh, elem_gate):
        p = HG.row_problem(T, H, dh, n_qkv, elem_gate, seed=3 * T + H * dh + n_qkv, gap=gap)
        hg, gc = p['hg_col'], p['gate_col']
        assert vec == (gc >= 0 and gc % 4 == 0 and n_qkv % 4 == 0)
        ref = HG.ref_bwd(p['C'], p['o'], p['proj'], p['dproj'], H, dh, hg, gc)
        dog, o, proj = p['C'].to(DEV), p['o'].to(DEV), p['proj'].to(DEV)
        dproj0 = p['dproj'].clone()
        dproj0[:, hg:] = float('nan')
        dproj = dproj0.to(DEV)
        rc = L.lib().xtrl_head_gate_bwd(L.ptr(dog), I, L.ptr(o), I, L.ptr(proj), n_qkv, L.ptr(dproj), n_qkv, T, H, dh, hg,
                                        gc, L.stream())
        torch.cuda.synchronize()
        assert rc == 0
        dog, dproj = dog.cpu(), dproj.cpu()
        assert torch.isfinite(dog).all() and torch.isfinite(dproj).all()
        worst = HG.bwd_excess(dog, dproj, ref, p)
        print(f'head_gate_bwd H={H} dh={dh} T={T} n_qkv={n_qkv} vec={vec}: error / bound {worst}')
        assert all(v <= 1. for v in worst.values()), (n_qkv, worst)
        own = torch.zeros(n_qkv, dtype=torch.bool)
        own[hg:] = True
        if gc >= 0:
            own[gc:gc + I] = True
        assert torch.equal(dproj[:, ~own], p['dproj'][:, ~own])
        assert torch.equal(o.cpu(), p['o']) and torch.equal(proj.cpu(), p['proj'])
        logits, grad = p['proj'][:, hg:].reshape(-1), dproj[:, hg:].reshape(-1)
        for i in range(min(T * H, len(HG.SPECIAL_LOGITS))):
            if abs(float(logits[i])) == 100.:
                assert float(grad[i]) == 0., (float(logits[i]), float(grad[i]))


def test_head_gate_entries_refuse_without_touching_their_outputs():
    """A refused call (dim_head 48; a leading dimension that is no multiple of 4; head-gate columns past the
    row) returns XTRL_E_ARG and launches nothing: og, dog and dproj keep their NaN."""
    from xtrl_amd import _lib as L
    lib = L.lib()
    nan = lambda *s: torch.full(s, float('nan'), device=DEV)   # noqa: E731
    o, og, dog, proj, dproj = torch.zeros(8, 96, device=DEV), nan(8, 96), nan(8, 96), torch.zeros(8, 104, device=DEV), nan(8, 104)
    calls = [lambda: lib.xtrl_head_gate_fwd(L.ptr(o), 96, L.ptr(proj), 104, L.ptr(og), 96, 8, 2, 48, 100, L.stream()),
             lambda: lib.xtrl_head_gate_fwd(L.ptr(o), 96, L.ptr(proj), 104, L.ptr(og), 94, 8, 6, 16, 98, L.stream()),
             lambda: lib.xtrl_head_gate_fwd(L.ptr(o), 96, L.ptr(proj), 104, L.ptr(og), 96, 8, 6, 16, 99, L.stream()),
             lambda: lib.xtrl_head_gate_bwd(L.ptr(dog), 96, L.ptr(o), 96, L.ptr(proj), 104, L.ptr(dproj), 104, 8, 2, 48, 100,
                                            -1, L.stream()),
             lambda: lib.xtrl_head_gate_bwd(L.ptr(dog), 96, L.ptr(o), 96, L.ptr(proj), 104, L.ptr(dproj), 104, 8, 6, 16, 98,
                                            5, L.stream())]
    for call in calls:
        assert call() == 1
        assert lib.xtrl_last_error().decode().startswith('head_gate_')
    torch.cuda.synchronize()
    for t in (og, dog, dproj):
        assert torch.isnan(t).all()


# ----------------------------------------------------------------------------------------------
# model level: the patched oracle, randomised gate weights
# ----------------------------------------------------------------------------------------------

T = 24
LEARNER = dict(episodes=6, batch=3, hazard=4)   # seed 3 at hazard 2^-4: ragged lengths up to T
# name -> (install_head_gate's keywords, G.make_learner's keywords)
CASES = {
    'plain': (dict(), dict(gates=False)),
    'gates+mix': (dict(), dict(gates=True)),
    'kv1-h3': (dict(Hkv=1), dict(gates=True, heads=3, kv_heads=1)),
    'w5+zero+mem2': (dict(W=5, Z=True, M=2), dict(gates=True, window=5, add_zero_kv=True, num_mem_kv=2)),
    'alibi+clamp': (dict(alibi=True, c=0.25), dict(gates=True)),
    'd256': (dict(), dict(gates=True, dim=256)),    # the attention decode kernel with the out-projection tail, FJ = 1
    'd384': (dict(), dict(gates=False, dim=384)),   # ... FJ = 2
}


def _gate_bites(oracle, S=8):
    """On the CPU: the patched oracle's actor and critic logits against the same oracle with every gate forced
    open (the unpatched oracle: test_attn_head_gate_cpu) differ by more than 100 x compare_rollout's tolerance
    (1e-4 relative + 1e-5) somewhere."""
    m = oracle.model
    was = m.training
    m.eval()
    state = torch.randn(2, 12, S, generator=torch.Generator().manual_seed(5))
    with torch.no_grad():
        live = m(state)[:2]
        with HG.force_gates_open(m):
            opened = m(state)[:2]
    m.train(was)
    excess = max(float(((a - b).abs() - 100 * (1e-5 + 1e-4 * b.abs())).max()) for a, b in zip(live, opened))
    print(f'head gate bite: logits beyond 100 x the tolerance by {excess:.3e}')
    assert excess > 0, excess


def _checks(heads):
    def checks(learner, env, oracle):
        cf = learner.agent.cfg
        assert cf.gate_value_heads and cf.heads == heads
        eng = learner._engine_for(env, T)
        assert eng.desc.head_gate == 1
        assert eng.desc.n_qkv == cf.inner + 2 * cf.kv_inner + (cf.inner if cf.gate_values else 0) + \
            (cf.n_kv_heads if (cf.value_residual and cf.learned_mix) else 0) + heads
        if oracle is not None:
            _gate_bites(oracle)
    return checks


def _rollout_and_learn(monkeypatch, name, minibatches, packed=False):
    inst, kw = CASES[name]
    heads = kw.get('heads', 4)
    return AH.rollout_and_learn(monkeypatch, lambda mp: HG.install_head_gate(mp, heads, **inst), T, minibatches, packed,
                                _checks(heads), **{**LEARNER, **kw})


@pytest.mark.parametrize('rows', ['1', '0'])
@pytest.mark.parametrize('name', ['plain', 'gates+mix', 'kv1-h3', 'w5+zero+mem2', 'alibi+clamp'])
def test_head_gate_rollout_and_learn_match_oracle(name, rows, monkeypatch):
    """Depth 2, d = 48, T = 24, 6 episodes: the rollout on the row-resident step (k_decode_row; one workgroup per
    env row, hidden_dim <= 128) and on the multi-kernel step (k_attn_decode), then two padded learn minibatches,
    against the patched oracle — the head gate alone; on top of attn_gate_values with the learned value-residual
    mix; one kv head under three query heads; window 5 with the zero key and 2 memory rows; ALiBi with the
    soft-clamp."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', rows)
    learner, lens, seen = _rollout_and_learn(monkeypatch, name, 2)
    assert (learner._engine[1].rows_max > 0) == (rows == '1')
    assert int(lens.max()) > 12 and len(seen) == 2


@pytest.mark.parametrize('name', ['d256', 'd384'])
def test_head_gate_fused_out_projection_rollout(name, monkeypatch):
    """d = 256 and d = 384: the attention decode kernel that applies the out-projection itself (FJ = 1, FJ = 2)."""
    monkeypatch.setenv('XTRL_DECODE_ROWS', '0')
    _, lens, _ = _rollout_and_learn(monkeypatch, name, 0)
    assert int(lens.max()) > 12


@pytest.mark.parametrize('name', ['plain', 'gates+mix'])
def test_head_gate_packed_learn_matches_oracle(name, monkeypatch):
    """The packed learn step (the valid rows only: the row kernels take their count as T)."""
    learner, _, seen = _rollout_and_learn(monkeypatch, name, 2, packed=True)
    assert learner.agent.packed_learn and len(seen) == 2


@pytest.mark.parametrize('p', [0., 0.25])
@pytest.mark.parametrize('name', ['plain', 'gates+mix', 'kv1-h3'])
def test_head_gate_fused_step_matches_reference_mode_autograd(name, p, monkeypatch):
    """The hand-scheduled learn step against the reference-mode autograd step (fused_learn=False: model.
    forward_train applies the gate), T = 24, 8 episodes: the bounds of test_fused_train_step_matches_autograd."""
    inst, kw = CASES[name]
    heads = kw.get('heads', 4)
    HG.install_head_gate(monkeypatch, heads, **inst)
    kw = dict(kw)
    gates = kw.pop('gates')
    G._fused_vs_autograd(False, False, gates, p, T, depth=2, episodes=8, batch=4, hazard=4, dim=64, checks=_checks(heads),
                         with_oracle=False, **kw)


@pytest.mark.parametrize('name', ['plain', 'gates+mix'])
def test_head_gate_deploy_forward_matches_oracle_cached_decode(name, monkeypatch):
    """Agent.forward over 10 steps against the patched oracle's cached decode (G.deploy_parity)."""
    inst, kw = CASES[name]
    HG.install_head_gate(monkeypatch, 4, **inst)
    learner, env, oracle = G.make_learner(T=T, **LEARNER, **kw)
    assert learner.agent.cfg.gate_value_heads
    _gate_bites(oracle)
    G.deploy_parity(learner, oracle, 10)
