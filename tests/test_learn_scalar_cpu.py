"""CPU companion of test_learn_scalar_gpu.py: settles the inputs of the scalar learn-step kernels'
tests without a GPU.  For every fused-loss input set the GPU file uses: the kink margin of the
fp64 reference (no token within 1e-5 of a decision boundary, so the fp32 kernel and the fp64
reference take the same branch everywhere), the direction of the global critic minimum, the branch
census and the saturation constructions.  For the other kernels: that the case tables hold the
sizes and edges they are there for."""
import math

import pytest
import torch

import learn_scalar_cases as C
from oracle import ref_port as R
from oracle import thirdparty as tp


@pytest.mark.parametrize('case', C.ALL_LOSS_CASES, ids=C.case_id)
def test_loss_inputs_margin_direction_census(case):
    C.check_case(case)
    ins = C.loss_inputs(case)
    if case.b > 1:
        assert case.n in ins['lens'].tolist() and 1 in ins['lens'].tolist()
    ref = C.loss_reference(case)
    assert all(bool(torch.isfinite(g).all()) for g in ref['grads']) and math.isfinite(float(ref['loss']))


def test_loss_shape_cases_cover_every_axis_value():
    cs = C.SHAPE_CASES
    assert {c.B for c in cs} >= {2, 63, 64, 65, 127}
    assert {c.A for c in cs if not c.cont} >= {1, 2, 32} and {c.A for c in cs if c.cont} >= {1, 6}
    assert {c.S1 for c in cs} >= {1, 2, 64, 65, 70}
    assert {(c.b, c.n) for c in cs} >= {(1, 2), (3, 17), (5, 23)}
    assert all((c.b * c.n) % 4 and (c.b * c.n) % 16 for c in cs if c.b > 1)
    for c in C.LARGE_CASES:   # a second trip of k_loss_stats' 1024-thread loop, 67 partials for k_loss_final
        assert -(-c.b * c.n // 16) == 1057 and -(-c.b * c.n // 256) == 67
    assert {c.hl_mean for c in C.LARGE_CASES} == {True, False}


def test_loss_both_directions_of_the_global_min():
    dirs = {c.direction for c in C.ALL_LOSS_CASES if c.hl_mean and c.direction}
    assert dirs == {'L', 'Lc'}
    modes = {(c.squash, c.hl_mean) for c in C.MODE_CASES if c.cont}
    assert modes >= {(False, True), (False, False), (True, False)}


def test_loss_reference_is_the_existing_tests_combination():
    """loss_reference restates test_gpu_parity.test_fused_loss_matches_oracle's combination: with
    its hyper-parameters the per-term means recombine to the loss."""
    c = C.MODE_CASES[2]
    ref, ins = C.loss_reference(c), C.loss_inputs(c)
    n_mask = int(ins['lens'].sum())
    assert n_mask == int(ref['tokens']['mask'].sum())
    T = ref['tokens']
    clip = C.HP['value_clip']
    zero = ((T['ret'] < T['v']) & (T['v'] < T['v_old'] - clip)) | ((T['v_old'] + clip < T['v']) & (T['v'] < T['ret']))
    critic = torch.where(zero, 0., torch.minimum(T['ceu'], T['cec']))
    assert abs(float(critic.mean()) - float(ref['critic'])) < 1e-12


def test_gae_cases_cover_the_edges():
    cs = C.GAE_CASES
    assert {c.B for c in cs} >= {2, 64, 65, 127, 200} and {c.n for c in cs} >= {1, 2, 37}
    assert any(c.n == c.T for c in cs) and any(c.n < c.T for c in cs)
    for c in cs:
        ins = C.gae_inputs(c)
        b = ins['bounds'][:, :c.n]
        assert b[0, c.n - 1] == 1 and b[1, 0] == 1 and int(b[3].sum()) == 0
        if c.n >= 5:
            assert bool(b[2, 2:5].all())
        if c.boot:
            nan = torch.isnan(ins['boot'])
            assert bool(nan.any()) and bool((~nan).any())
            lens = ins['lens']
            assert bool(((lens == c.n) & ~nan).any()), 'no bootstrap value lands on the padding slot'
            assert c.n == 1 or bool(((lens < c.n) & ~nan).any())
        v, r = C.gae_reference(c)
        assert v.shape == r.shape == (c.E, c.n) and bool(torch.isfinite(r).all())


def test_gae_f32_restatement_is_the_reference_in_float32():
    c = C.GAE_CASES[3]
    v, r = C.gae_reference(c)
    r32 = C.gae_f32_restatement(c, v.float())
    assert r32.dtype == torch.float32
    torch.testing.assert_close(r32.double(), r, rtol=1e-5, atol=1e-5)


def test_gather_cases_cover_the_edges():
    cs = C.GATHER_CASES
    assert {c.S for c in cs} >= {1, 8, 63} and {c.B for c in cs} >= {2, 100}
    assert {c.A for c in cs if c.cont} >= {1, 32} and {c.cont for c in cs} == {True, False}
    assert any(c.n < c.Tmax for c in cs) and any(c.n == c.Tmax for c in cs)
    for c in cs:
        ins = C.gather_inputs(c)
        idx = ins['idx'].tolist()
        assert 0 in idx and c.N - 1 in idx and len(set(idx)) < len(idx) and idx != sorted(idx)
        assert float(ins['rs_var'][0]) == 0. and 0 < float(ins['rs_var'][c.S]) < 1e-10
        ref = C.gather_reference(c)
        assert ref['swr'].shape == (c.b, c.n, c.S + 1) and bool(torch.isfinite(ref['swr']).all())
        fill = 0. if c.cont else -1
        assert bool((ref['prev_action'][:, 0] == fill).all())


def test_rsnorm_update_reference_matches_train_call():
    g = torch.Generator().manual_seed(2)
    x = torch.randn(5, 7, 9, generator=g, dtype=torch.float64)
    st = R.RSNormState(9, step=3, mean=torch.randn(9, generator=g, dtype=torch.float64),
                       var=torch.rand(9, generator=g, dtype=torch.float64))
    mean, var = C.rsnorm_update_reference(st.mean, st.var, x.reshape(-1, 9).mean(0), 3)
    st.train_call(x)
    assert torch.equal(mean, st.mean) and torch.equal(var, st.var)
    _, var1 = C.rsnorm_update_reference(st.mean, st.var, st.mean + 1., 1)
    assert float(var1.abs().max()) == 0.        # t = 1: the variance becomes 0


def test_adopt_cases_cover_layout_and_options():
    assert C.ADOPT_SIZES == [1, 255, 257, 1023, 1025, 2047, 2049, 5000]
    for step in range(4):
        gr = C.adopt_grads(step)
        assert float(gr[C.ADOPT_ZERO_SEG].abs().max()) == 0.
        assert all(int((g == 0).sum()) >= 1 for g in gr[3:])
        norm = float(torch.cat(gr).norm())
        assert (norm > 0.5) == (step == 2), norm    # clip coefficient below 1 on step 2 only
    ids = [r[0] for r in C.ADOPT_ROWS]
    assert ids == ['defaults', 'no_cautious_count', 'zero_cautious_factor', 'weight_decay', 'no_regen', 'decayed_lr',
                   'no_clip']
    # the reference optimiser's zero-factor mask mean of the all-zero segment clamps at 1e-5
    p = torch.nn.Parameter(torch.ones(4))
    opt = tp.AdoptAtan2([p], lr=C.ADOPT_LR, cautious_factor=0.)
    for _ in range(2):
        p.grad = torch.zeros(4)
        opt.step()
    assert bool(torch.isfinite(p).all())
