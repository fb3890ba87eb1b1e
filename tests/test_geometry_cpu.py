"""CPU companion of test_geometry_gpu.py: for every geometry of geometry_cases.py the oracle alone (on the
weights the device Learner starts from: the model is initialised on the host from the case's seed) must roll
out episodes that make the GPU comparison mean something — at least two distinct episode lengths, one
episode ending before T and one reaching it, and sampled actions that reach the action-embedding rows the
kernels treat differently (discrete A in 5..8: an action >= 4; A >= 9: a sampled and a previous action
>= 8, past the register-held rows of the decode embedding and into k_embed_grad_part<EMB_MAXA>'s upper
rows; A = 32: at least 16 distinct actions).  These are conditions on the inputs: a case that misses one
gets another seed in geometry_cases.py."""
import pytest

import geometry_cases as GC
import test_gpu_parity as G


def _oracle_rollout(c, **extra):
    _, _, oracle = G.make_learner(**c.learner_kwargs(), device='cpu', **extra)
    episodes, _ = oracle.rollout(0)
    return episodes


@pytest.mark.parametrize('c', GC.CASES + GC.EXTRA, ids=GC.case_id)
def test_oracle_rollout_meets_the_input_conditions(c):
    episodes = _oracle_rollout(c)
    assert len(episodes) == c.episodes * (3 if c.evo else 1)
    print(c.id, GC.action_conditions(c, episodes))


def test_fractal_oracle_rollout_meets_the_input_conditions():
    c = GC.FRACTAL
    print(c.id, GC.action_conditions(c, _oracle_rollout(c, fractal_levels=c.depth)))


def test_case_table_holds_the_geometries_it_is_there_for():
    cs = GC.BY_ID
    assert len(GC.CASES) == 10 and len(cs) == 10 + len(GC.EXTRA)
    assert {(c.H, c.dh) for c in GC.CASES} >= {(2, 32), (1, 64), (3, 16), (8, 16), (16, 16), (4, 32), (8, 64), (2, 64)}
    assert all(16 <= c.T <= 24 and 8 <= c.episodes <= 12 and c.episodes % c.batch == 0 for c in GC.CASES)
    # decode embedding: NC = 3 (d = 192), NC = 8 with d not a multiple of 512 (d = 320), d = 512
    assert {cs['h3x16_d192'].d, cs['h4x32_d320'].d, cs['h8x64_d512'].d} == {192, 320, 512}
    # the learn backward without the fused LayerNorms (d > 256), more than one block deep
    assert (cs['h4x32_d320_l2'].d, cs['h4x32_d320_l2'].depth) == (320, 2)
    # the learn step's limits (train.hip EMB_MAXS / EMB_MAXA) and the register-held action rows (EMB_AREG = 8)
    assert (cs['h8x16_max'].S, cs['h8x16_max'].A) == (32, 32) and cs['h3x16_d192'].A == 9 and cs['h1x64'].S == 1
    assert cs['h16x16'].H > 8                                   # the unfused out-projection at dh = 16
    assert all(('rows' in c.paths) == (c.d <= 128) for c in GC.CASES)   # (RolloutEngine._rows_max: c.dim > 128)
    assert {(c.A, c.squash) for c in GC.CASES if c.cont} == {(1, True), (6, False)}
    assert {GC.BY_ID[i].dh for i in GC.LEARN_DROPOUT} == {16, 32, 64}
    # k_heads_sample<2>'s 32 actor columns filled exactly; 2 A = 64 > 32 actor outputs at 4 d >= 768: k_sample
    assert (cs['a32_d256'].A, cs['a32_d256'].cont) == (32, False) and 4 * cs['a32_d256'].d >= 768
    assert cs['cont_a32_d192'].cont and 2 * cs['cont_a32_d192'].A == 64 and 4 * cs['cont_a32_d192'].d >= 768
    for ids in (GC.LEARN_DROPOUT, GC.PACKED, GC.DEPLOY, [i for i, _ in GC.FUSED_VS_AUTOGRAD]):
        assert set(ids) <= set(cs)
