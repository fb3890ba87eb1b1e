"""Model geometries away from the 4 x 16 heads / 8 states / 4 actions every other integrated test builds:
one named tuple per geometry, shared by test_geometry_cpu.py (which settles each case's inputs from the
oracle alone: episode lengths and sampled actions) and test_geometry_gpu.py (which runs the device
rollout, learn step, packed learn step and deploy forward against the oracle).

``paths``: the decode paths the rollout is compared on — 'rows' (the row-resident step,
RolloutEngine.rows_max > 0) and / or 'multi' (the multi-kernel step, XTRL_DECODE_ROWS=0).  A model wider
than 128 has no row-resident step (RolloutEngine._rows_max: ``c.dim > 128``), so it is multi only.

seed and hazard are chosen so that the oracle's rollout meets test_geometry_cpu's input conditions
(the synthetic Sim's terminations depend on seed, hazard and episode alone; the sampled actions on the
initial weights, which the seed fixes too)."""
from __future__ import annotations

from typing import NamedTuple


class Geometry(NamedTuple):
    id: str
    H: int
    dh: int
    d: int
    S: int
    A: int
    depth: int
    gates: bool
    paths: tuple
    seed: int
    hazard: int
    T: int
    episodes: int
    evo: bool = False
    cont: bool = False
    squash: bool = True
    ff_mult: int = 4
    batch: int = 4

    def learner_kwargs(self):
        """The keywords of test_gpu_parity.make_learner for this geometry."""
        return dict(S=self.S, A=self.A, depth=self.depth, gates=self.gates, evo=self.evo, cont=self.cont,
                    squash=self.squash, T=self.T, episodes=self.episodes, batch=self.batch, seed=self.seed,
                    hazard=self.hazard, dim=self.d, ff_mult=self.ff_mult, heads=self.H, dim_head=self.dh)

    def geom(self):
        """The geometry alone (make_learner keywords the fused-vs-autograd and packed helpers pass through)."""
        return dict(S=self.S, A=self.A, heads=self.H, dim_head=self.dh, ff_mult=self.ff_mult, squash=self.squash)


ROWS_MULTI, MULTI = ('rows', 'multi'), ('multi',)

CASES = [
    #        id            H   dh   d    S   A  depth gates paths       seed hz  T  episodes
    Geometry('h2x32', 2, 32, 64, 3, 2, 2, True, ROWS_MULTI, 3, 4, 20, 8),
    Geometry('h1x64', 1, 64, 48, 1, 5, 2, True, ROWS_MULTI, 3, 4, 20, 8, evo=True),
    Geometry('h3x16_d192', 3, 16, 192, 13, 9, 2, False, MULTI, 3, 4, 20, 8),
    Geometry('h8x16_max', 8, 16, 128, 32, 32, 1, True, ROWS_MULTI, 3, 4, 24, 12),
    Geometry('h16x16', 16, 16, 64, 8, 4, 2, True, ROWS_MULTI, 3, 4, 20, 8),
    Geometry('h4x32_d320', 4, 32, 320, 8, 6, 1, False, MULTI, 3, 4, 20, 8),
    # two blocks past the fused LayerNorms (d > 256) and without the learned mix: the learn backward's
    # single-plane scratch behind its cross-layer stream waits, every other operand a multiple of 4
    Geometry('h4x32_d320_l2', 4, 32, 320, 8, 6, 2, False, MULTI, 3, 4, 20, 8),
    Geometry('h8x64_d512', 8, 64, 512, 8, 4, 1, False, MULTI, 3, 4, 16, 8, ff_mult=2),
    Geometry('cont_a1', 2, 32, 64, 5, 1, 2, True, ROWS_MULTI, 3, 4, 20, 8, cont=True),
    Geometry('cont_a6', 2, 64, 128, 5, 6, 2, True, ROWS_MULTI, 3, 4, 20, 8, cont=True, squash=False),
]
# two more, past the table above: the decode's last head projection splits K in two for 4 d >= 768 (dg_ks), so its
# fused sampling (k_heads_sample<2>) holds 32 actor columns per workgroup — exactly a discrete A = 32 — and wider
# actor rows (continuous A > 16: 2 A outputs) take the projection GEMM and the stand-alone k_sample launch
EXTRA = [
    Geometry('a32_d256', 4, 16, 256, 8, 32, 1, True, MULTI, 3, 4, 20, 8),
    Geometry('cont_a32_d192', 3, 16, 192, 8, 32, 1, False, MULTI, 3, 4, 20, 8, cont=True),
]
BY_ID = {c.id: c for c in CASES + EXTRA}

# the fractal policy body at H = 2, dh = 32 (no gates: the fractal body has none)
FRACTAL = Geometry('fractal_h2x32', 2, 32, 64, 3, 5, 2, False, MULTI, 3, 4, 20, 8)

# sub-lists of the GPU tests (ids)
LEARN_DROPOUT = ('h2x32', 'h1x64', 'h16x16')                        # one per dim_head: learn parity at p = 0.25
FUSED_VS_AUTOGRAD = (('h2x32', 70), ('h1x64', 70), ('h8x16_max', 70), ('h2x32', 130))   # (id, T) at p = 0.25
PACKED = ('h1x64', 'h3x16_d192')
DEPLOY = ('h8x64_d512', 'h3x16_d192')


def case_id(c):
    return c.id


def action_conditions(c, episodes):
    """The input conditions of one case on the oracle's rollout (a list of episodes as
    OracleLearner.rollout returns them); returns the census it asserted on."""
    lens = [ep['len'] for ep in episodes]
    assert len(set(lens)) >= 2, lens
    assert min(lens) < c.T and max(lens) == c.T, lens
    census = dict(lens=lens)
    if c.cont:
        return census
    acts = [[int(m[1]) for m in ep['mem']] for ep in episodes]
    sampled = [a for ep in acts for a in ep]
    prev = [a for ep in acts for a in ep[:-1]]    # the actions that come back as a step's previous action
    census.update(distinct=len(set(sampled)), max_sampled=max(sampled), max_prev=max(prev, default=-1))
    assert max(sampled) < c.A
    if 5 <= c.A <= 8:
        assert max(sampled) >= 4, census
    if c.A >= 9:
        assert max(sampled) >= 8 and max(prev, default=-1) >= 8, census
    if c.A == 32:
        assert len(set(sampled)) >= 16, census
    return census
