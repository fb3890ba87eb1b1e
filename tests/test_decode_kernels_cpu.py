"""CPU-only checks behind tests/test_decode_kernels_gpu.py (no GPU): the tables of tests/decode_kernel_cases.py are
settled here.  Every case's fp32 restatement lies inside a quarter of its bound against the fp64 reference and each
composite constant is four times the restatement's worst error in the family's units, rounded up; the live rows of
every case are a strict non-identity subset of the slots; a host restatement of the dispatch names the kernel form
each case expects, and together the cases name every instantiation of the families they cover; the C ABI of the entry
(XtrlDecodeOpArgs / xtrl_decode_op, ABI 32) with the refusals that return before any launch."""
import ctypes
import math
import re
from collections import defaultdict
from pathlib import Path

import pytest
import torch

import decode_kernel_cases as DC

REPO = Path(__file__).resolve().parent.parent


def all_specs():
    return ([DC.embed_spec(c) for c in DC.EMBED_CASES] + [DC.attn_spec(c) for c in DC.ATTN_CASES] + DC.small_specs()
            + [DC.env_feedback_spec(*a) for a in DC.ENV_CASES] + [DC.rollout_begin_spec(*a) for a in DC.BEGIN_CASES]
            + [DC.sim_reset_spec(*a) for a in DC.SIM_RESET_CASES] + [DC.proj_spec(c) for c in DC.PROJ_CASES]
            + [DC.mlp_spec(c) for c in DC.MLP_CASES] + [DC.heads_spec(c) for c in DC.HEADS_CASES]
            + [DC.cont_spec(c) for c in DC.CONT_CASES] + [DC.row_spec(c) for c in DC.ROW_CASES])


@pytest.fixture(scope='module')
def specs():
    return all_specs()


def test_fp32_restatement_within_a_quarter_of_each_bound(specs):
    """expect(float32) against expect(float64), region by region: exact regions agree bit for bit, toleranced ones lie
    within a quarter of the bound, and each constant of C_COMP is 4 x the worst error in its units, rounded up."""
    worst = defaultdict(lambda: [0., 0., ''])     # family -> [error / bound, error / unit, case]
    for sp in specs:
        r64 = sp.expect(torch.float64)
        if sp.op in ('HEADS', 'STEP_ROWS') and not sp.desc.get('continuous'):     # at a tie the restatement is held to the reference's action, as the kernel is to its own
            assert sp.info['ties'] <= DC.TIE_CAP * len(sp.info['a_ref']), f"{sp.id}: {sp.info['ties']} ties; move the seed"
            r32 = sp.expect(torch.float32, taken=sp.info['a_ref'])
        else:
            r32 = sp.expect(torch.float32)
        assert len(r64) == len(r32)
        for a, b in zip(r64, r32):
            assert (a.buf, a.r0, a.c0) == (b.buf, b.r0, b.c0)
            if a.ref is None:
                continue
            if a.bound is None:
                x, y = a.ref, b.ref
                same = DC.bits(x) == DC.bits(y) if x.dtype == torch.float32 else x == y
                assert bool(same.all()), f'{sp.id} {a.buf}: the exact region depends on the precision'
                continue
            err = (b.ref.double() - a.ref.double()).abs().reshape(a.bound.shape)
            assert bool(torch.isfinite(a.bound).all()) and bool((a.bound > 0).all() | (err == 0).all()), sp.id
            w = worst[a.fam]
            rb = float((err / a.bound.clamp_min(1e-300)).max())
            if a.unit is not None:
                w[1] = max(w[1], float((err / a.unit.clamp_min(1e-300)).max()))
            if rb >= w[0]:
                w[0], w[2] = rb, sp.id
    print()
    for fam, (rb, ru, case) in sorted(worst.items()):
        print(f'  {fam:12s} restatement / bound {rb:.3f}   error / unit {ru:.3f}   C {DC.C_COMP.get(fam, "-")}   ({case})')
        assert rb <= 0.25 + 1e-9, f'{fam}: the fp32 restatement reaches {rb:.3f} of the bound at {case}'
        if fam in DC.C_COMP:
            assert DC.C_COMP[fam] == max(1., math.ceil(4 * ru)), f'{fam}: C should be {max(1., math.ceil(4 * ru))}'
    assert set(DC.C_COMP) <= set(worst)


def test_live_rows_are_a_strict_non_identity_subset(specs):
    """Row r is never slot r (E > 1), fewer rows than slots, stale entries past the count in range."""
    n = 0
    for sp in specs:
        if sp.op in ('ENV_FEEDBACK', 'ROLLOUT_BEGIN', 'SIM_RESET', 'EMBED', 'COPY_ROWS', 'STEP_ROWS'):
            continue
        E, t = sp.desc['E'], sp.t
        rows, cnt = sp.bufs['live_rows'], int(sp.bufs['live_count'][0, t & 1])
        assert 0 < cnt < E, sp.id
        live = rows[t & 1, :cnt]
        assert bool((live != torch.arange(cnt)).all()) and bool((live[1:] > live[:-1]).all()), sp.id
        assert int(rows.min()) >= 0 and int(rows.max()) < E, sp.id
        n += 1
    assert n > 400
    for c in DC.EMBED_CASES:     # the compaction's own input: slot 0 never live unless it is the only slot
        sp = DC.embed_spec(c)
        al = sp.bufs['alive'][0]
        assert set(al.tolist()) <= {0, 1, 2, 3, 4}
        if c.E > 1:
            assert int(al[0]) not in (1, 2, 3 + (c.t & 1)) and sp.info['n_live'] < c.E
    assert {c.t & 1 for c in DC.EMBED_CASES} == {0, 1}
    assert {int(v) for c in DC.EMBED_CASES[:24] for v in DC.embed_spec(c).bufs['alive'][0].tolist()} == {0, 1, 2, 3, 4}


# every instantiation decode.hip can launch for the families the tables cover ...
EXPECTED_FORMS = (
    {f'k_embed<{nc},true>' for nc in (1, 2, 3, 4, 8)} | {f'k_compact+k_embed<{nc},false>' for nc in (1, 2, 3, 4, 8)}
    | {f'k_attn_decode<{dh},{fj},{fl}>' for dh, fjs in ((16, (0, 1, 2)), (32, (0,)), (64, (0,))) for fj in fjs
       for fl in DC.FORM_FLAGS.values()}
    | {f'k_mlp<{nt},{fi}>' for nt in (1, 2, 3, 4) for fi in ('true', 'false')}
    | {'k_heads_mlp<2>', 'k_heads_mlp<3>', 'k_heads_mlp<6>', 'k_heads_sample<1>', 'k_heads_sample<2>', 'k_sample'}
    | {f'k_decode_row<{dh},{kp},{fl}>' for dh, kp in ((16, 2), (64, 1)) for fl in DC.FORM_FLAGS.values()}
    | {'k_glu_rows', 'k_fr_ln12', 'k_fr_ln3_tail', 'k_copy_rows', 'k_env_feedback', 'k_rollout_begin', 'k_sim_reset'})
# ... nothing else: every __global__ function has a case (the host-gated step runs k_decode_row behind its gate; the
# split-heads form and dh = 32 of the row step stay end to end only)
END_TO_END_ONLY = set()


def test_every_case_names_its_kernel_form_and_every_form_is_named(specs):
    assert all(sp.form for sp in specs)
    named = {f for sp in specs for f in ([sp.form] if sp.form.startswith('k_compact+') else sp.form.split('+'))}
    dgemm = {f for f in named if f.startswith('k_dgemm<')}
    assert named - dgemm == EXPECTED_FORMS, (sorted(EXPECTED_FORMS - named), sorted(named - dgemm - EXPECTED_FORMS))
    # the projection: both K splits, the 32-row panel, ReLU, the prologue with and without a residual
    assert {re.match(r'k_dgemm<(\d),1,(\d)', f).groups() for f in dgemm} == {('1', '1'), ('1', '2'), ('2', '1')}
    assert any('EPI_RELU' in f for f in dgemm) and any(f.endswith('true,true>') for f in dgemm)
    assert {c.ln for c in DC.PROJ_CASES} == {0, 1, 2} and any(c.n_split % 16 for c in DC.PROJ_CASES if c.n_split)
    # mlp_fused and heads_fused, restated: the shapes either side of each rule
    assert DC.mlp_fused(192, 1024, True, True, True, 0, True) and not DC.mlp_fused(260, 1024, True, True, True, 0, True)
    assert not DC.mlp_fused(128, 192, True, True, True, 0, True) and not DC.mlp_fused(128, 256, True, True, True, 1, True)
    assert not DC.mlp_fused(128, 256, True, True, True, 0, DC.attn_fused(9, 16, 128, 8, True))
    assert DC.heads_kernel(DC.HeadsCase(64, 0, 4, 'mlp', fn=1)).endswith('k_heads_sample<1>')      # the final norm: not fused
    assert DC.heads_kernel(DC.HeadsCase(96, 1, 4, 'mlp')).endswith('k_heads_sample<1>')            # in_dim 288: no JH
    assert DC.heads_kernel(DC.HeadsCase(192, 0, 64, 'hs')).endswith('k_sample')                    # n_act > 64 / KS
    # every __global__ function of decode.hip is covered by a named form or listed as end to end only
    src = (REPO / 'x-transformers-rl_amd' / 'csrc' / 'decode.hip').read_text()
    kernels = set(re.findall(r'__global__[^;{]*?void (k_\w+)\(', src))
    assert len(kernels) == 15
    covered = {re.match(r'(?:k_compact\+)?(k_\w+)', f).group(1) for f in EXPECTED_FORMS} | {'k_compact'}
    assert kernels == covered | END_TO_END_ONLY, (kernels - covered - END_TO_END_ONLY, (covered | END_TO_END_ONLY) - kernels)


def test_tables_reach_the_edges_the_issue_names():
    for (H, Hkv, dh) in DC.HEADS:
        CK = DC.ck_of(dh)
        cs = [c for c in DC.ATTN_CASES if (c.H, c.Hkv, c.dh) == (H, Hkv, dh)]
        assert {0, 1, CK - 1, CK, CK + 1, 2 * CK + 1} <= {c.t for c in cs}
        assert {(c.t, c.W) for c in cs} >= {(t, W) for t in (CK - 1, CK, CK + 1, 2 * CK + 1) for W in (0, 1, 63, CK, CK + 2)}
    fused = [c for c in DC.ATTN_CASES if c.tail != 'att']
    assert any(c.tail == 'attw' and c.H > 8 for c in fused)
    assert {c.d for c in fused} == {36, 256, 260, 512} and {c.tail for c in fused} == {'attw', 'x', 'xn', 'post0', 'postd'}
    assert {(c.M, c.zkv) for c in DC.ATTN_CASES} >= {(0, 0), (0, 1), (1, 0), (1, 1), (16, 0), (16, 1)}
    assert {c.alibi for c in DC.ATTN_CASES} == {0, 1, 2} and {c.regime for c in DC.ATTN_CASES} == {'o1', 'spread', 'sink'}
    assert any(c.cap > 0 and not c.alibi for c in DC.ATTN_CASES) and any(c.cap > 0 and c.alibi for c in DC.ATTN_CASES)
    assert all(DC.ATTN_LIVE * c.H % 4 for c in DC.ATTN_CASES if c.H in (3, 5, 9, 1))
    assert {c.E for c in DC.EMBED_CASES} >= {1, 15, 16, 17, 1025, 8192, 8200}
    assert {2 * c.d * c.S > DC.EMB_LDS_FLOATS for c in DC.EMBED_CASES} == {True, False}
    assert {c.A > DC.EMB_AREG for c in DC.EMBED_CASES if not c.cont} == {True, False}
    assert {(c.d, c.ff) for c in DC.MLP_CASES} == {(d, ff) for d in (64, 128, 192, 256) for ff in (128, 256, 1024)}
    assert {c.nl for c in DC.MLP_CASES} == {1, 16, 17, 33} and {c.kind for c in DC.MLP_CASES} == {'inner', 'last', 'fr0', 'fr1'}
    assert {(c.kind, c.t) for c in DC.MLP_CASES} >= {('fr0', 0), ('fr0', 3), ('fr1', 0), ('fr1', 3)}


# ----------------------------------------------------------------------------------------------
# the C ABI of the entry
# ----------------------------------------------------------------------------------------------

def test_abi_32_and_the_op_list():
    from xtrl_amd import _lib
    text = (REPO / 'include' / 'xtrl_hip.h').read_text()
    abi = int(re.search(r'#define XTRL_ABI_VERSION (\d+)', text).group(1))
    assert abi == _lib.ABI_VERSION >= 32
    lib = _lib.load()
    assert lib.xtrl_abi_version() == abi and hasattr(lib, 'xtrl_decode_op')
    assert lib.xtrl_struct_size(b'XtrlDecodeOpArgs') == ctypes.sizeof(_lib.DecodeOpArgs)
    ops = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define XTRL_DECODE_(\w+) (\d+)', text)}
    assert ops == DC.OP == _lib.DECODE_OP
    for name in DC.OPS:     # every op is documented beside the defines, as XTRL_ROWS_* are
        assert re.search(rf'^ \*   {name}\s', text, re.M), name
    assert 'xtrl_decode_op' in (REPO / 'INTEGRATION.md').read_text()


def test_argument_errors_return_before_any_launch():
    """Refusals of xtrl_decode_op: XTRL_E_ARG with a message, no launch (so they run without a GPU)."""
    from xtrl_amd import _lib as L
    lib = L.load()
    layers = (L.DecodeLayer * 2)()
    dummy = ctypes.create_string_buffer(64)
    p = ctypes.addressof(dummy)
    D = L.DecodeDesc()
    D.E, D.S, D.A, D.B, D.d, D.L, D.H, D.dh, D.Tmax, D.ff, D.in_dim, D.n_qkv = 4, 4, 4, 4, 64, 2, 4, 16, 8, 128, 128, 192
    D.layers, D.live_rows, D.live_count = layers, p, p
    a = L.DecodeOpArgs()

    def call(op, layer=0, t=0, desc=D, F=None):
        rc = lib.xtrl_decode_op(ctypes.byref(desc) if desc is not None else None, F, ctypes.byref(a),
                                DC.OP[op] if isinstance(op, str) else op, layer, t, None)
        return rc, lib.xtrl_last_error().decode()
    assert call('EMBED', desc=None)[0] == 1
    rc, msg = call('EMBED', t=8)
    assert rc == 1 and 'outside' in msg
    rc, msg = call('ATTN', layer=2)
    assert rc == 1 and 'layer' in msg
    rc, msg = call(99)
    assert rc == 1 and 'unknown op' in msg
    a.n[0] = 1
    assert call('EMBED')[0] == 1          # the pre-norm without xn / gain
    a.n[0] = 0
    assert call('ATTN')[0] == 1           # no q|k|v, no caches
    rc, msg = call('MLP')
    assert rc == 1 and 'one-launch' in msg
    rc, msg = call('GLU')
    assert rc == 1 and 'ff_glu' in msg
    for op in ('FR_LN12', 'FR_LN3_TAIL', 'COPY_ROWS'):
        rc, msg = call(op)
        assert rc == 1 and 'fractal' in msg, op
    assert call('PROJ')[0] == 1           # null operands
    assert call('HEADS')[0] == 1          # no head weights / input rows
    F = L.FractalDesc()                   # a fractal descriptor whose levels do not match
    F.levels = 3
    rc, msg = call('COPY_ROWS', F=ctypes.byref(F))
    assert rc == 1 and 'levels' in msg
    D2 = L.DecodeDesc.from_buffer_copy(D)
    D2.dh = 24
    assert call('EMBED', desc=D2)[0] == 1
