"""Kernel-level fp64 tests of the decode step's kernels (csrc/decode.hip through xtrl_decode_op and the one-launch
entries beside it), over the tables of tests/decode_kernel_cases.py: one launch per case through the launcher the
step itself calls, on a descriptor over buffers the case owns.  Every output is NaN (or its seeded old value) before
the call; owned elements must come back finite and inside their bound (module docstring of decode_kernel_cases),
everything else with its bits unchanged.  Each test prints its worst error as a fraction of the bound (pytest -s)."""
import ctypes as C

import pytest
import torch

import decode_kernel_cases as DC

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def build(spec, dev):
    """The descriptors of a case over its uploaded buffers: (DecodeDesc, FractalDesc or None, keep-alive list)."""
    from xtrl_amd import _lib as L

    def fill(obj, fields):
        kinds = dict(obj._fields_)
        for k, v in fields.items():
            if k in ('level',):
                continue
            if isinstance(v, str):
                setattr(obj, k, dev[v].data_ptr())
            elif v is None:
                setattr(obj, k, None)
            else:
                setattr(obj, k, kinds[k](v).value)
        return obj
    layers = (L.DecodeLayer * len(spec.layers))()
    for i, ly in enumerate(spec.layers):
        fill(layers[i], ly)
    desc = spec.desc
    D = fill(L.DecodeDesc(), {k: v for k, v in desc.items() if k != 'layers_dev'})
    D.layers = layers
    keep = [layers]
    if desc.get('layers_dev'):
        raw = torch.frombuffer(bytearray(bytes(layers)), dtype=torch.uint8).to(DEV)
        keep.append(raw)
        D.layers_dev = C.cast(raw.data_ptr(), C.POINTER(L.DecodeLayer))
    F = None
    if spec.fractal:
        lv = (L.FractalLevel * len(spec.fractal['level']))()
        for i, q in enumerate(spec.fractal['level']):
            fill(lv[i], q)
        F = fill(L.FractalDesc(), spec.fractal)
        F.level = lv
        keep.append(lv)
    return D, F, keep


def pack_weights(spec, dev):
    """The weight images a case asks for, built by the library's own packers (as the rollout engine builds them)."""
    from xtrl_amd import _lib as L
    lib, s = L.lib(), L.stream()
    for kind, src, dst, N, K in spec.info.get('pack', ()):
        if dst in dev:
            continue
        w = dev[src]
        if kind == 'dgemm':
            dev[dst] = torch.zeros(lib.xtrl_dgemm_packed_floats(N, K), device=DEV)
            rc = lib.xtrl_dgemm_pack(w.data_ptr(), w.shape[1], N, K, dev[dst].data_ptr(), s)
        elif kind == 'x6':
            dev[dst] = torch.zeros(lib.xtrl_dgemm_packed_x6_elems(N, K), dtype=torch.int16, device=DEV)
            rc = lib.xtrl_dgemm_pack_x6(w.data_ptr(), w.shape[1], N, K, dev[dst].data_ptr(), s)
        else:
            dev[dst] = torch.zeros(lib.xtrl_dgemm_packed_f8_floats(N, K), device=DEV)
            rc = lib.xtrl_dgemm_pack_f8(w.data_ptr(), w.shape[1], N, K, dev[dst].data_ptr(), s)
        assert rc == 0, L.load().xtrl_last_error().decode()
    if 'slots' in spec.info:
        dev['live_slots'] = spec.info['slots'].to(torch.int32).to(DEV)


def launch(spec, dev=None):
    """Upload the case's buffers (or use `dev`), make the one call, return (rc, the output buffers on the CPU)."""
    from xtrl_amd import _lib as L
    dev = dev if dev is not None else {k: v.to(DEV) for k, v in spec.bufs.items()}
    pack_weights(spec, dev)
    D, F, keep = build(spec, dev)
    lib, s = L.lib(), L.stream()
    if spec.op in DC.OP:
        a = L.DecodeOpArgs()
        for i, x in enumerate(spec.in_):
            a.in_[i] = None if x is None else dev[x].data_ptr()
        for i, x in enumerate(spec.out):
            a.out[i] = None if x is None else dev[x].data_ptr()
        for name in ('ld', 'n'):
            for i, v in enumerate(getattr(spec, name)):
                getattr(a, name)[i] = v
        rc = lib.xtrl_decode_op(C.byref(D), C.byref(F) if F is not None else None, C.byref(a), DC.OP[spec.op], spec.layer,
                                spec.t, s)
    elif spec.op == 'ENV_FEEDBACK':
        p = lambda k: None if spec.call.get(k) is None else dev[spec.call[k]].data_ptr()   # noqa: E731
        rc = lib.xtrl_rollout_env_feedback(C.byref(D), spec.t, p('next_state'), p('reward'), p('terminated'), p('truncated'),
                                           spec.call['t_limit'], spec.call['bootstrap'], s)
    elif spec.op == 'ROLLOUT_BEGIN':
        rc = lib.xtrl_rollout_begin(C.byref(D), s)
    elif spec.op == 'STEP_ROWS':
        rc = lib.xtrl_decode_step_rows(C.byref(D), spec.t, spec.call['max_rows'], s)
    elif spec.op == 'SIM_RESET':
        rc = lib.xtrl_sim_reset(dev['state'].data_ptr(), spec.desc['E'], spec.desc['S'], spec.call['seed'], spec.call['update'],
                                dev['episode_of_slot'].data_ptr(), s)
    else:
        raise AssertionError(spec.op)
    torch.cuda.synchronize()
    del keep
    return rc, {k: dev[k].cpu() for k in spec.outs}


def run(spec):
    from xtrl_amd import _lib as L
    rc, after = launch(spec)
    assert rc == 0, L.load().xtrl_last_error().decode()
    worst = DC.verify(spec, after, spec.expect(torch.float64))
    print(' worst / bound: ' + (', '.join(f'{k} {v:.3f}' for k, v in worst.items()) or 'exact'), end='')
    return after


@pytest.mark.parametrize('c', DC.EMBED_CASES, ids=lambda c: c.id)
def test_embed(c):
    run(DC.embed_spec(c))


@pytest.mark.parametrize('c', DC.ATTN_CASES, ids=lambda c: c.id)
def test_attn_decode(c):
    run(DC.attn_spec(c))


@pytest.mark.parametrize('spec', DC.small_specs(), ids=lambda s: s.id)
def test_small_row_kernels(spec):
    run(spec)


@pytest.mark.parametrize('a', DC.ENV_CASES, ids=str)
def test_env_feedback(a):
    run(DC.env_feedback_spec(*a))


@pytest.mark.parametrize('a', DC.BEGIN_CASES, ids=str)
def test_rollout_begin(a):
    run(DC.rollout_begin_spec(*a))


@pytest.mark.parametrize('a', DC.SIM_RESET_CASES, ids=str)
def test_sim_reset(a):
    run(DC.sim_reset_spec(*a))


@pytest.mark.parametrize('c', DC.PROJ_CASES, ids=lambda c: c.id)
def test_projection(c):
    run(DC.proj_spec(c))


@pytest.mark.parametrize('c', DC.MLP_CASES, ids=lambda c: c.id)
def test_mlp(c):
    """One launch inside the fp64 bound, the arrival counters left zero, and a second launch on the same device buffers
    (the partials and counters as the first left them; the rows a call updates in place restored) bit-identical to it."""
    spec = DC.mlp_spec(c)
    first = run(spec)
    dev = {k: v.to(DEV) for k, v in spec.bufs.items()}
    assert launch(spec, dev)[0] == 0
    for k, v in spec.bufs.items():     # the same mlp_part / mlp_cnt as the first launch left them; in-place rows restored
        if k not in ('mlp_part', 'mlp_cnt') and c.kind != 'last':
            dev[k].copy_(v)
    rc, second = launch(spec, dev)
    assert rc == 0
    for k in spec.outs:
        if k != 'mlp_part':
            same = DC.bits(first[k]) == DC.bits(second[k]) if first[k].dtype == torch.float32 else first[k] == second[k]
            assert bool(same.all()), k


@pytest.mark.parametrize('c', [c for c in DC.MLP_CASES if c.fi], ids=lambda c: c.id)
def test_mlp_weight_images_agree(c):
    """The fp32 fragment images and the split images give bit-identical outputs (the header's claim)."""
    from dataclasses import replace
    a, b = launch(DC.mlp_spec(c)), launch(DC.mlp_spec(replace(c, fi=0)))
    assert a[0] == 0 and b[0] == 0
    for k in a[1]:
        if k != 'mlp_part':
            same = DC.bits(a[1][k]) == DC.bits(b[1][k]) if a[1][k].dtype == torch.float32 else a[1][k] == b[1][k]
            assert bool(same.all()), k


@pytest.mark.parametrize('c', DC.HEADS_CASES, ids=lambda c: c.id)
def test_heads_sampling(c):
    """The hidden layer, the logits, the critic scatter, the sampled action with its log-probability and the Sim step.
    The action is exact unless the Philox uniform lies within the cdf's own bound of a cdf step (then the kernel's
    action, if it is one of the neighbours, is the one the rest of the row is held to)."""
    from xtrl_amd import _lib as L
    spec = DC.heads_spec(c)
    rc, after = launch(spec)
    assert rc == 0, L.load().xtrl_last_error().decode()
    slots = spec.bufs['live_rows'][spec.t & 1, :c.nl].long()
    taken = after['traj_actions'][slots, spec.t].tolist()
    worst = DC.verify(spec, after, spec.expect(torch.float64, taken=taken))
    assert spec.info['ties'] <= DC.TIE_CAP * c.nl
    print(' worst / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()) + f", ties {spec.info['ties']}", end='')


@pytest.mark.parametrize('c', DC.CONT_CASES, ids=lambda c: c.id)
def test_heads_sampling_continuous(c):
    run(DC.cont_spec(c))


@pytest.mark.parametrize('c', DC.ROW_CASES, ids=lambda c: c.id)
def test_row_resident_step(c):
    """One launch of xtrl_decode_step_rows on a pre-filled state against the composition of the per-kernel references:
    the written K / V / v1 rows, logits and critic logits, logp, the action (tie rule as test_heads_sampling) and the Sim
    bookkeeping; max_rows below the live rows, so workgroups loop over rows."""
    from xtrl_amd import _lib as L
    spec = DC.row_spec(c)
    rc, after = launch(spec)
    assert rc == 0, L.load().xtrl_last_error().decode()
    slots = after['live_rows'][spec.t & 1, :c.nl].long().clamp(0, c.E - 1)
    taken = after['traj_actions'][slots, spec.t].tolist()
    worst = DC.verify(spec, after, spec.expect(torch.float64, taken=taken))
    assert spec.info['ties'] <= DC.TIE_CAP * c.nl
    print(' worst / bound: ' + ', '.join(f'{k} {v:.3f}' for k, v in worst.items()) + f", ties {spec.info['ties']}", end='')
