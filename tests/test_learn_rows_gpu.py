"""Kernel-level fp64 tests of the learn step's row kernels (csrc/train.hip through xtrl_learn_rows), over the tables
of tests/learn_row_cases.py: one launch per case through the launcher the learn step calls.  Every output is NaN
(or its seeded old value) before the call; owned elements must come back finite and inside their bound (module
docstring of learn_row_cases), everything else with its bits unchanged.  Each test prints its worst error as a
fraction of the bound (pytest -s)."""
import ctypes as C

import pytest
import torch

import learn_row_cases as LC

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def launch(spec):
    """Upload the case's buffers, make the one call, return (rc, the output buffers back on the CPU)."""
    from xtrl_amd import _lib as L
    dev = {k: v.to(DEV) for k, v in spec.bufs.items()}

    def addr(x):
        if x is None:
            return None
        name, off = x if isinstance(x, tuple) else (x, 0)
        assert dev[name].element_size() == 4
        return dev[name].data_ptr() + 4 * off
    d = L.RowsDesc()
    for i, x in enumerate(spec.in_):
        d.in_[i] = addr(x)
    for i, x in enumerate(spec.out):
        d.out[i] = addr(x)
    for name in ('ld', 'n', 'f'):
        for i, v in enumerate(getattr(spec, name)):
            getattr(d, name)[i] = v
    if spec.part:
        d.part, d.part_floats = addr(spec.part), spec.part_floats
    jobs = (L.ColsumJob * max(1, len(spec.jobs)))()
    for j, (part, dst, chunks, cols) in enumerate(spec.jobs):
        jobs[j].part, jobs[j].dst, jobs[j].chunks, jobs[j].cols = addr(part), addr(dst), chunks, cols
    if spec.jobs:
        d.jobs, d.n_jobs = jobs, len(spec.jobs)
    rc = L.lib().xtrl_learn_rows(C.byref(d), LC.OP[spec.op], L.stream())
    torch.cuda.synchronize()
    return rc, {k: dev[k].cpu() for k in spec.outs}


def run(spec):
    from xtrl_amd import _lib as L
    rc, after = launch(spec)
    assert rc == 0, L.load().xtrl_last_error().decode()
    worst = LC.verify(spec, after, spec.expect(torch.float64))
    print(' worst / bound: ' + (', '.join(f'{k} {v:.3f}' for k, v in worst.items()) or 'exact'), end='')
    return after


@pytest.mark.parametrize('c', LC.EMBED_CASES, ids=lambda c: c.id)
def test_embed(c):
    run(LC.embed_spec(c))


@pytest.mark.parametrize('a', LC.LATENT_EMBED_CASES, ids=str)
def test_latent_embed(a):
    run(LC.latent_embed_spec(*a))


@pytest.mark.parametrize('a', LC.LN_FWD_CASES, ids=str)
def test_ln_fwd(a):
    run(LC.ln_fwd_spec(*a))


@pytest.mark.parametrize('a', LC.LN_BWD_CASES, ids=str)
def test_ln_bwd(a):
    run(LC.ln_bwd_spec(*a))


@pytest.mark.parametrize('c', LC.PREP_CASES, ids=lambda c: c.id)
def test_qkv_prep(c):
    run(LC.prep_spec(c))


@pytest.mark.parametrize('c', LC.PREP_BWD_CASES, ids=lambda c: c.id)
def test_qkv_prep_bwd(c):
    run(LC.prep_bwd_spec(c))


@pytest.mark.parametrize('a', LC.COLSUM_CASES, ids=str)
def test_colsum(a):
    run(LC.colsum_spec(*a))


@pytest.mark.parametrize('a', LC.QUEUE_CASES, ids=lambda a: a[0])
def test_colsum_queue(a):
    """Each queued sum inside the fp64 bound, and bit-identical to k_colsum_final on the same partials."""
    spec = LC.queue_spec(*a)
    after = run(spec)
    o = 0
    for j, (chunks, cols) in enumerate(spec.info['jobs']):
        one = LC.colsum_final_spec(spec.bufs[f'p{j}'], spec.info['olds'][j])
        rc, alone = launch(one)
        assert rc == 0
        assert bool((LC.bits(alone['dst'][:, :cols]) == LC.bits(after['dst'][:, o:o + cols])).all()), f'job {j}'
        assert bool(torch.isnan(alone['dst'][:, cols:]).all())
        o += cols


@pytest.mark.parametrize('a', LC.EMBED_GRAD_CASES, ids=str)
def test_embed_grad(a):
    run(LC.embed_grad_spec(*a))


@pytest.mark.parametrize('a', LC.LATENT_GRAD_CASES, ids=str)
def test_latent_grad(a):
    run(LC.latent_grad_spec(*a))


@pytest.mark.parametrize('a', LC.VALID_CASES, ids=str)
def test_valid_rows(a):
    run(LC.valid_rows_spec(*a))


@pytest.mark.parametrize('kind', ['gather', 'scatter'])
@pytest.mark.parametrize('a', LC.MOVE_CASES, ids=str)
def test_gather_scatter_rows(a, kind):
    run(LC.move_spec(kind, *a))


@pytest.mark.parametrize('a', LC.CAUSAL_CASES, ids=str)
def test_causal_mean(a):
    run(LC.causal_mean_spec(*a))


def test_action_rows():
    run(LC.action_rows_spec())


@pytest.mark.parametrize('a', LC.AXPB_CASES, ids=str)
def test_rows_axpb(a):
    run(LC.rows_axpb_spec(*a))


def test_rows_bcast_ep():
    run(LC.rows_bcast_spec())
