"""What the attention GPU tests share (test_gpu_parity.py, test_attn_window_gpu.py, test_attn_gqa_gpu.py,
test_attn_sink_gpu.py, test_attn_alibi_gpu.py, test_attn_softclamp_gpu.py): the one driver of the learn-step
attention kernels through the C ABI (attn_lib, which reaches every entry-point family: xtrl_attn_fwd / _bwd /
_bwd_part and their _win, _gqa, _sink, _alibi and _softclamp forms), the driver of the token-major forward
xtrl_attn_fwd_tokens (attn_tokens_lib; test_fractal_kernels_gpu.py), the kernel-level problem builder, the fp64
band softmax, the one fp64 autograd wrapper over the option files' dense references (fp64_ref), the bounds
against an fp64 reference (check_ref) and the model-level body "rollout, then n learn minibatches against a patched oracle" (rollout_and_learn).  The Learner
builder and the other model-level bodies are test_gpu_parity's: make_learner, _packed_vs_padded,
_fused_vs_autograd, deploy_parity.

A plain module that defines no tests, so pytest does not rewrite its asserts: each one carries its message."""
import contextlib
import os

import torch

import test_gpu_parity as G

DEV = 'cuda'
NAMES = ('o', 'lse', 'delta', 'dq', 'dk', 'dv')


# ----------------------------------------------------------------------------------------------
# kernel level
# ----------------------------------------------------------------------------------------------


@contextlib.contextmanager
def fused_bwd(on):
    """XTRL_ATTN_FUSED_BWD (read per launch) at 1 / 0 for the launches inside, then as it was."""
    old = os.environ.get('XTRL_ATTN_FUSED_BWD')
    os.environ['XTRL_ATTN_FUSED_BWD'] = '1' if on else '0'
    try:
        yield
    finally:
        if old is None:
            del os.environ['XTRL_ATTN_FUSED_BWD']
        else:
            os.environ['XTRL_ATTN_FUSED_BWD'] = old


def attn_lib(q, k, v, lens, do, scale, p, mode, abi, W=None, mem_k=None, mem_v=None, Z=False, seed=3, offset=1, sub=0,
             slopes=None, c=0.):
    """Forward + backward through the C ABI; every output and workspace holds NaN before the calls, so an
    element no kernel wrote shows.  Returns o, lse, delta, dq, dk, dv (and dmk, dmv at M > 0).  The calls are
    synchronised and the result dict is left in ``attn_lib.last`` also when one of them raises, so a test of a
    refused argument can see that no kernel ran.

    ``abi``: the entry-point family — 'plain' (xtrl_attn_fwd / xtrl_attn_bwd / xtrl_attn_bwd_part; no window),
    'win' (their _win forms; ``W`` None: the plain ones), 'gqa' (_gqa: k, v [b][Hkv][n][dh]; ``W`` None: window
    0, none), 'sink' (_sink: GQA and window as 'gqa', plus mem_k, mem_v [Hkv][M][dh] — None: M = 0, null
    pointers — and the zero key ``Z``), 'alibi' (_alibi: as 'sink', plus ``slopes`` [H] fp32 on the device, or
    None: a NULL pointer) or 'softclamp' (_softclamp: as 'alibi', plus the float ``c`` after the slopes; 0: off).
    ``mode``: 'two' (XTRL_ATTN_FUSED_BWD=0: the dK/dV + dQ kernel pair), 'fused' (=1 without a workspace: one
    launch for n <= 128 at Hkv = H without ALiBi or soft-clamp; the other forms have no fused one and run the
    pair) or 'part' (=1 through xtrl_attn_bwd_part*: the long-episode backward with the dQ partial workspace)."""
    from xtrl_amd import _lib as L
    lib = L.lib()
    b, H, n, dh = q.shape
    Hkv = k.shape[1]
    M = 0 if mem_k is None else mem_k.shape[1]
    FAMILIES = ('plain', 'win', 'gqa', 'sink', 'alibi', 'softclamp')   # each takes what the ones before it take
    assert abi in FAMILIES and mode in ('two', 'fused', 'part'), (abi, mode)
    rank = FAMILIES.index(abi)
    assert abi != 'plain' or W is None, f"abi 'plain' takes no window, W = {W}"
    assert rank >= 2 or Hkv == H, f'abi {abi!r} takes k, v with all H = {H} heads, not {Hkv}'
    assert rank >= 3 or (M == 0 and not Z), f'abi {abi!r} takes no sinks (M = {M}, Z = {Z})'
    assert rank >= 4 or slopes is None, f'abi {abi!r} takes no slopes'
    assert slopes is None or (slopes.shape == (H,) and slopes.dtype == torch.float32 and slopes.is_cuda), slopes
    assert rank >= 5 or c == 0., f'abi {abi!r} takes no soft-clamp value (c = {c})'
    suffix = '' if abi == 'plain' or (abi == 'win' and W is None) else '_' + abi
    nan = lambda *s: torch.full(s, float('nan'), device=DEV)   # noqa: E731
    o, dq, dk, dv = nan(*q.shape), nan(*q.shape), nan(*k.shape), nan(*v.shape)
    lse, delta = nan(b, H, n), nan(b, H, n)
    res = dict(o=o, lse=lse, delta=delta, dq=dq, dk=dk, dv=dv)
    # the arguments after the pointers: b, H, [Hkv,] n, dh, scale, p, seed, offset, sub, [window,] [M, Z,] [slopes,]
    # [c,] stream
    tail = (b, H) + ((Hkv,) if rank >= 2 else ()) + (n, dh, scale, p, seed, offset, sub) \
        + ((int(W or 0),) if suffix else ()) + ((M, int(Z)) if rank >= 3 else ()) \
        + ((L.ptr(slopes),) if rank >= 4 else ()) + ((float(c),) if rank >= 5 else ()) + (L.stream(),)
    fwd_sink = bwd_sink = ()
    if rank >= 3:
        nws = int(lib.xtrl_attn_sink_ws_floats(b, H, M, dh))
        dmk, dmv, ws = (nan(Hkv, M, dh), nan(Hkv, M, dh), nan(nws)) if M else (None, None, None)
        fwd_sink = (L.ptr(mem_k), L.ptr(mem_v))
        bwd_sink = fwd_sink + (L.ptr(dmk), L.ptr(dmv), L.ptr(ws), nws)
        if M:
            res.update(dmk=dmk, dmv=dmv)
    io = tuple(L.ptr(t) for t in (q, k, v, lens, o, lse))
    try:
        L.check(getattr(lib, 'xtrl_attn_fwd' + suffix)(*io, *fwd_sink, *tail), 'attn_fwd' + suffix)
        grads = tuple(L.ptr(t) for t in (do, dq, dk, dv, delta))
        with fused_bwd(mode != 'two'):
            if mode == 'part':
                nf = int(lib.xtrl_attn_bwd_part_floats(b, H, n, dh))
                part = nan(nf)
                L.check(getattr(lib, 'xtrl_attn_bwd_part' + suffix)(*io, *grads, L.ptr(part), nf, *bwd_sink, *tail),
                        'attn_bwd_part' + suffix)
            else:
                L.check(getattr(lib, 'xtrl_attn_bwd' + suffix)(*io, *grads, *bwd_sink, *tail), 'attn_bwd' + suffix)
    finally:
        torch.cuda.synchronize()
        attn_lib.last = res
    return res


def attn_tokens_lib(buf, lens, b, H, n, dh, scale, causal=False, ldo=None, ldk=None):
    """xtrl_attn_fwd_tokens through the C ABI, as xtrl_amd/fractal.py calls it: q, k, v are the column slices
    [0, I), [I, 2 I), [2 I, 3 I) (I = H dh) of ``buf`` [b n][ld] on the device, o is [b n][ldo] (``ldo`` None: I)
    and lse [b][H][n]; both hold NaN before the call, so an element the kernel did not write shows — the padding
    columns of a wide ``ldo`` among them.  ``ldk``: a row stride for k other than q's and v's (the entry point
    refuses it).  The call is synchronised and the result dict is left in ``attn_tokens_lib.last`` also when it
    raises.  Returns dict(o, lse)."""
    from xtrl_amd import _lib as L
    I, ld = H * dh, buf.stride(0)   # noqa: E741
    assert buf.is_cuda and buf.dtype == torch.float32 and buf.shape == (b * n, ld) and ld >= 3 * I, (buf.shape, I)
    assert lens.is_cuda and lens.dtype == torch.int32 and lens.shape == (b,), lens
    ldo = I if ldo is None else ldo
    assert ldo >= I, (ldo, I)
    res = dict(o=torch.full((b * n, ldo), float('nan'), device=DEV), lse=torch.full((b, H, n), float('nan'), device=DEV))
    try:
        L.check(L.lib().xtrl_attn_fwd_tokens(L.ptr(buf), ld, L.ptr(buf[:, I:]), ld if ldk is None else ldk,
                                             L.ptr(buf[:, 2 * I:]), ld, L.ptr(lens), L.ptr(res['o']), ldo,
                                             L.ptr(res['lse']), b, H, n, dh, scale, int(causal), L.stream()),
                'attn_fwd_tokens')
    finally:
        torch.cuda.synchronize()
        attn_tokens_lib.last = res
    return res


def fp64_ref(dense, q, k, v, do, lens, W, extra=(), mem_k=None, mem_v=None, Z=False, keep=None, keep_mem=None):
    """The fp64 reference of attn_lib's results: ``dense`` — one of the dense references attn_sink_ref,
    attn_alibi_ref, attn_softclamp_ref of the CPU test modules, called as dense(q, k, v, lens, scale, W, *extra,
    mem_k, mem_v, Z, keep, keep_mem) — on k, v and the memory rows repeated to the query heads by
    ops.kv_head_index; autograd sums dk / dv / dmem over each kv head's query heads.  ``extra``: what that
    reference takes after W — (slopes,) or (slopes, c); a tensor is widened to fp64 (the fp32 slopes), None stays.
    Without a sink the masked scores take x-transformers' finite fill, so the dead rows of a window (no visible
    key) are uniform over all n positions; their lse is set to the kernels' convention for such rows, 0.
    Returns a dict of CPU tensors: o, lse, dq, dk, dv (and dmk, dmv)."""
    from test_attn_sink_cpu import visible
    from xtrl_amd import ops
    H, Hkv, n, dh = q.shape[1], k.shape[1], q.shape[2], q.shape[3]
    idx = ops.kv_head_index(H, Hkv, device=k.device)
    leaves = [t.double().requires_grad_() for t in (q, k, v)]
    mems = [t.double().requires_grad_() for t in (mem_k, mem_v)] if mem_k is not None else [None, None]
    sinks = mem_k is not None or bool(Z)
    extra = [x.double().to(q.device) if torch.is_tensor(x) else x for x in extra]
    fill = {} if sinks else dict(fill=-torch.finfo(torch.float64).max)   # (with sinks: the references' own -inf)
    o, lse = dense(leaves[0], leaves[1][:, idx], leaves[2][:, idx], lens, dh ** -0.5, W, *extra,
                   None if mems[0] is None else mems[0][idx], None if mems[1] is None else mems[1][idx], bool(Z),
                   keep, keep_mem, **fill)
    (o * do.double()).sum().backward()
    lse = lse.detach().clone()
    if not sinks:
        dead = ~visible(n, lens, W).any(-1)[:, 0]   # [b][n]
        lse.transpose(1, 2)[dead] = 0.
    out = dict(o=o, lse=lse, dq=leaves[0].grad, dk=leaves[1].grad, dv=leaves[2].grad)
    if mems[0] is not None:
        out.update(dmk=mems[0].grad, dmv=mems[1].grad)
    return {name: t.detach().cpu() for name, t in out.items()}


def ragged_lens(g, b, n):
    """lens[0] = n, one episode of a single step, the others random."""
    lens = torch.randint(1, n + 1, (b,), generator=g).to(torch.int32)
    lens[0] = n
    lens[b - 1] = 1
    return lens.to(DEV)


def problem(b, H, n, dh, seed, Hkv=None, M=0):
    """q, k, v, do [b][H][n][dh] and ragged lens from one generator; ``Hkv``: k, v cut to their first Hkv heads;
    ``M`` > 0: mem_k, mem_v [Hkv][M][dh] (from a generator of their own, seed + 1000) follow in the tuple."""
    g = torch.Generator().manual_seed(seed)
    q, k, v, do = (torch.randn(b, H, n, dh, generator=g).to(DEV) for _ in range(4))
    lens = ragged_lens(g, b, n)
    if Hkv is not None:
        k, v = k[:, :Hkv].contiguous(), v[:, :Hkv].contiguous()
    if not M:
        return q, k, v, do, lens
    g = torch.Generator().manual_seed(seed + 1000)
    mem_k, mem_v = (torch.randn(H if Hkv is None else Hkv, M, dh, generator=g).to(DEV) for _ in range(2))
    return q, k, v, do, lens, mem_k, mem_v


def modes_of(n, dh):
    """The backward modes that exist for a shape: the pair always; at dh = 16 the partial-workspace form,
    and for n <= 128 the fused dispatch."""
    return ['two'] + (['part'] if dh == 16 else []) + (['fused'] if dh == 16 and n <= 128 else [])


def band_mask(n, lens, W):
    """[b][1][n][n]: key j visible to query i iff j <= i, i - j <= W and j < len."""
    i = torch.arange(n, device=lens.device)
    dist = i[:, None] - i[None, :]
    return ((dist >= 0) & (dist <= W))[None, None] & (i[None, None, None, :] < lens.long()[:, None, None, None])


def attn_win_ref(q, k, v, lens, scale, W, keep=None):
    """G.attn_ref (dense softmax, masked scores filled with the finite -max as x-transformers does)
    plus the band mask.  A row whose band holds no valid key — a padded row i >= len + W — therefore
    attends all n key positions uniformly and passes no gradient to its scores (without a window no
    row of an episode with a valid key is empty, so attn_ref never meets one)."""
    n = q.shape[2]
    mask = band_mask(n, lens, W)
    s = torch.einsum('bhid,bhjd->bhij', q, k) * scale
    p = s.masked_fill(~mask, -torch.finfo(s.dtype).max).softmax(-1)
    if keep is not None:
        p = p * keep
    return torch.einsum('bhij,bhjd->bhid', p, v)


def check_ref(res, ref):
    """attn_lib's results against an fp64 reference (a dict of CPU tensors): o — and lse and the row sum
    L = exp(lse), where the reference has lse — within 1e-5 + 1e-5, every gradient of the reference (dq, dk, dv;
    dmk, dmv) within 1e-4 + 1e-5."""
    grads = [name for name in ref if name.startswith('d')]
    assert 'o' in ref and set(grads) >= {'dq', 'dk', 'dv'} and set(ref) <= {'o', 'lse', *grads}, sorted(ref)
    G.tol(res['o'], ref['o'], 1e-5, 1e-5)
    if 'lse' in ref:
        G.tol(res['lse'], ref['lse'], 1e-5, 1e-5)
        G.tol(res['lse'].exp(), ref['lse'].exp(), 1e-5, 1e-5)
    for name in grads:
        G.tol(res[name], ref[name], 1e-4, 1e-5)


# ----------------------------------------------------------------------------------------------
# model level
# ----------------------------------------------------------------------------------------------


def rollout_and_learn(monkeypatch, install, T, minibatches, packed=False, checks=None, **learner_kw):
    """Rollout (G.compare_rollout: actions, lengths, rewards bit-exact; log-probs and logits within 1e-4) and
    ``minibatches`` learn minibatches (G._learn_parity: loss within 1e-4 relative, every gradient within 1e-4 of
    the gradient scale) against a patched oracle.  ``install(monkeypatch)`` puts the feature's Attention over the
    frozen oracle's before anything is built; ``learner_kw``: G.make_learner's keywords; ``packed``: the packed
    learn step, with the per-token critic reduction on both sides; ``checks(learner, env, oracle)``: the
    feature's own assertions, made after the rollout.  Returns (learner, lens, seen)."""
    install(monkeypatch)
    if packed:
        learner_kw['agent_extra'] = dict(learner_kw.get('agent_extra') or {}, hl_reduction_mean=False, packed_learn=True)
    learner, env, oracle = G.make_learner(T=T, **learner_kw)
    traj, lens, genes, cum = learner.rollout_device(env, 0, T)
    torch.cuda.synchronize()
    if checks is not None:
        checks(learner, env, oracle)
    episodes, _ = oracle.rollout(0)
    G.compare_rollout(traj, lens, episodes)
    seen = []
    if minibatches:
        with G._hl_reduction(not packed):
            seen = G._learn_parity(learner, oracle, traj, lens, genes, learner.fitness(cum, genes), minibatches,
                                   packed=packed)
    return learner, lens, seen
