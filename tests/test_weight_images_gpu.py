"""Pre-split weight images (XtrlTrainDesc.wimg): the build kernel against the numpy restatement
(tests/wimg_ref.py), and one decoder learn step, forward + backward, with the images on and off in one
process — same pieces, same MFMAs in the same order, so every stored activation and every gradient
must be bit-identical (torch.equal, no tolerance)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import wimg_ref as W

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _table(rows):
    from xtrl_amd import _lib as L
    tab = (L.WimgEntry * len(rows))()
    for e, r in zip(tab, rows):
        e.w_off, e.img_off, e.N, e.K, e.ld, e.trans_b, e.BN, e.blk0 = r
    return tab


def test_image_build_matches_numpy_restatement():
    """Every image of one build launch equals the restatement byte for byte, padding included: the issue's
    three weights (260 x 256: N off the tile, K tail of 4 transposed; 256 x 64: two slabs; 8 x 36: tail
    slab, N < 32) in both orientations and both tile heights, plus a column sub-view with ld > K."""
    from xtrl_amd import _lib as L
    rng = np.random.default_rng(3)
    entries, off = [], 3
    for Nw, Kw in ((260, 256), (256, 64), (8, 36)):
        for BN in (128, 256):
            entries += [(off, Nw, Kw, Kw, 0, BN), (off, Kw, Nw, Kw, 1, BN)]
        off += Nw * Kw
    entries.append((off + 64, 100, 72, 164, 1, 128))   # B[k][n] = w[k * 164 + 64 + n]: columns 64 .. 163 of [72][164]
    off += 72 * 164
    flat = (rng.standard_normal(off) * 0.05).astype(np.float32)
    flat[5] = 0.
    rows, nbytes = W.plan(entries)
    tab = _table(rows)
    tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(DEV)
    arena = torch.full((nbytes + 64,), 0xA5, device=DEV, dtype=torch.uint8)
    flat_dev = torch.from_numpy(flat).to(DEV)
    L.check(L.lib().xtrl_wimg_build(flat_dev.data_ptr(), tab, tab_dev.data_ptr(), len(rows), arena.data_ptr(), nbytes,
                                    L.stream()), 'wimg_build')
    torch.cuda.synchronize()
    got = arena.cpu().numpy()
    assert (got[nbytes:] == 0xA5).all()   # nothing past the last image
    for (w_off, N, K, ld, tb, BN), r in zip(entries, rows):
        ref = W.image(flat, w_off, N, K, ld, tb, BN)
        g = got[r[1]:r[1] + ref.nbytes].view(np.uint16).reshape(ref.shape)
        np.testing.assert_array_equal(g, ref, err_msg=f'image N={N} K={K} ld={ld} trans_b={tb} BN={BN}')


# ---- one decoder learn step, images on vs off ---------------------------------------------------

def _learner(dim, depth, b, n):
    from xtrl_amd import Learner
    torch.manual_seed(5)
    wm = dict(attn_dim_head=16, heads=4, depth=depth, attn_gate_values=True, add_value_residual=True,
              learned_value_residual_mix=True)
    learner = Learner(state_dim=8, num_actions=4, reward_range=(-2., 2.), world_model=wm, max_timesteps=n,
                      batch_size=b, num_episodes_per_update=b, agent_kwargs=dict(dropout=0.25, seed=5, hidden_dim=dim),
                      use_graph=False)
    with torch.no_grad():   # non-trivial gate / mix weights (their init is constant)
        g = torch.Generator().manual_seed(6)
        for name, p in learner.agent.model.named_parameters():
            if 'to_v_gate' in name or 'to_value_residual_mix' in name:
                p.copy_((torch.randn(p.shape, generator=g) * 0.3).to(p.device))
    return learner.agent


class _Step:
    """A FusedTrainStep with a fixed random minibatch and fixed loss gradients."""

    def __init__(self, dim, depth, b, n, lens, packed, plain=0):
        self.plain = plain   # image-fed launches of the plain 128 x 128 kernel this shape reaches
        self.agent = agent = _learner(dim, depth, b, n)
        self.step = step = agent.train_step(b, n)
        step.use_weight_images(True)   # (off by default: allocates the arena and the table)
        assert step.wimg is not None and len(step.wimg['tab']) == 4 * depth + 2
        assert os.environ.get('XTRL_WIMG', '1') != '0', 'XTRL_WIMG=0 turns the path under test off'
        g = torch.Generator().manual_seed(7)
        r = lambda *s: torch.randn(*s, generator=g).to(DEV)
        self.swr = r(b, n, 9).contiguous()
        act = torch.randint(0, 4, (b, n), generator=g, dtype=torch.int32)
        prev = torch.full_like(act, -1)
        prev[:, 1:] = act[:, :-1]
        self.act, self.prev = act.to(DEV), prev.to(DEV)
        self.lens = torch.tensor(lens, dtype=torch.int32, device=DEV)
        self.Tv, self.packed = int(sum(min(x, n) for x in lens)), packed
        for k in ('d_raw', 'd_values', 'd_pred', 'd_done'):
            step.buf[k].copy_(r(*step.buf[k].shape) * 0.1)

    def run(self, images):
        """Forward + backward; every buffer of the step (stored activations, backward planes) and the flat
        gradient, cloned."""
        step, flat = self.step, self.agent.flat
        from xtrl_amd import _lib as L
        step.use_weight_images(images)
        assert bool(step.D.wimg) == images
        count0 = L.lib().xtrl_wimg_launch_count()
        flat.grad.zero_()
        step.forward(self.swr, self.prev, self.act, None, self.lens, 1.0, 11, 0, 0, 0.25, Tv=self.Tv,
                     packed=self.packed)
        step.backward()
        torch.cuda.synchronize()
        # image-fed launches: per block the out-projection and FF2 (forward), FF1 and q|k|v (input
        # gradients); the final norm's input gradient; `plain` more where the test's shape reaches them
        self.fed = L.lib().xtrl_wimg_launch_count() - count0
        assert self.fed == ((4 * len(step.layers_py) + 1 + self.plain) if images else 0), self.fed
        out = {'grad': flat.grad.clone()}
        for k, t in step.buf.items():
            out['buf.' + k] = t.clone()
        for li, bufs in enumerate(step.layers_py):
            for k, t in bufs.items():
                out[f'layer{li}.{k}'] = t.clone()
        return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        # on the bit patterns (as test_weight_fragments_gpu): as strict on every number, and a plane the step leaves
        # unwritten in this mode (buf.dxn) holds whatever the allocator's block held before — NaN patterns once an
        # earlier test has filled its outputs with NaN — which never compare equal as floats
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert torch.isfinite(a['grad']).all() and float(a['grad'].abs().max()) > 0.


@pytest.mark.parametrize('dim,b,n,lens,packed', [
    (256, 2, 40, (40, 33), False),    # T = 80: a full and a partial 64-row tile; 64 x 256 tiles; n_qkv = 260 (K tail)
    (128, 2, 40, (40, 33), False),    # the 128 x 128 LayerNorm tiles
    (256, 2, 40, (40, 33), True),     # the packed step at 73 tokens (not a multiple of 32)
    (256, 96, 128, (128,) * 95 + (77,), False),   # 192 tiles of 128 x 128: the plain image-fed input gradient
])
def test_train_step_bit_identical_with_images(dim, b, n, lens, packed):
    s = _Step(dim, 1 if b > 2 else 2, b, n, lens, packed, plain=1 if b > 2 else 0)
    on = s.run(True)
    assert s.step.wimg['arena'].any()   # the forward built the images
    _same(on, s.run(False))


def test_images_follow_the_parameters():
    """Coherence: a step, the parameters changed in place, a step — the second equals the image-free path on
    the changed parameters (the forward rebuilds the images from what it is about to read)."""
    s = _Step(256, 2, 2, 40, (40, 33), False)
    first = s.run(True)
    with torch.no_grad():
        flat = s.agent.flat.flat
        flat.add_(torch.randn(flat.shape, generator=torch.Generator().manual_seed(8)).to(DEV) * 0.01)
    second = s.run(True)
    assert not torch.equal(first['grad'], second['grad'])
    _same(second, s.run(False))
