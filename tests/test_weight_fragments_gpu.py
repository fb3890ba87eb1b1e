"""Fragment-order weight images (XtrlTrainDesc.wfrag): the build kernel against the numpy restatement
(tests/wfrag_ref.py), and decoder learn steps, forward + backward, with the fragments on and off in one
process — same pieces, same MFMAs in the same order, so every stored activation, every backward plane and
the flat gradient must be bit-identical (torch.equal, no tolerance)."""
import numpy as np
import pytest
import torch

import wfrag_ref as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def test_fragment_build_matches_numpy_restatement():
    """Every image of one build launch equals the restatement byte for byte, zeros past N and K included:
    N in {256, 200} x K in {32, 64, 260, 1024}, both orientations, plus a column sub-view with ld > N."""
    from xtrl_amd import _lib as L
    rng = np.random.default_rng(3)
    entries, off = [], 3
    for N in (256, 200):
        for K in (32, 64, 260, 1024):
            entries += [(off, N, K, K, 0), (off, N, K, N, 1)]   # the same floats as [N][K] and as [K][N]
            off += N * K
    entries.append((off + 64, 200, 72, 264, 1))   # B[k][n] = w[k * 264 + 64 + n]: columns 64 .. 263 of [72][264]
    off += 72 * 264
    flat = (rng.standard_normal(off) * 0.05).astype(np.float32)
    flat[5] = 0.
    rows, nbytes = F.plan(entries)
    tab = (L.WfragEntry * len(rows))()
    for e, r in zip(tab, rows):
        e.w_off, e.img_off, e.N, e.K, e.ld, e.trans_b, e.blk0 = r
    tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(DEV)
    arena = torch.full((nbytes + 64,), 0xA5, device=DEV, dtype=torch.uint8)
    flat_dev = torch.from_numpy(flat).to(DEV)
    L.check(L.lib().xtrl_wfrag_build(flat_dev.data_ptr(), tab, tab_dev.data_ptr(), len(rows), arena.data_ptr(), nbytes,
                                     L.stream()), 'wfrag_build')
    torch.cuda.synchronize()
    got = arena.cpu().numpy()
    assert (got[nbytes:] == 0xA5).all()   # nothing past the last image
    for (w_off, N, K, ld, tb), r in zip(entries, rows):
        ref = F.image(flat, w_off, N, K, ld, tb)
        g = got[r[1]:r[1] + ref.nbytes].view(np.uint16).reshape(ref.shape)
        np.testing.assert_array_equal(g, ref, err_msg=f'image N={N} K={K} ld={ld} trans_b={tb}')


# ---- decoder learn steps, fragments on vs off ---------------------------------------------------

def _learner(dim, depth, heads, b, n):
    from xtrl_amd import Learner
    torch.manual_seed(5)
    # (two heads: without the learned mix, whose extra columns would leave n_qkv off a multiple of 4 and the
    # step off the fused LayerNorm path)
    wm = dict(attn_dim_head=16, heads=heads, depth=depth, attn_gate_values=True, add_value_residual=True,
              learned_value_residual_mix=heads % 4 == 0)
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

    def __init__(self, dim, heads, packed, depth=2, b=2, n=40, lens=(40, 33)):
        self.agent = agent = _learner(dim, depth, heads, b, n)
        self.step = step = agent.train_step(b, n)
        self.depth = depth
        # on by default, one image per launch that reads one
        assert step.wfrag is not None and len(step.wfrag['tab']) == 4 * depth + 1 and step.D.wfrag
        assert not step.D.wimg   # the LDS-DMA images stay off unless asked for
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

    def run(self, fragments, images=False):
        """Forward + backward; every buffer of the step (stored activations, backward planes) and the flat
        gradient, cloned.  self.fed / self.fed_img: the launches that read a fragment / an LDS-DMA image."""
        step, flat = self.step, self.agent.flat
        from xtrl_amd import _lib as L
        step.use_weight_fragments(fragments)
        step.use_weight_images(images)
        assert bool(step.D.wfrag) == fragments and bool(step.D.wimg) == images
        f0, i0 = L.lib().xtrl_wfrag_launch_count(), L.lib().xtrl_wimg_launch_count()
        flat.grad.zero_()
        step.forward(self.swr, self.prev, self.act, None, self.lens, 1.0, 11, 0, 0, 0.25, Tv=self.Tv,
                     packed=self.packed)
        step.backward()
        torch.cuda.synchronize()
        self.fed = L.lib().xtrl_wfrag_launch_count() - f0
        self.fed_img = L.lib().xtrl_wimg_launch_count() - i0
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
        # on the bit patterns: as strict on every number, and a plane the step leaves unwritten in this mode
        # (buf.dzp with the compact heads) may hold NaN patterns, which never compare equal as floats
        assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k
    assert torch.isfinite(a['grad']).all() and float(a['grad'].abs().max()) > 0.


@pytest.mark.parametrize('dim,heads,packed', [
    (256, 4, False),   # T = 80: a full and a partial 64-row tile; n_qkv = 260: a K tail, 9 slabs (odd)
    (256, 4, True),    # the packed step at 73 tokens
    (256, 2, False),   # out-projection K = 32: a single slab, shorter than the lookahead
    (192, 4, False),   # N < 256: the image's zero columns are read
])
def test_train_step_bit_identical_with_fragments(dim, heads, packed):
    s = _Step(dim, heads, packed)
    on = s.run(True)
    assert s.fed == 4 * s.depth + 1 and s.fed_img == 0
    assert s.step.wfrag['arena'].any()   # the forward built the images
    off = s.run(False)
    assert s.fed == 0 and s.fed_img == 0
    _same(on, off)


def test_launch_counters():
    """Per step: 4 * depth + 1 fragment-fed launches with the fragments on, none with them off; with the LDS-DMA
    images on those launches take that image (its counter as ever) and none reads a fragment."""
    s = _Step(256, 4, False)
    s.run(True)
    assert (s.fed, s.fed_img) == (4 * s.depth + 1, 0)
    s.run(False)
    assert (s.fed, s.fed_img) == (0, 0)
    both = s.run(True, images=True)
    assert (s.fed, s.fed_img) == (0, 4 * s.depth + 1)
    _same(both, s.run(True))
    assert (s.fed, s.fed_img) == (4 * s.depth + 1, 0)


def test_fragments_follow_the_parameters():
    """Coherence: a step, the parameters changed in place, a step — the second equals the fragment-free path
    on the changed parameters (the forward rebuilds the images from what it is about to read)."""
    s = _Step(256, 4, False)
    first = s.run(True)
    with torch.no_grad():
        flat = s.agent.flat.flat
        flat.add_(torch.randn(flat.shape, generator=torch.Generator().manual_seed(8)).to(DEV) * 0.01)
    second = s.run(True)
    assert not torch.equal(first['grad'], second['grad'])
    _same(second, s.run(False))
