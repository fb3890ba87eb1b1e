"""The numpy restatement of the fragment-order weight images (tests/wfrag_ref.py) checked on its own, and the
library's host-only fragment plan against it."""
import ctypes as C

import numpy as np

import wfrag_ref as F
import wimg_ref as W


def test_vectorised_restatement_matches_the_definition():
    """The reshaped form the GPU test compares with equals the layout written out lane by lane; the image is
    6 bytes per padded element and zero past N and K."""
    rng = np.random.default_rng(2)
    for N, K in ((200, 36), (256, 64)):
        for tb in (0, 1):
            ld = (N if tb else K) + 4
            flat = rng.standard_normal(7 + (K if tb else N) * ld).astype(np.float32)
            img = F.image(flat, 7, N, K, ld, tb)
            np.testing.assert_array_equal(img, F.image_loops(flat, 7, N, K, ld, tb))
            nkt = -(-K // 32)
            assert img.nbytes == F.units(K) * F.UNIT_BYTES == 256 * nkt * 32 * 6
            # lane l of block (st, p, j) of unit (w, s): column 64 w + 32 j + (l & 31), k = 32 s + 16 st + 8 (l >> 5)
            B = W.operand(flat, 7, N, K, ld, tb)
            pieces = W.split3_bits(B)
            for n, k in ((0, 0), (N - 1, K - 1), (N // 2, K // 3), (min(N - 1, 129), min(K - 1, 33))):
                w, j, c = n // 64, (n % 64) // 32, n % 32
                s, st, h, i = k // 32, (k % 32) // 16, (k % 16) // 8, k % 8
                for p in range(3):
                    assert img[w * nkt + s, st, p, j, 32 * h + c, i] == pieces[p][n, k]
            live = np.zeros((256, nkt * 32), bool)
            live[:N, :K] = True
            dead = ~live.reshape(4, 2, 32, nkt, 2, 2, 8).transpose(0, 3, 4, 1, 5, 2, 6).reshape(4 * nkt, 2, 2, 64, 8)
            for p in range(3):
                assert not img[:, :, p][dead].any()


def _decoder_desc(L, d, depth, H, dh, ff):
    I = H * dh
    layers = (L.TrainLayer * depth)()
    at, want = 0, []
    for li in range(depth):
        n_qkv = 4 * I + (H if li else 0)
        Ly = layers[li]
        Ly.n_qkv, Ly.mix = n_qkv, int(li > 0)
        Ly.w_proj, at = at, at + n_qkv * d
        Ly.w_out, at = at, at + d * I
        Ly.w_ff1, at = at, at + ff * d
        Ly.w_ff2, at = at, at + d * ff
        want += [(Ly.w_out, d, I, I, 0), (Ly.w_ff2, d, ff, ff, 0), (Ly.w_ff1, d, ff, d, 1), (Ly.w_proj, d, n_qkv, d, 1)]
    D = L.TrainDesc()
    D.d, D.L, D.H, D.dh, D.ff, D.in_dim, D.gate_values = d, depth, H, dh, ff, 2 * d, 1
    D.layers = C.cast(layers, C.POINTER(L.TrainLayer))
    D.w_h1 = at
    want.append((at, d, 4 * d, 2 * d, 1))   # the embed columns of the actor | critic first layer
    return D, layers, want


def test_library_plan_matches_restatement_plan():
    """xtrl_train_wfrag_plan (host-only) on a d = 256, depth 2 gated decoder: 4 images per block plus the embed
    columns of the actor | critic first layer, back to back, 12 KiB per (64-column block, slab); models whose
    LayerNorm GEMMs do not run on 64 x 256 tiles plan nothing."""
    from xtrl_amd import _lib as L
    lib = L.load()
    depth = 2
    D, layers, want = _decoder_desc(L, 256, depth, 4, 16, 1024)
    nbytes = C.c_int64(0)
    n = lib.xtrl_train_wfrag_plan(C.byref(D), None, 0, C.byref(nbytes))
    assert n == 4 * depth + 1
    tab = (L.WfragEntry * n)()
    assert lib.xtrl_train_wfrag_plan(C.byref(D), tab, n, C.byref(nbytes)) == n
    rows, total = F.plan(want)
    got = [(e.w_off, e.img_off, e.N, e.K, e.ld, e.trans_b, e.blk0) for e in tab]
    assert got == rows and nbytes.value == total
    assert L.WFRAG_UNIT_BYTES == F.UNIT_BYTES == 12288
    assert C.sizeof(L.WfragEntry) == 40
    # no fused LayerNorm path (d > 256); the 128 x 128 LayerNorm tiles (d <= 128); no layers
    for d in (512, 128):
        D2, layers2, _ = _decoder_desc(L, d, depth, 4, 16, 4 * d)
        assert lib.xtrl_train_wfrag_plan(C.byref(D2), None, 0, C.byref(nbytes)) == 0 and nbytes.value == 0
    D.L = 0
    assert lib.xtrl_train_wfrag_plan(C.byref(D), None, 0, C.byref(nbytes)) == 0 and nbytes.value == 0
