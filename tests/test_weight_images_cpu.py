"""The numpy restatement of the pre-split weight images (tests/wimg_ref.py) that the GPU test compares
the build kernel with, checked on its own; and the library's host-only image plan."""
import ctypes as C

import numpy as np

import wimg_ref as W


def test_split3_pieces_are_rne_bf16_and_sum_exactly():
    """hi + mid + lo == x exactly in float64, each piece the round-to-nearest-even bf16 of the running
    remainder: |remainder - piece| <= half a bf16 ulp of the piece's binade, ties to an even mantissa."""
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(4096).astype(np.float32) * np.float32(0.05),
                        np.float32([0., 1., -1., 1.00390625, 1.01171875, 3.0e-3, -7.5, 0.1])])
    hi, mid, lo = W.split3_bits(x)
    h, m, l = (W.bf16_value(b).astype(np.float64) for b in (hi, mid, lo))
    np.testing.assert_array_equal(h + m + l, x.astype(np.float64))
    # bf16 keeps 8 significand bits: the low 16 bits of the float32 pattern are gone
    for b in (hi, mid, lo):
        assert b.dtype == np.uint16
    # rne: 1 + 2^-8 is a tie between 1 and 1 + 2^-7 -> even (1); 1 + 3 * 2^-8 ties -> 1 + 2^-6 (even)
    assert W.bf16_value(W.bf16_rne_bits(np.float32([1.00390625])))[0] == np.float32(1.0)
    assert W.bf16_value(W.bf16_rne_bits(np.float32([1.01171875])))[0] == np.float32(1.015625)
    r = x.astype(np.float64) - h
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(h), 1e-300))) - 7)
    assert np.all(np.abs(r) <= ulp / 2)


def test_image_layout_both_orientations():
    """Element [tile j * nkt + s][p][r][c] is piece p of B[32 s + c][BN j + r]; rows past N, k past K and the
    pad columns are exactly zero — for the issue's three weights read forward and transposed."""
    rng = np.random.default_rng(1)
    for Nw, Kw in ((260, 256), (256, 64), (8, 36)):
        flat = rng.standard_normal(5 + Nw * Kw).astype(np.float32)
        for tb, N, K in ((0, Nw, Kw), (1, Kw, Nw)):   # the weight [Nw][Kw] as B "N", and as B "T"
            for BN in (128, 256):
                img = W.image(flat, 5, N, K, Kw, tb, BN)
                ntn, nkt = -(-N // BN), -(-K // 32)
                assert img.shape == (ntn * nkt, 3, BN, 40) and img.nbytes == ntn * nkt * W.tile_bytes(BN)
                B = W.operand(flat, 5, N, K, Kw, tb)
                w2 = flat[5:].reshape(Nw, Kw)
                np.testing.assert_array_equal(B, w2.T if tb else w2)
                pieces = W.split3_bits(B)
                for n, k in ((0, 0), (N - 1, K - 1), (N // 2, K // 3), (min(N - 1, 129), min(K - 1, 33))):
                    j, r, s, c = n // BN, n % BN, k // 32, k % 32
                    for p in range(3):
                        assert img[j * nkt + s, p, r, c] == pieces[p][n, k]
                assert not img[:, :, :, 32:].any()
                full = np.zeros((ntn * BN, nkt * 32), bool)
                full[:N, :K] = True
                pad = ~full.reshape(ntn, BN, nkt, 32).transpose(0, 2, 1, 3).reshape(ntn * nkt, BN, 32)
                for p in range(3):
                    assert not img[:, p, :, :32][pad].any()


def test_library_plan_matches_restatement_plan():
    """xtrl_train_wimg_plan (host-only) on a d = 256, depth 2 gated decoder: 4 images per block plus the two
    of the actor | critic first layer, back to back in the arena, each sized by its tile count."""
    from xtrl_amd import _lib as L
    lib = L.load()
    d, H, dh, ff, depth = 256, 4, 16, 1024, 2
    I = H * dh
    layers = (L.TrainLayer * depth)()
    at = 0
    want = []
    for li in range(depth):
        n_qkv = 4 * I + (H if li else 0)
        Ly = layers[li]
        Ly.n_qkv, Ly.mix = n_qkv, int(li > 0)
        Ly.w_proj, at = at, at + n_qkv * d
        Ly.w_out, at = at, at + d * I
        Ly.w_ff1, at = at, at + ff * d
        Ly.w_ff2, at = at, at + d * ff
        want += [(Ly.w_out, d, I, I, 0, 256), (Ly.w_ff2, d, ff, ff, 0, 256), (Ly.w_ff1, d, ff, d, 1, 256),
                 (Ly.w_proj, d, n_qkv, d, 1, 256)]
    D = L.TrainDesc()
    D.d, D.L, D.H, D.dh, D.ff, D.in_dim, D.gate_values = d, depth, H, dh, ff, 2 * d, 1
    D.layers = C.cast(layers, C.POINTER(L.TrainLayer))
    D.w_h1 = at
    want += [(at, d, 4 * d, 2 * d, 1, 256), (at + d, d, 4 * d, 2 * d, 1, 128)]
    nbytes = C.c_int64(0)
    n = lib.xtrl_train_wimg_plan(C.byref(D), None, 0, C.byref(nbytes))
    assert n == 4 * depth + 2
    tab = (L.WimgEntry * n)()
    assert lib.xtrl_train_wimg_plan(C.byref(D), tab, n, C.byref(nbytes)) == n
    rows, total = W.plan(want)
    got = [(e.w_off, e.img_off, e.N, e.K, e.ld, e.trans_b, e.BN, e.blk0) for e in tab]
    assert got == rows and nbytes.value == total
    assert L.wimg_tile_bytes(256) == W.tile_bytes(256) == 61440
    # a model the LayerNorm epilogues do not cover (d > 256) plans nothing
    D.d, D.in_dim = 512, 1024
    assert lib.xtrl_train_wimg_plan(C.byref(D), None, 0, C.byref(nbytes)) == 0 and nbytes.value == 0
