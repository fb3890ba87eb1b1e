"""numpy restatement of the fragment-order weight images (XtrlWfragEntry, include/xtrl_hip.h), shared by
test_weight_fragments_cpu.py and test_weight_fragments_gpu.py.

The B operand (N <= 256 columns, reduction length K) is padded with zeros to 256 columns and to whole
32-deep slabs and cut into the same three bf16 pieces as the LDS-DMA images (wimg_ref.split3_bits).
Unit (w, s) — the 64 columns of consumer wave w, slab s — is 12 blocks of 1 KiB at unit index
w * ceil(K / 32) + s; block ((st * 3 + p) * 2 + j) belongs to k16 step st, piece p, 32-column tile j; lane
l of a block holds the 8 values k = 32 s + 16 st + 8 (l >> 5) + 0..7 of column 64 w + 32 j + (l & 31)."""
import numpy as np

import wimg_ref as W

BK, UNIT_BYTES, COLS = 32, 12 * 1024, 256


def units(K):
    return 4 * -(-K // BK)


def image(flat, w_off, N, K, ld, trans_b):
    """uint16 [4 * nkt][2 st][3 p][2 j][64 lanes][8]: the image of one table entry."""
    assert 0 < N <= COLS
    nkt = -(-K // BK)
    B = np.zeros((COLS, nkt * BK), np.float32)
    B[:N, :K] = W.operand(flat, w_off, N, K, ld, trans_b)
    out = np.zeros((4, nkt, 2, 3, 2, 2, 32, 8), np.uint16)   # [w][s][st][p][j][l >> 5][l & 31][i]
    for p, bits in enumerate(W.split3_bits(B)):
        t = bits.reshape(4, 2, 32, nkt, 2, 2, 8)              # [w][j][c][s][st][h][i]
        out[:, :, :, p] = t.transpose(0, 3, 4, 1, 5, 2, 6)    # [w][s][st][j][h][c][i]
    return out.reshape(4 * nkt, 2, 3, 2, 64, 8)


def image_loops(flat, w_off, N, K, ld, trans_b):
    """The same image element by element, straight from the layout's definition (small cases only)."""
    nkt = -(-K // BK)
    B = np.zeros((COLS, nkt * BK), np.float32)
    B[:N, :K] = W.operand(flat, w_off, N, K, ld, trans_b)
    pieces = W.split3_bits(B)
    out = np.zeros((4 * nkt, 2, 3, 2, 64, 8), np.uint16)
    for w in range(4):
        for s in range(nkt):
            for st in range(2):
                for p in range(3):
                    for j in range(2):
                        for l in range(64):
                            col, k0 = 64 * w + 32 * j + (l & 31), 32 * s + 16 * st + 8 * (l >> 5)
                            out[w * nkt + s, st, p, j, l] = pieces[p][col, k0:k0 + 8]
    return out


def plan(entries):
    """entries: (w_off, N, K, ld, trans_b) -> rows (w_off, img_off, N, K, ld, trans_b, blk0) and the arena
    bytes, images back to back in table order."""
    rows, at, blk = [], 0, 0
    for w_off, N, K, ld, tb in entries:
        rows.append((w_off, at, N, K, ld, tb, blk))
        at += units(K) * UNIT_BYTES
        blk += units(K)
    return rows, at
