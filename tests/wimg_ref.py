"""numpy restatement of the pre-split weight images (XtrlWimgEntry, include/xtrl_hip.h), shared by
test_weight_images_cpu.py and test_weight_images_gpu.py.

A value x is cut into hi = bf16-rne(x), mid = bf16-rne(x - hi), lo = bf16-rne(x - hi - mid) (float32
subtractions, exact).  The image of a B operand with N columns and reduction length K is tiled by
(BN-row tile j, 32-deep K slab s); tile (j, s) is [piece hi | mid | lo][BN rows][40] bf16 with element
[p][r][c], c < 32, the piece p of B[32 s + c][BN j + r]; rows past N, k past K and the 8 pad columns
are zero."""
import numpy as np

BK, XRS = 32, 40


def bf16_rne_bits(x):
    """Round-to-nearest-even bf16 of finite float32 values, as uint16 bit patterns."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = u + 0x7FFF + ((u >> 16) & 1)
    return ((r >> 16) & 0xFFFF).astype(np.uint16)


def bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def split3_bits(x):
    """The three bf16 pieces of float32 x as bit patterns (hi, mid, lo)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    hi = bf16_rne_bits(x)
    r1 = (x - bf16_value(hi)).astype(np.float32)
    mid = bf16_rne_bits(r1)
    r2 = (r1 - bf16_value(mid)).astype(np.float32)
    return hi, mid, bf16_rne_bits(r2)


def operand(flat, w_off, N, K, ld, trans_b):
    """B as an [N][K] array (row n, reduction index k) from the flat float32 buffer."""
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing='ij')
    at = w_off + (k * ld + n if trans_b else n * ld + k)
    return np.asarray(flat, dtype=np.float32)[at]


def tile_bytes(bn):
    return 3 * bn * XRS * 2


def image(flat, w_off, N, K, ld, trans_b, BN):
    """uint16 [tiles][3][BN][40]: the image of one table entry, tile index j * ceil(K / 32) + s."""
    ntn, nkt = -(-N // BN), -(-K // BK)
    B = np.zeros((ntn * BN, nkt * BK), np.float32)
    B[:N, :K] = operand(flat, w_off, N, K, ld, trans_b)
    out = np.zeros((ntn * nkt, 3, BN, XRS), np.uint16)
    for p, bits in enumerate(split3_bits(B)):
        t = bits.reshape(ntn, BN, nkt, BK).transpose(0, 2, 1, 3)   # [j][s][r][c]
        out[:, p, :, :BK] = t.reshape(ntn * nkt, BN, BK)
    return out


def plan(entries):
    """entries: (w_off, N, K, ld, trans_b, BN) -> rows (w_off, img_off, N, K, ld, trans_b, BN, blk0) and the
    arena bytes, images back to back in table order."""
    rows, at, blk = [], 0, 0
    for w_off, N, K, ld, tb, BN in entries:
        tiles = -(-N // BN) * -(-K // BK)
        rows.append((w_off, at, N, K, ld, tb, BN, blk))
        at += tiles * tile_bytes(BN)
        blk += tiles
    return rows, at
