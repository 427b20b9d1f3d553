"""Lane maps of the 16x16x32 bf16 MFMA path of the inference convolutions, restated in numpy (no GPU).

The functions below carry the names of everyvoice_amd/csrc/mfma16_layout.h and must say what that header says (change both
together; ``test_header_and_restatement_agree`` compares the expressions as text).  What is checked:

(a) LDS banking of the ``ds_read_b128`` fragment reads: the hardware serves a wave's 64 addresses in four groups of 16 lanes, and a
    group is conflict-free when its addresses are 16 distinct 16-byte slots of the 256-byte bank row.  The weight image (swizzle of
    the 32x32 kernels, read at rows that are multiples of 16) and the activation tile (swizzle ``row & 6``, read at EVERY row offset
    a tap can produce) must be conflict-free; the 32x32 kernels' swizzle on the activation tile must NOT be, or this test could not fail.
(b) the A and B lanes of one instruction hold the same 32 k values, and the two k-steps cover a 64-channel chunk exactly once --
    through the swizzled addresses, on an LDS image filled the way the kernel's source-side permutation fills it.
(c) the epilogue: accumulator registers -> packed bf16 pairs -> v_permlane16_swap -> one 16-byte vector per lane; every (row,
    channel) of the 64 x 64 wave tile lands exactly once, at its flat index, and the whole chain equals W @ X.
"""
import re
from pathlib import Path

import numpy as np

HEADER = Path(__file__).resolve().parents[1] / "everyvoice_amd" / "csrc" / "mfma16_layout.h"


# ---- mfma16_layout.h, restated -------------------------------------------------------------------------------------------------
def x_swizzle(row):
    return row & 6


def w_swizzle(row):
    return (row >> 1) & 7


def frag_vec(lane, s):
    return (lane >> 4) + 4 * s


def frag_offset(row, vec, swz):
    return row * 128 + ((vec ^ swz) << 4)


def acc_row(lane):
    return lane & 15


def acc_channel(lane, i):
    return 4 * (lane >> 4) + i


def swapped_tile(lane):
    return (lane >> 4) & 1


def swapped_channel(lane):
    return 8 * (lane >> 5)


_RESTATED = {
    "x_swizzle": "row & 6",
    "w_swizzle": "(row >> 1) & 7",
    "frag_vec": "(lane >> 4) + 4 * s",
    "frag_offset": "row * 128 + ((vec ^ swz) << 4)",
    "acc_row": "lane & 15",
    "acc_channel": "4 * (lane >> 4) + i",
    "swapped_tile": "(lane >> 4) & 1",
    "swapped_channel": "8 * (lane >> 5)",
}

LANE = np.arange(64)
# ds_read_b128: the four 16-lane groups that are served together
_G0 = [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27]
_G1 = [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31]
B128_GROUPS = [np.array(g) for g in (_G0, _G1, [l + 32 for l in _G0], [l + 32 for l in _G1])]
MAX_TAP_SHIFT = 10 * 5  # (k11 - 1) taps x dilation 5


def ways(addr):
    """Worst number of lanes of one group on one 16-byte slot of the 256-byte bank row (1 = conflict-free)."""
    return max(int(np.bincount((addr[g] // 16) % 16, minlength=16).max()) for g in B128_GROUPS)


def read16(row0, s, swizzle):
    """Byte addresses of the 16x16x32 fragment read of k-step s on the 16 rows from row0."""
    row = row0 + (LANE & 15)
    return frag_offset(row, frag_vec(LANE, s), swizzle(row))


def read32(row0, ks, swizzle):
    """The 32x32x16 read (conv_tc_dma_kernel.h, off_a / off_b of that shape), for contrast."""
    row = row0 + (LANE & 31)
    return row * 128 + (((2 * ks + (LANE >> 5)) ^ swizzle(row)) << 4)


def test_header_and_restatement_agree():
    text = HEADER.read_text()
    for name, expr in _RESTATED.items():
        m = re.search(r"constexpr int " + name + r"\([^)]*\) \{ return (.*?); \}", text)
        assert m, f"{name} not found in {HEADER.name}"
        assert m.group(1) == expr, (name, m.group(1), expr)
    # and the python functions are those expressions
    for name, expr in _RESTATED.items():
        env = dict(row=77, lane=53, s=1, vec=5, swz=6, i=3)
        assert globals()[name](*[env[a] for a in globals()[name].__code__.co_varnames[: globals()[name].__code__.co_argcount]]) == eval(expr, {}, env)


def test_weight_image_reads_are_conflict_free_at_16_row_offsets():
    for row0 in range(0, 128, 16):
        for s in (0, 1):
            assert ways(read16(row0, s, w_swizzle)) == 1, (row0, s)


def test_activation_tile_reads_are_conflict_free_at_every_row_offset():
    for row0 in range(0, 256 + MAX_TAP_SHIFT):
        for s in (0, 1):
            assert ways(read16(row0, s, x_swizzle)) == 1, (row0, s)


def test_the_32x32_swizzle_would_conflict_under_the_16_row_read_and_vice_versa():
    """The swizzle is a property of the shape: each one is conflict-free under its own read only."""
    old16 = [ways(read16(r, s, w_swizzle)) for r in range(256 + MAX_TAP_SHIFT) for s in (0, 1)]
    assert max(old16) == 2
    # conflict-free only where the first row is a multiple of 4
    assert all((w == 1) == (r % 4 == 0) for r in range(256 + MAX_TAP_SHIFT) for w in [ways(read16(r, 0, w_swizzle))])
    assert all(ways(read32(r, ks, w_swizzle)) == 1 for r in range(256 + MAX_TAP_SHIFT) for ks in range(4))
    assert all(ways(read32(r, ks, x_swizzle)) == 2 for r in range(256 + MAX_TAP_SHIFT) for ks in range(4))


def _lds_image(values, swizzle):
    """[rows][64 channels] -> bytes-as-elements image [rows * 64]: slot p of row r holds channel vector p ^ swizzle(r) -- what
    issue_x's source-side permutation (and relayout_conv's layout 1 for the weights) leaves in the LDS."""
    rows = values.shape[0]
    img = np.empty((rows, 8, 8), values.dtype)
    for r in range(rows):
        for p in range(8):
            img[r, p] = values[r, 8 * (p ^ swizzle(r)) : 8 * (p ^ swizzle(r)) + 8]
    return img.reshape(rows * 64)


def _fragment(img, row0, s, swizzle):
    """[64 lanes][8]: the 16 bytes (8 elements) each lane's ds_read_b128 returns, and the channel each element is."""
    off = read16(row0, s, swizzle) // 2  # elements
    return np.stack([img[o : o + 8] for o in off])


def test_operand_lanes_cover_the_same_k_once_per_chunk():
    # an image whose element values are their own channel numbers
    chan = np.tile(np.arange(64), (128, 1))
    seen = np.zeros((64, 64), int)  # [lane][channel]
    for row0, swz in ((16, w_swizzle), (37, x_swizzle)):  # a weight tile, an activation tile at an odd tap offset
        img = _lds_image(chan, swz)
        for s in (0, 1):
            got = _fragment(img, row0, s, swz)
            # lane l holds k = 8 (l >> 4) + j of the 32-deep step: channels 32 s + 8 (l >> 4) + j... as frag_vec says
            want = 8 * frag_vec(LANE, s)[:, None] + np.arange(8)[None, :]
            assert np.array_equal(got, want), (row0, s)
            if swz is x_swizzle:
                for l in range(64):
                    seen[l, got[l]] += 1
    # over the two k-steps the four lanes (l & 15 fixed) of a row see each of the 64 channels exactly once
    per_row = seen.reshape(4, 16, 64).sum(axis=0)
    assert np.array_equal(per_row, np.ones((16, 64), int))
    # A and B of one instruction: same k per lane (same frag_vec), and one instruction's 64 lanes cover 32 distinct k per row
    for s in (0, 1):
        k = (8 * frag_vec(LANE, s)[:, None] + np.arange(8)[None, :]).reshape(4, 16, 8)
        assert all(len(set(k[:, n].ravel())) == 32 for n in range(16))


def _mfma_16x16x32(a_frag, b_frag, acc):
    """acc[lane][4] += the instruction, through its lane maps: A[row l & 15][k = 8 (l >> 4) + j], B[k][col l & 15],
    D[row 4 (l >> 4) + i][col l & 15]."""
    A = np.zeros((16, 32))
    B = np.zeros((32, 16))
    for l in range(64):
        A[l & 15, 8 * (l >> 4) : 8 * (l >> 4) + 8] = a_frag[l]
        B[8 * (l >> 4) : 8 * (l >> 4) + 8, l & 15] = b_frag[l]
    D = A @ B
    for l in range(64):
        for i in range(4):
            acc[l, i] += D[acc_channel(l, i), acc_row(l)]


def _permlane16_swap(vdst, src):
    """v_permlane16_swap: the odd 16-lane rows of vdst change places with the even rows of src."""
    d, s = vdst.copy(), src.copy()
    for base in (0, 32):
        d[base + 16 : base + 32] = src[base : base + 16]
        s[base : base + 16] = vdst[base + 16 : base + 32]
    return d, s


def test_wave_tile_through_fragments_mfma_and_swap_equals_the_gemm():
    rng = np.random.default_rng(0)
    tap_shift = 13  # an activation row offset that is not a multiple of 4
    W = rng.integers(-4, 5, (64, 64)).astype(float)  # [channel out][channel in]: one wave's 64 rows of a weight image
    X = rng.integers(-4, 5, (64 + tap_shift, 64)).astype(float)  # [row][channel in]
    w_img, x_img = _lds_image(W, w_swizzle), _lds_image(X, x_swizzle)
    acc = np.zeros((4, 4, 64, 4))  # [mt][nt][lane][reg]
    for s in (0, 1):
        for mt in range(4):
            for nt in range(4):
                _mfma_16x16x32(_fragment(w_img, mt * 16, s, w_swizzle), _fragment(x_img, tap_shift + nt * 16, s, x_swizzle), acc[mt, nt])
    want = X[tap_shift:] @ W.T  # [row][channel out]

    # the accumulator map (LDS-staged epilogue and bias initialisation): register i of lane l of tile (mt, nt)
    for mt in range(4):
        for nt in range(4):
            for l in range(64):
                for i in range(4):
                    assert acc[mt, nt, l, i] == want[nt * 16 + acc_row(l), mt * 16 + acc_channel(l, i)]

    # the direct epilogue: per channel tile mt and pair of row tiles (2 np, 2 np + 1), d = (quad of tile 2 np | quad of tile 2 np + 1)
    # as dword pairs; swap d[0] <-> d[2], d[1] <-> d[3]; the lane stores (d0, d1, d2, d3) = 8 channels at
    # row np * 32 + (lane & 31), channel mt * 16 + 8 (lane >> 5)
    out = np.full((64, 64), np.nan)
    count = np.zeros((64, 64), int)
    for mt in range(4):
        for np_ in range(2):
            lo, hi = acc[mt, 2 * np_], acc[mt, 2 * np_ + 1]  # [lane][4]
            # a packed dword = two channels; keep them as pairs of floats
            d = [lo[:, 0:2], lo[:, 2:4], hi[:, 0:2], hi[:, 2:4]]
            d[0], d[2] = _permlane16_swap(d[0], d[2])
            d[1], d[3] = _permlane16_swap(d[1], d[3])
            vec = np.concatenate(d, axis=1)  # [lane][8 channels]
            for l in range(64):
                row = np_ * 32 + (l & 31)
                assert row == (2 * np_ + swapped_tile(l)) * 16 + acc_row(l)
                c0 = mt * 16 + swapped_channel(l)
                out[row, c0 : c0 + 8] = vec[l]
                count[row, c0 : c0 + 8] += 1
    assert np.array_equal(count, np.ones((64, 64), int))
    assert np.array_equal(out, want)
    # the swap is its own inverse (the running-sum load goes through it the other way)
    a, b = rng.random((64, 2)), rng.random((64, 2))
    a2, b2 = _permlane16_swap(*_permlane16_swap(a, b))
    assert np.array_equal(a, a2) and np.array_equal(b, b2)
