"""(no GPU) NumPy model of the splits' remainder instruction as the kernels use it (w16_ident / w16_rem, epnn_common.h):
v_mfma_f32_4x4x4_16b_bf16 is sixteen independent 4x4x4 products D = C + A B.  Lane 4 b + i holds row i of block b's A and column i of
its B, each as two dwords of bf16 pairs (K slots 0 | 1 and 2 | 3, even slot in the low half), and column i of its C / D as four
registers (rows 0..3).  With A = -I per block (the dwords of w16_ident), a lane's four values as its accumulator and their packed upper
halves (w16_pack_hi2) as its B operand, D is the truncated remainder x - piece of tests/split_ref.py inside every lane, bit for bit."""
import numpy as np

from split_ref import pieces


def _bf16_slots(dwords):
    """[64 lanes][2 dwords] of bf16 pairs -> [64][4 K slots] as float64 (even slot in the low half)."""
    d = np.asarray(dwords, dtype=np.uint32)
    halves = np.stack([d[:, 0] << 16, d[:, 0] & 0xFFFF0000, d[:, 1] << 16, d[:, 1] & 0xFFFF0000], axis=1).astype(np.uint32)
    return halves.view(np.float32).astype(np.float64)


def w16_ident():
    i = np.arange(64) & 3
    return np.stack([np.where(d == (i >> 1), 0xBF80 << (16 * (i & 1)), 0) for d in (0, 1)], axis=1).astype(np.uint32)


def w16_pack_hi2(x):
    """v_perm_b32 0x07060302: the upper halves of x[2 j] (low) and x[2 j + 1] (high) side by side."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.stack([(u[:, 2 * j + 1] & 0xFFFF0000) | (u[:, 2 * j] >> 16) for j in (0, 1)], axis=1)


def mfma_4x4x4(a_dwords, b_dwords, c):
    """D[lane 4 b + j][r] = C[lane 4 b + j][r] + sum_k A[b][r][k] B[b][k][j]; A's row r of block b is lane 4 b + r's operand."""
    A = _bf16_slots(a_dwords).reshape(16, 4, 4)                    # [block][row][k]
    B = _bf16_slots(b_dwords).reshape(16, 4, 4).transpose(0, 2, 1)  # [block][k][column]
    D = np.einsum("brk,bkj->bjr", A, B).reshape(64, 4) + np.asarray(c, dtype=np.float64)
    out = D.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), D)                # nothing is rounded: the result is a float32 number
    return out


def test_the_operand_is_minus_identity_in_every_block():
    A = _bf16_slots(w16_ident()).reshape(16, 4, 4)
    assert all(np.array_equal(A[b], -np.eye(4)) for b in range(16))


def test_remainders_are_the_truncated_split_s():
    rng = np.random.default_rng(2104)
    for trial in range(16):                                         # 16 x 256 values
        x = (rng.standard_normal((64, 4)) * 10.0 ** rng.integers(-6, 7, size=(64, 4))).astype(np.float32)
        if trial == 0:
            x[::5] = 0.0
            x[1::7] = np.float32(-1.5)                              # a bf16 number: every remainder zero
        p1, p2, p3 = pieces(x)
        I = w16_ident()
        r1 = mfma_4x4x4(I, w16_pack_hi2(x), x)
        assert np.array_equal(r1.view(np.uint32), (x - p1).view(np.uint32))
        assert np.array_equal(w16_pack_hi2(r1), w16_pack_hi2(p2))   # the second piece's operand words
        r2 = mfma_4x4x4(I, w16_pack_hi2(r1), r1)
        assert np.array_equal(r2.view(np.uint32), (x - p1 - p2).view(np.uint32))
        assert np.array_equal(w16_pack_hi2(r2), w16_pack_hi2(p3))


def test_a_lane_s_values_stay_in_the_lane():
    """Values in one lane only: its results are its remainders in order, every other lane keeps its zeros (a wrong row / column
    placement would hand them to a neighbour of the block or reorder them)."""
    for lane in (0, 5, 18, 27, 46, 63):
        x = np.zeros((64, 4), dtype=np.float32)
        x[lane] = np.array([1.2345678, -0.0078112348, 517.00391, 3.0000002], dtype=np.float32)
        r = mfma_4x4x4(w16_ident(), w16_pack_hi2(x), x)
        assert np.array_equal(r[lane], x[lane] - pieces(x[lane])[0]) and np.all(r[lane] != 0)
        assert not np.delete(r, lane, axis=0).any()
