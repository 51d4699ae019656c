"""The K = 16 products of the fused kernels as three K = 32 MFMAs (w16_mm_bfk16, epnn_common.h), emulated in NumPy: no GPU.

Both operands are split by truncation into three bf16 pieces, x = x1 + x2 + x3 exactly.  Two K = 16 operands side by side in four
dwords are one K = 32 operand (lane group q: K slots 8q .. 8q + 3 from the first, 8q + 4 .. 8q + 7 from the second), so

    (w1|w2) . (z3|z1) = w1 z3 + w2 z1,    (w3|w1) . (z1|z2) = w3 z1 + w1 z2,    (w1|w2) . (z1|z2) = w1 z1 + w2 z2

The layout, stated once here and in the header: a lane's row block of a K = 16 kernel is the 32-byte string w1 w2 w3 w1 (eight
dwords, two bf16 each, even slot low), packed by frag_bf3k16 (epnn_api_weights.hip.h) as [2 row blocks][2 halves][64 lanes][4 dwords]
with the halves w1 w2 | w3 w1; the activation is a = z3 z1 (four dwords, W16K16::a) and z2 (two dwords), b = z1 z2 being put
together where it is used.  The packer sits inside the library's weight set-up and cannot be reached without a handle on a GPU;
tests/test_gpu_k16_pairs.py checks it through the charges."""
import math

import numpy as np


def _split3(x):
    """Truncating split of float32 values: three float32 arrays, each a bf16 number, adding up to x exactly."""
    x = np.asarray(x, dtype=np.float32)
    pieces = []
    for _ in range(3):
        top = (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
        pieces.append(top)
        x = x - top                      # exact: the remainder of a truncation is representable
    return pieces


def _dwords(piece):
    """A piece of a lane's four K slots as its two dwords: (slot 0, slot 1), (slot 2, slot 3), each slot tagged with its value."""
    return [(piece[0], piece[1]), (piece[2], piece[3])]


def _lane_strings(w, z):
    """The kernel's and the activation's registers of one lane (four K slots each), every dword tagged with its piece number."""
    w1, w2, w3 = _split3(w)
    z1, z2, z3 = _split3(z)
    tag = lambda k, piece: [(k, d) for d in _dwords(piece)]
    wstr = tag(1, w1) + tag(2, w2) + tag(3, w3) + tag(1, w1)          # w1 w2 | w3 w1: eight dwords
    za = tag(3, z3) + tag(1, z1)                                      # a = z3 z1
    zb = za[2:4] + tag(2, z2)                                         # b = a's upper half and z2
    return wstr, za, zb, (w1, w2, w3), (z1, z2, z3)


def _mfma_terms(a4, b4):
    """One lane's share of a K = 32 product: dword j of A meets dword j of B, low half with low half."""
    terms = []
    for (ka, da), (kb, db) in zip(a4, b4):
        for h in range(2):
            terms.append(((ka, kb), float(da[h]) * float(db[h])))
    return terms


def test_three_paired_products_are_the_six_partial_products():
    rng = np.random.default_rng(316)
    for _ in range(200):
        w = rng.uniform(-2.0, 2.0, size=4).astype(np.float32)
        z = rng.uniform(-1.0, 3.0, size=4).astype(np.float32)
        w.view(np.uint32)[...] |= 0x101                               # bits in the second and in the third piece of every value
        z.view(np.uint32)[...] |= 0x101
        wstr, za, zb, wp, zp = _lane_strings(w, z)
        assert all(np.all(p != 0) for p in wp + zp)
        assert all(float(a) + float(b) + float(c) == float(x) for a, b, c, x in zip(*wp, w))       # the split is exact
        # the three instructions as w16_mm_bfk16 indexes them: w[rb][0] = dwords 0..3, w[rb][1] = dwords 4..7
        terms = _mfma_terms(wstr[0:4], za) + _mfma_terms(wstr[4:8], zb) + _mfma_terms(wstr[0:4], zb)
        # every one of the six partial products once per K slot, and nothing else
        want = sorted([(1, 3), (2, 1), (3, 1), (1, 2), (1, 1), (2, 2)] * 4)
        assert sorted(t[0] for t in terms) == want
        # the same numbers as the six products formed one by one in float64 (bf16 x bf16 is exact there; fsum adds exactly)
        one_by_one = [float(wp[i - 1][s]) * float(zp[j - 1][s]) for (i, j) in [(1, 3), (2, 2), (3, 1), (1, 2), (2, 1), (1, 1)] for s in range(4)]
        assert math.fsum(t[1] for t in terms) == math.fsum(one_by_one)
        assert sorted(t[1] for t in terms) == sorted(one_by_one)
        # what is left out -- w2 z3, w3 z2, w3 z3 -- is small: a truncated piece keeps 8 significant bits, so |x2| < 2^-7 |x| and
        # |x3| < 2^-14 |x|, the three terms together below (2 x 2^-21 + 2^-28) < 2^-19 of |w z|
        full = math.fsum(float(a) * float(b) for a, b in zip(w, z))
        assert abs(math.fsum(one_by_one) - full) <= 2.0 ** -19 * math.fsum(abs(float(a) * float(b)) for a, b in zip(w, z))


def test_each_instruction_holds_its_two_products():
    """(w1|w2).(z3|z1), (w3|w1).(z1|z2), (w1|w2).(z1|z2): the small terms in the first two instructions, the largest in the last."""
    w = np.array([1.2345678, -0.3456789, 0.0123456, 1.9876543], dtype=np.float32)
    z = np.array([2.3456789, 0.4567891, -0.9876543, 0.1234567], dtype=np.float32)
    wstr, za, zb, _, _ = _lane_strings(w, z)
    per_instr = [_mfma_terms(wstr[0:4], za), _mfma_terms(wstr[4:8], zb), _mfma_terms(wstr[0:4], zb)]
    assert [sorted(set(t[0] for t in ts)) for ts in per_instr] == [[(1, 3), (2, 1)], [(1, 2), (3, 1)], [(1, 1), (2, 2)]]
