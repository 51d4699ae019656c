"""The scaled packs of the fused kernel's clamp form (pack_weights, epnn_api_weights.hip.h; k_wave_forward<.., CLAMP>), without a GPU.

The clamp form takes relu(a + b) as the add's output clamp, min(max(a + b, 0), 1), so it runs every pair MLP on operands scaled by
s = 2^-EPNN_RELU_SHIFT and the one linear map behind the pair MLP scaled by 1 / s.  That gives the unscaled kernel's bits only if
scaling commutes with the three-piece split: the pieces of s W must be s times the pieces of W -- the same sign and mantissa bits,
the exponent field moved by the shift -- with every piece still a normal float32.  Checked here on the reference's weights, for the
matrices the host scales, built the way it builds them (float64 products rounded to float32, then scaled, then split)."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from split_ref import pieces

NX, EDIM = 9, 48


def _shift():
    text = open(os.path.join(ROOT, "epnn_amd", "csrc", "epnn_common.h")).read()
    return int(re.search(r"#define EPNN_RELU_SHIFT (\d+)", text).group(1))


def _weights():
    from epnn_amd import checkpoint
    return checkpoint.load_epnn_weights(os.path.join(ROOT, "models", "decay_model_weights"))


def _matrices():
    """name -> (float32 array, +1: packed times s | -1: packed times 1 / s)."""
    w = _weights()
    T = len(w["msg"])
    F = NX + EDIM + 1
    Wu1, Wu3 = (np.asarray(w["upd"][k][0], dtype=np.float64) for k in (0, 2))
    bu3 = np.asarray(w["upd"][2][1], dtype=np.float64)
    out = {}
    for kind in ("msg", "pas"):
        for t in range(T):
            W1, b1 = (np.asarray(a, dtype=np.float32) for a in w[kind][t][0])
            assert W1.shape == (2 * F + EDIM, 32)
            out[f"{kind}{t}.W1"] = (W1, +1)                                   # the x, q and edge rows as they are (we16b: through the edge basis)
            out[f"{kind}{t}.b1"] = (b1, +1)
            out[f"{kind}{t}.b2"] = (np.asarray(w[kind][t][1][1], dtype=np.float32), +1)
            for side in (0, 1):                                              # h rows folded with Wu3, bu3 (float64, then float32)
                Wh = W1[side * F + NX: side * F + NX + EDIM].astype(np.float64)
                out[f"{kind}{t}.fold{side}"] = ((Wu3 @ Wh).astype(np.float32), +1)
                out[f"{kind}{t}.cb{side}"] = ((bu3 @ Wh).astype(np.float32), +1)
        # what takes the pair MLP's summed output
    for t in range(T):
        W3 = np.asarray(w["msg"][t][2][0], dtype=np.float64)
        out[f"msg{t}.u1s"] = ((W3 @ Wu1[EDIM:EDIM + 32]).astype(np.float32), -1)
        out[f"pas{t}.w3"] = (np.asarray(w["pas"][t][2][0], dtype=np.float32).reshape(-1), -1)
    return out


def test_shift_leaves_both_ends_of_float32():
    k = _shift()
    # the clamp's range ends at 2^(k - 1) of an unscaled row; the third piece of a scaled operand (2^-24 of it) stays normal down to
    # 2^(-126 + 24 + k); 1 / s packs times weights of up to 2^10 stay far below float32's largest number
    assert 24 <= k <= 48
    assert 2.0 ** (k - 1) >= 1e6 and 2.0 ** (-126 + 24 + k) <= 1e-15 and 2.0 ** (k + 10) < 1e30


@pytest.mark.parametrize("sign", (+1, -1))
def test_pieces_of_scaled_weights_are_the_pieces_with_shifted_exponents(sign):
    k = _shift()
    s = np.float32(2.0) ** np.float32(-k * sign)
    checked = 0
    for name, (W, how) in _matrices().items():
        if how != sign:
            continue
        W = np.ascontiguousarray(W, dtype=np.float32)
        scaled = W * s                                                       # float32 product, as the host's
        assert np.array_equal(scaled.astype(np.float64), W.astype(np.float64) * float(s)), name      # exact: nothing rounded, nothing flushed
        for level, (p, ps) in enumerate(zip(pieces(W), pieces(scaled))):
            assert np.array_equal(ps, p * s), (name, level)
            bits, sbits = p.view(np.uint32), ps.view(np.uint32)
            nz = p != 0
            assert np.array_equal(sbits[nz] & np.uint32(0x807FFFFF), bits[nz] & np.uint32(0x807FFFFF)), (name, level)     # sign, mantissa
            e, es = (bits[nz] >> 23) & 0xFF, (sbits[nz] >> 23) & 0xFF
            assert np.array_equal(es.astype(np.int64), e.astype(np.int64) - k * sign), (name, level)
            assert (es >= 1).all() and (es <= 254).all(), (name, level)      # normal numbers
            assert not (sbits & np.uint32(0xFFFF)).any(), (name, level)      # still bf16 numbers
            checked += int(nz.sum())
        rest = W.astype(np.float64) - sum(p.astype(np.float64) for p in pieces(W))
        rest_s = scaled.astype(np.float64) - sum(p.astype(np.float64) for p in pieces(scaled))
        assert np.array_equal(rest_s, rest * float(s)), name                 # what the three pieces leave out scales too
    print(f"RELU_CLAMP packs x 2^{-k * sign}: {checked} non-zero pieces checked")
    assert checked > 1000
