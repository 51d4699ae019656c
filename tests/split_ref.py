"""NumPy model of the inference kernels' Dense arithmetic -- TEST INFRASTRUCTURE.

A float32-grade Dense of the kernels splits both operands exactly into three bf16 pieces, x = x1 + x2 + x3 with each piece the upper 16
bits of what is left, and sums the six partial products x_a w_b with a + b <= 4 of the nine.  Here the chosen partial products are
summed in float64, so a model shows only what it leaves out: SIX is the design, TWO_PIECES the two-piece form (x1 w1 + x1 w2 + x2 w1)
and DROP_ONE the six ways of losing one partial product of the design.  `swapped_mlp` runs the float64 oracle with such a Dense in
place of its own; tests/test_split_ref.py holds the models' errors against the float32 oracle's noise, which is what lets
tests/test_gpu_f32_grade.py bind the device to that noise."""
import contextlib

import numpy as np

SIX = tuple((a, b) for a in (1, 2, 3) for b in (1, 2, 3) if a + b <= 4)
TWO_PIECES = ((1, 1), (1, 2), (2, 1))
DROP_ONE = {f"six without x{a}w{b}": tuple(p for p in SIX if p != (a, b)) for a, b in SIX}
DEFECTS = dict({"two pieces": TWO_PIECES}, **DROP_ONE)


def pieces(a, k=3):
    """The truncation split of float32 values: k float32 arrays, each the upper 16 bits (a bf16 number) of what the ones before it
    leave of `a`.  The remainders are exact float32 subtractions while the last piece is a normal number (|a| >= 2^-100 for k = 3)."""
    rest = np.array(a, dtype=np.float32)
    out = []
    for _ in range(k):
        top = (rest.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
        out.append(top)
        rest = rest - top
    return out


def split_dense(rows, W, b, keep=SIX):
    """rows @ W + b with both operands rounded to float32 and split: the float64 sum of the partial products x_a w_b, (a, b) in keep.
    (One product per piece of W, with the sum of its partners among the pieces of rows.)"""
    xs, ws = pieces(rows, max(a for a, _ in keep)), pieces(W)
    acc = np.asarray(b, dtype=np.float64)
    for c in (3, 2, 1):                                                 # (smallest terms first, like the kernels)
        partners = [xs[a - 1] for a, cc in keep if cc == c]
        if partners:
            x = partners[0]
            for p in partners[1:]:
                x = x + p                 # (float32, exact: pieces of one value share its 24 bits)
            acc = x.astype(np.float64) @ ws[c - 1].astype(np.float64) + acc
    return acc


@contextlib.contextmanager
def swapped_mlp(keep=SIX, layer=None):
    """While it runs, oracle.epnn_oracle.mlp (which gnn_layer and epn_layer look up in their module) computes its Dense layers with
    split_dense(..., keep): every layer, or the one of index `layer` alone (1: the second Dense, all that the tiled path splits) with
    the others as they are.  For the oracle's float64 runs."""
    from oracle import epnn_oracle as orc
    keep = tuple(keep)

    def mlp(rows, layers, activation="relu"):
        act = orc._activation(activation)
        for l, (W, b) in enumerate(layers):
            rows = split_dense(rows, W, b, keep) if layer is None or l == layer else rows @ W + b
            if l + 1 < len(layers):
                rows = act(rows)
        return rows

    saved = orc.mlp
    orc.mlp = mlp
    try:
        yield
    finally:
        orc.mlp = saved
