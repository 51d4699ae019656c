#!/usr/bin/env python3
"""Stores the blocked float64 reference (tests/grad_large_ref.py) of the charge gradients of a 4096-atom periodic box, so that
the GPU suite does not spend minutes of host time per run recomputing it.

NOT reference data: the arrays are produced by this repository's own float64 restatement on synthetic inputs with random
weights; they only cache a deterministic computation.  The fixture records a SHA-256 of the inputs (coordinates, features, box,
cotangent, every weight tensor); the test recomputes the inputs, compares the hash and runs the reference itself when it differs.

    python tests/golden/make_grad_large_fixtures.py          (a few minutes)
writes tests/golden/grad_large_box4096.npz: q, gxyz and the gradients with the ReLU-kink bracket kink_shift = +-2e-5.
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TAU = 2e-5
NAME = "grad_large_box4096.npz"


def box4096_case():
    """inputs of tests/test_gpu_grad_large.py::test_box_4096_against_the_blocked_reference"""
    from conftest import random_weights
    from epnn_amd import synth
    offsets, xyz, x, Q, N, box = synth.periodic_box_system(n_atoms=4096, seed=3)
    w = random_weights(9, 2, seed=23, scale=0.35)
    for t in range(2):                       # all-pairs sums over 4096 partners: |h| stays O(1), as in a trained model
        w["msg"][t][2] = (w["msg"][t][2][0] / 64.0, w["msg"][t][2][1] / 64.0)
    g = np.random.default_rng(9).normal(size=xyz.shape[0]).astype(np.float32)
    return xyz, x, Q, np.asarray(box, np.float32).reshape(3), g, w


def inputs_hash(xyz, x, Q, box, g, w):
    h = hashlib.sha256()
    for a in (xyz, x, np.asarray(Q, np.float32), box, g):
        h.update(np.ascontiguousarray(a).tobytes())
    for m in list(w["msg"]) + [w["upd"]] + list(w["pas"]):
        for W, b in m:
            h.update(np.ascontiguousarray(W).tobytes())
            h.update(np.ascontiguousarray(b).tobytes())
    return h.hexdigest()


def compute(xyz, x, Q, box, g, w):
    from grad_large_ref import vjp64_large
    g64 = g.astype(np.float64)
    q, ref = vjp64_large(xyz, x, Q[0], g64, w, box=box)
    lo = vjp64_large(xyz, x, Q[0], g64, w, box=box, kink_shift=+TAU)[1]
    hi = vjp64_large(xyz, x, Q[0], g64, w, box=box, kink_shift=-TAU)[1]
    return q, ref, lo, hi


def load(xyz, x, Q, box, g, w):
    """(q, gxyz, lo, hi) from the fixture if it was made from exactly these inputs, else None"""
    path = os.path.join(HERE, NAME)
    if not os.path.exists(path):
        return None
    z = np.load(path)
    if str(z["inputs_sha256"]) != inputs_hash(xyz, x, Q, box, g, w):
        return None
    return z["q"], z["gxyz"], z["gxyz_kink_plus"], z["gxyz_kink_minus"]


def main():
    case = box4096_case()
    q, ref, lo, hi = compute(*case)
    np.savez_compressed(os.path.join(HERE, NAME), q=q, gxyz=ref, gxyz_kink_plus=lo, gxyz_kink_minus=hi, inputs_sha256=inputs_hash(*case),
                        made_by="tests/golden/make_grad_large_fixtures.py: tests/grad_large_ref.vjp64_large (this repo's reference, not reference data)")
    print("box4096 done: max |gxyz|", np.abs(ref).max(), "kink", np.abs(lo - hi).max(), flush=True)


if __name__ == "__main__":
    main()
