#!/usr/bin/env python3
"""Stores the blocked float64 reference (tests/train_large_ref.py) of the training step's loss, charges and weight gradients for a
600-atom open cluster and a 600-atom sheared cell, so that the GPU suite does not recompute it on every run.

NOT reference data: the arrays are produced by this repository's own float64 restatement on synthetic inputs with random weights;
they only cache a deterministic computation.  Each fixture records a SHA-256 of its inputs (coordinates, features, cell, labels,
every weight tensor); the test recomputes the inputs, compares the hash and runs the reference itself when it differs.

    python tests/golden/make_train_large_fixtures.py          (about a minute)
writes tests/golden/train_large_cluster600.npz and train_large_cell600.npz: loss, q, the flat gradient (trainable_variables order,
float64) and the width of its ReLU-kink bracket kink_shift = +-2e-6 (float32).
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TAU = 2e-6
N_ATOMS = 600


def case(kind):
    """inputs of tests/test_gpu_train_cell.py::test_600_atoms_against_the_fixture: (xyz, x, Q, cell or None, y, w)"""
    from conftest import random_weights
    from epnn_amd import synth
    rng = np.random.default_rng(600 + (kind == "cell"))
    if kind == "cell":                                       # a sheared cell at 0.1 atoms per A^3: widths of 15 A and more
        _, xyz, x, _, _, cell = synth.triclinic_cell_system(n_atoms=N_ATOMS, seed=6)
        cell = np.asarray(cell, np.float32).reshape(3, 3)
    else:
        cell = None
        k = int(np.ceil(N_ATOMS ** (1 / 3)))
        grid = np.array([(a, b, c) for a in range(k) for b in range(k) for c in range(k)], dtype=np.float64)[:N_ATOMS] * 1.3
        xyz = (grid + rng.uniform(-0.2, 0.2, grid.shape)).astype(np.float32)
        x = np.zeros((N_ATOMS, 9), dtype=np.float32)
        el = rng.integers(0, 8, N_ATOMS)
        x[np.arange(N_ATOMS), 1 + el] = 1.0
        x[:, 0] = np.array([1, 6, 7, 8, 9, 15, 16, 17, 35])[el % 9]
    Q = np.float32(rng.integers(-1, 2))
    xyz, x = np.ascontiguousarray(xyz, np.float32), np.ascontiguousarray(x, np.float32)
    y = rng.normal(scale=0.3, size=N_ATOMS).astype(np.float32)
    w = random_weights(9, 2, seed=31, scale=0.4)
    for t in range(2):                       # all-pairs sums over 600 partners: |h| stays O(1), as in a trained model
        w["msg"][t][2] = (w["msg"][t][2][0] / 16.0, w["msg"][t][2][1] / 16.0)
    return xyz, x, Q, cell, y, w


def inputs_hash(xyz, x, Q, cell, y, w):
    h = hashlib.sha256()
    for a in (xyz, x, np.asarray(Q, np.float32), np.zeros((3, 3), np.float32) if cell is None else cell, y):
        h.update(np.ascontiguousarray(a).tobytes())
    for m in list(w["msg"]) + [w["upd"]] + list(w["pas"]):
        for W, b in m:
            h.update(np.ascontiguousarray(W).tobytes())
            h.update(np.ascontiguousarray(b).tobytes())
    return h.hexdigest()


def compute(xyz, x, Q, cell, y, w):
    from oracle import epnn_oracle_train as ot
    from train_large_ref import loss_and_grads_large
    loss, q, g = loss_and_grads_large(xyz, x, Q, y, w, cell=cell)
    lo = ot.flatten(loss_and_grads_large(xyz, x, Q, y, w, cell=cell, kink_shift=+TAU)[2])
    hi = ot.flatten(loss_and_grads_large(xyz, x, Q, y, w, cell=cell, kink_shift=-TAU)[2])
    return loss, q, ot.flatten(g), np.abs(lo - hi).astype(np.float32)


def _path(kind):
    return os.path.join(HERE, f"train_large_{'cell' if kind == 'cell' else 'cluster'}600.npz")


def load(kind, inputs):
    """(loss, q, grad, band) from the fixture if it was made from exactly these inputs, else None"""
    if not os.path.exists(_path(kind)):
        return None
    z = np.load(_path(kind))
    if str(z["inputs_sha256"]) != inputs_hash(*inputs):
        return None
    return float(z["loss"]), z["q"], z["grad"], z["band"]


def main():
    for kind in ("cluster", "cell"):
        inputs = case(kind)
        loss, q, grad, band = compute(*inputs)
        np.savez_compressed(_path(kind), loss=loss, q=q, grad=grad, band=band, inputs_sha256=inputs_hash(*inputs),
                            made_by="tests/golden/make_train_large_fixtures.py: tests/train_large_ref.loss_and_grads_large (this repo's reference, not reference data)")
        print(kind, "done: loss", loss, "max |grad|", np.abs(grad).max(), "kink band", band.max(), os.path.getsize(_path(kind)), "bytes", flush=True)


if __name__ == "__main__":
    main()
