#!/usr/bin/env python3
"""Charge gradients with respect to the coordinates (epnn_charges_vjp_xyz): ms per call and molecules per second on three
batches, each beside a train step without the optimizer (train_step_xyz(apply=0)) on the same batch:
  * one molecule of the recorded validation split padded to N = 41;
  * 8 molecules of the recorded validation split (N = 41);
  * 1024 QM9-like molecules at N = 29 (epnn_amd.synth).
Prints one line per batch and a JSON line with every figure."""
import json
import os
import sys
import tarfile
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epnn_amd import checkpoint, synth  # noqa: E402
from epnn_amd.engine import Engine  # noqa: E402
from oracle import epnn_oracle as orc  # noqa: E402  (xyz parser only)


def val_batch(k):
    d = tempfile.mkdtemp()
    with tarfile.open(os.path.join(ROOT, "tests", "golden", "mixed_val.tar.gz")) as tf:
        tf.extractall(d)
    names = [str(n) for n in np.load(os.path.join(ROOT, "tests", "golden", "val_names.npy"), allow_pickle=True)][:k]
    mols = [orc.parse_xyz(os.path.join(d, "mixed_val", nm + ".xyz"), 10) for nm in names]
    off = np.zeros(k + 1, np.int32)
    off[1:] = np.cumsum([m[1].shape[0] for m in mols])
    return off, np.concatenate([m[0] for m in mols]), np.concatenate([m[1] for m in mols]), np.array([m[2] for m in mols], np.float32)


def timed(fn, reps):
    for _ in range(3):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def main():
    w10 = checkpoint.load_epnn_weights(os.path.join(ROOT, "models", "model_weights"))
    w9 = checkpoint.load_epnn_weights(os.path.join(ROOT, "models", "decay_model_weights"))
    o, xyz, x, Q, _ = synth.qm9_like_batch(1024, seed=0, N=29)
    cases = [("1 validation molecule, N=41", val_batch(1), 41, w10, 10, 50),
             ("8 validation molecules, N=41", val_batch(8), 41, w10, 10, 30),
             ("1024 QM9-like molecules, N=29", (o, xyz, x, Q), 29, w9, 9, 5)]
    out = {}
    for label, (off, xyz, x, Q), N, w, nx, reps in cases:
        eng = Engine(nx=nx, T=len(w["msg"]))
        eng.set_weights(w)
        B, A = len(off) - 1, int(off[-1])
        g = np.random.default_rng(0).normal(size=A).astype(np.float32)
        y = np.zeros(A, np.float32)
        t_vjp = timed(lambda: eng.charges_vjp_xyz(off, xyz, x, Q, g, N), reps)
        eng.train_init()
        eng.set_option("train_async", 0)                        # (a step that returns when all of it is done)

        def step():
            eng.train_step_xyz(off, xyz, x, Q, y, N, apply=False)
            eng.sync()
        t_step = timed(step, reps)
        eng.close()
        print(f"{label}: charges_vjp_xyz {t_vjp * 1e3:.3f} ms ({B / t_vjp:.0f} molecules/s); "
              f"train_step_xyz(apply=0) {t_step * 1e3:.3f} ms ({B / t_step:.0f} molecules/s); ratio {t_vjp / t_step:.2f}", flush=True)
        out[label] = {"vjp_ms": t_vjp * 1e3, "vjp_molecules_per_s": B / t_vjp, "train_step_apply0_ms": t_step * 1e3,
                      "train_step_apply0_molecules_per_s": B / t_step}
    print(json.dumps({"metric": "charges_vjp_xyz vs train_step_xyz(apply=0)", "cases": out}))


if __name__ == "__main__":
    main()
