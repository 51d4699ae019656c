#!/usr/bin/env python3
"""The bits of the pair-list entries (charges_vjp_xyz at "grad_path" 2, with strain where there is a cell and there also without;
charges_vjp_xyz_multi at K = 1, 3 and 7, which runs sweep chunks 4 + 2 + 1; train_step_xyz at "train_path" 2 with apply=False;
charges_jvp_xyz, charges_jvp_xyz_multi at K = 1 and at K = 3, which runs sweep chunks 2 + 1) on the smallest systems that reach each
branch of their shared set-up (csrc/epnn_api_pairlist.hip.h):
    python tools/pairlist_bits.py record FILE      # on the build to compare against
    python tools/pairlist_bits.py compare FILE     # on the build under test: every array, hash and last_stats() must be equal
Random weights (random_weights(9, 2, ...)), fixed seeds, the generators of the GPU tests.  The bits belong to a build and a card:
FILE is not a fixture."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cell_ref  # noqa: E402
from conftest import random_weights  # noqa: E402
from epnn_amd.engine import Engine  # noqa: E402
from test_gpu_grad_large import _batch, _lattice_molecule  # noqa: E402
from test_gpu_train_cell import ZERO, _system, _tensor_slices  # noqa: E402

BOX = np.float32([13.0, 12.0, 12.5])


def systems():
    """name -> (molecules [(xyz, x, Q)], N, geometry keywords)"""
    far = _lattice_molecule(2, 9, seed=2)
    far[0][1] = far[0][0] + np.float32([50.0, 0.0, 0.0])                    # no listed pair: P1 = max(np, 1)
    return {"open4": ([_lattice_molecule(n, 9, seed=n) for n in (1, 17, 40, 97)], 100, {}),
            "far2": ([far], 4, {}),
            "open300": ([_lattice_molecule(300, 9, seed=300)], 320, {}),
            "box60": ([_system(60, 9, np.diag(BOX), seed=60)[:3]], 64, {"box": BOX}),
            "sheared60": ([_system(60, 9, cell_ref.SHEARED, seed=61)[:3]], 64, {"cell": cell_ref.SHEARED})}


def run():
    out = {}
    w = random_weights(9, 2, seed=5, scale=0.6)
    for k, (name, (mols, N, geo)) in enumerate(systems().items()):
        eng = Engine(nx=9, T=2)
        eng.set_weights(w)
        eng.set_option("grad_path", 2)
        eng.set_option("train_path", 2)
        eng.train_init()
        offsets, xyz, x, Q = _batch(mols)
        A, B = int(offsets[-1]), len(mols)
        rng = np.random.default_rng(1000 + k)
        g, y = rng.normal(size=A).astype(np.float32), rng.normal(scale=0.3, size=A).astype(np.float32)
        v = rng.normal(size=(A, 3)).astype(np.float32)
        E, dQ = (0.3 * rng.normal(size=(B, 3, 3))).astype(np.float32), rng.normal(size=B).astype(np.float32)

        def keep(tag, names, arrays):
            for nm, a in zip(names, arrays):
                out[f"{name}.{tag}.{nm}"] = np.asarray(a)
            out[f"{name}.{tag}.stats"] = eng.last_stats()

        strain = "cell" in geo
        keep("vjp", ("q", "gxyz", "gstrain"), eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, strain=strain, **geo))
        if strain:
            keep("vjp_nostrain", ("q", "gxyz"), eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, **geo))
        gk = np.concatenate([g[None], np.random.default_rng(4000 + k).normal(size=(6, A)).astype(np.float32)])
        for K in (1, 3, 7):
            keep(f"vjp_multi_K{K}", ("q", "gxyz", "gstrain"), eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, gk[:K], N, strain=strain, **geo))
        q, loss = eng.train_step_xyz(offsets, xyz, x, Q, y, N, apply=False, **(geo or {"cell": ZERO}))
        grad = eng.get_gradients()
        sums = np.array([grad[sl].astype(np.float64).sum() for sl in _tensor_slices(w)])
        sha = np.frombuffer(hashlib.sha256(grad.tobytes()).digest(), np.uint8)
        keep("train", ("q", "loss", "sha256", "sums") + (("grad",) if k == 0 else ()), (q, np.float32(loss), sha, sums, grad))
        tangents = {"all": dict(v=v, strain=E, dQ=dQ)}
        if strain:
            tangents.update(v=dict(v=v), strain=dict(strain=E), dQ=dict(dQ=dQ))
        for tag, tan in tangents.items():
            keep("jvp_" + tag, ("q", "tq"), eng.charges_jvp_xyz(offsets, xyz, x, Q, N, **tan, **geo))
        cols = [dict(v=v, strain=E, dQ=dQ)]                                 # the multi entry's columns: the tangent above, two more seeds
        for seed in (2000 + k, 3000 + k):
            r = np.random.default_rng(seed)
            cols.append(dict(v=r.normal(size=(A, 3)).astype(np.float32), strain=(0.3 * r.normal(size=(B, 3, 3))).astype(np.float32),
                             dQ=r.normal(size=B).astype(np.float32)))
        for K in (1, 3):
            tan = {nm: np.stack([c[nm] for c in cols[:K]]) for nm in ("v", "strain", "dQ")}
            keep(f"jvp_multi_K{K}", ("q", "tq"), eng.charges_jvp_xyz_multi(offsets, xyz, x, Q, N, **tan, **geo))
        eng.close()
    return out


def main():
    mode, path = sys.argv[1], sys.argv[2]
    got = run()
    if mode == "record":
        np.savez(path, **got)
        print(f"recorded {len(got)} arrays of {len(systems())} systems in {path}")
        return 0
    want = np.load(path)
    bad = [k for k in sorted(set(want.files) | set(got)) if k not in got or k not in want.files or
           want[k].dtype != got[k].dtype or not np.array_equal(want[k], got[k])]
    for k in bad:
        print("DIFFERENT", k, None if k not in want.files else want[k].ravel()[:4], None if k not in got else got[k].ravel()[:4])
    print(f"compared {len(got)} arrays against {path}: {len(bad)} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
