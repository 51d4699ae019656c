#!/usr/bin/env python3
"""The bits of the entries that take a geometry and that tools/pairlist_bits.py does not reach (forward_xyz, forward_xyz_dev, edges_ex,
charges_vjp_xyz at "grad_path" 1, train_step_xyz with apply=False at "train_path" 1, coulomb_xyz), each as open molecules, in a box and
in a sheared cell, on the smallest molecules that take the fused, the multi-wave and the tiled route:
    python tools/geometry_bits.py record FILE      # on the build to compare against
    python tools/geometry_bits.py compare FILE     # on the build under test: every array, hash and last_stats() must be equal
Random weights (random_weights(9, 2, ...)), fixed seeds, T = 2.  The bits belong to a build and a card: FILE is not a fixture."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cell_ref  # noqa: E402
from conftest import random_weights  # noqa: E402
from epnn_amd.engine import Engine  # noqa: E402
from test_gpu_train_cell import _system  # noqa: E402

BOX = np.float32([13.0, 12.0, 12.5])
N = 100
GEOMETRIES = {"open": {}, "box": {"box": BOX}, "sheared": {"cell": cell_ref.SHEARED}}


def run():
    out = {}
    w = random_weights(9, 2, seed=5, scale=0.6)
    for n in (9, 40, 97):                                                  # fused, multi-wave, tiled
        xyz, x, Q, y = _system(n, 9, cell_ref.SHEARED, seed=n)             # the same atoms in every geometry
        offsets, Q = np.int32([0, n]), np.float32([Q])
        g = np.random.default_rng(100 + n).normal(size=n).astype(np.float32)
        for gname, geo in GEOMETRIES.items():
            eng = Engine(nx=9, T=2)
            eng.set_weights(w)
            eng.set_option("grad_path", 1)
            eng.set_option("train_path", 1)
            eng.train_init()

            def keep(tag, names, arrays):
                for nm, a in zip(names, arrays):
                    out[f"n{n}.{gname}.{tag}.{nm}"] = np.asarray(a)
                out[f"n{n}.{gname}.{tag}.stats"] = eng.last_stats()

            keep("forward", ("q",), (eng.forward_xyz(offsets, xyz, x, Q, N, **geo),))
            dev = [eng.to_device(a) for a in (xyz, x, Q)] + [eng.alloc(n * 4)]
            for rep in range(2):                                           # the second call finds the first one pending
                eng.forward_xyz_dev(offsets, *dev, N, **geo)
            eng.sync()
            keep("forward_dev", ("q",), (dev[3].download((n,)),))
            for d in dev:
                d.free()
            if n == 9:
                keep("edges_ex", ("e", "c"), eng.edges_ex(xyz, 48, **geo))
            strain = "box" not in geo
            keep("vjp", ("q", "gxyz", "gstrain"), eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, strain=strain, **geo))
            for inline in (1, 0) if not geo else (() if "box" in geo else (1,)):
                eng.set_option("train_inline", inline)
                q, loss = eng.train_step_xyz(offsets, xyz, x, Q, y, N, apply=False, **geo)
                sha = np.frombuffer(hashlib.sha256(eng.get_gradients().tobytes()).digest(), np.uint8)
                keep(f"train_inline{inline}", ("q", "loss", "sha256"), (q, np.float32(loss), sha))
            if not geo:
                keep("coulomb", ("q", "phi", "E", "F", "ffix", "fq"), eng.coulomb_xyz(offsets, xyz, x, Q, N, parts=True))
            eng.close()
    return out


def main():
    mode, path = sys.argv[1], sys.argv[2]
    got = run()
    if mode == "record":
        np.savez(path, **got)
        print(f"recorded {len(got)} arrays in {path}")
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
