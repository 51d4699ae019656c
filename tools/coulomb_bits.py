#!/usr/bin/env python3
"""The bits of the six electrostatics entries (coulomb_xyz, coulomb_xyz_cell and their _excl forms, coulomb_xyz_slab and
coulomb_xyz_slab_strain; parts=True, in cells strain=True) on the smallest batches that reach every branch of their one driver and of the
sweeps (csrc/epnn_api_coulomb_run.hip.h, csrc/epnn_coulomb.hip.h):
    python tools/coulomb_bits.py record FILE      # on the build to compare against
    python tools/coulomb_bits.py compare FILE     # on the build under test: every array and last_stats() must be equal
  * open: one batch of molecules of 1, 2, 17, 40, 64, 65 and 300 atoms (1 .. 64 pack several to a wavefront, 65 is the first size cut
    into blocks, 300 is 5 blocks times 3 pieces);
  * cells: one batch of cell_ref.SHEARED scaled by 1, 1, 1.5 and 1.9 around 2, 17, 65 and 130 atoms (the k box of the rule depends on
    the cell's shape alone, 23 x 23 x 11 slots at every scale), and one cubic box of 9 A handed over as box=;
  * slabs, on the cells and generators of tests/test_gpu_coulomb_slab.py: slabpack, its BATCH (20, 1, 9 and 30 atoms in sq65, tilted,
    openy and sq14: one wavefront, three different open rows, each cell with its own slots); slabcut, tilted with 65 atoms (cut into
    blocks) and sq14 with 129 (pieces of the partner range: cpieces > 1, a cell spans tasks); slabbox, 40 atoms in a slab of 9 A open
    along y, handed over as box= with one zero;
  * alpha 0, 0.5 and 2.0 on each.  At 0.5 the rule caps beta at alpha in every cell here (w_min <= 14 A < 2 sqrt(-ln 1e-6) / 0.5
    = 14.9 A), so rc = 0 and the sweep is skipped: run() asserts it, and that rc > 0 at the other two;
  * open and cells: every geometry plain, with an empty list, and with the list of coulomb_excl_ref.exclusion_cases, about two pairs per
    atom at factors 0, 0.5 and 0.8333, shuffled with half of the rows swapped; the open batch also with all 136 pairs of its 17-atom
    molecule at factor 0 (in a cell most of those pairs lie beyond half the smallest width and the list is refused by name);
  * slabs: both entries without a list and with that shuffled list (every listed pair lies within 0.95 of half the smaller width).
Random weights (random_weights(9, 2, ...)), fixed seeds, T = 2, the generators of the GPU tests.  The bits belong to a build and a card:
FILE is not a fixture."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import cell_ref  # noqa: E402
from conftest import random_weights  # noqa: E402
from coulomb_excl_ref import exclusion_cases, shuffled  # noqa: E402
from epnn_amd.engine import Engine  # noqa: E402
import test_gpu_coulomb_slab as slab  # noqa: E402
from test_gpu_grad_large import _batch, _features, _lattice_molecule  # noqa: E402
from test_gpu_train_cell import _system  # noqa: E402

ALPHAS = (0.0, 0.5, 2.0)
NAMES = ("q", "phi", "E", "F", "gstrain", "ffix", "fq", "gstrain_fix", "gstrain_q")
OPEN_NAMES = tuple(n for n in NAMES if "gstrain" not in n)


def systems():
    """name -> (molecules [(xyz, x, Q)], N, cells (B, 3, 3) or None, geometry keywords, near: the list rule's distance, slab or not)"""
    cells = np.stack([cell_ref.SHEARED * np.float32(s) for s in (1.0, 1.0, 1.5, 1.9)])
    cube = np.diag(np.float32([9.0, 9.0, 9.0]))
    out = {"open": ([_lattice_molecule(n, 9, seed=n) for n in (1, 2, 17, 40, 64, 65, 300)], 320, None, {}, 1.3, False),
           "sheared": ([_system(n, 9, c, seed=n)[:3] for n, c in zip((2, 17, 65, 130), cells)], 160, cells, {"cell": cells}, 2.6, False),
           "cube": ([_system(40, 9, cube, seed=41)[:3]], 64, cube[None], {"box": np.float32([9.0, 9.0, 9.0])}, 2.6, False)}
    for name, members, N in (("slabpack", slab.BATCH, 32), ("slabcut", [("tilted", 65), ("sq14", 129)], 136)):
        mols = [slab._system(c, n, 700 + n) for c, n in members]
        cells = np.stack([m[3] for m in mols])
        out[name] = (mols, N, cells, {"cell": cells}, 2.0, True)
    rng = np.random.default_rng(43)
    box = np.float32([9.0, 0.0, 9.0])
    x, Q = _features(rng, 40, 9)
    out["slabbox"] = ([(slab._place(rng, 40, np.diag(box), 5.0), x, Q, np.diag(box))], 40, np.diag(box)[None], {"box": box}, 2.0, True)
    return out


def lists(mols, offsets, cells, near, is_slab):
    """name -> (pairs, scale) in flat atom indices, or None for the plain entry (a slab entry then takes an empty list)"""
    per = [exclusion_cases(m[0], None if cells is None else cells[b], near=near) for b, m in enumerate(mols)]
    pairs = np.concatenate([p + offsets[b] for b, (p, _) in enumerate(per)])
    out = {"plain": None, "empty": (np.zeros((0, 2), np.int32), np.zeros((0,), np.float32)),
           "near": shuffled(pairs, np.concatenate([s for _, s in per]))}
    if is_slab:
        del out["empty"]
    if cells is None:
        b = [m[0].shape[0] for m in mols].index(17)
        i, j = np.triu_indices(17, 1)
        out["all17"] = (np.stack([i, j], 1).astype(np.int32) + offsets[b], np.float32(0.0))
    return out


def run():
    out = {}
    w = random_weights(9, 2, seed=5, scale=0.6)
    for name, (mols, N, cells, geo, near, is_slab) in systems().items():
        eng = Engine(nx=9, T=2)
        eng.set_weights(w)
        offsets, xyz, x, Q = slab._batch(mols)[0] if is_slab else _batch(mols)
        for alpha in ALPHAS:
            if cells is not None:
                for c in cells:
                    rule = eng.ewald_slab_params if is_slab else eng.ewald_params
                    assert (rule(c, alpha)[1] == 0.0) == (alpha == 0.5), (name, alpha)
            for lname, ex in lists(mols, offsets, cells, near, is_slab).items():
                if cells is None:
                    got = {"": eng.coulomb_xyz_excl(offsets, xyz, x, Q, N, alpha=alpha, parts=True, exclusions=ex)}
                elif is_slab:
                    got = {"": eng.coulomb_xyz_slab(offsets, xyz, x, Q, N, alpha=alpha, parts=True, exclusions=ex, **geo)}
                    stats = np.asarray(eng.last_stats())
                    got[".strain"] = eng.coulomb_xyz_slab_strain(offsets, xyz, x, Q, N, alpha=alpha, parts=True, exclusions=ex, **geo)
                    out[f"{name}.alpha{alpha}.{lname}.plainstats"] = stats
                else:
                    got = {"": eng.coulomb_xyz_cell_excl(offsets, xyz, x, Q, N, alpha=alpha, parts=True, strain=True, exclusions=ex, **geo)}
                tag = f"{name}.alpha{alpha}.{lname}"
                for entry, arrays in got.items():
                    for nm, a in zip(OPEN_NAMES if len(arrays) == len(OPEN_NAMES) else NAMES, arrays):
                        out[f"{tag}{entry}.{nm}"] = np.asarray(a)
                out[f"{tag}.stats"] = np.asarray(eng.last_stats())
                if ex is not None:
                    out[f"{tag}.pairs"] = np.asarray(ex[0])
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
