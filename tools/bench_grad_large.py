#!/usr/bin/env python3
"""Charge gradients from the pair list ("grad_path" = 2) beside the forward of the same system:
  * the 2220-atom protein (open), with the dense path ("grad_path" = 1) on the same handle beside it;
  * 10 000- and 100 000-atom cells: synth.periodic_box_system as an open cluster and with box=, synth.triclinic_cell_system with
    cell= and strain=True.
    python tools/bench_grad_large.py [--sizes 2220,10000,100000] [--no-dense] [--crossover]
--crossover instead times both paths on single open systems of 32 .. 1024 atoms (synth.box_system) and on the 1024-molecule
QM9-sized batch at N = 29: where the pair-list path overtakes the dense path.
Times are wall clock per blocking host call (uploads and downloads included) after one warm-up call; the device scratch of a
gradient call is what the library reports (epnn_last_stats()[2]) beside the formula

    bytes = A (4 (T + 1) 48 + 4 T 32 + 4 (T + 1) + 5 * 128 + 2 * 192 + 48 + 20 + 72) + A pieces (2 * 128 + 1)   per atom
          + P (2 * 48 * 4 + 9 * 4 + 32 + 2 (2 * 128 + 4 + 72))                                           per listed pair

(h_t, S_t, q_t checkpoints; P, R, Yb, Yc, dS rows; gh twice; strain shares, outputs, inputs and the front-end's counts; the
partner-range pieces of dP and dR and their tasks; pieces = 1 from 32 768 atoms on, at most 16 --
pe and gE rows, pair records and incidence links; per incidence slot two 32-float rows, a transfer and nine float64)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epnn_amd import charge_gn, checkpoint, synth  # noqa: E402
from epnn_amd.engine import Engine  # noqa: E402


def pieces(n):
    tiles = (n + 15) // 16
    return min(16, max(1, (2048 + tiles - 1) // tiles))


def scratch_formula(A, P, T, n):
    per_atom = 4 * (T + 1) * 48 + 4 * T * 32 + 4 * (T + 1) + 5 * 128 + 2 * 192 + 48 + 20 + 72 + pieces(n) * (2 * 128 + 1)
    per_pair = 2 * 48 * 4 + 9 * 4 + 32 + 2 * (2 * 128 + 4 + 72)
    return A * per_atom + max(P, 1) * per_pair


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def crossover(eng):
    cases = [(f"{n} atoms, open", synth.box_system(n_atoms=n, seed=0)) for n in (32, 64, 128, 256, 512, 1024)]
    cases.append(("1024 QM9-sized molecules, N = 29", synth.qm9_like_batch(1024, seed=0, N=29)))
    for name, (offsets, xyz, x, Q, N) in cases:
        A = int(offsets[-1])
        g = np.random.default_rng(0).normal(size=A).astype(np.float32)
        line = {"workload": name, "atoms": A, "B_N2": (len(offsets) - 1) * int(N) ** 2}
        for path, key in ((1, "dense_path_ms"), (2, "pair_list_ms")):
            eng.set_option("grad_path", path)
            t, _ = timed(lambda: eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N), 10)
            line[key] = round(t * 1e3, 3)
        eng.set_option("grad_path", 0)
        print(json.dumps(line), flush=True)


def main():
    sizes = [2220, 10_000, 100_000]
    if "--sizes" in sys.argv:
        sizes = [int(s) for s in sys.argv[sys.argv.index("--sizes") + 1].split(",")]
    dense = "--no-dense" not in sys.argv
    w = checkpoint.load_epnn_weights(os.path.join(ROOT, "models/decay_model_weights"))
    T = len(w["msg"])
    eng = Engine(nx=9, T=T)
    eng.set_weights(w)
    rows = []
    if "--crossover" in sys.argv:
        crossover(eng)
        eng.close()
        return
    for n in sizes:
        cases = []
        if n == 2220:
            xyz, x, Q, _ = charge_gn.read_xyz(os.path.join(ROOT, "tests/golden/protein/6qlp_capped.xyz"), 9)
            cases.append(("protein 6qlp_capped, open", np.array([0, len(x)], np.int32), xyz, x, np.array([Q], np.float32), len(x), {}))
        else:
            t0 = time.time()
            offsets, xyz, x, Q, N, box = synth.periodic_box_system(n, seed=0)
            co, cxyz, cx, cQ, cN, cell = synth.triclinic_cell_system(n, seed=0)
            print(f"# generated the {n}-atom cells in {time.time() - t0:.1f} s", flush=True)
            cases.append((f"{n} atoms, open cluster", offsets, xyz, x, Q, N, {}))
            cases.append((f"{n} atoms, box=", offsets, xyz, x, Q, N, {"box": np.asarray(box, np.float32).reshape(3)}))
            cases.append((f"{n} atoms, sheared cell=, strain=True", co, cxyz, cx, cQ, cN,
                          {"cell": np.asarray(cell, np.float32).reshape(3, 3), "strain": True}))
        for name, offsets, xyz, x, Q, N, geo in cases:
            A = int(offsets[-1])
            g = np.random.default_rng(0).normal(size=A).astype(np.float32)
            fgeo = {k: v for k, v in geo.items() if k != "strain"}
            reps = 20 if A <= 4096 else (3 if A <= 20_000 else 1)
            t_fwd, q_fwd = timed(lambda: eng.forward_xyz(offsets, xyz, x, Q, N, **fgeo), max(reps, 3))
            eng.set_option("grad_path", 2)
            t_grad, out = timed(lambda: eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, **geo), reps)
            st = eng.last_stats()
            line = {"workload": name, "atoms": A, "near_pairs": int(st[0]), "forward_ms": round(t_fwd * 1e3, 3),
                    "gradient_ms": round(t_grad * 1e3, 3), "gradient_over_forward": round(t_grad / t_fwd, 2),
                    "scratch_bytes": int(st[2]), "scratch_formula_bytes": scratch_formula(A, int(st[0]), T, A),
                    "q_vs_forward": float(np.abs(out[0] - q_fwd).max()), "max_abs_gxyz": float(np.abs(out[1]).max())}
            if dense and A <= 2220:
                eng.set_option("grad_path", 1)
                t_dense, out_d = timed(lambda: eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, **geo), 5)
                line["dense_path_ms"] = round(t_dense * 1e3, 3)
                line["dense_vs_pair_list_gxyz"] = float(np.abs(out_d[1] - out[1]).max())
                line["dense_path_gE_bytes"] = 2 * A * A * 48 * 4
            eng.set_option("grad_path", 0)
            rows.append(line)
            print(json.dumps(line), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
