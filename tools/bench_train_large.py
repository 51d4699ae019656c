#!/usr/bin/env python3
"""Training steps from the pair list ("train_path" = 2, apply = 0) beside the charge gradients ("grad_path" = 2) of the same system:
  * the 2220-atom protein (open), with the dense layer-by-layer step ("train_path" = 1) on the same handle beside it;
  * 10 000- and 100 000-atom systems: synth.periodic_box_system as an open cluster and with box=, synth.triclinic_cell_system
    with cell=.
    python tools/bench_train_large.py [--sizes 2220,10000,100000] [--no-dense]
Times are wall clock per blocking host call (uploads and downloads included) after one warm-up call.  step_over_gradient is the
ratio the issue of this path asks for: the weight gradients add the MFMAs of half a backward sweep plus the per-atom and per-pair
outer products, so a step should stay near twice the gradient call.  The device scratch is what the library reports
(epnn_last_stats()[2]); labels are random (the time does not depend on them)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epnn_amd import charge_gn, checkpoint, synth  # noqa: E402
from epnn_amd.engine import Engine  # noqa: E402


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def main():
    sizes = [2220, 10_000, 100_000]
    if "--sizes" in sys.argv:
        sizes = [int(s) for s in sys.argv[sys.argv.index("--sizes") + 1].split(",")]
    dense = "--no-dense" not in sys.argv
    w = checkpoint.load_epnn_weights(os.path.join(ROOT, "models/decay_model_weights"))
    eng = Engine(nx=9, T=len(w["msg"]))
    eng.set_weights(w)
    eng.train_init()
    zero = np.zeros((3, 3), np.float32)
    for n in sizes:
        cases = []
        if n == 2220:
            xyz, x, Q, _ = charge_gn.read_xyz(os.path.join(ROOT, "tests/golden/protein/6qlp_capped.xyz"), 9)
            cases.append(("protein 6qlp_capped, open", np.array([0, len(x)], np.int32), xyz, x, np.array([Q], np.float32), len(x), zero))
        else:
            t0 = time.time()
            offsets, xyz, x, Q, N, box = synth.periodic_box_system(n, seed=0)
            co, cxyz, cx, cQ, cN, cell = synth.triclinic_cell_system(n, seed=0)
            print(f"# generated the {n}-atom cells in {time.time() - t0:.1f} s", flush=True)
            cases.append((f"{n} atoms, open cluster", offsets, xyz, x, Q, N, zero))
            if n <= 20_000:
                cases.append((f"{n} atoms, box=", offsets, xyz, x, Q, N, np.diag(np.asarray(box, np.float32).reshape(3))))
            cases.append((f"{n} atoms, sheared cell=", co, cxyz, cx, cQ, cN, np.asarray(cell, np.float32).reshape(3, 3)))
        for name, offsets, xyz, x, Q, N, cell in cases:
            A = int(offsets[-1])
            rng = np.random.default_rng(0)
            g = rng.normal(size=A).astype(np.float32)
            y = rng.normal(scale=0.3, size=A).astype(np.float32)
            reps = 20 if A <= 4096 else (3 if A <= 20_000 else 1)
            eng.set_option("grad_path", 2)
            t_grad, _ = timed(lambda: eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, cell=cell), reps)
            grad_scratch = int(eng.last_stats()[2])
            eng.set_option("train_path", 2)
            t_step, out = timed(lambda: eng.train_step_xyz(offsets, xyz, x, Q, y, N, apply=False, cell=cell), reps)
            st = eng.last_stats()
            gl = eng.get_gradients()
            line = {"workload": name, "atoms": A, "near_pairs": int(st[0]), "gradient_ms": round(t_grad * 1e3, 3),
                    "train_step_ms": round(t_step * 1e3, 3), "step_over_gradient": round(t_step / t_grad, 2),
                    "scratch_bytes": int(st[2]), "gradient_scratch_bytes": grad_scratch, "loss": float(out[1]),
                    "max_abs_weight_gradient": float(np.abs(gl).max())}
            if dense and A <= 2220:
                eng.set_option("train_path", 1)
                t_dense, out_d = timed(lambda: eng.train_step_xyz(offsets, xyz, x, Q, y, N, apply=False, cell=cell), 3)
                gd = eng.get_gradients()
                line["dense_step_ms"] = round(t_dense * 1e3, 3)
                line["dense_vs_pair_list_gradient"] = float(np.abs(gd - gl).max())
                line["dense_vs_pair_list_q"] = float(np.abs(out_d[0] - out[0]).max())
            eng.set_option("grad_path", 0)
            eng.set_option("train_path", 0)
            print(json.dumps(line), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
