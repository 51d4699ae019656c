#!/usr/bin/env python3
"""General (triclinic) cells beside orthorhombic boxes, in one process, alternating (profiles/r08_cells.txt):
  (a) the 100 000-, 10 000- and 2220-atom cubic cells of synth.periodic_box_system through box= and through cell=diag(box);
  (b) synth.triclinic_cell_system (a sheared cell of the same density) at the same sizes;
  (c) 1024 QM9-sized molecules in 6 A cells, box= and cell=diag;
  (d) charges_vjp_xyz with and without the strain derivative on the three batches of tools/bench_grad.py (open molecules: the plain
      call beside all-zero cells) and on a batch of 64-atom cells, box= beside a sheared cell of the same volume.
    python tools/bench_cell.py [--quick]          (--quick: no 100 000-atom cells)
Every line is measured three times (the alternation is repeated), so that the spread can be read beside the differences.
Forward times are wall clock per forward of the device-resident entry, back to back, after a warm-up, with the front-end's share
from epnn_last_timing in a separate blocking call; gradient times are wall clock per blocking call.  partners = 2 pairs / atoms."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from epnn_amd import checkpoint, synth  # noqa: E402
from epnn_amd.engine import Engine  # noqa: E402

REPEATS = 3


def timed_forward(eng, offsets, xyz, x, Q, N, steps, **kw):
    A = int(offsets[-1])
    d = [eng.to_device(a) for a in (xyz, x, Q)]
    dq = eng.alloc(A * 4)
    for _ in range(2):
        eng.forward_xyz_dev(offsets, d[0], d[1], d[2], dq, N, **kw)
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.forward_xyz_dev(offsets, d[0], d[1], d[2], dq, N, **kw)
    eng.sync()
    dt = (time.perf_counter() - t0) / steps
    pairs = int(eng.last_stats()[0])
    q = dq.download((A,))
    for a in d + [dq]:
        a.free()
    return dt, pairs, q


def timed_call(fn, reps):
    for _ in range(3):
        fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def cell_batch(B, n, cell, seed):
    """B cells of n atoms each, uniform in `cell` (3, 3) with an image separation of 0.9 A (a grid of fractional bins)."""
    rng = np.random.default_rng(seed)
    H = np.asarray(cell, np.float64)
    G = np.linalg.inv(H)
    xyz = []
    for _ in range(B):
        pts = []
        while len(pts) < n:
            f = rng.uniform(0, 1, 3)
            if pts:
                u = f[None] - np.array(pts)
                u -= np.rint(u)
                if (((u @ H) ** 2).sum(1) < 0.81).any():
                    continue
            pts.append(f)
        xyz.append(np.array(pts) @ H)
    xyz = np.concatenate(xyz).astype(np.float32)
    names = [e for e, _ in synth.PROTEIN_ELEMS]
    ep = np.array([p for _, p in synth.PROTEIN_ELEMS])
    x = synth.features(rng.choice(names, size=B * n, p=ep / ep.sum()))
    offsets = (np.arange(B + 1) * n).astype(np.int32)
    return offsets, xyz, x, np.zeros(B, np.float32)


def main():
    quick = "--quick" in sys.argv
    w = checkpoint.load_epnn_weights(os.path.join(ROOT, "models/decay_model_weights"))
    eng = Engine(nx=9, T=5)
    eng.set_weights(w)
    rows = []

    def report(name, rep, A, dt, pairs, q, Q):
        line = {"workload": name, "repeat": rep, "atoms": A, "ms_per_forward": round(dt * 1e3, 4), "atoms_per_s": A / dt,
                "near_pairs": pairs, "partners_per_atom": round(2 * pairs / A, 3),
                "charge_error": float(abs(q.sum(dtype=np.float64) - Q.sum()))}
        rows.append(line)
        print(json.dumps(line), flush=True)

    def summary(names):
        by = {n: [r["ms_per_forward"] if "ms_per_forward" in r else r["ms_per_call"] for r in rows if r["workload"] == n] for n in names}
        base = np.median(by[names[0]])
        for n in names:
            v = by[n]
            print(f"#   {n}: median {np.median(v):.4f} ms, spread {min(v):.4f} .. {max(v):.4f} ({(max(v) - min(v)) / np.median(v) * 100:.1f} %), "
                  f"{np.median(v) / base:.3f}x of the first", flush=True)

    # ---- (a), (b): large cells
    sizes = ([] if quick else [100_000]) + [10_000, 2220]
    for n in sizes:
        t0 = time.time()
        offsets, xyz, x, Q, N, box = synth.periodic_box_system(n, seed=0)
        to, txyz, tx, tQ, tN, tcell = synth.triclinic_cell_system(n, seed=0)
        print(f"# generated the {n}-atom cells (cubic L = {box[0, 0]:.3f} A; sheared, same volume) in {time.time() - t0:.1f} s", flush=True)
        steps = 3 if n >= 100_000 else (20 if n >= 10_000 else 200)
        names = [f"cubic cell {n}, box=", f"cubic cell {n}, cell=diag", f"sheared cell {n}, cell="]
        for rep in range(REPEATS):
            report(names[0], rep, n, *timed_forward(eng, offsets, xyz, x, Q, N, steps, box=box), Q)
            report(names[1], rep, n, *timed_forward(eng, offsets, xyz, x, Q, N, steps, cell=np.diag(box[0])), Q)
            report(names[2], rep, n, *timed_forward(eng, to, txyz, tx, tQ, tN, steps, cell=tcell), tQ)
        summary(names)
        for nm, kw, arrs in ((names[0], {"box": box}, (offsets, xyz, x, Q, N)), (names[2], {"cell": tcell}, (to, txyz, tx, tQ, tN))):
            eng.set_option("profile", 1)                           # a blocking, profiled call: epnn_last_timing splits off the front-end
            eng.forward_xyz(*arrs, **kw)
            tm = eng.last_timing()
            eng.set_option("profile", 0)
            print(f"#   {nm}: device ms front-end {tm[0]:.4f}, fused {tm[1]:.4f}, tiled {tm[2]:.4f}, total {tm[3]:.4f}", flush=True)
    # ---- (c): many small cells
    offsets, xyz, x, Q, N = synth.qm9_like_batch(B=1024, seed=0, N=29)
    A = int(offsets[-1])
    L = np.full(3, 6.0, np.float32)
    names = ["1024 QM9-sized molecules, 6 A cells, box=", "1024 QM9-sized molecules, 6 A cells, cell=diag"]
    for rep in range(REPEATS):
        report(names[0], rep, A, *timed_forward(eng, offsets, xyz, x, Q, N, 200, box=L), Q)
        report(names[1], rep, A, *timed_forward(eng, offsets, xyz, x, Q, N, 200, cell=np.diag(L)), Q)
    summary(names)
    eng.close()

    # ---- (d): gradients, with and without the strain derivative
    import bench_grad
    w10 = checkpoint.load_epnn_weights(os.path.join(ROOT, "models", "model_weights"))
    sheared = np.float32([[8, 0, 0], [3, 8, 0], [-2.5, 2, 8]])           # the volume of the 8 A cube, widths 7.3 / 7.8 / 8.0
    cases = [("1 validation molecule, N=41", bench_grad.val_batch(1), 41, w10, 10, 50, None),
             ("8 validation molecules, N=41", bench_grad.val_batch(8), 41, w10, 10, 30, None),
             ("1024 QM9-like molecules, N=29", (offsets, xyz, x, Q), 29, w, 9, 5, None),
             ("16 cells of 64 atoms, N=64", None, 64, w, 9, 10, sheared)]
    for label, batch, N, wts, nx, reps, cell in cases:
        e = Engine(nx=nx, T=len(wts["msg"]))
        e.set_weights(wts)
        if cell is None:
            off, cx, cxx, cQ = batch
            g = np.random.default_rng(0).normal(size=int(off[-1])).astype(np.float32)
            zero = np.zeros((3, 3), np.float32)
            variants = [(f"{label}: plain call", lambda: e.charges_vjp_xyz(off, cx, cxx, cQ, g, N)),
                        (f"{label}: all-zero cells", lambda: e.charges_vjp_xyz(off, cx, cxx, cQ, g, N, cell=zero)),
                        (f"{label}: all-zero cells, strain", lambda: e.charges_vjp_xyz(off, cx, cxx, cQ, g, N, cell=zero, strain=True))]
            pairs_of = [(off, cx, cxx, cQ, {})] * 3
        else:
            off, bx, bxx, bQ = cell_batch(16, 64, np.diag(np.float32([8, 8, 8])), seed=1)
            _, sx, sxx, sQ = cell_batch(16, 64, cell, seed=1)
            g = np.random.default_rng(0).normal(size=int(off[-1])).astype(np.float32)
            box = np.float32([8, 8, 8])
            variants = [(f"{label}: box=", lambda: e.charges_vjp_xyz(off, bx, bxx, bQ, g, N, box=box)),
                        (f"{label}: sheared cell", lambda: e.charges_vjp_xyz(off, sx, sxx, sQ, g, N, cell=cell)),
                        (f"{label}: sheared cell, strain", lambda: e.charges_vjp_xyz(off, sx, sxx, sQ, g, N, cell=cell, strain=True))]
            pairs_of = [(off, bx, bxx, bQ, {"box": box}), (off, sx, sxx, sQ, {"cell": cell}), (off, sx, sxx, sQ, {"cell": cell})]
        partners = []
        for o_, a_, b_, c_, kw in pairs_of:
            e.forward_xyz(o_, a_, b_, c_, N, **kw)
            partners.append(round(2 * int(e.last_stats()[0]) / int(o_[-1]), 3))
        for rep in range(REPEATS):
            for (name, fn), pp in zip(variants, partners):
                t = timed_call(fn, reps)
                line = {"workload": name, "repeat": rep, "molecules": len(off) - 1, "atoms": int(off[-1]), "ms_per_call": round(t * 1e3, 4),
                        "partners_per_atom": pp}
                rows.append(line)
                print(json.dumps(line), flush=True)
        summary([v[0] for v in variants])
        e.close()


if __name__ == "__main__":
    main()
