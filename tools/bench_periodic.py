#!/usr/bin/env python3
"""Periodic cells beside open systems, in one process (profiles/r06_periodic.txt):
  * the 100 000- and 10 000-atom cells of synth.periodic_box_system, periodic and the same coordinates as an open cluster;
  * a 2220-atom periodic cell, beside its open run with the merged ("large_merge" 1, the default) and the separate front-end;
  * 1024 QM9-sized molecules in 6 A cells (synth.qm9_like_batch) beside the same batch open with "wave_front" 0 and 1.
    python tools/bench_periodic.py [--quick]          (--quick: 10 000 atoms instead of 100 000)
Times are wall clock per forward of the device-resident entry, back to back, after a warm-up; partners = 2 pairs / atoms."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epnn_amd import checkpoint, synth
from epnn_amd.engine import Engine


def timed(eng, offsets, xyz, x, Q, N, box, steps):
    A = int(offsets[-1])
    d = [eng.to_device(a) for a in (xyz, x, Q)]
    dq = eng.alloc(A * 4)
    for _ in range(2):
        eng.forward_xyz_dev(offsets, d[0], d[1], d[2], dq, N, box=box)
    eng.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        eng.forward_xyz_dev(offsets, d[0], d[1], d[2], dq, N, box=box)
    eng.sync()
    dt = (time.perf_counter() - t0) / steps
    pairs = int(eng.last_stats()[0])
    q = dq.download((A,))
    for a in d + [dq]:
        a.free()
    return dt, pairs, q


def main():
    quick = "--quick" in sys.argv
    w = checkpoint.load_epnn_weights(os.path.join(ROOT, "models/decay_model_weights"))
    eng = Engine(nx=9, T=5)
    eng.set_weights(w)
    rows = []

    def report(name, A, dt, pairs, q, Q):
        line = {"workload": name, "atoms": A, "ms_per_forward": round(dt * 1e3, 4), "atoms_per_s": A / dt,
                "near_pairs": pairs, "partners_per_atom": round(2 * pairs / A, 3), "charge_error": float(abs(q.sum(dtype=np.float64) - Q.sum()))}
        rows.append(line)
        print(json.dumps(line), flush=True)

    sizes = [10_000] if quick else [100_000, 10_000]
    for n in sizes + [2220]:
        t0 = time.time()
        offsets, xyz, x, Q, N, box = synth.periodic_box_system(n, seed=0)
        print(f"# generated the {n}-atom cell (L = {box[0, 0]:.3f} A) in {time.time() - t0:.1f} s", flush=True)
        steps = 3 if n >= 100_000 else (20 if n >= 10_000 else 200)
        for name, b, opt in ((f"periodic cell {n}", box, None), (f"open cluster {n} (same coordinates)", None, None),
                             (f"open cluster {n}, large_merge 0", None, ("large_merge", 0))):
            if opt and n != 2220:
                continue
            if opt:
                eng.set_option(*opt)
            dt, pairs, q = timed(eng, offsets, xyz, x, Q, N, b, steps)
            if opt:
                eng.set_option(opt[0], 1)
            report(name, n, dt, pairs, q, Q)
    offsets, xyz, x, Q, N = synth.qm9_like_batch(B=1024, seed=0, N=29)
    A = int(offsets[-1])
    box = np.full(3, 6.0, np.float32)
    dt, pairs, q = timed(eng, offsets, xyz, x, Q, N, box, 200)
    report("1024 QM9-sized molecules, 6 A periodic cells", A, dt, pairs, q, Q)
    for wf in (0, 1):
        eng.set_option("wave_front", wf)
        dt, pairs, q = timed(eng, offsets, xyz, x, Q, N, None, 200)
        report(f"1024 QM9-sized molecules, open, wave_front {wf}", A, dt, pairs, q, Q)
    eng.set_option("wave_front", 1)
    by = {r["workload"]: r for r in rows}
    for n in sizes + [2220]:
        p, o = by[f"periodic cell {n}"], by[f"open cluster {n} (same coordinates)"]
        print(f"# {n} atoms: periodic / open = {p['ms_per_forward'] / o['ms_per_forward']:.3f}x "
              f"({p['ms_per_forward'] - o['ms_per_forward']:+.3f} ms); partners per atom {p['partners_per_atom']} vs {o['partners_per_atom']}")
    p, o = by["1024 QM9-sized molecules, 6 A periodic cells"], by["1024 QM9-sized molecules, open, wave_front 0"]
    print(f"# QM9-sized batch: periodic / open wave_front 0 = {p['ms_per_forward'] / o['ms_per_forward']:.3f}x")
    eng.close()


if __name__ == "__main__":
    main()
