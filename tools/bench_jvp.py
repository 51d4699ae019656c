#!/usr/bin/env python3
"""The forward-mode call charges_jvp_xyz beside the forward and the pair-list gradient call ("grad_path" = 2) of the same system, on
one handle (profiles/r11_jvp.txt):
  * the 2220-atom protein (open), tangent v;
  * a 10 000-atom cubic box (synth.periodic_box_system, box=), tangent v;
  * a 10 000-atom sheared cell (synth.triclinic_cell_system, cell=), tangents v, strain and dQ; the gradient call with strain=True.
    python tools/bench_jvp.py [--sizes 2220,10000] [--rounds 5]
The three calls alternate, `--rounds` times; every figure is wall clock per blocking host call (uploads, the pair count's round
trip and downloads included) over enough calls for a window of about half a second, after a warm-up call of each kind.  Printed
per system: the median and the range over the rounds, the ratios of the medians JVP / forward and JVP / gradient, the device
scratch the library reports (epnn_last_stats()[2]) beside the formula of include/epnn.h, and two checks of what was timed: q of
the JVP call against q of the gradient call (bits) and the adjoint identity g . tq = gxyz . v + gstrain : E between them.

The multi-tangent arm (profiles/r12_jvp_multi.txt):
    python tools/bench_jvp.py --multi [--systems protein,cell10000,qm9] [--rounds 5]
times, on one handle per system and over windows of about 0.3 s (shorter than the base arm's: 15 kinds of call alternate), the forward, the gradient call, the single-tangent call,
charges_jvp_xyz_multi at K = 1, 2, 4, 7, 8, 16 and K single-tangent calls in a row at the same K; the systems are the 2220-atom
protein (tangents v), a 10 000-atom sheared cell (v, strain, dQ) and 1024 QM9-sized molecules at N = 29 (v).  Printed per system:
medians and ranges, the ratio multi(K) / (K single calls) beside the sweep's operation-count model sum over chunks of
(16 + 16 kc) / (32 K), and whether every row of the K = 7 call has the bits of its single call."""
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


def scratch_formula(A, P, nx, n, with_v):
    return A * (1592 + 4 * nx + 257 * pieces(n) + (12 if with_v else 0)) + 980 * max(P, 1) + 13 * 1024


def window(fn, seconds=0.5):
    """seconds per call over a window of about `seconds` (at least 3 calls), the first call's time deciding the count"""
    t0 = time.perf_counter()
    out = fn()
    one = time.perf_counter() - t0
    reps = max(3, int(seconds / max(one, 1e-6)))
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


MULTI_KS = (1, 2, 4, 7, 8, 16)


def chunks(K):
    """the sweep's chunk widths for K tangents: the widest of 4, 2, 1 that fits what is left"""
    out = []
    while K:
        out.append(4 if K >= 4 else 2 if K >= 2 else 1)
        K -= out[-1]
    return out


def sweep_model(K):
    return sum(16 + 16 * kc for kc in chunks(K)) / (32.0 * K)


def multi_arm(w, systems, rounds):
    for system in systems:
        if system == "protein":
            xyz, x, Q, _ = charge_gn.read_xyz(os.path.join(ROOT, "tests/golden/protein/6qlp_capped.xyz"), 9)
            name, offsets, Q, N, geo, full = "protein 6qlp_capped, open", np.array([0, len(x)], np.int32), np.array([Q], np.float32), len(x), {}, False
        elif system.startswith("cell"):
            offsets, xyz, x, Q, N, cell = synth.triclinic_cell_system(int(system[4:]), seed=0)
            name, geo, full = f"{int(system[4:])} atoms, sheared cell=", {"cell": np.asarray(cell, np.float32).reshape(3, 3)}, True
        elif system == "qm9":
            offsets, xyz, x, Q, N = synth.qm9_like_batch(B=1024, seed=0, N=29)
            name, geo, full = "1024 QM9-sized molecules, N = 29", {}, False
        else:
            raise SystemExit(f"unknown system {system}")
        eng = Engine(nx=9, T=len(w["msg"]))
        eng.set_weights(w)
        eng.set_option("grad_path", 2)
        A, B = int(offsets[-1]), len(offsets) - 1
        rng = np.random.default_rng(0)
        g = rng.normal(size=A).astype(np.float32)
        KM = max(MULTI_KS)
        tan = {"v": rng.normal(size=(KM, A, 3)).astype(np.float32)}
        if full:
            tan["strain"] = (0.1 * rng.normal(size=(KM, 3, 3))).astype(np.float32)
            tan["dQ"] = rng.normal(size=KM).astype(np.float32)
        col = lambda k: {n: a[k] for n, a in tan.items()}
        first = lambda K: {n: a[:K] for n, a in tan.items()}

        def singles(K):
            for k in range(K):
                out = eng.charges_jvp_xyz(offsets, xyz, x, Q, N, **col(k), **geo)
            return out

        calls = {"forward": lambda: eng.forward_xyz(offsets, xyz, x, Q, N, **geo),
                 "gradient": lambda: eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, **geo),
                 "jvp": lambda: eng.charges_jvp_xyz(offsets, xyz, x, Q, N, **col(0), **geo)}
        for K in MULTI_KS:
            calls[f"multi_K{K}"] = lambda K=K: eng.charges_jvp_xyz_multi(offsets, xyz, x, Q, N, **first(K), **geo)
            calls[f"singles_K{K}"] = lambda K=K: singles(K)
        for fn in reversed(list(calls.values())):                    # warm-up, the largest scratch first
            fn()
        times = {k: [] for k in calls}
        for _ in range(rounds):
            for k, fn in calls.items():
                times[k].append(window(fn, 0.3)[0] * 1e3)
        q7, t7 = calls["multi_K7"]()
        st = eng.last_stats()
        bits = all(np.array_equal(t7[k], eng.charges_jvp_xyz(offsets, xyz, x, Q, N, **col(k), **geo)[1]) for k in range(7))
        med = {k: float(np.median(t)) for k, t in times.items()}
        line = {"workload": name, "atoms": A, "molecules": B, "near_pairs": int(st[0]), "rounds": rounds, "K7_scratch_bytes": int(st[2]),
                "K7_rows_have_single_call_bits": bool(bits), "max_abs_tq": float(np.abs(t7).max())}
        for k, t in times.items():
            line[k + "_ms"] = {"median": round(med[k], 3), "range": [round(min(t), 3), round(max(t), 3)]}
        for K in MULTI_KS:
            line[f"K{K}"] = {"chunks": chunks(K), "multi_over_singles": round(med[f"multi_K{K}"] / med[f"singles_K{K}"], 3),
                             "sweep_model": round(sweep_model(K), 3), "multi_over_gradient": round(med[f"multi_K{K}"] / med["gradient"], 3)}
        print(json.dumps(line), flush=True)
        eng.close()


def main():
    sizes = [2220, 10_000]
    rounds = 5
    if "--sizes" in sys.argv:
        sizes = [int(s) for s in sys.argv[sys.argv.index("--sizes") + 1].split(",")]
    if "--rounds" in sys.argv:
        rounds = int(sys.argv[sys.argv.index("--rounds") + 1])
    w = checkpoint.load_epnn_weights(os.path.join(ROOT, "models/decay_model_weights"))
    if "--multi" in sys.argv:
        systems = ["protein", "cell10000", "qm9"]
        if "--systems" in sys.argv:
            systems = sys.argv[sys.argv.index("--systems") + 1].split(",")
        return multi_arm(w, systems, rounds)
    eng = Engine(nx=9, T=len(w["msg"]))
    eng.set_weights(w)
    eng.set_option("grad_path", 2)
    cases = []
    for n in sizes:
        if n == 2220:
            xyz, x, Q, _ = charge_gn.read_xyz(os.path.join(ROOT, "tests/golden/protein/6qlp_capped.xyz"), 9)
            cases.append(("protein 6qlp_capped, open", np.array([0, len(x)], np.int32), xyz, x, np.array([Q], np.float32), len(x), {}, False))
        else:
            offsets, xyz, x, Q, N, box = synth.periodic_box_system(n, seed=0)
            co, cxyz, cx, cQ, cN, cell = synth.triclinic_cell_system(n, seed=0)
            cases.append((f"{n} atoms, cubic box=", offsets, xyz, x, Q, N, {"box": np.asarray(box, np.float32).reshape(3)}, False))
            cases.append((f"{n} atoms, sheared cell=, strain", co, cxyz, cx, cQ, cN, {"cell": np.asarray(cell, np.float32).reshape(3, 3)}, True))
    for name, offsets, xyz, x, Q, N, geo, strain in cases:
        A = int(offsets[-1])
        rng = np.random.default_rng(0)
        g = rng.normal(size=A).astype(np.float32)
        v = rng.normal(size=(A, 3)).astype(np.float32)
        E = (0.1 * rng.normal(size=(3, 3))).astype(np.float32) if strain else None
        dQ = 1.0 if strain else None
        vgeo = dict(geo, strain=True) if strain else geo
        calls = {"forward": lambda: eng.forward_xyz(offsets, xyz, x, Q, N, **geo),
                 "jvp": lambda: eng.charges_jvp_xyz(offsets, xyz, x, Q, N, v=v, strain=E, dQ=dQ, **geo),
                 "gradient": lambda: eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, **vgeo)}
        for fn in calls.values():                                    # warm-up: code objects, scratch of the largest call
            fn()
        times = {k: [] for k in calls}
        outs = {}
        for _ in range(rounds):
            for k, fn in calls.items():
                t, outs[k] = window(fn)
                times[k].append(t * 1e3)
        calls["jvp"]()
        st = eng.last_stats()
        calls["gradient"]()
        sg = eng.last_stats()
        q, tq = outs["jvp"]
        gq, gx = outs["gradient"][:2]
        lhs = float(g.astype(np.float64) @ tq.astype(np.float64))
        rhs = float((gx.astype(np.float64) * v).sum())
        if strain:
            rhs += float((outs["gradient"][2][0].astype(np.float64) * E).sum())
            lhs -= float(g.astype(np.float64) @ eng.charges_jvp_xyz(offsets, xyz, x, Q, N, dQ=dQ, **geo)[1].astype(np.float64))
        med = {k: float(np.median(t)) for k, t in times.items()}
        line = {"workload": name, "atoms": A, "near_pairs": int(st[0]), "rounds": rounds}
        for k, t in times.items():
            line[k + "_ms_median"] = round(med[k], 3)
            line[k + "_ms_range"] = [round(min(t), 3), round(max(t), 3)]
        line.update({"jvp_over_forward": round(med["jvp"] / med["forward"], 3), "jvp_over_gradient": round(med["jvp"] / med["gradient"], 3),
                     "jvp_scratch_bytes": int(st[2]), "jvp_scratch_formula_bytes": scratch_formula(A, int(st[0]), 9, A, True),
                     "gradient_scratch_bytes": int(sg[2]), "q_bits_equal_gradient_call": bool(np.array_equal(q, gq)),
                     "q_vs_forward": float(np.abs(q - outs["forward"]).max()), "g_dot_tq": lhs, "gxyz_dot_v_plus_gstrain_E": rhs,
                     "max_abs_tq": float(np.abs(tq).max())})
        print(json.dumps(line), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
