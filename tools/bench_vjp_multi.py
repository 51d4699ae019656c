#!/usr/bin/env python3
"""charges_vjp_xyz_multi (epnn_charges_vjp_multi_xyz_cell) beside K calls of the single entry charges_vjp_xyz on "grad_path" 2, on one
handle per system (profiles/r24_vjp_multi.txt):
    python tools/bench_vjp_multi.py [--systems protein,cell10000,qm9] [--rounds 5] [--once SYSTEM]
  * the 2220-atom protein (open), a 10 000-atom sheared cell (synth.triclinic_cell_system, cell=, strain=True on both sides) and
    1024 QM9-sized molecules at N = 29;
  * the forward, the single gradient call, the K = 3 and K = 16 calls and K single calls in a row at the same K alternate, `--rounds`
    times; every figure is wall clock per blocking host call (uploads, the pair count's round trip and downloads included) over
    enough calls for a window of about 0.3 s, after a warm-up call of each kind.
Printed per system, one JSON line: medians and ranges, the ratio multi(K) / (K single calls) and whether the two ranges overlap,
the sweeps' operation-count model sum over chunks of (32 + 32 kc) / (64 K), the forward's share of a single gradient call (what
each of the K - 1 saved forwards is worth), the reported scratch beside the formula of include/epnn.h, and whether every row of
the K = 3 call has the bits of its single call.
--once SYSTEM makes one warm K = 3 call and stops: the run to put under a kernel trace."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epnn_amd import charge_gn, checkpoint, synth  # noqa: E402
from epnn_amd.engine import Engine  # noqa: E402

KS = (3, 16)


def pieces(n):
    tiles = (n + 15) // 16
    return min(16, max(1, (2048 + tiles - 1) // tiles))


def scratch_formula(A, B, P, nx, T, n, K):
    return A * (744 + 4 * nx + 324 * T + pieces(n) + K * (580 + 256 * pieces(n))) + (268 + 848 * K) * max(P, 1) + 36 * K * B + 13 * 1024


def window(fn, seconds=0.3):
    """seconds per call over a window of about `seconds` (at least 3 calls), the first call's time deciding the count"""
    t0 = time.perf_counter()
    out = fn()
    one = time.perf_counter() - t0
    reps = max(3, int(seconds / max(one, 1e-6)))
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps, out


def chunks(K):
    """the sweeps' chunk widths for K cotangents: the widest of 4, 2, 1 that fits what is left"""
    out = []
    while K:
        out.append(4 if K >= 4 else 2 if K >= 2 else 1)
        K -= out[-1]
    return out


def sweep_model(K):
    return sum(32 + 32 * kc for kc in chunks(K)) / (64.0 * K)


def load(system):
    if system == "protein":
        xyz, x, Q, _ = charge_gn.read_xyz(os.path.join(ROOT, "tests/golden/protein/6qlp_capped.xyz"), 9)
        return "protein 6qlp_capped, open", np.array([0, len(x)], np.int32), xyz, x, np.array([Q], np.float32), len(x), {}
    if system.startswith("cell"):
        offsets, xyz, x, Q, N, cell = synth.triclinic_cell_system(int(system[4:]), seed=0)
        return f"{int(system[4:])} atoms, sheared cell=, strain", offsets, xyz, x, Q, N, {"cell": np.asarray(cell, np.float32).reshape(3, 3), "strain": True}
    if system == "qm9":
        offsets, xyz, x, Q, N = synth.qm9_like_batch(B=1024, seed=0, N=29)
        return "1024 QM9-sized molecules, N = 29", offsets, xyz, x, Q, N, {}
    raise SystemExit(f"unknown system {system}")


def bench(w, system, rounds, once):
    name, offsets, xyz, x, Q, N, geo = load(system)
    eng = Engine(nx=9, T=len(w["msg"]))
    eng.set_weights(w)
    eng.set_option("grad_path", 2)
    A, B = int(offsets[-1]), len(offsets) - 1
    g = np.random.default_rng(0).normal(size=(max(KS), A)).astype(np.float32)
    fgeo = {k: v for k, v in geo.items() if k != "strain"}
    if once:
        eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, g[:3], N, **geo)
        eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, g[:3], N, **geo)
        eng.close()
        return

    def singles(K):
        for k in range(K):
            out = eng.charges_vjp_xyz(offsets, xyz, x, Q, g[k], N, **geo)
        return out

    calls = {"forward": lambda: eng.forward_xyz(offsets, xyz, x, Q, N, **fgeo),
             "gradient": lambda: eng.charges_vjp_xyz(offsets, xyz, x, Q, g[0], N, **geo)}
    for K in KS:
        calls[f"multi_K{K}"] = lambda K=K: eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, g[:K], N, **geo)
        calls[f"singles_K{K}"] = lambda K=K: singles(K)
    for fn in reversed(list(calls.values())):                        # warm-up, the largest scratch first
        fn()
    times = {k: [] for k in calls}
    for _ in range(rounds):
        for k, fn in calls.items():
            times[k].append(window(fn)[0] * 1e3)
    out3 = calls["multi_K3"]()
    st = eng.last_stats()
    bits = True
    for k in range(3):
        one = eng.charges_vjp_xyz(offsets, xyz, x, Q, g[k], N, **geo)
        bits = bits and np.array_equal(out3[0], one[0]) and all(np.array_equal(out3[i][k], one[i]) for i in range(1, len(one)))
    med = {k: float(np.median(t)) for k, t in times.items()}
    line = {"workload": name, "atoms": A, "molecules": B, "near_pairs": int(st[0]), "rounds": rounds, "K3_scratch_bytes": int(st[2]),
            "K3_scratch_formula_bytes": scratch_formula(A, B, int(st[0]), 9, len(w["msg"]), int(np.diff(offsets).max()), 3),
            "K3_rows_have_single_call_bits": bool(bits), "max_abs_gxyz": float(np.abs(out3[1]).max())}
    for k, t in times.items():
        line[k + "_ms"] = {"median": round(med[k], 3), "range": [round(min(t), 3), round(max(t), 3)]}
    fwd_share = med["forward"] / med["gradient"]                     # (the tiled forward's time: an estimate of the checkpointed one's)
    for K in KS:
        m, s = times[f"multi_K{K}"], times[f"singles_K{K}"]
        line[f"K{K}"] = {"chunks": chunks(K), "multi_over_singles": round(med[f"multi_K{K}"] / med[f"singles_K{K}"], 3),
                         "ranges_apart": bool(max(m) < min(s) or max(s) < min(m)), "sweep_model": round(sweep_model(K), 3),
                         "multi_over_gradient": round(med[f"multi_K{K}"] / med["gradient"], 3)}
    line["forward_over_gradient"] = round(fwd_share, 3)
    print(json.dumps(line), flush=True)
    eng.close()


def main():
    systems, rounds = ["protein", "cell10000", "qm9"], 5
    if "--systems" in sys.argv:
        systems = sys.argv[sys.argv.index("--systems") + 1].split(",")
    if "--rounds" in sys.argv:
        rounds = int(sys.argv[sys.argv.index("--rounds") + 1])
    w = checkpoint.load_epnn_weights(os.path.join(ROOT, "models/decay_model_weights"))
    if "--once" in sys.argv:
        return bench(w, sys.argv[sys.argv.index("--once") + 1], 0, True)
    for system in systems:
        bench(w, system, rounds, False)


if __name__ == "__main__":
    main()
