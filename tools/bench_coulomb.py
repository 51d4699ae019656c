#!/usr/bin/env python3
"""The electrostatics call coulomb_xyz beside the pair-list gradient call charges_vjp_xyz ("grad_path" = 2) of the same system, on
one handle (profiles/r16_coulomb.txt):
  * the 2220-atom protein (open);
  * a 10 000-atom open cluster (synth.periodic_box_system's atoms without its box, as tools/bench_grad_large.py runs them);
  * 1024 QM9-sized molecules at N = 29.
    python tools/bench_coulomb.py [--systems protein,cluster10000,qm9] [--rounds 5] [--alpha 0.0]
The two calls alternate, `--rounds` times; every figure is wall clock per blocking host call (uploads, the pair count's round
trip and downloads included) over enough calls for a window of about half a second, after a warm-up call of each kind.  Printed
per system: the median and the range over the rounds, the ratio of the medians coulomb / gradient, the device scratch the library
reports (epnn_last_stats()[2]) beside the formula of include/epnn.h, and checks of what was timed: q of the two calls (bits), fq
against -gxyz of the gradient call seeded with phi (bits), and sum_i f_i over the batch.
    python tools/bench_coulomb.py --trace [--systems ...]
makes three calls of coulomb_xyz per system and nothing else: the run to put under a kernel trace, whose k_cl_* rows are the Coulomb
kernels.
    python tools/bench_coulomb.py --cell [--systems qm9cell,cell10000,cell100000] [--rounds 5] [--alpha 0.0] [--tol 1e-6] [--trace]
is the periodic call coulomb_xyz_cell beside charges_vjp_xyz(cell=, strain=True) of the same system (profiles/r17_coulomb_cell.txt):
1024 QM9-sized cells of 6 A, a 10 000-atom and a 100 000-atom cubic cell (synth.periodic_box_system).  The same alternation and
windows; printed besides: the k slots of the batch, and the checks q (bits), fq and gstrain_q against the gradient call seeded with
phi (bits), sum_i f_i.  With --trace: three calls of coulomb_xyz_cell per system (the k_ew_* rows are the Ewald kernels).
    python tools/bench_coulomb.py --excl [--cell] [--systems ...] [--rounds 5] [--alpha 0.0] [--near 2.2] [--trace]
is the call with bonded exclusions, coulomb_xyz_excl or coulomb_xyz_cell_excl, beside the plain call of the same batch
(profiles/r18_coulomb_excl.txt).  The list: every pair of a molecule with (minimum-image) D < --near, factors cycling through 0, 0.5,
0.8333 in sorted pair order, handed over shuffled with half of the rows swapped -- a few pairs per atom.  Printed per system: the two
medians and their ratio, pairs per atom, the scratch the list adds beside the formula of include/epnn.h, and the checks q (bits
against the plain call) and fq against -gxyz of the gradient call seeded with phi (bits).  With --trace: three calls of the _excl
entry per system (the k_cl_excl row is the new kernel).
    python tools/bench_coulomb.py --slab [--systems qm9slab,slab2048,slab10000] [--rounds 5] [--alpha 0.0] [--tol 1e-6] [--trace]
is the slab call coulomb_xyz_slab (two periodic axes, the exact two-dimensional Ewald sum; profiles/r19_coulomb_slab.txt) beside two
figures of the same process: charges_vjp_xyz(cell=slab cell) of the same atoms, the tool's yardstick, and coulomb_xyz_cell of the same
atoms in a cell whose third vector is nhat times three slab thicknesses and at least twice the cutoff, which is what a caller had to
do before.  The workloads: 1024 QM9-sized 6.5 A square slabs 5 A thick, a 2048-atom and a 10 000-atom slab on a jittered lattice at
the tool's cell density (0.1 per A^3, four layers).  Printed besides: the listed half-plane slots, the scratch beside the formula of
include/epnn.h, and the checks q (bits) and fq against -gxyz of the gradient call seeded with phi (bits).  With --trace: three calls
of coulomb_xyz_slab per system (the k_sl_* rows are the new kernels; k_ew_sweep is the real-space part).
    python tools/bench_coulomb.py --slab --strain [--systems ...] [--rounds 5] [--alpha 0.0] [--tol 1e-6] [--against FILE] [--trace]
is the strain call coulomb_xyz_slab_strain beside the plain slab call of the same build, alternating, on the same three workloads
(profiles/r20_coulomb_slab_strain.txt).  Printed per system: the two medians and their ratio, the scratch of the strain call beside
the formula of include/epnn.h, and the checks: q, phi, E, F, ffix, fq of the two calls (bits), gstrain_q against gs of the gradient
call seeded with phi (bits), gstrain == gstrain_fix + gstrain_q and its symmetry (bits).  --against FILE: the JSON lines that
`--slab` printed on another build (the parent commit) in the same session; adds the ratio of this build's plain call to that one's.
With --trace: three calls of coulomb_xyz_slab_strain per system (k_sl_sweep_strain, k_sl_atom_strain, k_sl_energy_strain).
    python tools/bench_coulomb.py --site [--cell] [--systems ...] [--rounds 5] [--alpha 0.0] [--near 2.2] [--tol 1e-6] [--trace]
is the call with per-atom Gaussian widths, self-energy and on-site terms, coulomb_xyz_site or coulomb_xyz_cell_site, beside the _excl
call of the same batch and list at --alpha, alternating on one handle (profiles/r25_coulomb_site.txt).  Widths, chi and J come from
tables by element through engine.per_element; in cells the widths' table is scaled so that the widest Gaussian is 0.9 of the largest
width 1 / (2 beta) the batch's cells allow.  Printed per system: the two medians and their ratio, the scratch the site data adds beside
the formula of include/epnn.h, and the checks q (bits against the _excl call) and fq (and gstrain_q) against the gradient call
seeded with mu (bits).  With --trace: three calls of the site entry per system (k_cl_sweep_site, k_ew_sweep_site, k_cl_atom_site,
k_ew_atom_site, k_ew_wsum, k_ew_energy_site and the widths instances of k_cl_excl are the new kernels).
    python tools/bench_coulomb.py --slab --site [--strain] [--systems qm9slab,slab2048,slab10000] [--rounds 5] [--near 2.2] [--tol 1e-6] [--trace]
is the slab call with per-atom widths, self-energy and on-site terms, coulomb_xyz_slab_site, beside coulomb_xyz_slab with the same list,
alternating on one handle (profiles/r26_coulomb_slab_site.txt); with --strain the two strain entries.  Widths, chi and J by element as
for --site, the widths scaled down only where the widest would exceed 0.9 of the largest width 1 / (2 beta) the batch's cells allow (the
6.5 A slabs).  Printed per system: the two medians and their ratio, the scratch the site data adds beside 20 A, and the checks q (bits
against the slab call) and fq (with --strain gstrain_q too) against the gradient call seeded with mu (bits).  With --trace: three calls
of the site entry per system (k_sl_atom_site or k_sl_atom_strain_site are the new kernels; k_ew_sweep_site is the real-space part)."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from epnn_amd import charge_gn, checkpoint, synth  # noqa: E402
from epnn_amd.engine import Engine  # noqa: E402


def gl_pieces(n):
    tiles = (n + 15) // 16
    return min(16, max(1, (2048 + tiles - 1) // tiles))


def cl_pieces(n):
    return 1 if n <= 64 else max(1, min(32, (n + 127) // 128, (2048 + (n + 63) // 64 - 1) // ((n + 63) // 64)))


def cl_tasks(ns):
    """the Coulomb sweep's wavefronts: molecules of up to 64 atoms packed in batch order, blocks x pieces for larger ones"""
    tasks, b = 0, 0
    while b < len(ns):
        if ns[b] <= 64:
            tot = 0
            while b < len(ns) and ns[b] <= 64 and tot + ns[b] <= 64:
                tot += ns[b]
                b += 1
            tasks += 1
        else:
            tasks += (ns[b] + 63) // 64 * cl_pieces(ns[b])
            b += 1
    return tasks


def scratch_formula(ns, P, nx, T):
    A, B = sum(ns), len(ns)
    gtasks = sum((n + 15) // 16 * gl_pieces(n) for n in ns)
    return (A * (1344 + 4 * nx + 324 * T + 256 * max(map(gl_pieces, ns)) + 32 * max(map(cl_pieces, ns))) + 16 * (gtasks + cl_tasks(ns))
            + 1116 * max(P, 1) + 56 * B + 8240)


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


def load(system):
    if system == "protein":
        xyz, x, Q, _ = charge_gn.read_xyz(os.path.join(ROOT, "tests/golden/protein/6qlp_capped.xyz"), 9)
        return "protein 6qlp_capped, open", np.array([0, len(x)], np.int32), xyz, x, np.array([Q], np.float32), len(x)
    if system.startswith("cluster"):
        offsets, xyz, x, Q, N, _ = synth.periodic_box_system(int(system[7:]), seed=0)
        return f"{int(system[7:])} atoms, open cluster", offsets, xyz, x, Q, N
    if system == "qm9":
        offsets, xyz, x, Q, N = synth.qm9_like_batch(B=1024, seed=0, N=29)
        return "1024 QM9-sized molecules, N = 29", offsets, xyz, x, Q, N
    raise SystemExit(f"unknown system {system}")


def load_cell(system):
    """(name, offsets, xyz, x, Q, N, cells (B, 3, 3))"""
    if system == "qm9cell":
        ns = np.diff(synth.qm9_like_batch(B=1024, seed=0, N=29)[0])
        parts = [synth.periodic_box_system(int(n), seed=k, density=int(n) / 6.0001 ** 3) for k, n in enumerate(ns)]
        offsets = np.zeros(len(ns) + 1, np.int32)
        offsets[1:] = np.cumsum(ns)
        cells = np.stack([np.diag(p[5][0]) for p in parts]).astype(np.float32)
        return ("1024 QM9-sized cells of 6 A, N = 29", offsets, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]),
                np.concatenate([p[3] for p in parts]).astype(np.float32), 29, cells)
    if system.startswith("cell"):
        offsets, xyz, x, Q, N, box = synth.periodic_box_system(int(system[4:]), seed=0)
        return f"{int(system[4:])} atoms, cubic cell of {float(box[0][0]):.2f} A", offsets, xyz, x, Q, N, np.diag(box[0]).astype(np.float32)[None]
    raise SystemExit(f"unknown system {system}")


def lattice_slab(nx, ny, layers, seed, density=0.1):
    """nx x ny x layers atoms on a lattice of spacing density^(-1/3), each moved by up to 0.5 A per axis (no two closer than the
    spacing less 1 A), in the rectangular slab cell of that lattice, open along z; the element mix of periodic_box_system."""
    rng = np.random.default_rng(seed)
    d = density ** (-1.0 / 3.0)
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(layers), indexing="ij"), -1).reshape(-1, 3) * d
    xyz = (g + rng.uniform(-0.5, 0.5, g.shape)).astype(np.float32)
    names = [e for e, _ in synth.PROTEIN_ELEMS]
    ep = np.array([p for _, p in synth.PROTEIN_ELEMS])
    x = synth.features(rng.choice(names, size=len(xyz), p=ep / ep.sum()))
    cell = np.float32([[nx * d, 0, 0], [0, ny * d, 0], [0, 0, 0]])
    return np.array([0, len(xyz)], np.int32), xyz, x, np.zeros(1, np.float32), len(xyz), cell[None], layers * d


def load_slab(system):
    """(name, offsets, xyz, x, Q, N, cells (B, 3, 3) with a zero third row, thickness)"""
    if system == "qm9slab":
        offsets, _, x, Q, N = synth.qm9_like_batch(B=1024, seed=0, N=29)
        rng = np.random.default_rng(0)
        L, thick, pts = 6.5, 5.0, []
        for n in np.diff(offsets):
            mol = np.zeros((0, 3))
            while len(mol) < n:
                p = rng.uniform(0, 1, 3) * [L, L, thick]
                v = mol - p
                v[:, :2] -= L * np.rint(v[:, :2] / L)
                if not len(mol) or (v * v).sum(1).min() >= 0.81:
                    mol = np.vstack([mol, p])
            pts.append(mol)
        cells = np.tile(np.diag(np.float32([L, L, 0])), (len(offsets) - 1, 1, 1))
        return "1024 QM9-sized square slabs of 6.5 A, N = 29", offsets, np.concatenate(pts).astype(np.float32), x, Q, N, cells, thick
    if system.startswith("slab"):
        n = int(system[4:])
        nx = {2048: 32, 10000: 50}.get(n)
        if nx is None or n % (4 * nx):
            raise SystemExit("slab systems: slab2048 (32 x 16 x 4) and slab10000 (50 x 50 x 4)")
        o, xyz, x, Q, N, cells, thick = lattice_slab(nx, n // (4 * nx), 4, seed=0)
        return (f"{n} atoms, slab of {float(cells[0][0, 0]):.2f} x {float(cells[0][1, 1]):.2f} A, {thick:.2f} A thick", o, xyz, x, Q, N, cells, thick)
    raise SystemExit(f"unknown system {system}")


def slab_slots(cells, rows):
    """the listed slots of the batch: the half plane m1 > 0, or m1 == 0 and m0 > 0, inside kc (cells open along z)"""
    total = 0
    for c, r in zip(cells, rows):
        m0, m1 = np.meshgrid(np.arange(-r[3], r[3] + 1), np.arange(0, r[4] + 1), indexing="ij")
        k = 2 * np.pi * np.sqrt((m0 / float(c[0, 0])) ** 2 + (m1 / float(c[1, 1])) ** 2)
        total += int(((k <= r[2]) & ((m1 > 0) | (m0 > 0))).sum())
    return total


def main_slab(eng, T, systems, rounds, alpha, tol, cutoff=3.0):
    for system in systems:
        name, offsets, xyz, x, Q, N, cells, thick = load_slab(system)
        A = int(offsets[-1])
        rows = np.stack([eng.ewald_slab_params(c, alpha, tol) for c in cells])
        slots = slab_slots(cells, rows)
        if "--trace" in sys.argv:
            for _ in range(3):
                eng.coulomb_xyz_slab(offsets, xyz, x, Q, N, cell=cells, alpha=alpha, ewald=rows)
            print(json.dumps({"workload": name, "atoms": A, "calls": 3, "alpha": alpha, "tol": tol, "k_slots": slots}), flush=True)
            continue
        padded = cells.copy()
        padded[:, 2, 2] = max(3.0 * thick, 2.0 * cutoff)
        rows3 = np.stack([eng.ewald_params(c, alpha, tol) for c in padded])
        g = np.random.default_rng(0).normal(size=A).astype(np.float32)
        calls = {"coulomb_slab": lambda: eng.coulomb_xyz_slab(offsets, xyz, x, Q, N, cell=cells, alpha=alpha, ewald=rows, parts=True),
                 "gradient": lambda: eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, cell=cells),
                 "coulomb_cell_padded": lambda: eng.coulomb_xyz_cell(offsets, xyz, x, Q, N, cell=padded, alpha=alpha, ewald=rows3, parts=True)}
        for fn in calls.values():
            fn()
        times = {k: [] for k in calls}
        outs = {}
        for _ in range(rounds):
            for k, fn in calls.items():
                t, outs[k] = window(fn)
                times[k].append(t * 1e3)
        q, phi, E, F, ffix, fq = outs["coulomb_slab"]
        st = eng.last_stats() if calls["coulomb_slab"]() else None
        seeded = eng.charges_vjp_xyz(offsets, xyz, x, Q, phi, N, cell=cells)
        med = {k: float(np.median(t)) for k, t in times.items()}
        ns = [int(n) for n in np.diff(offsets)]
        line = {"workload": name, "atoms": A, "cells": len(cells), "near_pairs": int(st[0]), "rounds": rounds, "alpha": alpha, "tol": tol,
                "k_slots": slots, "ewald_first_cell": [round(float(v), 4) for v in rows[0]], "padded_third_vector": float(padded[0, 2, 2]),
                "padded_k_slots": int(((2 * rows3[:, 3] + 1) * (2 * rows3[:, 4] + 1) * (rows3[:, 5] + 1)).sum())}
        for k, t in times.items():
            line[k + "_ms_median"] = round(med[k], 3)
            line[k + "_ms_range"] = [round(min(t), 3), round(max(t), 3)]
        line.update({"slab_over_gradient": round(med["coulomb_slab"] / med["gradient"], 3),
                     "slab_over_padded_cell": round(med["coulomb_slab"] / med["coulomb_cell_padded"], 3), "slab_scratch_bytes": int(st[2]),
                     "slab_scratch_formula_bytes": scratch_formula(ns, int(st[0]), 9, T) + 88 * A * max(map(cl_pieces, ns)) + 304 * len(ns) + 56 * slots,
                     "q_bits_equal_gradient_call": bool(np.array_equal(q, outs["gradient"][0])),
                     "fq_bits_equal_minus_gxyz_of_phi": bool(np.array_equal(fq, -seeded[1])),
                     "energy_sum": float(E.sum()), "energy_sum_padded_cell": float(outs["coulomb_cell_padded"][2].sum()),
                     "max_abs_f": float(np.abs(F).max()), "max_abs_ffix": float(np.abs(ffix).max()), "max_abs_fq": float(np.abs(fq).max()),
                     "max_abs_sum_f": float(np.abs(F.sum(0, dtype=np.float64)).max())})
        print(json.dumps(line), flush=True)


def main_slab_strain(eng, T, systems, rounds, alpha, tol, against):
    other = {}
    if against:
        for text in open(against):
            if text.startswith("{"):
                rec = json.loads(text)
                other[rec["workload"]] = rec
    for system in systems:
        name, offsets, xyz, x, Q, N, cells, thick = load_slab(system)
        A = int(offsets[-1])
        rows = np.stack([eng.ewald_slab_params(c, alpha, tol) for c in cells])
        slots = slab_slots(cells, rows)
        if "--trace" in sys.argv:
            for _ in range(3):
                eng.coulomb_xyz_slab_strain(offsets, xyz, x, Q, N, cell=cells, alpha=alpha, ewald=rows)
            print(json.dumps({"workload": name, "atoms": A, "calls": 3, "alpha": alpha, "tol": tol, "k_slots": slots}), flush=True)
            continue
        calls = {"coulomb_slab": lambda: eng.coulomb_xyz_slab(offsets, xyz, x, Q, N, cell=cells, alpha=alpha, ewald=rows, parts=True),
                 "coulomb_slab_strain": lambda: eng.coulomb_xyz_slab_strain(offsets, xyz, x, Q, N, cell=cells, alpha=alpha, ewald=rows, parts=True)}
        for fn in calls.values():
            fn()
        times = {k: [] for k in calls}
        outs = {}
        for _ in range(rounds):
            for k, fn in calls.items():
                t, outs[k] = window(fn)
                times[k].append(t * 1e3)
        q, phi, E, F, gs, ffix, fq, gs_fix, gs_q = outs["coulomb_slab_strain"]
        st = eng.last_stats() if calls["coulomb_slab_strain"]() else None
        seeded = eng.charges_vjp_xyz(offsets, xyz, x, Q, phi, N, cell=cells, strain=True)
        med = {k: float(np.median(t)) for k, t in times.items()}
        ns = [int(n) for n in np.diff(offsets)]
        cp = max(map(cl_pieces, ns))
        line = {"workload": name, "atoms": A, "cells": len(cells), "near_pairs": int(st[0]), "rounds": rounds, "alpha": alpha, "tol": tol,
                "k_slots": slots}
        for k, t in times.items():
            line[k + "_ms_median"] = round(med[k], 3)
            line[k + "_ms_range"] = [round(min(t), 3), round(max(t), 3)]
        line["strain_over_plain"] = round(med["coulomb_slab_strain"] / med["coulomb_slab"], 3)
        if name in other:
            line["parent_plain_ms_median"] = other[name]["coulomb_slab_ms_median"]
            line["plain_over_parent"] = round(med["coulomb_slab"] / other[name]["coulomb_slab_ms_median"], 3)
        line.update({"strain_scratch_bytes": int(st[2]),
                     "strain_scratch_formula_bytes": scratch_formula(ns, int(st[0]), 9, T) + 88 * A * cp + 304 * len(ns) + 56 * slots
                     + 48 * A * cp + 48 * A + 36 * len(ns),
                     "six_outputs_bits_equal_plain_call": bool(all(np.array_equal(a, b) for a, b in zip((q, phi, E, F, ffix, fq), outs["coulomb_slab"]))),
                     "gstrain_q_bits_equal_gs_of_phi": bool(np.array_equal(gs_q, seeded[2])),
                     "gstrain_is_the_float32_sum_and_symmetric": bool(np.array_equal(gs, gs_fix + gs_q) and np.array_equal(gs, gs.transpose(0, 2, 1))),
                     "max_abs_gstrain_fix": float(np.abs(gs_fix).max()), "max_abs_gstrain_q": float(np.abs(gs_q).max())})
        print(json.dumps(line), flush=True)


def exclusion_list(offsets, xyz, cells, near):
    """Every pair of a molecule nearer than `near` (minimum image in a cubic cell), factors cycling in sorted order; shuffled."""
    from scipy.spatial import cKDTree
    out = []
    for b in range(len(offsets) - 1):
        a0, a1 = int(offsets[b]), int(offsets[b + 1])
        if a1 - a0 < 2:
            continue
        r = xyz[a0:a1].astype(np.float64)
        if cells is None:
            tree = cKDTree(r)
        else:
            L = float(cells[b][0, 0])
            assert np.array_equal(cells[b], np.diag([cells[b][0, 0]] * 3)), "the list maker takes cubic cells"
            tree = cKDTree(r - L * np.floor(r / L), boxsize=L)
        p = tree.query_pairs(near, output_type="ndarray")
        if len(p):
            out.append(np.sort(p, 1) + a0)
    pairs = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
    scale = np.float32([0.0, 0.5, 0.8333])[np.arange(len(pairs)) % 3]
    rng = np.random.default_rng(11)
    o = rng.permutation(len(pairs))
    pairs, scale = pairs[o], scale[o]
    swap = rng.permutation(len(pairs))[:len(pairs) // 2]
    pairs[swap] = pairs[swap][:, ::-1]
    return np.ascontiguousarray(pairs.astype(np.int32)), scale


def main_excl(eng, systems, rounds, alpha, tol, near, cell_mode):
    for system in systems:
        if cell_mode:
            name, offsets, xyz, x, Q, N, cells = load_cell(system)
            rows = np.stack([eng.ewald_params(c, alpha, tol) for c in cells])
            kw = dict(cell=cells, alpha=alpha, ewald=rows, parts=True, strain=True)
            plain_fn, excl_fn = eng.coulomb_xyz_cell, eng.coulomb_xyz_cell_excl
        else:
            name, offsets, xyz, x, Q, N = load(system)
            cells, kw = None, dict(alpha=alpha, parts=True)
            plain_fn, excl_fn = eng.coulomb_xyz, eng.coulomb_xyz_excl
        A = int(offsets[-1])
        ex = exclusion_list(offsets, xyz, cells, near)
        P = len(ex[0])
        if "--trace" in sys.argv:
            for _ in range(3):
                excl_fn(offsets, xyz, x, Q, N, exclusions=ex, **kw)
            print(json.dumps({"workload": name, "atoms": A, "calls": 3, "alpha": alpha, "listed_pairs": P}), flush=True)
            continue
        calls = {"plain": lambda: plain_fn(offsets, xyz, x, Q, N, **kw), "excl": lambda: excl_fn(offsets, xyz, x, Q, N, exclusions=ex, **kw)}
        for fn in calls.values():
            fn()
        times = {k: [] for k in calls}
        outs, stats = {}, {}
        for _ in range(rounds):
            for k, fn in calls.items():
                t, outs[k] = window(fn)
                stats[k] = eng.last_stats()
                times[k].append(t * 1e3)
        phi, fq = outs["excl"][1], outs["excl"][6 if cell_mode else 5]
        seeded = eng.charges_vjp_xyz(offsets, xyz, x, Q, phi, N, **({"cell": cells, "strain": True} if cell_mode else {}))
        med = {k: float(np.median(t)) for k, t in times.items()}
        line = {"workload": name, "atoms": A, "listed_pairs": P, "pairs_per_atom": round(P / A, 2), "near": near, "rounds": rounds, "alpha": alpha}
        for k, t in times.items():
            line[k + "_ms_median"] = round(med[k], 3)
            line[k + "_ms_range"] = [round(min(t), 3), round(max(t), 3)]
        line.update({"excl_over_plain": round(med["excl"] / med["plain"], 4), "scratch_bytes_added": int(stats["excl"][2]) - int(stats["plain"][2]),
                     "scratch_formula_added": (A + 1) * 4 + 16 * P + A * (80 if cell_mode else 32),
                     "q_bits_equal_plain_call": bool(np.array_equal(outs["excl"][0], outs["plain"][0])),
                     "fq_bits_equal_minus_gxyz_of_phi": bool(np.array_equal(fq, -seeded[1])),
                     "max_abs_phi_plain": float(np.abs(outs["plain"][1]).max()), "max_abs_phi_excl": float(np.abs(phi).max()),
                     "energy_sum_plain": float(outs["plain"][2].sum()), "energy_sum_excl": float(outs["excl"][2].sum())})
        print(json.dumps(line), flush=True)


# widths (A), electronegativities and hardnesses (eV, eV / e^2) by element for --site: round numbers of the size such models fit
SITE_SIGMA = {1: 0.45, 6: 0.75, 7: 0.70, 8: 0.65, 9: 0.60, 15: 1.05, 16: 1.00, 17: 0.95, 35: 1.15}
SITE_CHI = {1: -1.0, 6: 0.2, 7: 1.1, 8: 1.9, 9: 2.6, 15: -0.2, 16: 0.6, 17: 1.6, 35: 1.3}
SITE_J = {1: 13.0, 6: 10.0, 7: 11.5, 8: 12.5, 9: 14.0, 15: 8.0, 16: 8.5, 17: 9.5, 35: 8.5}


def main_site(eng, systems, rounds, alpha, tol, near, cell_mode):
    from epnn_amd.engine import per_element
    for system in systems:
        if cell_mode:
            name, offsets, xyz, x, Q, N, cells = load_cell(system)
            rows = np.stack([eng.ewald_params(c, 0.0, tol) for c in cells])
            rows_excl = np.stack([eng.ewald_params(c, alpha, tol) for c in cells])
            kw, kw_excl = dict(cell=cells, ewald=rows, parts=True, strain=True), dict(cell=cells, ewald=rows_excl, parts=True, strain=True)
            site_fn, excl_fn = eng.coulomb_xyz_cell_site, eng.coulomb_xyz_cell_excl
        else:
            name, offsets, xyz, x, Q, N = load(system)
            cells, kw = None, dict(parts=True)
            kw_excl = kw
            site_fn, excl_fn = eng.coulomb_xyz_site, eng.coulomb_xyz_excl
        A, B = int(offsets[-1]), len(offsets) - 1
        sigma, chi, J = (per_element(x[:, 0], t) for t in (SITE_SIGMA, SITE_CHI, SITE_J))
        if cell_mode:
            sigma = (sigma * np.float32(0.9 * 0.5 / rows[:, 0].max() / max(SITE_SIGMA.values()))).astype(np.float32)
        ex = exclusion_list(offsets, xyz, cells, near)
        P = len(ex[0])
        site_kw = dict(sigma=sigma, chi=chi, hardness=J, self_energy=True, exclusions=ex, **kw)
        if "--trace" in sys.argv:
            for _ in range(3):
                site_fn(offsets, xyz, x, Q, N, **site_kw)
            print(json.dumps({"workload": name, "atoms": A, "calls": 3, "listed_pairs": P}), flush=True)
            continue
        calls = {"excl": lambda: excl_fn(offsets, xyz, x, Q, N, alpha=alpha, exclusions=ex, **kw_excl),
                 "site": lambda: site_fn(offsets, xyz, x, Q, N, **site_kw)}
        for fn in calls.values():
            fn()
        times = {k: [] for k in calls}
        outs, stats = {}, {}
        for _ in range(rounds):
            for k, fn in calls.items():
                t, outs[k] = window(fn)
                stats[k] = eng.last_stats()
                times[k].append(t * 1e3)
        mu, fq = outs["site"][2], outs["site"][7 if cell_mode else 6]
        seeded = eng.charges_vjp_xyz(offsets, xyz, x, Q, mu, N, **({"cell": cells, "strain": True} if cell_mode else {}))
        med = {k: float(np.median(t)) for k, t in times.items()}
        line = {"workload": name, "atoms": A, "listed_pairs": P, "near": near, "rounds": rounds, "alpha_of_the_excl_call": alpha,
                "sigma_range": [round(float(sigma.min()), 4), round(float(sigma.max()), 4)]}
        for k, t in times.items():
            line[k + "_ms_median"] = round(med[k], 3)
            line[k + "_ms_range"] = [round(min(t), 3), round(max(t), 3)]
        line.update({"site_over_excl": round(med["site"] / med["excl"], 4), "scratch_bytes_added": int(stats["site"][2]) - int(stats["excl"][2]),
                     "scratch_formula_added": 20 * A + (8 * B if cell_mode else 0),
                     "q_bits_equal_excl_call": bool(np.array_equal(outs["site"][0], outs["excl"][0])),
                     "fq_bits_equal_minus_gxyz_of_mu": bool(np.array_equal(fq, -seeded[1])),
                     "max_abs_phi": float(np.abs(outs["site"][1]).max()), "max_abs_mu": float(np.abs(mu).max()),
                     "energy_sum_excl": float(outs["excl"][2].sum()), "energy_sum_site": float(outs["site"][3].sum())})
        if cell_mode:
            line["gstrain_q_bits_equal_gstrain_of_mu"] = bool(np.array_equal(outs["site"][9], seeded[2]))
        print(json.dumps(line), flush=True)


def exclusion_list_slab(offsets, xyz, cells, near):
    """exclusion_list for rectangular slab cells open along z: every pair of a cell nearer than `near` through the in-plane minimum image"""
    from scipy.spatial import cKDTree
    out = []
    for b in range(len(offsets) - 1):
        a0, a1 = int(offsets[b]), int(offsets[b + 1])
        if a1 - a0 < 2:
            continue
        c = cells[b]
        assert np.array_equal(c, np.diag([c[0, 0], c[1, 1], 0])), "the list maker takes rectangular slab cells open along z"
        L = np.float64([c[0, 0], c[1, 1], 1e6])
        r = xyz[a0:a1].astype(np.float64)
        r[:, 2] -= r[:, 2].min()
        r[:, :2] -= L[:2] * np.floor(r[:, :2] / L[:2])
        p = cKDTree(r, boxsize=L).query_pairs(near, output_type="ndarray")
        if len(p):
            out.append(np.sort(p, 1) + a0)
    pairs = np.concatenate(out) if out else np.zeros((0, 2), np.int64)
    pairs = pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]
    scale = np.float32([0.0, 0.5, 0.8333])[np.arange(len(pairs)) % 3]
    rng = np.random.default_rng(11)
    o = rng.permutation(len(pairs))
    pairs, scale = pairs[o], scale[o]
    swap = rng.permutation(len(pairs))[:len(pairs) // 2]
    pairs[swap] = pairs[swap][:, ::-1]
    return np.ascontiguousarray(pairs.astype(np.int32)), scale


def main_slab_site(eng, systems, rounds, tol, near, strain):
    """--slab --site [--strain]: coulomb_xyz_slab_site beside coulomb_xyz_slab (or, with --strain, the two strain entries) with the same
    list, alternating on one handle.  Widths by element, scaled down where the widest Gaussian would exceed 0.9 of 1 / (2 beta_max)."""
    from epnn_amd.engine import per_element
    for system in systems:
        name, offsets, xyz, x, Q, N, cells, thick = load_slab(system)
        A = int(offsets[-1])
        rows = np.stack([eng.ewald_slab_params(c, 0.0, tol) for c in cells])
        sigma, chi, J = (per_element(x[:, 0], t) for t in (SITE_SIGMA, SITE_CHI, SITE_J))
        sigma = (sigma * np.float32(min(1.0, 0.9 * 0.5 / rows[:, 0].max() / max(SITE_SIGMA.values())))).astype(np.float32)
        ex = exclusion_list_slab(offsets, xyz, cells, near)
        P = len(ex[0])
        kw = dict(cell=cells, ewald=rows, parts=True, exclusions=ex)
        plain_fn = eng.coulomb_xyz_slab_strain if strain else eng.coulomb_xyz_slab
        site_kw = dict(sigma=sigma, chi=chi, hardness=J, self_energy=True, strain=strain, **kw)
        if "--trace" in sys.argv:
            for _ in range(3):
                eng.coulomb_xyz_slab_site(offsets, xyz, x, Q, N, **site_kw)
            print(json.dumps({"workload": name, "atoms": A, "calls": 3, "listed_pairs": P, "strain": strain}), flush=True)
            continue
        calls = {"slab": lambda: plain_fn(offsets, xyz, x, Q, N, **kw), "site": lambda: eng.coulomb_xyz_slab_site(offsets, xyz, x, Q, N, **site_kw)}
        for fn in calls.values():
            fn()
        times = {k: [] for k in calls}
        outs, stats = {}, {}
        for _ in range(rounds):
            for k, fn in calls.items():
                t, outs[k] = window(fn)
                stats[k] = eng.last_stats()
                times[k].append(t * 1e3)
        mu, fq = outs["site"][2], outs["site"][7 if strain else 6]
        seeded = eng.charges_vjp_xyz(offsets, xyz, x, Q, mu, N, cell=cells, strain=True)
        med = {k: float(np.median(t)) for k, t in times.items()}
        line = {"workload": name, "atoms": A, "cells": len(cells), "strain": strain, "listed_pairs": P, "near": near, "rounds": rounds, "tol": tol,
                "k_slots": slab_slots(cells, rows), "sigma_range": [round(float(sigma.min()), 4), round(float(sigma.max()), 4)]}
        for k, t in times.items():
            line[k + "_ms_median"] = round(med[k], 3)
            line[k + "_ms_range"] = [round(min(t), 3), round(max(t), 3)]
        line.update({"site_over_slab": round(med["site"] / med["slab"], 4), "scratch_bytes_added": int(stats["site"][2]) - int(stats["slab"][2]),
                     "scratch_formula_added": 20 * A, "q_bits_equal_slab_call": bool(np.array_equal(outs["site"][0], outs["slab"][0])),
                     "fq_bits_equal_minus_gxyz_of_mu": bool(np.array_equal(fq, -seeded[1])),
                     "max_abs_phi": float(np.abs(outs["site"][1]).max()), "max_abs_mu": float(np.abs(mu).max()),
                     "energy_sum_slab": float(outs["slab"][2].sum()), "energy_sum_site": float(outs["site"][3].sum())})
        if strain:
            line["gstrain_q_bits_equal_gstrain_of_mu"] = bool(np.array_equal(outs["site"][9], seeded[2]))
        print(json.dumps(line), flush=True)


def main_cell(eng, T, systems, rounds, alpha, tol):
    for system in systems:
        name, offsets, xyz, x, Q, N, cells = load_cell(system)
        A = int(offsets[-1])
        rows = np.stack([eng.ewald_params(c, alpha, tol) for c in cells])
        slots = int(((2 * rows[:, 3] + 1) * (2 * rows[:, 4] + 1) * (rows[:, 5] + 1)).sum())
        if "--trace" in sys.argv:
            for _ in range(3):
                eng.coulomb_xyz_cell(offsets, xyz, x, Q, N, cell=cells, alpha=alpha, ewald=rows)
            print(json.dumps({"workload": name, "atoms": A, "calls": 3, "alpha": alpha, "tol": tol, "k_slots": slots}), flush=True)
            continue
        g = np.random.default_rng(0).normal(size=A).astype(np.float32)
        calls = {"coulomb_cell": lambda: eng.coulomb_xyz_cell(offsets, xyz, x, Q, N, cell=cells, alpha=alpha, ewald=rows, parts=True, strain=True),
                 "gradient": lambda: eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, cell=cells, strain=True)}
        for fn in calls.values():
            fn()
        times = {k: [] for k in calls}
        outs = {}
        for _ in range(rounds):
            for k, fn in calls.items():
                t, outs[k] = window(fn)
                times[k].append(t * 1e3)
        q, phi, E, F, gs, ffix, fq, gs_fix, gs_q = outs["coulomb_cell"]
        st = eng.last_stats() if calls["coulomb_cell"]() else None
        seeded = eng.charges_vjp_xyz(offsets, xyz, x, Q, phi, N, cell=cells, strain=True)
        sg = eng.last_stats()
        med = {k: float(np.median(t)) for k, t in times.items()}
        line = {"workload": name, "atoms": A, "cells": len(cells), "near_pairs": int(st[0]), "rounds": rounds, "alpha": alpha, "tol": tol,
                "k_slots": slots, "ewald_first_cell": [round(float(v), 4) for v in rows[0]]}
        for k, t in times.items():
            line[k + "_ms_median"] = round(med[k], 3)
            line[k + "_ms_range"] = [round(min(t), 3), round(max(t), 3)]
        line.update({"coulomb_cell_over_gradient": round(med["coulomb_cell"] / med["gradient"], 3), "coulomb_cell_scratch_bytes": int(st[2]),
                     "gradient_scratch_bytes": int(sg[2]), "q_bits_equal_gradient_call": bool(np.array_equal(q, outs["gradient"][0])),
                     "fq_bits_equal_minus_gxyz_of_phi": bool(np.array_equal(fq, -seeded[1])),
                     "gstrain_q_bits_equal_gstrain_of_phi": bool(np.array_equal(gs_q, seeded[2])),
                     "energy_sum": float(E.sum()), "max_abs_f": float(np.abs(F).max()), "max_abs_ffix": float(np.abs(ffix).max()),
                     "max_abs_fq": float(np.abs(fq).max()), "max_abs_sum_f": float(np.abs(F.sum(0, dtype=np.float64)).max()),
                     "max_abs_gstrain": float(np.abs(gs).max())})
        print(json.dumps(line), flush=True)


def main():
    arg = lambda name, default: sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default
    cell_mode = "--cell" in sys.argv
    slab_mode = "--slab" in sys.argv
    systems = arg("--systems", "qm9slab,slab2048,slab10000" if slab_mode else "qm9cell,cell10000,cell100000" if cell_mode
                  else "protein,cluster10000,qm9").split(",")
    rounds, alpha = int(arg("--rounds", "5")), float(arg("--alpha", "0.0"))
    w = checkpoint.load_epnn_weights(os.path.join(ROOT, "models/decay_model_weights"))
    T = len(w["msg"])
    eng = Engine(nx=9, T=T)
    eng.set_weights(w)
    eng.set_option("grad_path", 2)
    if slab_mode and "--site" in sys.argv:
        main_slab_site(eng, systems, rounds, float(arg("--tol", "1e-6")), float(arg("--near", "2.2")), "--strain" in sys.argv)
        eng.close()
        return
    if slab_mode and "--strain" in sys.argv:
        main_slab_strain(eng, T, systems, rounds, alpha, float(arg("--tol", "1e-6")), arg("--against", None))
        eng.close()
        return
    if slab_mode:
        main_slab(eng, T, systems, rounds, alpha, float(arg("--tol", "1e-6")))
        eng.close()
        return
    if "--site" in sys.argv:
        main_site(eng, systems, rounds, alpha, float(arg("--tol", "1e-6")), float(arg("--near", "2.2")), cell_mode)
        eng.close()
        return
    if "--excl" in sys.argv:
        main_excl(eng, systems, rounds, alpha, float(arg("--tol", "1e-6")), float(arg("--near", "2.2")), cell_mode)
        eng.close()
        return
    if cell_mode:
        main_cell(eng, T, systems, rounds, alpha, float(arg("--tol", "1e-6")))
        eng.close()
        return
    for system in systems:
        name, offsets, xyz, x, Q, N = load(system)
        A = int(offsets[-1])
        if "--trace" in sys.argv:
            for _ in range(3):
                eng.coulomb_xyz(offsets, xyz, x, Q, N, alpha=alpha)
            print(json.dumps({"workload": name, "atoms": A, "calls": 3, "alpha": alpha}), flush=True)
            continue
        g = np.random.default_rng(0).normal(size=A).astype(np.float32)
        calls = {"coulomb": lambda: eng.coulomb_xyz(offsets, xyz, x, Q, N, alpha=alpha, parts=True),
                 "gradient": lambda: eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N)}
        for fn in calls.values():                                    # warm-up: code objects, scratch of the largest call
            fn()
        times = {k: [] for k in calls}
        outs = {}
        for _ in range(rounds):
            for k, fn in calls.items():
                t, outs[k] = window(fn)
                times[k].append(t * 1e3)
        q, phi, E, F, ffix, fq = outs["coulomb"]
        st = eng.last_stats() if calls["coulomb"]() else None
        seeded = eng.charges_vjp_xyz(offsets, xyz, x, Q, phi, N)
        sg = eng.last_stats()
        med = {k: float(np.median(t)) for k, t in times.items()}
        ns = [int(n) for n in np.diff(offsets)]
        line = {"workload": name, "atoms": A, "molecules": len(ns), "near_pairs": int(st[0]), "rounds": rounds, "alpha": alpha}
        for k, t in times.items():
            line[k + "_ms_median"] = round(med[k], 3)
            line[k + "_ms_range"] = [round(min(t), 3), round(max(t), 3)]
        line.update({"coulomb_over_gradient": round(med["coulomb"] / med["gradient"], 3), "coulomb_scratch_bytes": int(st[2]),
                     "coulomb_scratch_formula_bytes": scratch_formula(ns, int(st[0]), 9, T), "gradient_scratch_bytes": int(sg[2]),
                     "q_bits_equal_gradient_call": bool(np.array_equal(q, outs["gradient"][0])),
                     "fq_bits_equal_minus_gxyz_of_phi": bool(np.array_equal(fq, -seeded[1])),
                     "energy_sum": float(E.sum()), "max_abs_f": float(np.abs(F).max()), "max_abs_ffix": float(np.abs(ffix).max()),
                     "max_abs_fq": float(np.abs(fq).max()), "max_abs_sum_f": float(np.abs(F.sum(0, dtype=np.float64)).max())})
        print(json.dumps(line), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
