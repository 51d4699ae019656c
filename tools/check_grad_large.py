#!/usr/bin/env python3
"""Small-system check of the charge gradients from the pair list ("grad_path" = 2): errors of both paths against the float64
restatement tests/grad_large_ref.py and the time of the first blocking call of each size (allocation included), on lattice
molecules of 40 / 97 / 300 atoms, a 200-atom periodic box and a 200-atom sheared cell with strain; random weights, T = 2.
    python tools/check_grad_large.py          (its output is the first part of profiles/r09_grad_large.txt)
stats = epnn_last_stats after the pair-list call: [listed pairs, 0, bytes of device scratch, 0]."""
import os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import random_weights
from test_grad_large_ref import _lattice_molecule, _features
from xyz_grad_ref import vjp64
import periodic_ref, cell_ref
from grad_large_ref import vjp64_large
from epnn_amd.engine import Engine

def report(tag, got, ref):
    print(f"{tag}: err {np.abs(got-ref).max():.3e} scale {np.abs(ref).max():.3e}", flush=True)

w = random_weights(9, 2, seed=5, scale=0.6)
eng = Engine(nx=9, T=2); eng.set_weights(w)
for n, N in ((40, 40), (97, 101), (300, 320)):
    xyz, x, Q = _lattice_molecule(n, 9, seed=n)
    g = np.random.default_rng(n).normal(size=n).astype(np.float32)
    off = np.int32([0, n]); Qa = np.float32([Q])
    eng.set_option("grad_path", 1); q1, g1 = eng.charges_vjp_xyz(off, xyz, x, Qa, g, N)
    eng.set_option("grad_path", 2); t0 = time.time(); q2, g2 = eng.charges_vjp_xyz(off, xyz, x, Qa, g, N); dt = time.time() - t0
    qr, gr = vjp64_large(xyz, x, Q, g.astype(np.float64), w, N=N)
    print(f"n={n} N={N} call {dt*1e3:.2f} ms stats {eng.last_stats()}")
    report("  q  path2 vs ref", q2, qr); report("  q  path1 vs ref", q1, qr)
    report("  gx path2 vs ref", g2, gr); report("  gx path1 vs ref", g1, gr)
    q2b, g2b = eng.charges_vjp_xyz(off, xyz, x, Qa, g, N)
    print("  deterministic", np.array_equal(q2, q2b) and np.array_equal(g2, g2b))
rng = np.random.default_rng(1)
L = np.float32([11, 11.5, 12]); n = 200
xyz = periodic_ref.random_cell(rng, n, L); x, Q = _features(rng, n, 9); g = rng.normal(size=n).astype(np.float32)
q2, g2 = eng.charges_vjp_xyz(np.int32([0, n]), xyz, x, np.float32([Q]), g, n, box=L)
qr, gr = vjp64_large(xyz, x, Q, g.astype(np.float64), w, box=L)
report("box q", q2, qr); report("box gx", g2, gr)
cell = cell_ref.BASIS_A
xyz = cell_ref.random_cell(rng, n, cell)
q2, g2, s2 = eng.charges_vjp_xyz(np.int32([0, n]), xyz, x, np.float32([Q]), g, n, cell=cell, strain=True)
qr, gr, sr = vjp64_large(xyz, x, Q, g.astype(np.float64), w, cell=cell, strain=True)
report("cell q", q2, qr); report("cell gx", g2, gr); report("cell strain", s2[0], sr)
eng.set_option("grad_path", 1)
q1, g1, s1 = eng.charges_vjp_xyz(np.int32([0, n]), xyz, x, np.float32([Q]), g, n, cell=cell, strain=True)
report("cell gx path1", g1, gr); report("cell strain path1", s1[0], sr)
