"""Float64 reference for bonded exclusions and pair scaling in the Coulomb calls (epnn_coulomb_xyz_excl, epnn_coulomb_xyz_cell_excl).
Test helper.

A listed pair (i, j) with factor s interacts with weight s instead of 1.  Open molecules: coulomb_ref.coulomb64 with w_ij applied.
Cells: ewald_ref.ewald64 over all pairs and images as it is, plus, for the one minimum image d (cell_ref.mic64) of each listed pair,
    phi_i += ke (s - 1) q_j kappa_alpha(D);  ffix_i -= ke (s - 1) q_i q_j kappa_alpha'(D) d / D;
    strain += ke (s - 1) q_i q_j kappa_alpha'(D) d_a d_b / D  once per pair;  E = 1/2 sum q_i phi_i
with the bare kappa_alpha = e_alpha(D) / D of coulomb_ref.kappa64 (no beta in it).  Beside every result the sum of the absolute
values of the terms actually added: an excluded pair's full term is added by the all-pairs sum and taken away by the correction, so
both count.  exclusion_cases is the deterministic list rule of the GPU tests.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import cell_ref
from coulomb_ref import coulomb64, kappa64
from ewald_ref import ewald64  # noqa: F401  (the namespace excl_correction64's results are added to)

FACTORS = (0.0, 0.5, 0.8333)


def _lists(pairs, scale):
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    scale = np.asarray(scale, dtype=np.float32).astype(np.float64)              # (the library takes float32 factors)
    return pairs, (np.full(len(pairs), float(scale)) if scale.ndim == 0 else scale)


def excl_correction64(xyz, q, cell, ke, alpha, pairs, scale):
    """The listed pairs' correction of one molecule or cell (cell None: plain displacements), as a namespace: dphi (n,), dE, dffix
    (n, 3), dstrain (3, 3) and the sums of their absolute terms s_phi (n,), s_E, s_ffix (n,), s_strain (3, 3).  Factors are s, the
    terms carry s - 1 taken in float32 as the library takes it."""
    r = np.asarray(xyz, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    pairs, scale = _lists(pairs, scale)
    n = r.shape[0]
    out = SimpleNamespace(dphi=np.zeros(n), dE=0.0, dffix=np.zeros((n, 3)), dstrain=np.zeros((3, 3)), s_phi=np.zeros(n), s_E=0.0,
                          s_ffix=np.zeros(n), s_strain=np.zeros((3, 3)))
    if not len(pairs):
        return out
    i, j = pairs[:, 0], pairs[:, 1]
    f = (scale.astype(np.float32) - np.float32(1)).astype(np.float64)
    d = r[i] - r[j]
    if cell is not None:
        d = cell_ref.mic64(d, *cell_ref.duals64(np.asarray(cell, dtype=np.float64)))
    D = np.sqrt((d * d).sum(-1))
    kap, dkap = kappa64(D, alpha)
    np.add.at(out.dphi, i, ke * f * q[j] * kap)
    np.add.at(out.dphi, j, ke * f * q[i] * kap)
    np.add.at(out.s_phi, i, np.abs(ke * f * q[j] * kap))
    np.add.at(out.s_phi, j, np.abs(ke * f * q[i] * kap))
    t = ke * f * q[i] * q[j] * dkap                                              # ke (s - 1) q_i q_j kappa'
    np.add.at(out.dffix, i, -(t / D)[:, None] * d)
    np.add.at(out.dffix, j, (t / D)[:, None] * d)
    np.add.at(out.s_ffix, i, np.abs(t))
    np.add.at(out.s_ffix, j, np.abs(t))
    dd = d[:, :, None] * d[:, None, :]
    out.dstrain = ((t / D)[:, None, None] * dd).sum(0)
    out.s_strain = (np.abs(t / D)[:, None, None] * np.abs(dd)).sum(0)
    out.dE = float((ke * f * q[i] * q[j] * kap).sum())
    out.s_E = float(np.abs(ke * f * q[i] * q[j] * kap).sum())
    return out


def coulomb64_w(xyz, q, ke, alpha, pairs, scale):
    """coulomb64's tuple (phi, E, ffix, sum |terms of phi|, sum |ke q_i q_j kappa'|) of one open molecule with w_ij applied; the two
    absolute sums include the correction terms |(s - 1) term|."""
    phi, E, ffix, sp, sf = coulomb64(xyz, q, ke, alpha)
    c = excl_correction64(xyz, q, None, ke, alpha, pairs, scale)
    return phi + c.dphi, E + c.dE, ffix + c.dffix, sp + c.s_phi, sf + c.s_ffix


def add_correction(e, c, q):
    """ewald64's namespace with the correction added; the absolute sums go to the "real" part (the 2e-6 bound covers them)."""
    q = np.asarray(q, dtype=np.float64)
    s_phi, s_ffix, s_strain, s_E = dict(e.s_phi), dict(e.s_ffix), dict(e.s_strain), dict(e.s_E)
    s_phi["real"] = s_phi["real"] + c.s_phi
    s_ffix["real"] = s_ffix["real"] + c.s_ffix
    s_strain["real"] = s_strain["real"] + c.s_strain
    s_E["real"] = s_E["real"] + c.s_E
    phi = e.phi + c.dphi
    return SimpleNamespace(phi=phi, E=0.5 * float(q @ phi), ffix=e.ffix + c.dffix, strain=e.strain + c.dstrain, s_phi=s_phi, s_E=s_E,
                           s_ffix=s_ffix, s_strain=s_strain)


def pair_shifts(xyz, cell, pairs):
    """The lattice shift n (P, 3) of each listed pair's minimum image, d = (r_i - r_j) - n a."""
    r = np.asarray(xyz, dtype=np.float64)
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    a, g = cell_ref.duals64(np.asarray(cell, dtype=np.float32).astype(np.float64))
    return np.rint((r[pairs[:, 0]] - r[pairs[:, 1]]) @ g.T)


def exclusion_cases(xyz, cell=None, near=2.0, most=12):
    """The list rule for one molecule or cell of n atoms (local indices), deterministic: every pair with minimum-image (or plain)
    D < near, factors cycling through FACTORS in sorted pair order; atom 0 at factor 0 with up to `most` of its nearest neighbours,
    in cells those within 0.95 w_min / 2; for n >= 3 every pair that holds the last atom dropped.  Returns (pairs (P, 2) int32 with
    i < j, sorted, scale (P,) float32); empty for n < 2."""
    r = np.asarray(xyz, dtype=np.float64)
    n = r.shape[0]
    if n < 2:
        return np.zeros((0, 2), dtype=np.int32), np.zeros((0,), dtype=np.float32)
    d = r[:, None, :] - r[None, :, :]
    limit = np.inf
    if cell is not None:
        d = cell_ref.mic64(d, *cell_ref.duals(cell))
        limit = 0.95 * 0.5 * cell_ref.widths(cell).min()
    D = np.sqrt((d * d).sum(-1))
    table = {}
    k = 0
    for i in range(n):
        for j in range(i + 1, n):
            if D[i, j] < near:
                table[i, j] = FACTORS[k % len(FACTORS)]
                k += 1
    order = [j for j in np.argsort(D[0], kind="stable") if j != 0 and D[0, j] <= limit][:most]
    for j in order:
        table[0, int(j)] = 0.0
    if n >= 3:
        table = {p: s for p, s in table.items() if n - 1 not in p}
    keys = sorted(table)
    return np.array(keys, dtype=np.int32).reshape(-1, 2), np.array([table[p] for p in keys], dtype=np.float32)


def shuffled(pairs, scale, seed=11):
    """The list as it is handed to the library: rows in a fixed random order, half of them swapped i <-> j."""
    rng = np.random.default_rng(seed)
    o = rng.permutation(len(pairs))
    p, s = np.asarray(pairs)[o].copy(), np.asarray(scale)[o].copy()
    swap = rng.permutation(len(p))[:len(p) // 2]
    p[swap] = p[swap][:, ::-1]
    return np.ascontiguousarray(p), s


def list_stats(n, pairs):
    """(most partners of one atom, atoms without any pair)."""
    deg = np.bincount(np.asarray(pairs, dtype=np.int64).reshape(-1), minlength=n)
    return int(deg.max()) if n else 0, int((deg == 0).sum())
