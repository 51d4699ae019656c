"""The float64 reference of the slab electrostatics (slab_ref.py) is pinned here before anything is compared with it: independence of
the splitting parameter within the three tol bounds of include/epnn.h, the constant of the square lattice, agreement with the fully
periodic Ewald sum in a cell padded with vacuum plus the Yeh-Berkowitz term, forces against central differences, a tilted plane with
the open row first, and alpha > 0 against the run without a real-space part.  CPU only."""
import math

import numpy as np
import pytest

from ewald_ref import ewald64, ewald_params64
from slab_ref import slab64, slab_geometry64, slab_params64

KE = 14.3996454784255
SHEARED = np.float32([[7, 0, 0], [2, 6.9, 0], [0, 0, 0]])
TILTED = np.float32([[0, 0, 0], [6.8, 1.0, 1.5], [-0.5, 6.0, 3.5]])             # the open row first, the plane tilted against every axis


def _slab(cell, n, seed, Q=0.0, thick=5.0):
    """n atoms uniform over the cell's two periodic rows and `thick` along its normal, on the float32 grid; charges of sum Q."""
    rng = np.random.default_rng(seed)
    a, _, per, _, _, nhat = slab_geometry64(cell)
    f = rng.uniform(0, 1, (n, 3))
    xyz = (f[:, :1] * a[per[0]] + f[:, 1:2] * a[per[1]] + thick * f[:, 2:] * nhat).astype(np.float32)
    q = rng.normal(size=n)
    return xyz, q - q.mean() + Q / n


def _at(xyz, q, cell, alpha, tol):
    p = slab_params64(cell, alpha, tol)
    return slab64(xyz, q, cell, KE, alpha, p[0], p[1], p[2], p[3:]), p


@pytest.mark.parametrize("Q", [0.0, 1.5])
def test_independent_of_beta_within_the_three_tol_bounds(Q):
    """tol = 1e-6 against 1e-10, neutral and charged: phi within tol ke beta sum|q|, E within tol 1/2 ke beta (sum|q|)^2 and ffix
    within tol ke beta^2 sum|q| max|q|.  The k = 0 term of a charged slab is the finite part of a sheet's potential: the constant that
    is dropped does not depend on beta."""
    xyz, q = _slab(SHEARED, 12, 3, Q)
    (lo, p), (hi, p10) = _at(xyz, q, SHEARED, 0.0, 1e-6), _at(xyz, q, SHEARED, 0.0, 1e-10)
    assert p10[0] > 1.2 * p[0] and p10[3] > p[3]
    beta, Qa, qm = p[0], np.abs(q).sum(), np.abs(q).max()
    assert abs(q.sum() - Q) < 1e-12
    assert np.abs(lo.phi - hi.phi).max() <= 1e-6 * KE * beta * Qa
    assert abs(lo.E - hi.E) <= 1e-6 * 0.5 * KE * beta * Qa * Qa
    assert np.abs(lo.ffix - hi.ffix).max() <= 1e-6 * KE * beta * beta * Qa * qm


def test_one_charge_in_a_square_cell_gives_the_lattice_constant():
    L = 6.5
    cell = np.diag(np.float32([L, L, 0]))
    e, _ = _at(np.zeros((1, 3)), np.ones(1), cell, 0.0, 1e-12)
    assert abs(e.phi[0] * L / KE + 3.9002649200) <= 1e-9
    assert np.abs(e.ffix).max() <= 1e-12
    low, _ = _at(np.zeros((1, 3)), np.ones(1), cell, 0.0, 1e-6)
    assert abs(low.phi[0] * L / KE + 3.9002649200) <= 1e-6 * L * slab_params64(cell, 0.0, 1e-6)[0]


def test_neutral_slab_equals_the_padded_3d_sum_plus_yeh_berkowitz():
    xyz, q = _slab(SHEARED, 12, 3)
    e, _ = _at(xyz, q, SHEARED, 0.0, 1e-12)
    cell3 = SHEARED.astype(np.float64)
    cell3[2] = [0, 0, 80.0]
    p3 = ewald_params64(cell3, 0.0, 1e-12)
    e3 = ewald64(xyz, q, cell3, KE, 0.0, p3[0], p3[1], p3[2], p3[3:])
    Mz = float(q @ xyz[:, 2].astype(np.float64))
    yb = KE * 2.0 * math.pi * Mz * Mz / abs(np.linalg.det(cell3))
    assert abs(Mz) > 0.1
    assert abs(e.E - (e3.E + yb)) <= 1e-9 * abs(e.E)


@pytest.mark.parametrize("cell,alpha", [(SHEARED, 0.0), (TILTED, 0.0), (TILTED, 0.7)])
def test_forces_are_minus_the_gradient_of_the_energy(cell, alpha):
    xyz, q = _slab(cell, 7, 11, 0.8)
    p = slab_params64(cell, alpha, 1e-10)
    r = xyz.astype(np.float64)
    e = slab64(r, q, cell, KE, alpha, p[0], p[1], p[2], p[3:])
    h = 1e-4
    for i in (0, 3, 6):
        for c in range(3):
            E = []
            for s in (-2, -1, 1, 2):
                rr = r.copy()
                rr[i, c] += s * h
                E.append(slab64(rr, q, cell, KE, alpha, p[0], p[1], p[2], p[3:]).E)
            fd = -(E[0] - 8 * E[1] + 8 * E[2] - E[3]) / (12 * h)
            assert abs(fd - e.ffix[i, c]) <= 1e-8 * max(1.0, np.abs(e.ffix).max()), (i, c)
    assert np.abs(e.ffix.sum(0)).max() <= 1e-9 * np.abs(e.ffix).sum()


def test_tilted_plane_with_alpha_against_the_run_without_a_real_space_part():
    """alpha = 2 in the tilted cell (open row first): tol = 1e-9 and 1e-12 agree to the tol bound, and the 1e-12 value equals the sum at
    beta == alpha, rc = 0, whose real-space term vanishes identically."""
    xyz, q = _slab(TILTED, 10, 5, 0.5)
    (e9, p9), (e12, p12) = _at(xyz, q, TILTED, 2.0, 1e-9), _at(xyz, q, TILTED, 2.0, 1e-12)
    assert p9[1] > 0 and p12[0] < 2.0 and p9[3] == 0 and p12[3] == 0
    Qa = np.abs(q).sum()
    assert abs(e9.E - e12.E) <= 1e-9 * 0.5 * KE * p9[0] * Qa * Qa
    s = math.sqrt(-math.log(1e-12))
    a = TILTED.astype(np.float64)
    kc = 2 * 2.0 * s
    M = np.ceil(kc * np.sqrt((a * a).sum(1)) / (2 * math.pi))
    full = slab64(xyz, q, TILTED, KE, 2.0, 2.0, 0.0, kc, M)
    assert full.s_phi["real"].max() == 0
    assert abs(full.E - e12.E) <= 1e-11 * abs(full.E)
    assert np.abs(full.phi - e12.phi).max() <= 1e-11 * np.abs(full.phi).max()
    assert np.abs(full.ffix - e12.ffix).max() <= 1e-11 * np.abs(full.ffix).max()


def test_the_rule():
    for cell, open_row in ((SHEARED, 2), (TILTED, 0), (np.float32([[6.5, 0, 0], [0, 0, 0], [0, 1, 9]]), 1)):
        p = slab_params64(cell, 0.0, 1e-6)
        _, g, per, o, _, _ = slab_geometry64(cell)
        assert o == open_row and p[3 + o] == 0 and min(p[3 + k] for k in per) >= 1
        assert p[1] == 0.5 * min(1 / np.linalg.norm(g[k]) for k in per) and abs(p[0] * p[1] - math.sqrt(-math.log(1e-6))) < 1e-12
        capped = slab_params64(cell, 0.3, 1e-6)
        assert capped[0] == 0.3 and capped[1] == 0
    # about 131 half-plane vectors in a near-square cell at tol = 1e-6, whatever its size
    for L in (6.5, 14.0, 50.0):
        cell = np.diag(np.float32([L, L, 0]))
        p = slab_params64(cell, 0.0, 1e-6)
        m0, m1 = np.meshgrid(np.arange(-p[3], p[3] + 1), np.arange(0, p[4] + 1), indexing="ij")
        k = 2 * math.pi / L * np.sqrt(m0 ** 2 + m1 ** 2)
        assert 120 <= int(((k <= p[2]) & ((m1 > 0) | (m0 > 0))).sum()) <= 140
