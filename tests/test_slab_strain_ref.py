"""The float64 reference of the slab sum's strain derivative (slab_strain_ref.slab_strain64) checked on the CPU before anything is
compared with it: central differences of the energy on a fixed slot list and fixed pairs, the padded three-dimensional sum plus the
Yeh-Berkowitz term's strain, the single charge in a square cell, symmetry and rotation."""
import math

import numpy as np
import pytest

from ewald_ref import ewald64, ewald_params64
from slab_ref import slab64, slab_geometry64, slab_params64
from slab_strain_ref import slab_energy64, slab_pairs64, slab_slots64, slab_strain64
from test_slab_ref import KE, SHEARED, TILTED, _slab

COMPONENTS = [(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]


def _strained_energy(xyz, q, cell, alpha, p, eps, exclusions=None):
    """The energy at r -> (1 + eps) r, a_k -> (1 + eps) a_k on the unstrained cell's slots, in-range pairs and images."""
    r, a = xyz.astype(np.float64), cell.astype(np.float64)
    slots = slab_slots64(cell, p[2], p[3:])
    mask, shifts = slab_pairs64(xyz, cell, p[1])
    F = np.eye(3) + eps
    return sum(slab_energy64(r @ F.T, q, a @ F.T, KE, alpha, p[0], slots, mask, shifts, exclusions).values())


@pytest.mark.parametrize("alpha", [0.0, 0.5])
@pytest.mark.parametrize("Q", [0.0, 0.7])
@pytest.mark.parametrize("cell", [SHEARED, TILTED], ids=["sheared", "tilted"])
def test_central_differences_of_the_energy_on_fixed_lists(cell, Q, alpha):
    xyz, q = _slab(cell, 9, 5, Q)
    p = slab_params64(cell, alpha, 1e-6)
    assert (p[1] == 0) == (alpha > 0)
    ex = (np.int32([[0, 1], [2, 5], [3, 4]]), np.float32([0.0, 0.5, 0.8333]))
    for exclusions in (None, ex):
        W, s = slab_strain64(xyz, q, cell, KE, alpha, p[0], p[1], p[2], p[3:], exclusions)
        # the unstrained energy on the fixed lists is slab64's, without its self term
        e = slab64(xyz, q, cell, KE, alpha, p[0], p[1], p[2], p[3:])
        if exclusions is None:
            e_self = -0.5 * KE * 2.0 * p[0] / math.sqrt(math.pi) * float(q @ q)
            assert abs(_strained_energy(xyz, q, cell, alpha, p, np.zeros((3, 3))) - (e.E - e_self)) <= 1e-12 * abs(e.E)
        h, worst = 1e-5, 0.0
        for a, b in COMPONENTS:
            eps = np.zeros((3, 3))
            eps[a, b] += 0.5 * h
            eps[b, a] += 0.5 * h
            fd = (_strained_energy(xyz, q, cell, alpha, p, eps, exclusions) - _strained_energy(xyz, q, cell, alpha, p, -eps, exclusions)) / (2 * h)
            # eps_ab = eps_ba = h / 2 for a != b: dE = (W_ab + W_ba) h / 2 = W_ab h
            worst = max(worst, abs(fd - W[a, b]))
        print(f"central differences: {worst:.2e} absolute, {worst / np.abs(W).max():.2e} of max |W|")
        assert worst <= 1e-8 * np.abs(W).max()
        assert all((v >= 0).all() for v in s.values()) and ("excl" in s) == (exclusions is not None)
        assert (np.abs(W) <= sum(s.values()) * (1 + 1e-12)).all()


def test_neutral_slab_equals_the_padded_3d_sum_plus_the_yeh_berkowitz_strain():
    xyz, q = _slab(SHEARED, 12, 3)
    p = slab_params64(SHEARED, 0.0, 1e-12)
    W, _ = slab_strain64(xyz, q, SHEARED, KE, 0.0, p[0], p[1], p[2], p[3:])
    cell3 = SHEARED.astype(np.float64)
    cell3[2] = [0, 0, 80.0]
    p3 = ewald_params64(cell3, 0.0, 1e-12)
    e3 = ewald64(xyz, q, cell3, KE, 0.0, p3[0], p3[1], p3[2], p3[3:])
    Mz = float(q @ xyz[:, 2].astype(np.float64))
    yb = KE * 2.0 * math.pi * Mz * Mz / abs(np.linalg.det(cell3))
    n = np.float64([0, 0, 1])
    want = e3.strain + yb * (2.0 * np.outer(n, n) - np.eye(3))
    err = np.abs(W - want).max()
    print(f"padded 3D sum: {err:.2e} absolute of {np.abs(W).max():.4g}")
    assert abs(Mz) > 0.1 and err <= 1e-9 * np.abs(W).max()


def test_one_charge_in_a_square_cell():
    """E ~ 1 / L and the square's symmetry: W = diag(-E/2, -E/2, 0)."""
    L = 6.5
    cell = np.diag(np.float32([L, L, 0]))
    p = slab_params64(cell, 0.0, 1e-12)
    W, s = slab_strain64(np.zeros((1, 3)), np.ones(1), cell, KE, 0.0, p[0], p[1], p[2], p[3:])
    E = -0.5 * KE * 3.9002649200 / L
    assert abs(W[0, 0] + 0.5 * E) <= 1e-9 * abs(E) and abs(W[1, 1] + 0.5 * E) <= 1e-9 * abs(E)
    off = W.copy()
    off[0, 0] = off[1, 1] = 0.0
    assert np.abs(off).max() <= 1e-12
    assert not s["real"].any() and s["rec"][0, 0] > 0 and s["k0"][0, 0] > 0


@pytest.mark.parametrize("alpha", [0.0, 0.7])
def test_symmetric_and_covariant_under_rotation(alpha):
    xyz, q = _slab(TILTED, 9, 7, 0.7)
    p = slab_params64(TILTED, alpha, 1e-8)
    ex = (np.int32([[0, 1], [2, 5]]), 0.5)
    W, _ = slab_strain64(xyz, q, TILTED, KE, alpha, p[0], p[1], p[2], p[3:], ex)
    assert np.abs(W - W.T).max() <= 1e-12 * np.abs(W).max()
    rng = np.random.default_rng(2)
    R, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    cell_r = TILTED.astype(np.float64) @ R.T
    assert not cell_r[0].any() and len(slab_geometry64(cell_r)[2]) == 2
    Wr, _ = slab_strain64(xyz.astype(np.float64) @ R.T, q, cell_r, KE, alpha, p[0], p[1], p[2], p[3:], ex)
    assert np.abs(Wr - R @ W @ R.T).max() <= 1e-10 * np.abs(W).max()
