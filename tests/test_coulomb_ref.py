"""The float64 reference of the electrostatics entry (tests/coulomb_ref.py) against itself: the total force against central
differences of E(r), its sum over a molecule, and E = q . phi / 2.  Reference models with random weights, step and tolerance of
test_xyz_grad_ref.py. CPU only."""
import numpy as np
import pytest

import xyz_grad_ref as xr
from conftest import random_weights
from coulomb_ref import coulomb64, coulomb_forces64
from test_gpu_grad_large import _lattice_molecule
from test_xyz_grad_ref import _edges_at

KE = 14.3996454784255
CASES = [(2, 8), (17, 24), (40, 40)]


@pytest.fixture(scope="module")
def weights():
    return random_weights(9, 2, seed=7, scale=0.7)


def _energy_at(r, xyz, x, Q, w, N, alpha):
    """E of the molecule at float64 coordinates r (the helper's forward casts to float32 first: patched as in test_xyz_grad_ref)."""
    orig = xr.edges64
    xr.edges64 = lambda _xyz, num, cutoff=3.0, eta=2.0: _edges_at(r, num, cutoff, eta)
    try:
        q = xr.forward64(xyz, x, Q, w, N=N)[:r.shape[0]]
    finally:
        xr.edges64 = orig
    return coulomb64(r, q, KE, alpha)[1]


def _central(i, c, step, base, xyz, x, Q, w, N, alpha):
    rp, rm = base.copy(), base.copy()
    rp[i, c] += step
    rm[i, c] -= step
    return -(_energy_at(rp, xyz, x, Q, w, N, alpha) - _energy_at(rm, xyz, x, Q, w, N, alpha)) / (2 * step)


@pytest.mark.parametrize("alpha", [0.0, 0.5])
@pytest.mark.parametrize("n,N", CASES)
def test_total_force_equals_central_differences_of_the_energy(weights, n, N, alpha):
    """-dE/dr against central differences of E(r) on float64 coordinates: step 1e-4 A, |f - fd| <= 1e-6 + 1e-5 max |fd|, every
    component.  E(r) is a ReLU network's: where a ReLU changes sign between r - step and r + step the central difference is not
    the derivative on either side (17 atoms, alpha 0: four components off by 3e-4 and 5e-4 of 18 at step 1e-4, all within 1e-8 at
    1e-5, against a median of 2e-8).  The differences themselves show it -- that of half the step disagrees -- so such a component
    is held to the same tolerance at the first halved step whose own half agrees with it; none may need a step below 1e-6."""
    xyz, x, Q = _lattice_molecule(n, 9, seed=n)
    q, phi, E, f, ffix, fq = coulomb_forces64(xyz, x, Q, weights, N, KE, alpha)
    assert np.isfinite(f).all() and np.abs(fq).max() > 1e-6
    base = xyz.astype(np.float64)
    args = (base, xyz, x, Q, weights, N, alpha)
    step = 1e-4
    fd = np.array([[_central(i, c, step, *args) for c in range(3)] for i in range(n)])
    half = np.array([[_central(i, c, step / 2, *args) for c in range(3)] for i in range(n)])
    tol = 1e-6 + 1e-5 * np.abs(fd).max()
    halved = 0
    for i, c in zip(*np.nonzero(np.abs(fd - half) > tol)):
        h, coarse, fine = step / 2, fd[i, c], half[i, c]
        while abs(coarse - fine) > tol:
            h, coarse = h / 2, fine
            assert h >= 1e-6, (i, c, "no step down to 1e-6 at which the central difference settles")
            fine = _central(i, c, h, *args)
        fd[i, c] = coarse
        halved += 1
    err = np.abs(f - fd).max()
    print(f"n = {n}, alpha = {alpha}: |f - fd| {err:.3e} of {np.abs(fd).max():.3e}; |ffix| {np.abs(ffix).max():.3e}, |fq| {np.abs(fq).max():.3e}; "
          f"{halved} of {3 * n} components at a halved step")
    assert halved <= 0.1 * 3 * n + 1
    assert err <= tol, (err, np.abs(fd).max())


@pytest.mark.parametrize("alpha", [0.0, 0.5])
@pytest.mark.parametrize("n,N", CASES)
def test_forces_sum_to_zero_and_energy_is_half_q_phi(weights, n, N, alpha):
    xyz, x, Q = _lattice_molecule(n, 9, seed=n)
    q, phi, E, f, ffix, fq = coulomb_forces64(xyz, x, Q, weights, N, KE, alpha)
    assert np.abs(f.sum(0)).max() <= 1e-10 * np.abs(f).max()
    assert np.abs(ffix.sum(0)).max() <= 1e-10 * np.abs(f).max()
    assert E == 0.5 * float(q @ phi)
    # the pair form of the energy: ke sum_{i<j} q_i q_j kappa(D_ij)
    from coulomb_ref import kappa64
    r = xyz.astype(np.float64)
    iu = np.triu_indices(n, 1)
    D = np.sqrt(((r[iu[0]] - r[iu[1]]) ** 2).sum(-1))
    pair = KE * float((q[iu[0]] * q[iu[1]] * kappa64(D, alpha)[0]).sum())
    assert abs(E - pair) <= 1e-12 * max(abs(pair), np.abs(q[:, None] * q[None, :]).sum() * KE)
