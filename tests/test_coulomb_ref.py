"""The float64 reference of the electrostatics entry (tests/coulomb_ref.py) against itself: the total force against central
differences of E(r), its sum over a molecule, and E = q . phi / 2; g(u) of kappa' from its series against its closed form where
both are good, and against mpmath from 1e-6 to 50; the conditions on the inputs of tests/test_gpu_coulomb_domain.py.  Reference models with random weights, step and tolerance of
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


# ---------------------------------------------------------------------------------------------------- g(u) of kappa'
def test_g_series_and_closed_form_agree_on_the_overlap():
    """Where the series is summed far enough and the closed form has not yet cancelled (0.25 <= u <= 1) the two are within 1e-12
    relative: about 1e-16 / u^2 of cancellation in the closed form, a few ulp of erf, and the series' remainder below 1e-24.  The
    switch of g64 lies inside that interval, and g64 is one or the other on either side of it."""
    import coulomb_ref as cr
    lo, hi = cr.G_OVERLAP
    assert lo < cr.G_U0 < hi
    u = np.concatenate([np.linspace(lo, hi, 3001), [cr.G_U0, np.nextafter(cr.G_U0, 0.0), np.nextafter(cr.G_U0, 1.0)]])
    a, b = cr.g_series64(u), cr.g_closed64(u)
    rel = np.abs(a - b) / b
    print(f"series against closed form on [{lo}, {hi}]: {rel.max():.2e} relative, worst at u = {u[np.argmax(rel)]:.4f}")
    assert (b > 0).all() and rel.max() <= 1e-12
    got = cr.g64(u)
    assert np.array_equal(got[u < cr.G_U0], a[u < cr.G_U0]) and np.array_equal(got[u >= cr.G_U0], b[u >= cr.G_U0])
    # the next term the series leaves out, at the largest u it is used for
    k = cr.G_TERMS + 1
    assert 2 * k / ((2 * k + 1) * float(np.prod(np.arange(1.0, k + 1)))) * hi ** (2 * k) <= 1e-20
    # kappa' is -g / D^2 and kappa erf / D, at both forms and at alpha = 0
    D = np.float64([0.6, 1.7, 80.0])
    for alpha in (1e-3, 0.3, 4.0):
        kap, dkap = cr.kappa64(D, alpha)
        assert np.array_equal(dkap, -cr.g64(alpha * D) / (D * D)) and np.array_equal(kap, cr._erf(alpha * D) / D)
    assert np.array_equal(cr.kappa64(D, 0.0)[1], -1.0 / (D * D))


def test_g_against_mpmath_from_1e_6_to_50():
    """g64 at 200 values of u spaced geometrically over 1e-6 .. 50, and at the switch and the ends of the kernel's own branch, against
    mpmath at 40 digits: within 1e-12 relative.  (The closed form alone is off by 8e-7 at u = 1e-5.)"""
    mp = pytest.importorskip("mpmath")
    import coulomb_ref as cr
    mp.mp.dps = 40
    u = np.concatenate([np.geomspace(1e-6, 50.0, 200), [cr.G_U0, np.nextafter(cr.G_U0, 0.0), 0.9, 1.0, 1.1]])
    want = np.array([float(mp.erf(mp.mpf(float(v))) - 2 / mp.sqrt(mp.pi) * mp.mpf(float(v)) * mp.exp(-mp.mpf(float(v)) ** 2)) for v in u])
    rel = np.abs(cr.g64(u) - want) / want
    closed = np.abs(cr.g_closed64(u) - want) / want
    print(f"g64 against mpmath: {rel.max():.2e} relative, worst at u = {u[np.argmax(rel)]:.3e}; the closed form alone {closed.max():.2e} "
          f"at u = {u[np.argmax(closed)]:.3e}")
    assert (want > 0).all() and rel.max() <= 1e-12
    # and through kappa64: kappa' D^2 = -g
    D = u / 0.3
    assert (np.abs(-cr.kappa64(D, 0.3)[1] * D * D - want) <= 2e-12 * want).all()


# ---------------------------------------------------------------------------------------------------- inputs of test_gpu_coulomb_domain.py
def test_the_two_atom_inputs_are_usable():
    """On the references alone: u = alpha D covers what the GPU test says it covers; forward64 gives every atom of every two-atom
    molecule |q| >= 0.05 with the GPU test's weights (a vanishing charge would empty the per-pair check); a molecule without a listed
    pair has q == Q / 2 and a zero charge gradient, exactly."""
    import test_gpu_coulomb as tc
    import test_gpu_coulomb_domain as td
    td.assert_u_coverage()
    w = tc._weights()
    least, unlisted = np.inf, 0
    for kind in ("geometric", "branch", "both"):
        for xyz, x, Q in td.two_atom_molecules(kind):
            q = xr.forward64(xyz, x, Q, w, N=td.PAIR_N)[:2]
            least = min(least, float(np.abs(q).min()))
            if td.pair_distance((xyz, x, Q)) > td.CUTOFF:
                unlisted += 1
                phi = coulomb64(xyz, q, KE, 0.3)[0]
                assert (q == np.float32(Q) / np.float32(2)).all() and not xr.vjp64(xyz, x, Q, phi, w, N=td.PAIR_N)[1].any()
    print(f"two-atom molecules: least |q| {least:.3f}; {unlisted} without a listed pair")
    assert least >= 0.05 and unlisted >= 16


def test_the_packed_molecules_have_charges():
    """Every molecule of two or more atoms in the packed batches has a reference charge of at least 0.05 somewhere."""
    import test_gpu_coulomb as tc
    import test_gpu_coulomb_domain as td
    w = tc._weights()
    least = min(float(np.abs(xr.forward64(*m, w, N=N)[:len(m[0])]).max()) for ns, N, _ in td.PACKED for m in td.packed_molecules(ns) if len(m[0]) > 1)
    print(f"packed batches: the smallest of the molecules' largest |q| is {least:.3f}")
    assert least >= 0.05


def test_the_blocked_rows_are_the_dense_ones():
    """coulomb64_rows and coulomb_energy64 (the large clusters of test_gpu_coulomb_domain.py) against coulomb64."""
    from coulomb_ref import coulomb64_rows, coulomb_energy64
    xyz = _lattice_molecule(150, 9, seed=150)[0]
    q = np.random.default_rng(1).normal(scale=0.3, size=150)
    rows = np.concatenate([np.arange(5), np.arange(7, 150, 8)])
    for alpha in (0.0, 0.3):
        phi, E, ffix, sphi, sff = coulomb64(xyz, q, KE, alpha)
        for sel, got in ((np.arange(150), coulomb64_rows(xyz, q, KE, alpha, block=64)), (rows, coulomb64_rows(xyz, q, KE, alpha, rows, block=16))):
            for a, b in zip(got, (phi, ffix, sphi, sff)):
                assert np.abs(a - b[sel]).max() <= 1e-13 * np.abs(b).max()
        Eb, sE = coulomb_energy64(xyz, q, KE, alpha, block=64)
        assert abs(Eb - E) <= 1e-13 * sE and abs(sE - 0.5 * np.abs(q) @ sphi) <= 1e-13 * sE
