"""The float64 Ewald reference (tests/ewald_ref.py) against what is known without it: three lattice constants, independence of the
splitting parameter, forces and strain as central differences of the energy, the library's parameter rule (epnn_ewald_params,
loaded without a GPU) and what its tol means. CPU only."""
import ctypes as C
import math

import numpy as np
import pytest

import cell_ref
from ewald_ref import SLOT_CAP, ewald64, ewald_params64

SHEARED = np.float32([[7, 0, 0], [1.5, 6.5, 0], [-1, 2, 8]])
S_TIGHT = 5.2                    # erfc(5.2) = 2e-13, exp(-5.2^2) = 2e-12: the truncated terms of the "exact" sums below


def _tight(cell, alpha, beta=None):
    """Parameters at which both truncations are below 1e-11 of the leading terms: rc = w_min / 2 and beta = S_TIGHT / rc, or a
    given beta (which must keep min(alpha, beta) rc >= S_TIGHT where there is a real-space part); beta == alpha: rc = 0."""
    a = np.asarray(cell, dtype=np.float64)
    _, g = cell_ref.duals64(a)
    rc = 0.5 * (1.0 / np.sqrt((g * g).sum(1))).min()
    if beta is None:
        beta = S_TIGHT / rc
        if alpha > 0 and alpha <= beta:
            beta = alpha
    if alpha > 0 and beta == alpha:
        rc = 0.0
    else:
        assert (beta if alpha == 0 else min(alpha, beta)) * rc >= S_TIGHT - 1e-9
    kc = 2.0 * beta * S_TIGHT
    M = np.ceil(kc * np.sqrt((a * a).sum(1)) / (2.0 * math.pi))
    return beta, rc, kc, M


def _system(n, cell, seed, Qtot=0.7):
    rng = np.random.default_rng(seed)
    xyz = cell_ref.random_cell(rng, n, np.asarray(cell, dtype=np.float32)).astype(np.float64)
    q = rng.normal(size=n) * 0.4
    return xyz, q + (Qtot - q.sum()) / n


# ---------------------------------------------------------------------------------------------------- lattice constants
def test_nacl_madelung_constant():
    cell = 2.0 * np.eye(3)
    xyz = np.array([(i, j, k) for i in range(2) for j in range(2) for k in range(2)], dtype=np.float64)
    q = (-1.0) ** xyz.sum(1)
    e = ewald64(xyz, q, cell, 1.0, 0.0, *_tight(cell, 0.0))
    assert np.abs(-e.phi * q - 1.7475645946).max() < 1e-10
    assert abs(e.E + 4 * 1.7475645946) < 1e-9 and np.abs(e.ffix).max() < 1e-10


def test_cscl_madelung_constant():
    cell = np.eye(3)
    xyz = np.array([[0, 0, 0], [0.5, 0.5, 0.5]], dtype=np.float64)
    q = np.array([1.0, -1.0])
    e = ewald64(xyz, q, cell, 1.0, 0.0, *_tight(cell, 0.0))
    assert np.abs(-e.phi * q * math.sqrt(3) / 2 - 1.7626747731).max() < 1e-10


def test_wigner_constant_of_one_charge_with_its_background():
    for L in (1.0, 3.5):
        e = ewald64(np.array([[0.3, -0.2, 0.9]]) * L, np.array([1.0]), L * np.eye(3), 1.0, 0.0, *_tight(L * np.eye(3), 0.0))
        assert abs(-e.phi[0] * L - 2.8372974795) < 1e-10 and abs(-2.0 * e.E * L - 2.8372974795) < 1e-10
        assert np.abs(e.ffix).max() < 1e-10


# ---------------------------------------------------------------------------------------------------- the splitting parameter drops out
@pytest.mark.parametrize("alpha", [0.0, 0.8, 0.2])
def test_beta_independence(alpha):
    """E, phi, ffix and the strain at two splitting parameters, Q = 0.7, a sheared cell.  For alpha > 0 the real-space term decays
    with min(alpha, beta), so the cell is scaled until a beta below alpha converges within rc; the other beta is alpha itself
    (no real-space part at all)."""
    if alpha == 0:
        cell = SHEARED.astype(np.float64)
        betas = [_tight(cell, 0.0)[0], 1.2 * _tight(cell, 0.0)[0]]
    else:
        scale = 2.0 * S_TIGHT / (0.75 * alpha) / cell_ref.widths(SHEARED).min()
        cell = SHEARED.astype(np.float64) * scale
        betas = [alpha, 0.75 * alpha * 1.0000001]
    xyz, q = _system(12, SHEARED, 3)
    xyz = xyz * (cell[0, 0] / float(SHEARED[0, 0]))
    one, two = (ewald64(xyz, q, cell, 14.4, alpha, *_tight(cell, alpha, b)) for b in betas)
    for name in ("phi", "E", "ffix", "strain"):
        a, b = np.asarray(getattr(one, name)), np.asarray(getattr(two, name))
        scale = max(np.abs(a).max(), 1e-3 * np.abs(one.phi).max())
        assert np.abs(a - b).max() <= 1e-9 * scale, (name, np.abs(a - b).max(), scale)


# ---------------------------------------------------------------------------------------------------- forces and strain are derivatives of E
@pytest.mark.parametrize("alpha", [0.0, 0.8, 0.2])
def test_forces_and_strain_are_central_differences_of_the_energy(alpha):
    """ffix = -dE/dr and strain = dE/d eps at fixed charges and fixed parameters, all nine components, Q = 0.7.  Steps of 1e-5: the
    difference quotient carries 1e-16 |E| / 1e-5 of rounding and 1e-10 f''' / 6 of truncation, both under 1e-6 of the largest force."""
    cell = SHEARED.astype(np.float64)
    xyz, q = _system(8, SHEARED, 5)
    par = _tight(cell, alpha)
    e = ewald64(xyz, q, cell, 14.4, alpha, *par)
    E = lambda r, c: ewald64(r, q, c, 14.4, alpha, *par).E
    h = 1e-5
    fd = np.zeros_like(xyz)
    for i in range(xyz.shape[0]):
        for c in range(3):
            d = np.zeros_like(xyz)
            d[i, c] = h
            fd[i, c] = -(E(xyz + d, cell) - E(xyz - d, cell)) / (2 * h)
    assert np.abs(fd - e.ffix).max() <= 1e-6 * np.abs(e.ffix).max(), np.abs(fd - e.ffix).max()
    sd = np.zeros((3, 3))
    for a in range(3):
        for b in range(3):
            eps = np.zeros((3, 3))
            eps[a, b] = h
            up, dn = np.eye(3) + eps, np.eye(3) - eps
            sd[a, b] = (E(xyz @ up.T, cell @ up.T) - E(xyz @ dn.T, cell @ dn.T)) / (2 * h)
    assert np.abs(sd - e.strain).max() <= 1e-6 * np.abs(e.strain).max(), np.abs(sd - e.strain).max()
    assert np.abs(e.strain - e.strain.T).max() <= 1e-12 * np.abs(e.strain).max()
    assert np.abs(e.ffix.sum(0)).max() <= 1e-10 * np.abs(e.ffix).max()


# ---------------------------------------------------------------------------------------------------- the library's rule
def _params(cell, alpha, tol):
    from epnn_amd import _lib
    lib = _lib.load()
    cell = np.ascontiguousarray(cell, dtype=np.float32)
    out = np.empty(6, dtype=np.float64)
    _lib.check(lib.epnn_ewald_params(_lib.fptr(cell), float(alpha), float(tol), out.ctypes.data_as(C.POINTER(C.c_double))), lib)
    return out


CELLS = {"cube8": 8 * np.eye(3), "sheared": SHEARED, "6x6x20": np.diag([6.0, 6.0, 20.0]), "cube14": 14 * np.eye(3), "cube100": 100 * np.eye(3)}


@pytest.mark.parametrize("name", sorted(CELLS))
def test_the_librarys_rule(name):
    cell = np.float32(CELLS[name])
    for alpha in (0.0, 0.5, 0.05, 3.0):
        for tol in (1e-4, 1e-6, 1e-8):
            got, want = _params(cell, alpha, tol), ewald_params64(cell, alpha, tol)
            assert np.allclose(got[:3], want[:3], rtol=1e-12, atol=0) and np.array_equal(got[3:], want[3:]), (alpha, tol, got, want)
            beta, rc, kc = got[:3]
            s = math.sqrt(-math.log(tol))
            assert kc == pytest.approx(2 * beta * s, rel=1e-12)
            if rc == 0:
                assert alpha > 0 and beta == alpha
            else:
                assert rc == pytest.approx(0.5 * cell_ref.widths(cell).min(), rel=1e-12) and beta == pytest.approx(s / rc, rel=1e-12)
                assert alpha == 0 or beta <= alpha
    # the number of reciprocal vectors depends on the accuracy and the shape, not on the size: about 1450 in the half space of a cube
    if name.startswith("cube"):
        beta, rc, kc, M0, M1, M2 = _params(cell, 0.0, 1e-6)
        L = float(cell[0, 0])
        m = np.stack(np.meshgrid(*[np.arange(-M0, M0 + 1)] * 3, indexing="ij"), -1).reshape(-1, 3)
        inside = int(((m * m).sum(1) * (2 * math.pi / L) ** 2 <= kc * kc).sum()) - 1
        assert 1300 <= inside // 2 <= 1600, inside


def test_the_rule_refuses_by_name():
    from epnn_amd._lib import EpnnError
    cube = 8 * np.eye(3)
    for cell, match in ((np.diag([8.0, 8.0, 0.0]), "open"), (np.float32([[8, 0, 0], [0, 0, 0], [0, 0, 8]]), "open"),
                        (np.float32([[8, 0, 0], [0, 8, 0], [8, 8, 0]]), "linearly dependent"),
                        (np.float32([[8, 0, 0], [0, np.inf, 0], [0, 0, 8]]), "not finite"),
                        (np.diag([6.0, 6.0, 20000.0]), "cap")):
        with pytest.raises(EpnnError, match=match):
            _params(cell, 0.0, 1e-6)
    for tol in (0.0, 1.0, -1e-6, 2.0, float("nan"), float("inf")):
        with pytest.raises(EpnnError, match=r"tol must be finite and inside \(0, 1\)"):
            _params(cube, 0.0, tol)
    for alpha in (-1.0, float("nan"), float("inf")):
        with pytest.raises(EpnnError, match="alpha must be finite"):
            _params(cube, alpha, 1e-6)
    M = _params(np.diag([6.0, 6.0, 400.0]), 0.0, 1e-6)[3:]
    assert (2 * M[0] + 1) * (2 * M[1] + 1) * (M[2] + 1) <= SLOT_CAP


# ---------------------------------------------------------------------------------------------------- what tol means
@pytest.mark.parametrize("alpha", [0.0, 0.5, 2.5])
@pytest.mark.parametrize("tol", [1e-6, 1e-4])
def test_truncation_at_the_rules_parameters(tol, alpha):
    """The reference at the rule's parameters against itself at tol = 1e-14, a 20-atom sheared cell with Q = 0.7: phi within
    tol ke beta sum |q|, E within tol 1/2 ke beta (sum |q|)^2, ffix within tol ke beta^2 sum |q| max |q| -- the documented meaning of
    tol (include/epnn.h).  Measured at alpha = 0: 0.02 to 0.03 of these scales."""
    ke = 14.3996454784255
    xyz, q = _system(20, SHEARED, 7)
    p, p0 = _params(SHEARED, alpha, tol), _params(SHEARED, alpha, 1e-14)
    e, e0 = (ewald64(xyz, q, SHEARED, ke, alpha, v[0], v[1], v[2], v[3:]) for v in (p, p0))
    beta, Qa = p[0], np.abs(q).sum()
    ephi, eE, eff = np.abs(e.phi - e0.phi).max(), abs(e.E - e0.E), np.abs(e.ffix - e0.ffix).max()
    sphi, sE, sff = tol * ke * beta * Qa, tol * 0.5 * ke * beta * Qa * Qa, tol * ke * beta * beta * Qa * np.abs(q).max()
    print(f"tol {tol}, alpha {alpha}: beta {beta:.4f} rc {p[1]:.3f} kc {p[2]:.3f} M {p[3:]}; phi {ephi:.2e} = {ephi / sphi:.3f}, "
          f"E {eE:.2e} = {eE / sE:.3f}, ffix {eff:.2e} = {eff / sff:.3f} of the scales")
    assert ephi <= sphi and eE <= sE and eff <= sff
