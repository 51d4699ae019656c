"""The float64 reference of the slab site entries (tests/slab_site_ref.py) against what is known without it: (a) equal widths are
slab64 / slab_strain64 at alpha = 1 / (2 sigma); (b) the energy equals the Gaussians' own two-dimensional sum, which has no beta, no
real-space part and no self term, neutral and charged: this pins that the slab takes no background term and no per-pair k = 0
correction; (c) a neutral slab equals ewald_site64 in a cell padded with vacuum plus the Yeh-Berkowitz term; (d) the splitting
parameter drops out; (e) forces, mu and all nine strain components are central differences of the energy, with a list.  Thresholds of
(b), (d), (e) are made as in test_site_ref.py, from the references' own convergence.  CPU only."""
import math

import numpy as np
import pytest

from coulomb_excl_ref import excl_correction64, exclusion_cases
from ewald_ref import ewald_params64
from site_ref import ewald_site64
from slab_ref import slab64, slab_geometry64, slab_params64
from slab_site_ref import PARTS, slab_gauss64, slab_site64
from slab_strain_ref import slab_strain64
from test_site_ref import EPS, _fd_check
from test_slab_ref import KE, SHEARED, TILTED, _slab


def _tight(cell, s):
    """Parameters at which both truncations are erfc(s) and exp(-s^2) of the leading terms: rc = w_min / 2 over the two periodic
    rows, beta = s / rc, kc = 2 beta s, M of the open row 0"""
    a, g, per, _, _, _ = slab_geometry64(cell)
    rc = 0.5 * min(1.0 / math.sqrt(float(g[k] @ g[k])) for k in per)
    beta = s / rc
    kc = 2.0 * beta * s
    M = np.zeros(3)
    for k in per:
        M[k] = math.ceil(kc * math.sqrt(float(a[k] @ a[k])) / (2.0 * math.pi))
    return beta, rc, kc, M


def _system(n, cell, seed, Qtot, s_max=6.2, thick=5.0):
    """Positions, charges summing to Qtot, widths in [0.4, 1] of the largest width 1 / (2 beta) the tightest split (s_max) allows, chi, J"""
    xyz, q = _slab(cell, n, seed, Qtot, thick)
    rng = np.random.default_rng(seed + 100)
    sigma = rng.uniform(0.4, 1.0, size=n) * 0.5 / _tight(cell, s_max)[0]
    return xyz.astype(np.float64), 0.4 * q + 0.6 * Qtot / n, sigma, rng.normal(size=n), np.abs(rng.normal(size=n)) * 5.0


# ---------------------------------------------------------------------------------------------------- (a) equal widths
@pytest.mark.parametrize("sigma", [0.3, 0.45])
@pytest.mark.parametrize("cell", [SHEARED, TILTED], ids=["sheared", "tilted"])
def test_equal_widths_are_the_existing_slab_references(cell, sigma):
    """sigma_i = sigma, chi = J = 0, no self term: slab64 / slab_strain64 at alpha = 1 / (2 sigma) on the same parameters, to 1e-12
    relative, with and without a list, absolute sums included (the listed pairs' sums go to "real", as site_ref counts them)."""
    alpha = 0.5 / sigma
    xyz, q, _, _, _ = _system(12, cell, 2, 0.7)
    p = slab_params64(cell, 0.0, 1e-6)
    assert p[1] > 0 and alpha >= p[0]
    sg = np.full(12, sigma)
    pairs, scale = exclusion_cases(xyz, cell)
    assert len(pairs) >= 3
    for pl in (None, pairs):
        s = slab_site64(xyz, q, cell, KE, 0.0, sg, None, None, 0, p[0], p[1], p[2], p[3:], pairs=pl, scale=scale)
        e = slab64(xyz, q, cell, KE, alpha, p[0], p[1], p[2], p[3:])
        W, sW = slab_strain64(xyz, q, cell, KE, alpha, p[0], p[1], p[2], p[3:], None if pl is None else (pairs, scale))
        want = {"phi": e.phi, "mu": e.phi, "E": e.E, "ffix": e.ffix, "strain": W}
        sums = {"s_phi": dict(e.s_phi), "s_ffix": dict(e.s_ffix), "s_E": dict(e.s_E), "s_strain": dict(sW)}
        sums["s_strain"]["rest"] = np.zeros((3, 3))
        if pl is not None:
            c = excl_correction64(xyz, q, cell, KE, alpha, pairs, scale)
            want["phi"] = want["mu"] = e.phi + c.dphi
            want["E"] = 0.5 * float(q @ want["phi"])
            want["ffix"] = e.ffix + c.dffix
            sums["s_phi"]["real"] = e.s_phi["real"] + c.s_phi
            sums["s_ffix"]["real"] = e.s_ffix["real"] + c.s_ffix
            sums["s_E"]["real"] = e.s_E["real"] + c.s_E
            sums["s_strain"]["real"] = sW["real"] + sums["s_strain"].pop("excl")
        for name, w in want.items():
            assert np.abs(np.asarray(getattr(s, name)) - w).max() <= 1e-12 * np.abs(w).max(), name
        for name, parts in sums.items():
            assert set(getattr(s, name)) == set(PARTS) == set(parts), name
            for part in PARTS:
                got, w = np.asarray(getattr(s, name)[part]), np.asarray(parts[part])
                assert np.abs(got - w).max() <= 1e-12 * max(np.abs(w).max(), 1e-300), (name, part)
    # through alpha instead of sigma, with the self term: E grows by ke alpha / sqrt(pi) sum q^2
    s = slab_site64(xyz, q, cell, KE, alpha, None, None, None, 1, p[0], p[1], p[2], p[3:])
    e = slab64(xyz, q, cell, KE, alpha, p[0], p[1], p[2], p[3:])
    assert abs(s.E - e.E - KE * alpha / math.sqrt(math.pi) * (q * q).sum()) <= 1e-12 * abs(s.E)


# ---------------------------------------------------------------------------------------------------- (b) the Gaussians' own sum
@pytest.mark.parametrize("Qtot", [0.0, 0.7])
def test_energy_is_the_two_dimensional_sum_of_the_gaussians(Qtot):
    """Mixed widths, self term on, chi = J = 0, 8 atoms in the sheared 7 / 6.9 A cell: E of slab_site64 (the point charges' slab sum
    minus the real-space erfc(gamma_ij D) / D plus the Gaussians' self-energy) equals slab_gauss64, the reciprocal and k = 0 formulas
    with beta = gamma_ij per pair, j == i included, with no real-space part and no self term.  Nothing is added for a background or
    for k = 0 per pair, for Q = 0.7 either: the constant dropped for a charged sheet depends on neither beta nor gamma.  Threshold as
    in test_site_ref.py: twice the change of E between the splits s = 5.2 and s = 6.2 plus 64 * 2^-52 of the absolute terms.
    The slab is 1 A thick, so that neighbours overlap and the Gaussians' pair part of E is large (0.31 and 0.22 here, asserted above
    a thousand thresholds).
    Achieved: Q = 0: |dE| 4.0e-13 of a threshold 2.3e-12 (E = 21.37); Q = 0.7: 4.4e-13 of 2.3e-12 (E = 24.99)."""
    xyz, q, sigma, _, _ = _system(8, SHEARED, 3, Qtot, thick=1.0)
    assert abs(q.sum() - Qtot) <= 1e-12 and sigma.max() > 1.5 * sigma.min()
    one = slab_site64(xyz, q, SHEARED, KE, 0.0, sigma, None, None, 1, *_tight(SHEARED, 5.2))
    two = slab_site64(xyz, q, SHEARED, KE, 0.0, sigma, None, None, 1, *_tight(SHEARED, 6.2))
    want = slab_gauss64(xyz, q, SHEARED, KE, sigma)
    bound = 2.0 * abs(one.E - two.E) + 64 * EPS * sum(one.s_E.values())
    print(f"Q {Qtot}: E {one.E:.6f} gauss {want:.6f} |dE| {abs(one.E - want):.2e} bound {bound:.2e} split change {abs(one.E - two.E):.2e}")
    assert abs(one.E - want) <= bound
    # what the pin is about: the real-space erfc(gamma_ij D) / D sum that stands for every difference to the point charges' slab sum
    par = _tight(SHEARED, 5.2)
    gauss_part = one.E - slab64(xyz, q, SHEARED, KE, 0.0, *par).E - KE * float((q * q / (2.0 * math.sqrt(math.pi) * sigma)).sum())
    print(f"the Gaussians' real-space part of E: {gauss_part:.4f}")
    assert abs(gauss_part) > 1e3 * bound                        # (the pin resolves it to a thousandth)


# ---------------------------------------------------------------------------------------------------- (c) the padded 3D sum
def test_neutral_slab_equals_the_padded_3d_site_sum_plus_yeh_berkowitz():
    """A neutral slab with mixed widths, chi, J and the self term against ewald_site64 in the cell padded with 80 A of vacuum plus the
    Yeh-Berkowitz term 2 pi ke Mz^2 / V (for Q = 0 the per-pair background of the periodic entry adds a constant to phi and nothing
    to E).  The threshold of the existing slab tests of that name: 1e-9 of |E|, and of max |W| for the strain."""
    xyz, q, _, chi, J = _system(12, SHEARED, 3, 0.0)
    p = slab_params64(SHEARED, 0.0, 1e-12)
    cell3 = SHEARED.astype(np.float64)
    cell3[2] = [0, 0, 80.0]
    p3 = ewald_params64(cell3, 0.0, 1e-12)
    sigma = np.random.default_rng(9).uniform(0.4, 1.0, size=12) * 0.5 / max(p[0], p3[0])
    s = slab_site64(xyz, q, SHEARED, KE, 0.0, sigma, chi, J, 1, p[0], p[1], p[2], p[3:])
    e3 = ewald_site64(xyz, q, cell3, KE, 0.0, sigma, chi, J, 1, p3[0], p3[1], p3[2], p3[3:])
    Mz = float(q @ xyz[:, 2])
    yb = KE * 2.0 * math.pi * Mz * Mz / abs(np.linalg.det(cell3))
    n = np.float64([0, 0, 1])
    assert abs(Mz) > 0.1 and abs(e3.E_bg) <= 1e-12
    assert abs(s.E - (e3.E + yb)) <= 1e-9 * abs(s.E)
    assert np.abs(s.strain - (e3.strain + yb * (2.0 * np.outer(n, n) - np.eye(3)))).max() <= 1e-9 * np.abs(s.strain).max()


# ---------------------------------------------------------------------------------------------------- (d) the splitting parameter drops out
@pytest.mark.parametrize("with_list", [False, True])
@pytest.mark.parametrize("cell", [SHEARED, TILTED], ids=["sheared", "tilted"])
def test_beta_independence(cell, with_list):
    """phi, mu, E, ffix and the strain at the splits s = 5.2 and s = 6.2, mixed widths, Q = 0.7, chi, J and the self term on.  The
    bound of test_site_ref.py: the truncated terms are erfc(s) and exp(-s^2) of the leading ones at s = 5.2, so each result agrees
    within twice their sum, plus 64 * 2^-52, of its sum of absolute terms.  Achieved: at most 0.033 of that bound (the strain; phi, mu and E 0.001 to 0.002, ffix 0.017)."""
    xyz, q, sigma, chi, J = _system(12, cell, 4, 0.7)
    pairs, scale = exclusion_cases(xyz, cell) if with_list else (None, None)
    one, two = (slab_site64(xyz, q, cell, KE, 0.0, sigma, chi, J, 1, *_tight(cell, s), pairs=pairs, scale=scale) for s in (5.2, 6.2))
    rel = 2.0 * (math.erfc(5.2) + math.exp(-5.2 ** 2)) + 64 * EPS
    worst = 0.0
    for name, sums in (("phi", "s_phi"), ("mu", "s_mu"), ("E", "s_E"), ("ffix", "s_ffix"), ("strain", "s_strain")):
        a, b = np.asarray(getattr(one, name)), np.asarray(getattr(two, name))
        tot = sum(np.asarray(v) for v in getattr(one, sums).values())
        tot = tot[:, None] if name == "ffix" else tot
        share = float((np.abs(a - b) / (rel * tot)).max())
        worst = max(worst, share)
        print(f"list {with_list} {name}: {share:.3f} of the bound")
        assert share <= 1.0, name
    assert worst > 0.0


# ---------------------------------------------------------------------------------------------------- (e) derivatives of the energy
@pytest.mark.parametrize("cell", [SHEARED, TILTED], ids=["sheared", "tilted"])
def test_forces_mu_and_strain_are_central_differences_of_the_energy(cell):
    """ffix = -dE/dr, mu = dE/dq and strain = dE/d eps, all nine components under r -> (1 + eps) r, a_k -> (1 + eps) a_k, at fixed
    parameters with a list: mixed widths, chi, J and the self term on, Q = 0.7.  Steps and thresholds: test_site_ref._fd_check's
    (h = 1e-4 in r and eps, 1e-3 in q; the quotients at h and 2 h and the rounding of E).
    Achieved (err / bound): r 0.12 and 0.23, q 0.01, eps 0.23 and 0.30."""
    xyz, q, sigma, chi, J = _system(8, cell, 5, 0.7)
    cell = cell.astype(np.float64)
    pairs, scale = exclusion_cases(xyz, cell, near=3.0)
    assert len(pairs) >= 3
    par = _tight(cell, 5.2)
    f = lambda r, qq, c: slab_site64(r, qq, c, KE, 0.0, sigma, chi, J, 1, *par, pairs=pairs, scale=scale)
    e = f(xyz, q, cell)
    s_E = sum(e.s_E.values())
    _fd_check("r", lambda r: f(r, q, cell).E, xyz, -e.ffix, s_E, 1e-4)
    _fd_check("q", lambda qq: f(xyz, qq, cell).E, q, e.mu, s_E, 1e-3)

    def strained(eps):
        up = np.eye(3) + eps
        return f(xyz @ up.T, q, cell @ up.T).E
    _fd_check("eps", strained, np.zeros((3, 3)), e.strain, s_E, 1e-4)
    assert np.abs(e.strain - e.strain.T).max() <= 1e-12 * np.abs(e.strain).max()
    nhat = slab_geometry64(cell)[5]
    inplane = e.ffix.sum(0) - (e.ffix.sum(0) @ nhat) * nhat
    assert np.abs(inplane).max() <= 1e-10 * np.abs(e.ffix).max()
