"""The float64 references of the site entries (tests/site_ref.py) against what is known without them: (a) equal widths are the existing
references at alpha = 1 / (2 sigma); (b) a cell's energy from the reciprocal sum of the Gaussians alone, which has no beta and no
real-space part, neutral and charged; (c) the splitting parameter drops out; (d) forces, mu and all nine strain components as central
differences of the energy.  Every threshold of (b)-(d) is made in the test from the references' own convergence: the change under
tighter sums, and for the difference quotients the change between steps h and 2 h (their truncation, ~h^2) plus the rounding of E
over h.  CPU only."""
import math

import numpy as np
import pytest

import cell_ref
from coulomb_excl_ref import add_correction, coulomb64_w, excl_correction64, exclusion_cases
from coulomb_ref import coulomb64
from ewald_ref import ewald64
from site_ref import coulomb_site64, ewald_gauss_recip64, ewald_site64

KE = 14.3996454784255
SHEARED = np.float32([[7, 0, 0], [1.5, 6.5, 0], [-1, 2, 8]])
EPS = 2.0 ** -52


def _tight(cell, s):
    """Parameters at which both truncations are erfc(s) and exp(-s^2) of the leading terms: rc = w_min / 2, beta = s / rc, kc = 2 beta s"""
    a = np.asarray(cell, dtype=np.float64)
    rc = 0.5 * cell_ref.widths(a).min()
    beta = s / rc
    kc = 2.0 * beta * s
    return beta, rc, kc, np.ceil(kc * np.sqrt((a * a).sum(1)) / (2.0 * math.pi))


def _system(n, cell, seed, Qtot, s_max=6.2):
    """Positions, charges summing to Qtot, and widths in [0.4, 1] of the largest width 1 / (2 beta) the tightest split (s_max) allows"""
    rng = np.random.default_rng(seed)
    xyz = cell_ref.random_cell(rng, n, np.asarray(cell, dtype=np.float32)).astype(np.float64)
    q = rng.normal(size=n) * 0.4
    sigma = rng.uniform(0.4, 1.0, size=n) * 0.5 / _tight(cell, s_max)[0]
    return xyz, q + (Qtot - q.sum()) / n, sigma, rng.normal(size=n), np.abs(rng.normal(size=n)) * 5.0


# ---------------------------------------------------------------------------------------------------- (a) equal widths
@pytest.mark.parametrize("sigma", [0.3, 1.1])
def test_equal_widths_are_the_existing_references(sigma):
    """sigma_i = sigma, chi = J = 0, no self term: coulomb64 / ewald64 at alpha = 1 / (2 sigma), to 1e-12 relative, with and without a
    list; and the absolute sums agree.  Charged cell (Q = 0.7): the per-pair background reduces to the existing one."""
    alpha = 0.5 / sigma
    xyz, q, _, _, _ = _system(14, SHEARED, 2, 0.7)
    sg = np.full(14, sigma)
    pairs, scale = exclusion_cases(xyz)
    assert len(pairs) >= 3
    for pl, sc in ((None, None), (pairs, scale)):
        s = coulomb_site64(xyz, q, KE, sigma=sg, pairs=pl, scale=sc)
        phi, E, ffix, sp, sf = coulomb64_w(xyz, q, KE, alpha, pairs, scale) if pl is not None else coulomb64(xyz, q, KE, alpha)
        for got, want in ((s.phi, phi), (s.mu, phi), (s.E, E), (s.ffix, ffix), (s.s_phi["real"], sp), (s.s_ffix["real"], sf)):
            assert np.abs(np.asarray(got) - want).max() <= 1e-12 * np.abs(want).max()
    grow = max(1.0, _tight(SHEARED, 5.2)[0] / (0.9 * alpha))     # (the cell scaled until beta <= 0.9 alpha: the erf(alpha D) tail converges in rc)
    cell = SHEARED.astype(np.float64) * grow
    xyz = xyz * grow
    par = _tight(cell, 5.2)
    assert par[0] <= 0.91 * alpha
    pairs, scale = exclusion_cases(xyz, cell, near=3.0)
    for pl in (None, pairs):
        s = ewald_site64(xyz, q, cell, KE, 0.0, sg, None, None, 0, *par, pairs=pl, scale=scale)
        e = ewald64(xyz, q, cell, KE, alpha, *par)
        if pl is not None:
            e = add_correction(e, excl_correction64(xyz, q, cell, KE, alpha, pairs, scale), q)
        for name in ("phi", "E", "ffix", "strain"):
            got, want = np.asarray(getattr(s, name)), np.asarray(getattr(e, name))
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), name
        for name in ("s_phi", "s_ffix", "s_strain", "s_E"):
            for part in ("real", "rec", "rest"):
                got, want = np.asarray(getattr(s, name)[part]), np.asarray(getattr(e, name)[part])
                assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300), (name, part)
    # the same through alpha instead of sigma, with the self term: E differs from the plain sum by ke alpha / sqrt(pi) sum q^2
    s = coulomb_site64(xyz, q, KE, alpha=alpha, self_term=1)
    assert abs(s.E - coulomb64(xyz, q, KE, alpha)[1] - KE * alpha / math.sqrt(math.pi) * (q * q).sum()) <= 1e-12 * abs(s.E)


# ---------------------------------------------------------------------------------------------------- (b) the pure reciprocal sum
@pytest.mark.parametrize("Qtot", [0.0, 0.7])
def test_energy_is_the_reciprocal_sum_of_the_gaussians(Qtot):
    """Mixed widths, self term on, chi = J = 0: E of ewald_site64 equals 1/2 sum_{k != 0} (4 pi ke / V k^2) |sum_j q_j exp(-k^2 sigma_j^2 / 2)
    exp(i k r_j)|^2, a formula with no beta and no real-space part.  Leaving k = 0 out is the convention in which every pair potential
    averages to zero over the cell, the one the stated background puts ewald_site64 in, so for Q = 0.7 the two agree with E_bg inside
    E and nothing added; that pins E_bg (-7.4e-3 here, of which the widths' part is about 2e-3: either is 1e8 thresholds).  Threshold: twice the change of
    E between the splits s = 5.2 and s = 6.2 (the truncated terms fall from 2e-13 to 2e-18 of the leading ones) plus 64 * 2^-52 of
    the sum of absolute terms (the roundings of sums of ~10^4 terms).
    Achieved: Q = 0: |dE| 3.9e-12 of a threshold 9.6e-12 (E = 31.6); Q = 0.7: 4.1e-12 of 9.7e-12 (E = 32.8, E_bg = -0.0074)."""
    xyz, q, sigma, _, _ = _system(12, SHEARED, 3, Qtot)
    cell = SHEARED.astype(np.float64)
    one = ewald_site64(xyz, q, cell, KE, 0.0, sigma, None, None, 1, *_tight(cell, 5.2))
    two = ewald_site64(xyz, q, cell, KE, 0.0, sigma, None, None, 1, *_tight(cell, 6.2))
    want = ewald_gauss_recip64(xyz, q, cell, KE, sigma)
    bound = 2.0 * abs(one.E - two.E) + 64 * EPS * sum(one.s_E.values())
    print(f"Q {Qtot}: E {one.E:.6f} recip {want:.6f} |dE| {abs(one.E - want):.2e} bound {bound:.2e} E_bg {one.E_bg:.4f}")
    assert abs(one.E - want) <= bound
    assert Qtot == 0.0 or abs(one.E_bg) > 1e6 * bound
    assert Qtot != 0.0 or abs(one.E_bg) <= 1e-15                 # (Q is zero to rounding)


# ---------------------------------------------------------------------------------------------------- (c) the splitting parameter drops out
@pytest.mark.parametrize("with_list", [False, True])
def test_beta_independence(with_list):
    """phi, mu, E, ffix and the strain at the splits s = 5.2 and s = 6.2 (beta differs by 19 %), mixed widths, Q = 0.7, chi, J and the
    self term on, with and without a list.  What tol means at these parameters: the truncated terms are erfc(s) and exp(-s^2) of the
    leading ones, 2e-13 and 2e-12 at s = 5.2, so each result agrees within 4e-12 (their sum, doubled) of its sum of absolute terms,
    plus 64 * 2^-52 of them for the roundings.  Achieved: at most 0.074 of that bound (the strain; phi, mu, E and ffix 0.003 to 0.006), the same with a list."""
    xyz, q, sigma, chi, J = _system(12, SHEARED, 4, 0.7)
    cell = SHEARED.astype(np.float64)
    pairs, scale = exclusion_cases(xyz, cell) if with_list else (None, None)
    one, two = (ewald_site64(xyz, q, cell, KE, 0.0, sigma, chi, J, 1, *_tight(cell, s), pairs=pairs, scale=scale) for s in (5.2, 6.2))
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


# ---------------------------------------------------------------------------------------------------- (d) derivatives of the energy
def _quotients(E, x0, h):
    out = np.zeros(x0.size)
    for k in range(x0.size):
        d = np.zeros(x0.size)
        d[k] = h
        out[k] = (E((x0.reshape(-1) + d).reshape(x0.shape)) - E((x0.reshape(-1) - d).reshape(x0.shape))) / (2 * h)
    return out.reshape(x0.shape)


def _fd_check(what, E, x0, want, s_E, h):
    """Central differences at h against `want`.  Threshold, from the quotient's own convergence: its truncation is c h^2, so
    |q(2 h) - q(h)| = 3 c h^2 bounds it with room (taken whole, not a third); its rounding is that of E, 16 * 2^-52 of E's absolute
    terms, over h."""
    q1, q2 = _quotients(E, x0, h), _quotients(E, x0, 2 * h)
    bound = np.abs(q2 - q1).max() + 16 * EPS * s_E / h
    err = np.abs(q1 - want).max()
    print(f"{what}: h {h:g} err {err:.2e} bound {bound:.2e} ({err / bound:.2f}) scale {np.abs(want).max():.2e}")
    assert err <= bound, what
    assert bound <= 1e-5 * np.abs(want).max(), what + ": the step resolves nothing"
    return err / bound


@pytest.mark.parametrize("geometry", ["open", "cell"])
@pytest.mark.parametrize("with_list", [False, True])
def test_forces_mu_and_strain_are_central_differences_of_the_energy(geometry, with_list):
    """ffix = -dE/dr and mu = dE/dq, and in cells strain = dE/d eps (all nine components; open molecules: the virial under r -> (1 +
    eps) r), at fixed parameters: mixed widths, chi, J and the self term on, Q = 0.7.  Steps: h = 1e-4 in r and eps, 1e-3 in q (E is
    quadratic in q: no truncation).  Thresholds: _fd_check's, from the quotients at h and 2 h and the rounding of E.
    Achieved (err / bound, over the four cases): r 0.09 to 0.17, q 0.02 to 0.06, eps 0.29 to 0.31; every bound is under 3e-8 of the largest component (asserted under 1e-5: the step resolves the derivative)."""
    cell = SHEARED.astype(np.float64)
    xyz, q, sigma, chi, J = _system(8, SHEARED, 5, 0.7)
    pairs, scale = (exclusion_cases(xyz, cell if geometry == "cell" else None, near=3.0) if with_list else (None, None))
    assert not with_list or len(pairs) >= 3
    par = _tight(cell, 5.2)
    if geometry == "cell":
        f = lambda r, qq, c: ewald_site64(r, qq, c, KE, 0.0, sigma, chi, J, 1, *par, pairs=pairs, scale=scale)
    else:
        f = lambda r, qq, c: coulomb_site64(r, qq, KE, sigma=sigma, chi=chi, hard=J, self_term=1, pairs=pairs, scale=scale)
    e = f(xyz, q, cell)
    s_E = sum(e.s_E.values())
    _fd_check("r", lambda r: f(r, q, cell).E, xyz, -e.ffix, s_E, 1e-4)
    _fd_check("q", lambda qq: f(xyz, qq, cell).E, q, e.mu, s_E, 1e-3)

    def strained(eps):
        up = np.eye(3) + eps
        return f(xyz @ up.T, q, cell @ up.T).E
    _fd_check("eps", strained, np.zeros((3, 3)), e.strain, s_E, 1e-4)
    assert np.abs(e.strain - e.strain.T).max() <= 1e-12 * np.abs(e.strain).max()
    assert np.abs(e.ffix.sum(0)).max() <= 1e-10 * np.abs(e.ffix).max()
