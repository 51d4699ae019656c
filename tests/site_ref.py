"""Float64 references for per-atom Gaussian widths, self-energy and on-site terms in the Coulomb calls (epnn_coulomb_xyz_site,
epnn_coulomb_xyz_cell_site). Test helper.

One molecule or cell, its real atoms only.  With gamma_ij = 1 / sqrt(2 (sigma_i^2 + sigma_j^2)), or the call's alpha where sigma is
None (alpha == 0: bare 1 / D), gamma_ii = 1 / (2 sigma_i) or alpha, w_ij = s for a listed pair and 1 otherwise:
    open    phi_i = ke [sum_{j != i} w_ij q_j erf(gamma_ij D_ij) / D_ij + [self] 2 gamma_ii q_i / sqrt(pi)]
            mu_i  = chi_i + J_i q_i + phi_i;     E = sum_i [chi_i q_i + 1/2 J_i q_i^2 + 1/2 q_i phi_i]
            ffix_i = -ke q_i sum_{j != i} w_ij q_j kappa_ij'(D_ij) (r_i - r_j) / D_ij,    kappa_ij' = -g(gamma_ij D) / D^2
    cells   ewald_ref.ewald64's sum with gamma_ij in its real-space term [erf(gamma_ij D) - erf(beta D)] / D, D <= rc, the listed pairs'
            correction (s - 1) erf(gamma_ij D) / D on the minimum image, and the background per pair,
            phi_bg_i = -ke (pi / V) [Q / beta^2 - w_i Q - sum_j q_j w_j],   w = 2 sigma^2 (sigma None: 1 / (2 alpha^2), or 0);
            E_bg = 1/2 sum_i q_i phi_bg_i with strain -E_bg delta_ab; self and on-site terms have no strain.
Beside every result the sums of its absolute terms by part, counted as ewald_ref.ewald64 counts them: "real" (erf_gamma + erf_beta) / D
per pair (open: erf_gamma / D) plus the listed pairs' |(s - 1) term|, "rec" c(k) sum |q_j|, "rest" everything else as it is (the
self terms, the background, and for mu and E the on-site terms).
ewald_gauss_recip64 is the same energy of a cell from a formula that has no beta and no real-space part.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np

import cell_ref
from coulomb_ref import g64

try:
    from scipy.special import erf as _erf, erfc as _erfc
except ImportError:
    _erf = np.vectorize(math.erf, otypes=[np.float64])
    _erfc = np.vectorize(math.erfc, otypes=[np.float64])

TWO_RPI = 2.0 / math.sqrt(math.pi)


def _site(n, alpha, sigma, chi, hard, self_term):
    """(gamma (n, n) with gamma_ii on the diagonal, w (n,), chi (n,), J (n,), whether the pair terms are bare)"""
    if sigma is not None:
        assert alpha == 0
        s = np.asarray(sigma, dtype=np.float64)
        assert s.shape == (n,) and (s > 0).all()
        s2 = s * s
        gam = 1.0 / np.sqrt(2.0 * (s2[:, None] + s2[None, :]))
        w = 2.0 * s2
    else:
        gam = np.full((n, n), float(alpha))
        w = np.full(n, 0.5 / (alpha * alpha) if alpha > 0 else 0.0)
    bare = sigma is None and alpha == 0
    assert not (self_term and bare), "a point charge has no finite self-energy"
    z = np.zeros(n)
    return gam, w, (z if chi is None else np.asarray(chi, dtype=np.float64)), (z if hard is None else np.asarray(hard, dtype=np.float64)), bare


def _erf_terms(D, gam, bare):
    """(erf(gamma D), erfc(gamma D), g(gamma D)) at the distances D; bare: (1, 0, 1)"""
    if bare:
        return np.ones_like(D), np.zeros_like(D), np.ones_like(D)
    u = gam * D
    return _erf(u), _erfc(u), g64(u)


def _listed(r, q, ke, gam, bare, cell, pairs, scale):
    """The listed pairs' correction on the one minimum image (cell None: the plain displacement): dphi, dffix, dstrain and their
    absolute sums s_phi, s_ffix (n,), s_strain, and per pair the energy terms t_E; factors s - 1 in float32, as the library takes them."""
    n = r.shape[0]
    out = SimpleNamespace(dphi=np.zeros(n), dffix=np.zeros((n, 3)), dstrain=np.zeros((3, 3)), s_phi=np.zeros(n), s_ffix=np.zeros(n),
                          s_strain=np.zeros((3, 3)), s_E=0.0)
    if pairs is None or not len(pairs):
        return out
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    scale = np.asarray(scale, dtype=np.float32)
    scale = np.full(len(pairs), scale, dtype=np.float32) if scale.ndim == 0 else scale
    f = (scale - np.float32(1)).astype(np.float64)
    i, j = pairs[:, 0], pairs[:, 1]
    d = r[i] - r[j]
    if cell is not None:
        d = cell_ref.mic64(d, *cell_ref.duals64(np.asarray(cell, dtype=np.float64)))
    D = np.sqrt((d * d).sum(-1))
    e, _, g = _erf_terms(D, gam[i, j], bare)
    kap, dkap = e / D, -g / (D * D)
    np.add.at(out.dphi, i, ke * f * q[j] * kap)
    np.add.at(out.dphi, j, ke * f * q[i] * kap)
    np.add.at(out.s_phi, i, np.abs(ke * f * q[j] * kap))
    np.add.at(out.s_phi, j, np.abs(ke * f * q[i] * kap))
    t = ke * f * q[i] * q[j] * dkap
    np.add.at(out.dffix, i, -(t / D)[:, None] * d)
    np.add.at(out.dffix, j, (t / D)[:, None] * d)
    np.add.at(out.s_ffix, i, np.abs(t))
    np.add.at(out.s_ffix, j, np.abs(t))
    dd = d[:, :, None] * d[:, None, :]
    out.dstrain = ((t / D)[:, None, None] * dd).sum(0)
    out.s_strain = (np.abs(t / D)[:, None, None] * np.abs(dd)).sum(0)
    out.s_E = float(np.abs(ke * f * q[i] * q[j] * kap).sum())
    return out


def _finish(q, ke, phi, ffix, strain, s_phi, s_ffix, s_strain, gam, chi, J, self_term):
    """The self and on-site terms on top of the pair sums, and the namespace"""
    n = q.shape[0]
    aq = np.abs(q)
    if self_term:
        st = ke * TWO_RPI * np.diag(gam) * q
        phi = phi + st
        s_phi["rest"] = s_phi["rest"] + np.abs(st)
    mu = chi + J * q + phi
    E = float((q * (chi + 0.5 * J * q)).sum() + 0.5 * (q @ phi))
    s_mu = dict(s_phi)
    s_mu["rest"] = s_phi["rest"] + np.abs(chi) + np.abs(J * q)
    s_E = {p: 0.5 * float(aq @ s_phi[p]) for p in s_phi}
    s_E["rest"] += float((np.abs(q * chi) + 0.5 * np.abs(J) * q * q).sum())
    return SimpleNamespace(phi=phi, mu=mu, E=E, ffix=ffix, strain=strain, s_phi=s_phi, s_mu=s_mu, s_E=s_E, s_ffix=s_ffix, s_strain=s_strain)


def coulomb_site64(xyz, q, ke, alpha=0.0, sigma=None, chi=None, hard=None, self_term=0, pairs=None, scale=None):
    """One open molecule: a namespace with phi (n,), mu (n,), E, ffix (n, 3), strain (3, 3) (the virial at fixed charges, dE/d eps under
    r -> (1 + eps) r) and the absolute sums s_phi, s_mu, s_ffix (n,), s_E, s_strain (3, 3), each a dict of "real", "rec" (zeros), "rest"."""
    r = np.asarray(xyz, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    n = r.shape[0]
    gam, w, chi, J, bare = _site(n, alpha, sigma, chi, hard, self_term)
    d = r[:, None, :] - r[None, :, :]
    D = np.sqrt((d * d).sum(-1))
    off = ~np.eye(n, dtype=bool)
    Ds = np.where(off, D, 1.0)
    e, _, g = _erf_terms(Ds, gam, bare)
    kap = np.where(off, e / Ds, 0.0)
    dkap = np.where(off, -g / (Ds * Ds), 0.0)
    qq = q[:, None] * q[None, :]
    aq = np.abs(q)
    x = _listed(r, q, ke, gam, bare, None, pairs, scale)
    phi = ke * (kap @ q) + x.dphi
    ffix = -ke * ((qq * dkap / Ds)[:, :, None] * d).sum(1) + x.dffix
    dd = d[:, :, :, None] * d[:, :, None, :]
    strain = 0.5 * ke * ((qq * dkap / Ds)[:, :, None, None] * dd).sum((0, 1)) + x.dstrain
    s_phi = {"real": ke * (kap @ aq) + x.s_phi, "rec": np.zeros(n), "rest": np.zeros(n)}
    s_ffix = {"real": ke * aq * (np.abs(dkap) @ aq) + x.s_ffix, "rec": np.zeros(n), "rest": np.zeros(n)}
    s_strain = {"real": 0.5 * ke * ((np.abs(qq * dkap) / Ds)[:, :, None, None] * np.abs(dd)).sum((0, 1)) + x.s_strain,
                "rec": np.zeros((3, 3)), "rest": np.zeros((3, 3))}
    return _finish(q, ke, phi, ffix, strain, s_phi, s_ffix, s_strain, gam, chi, J, self_term)


def ewald_site64(xyz, q, cell, ke, alpha, sigma, chi, hard, self_term, beta, rc, kc, M, pairs=None, scale=None):
    """One cell at the parameters beta, rc, kc, M (3,): the namespace of coulomb_site64, strain the fixed-charge dE/d eps under a
    homogeneous strain of coordinates and cell.  xyz, q and cell are taken as given (float64 cells stay off the float32 grid)."""
    r = np.asarray(xyz, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    n = r.shape[0]
    gam, w, chi, J, bare = _site(n, alpha, sigma, chi, hard, self_term)
    a, g = cell_ref.duals64(np.asarray(cell, dtype=np.float64))
    V = abs(np.linalg.det(a))
    aq, Qs, Qa = np.abs(q), q.sum(), np.abs(q).sum()
    # ---- real space: [erf(gamma_ij D) - erf(beta D)] / D between the complements
    d = cell_ref.mic64(r[:, None, :] - r[None, :, :], a, g)
    D = np.sqrt((d * d).sum(-1))
    use = ~np.eye(n, dtype=bool) & (D <= rc)
    Ds = np.where(use, D, 1.0)
    ea, eca, ga = _erf_terms(Ds, gam, bare)
    eb, ecb, gb = _erf(beta * Ds), _erfc(beta * Ds), g64(beta * Ds)
    kap = np.where(use, (ecb - eca) / Ds, 0.0)
    akap = np.where(use, (ea + eb) / Ds, 0.0)
    dkap = np.where(use, -(ga - gb) / (Ds * Ds), 0.0)
    adkap = np.where(use, (ga + gb) / (Ds * Ds), 0.0)
    qq = q[:, None] * q[None, :]
    x = _listed(r, q, ke, gam, bare, a, pairs, scale)
    phi = ke * (kap @ q) + x.dphi
    ffix = -ke * ((qq * dkap / Ds)[:, :, None] * d).sum(1) + x.dffix
    dd = d[:, :, :, None] * d[:, :, None, :]
    strain = 0.5 * ke * ((qq * dkap / Ds)[:, :, None, None] * dd).sum((0, 1)) + x.dstrain
    s_phi = {"real": ke * (akap @ aq) + x.s_phi}
    s_ffix = {"real": ke * aq * (adkap @ aq) + x.s_ffix}
    s_strain = {"real": 0.5 * ke * ((np.abs(qq) * adkap / Ds)[:, :, None, None] * np.abs(dd)).sum((0, 1)) + x.s_strain}
    # ---- reciprocal space: the point charges' sum of ewald_ref.ewald64, the whole sphere
    M = [int(v) for v in M]
    m = np.stack(np.meshgrid(*[np.arange(-v, v + 1) for v in M], indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    k = 2.0 * math.pi * (m @ g)
    k2 = (k * k).sum(1)
    keep = (k2 > 0) & (np.sqrt(k2) <= kc)
    m, k, k2 = m[keep], k[keep], k2[keep]
    c = ke * 4.0 * math.pi / V * np.exp(-k2 / (4.0 * beta * beta)) / k2
    frac = r @ g.T
    frac -= np.rint(frac)
    th = 2.0 * math.pi * (frac @ m.T)
    S = (q[:, None] * np.exp(1j * th)).sum(0)
    T = np.exp(-1j * th) * S[None, :]
    phi += T.real @ c
    ffix -= q[:, None] * ((T.imag * c[None, :]) @ k)
    wk = 0.5 * c * np.abs(S) ** 2
    u = 2.0 * (1.0 / k2 + 0.25 / (beta * beta))
    kk = k[:, :, None] * k[:, None, :]
    strain += (wk[:, None, None] * (u[:, None, None] * kk - np.eye(3)[None])).sum(0)
    s_phi["rec"] = np.full(n, c.sum() * Qa)
    s_ffix["rec"] = aq * (c * np.sqrt(k2)).sum() * Qa
    s_strain["rec"] = 0.5 * Qa * Qa * (c[:, None, None] * (u[:, None, None] * np.abs(kk) + np.eye(3)[None])).sum(0)
    # ---- the split's self term and the background, per pair
    self_t = -ke * TWO_RPI * beta * q
    bg_t = -ke * math.pi / V * (Qs / (beta * beta) - w * Qs - float(q @ w))
    phi += self_t + bg_t
    E_bg = 0.5 * float(q @ bg_t)
    strain -= E_bg * np.eye(3)
    s_phi["rest"] = np.abs(self_t) + np.abs(bg_t)
    s_ffix["rest"] = np.zeros(n)
    s_strain["rest"] = abs(E_bg) * np.eye(3)
    out = _finish(q, ke, phi, ffix, strain, s_phi, s_ffix, s_strain, gam, chi, J, self_term)
    out.E_bg = E_bg
    return out


def ewald_gauss_recip64(xyz, q, cell, ke, sigma, tiny=1e-34):
    """The energy of Gaussian charges of widths sigma in a cell, self-energy included, from the reciprocal sum alone:
        E = 1/2 sum_{k != 0} (4 pi ke / V k^2) |sum_j q_j exp(-k^2 sigma_j^2 / 2) exp(i k r_j)|^2
    over every k with exp(-k^2 sigma_min^2) >= tiny.  No beta, no real-space part.  k = 0 is left out, which is the convention in
    which every pair potential averages to zero over the cell: that of the background term of ewald_site64, E_bg included."""
    r = np.asarray(xyz, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    s = np.asarray(sigma, dtype=np.float64)
    a, g = cell_ref.duals64(np.asarray(cell, dtype=np.float64))
    V = abs(np.linalg.det(a))
    kmax = math.sqrt(-math.log(tiny)) / s.min()
    M = np.ceil(kmax * np.sqrt((a * a).sum(1)) / (2.0 * math.pi)).astype(int)
    m = np.stack(np.meshgrid(*[np.arange(-v, v + 1) for v in M], indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    k = 2.0 * math.pi * (m @ g)
    k2 = (k * k).sum(1)
    keep = (k2 > 0) & (k2 <= kmax * kmax)
    m, k2 = m[keep], k2[keep]
    frac = r @ g.T
    E = 0.0
    for lo in range(0, len(k2), 20000):
        th = 2.0 * math.pi * (frac @ m[lo:lo + 20000].T)
        S = (q[:, None] * np.exp(-0.5 * k2[None, lo:lo + 20000] * (s * s)[:, None]) * np.exp(1j * th)).sum(0)
        E += float((0.5 * ke * 4.0 * math.pi / V / k2[lo:lo + 20000] * np.abs(S) ** 2).sum())
    return E
