"""Float64 references for per-atom Gaussian widths, self-energy and on-site terms in slab cells (epnn_coulomb_xyz_slab_site,
epnn_coulomb_xyz_slab_strain_site). Test helper, built on slab_ref, slab_strain_ref and site_ref.

One slab cell, its real atoms only.  gamma_ij = 1 / sqrt(2 (sigma_i^2 + sigma_j^2)), or the call's alpha where sigma is None (alpha == 0:
bare 1 / D); gamma_ii = 1 / (2 sigma_i) or alpha; w_ij = s for a listed pair and 1 otherwise.  The sum of slab_ref.slab64 with
    real     kappa_s = [erf(gamma_ij D) - erf(beta D)] / D over the minimum image, j != i, D <= rc
    listed   (s - 1) erf(gamma_ij D) / D on the one nearest image, whatever beta
    self     [self] phi_i += ke 2 gamma_ii q_i / sqrt(pi), behind the split's -ke 2 beta q_i / sqrt(pi)
    mu_i = chi_i + J_i q_i + phi_i;     E = sum_i [chi_i q_i + 1/2 J_i q_i^2 + 1/2 q_i phi_i]
and the reciprocal and k = 0 parts of the point charges as they are: no background and no per-pair k = 0 correction, whatever Q.
The strain is slab_strain_ref.slab_strain64's with the new kappa' in the real-space virial and in the listed pairs' virial; the self
and on-site terms have none.
Beside every result the sums of its absolute terms by part, "real" (with the listed pairs' terms, as site_ref counts them), "rec",
"k0" (both as slab_ref and slab_strain_ref count them) and "rest": the split's and the Gaussians' self terms and, for mu and E, the
on-site terms.
slab_gauss64 is the same energy from the Gaussians' own two-dimensional sum, which has no beta and no real-space part.
"""
from __future__ import annotations

import math

import numpy as np
from scipy.special import erf as _erf, erfc as _erfc, erfcx as _erfcx

import cell_ref
from coulomb_ref import g64
from site_ref import _erf_terms, _finish, _listed, _site
from slab_ref import slab64, slab_geometry64
from slab_strain_ref import slab_strain64

PARTS = ("real", "rec", "k0", "rest")


def slab_site64(xyz, q, cell, ke, alpha, sigma, chi, hard, self_term, beta, rc, kc, M, pairs=None, scale=None):
    """One slab cell at the parameters beta, rc, kc, M (3,): a namespace with phi (n,), mu (n,), E, ffix (n, 3), strain (3, 3) (the
    fixed-charge dE/d eps of slab_strain_ref) and the absolute sums s_phi, s_mu, s_ffix (n,), s_E, s_strain (3, 3), each a dict of
    "real", "rec", "k0", "rest".  xyz, q and cell are taken as given."""
    r = np.asarray(xyz, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    n = r.shape[0]
    gam, _, chi, J, bare = _site(n, alpha, sigma, chi, hard, self_term)
    a, g, _, _, _, _ = slab_geometry64(cell)
    aq = np.abs(q)
    # ---- the point charges' reciprocal, k = 0 and self parts: slab64 without a real-space part (rc = 0: no pair is in range)
    base = slab64(r, q, cell, ke, 0.0, beta, 0.0, kc, M)
    W, sW = slab_strain64(r, q, cell, ke, 0.0, beta, 0.0, kc, M)
    assert not base.s_phi["real"].any() and not sW["real"].any()
    # ---- real space: [erf(gamma_ij D) - erf(beta D)] / D between the complements
    raw = r[:, None, :] - r[None, :, :]
    d = cell_ref.mic64(raw, a, g)
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
    dd = d[:, :, :, None] * d[:, :, None, :]
    phi = base.phi + ke * (kap @ q) + x.dphi
    ffix = base.ffix - ke * ((qq * dkap / Ds)[:, :, None] * d).sum(1) + x.dffix
    strain = W + 0.5 * ke * ((qq * dkap / Ds)[:, :, None, None] * dd).sum((0, 1)) + x.dstrain
    s_phi = {"real": ke * (akap @ aq) + x.s_phi, "rec": base.s_phi["rec"], "k0": base.s_phi["k0"], "rest": base.s_phi["rest"]}
    s_ffix = {"real": ke * aq * (adkap @ aq) + x.s_ffix, "rec": base.s_ffix["rec"], "k0": base.s_ffix["k0"], "rest": np.zeros(n)}
    s_strain = {"real": 0.5 * ke * ((np.abs(qq) * adkap / Ds)[:, :, None, None] * np.abs(dd)).sum((0, 1)) + x.s_strain,
                "rec": sW["rec"], "k0": sW["k0"], "rest": np.zeros((3, 3))}
    return _finish(q, ke, phi, ffix, strain, s_phi, s_ffix, s_strain, gam, chi, J, self_term)


def slab_gauss64(xyz, q, cell, ke, sigma, tiny=1e-34):
    """The energy of Gaussian charges of widths sigma in a slab cell, self-energy included, from their own two-dimensional sum: the
    reciprocal and k = 0 formulas of slab_ref.slab64 with beta = gamma_ij per pair, j == i included (gamma_ii = 1 / (2 sigma_i)),
        E = 1/2 ke sum_ij q_i q_j { sum_{k != 0} pi / (A k) cos(k . d_ij) [F+ + F-](k, z_ij; gamma_ij)
                                    - 2 sqrt(pi) / A [exp(-gamma_ij^2 z_ij^2) / gamma_ij + sqrt(pi) z_ij erf(gamma_ij z_ij)] }
    over every k with exp(-k^2 / (4 gamma_max^2)) >= tiny.  No real-space part, no self term and no splitting parameter: a Gaussian
    pair's interaction erf(gamma D) / D is smooth, its whole lattice sum converges in reciprocal space."""
    r = np.asarray(xyz, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    s2 = np.asarray(sigma, dtype=np.float64) ** 2
    gam = 1.0 / np.sqrt(2.0 * (s2[:, None] + s2[None, :]))
    a, g, (p, b), _, A, nhat = slab_geometry64(cell)
    kmax = 2.0 * gam.max() * math.sqrt(-math.log(tiny))
    Mp, Mb = (int(math.ceil(kmax * math.sqrt(float(a[t] @ a[t])) / (2.0 * math.pi))) for t in (p, b))
    m0, m1 = np.meshgrid(np.arange(-Mp, Mp + 1), np.arange(0, Mb + 1), indexing="ij")
    m = np.stack([m0.ravel(), m1.ravel()], -1).astype(np.float64)
    kv = 2.0 * math.pi * (m[:, :1] * g[p][None, :] + m[:, 1:] * g[b][None, :])
    k = np.sqrt((kv * kv).sum(1))
    keep = (k <= kmax) & ((m[:, 1] > 0) | ((m[:, 1] == 0) & (m[:, 0] > 0)))
    m, k = m[keep], k[keep]
    c = 2.0 * math.pi / (A * k)                                                  # the half plane, doubled
    dr = r[:, None, :] - r[None, :, :]
    z = dr @ nhat
    frac = np.stack([dr @ g[p], dr @ g[b]], -1)
    frac -= np.rint(frac)
    qq = q[:, None] * q[None, :]
    az, gz = np.abs(z), gam * np.abs(z)
    E = -0.5 * ke * float((qq * 2.0 * math.sqrt(math.pi) / A * (np.exp(-gz * gz) / gam + math.sqrt(math.pi) * az * _erf(gz))).sum())
    for lo in range(0, len(k), 2000):
        kk, cc = k[None, None, lo:lo + 2000], c[lo:lo + 2000]
        th = 2.0 * math.pi * (frac @ m[lo:lo + 2000].T)
        u = kk / (2.0 * gam[:, :, None])
        ex = np.exp(-u * u - (gz * gz)[:, :, None])
        Fa = ex * _erfcx(u + gz[:, :, None])
        am = u - gz[:, :, None]
        with np.errstate(over="ignore", invalid="ignore"):
            Fb = np.where(am >= 0, ex * _erfcx(np.where(am >= 0, am, 0.0)),
                          2.0 * np.exp(-kk * az[:, :, None]) - ex * _erfcx(np.where(am < 0, -am, 0.0)))
        E += 0.5 * ke * float((qq * ((np.cos(th) * (Fa + Fb)) @ cc)).sum())
    return E


def slab_site_forces64(xyz, x, Q, cell, weights, N, ke, alpha, params, sigma=None, chi=None, hard=None, self_term=0, pairs=None, scale=None,
                       kink_shift=0.0, dtype=np.float64, **ref_kw):
    """The total-forces twin: (q (n,), e, f (n, 3), fq (n, 3), gstrain (3, 3), gstrain_q) of one slab cell padded to N.  q from
    cell_ref.forward64_cell, e = slab_site64 on them at params = (beta, rc, kc, M0, M1, M2), fq = -gxyz and gstrain_q = the strain rows
    of cell_ref.strain64 at g = e.mu, as slab_ref.slab_forces64 and slab_strain_ref.slab_strain_forces64 do at g = phi (dtype as there)."""
    n = np.asarray(x).shape[0]
    f64 = np.dtype(dtype) == np.float64
    if f64:
        q = cell_ref.forward64_cell(xyz, x, Q, cell, weights, N=N, **ref_kw)[:n]
    else:
        q = cell_ref.strain64(xyz, x, Q, np.zeros(n), cell, weights, N=N, dtype=dtype, **ref_kw)[0][:n].astype(np.float32).astype(np.float64)
    e = slab_site64(np.asarray(xyz, dtype=np.float32), q, np.asarray(cell, dtype=np.float32), ke, alpha, sigma, chi, hard, self_term,
                    params[0], params[1], params[2], params[3:6], pairs=pairs, scale=scale)
    if not f64:
        e.mu = e.mu.astype(np.float32).astype(np.float64)
    _, gxyz, gsq = cell_ref.strain64(xyz, x, Q, e.mu, cell, weights, N=N, kink_shift=kink_shift, dtype=dtype, **ref_kw)
    return q, e, e.ffix - gxyz, -gxyz, e.strain + gsq, gsq
