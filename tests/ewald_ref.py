"""Float64 reference for the electrostatics of the predicted charges in fully periodic cells (epnn_coulomb_xyz_cell). Test helper.

The Ewald sum of include/epnn.h, written out term by term over one cell H (3,3), V = |det H|, Q = sum q_i, d_ij the minimum image
(cell_ref.mic64) and D = |d_ij|; e_alpha = 1 (alpha == 0) or erf(alpha D), g from coulomb_ref.g64 with g_0 = 1:
    real        kappa_s = [e_alpha - erf(beta D)] / D for j != i, D <= rc;  kappa_s' = -[g_alpha - g_beta] / D^2
    reciprocal  k = 2 pi m G != 0, |k| <= kc, the whole sphere;  c = ke 4 pi / V exp(-k^2 / 4 beta^2) / k^2;  S = sum_j q_j exp(i k r_j)
                phi_i += sum_k c Re[exp(-i k r_i) S];  ffix_i -= q_i sum_k c k Im[exp(-i k r_i) S];  E_rec = 1/2 sum_k c |S|^2
    self        phi_i -= ke 2 beta / sqrt(pi) q_i;     background  phi_i -= ke pi Q / V (1 / beta^2 - [alpha > 0] / alpha^2)
    E = 1/2 sum q_i phi_i;  strain (fixed charges) = 1/2 ke sum_{i != j} q_i q_j kappa_s' d_a d_b / D
                + 1/2 sum_k c |S|^2 [-delta_ab + 2 k_a k_b (1 / k^2 + 1 / 4 beta^2)] - E_bg delta_ab
Beside every result the sum of its absolute terms, by part: a real term counts (e_alpha + erf(beta D)) / D (and (g_alpha + g_beta) / D^2),
so that the cancellation at alpha ~ beta is the kernel's to get right and not hidden in the scale; a reciprocal term counts
c(k) sum_j |q_j|; the self and background terms count as they are.
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

SLOT_CAP = 1 << 18


def ewald_params64(cell, alpha, tol):
    """The rule of epnn_ewald_params in numpy: float64 (6,) = beta, rc, kc, M0, M1, M2."""
    a = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    s = math.sqrt(-math.log(tol))
    _, g = cell_ref.duals64(a)
    rc = 0.5 * (1.0 / np.sqrt((g * g).sum(1))).min()
    beta = s / rc
    if alpha > 0 and alpha <= beta:
        beta, rc = alpha, 0.0
    kc = 2.0 * beta * s
    M = np.ceil(kc * np.sqrt((a * a).sum(1)) / (2.0 * math.pi))
    return np.array([beta, rc, kc, M[0], M[1], M[2]])


def _e_and_g(D, alpha):
    """(e_alpha, complement 1 - e_alpha, g_alpha) at the distances D."""
    if alpha == 0:
        return np.ones_like(D), np.zeros_like(D), np.ones_like(D)
    return _erf(alpha * D), _erfc(alpha * D), g64(alpha * D)


def ewald64(xyz, q, cell, ke, alpha, beta, rc, kc, M):
    """One cell.  xyz (n,3), q (n,), cell (3,3) are taken as given (float32 arrays convert exactly; a float64 cell stays as it
    is: finite differences deform it off the float32 grid).  Returns a namespace: phi (n,), E, ffix (n,3), strain (3,3), and the
    sums of absolute terms s_phi (n,), s_E, s_ffix (n,), s_strain (3,3), each as a dict of its parts "real", "rec", "rest"."""
    r = np.asarray(xyz, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    n = r.shape[0]
    a, g = cell_ref.duals64(np.asarray(cell, dtype=np.float64))
    V = abs(np.linalg.det(a))
    aq, Qs, Qa = np.abs(q), q.sum(), np.abs(q).sum()
    # ---- real space
    d = cell_ref.mic64(r[:, None, :] - r[None, :, :], a, g)
    D = np.sqrt((d * d).sum(-1))
    use = ~np.eye(n, dtype=bool) & (D <= rc)
    Ds = np.where(use, D, 1.0)
    ea, eca, ga = _e_and_g(Ds, alpha)
    eb, ecb, gb = _erf(beta * Ds), _erfc(beta * Ds), g64(beta * Ds)
    kap = np.where(use, (ecb - eca) / Ds if alpha > 0 else ecb / Ds, 0.0)        # e_alpha - erf(beta D) between the complements
    akap = np.where(use, (ea + eb) / Ds, 0.0)
    gs = (1.0 - gb if alpha == 0 else ga - gb)
    dkap = np.where(use, -gs / (Ds * Ds), 0.0)
    adkap = np.where(use, (ga + gb) / (Ds * Ds), 0.0)
    qq = q[:, None] * q[None, :]
    phi = ke * (kap @ q)
    ffix = -ke * ((qq * dkap / Ds)[:, :, None] * d).sum(1)
    dd = d[:, :, :, None] * d[:, :, None, :]
    strain = 0.5 * ke * ((qq * dkap / Ds)[:, :, None, None] * dd).sum((0, 1))
    s_phi = {"real": ke * (akap @ aq)}
    s_ffix = {"real": ke * aq * (adkap @ aq)}
    s_strain = {"real": 0.5 * ke * ((np.abs(qq) * adkap / Ds)[:, :, None, None] * np.abs(dd)).sum((0, 1))}
    # ---- reciprocal space, the whole sphere
    M = [int(v) for v in M]
    m = np.stack(np.meshgrid(*[np.arange(-v, v + 1) for v in M], indexing="ij"), -1).reshape(-1, 3).astype(np.float64)
    k = 2.0 * math.pi * (m @ g)
    k2 = (k * k).sum(1)
    keep = (k2 > 0) & (np.sqrt(k2) <= kc)
    m, k, k2 = m[keep], k[keep], k2[keep]
    c = ke * 4.0 * math.pi / V * np.exp(-k2 / (4.0 * beta * beta)) / k2
    frac = r @ g.T
    frac -= np.rint(frac)
    th = 2.0 * math.pi * (frac @ m.T)                                            # (n, nk): k . r_j
    S = (q[:, None] * np.exp(1j * th)).sum(0)
    T = np.exp(-1j * th) * S[None, :]                                            # exp(-i k r_i) S(k)
    phi += T.real @ c
    ffix -= q[:, None] * ((T.imag * c[None, :]) @ k)
    w = 0.5 * c * np.abs(S) ** 2
    u = 2.0 * (1.0 / k2 + 0.25 / (beta * beta))
    kk = k[:, :, None] * k[:, None, :]
    strain += (w[:, None, None] * (u[:, None, None] * kk - np.eye(3)[None])).sum(0)
    s_phi["rec"] = np.full(n, c.sum() * Qa)
    s_ffix["rec"] = aq * (c * np.sqrt(k2)).sum() * Qa
    s_strain["rec"] = 0.5 * Qa * Qa * (c[:, None, None] * (u[:, None, None] * np.abs(kk) + np.eye(3)[None])).sum(0)
    # ---- self and background
    bgc = math.pi / V * (1.0 / (beta * beta) - (1.0 / (alpha * alpha) if alpha > 0 else 0.0))
    self_t = -ke * 2.0 * beta / math.sqrt(math.pi) * q
    bg_t = -ke * bgc * Qs
    phi += self_t + bg_t
    E_bg = 0.5 * Qs * bg_t
    strain -= E_bg * np.eye(3)
    s_phi["rest"] = np.abs(self_t) + abs(bg_t)
    s_ffix["rest"] = np.zeros(n)
    s_strain["rest"] = abs(E_bg) * np.eye(3)
    s_E = {p: 0.5 * float(aq @ s_phi[p]) for p in ("real", "rec", "rest")}
    return SimpleNamespace(phi=phi, E=0.5 * float(q @ phi), ffix=ffix, strain=strain, s_phi=s_phi, s_E=s_E, s_ffix=s_ffix,
                           s_strain=s_strain)


def ewald_forces64(xyz, x, Q, cell, weights, N, ke, alpha, params, kink_shift=0.0, dtype=np.float64, **ref_kw):
    """(q (n,), phi (n,), E, f (n,3), gstrain (3,3), ffix, fq, gstrain_fix, gstrain_q) of one cell padded to N: q from
    cell_ref.forward64_cell, the fixed-charge parts from ewald64 on them at params = (beta, rc, kc, M0, M1, M2), fq = -gxyz and
    gstrain_q = gstrain of cell_ref.strain64 at g = phi, as coulomb_ref.coulomb_forces64 does for open molecules (dtype as there:
    charges and the backward from the float32 model, its seed phi rounded to float32)."""
    n = np.asarray(x).shape[0]
    f64 = np.dtype(dtype) == np.float64
    if f64:
        q = cell_ref.forward64_cell(xyz, x, Q, cell, weights, N=N, **ref_kw)[:n]
    else:
        q = cell_ref.strain64(xyz, x, Q, np.zeros(n), cell, weights, N=N, dtype=dtype, **ref_kw)[0][:n].astype(np.float32).astype(np.float64)
    e = ewald64(np.asarray(xyz, dtype=np.float32), q, np.asarray(cell, dtype=np.float32), ke, alpha, params[0], params[1], params[2], params[3:6])
    if not f64:
        e.phi = e.phi.astype(np.float32).astype(np.float64)
    _, gxyz, gsq = cell_ref.strain64(xyz, x, Q, e.phi, cell, weights, N=N, kink_shift=kink_shift, dtype=dtype, **ref_kw)
    return q, e.phi, e.E, e.ffix - gxyz, e.strain + gsq, e.ffix, -gxyz, e.strain, gsq
