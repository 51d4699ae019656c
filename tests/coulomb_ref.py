"""Float64 reference for the electrostatics of the predicted charges (epnn_coulomb_xyz). Test helper.

One open molecule, its real atoms only:
    kappa(D) = 1 / D (alpha == 0) or erf(alpha D) / D (alpha > 0);  kappa'(D) = -g(alpha D) / D^2, g = 1 (alpha == 0) or
               g(u) = erf(u) - 2 / sqrt(pi) u exp(-u^2): from its Taylor series below u = 0.5, where the closed form cancels
    phi_i    = ke sum_{j != i} q_j kappa(D_ij)                          E = 1/2 sum_i q_i phi_i
    ffix_i   = -ke q_i sum_{j != i} q_j kappa'(D_ij) (r_i - r_j) / D_ij
    fq_i     = -sum_k phi_k dq_k/dr_i = -vjp64(g = phi)                 f = ffix + fq
The coordinates are taken as given (float32 arrays convert exactly); the charges' part is tests/xyz_grad_ref.py's.
"""
from __future__ import annotations

import math

import numpy as np

from xyz_grad_ref import forward64, vjp64

try:
    from scipy.special import erf as _erf                                   # (the same values to an ulp, and fast at thousands of atoms)
except ImportError:
    _erf = np.vectorize(math.erf, otypes=[np.float64])

G_U0 = 0.5           # g64: the series below it, the closed form from it on; both are good to 1e-12 on G_OVERLAP
G_TERMS = 24         # the 25th term is below 1e-24 of the sum at u = 1
G_OVERLAP = (0.25, 1.0)
_G_COEF = [(-1.0) ** (k + 1) * 2 * k / ((2 * k + 1) * math.factorial(k)) for k in range(1, G_TERMS + 1)]


def g_series64(u):
    """g(u) = 2 / sqrt(pi) sum_{k >= 1} (-1)^(k + 1) 2 k / ((2 k + 1) k!) u^(2 k + 1), G_TERMS terms: no cancellation for u <= 1
    (the first term is 2/3 u^3, the absolute terms add to less than three times the sum at u = 1)."""
    u = np.asarray(u, dtype=np.float64)
    w = u * u
    s = np.full_like(u, _G_COEF[-1])
    for c in _G_COEF[-2::-1]:
        s = s * w + c
    return 2.0 / math.sqrt(math.pi) * (u * w) * s


def g_closed64(u):
    """g(u) = erf(u) - 2 / sqrt(pi) u exp(-u^2) as written: its two terms cancel to 4 / (3 sqrt(pi)) u^3 at small u (a relative
    error of about 1e-16 / u^2, and the error of erf itself on top)."""
    u = np.asarray(u, dtype=np.float64)
    return _erf(u) - 2.0 / math.sqrt(math.pi) * u * np.exp(-u * u)


def g64(u):
    """g(u) for every u >= 0, within 1e-12 relative (tests/test_coulomb_ref.py: against mpmath from 1e-6 to 50)."""
    u = np.asarray(u, dtype=np.float64)
    g = np.asarray(g_closed64(u))
    low = u < G_U0
    if low.any():
        g[low] = g_series64(u[low])
    return g


def kappa64(D, alpha):
    """(kappa, kappa') at the distances D > 0; kappa' = -g(alpha D) / D^2."""
    if alpha == 0:
        return 1.0 / D, -1.0 / (D * D)
    u = alpha * D
    return _erf(u) / D, -g64(u) / (D * D)


def coulomb64(xyz, q, ke, alpha):
    """(phi (n,), E, ffix (n, 3), sum_j |ke q_j kappa| (n,), sum_j |ke q_i q_j kappa'| (n,)), all float64."""
    r = np.asarray(xyz, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    n = r.shape[0]
    d = r[:, None, :] - r[None, :, :]
    D = np.sqrt((d * d).sum(-1))
    off = ~np.eye(n, dtype=bool)
    Ds = np.where(off, D, 1.0)
    kap, dkap = kappa64(Ds, alpha)
    kap = np.where(off, kap, 0.0)
    dkap = np.where(off, dkap, 0.0)
    tp = ke * q[None, :] * kap                                              # the terms of phi_i, by partner
    tf = ke * q[:, None] * q[None, :] * dkap                                # ke q_i q_j kappa'
    phi = tp.sum(1)
    ffix = -((tf / Ds)[:, :, None] * d).sum(1)
    return phi, 0.5 * float(q @ phi), ffix, np.abs(tp).sum(1), np.abs(tf).sum(1)


def coulomb64_rows(xyz, q, ke, alpha, rows=None, block=256):
    """coulomb64's (phi, ffix, sum_j |ke q_j kappa|, sum_j |ke q_i q_j kappa'|) for the atoms `rows` (None: all) of a molecule too large
    for its n x n x 3 arrays: the same expressions, `block` rows at a time against all partners."""
    r = np.asarray(xyz, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    rows = np.arange(r.shape[0]) if rows is None else np.asarray(rows)
    phi, sphi, sff = (np.zeros(len(rows)) for _ in range(3))
    ffix = np.zeros((len(rows), 3))
    for k in range(0, len(rows), block):
        i = rows[k:k + block]
        d = r[i, None, :] - r[None, :, :]
        D = np.sqrt((d * d).sum(-1))
        off = np.ones(D.shape, dtype=bool)
        off[np.arange(len(i)), i] = False
        Ds = np.where(off, D, 1.0)
        kap, dkap = kappa64(Ds, alpha)
        tp = ke * q[None, :] * np.where(off, kap, 0.0)
        tf = ke * q[i, None] * q[None, :] * np.where(off, dkap, 0.0)
        phi[k:k + block], sphi[k:k + block], sff[k:k + block] = tp.sum(1), np.abs(tp).sum(1), np.abs(tf).sum(1)
        ffix[k:k + block] = -((tf / Ds)[:, :, None] * d).sum(1)
    return phi, ffix, sphi, sff


def coulomb_energy64(xyz, q, ke, alpha, block=256):
    """(E, 1/2 sum_ij |ke q_i q_j kappa|) of a large molecule from kappa alone, `block` rows at a time: E = 1/2 sum_i q_i phi_i."""
    r = np.asarray(xyz, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    n = r.shape[0]
    E = sE = 0.0
    for k in range(0, n, block):
        i = np.arange(k, min(k + block, n))
        d = r[i, None, :] - r[None, :, :]
        D = np.sqrt((d * d).sum(-1))
        D[np.arange(len(i)), i] = 1.0
        kap = kappa64(D, alpha)[0] if alpha == 0 else _erf(alpha * D) / D
        kap[np.arange(len(i)), i] = 0.0
        E += 0.5 * ke * float(q[i] @ (kap @ q))
        sE += 0.5 * ke * float(np.abs(q[i]) @ (kap @ np.abs(q)))
    return E, sE


def coulomb_forces64(xyz, x, Q, weights, N, ke, alpha, kink_shift=0, dtype=np.float64, **ref_kw):
    """(q (n,), phi (n,), E, f (n, 3), ffix (n, 3), fq (n, 3)) of one molecule padded to N: q from forward64, phi, E and ffix from
    coulomb64 on them, fq = -vjp64(g = phi) with the reference's ReLU-kink bracket, f = ffix + fq the total force.  ref_kw: the
    references' own keywords (h_dim, cutoff, eta, near_tol: edge_constants.ref_kwargs).  dtype=np.float32: the float32 model of
    the charges' part -- q from vjp64's float32 model, phi from them in float64 and rounded to float32 (the seed the device's
    backward sees), fq from the float32 model's backward; phi, E and ffix are coulomb64's on those charges."""
    n = np.asarray(x).shape[0]
    if np.dtype(dtype) == np.float64:
        q = forward64(xyz, x, Q, weights, N=N, **ref_kw)[:n]
        phi, E, ffix = coulomb64(np.asarray(xyz, dtype=np.float32), q, ke, alpha)[:3]
        fq = -vjp64(xyz, x, Q, phi, weights, N=N, kink_shift=kink_shift, **ref_kw)[1]
        return q, phi, E, ffix + fq, ffix, fq
    q = vjp64(xyz, x, Q, np.zeros(n), weights, N=N, dtype=dtype, **ref_kw)[0][:n].astype(np.float32).astype(np.float64)
    phi, E, ffix = coulomb64(np.asarray(xyz, dtype=np.float32), q, ke, alpha)[:3]
    phi = phi.astype(np.float32).astype(np.float64)
    fq = -vjp64(xyz, x, Q, phi, weights, N=N, kink_shift=kink_shift, dtype=dtype, **ref_kw)[1]
    return q, phi, E, ffix + fq, ffix, fq
