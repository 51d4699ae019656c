"""Float64 reference for the electrostatics of the predicted charges (epnn_coulomb_xyz). Test helper.

One open molecule, its real atoms only:
    kappa(D) = 1 / D (alpha == 0) or erf(alpha D) / D (alpha > 0)
    phi_i    = ke sum_{j != i} q_j kappa(D_ij)                          E = 1/2 sum_i q_i phi_i
    ffix_i   = -ke q_i sum_{j != i} q_j kappa'(D_ij) (r_i - r_j) / D_ij
    fq_i     = -sum_k phi_k dq_k/dr_i = -vjp64(g = phi)                 f = ffix + fq
The coordinates are taken as given (float32 arrays convert exactly); the charges' part is tests/xyz_grad_ref.py's.
"""
from __future__ import annotations

import math

import numpy as np

from xyz_grad_ref import forward64, vjp64

_erf = np.vectorize(math.erf, otypes=[np.float64])


def kappa64(D, alpha):
    """(kappa, kappa') at the distances D > 0."""
    if alpha == 0:
        return 1.0 / D, -1.0 / (D * D)
    er = _erf(alpha * D)
    return er / D, 2.0 * alpha / math.sqrt(math.pi) * np.exp(-(alpha * D) ** 2) / D - er / (D * D)


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


def coulomb_forces64(xyz, x, Q, weights, N, ke, alpha, kink_shift=0):
    """(q (n,), phi (n,), E, f (n, 3), ffix (n, 3), fq (n, 3)) of one molecule padded to N: q from forward64, phi, E and ffix from
    coulomb64 on them, fq = -vjp64(g = phi) with the reference's ReLU-kink bracket, f = ffix + fq the total force."""
    n = np.asarray(x).shape[0]
    q = forward64(xyz, x, Q, weights, N=N)[:n]
    phi, E, ffix = coulomb64(np.asarray(xyz, dtype=np.float32), q, ke, alpha)[:3]
    fq = -vjp64(xyz, x, Q, phi, weights, N=N, kink_shift=kink_shift)[1]
    return q, phi, E, ffix + fq, ffix, fq
