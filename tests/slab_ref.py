"""Float64 reference for the electrostatics of the predicted charges in slab cells (epnn_coulomb_xyz_slab). Test helper.

The exact two-dimensional Ewald sum of include/epnn.h, term by term over one cell with two periodic rows a, b and one row of zeros:
A = |a x b|, nhat = a x b / A, d_ij = r_i - r_j, z = nhat . d_ij, beta the splitting parameter; e_alpha = 1 (alpha == 0) or erf(alpha D):
    real        kappa_s = [e_alpha - erf(beta D)] / D over the minimum image (cell_ref.mic64; z is not wrapped), j != i, D <= rc
    reciprocal  k = 2 pi (m0 g_a + m1 g_b) != 0, |k| <= kc; u = k / 2 beta;   (summed over the half plane, doubled: the summand is even in k)
                F+ = e^{kz} erfc(u + beta z), F- = e^{-kz} erfc(u - beta z)
                phi_i  += sum_k pi / (A k) sum_j q_j cos(k . d_ij) [F+ + F-]                                      (j == i included)
                ffix_i -= q_i sum_k pi / (A k) sum_j q_j {-k sin(k . d_ij) [F+ + F-] + nhat k cos(k . d_ij) [F+ - F-]}
    k = 0       phi_i  -= 2 sqrt(pi) / A sum_j q_j [exp(-beta^2 z^2) / beta + sqrt(pi) z erf(beta z)];  ffix_i += q_i nhat 2 pi / A sum_j q_j erf(beta z)
    self        phi_i  -= 2 beta / sqrt(pi) q_i;       E = 1/2 sum q_i phi_i        (all times ke; no background, whatever Q)
F+- through erfcx (scipy.special), without overflow or cancellation.  Beside every result the sum of its absolute terms, by part, in
the convention of ewald_ref.ewald64: "real" counts (e_alpha + erf(beta D)) / D and (g_alpha + g_beta) / D^2; "rec" counts
pi / (A k) [F+ + F-] |q_j| over all j, for the forces k times that; "k0" counts 2 sqrt(pi) / A (exp(-beta^2 z^2) / beta + sqrt(pi) |z|
erf(beta |z|)) |q_j|, for the forces 2 pi / A erf(beta |z|) |q_i q_j|; "rest" the self term.
"""
from __future__ import annotations

import math
from types import SimpleNamespace

import numpy as np
from scipy.special import erf as _erf, erfc as _erfc, erfcx as _erfcx

import cell_ref
from coulomb_ref import g64

SLOT_CAP = 1 << 16
PARTS = ("real", "rec", "k0", "rest")


def slab_geometry64(cell):
    """(a, g, periodic rows (p, q), open row, A, nhat) of a float64 cell with exactly one row of zeros."""
    a, g = cell_ref.duals64(np.asarray(cell, dtype=np.float64))
    per = [k for k in range(3) if np.any(a[k] != 0.0)]
    if len(per) != 2:
        raise ValueError(f"a slab cell has exactly two non-zero rows, got {len(per)}")
    n = np.cross(a[per[0]], a[per[1]])
    A = math.sqrt(float(n @ n))
    return a, g, per, ({0, 1, 2} - set(per)).pop(), A, n / A


def slab_params64(cell, alpha, tol):
    """The rule of epnn_ewald_slab_params in numpy: float64 (6,) = beta, rc, kc, M0, M1, M2; M of the open row is 0."""
    a, g, per, _, _, _ = slab_geometry64(np.asarray(cell, dtype=np.float32))
    s = math.sqrt(-math.log(tol))
    rc = 0.5 * min(1.0 / math.sqrt(float(g[k] @ g[k])) for k in per)
    beta = s / rc
    if alpha > 0 and alpha <= beta:
        beta, rc = alpha, 0.0
    kc = 2.0 * beta * s
    M = np.zeros(3)
    for k in per:
        M[k] = math.ceil(kc * math.sqrt(float(a[k] @ a[k])) / (2.0 * math.pi))
    return np.array([beta, rc, kc, M[0], M[1], M[2]])


def _fpm(k, u, beta, z):
    """(F+ + F-, F+ - F-) at k, u (nk,) and z (n, n): arrays (n, n, nk)."""
    az = np.abs(z)[:, :, None]
    ex = np.exp(-u * u - (beta * az) ** 2)
    Fa = ex * _erfcx(u + beta * az)                                              # the one whose erfc argument is u + beta |z|
    am = u - beta * az
    with np.errstate(over="ignore", invalid="ignore"):                          # (erfcx of the other branch's argument)
        Fb = np.where(am >= 0, ex * _erfcx(np.where(am >= 0, am, 0.0)), 2.0 * np.exp(-k * az) - ex * _erfcx(np.where(am < 0, -am, 0.0)))
    return Fa + Fb, np.sign(z)[:, :, None] * (Fa - Fb)


def slab64(xyz, q, cell, ke, alpha, beta, rc, kc, M):
    """One cell.  xyz (n,3), q (n,), cell (3,3) are taken as given (float32 arrays convert exactly).  Returns a namespace: phi (n,), E,
    ffix (n,3), and the sums of absolute terms s_phi (n,), s_E, s_ffix (n,), each a dict of its parts "real", "rec", "k0", "rest"."""
    r = np.asarray(xyz, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    n = r.shape[0]
    a, g, per, open_row, A, nhat = slab_geometry64(cell)
    aq = np.abs(q)
    if M[open_row] != 0:
        raise ValueError("M of the open row must be 0")
    # ---- real space
    d = cell_ref.mic64(r[:, None, :] - r[None, :, :], a, g)
    D = np.sqrt((d * d).sum(-1))
    use = ~np.eye(n, dtype=bool) & (D <= rc)
    Ds = np.where(use, D, 1.0)
    if alpha == 0:
        ea, eca, ga = np.ones_like(Ds), np.zeros_like(Ds), np.ones_like(Ds)
    else:
        ea, eca, ga = _erf(alpha * Ds), _erfc(alpha * Ds), g64(alpha * Ds)
    eb, ecb, gb = _erf(beta * Ds), _erfc(beta * Ds), g64(beta * Ds)
    kap = np.where(use, (ecb - eca) / Ds if alpha > 0 else ecb / Ds, 0.0)
    akap = np.where(use, (ea + eb) / Ds, 0.0)
    dkap = np.where(use, -(1.0 - gb if alpha == 0 else ga - gb) / (Ds * Ds), 0.0)
    adkap = np.where(use, (ga + gb) / (Ds * Ds), 0.0)
    qq = q[:, None] * q[None, :]
    phi = ke * (kap @ q)
    ffix = -ke * ((qq * dkap / Ds)[:, :, None] * d).sum(1)
    s_phi = {"real": ke * (akap @ aq)}
    s_ffix = {"real": ke * aq * (adkap @ aq)}
    # ---- reciprocal space: the half plane m1 > 0, or m1 == 0 and m0 > 0, with the weight doubled
    p, b = per
    m0, m1 = np.meshgrid(np.arange(-int(M[p]), int(M[p]) + 1), np.arange(-int(M[b]), int(M[b]) + 1), indexing="ij")
    m = np.stack([m0.ravel(), m1.ravel()], -1).astype(np.float64)
    kv = 2.0 * math.pi * (m[:, :1] * g[p][None, :] + m[:, 1:] * g[b][None, :])
    k = np.sqrt((kv * kv).sum(1))
    keep = (k <= kc) & ((m[:, 1] > 0) | ((m[:, 1] == 0) & (m[:, 0] > 0)))
    m, kv, k = m[keep], kv[keep], k[keep]
    u = k / (2.0 * beta)
    c = 2.0 * math.pi / (A * k)
    s_phi.update(rec=np.zeros(n), k0=np.zeros(n))
    s_ffix.update(rec=np.zeros(n), k0=np.zeros(n))
    for i0 in range(0, n, 32):                                                   # (row blocks: the (n, n, nk) arrays stay small)
        I = slice(i0, min(i0 + 32, n))
        dr = r[I, None, :] - r[None, :, :]
        z = dr @ nhat
        frac = np.stack([dr @ g[p], dr @ g[b]], -1)
        frac -= np.rint(frac)
        th = 2.0 * math.pi * (frac @ m.T)                                        # (rows, n, nk): k . d_ij
        Fs, Fd = _fpm(k, u, beta, z)
        phi[I] += ke * (((np.cos(th) * Fs) @ c) @ q)
        inpl = np.einsum("ijk,k,kx->ijx", np.sin(th) * Fs, c, kv)               # sum_k c k sin [F+ + F-]
        norm = (np.cos(th) * Fd) @ (c * k)                                       # sum_k c k cos [F+ - F-]
        ffix[I] -= ke * q[I, None] * ((-inpl + norm[:, :, None] * nhat[None, None, :]) * q[None, :, None]).sum(1)
        s_phi["rec"][I] = ke * ((Fs @ c) @ aq)
        s_ffix["rec"][I] = ke * aq[I] * ((Fs @ (c * k)) @ aq)
        # ---- k = 0
        az = np.abs(z)
        t0 = 2.0 * math.sqrt(math.pi) / A * (np.exp(-(beta * z) ** 2) / beta + math.sqrt(math.pi) * az * _erf(beta * az))
        phi[I] -= ke * (t0 @ q)
        ffix[I] += ke * q[I, None] * nhat[None, :] * (2.0 * math.pi / A * (_erf(beta * z) @ q))[:, None]
        s_phi["k0"][I] = ke * (t0 @ aq)
        s_ffix["k0"][I] = ke * aq[I] * (2.0 * math.pi / A * (_erf(beta * az) @ aq))
    # ---- self
    self_t = -ke * 2.0 * beta / math.sqrt(math.pi) * q
    phi += self_t
    s_phi["rest"] = np.abs(self_t)
    s_ffix["rest"] = np.zeros(n)
    s_E = {part: 0.5 * float(aq @ s_phi[part]) for part in PARTS}
    return SimpleNamespace(phi=phi, E=0.5 * float(q @ phi), ffix=ffix, s_phi=s_phi, s_E=s_E, s_ffix=s_ffix)


def slab_forces64(xyz, x, Q, cell, weights, N, ke, alpha, params, kink_shift=0.0, dtype=np.float64, **ref_kw):
    """(q (n,), phi (n,), E, f (n,3), ffix, fq) of one slab cell padded to N: q from cell_ref.forward64_cell, the fixed-charge parts
    from slab64 on them at params = (beta, rc, kc, M0, M1, M2), fq = -gxyz of cell_ref.strain64 at g = phi, as
    ewald_ref.ewald_forces64 does for fully periodic cells (dtype as there)."""
    n = np.asarray(x).shape[0]
    f64 = np.dtype(dtype) == np.float64
    if f64:
        q = cell_ref.forward64_cell(xyz, x, Q, cell, weights, N=N, **ref_kw)[:n]
    else:
        q = cell_ref.strain64(xyz, x, Q, np.zeros(n), cell, weights, N=N, dtype=dtype, **ref_kw)[0][:n].astype(np.float32).astype(np.float64)
    e = slab64(np.asarray(xyz, dtype=np.float32), q, np.asarray(cell, dtype=np.float32), ke, alpha, params[0], params[1], params[2], params[3:6])
    if not f64:
        e.phi = e.phi.astype(np.float32).astype(np.float64)
    _, gxyz, _ = cell_ref.strain64(xyz, x, Q, e.phi, cell, weights, N=N, kink_shift=kink_shift, dtype=dtype, **ref_kw)
    return q, e.phi, e.E, e.ffix - gxyz, e.ffix, -gxyz
