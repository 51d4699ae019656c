"""Float64 reference for the strain derivative of the slab Ewald sum (epnn_coulomb_xyz_slab_strain). Test helper, beside slab_ref.py.

The strain is that of charges_vjp_xyz(strain=True): r -> (1 + eps) r and a_k -> (1 + eps) a_k with eps symmetric; beta, rc, kc, the
listed k slots (m0, m1) and the set of in-range pairs are held fixed.  To first order A -> A (1 + tr eps - n eps n), |k| -> |k| -
(k eps k) / |k|, z_ij -> z_ij (1 + n eps n) and the phase k . d_ij changes by 2 z_ij (n eps k): the plane tilts under a symmetric
out-of-plane shear and the in-plane dual vectors stay in it.  With c = pi / (A k) over the whole plane (here the half plane of
slab_ref.slab64, doubled), Fs = F+ + F-, Fd = F+ - F-, theta = k . d_ij, u = k / 2 beta:
    dFs/dz = k Fd;   dFs/dk = z Fd - 2 / (beta sqrt(pi)) exp(-u^2 - beta^2 z^2);   d/dz [k = 0 bracket] = sqrt(pi) erf(beta z)
    W_ab = -(E_rec + E_k0) (delta_ab - n_a n_b)
           + 1/2 sum_ij q_i q_j sum_k c cos(theta) [Fs / k^2 - (dFs/dk) / k] k_a k_b
           + n_a n_b 1/2 sum_ij q_i q_j z_ij {sum_k c k cos(theta) Fd - (2 pi / A) erf(beta z_ij)}
           - 1/2 sum_ij q_i q_j z_ij sum_k c sin(theta) Fs (n_a k_b + k_a n_b)                          (j == i included; times ke)
    real space: 1/2 ke sum_{i != j} q_i q_j kappa_s'(D) d_a d_b / D, the periodic call's (ewald_ref.ewald64)
    listed pairs: ke (s - 1) q_i q_j kappa_alpha'(D) d_a d_b / D once per pair (coulomb_excl_ref.excl_correction64)
The self term has no strain, and there is no background.  Beside the result the sums of the absolute terms actually added, by part
and per component, in the convention of ewald_ref / slab_ref (cosine and sine count as 1, charges by their absolute values):
"real" as ewald_ref; "rec" counts, with |Fd| taken as Fs as slab_ref does for the force along nhat, c Fs |delta_ab - n_a n_b|,
c [Fs / k^2 + (|z| Fs + G) / k] {k_a k_b}, G the Gaussian term of dFs/dk (the bracket's three terms are of one sign: nothing cancels
inside it), c k |z| Fs |n_a n_b| and c |z| Fs (|n_a| {k_b} + {k_a} |n_b|), where {.} is the absolute sum in the basis the terms are
added in, that of the slot integers: {k_a} = 2 pi (|m0 g_a,a| + |m1 g_b,a|) and {k_a k_b} = 4 pi^2 (m0^2 |g_a,a g_a,b| + |m0 m1|
(|g_a,a g_b,b| + |g_b,a g_a,b|) + m1^2 |g_b,a g_b,b|), which are |k_a| and |k_a k_b| in a rectangular cell; "k0" counts the k = 0
bracket times |delta_ab - n_a n_b| and (2 pi / A) |z| erf(beta |z|) |n_a n_b|; "excl" the listed pairs' terms.
"""
from __future__ import annotations

import math

import numpy as np
from scipy.special import erf as _erf, erfc as _erfc

import cell_ref
import coulomb_excl_ref as xref
from coulomb_ref import g64, kappa64
from slab_ref import _fpm, slab64, slab_geometry64


def slab_slots64(cell, kc, M):
    """The listed slots of slab_ref.slab64: float64 (ns, 2) = (m0, m1) of the half plane m1 > 0, or m1 == 0 and m0 > 0, inside kc."""
    _, g, (p, b), _, _, _ = slab_geometry64(cell)
    m0, m1 = np.meshgrid(np.arange(-int(M[p]), int(M[p]) + 1), np.arange(-int(M[b]), int(M[b]) + 1), indexing="ij")
    m = np.stack([m0.ravel(), m1.ravel()], -1).astype(np.float64)
    kv = 2.0 * math.pi * (m[:, :1] * g[p][None, :] + m[:, 1:] * g[b][None, :])
    k = np.sqrt((kv * kv).sum(1))
    return m[(k <= kc) & ((m[:, 1] > 0) | ((m[:, 1] == 0) & (m[:, 0] > 0)))]


def slab_pairs64(xyz, cell, rc):
    """(mask (n, n) of the in-range pairs j != i, D <= rc, and the lattice shifts (n, n, 3) of their minimum images): what a strained
    evaluation holds fixed."""
    r = np.asarray(xyz, dtype=np.float64)
    a, g, _, _, _, _ = slab_geometry64(cell)
    raw = r[:, None, :] - r[None, :, :]
    d = cell_ref.mic64(raw, a, g)
    D = np.sqrt((d * d).sum(-1))
    return ~np.eye(len(r), dtype=bool) & (D <= rc), np.rint((raw - d) @ g.T)


def slab_energy64(xyz, q, cell, ke, alpha, beta, slots, mask, shifts, exclusions=None):
    """The slab sum's energy by part, {"real", "rec", "k0", "excl"}, of coordinates and cell taken as they are (float64, strained or
    not), on a given slot list (m0, m1) and given in-range pairs with their lattice shifts (slab_slots64, slab_pairs64 of the
    unstrained cell).  Without the self term, which no strain moves."""
    r = np.asarray(xyz, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    a, g, (p, b), _, A, nhat = slab_geometry64(cell)
    qq = q[:, None] * q[None, :]
    raw = r[:, None, :] - r[None, :, :]
    d = raw - shifts @ a
    D = np.where(mask, np.sqrt((d * d).sum(-1)), 1.0)
    kap = (_erfc(beta * D) - _erfc(alpha * D)) / D if alpha > 0 else _erfc(beta * D) / D
    out = {"real": 0.5 * ke * float((qq * np.where(mask, kap, 0.0)).sum())}
    kv = 2.0 * math.pi * (slots[:, :1] * g[p][None, :] + slots[:, 1:] * g[b][None, :])
    k = np.sqrt((kv * kv).sum(1))
    z = raw @ nhat
    th = raw @ kv.T                                                              # (the phase is periodic: no reduction needed in float64)
    Fs, _ = _fpm(k, k / (2.0 * beta), beta, z)
    out["rec"] = 0.5 * ke * float((qq * ((np.cos(th) * Fs) @ (2.0 * math.pi / (A * k)))).sum())
    t0 = 2.0 * math.sqrt(math.pi) / A * (np.exp(-(beta * z) ** 2) / beta + math.sqrt(math.pi) * z * _erf(beta * z))
    out["k0"] = -0.5 * ke * float((qq * t0).sum())
    out["excl"] = 0.0
    if exclusions is not None:
        pairs, scale = xref._lists(*exclusions)
        i, j = pairs[:, 0], pairs[:, 1]
        f = (scale.astype(np.float32) - np.float32(1)).astype(np.float64)
        dn = raw[i, j] - shifts[i, j] @ a                                       # the nearest image of the unstrained cell, whatever rc is
        Dn = np.sqrt((dn * dn).sum(-1))
        out["excl"] = float((ke * f * q[i] * q[j] * kappa64(Dn, alpha)[0]).sum())
    return out


def slab_strain64(xyz, q, cell, ke, alpha, beta, rc, kc, M, exclusions=None):
    """(strain (3, 3), s_strain) of one cell at fixed charges: dE/d eps of slab_ref.slab64's energy (plus the listed pairs' correction,
    exclusions = (pairs, scale)), and the sums of the absolute terms by part, a dict of (3, 3) arrays: "real", "rec", "k0" and, with a
    list, "excl"."""
    r = np.asarray(xyz, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    n = r.shape[0]
    a, g, (p, b), open_row, A, nhat = slab_geometry64(cell)
    if M[open_row] != 0:
        raise ValueError("M of the open row must be 0")
    qq = q[:, None] * q[None, :]
    aqq = np.abs(qq)
    eye, nn = np.eye(3), np.outer(nhat, nhat)
    # ---- real space: ewald_ref.ewald64's
    d = cell_ref.mic64(r[:, None, :] - r[None, :, :], a, g)
    D = np.sqrt((d * d).sum(-1))
    use = ~np.eye(n, dtype=bool) & (D <= rc)
    Ds = np.where(use, D, 1.0)
    ga = np.ones_like(Ds) if alpha == 0 else g64(alpha * Ds)
    gb = g64(beta * Ds)
    dkap = np.where(use, -(ga - gb) / (Ds * Ds), 0.0)
    adkap = np.where(use, (ga + gb) / (Ds * Ds), 0.0)
    dd = d[:, :, :, None] * d[:, :, None, :]
    W = 0.5 * ke * ((qq * dkap / Ds)[:, :, None, None] * dd).sum((0, 1))
    s = {"real": 0.5 * ke * ((aqq * adkap / Ds)[:, :, None, None] * np.abs(dd)).sum((0, 1))}
    # ---- reciprocal space and k = 0
    m = slab_slots64(cell, kc, M)
    kv = 2.0 * math.pi * (m[:, :1] * g[p][None, :] + m[:, 1:] * g[b][None, :])
    k = np.sqrt((kv * kv).sum(1))
    u = k / (2.0 * beta)
    c = 2.0 * math.pi / (A * k)
    kk = kv[:, :, None] * kv[:, None, :]
    nk = nhat[None, :, None] * kv[:, None, :] + kv[:, :, None] * nhat[None, None, :]
    am, gp, gb_ = np.abs(m), np.abs(g[p]), np.abs(g[b])
    akv = 2.0 * math.pi * (am[:, :1] * gp[None, :] + am[:, 1:] * gb_[None, :])     # {k_a}
    akk = 4.0 * math.pi ** 2 * ((am[:, 0] ** 2)[:, None, None] * np.outer(gp, gp)[None] + (am[:, 1] ** 2)[:, None, None] * np.outer(gb_, gb_)[None]
                                + (am[:, 0] * am[:, 1])[:, None, None] * (np.outer(gp, gb_) + np.outer(gb_, gp))[None])
    ank = np.abs(nhat)[None, :, None] * akv[:, None, :] + akv[:, :, None] * np.abs(nhat)[None, None, :]
    E_rec = E_k0 = sE_rec = sE_k0 = 0.0
    Tk, sTk, Pk, sPk = np.zeros(len(k)), np.zeros(len(k)), np.zeros(len(k)), np.zeros(len(k))
    Nz = sNz = N0 = sN0 = 0.0
    for i0 in range(0, n, 32):
        I = slice(i0, min(i0 + 32, n))
        dr = r[I, None, :] - r[None, :, :]
        z = dr @ nhat
        frac = np.stack([dr @ g[p], dr @ g[b]], -1)
        frac -= np.rint(frac)
        th = 2.0 * math.pi * (frac @ m.T)
        Fs, Fd = _fpm(k, u, beta, z)
        G = 2.0 / (beta * math.sqrt(math.pi)) * np.exp(-u * u - (beta * z[:, :, None]) ** 2)
        cs, sn, z3 = np.cos(th), np.sin(th), z[:, :, None]
        w, aw = qq[I][:, :, None], aqq[I][:, :, None]
        E_rec += 0.5 * ke * float(((w * cs * Fs) @ c).sum())
        sE_rec += 0.5 * ke * float(((aw * Fs) @ c).sum())
        Tk += (w * cs * (Fs / (k * k) - (z3 * Fd - G) / k)).sum((0, 1)) * c
        sTk += (aw * (Fs / (k * k) + (np.abs(z3) * Fs + G) / k)).sum((0, 1)) * c
        Nz += float(((w * z3 * cs * Fd) @ (c * k)).sum())
        sNz += float(((aw * np.abs(z3) * Fs) @ (c * k)).sum())
        Pk += (w * z3 * sn * Fs).sum((0, 1)) * c
        sPk += (aw * np.abs(z3) * Fs).sum((0, 1)) * c
        az = np.abs(z)
        t0 = 2.0 * math.sqrt(math.pi) / A * (np.exp(-(beta * z) ** 2) / beta + math.sqrt(math.pi) * az * _erf(beta * az))
        E_k0 -= 0.5 * ke * float((qq[I] * t0).sum())
        sE_k0 += 0.5 * ke * float((aqq[I] * t0).sum())
        N0 -= float((qq[I] * z * (2.0 * math.pi / A) * _erf(beta * z)).sum())
        sN0 += float((aqq[I] * az * (2.0 * math.pi / A) * _erf(beta * az)).sum())
    W_rec = -E_rec * (eye - nn) + 0.5 * ke * ((Tk[:, None, None] * kk).sum(0) + nn * Nz - (Pk[:, None, None] * nk).sum(0))
    W_k0 = -E_k0 * (eye - nn) + 0.5 * ke * nn * N0
    s["rec"] = sE_rec * np.abs(eye - nn) + 0.5 * ke * ((sTk[:, None, None] * akk).sum(0) + np.abs(nn) * sNz + (sPk[:, None, None] * ank).sum(0))
    s["k0"] = sE_k0 * np.abs(eye - nn) + 0.5 * ke * np.abs(nn) * sN0
    W = W + W_rec + W_k0
    if exclusions is not None:
        cx = xref.excl_correction64(r, q, cell, ke, alpha, *exclusions)
        W = W + cx.dstrain
        s["excl"] = cx.s_strain
    return W, s


def slab_strain_forces64(xyz, x, Q, cell, weights, N, ke, alpha, params, kink_shift=0.0, dtype=np.float64, **ref_kw):
    """(gstrain (3, 3), gstrain_fix, gstrain_q) of one slab cell padded to N, beside slab_ref.slab_forces64: the charges from
    cell_ref.forward64_cell, the fixed-charge part from slab_strain64 on them at params = (beta, rc, kc, M0, M1, M2), the charges' part
    the third value of cell_ref.strain64 at g = phi (phi of slab_ref.slab64 on the same charges)."""
    n = np.asarray(x).shape[0]
    f64 = np.dtype(dtype) == np.float64
    if f64:
        q = cell_ref.forward64_cell(xyz, x, Q, cell, weights, N=N, **ref_kw)[:n]
    else:
        q = cell_ref.strain64(xyz, x, Q, np.zeros(n), cell, weights, N=N, dtype=dtype, **ref_kw)[0][:n].astype(np.float32).astype(np.float64)
    xyz32, cell32 = np.asarray(xyz, dtype=np.float32), np.asarray(cell, dtype=np.float32)
    phi = slab64(xyz32, q, cell32, ke, alpha, params[0], params[1], params[2], params[3:6]).phi
    if not f64:
        phi = phi.astype(np.float32).astype(np.float64)
    fix, _ = slab_strain64(xyz32, q, cell32, ke, alpha, params[0], params[1], params[2], params[3:6])
    _, _, gsq = cell_ref.strain64(xyz, x, Q, phi, cell, weights, N=N, kink_shift=kink_shift, dtype=dtype, **ref_kw)
    return fix + gsq, fix, gsq
