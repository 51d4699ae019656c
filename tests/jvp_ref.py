"""Float64 reference for the forward-mode derivative of the charges (epnn_charges_jvp_xyz_cell). Test helper.

One molecule padded to N, as tests/xyz_grad_ref.py sees it: per-atom x, h = 0, q = Q / n, mask 1 on real pairs, padded partners with
zero rows.  The model is evaluated literally, one row [a_i | a_j | e_ij] per ordered pair and MLP (not in the factorised form the
kernels use), with a tangent beside every tensor:

    coordinates r -> r + t v, strain r -> (1 + t E) r with a_k -> (1 + t E) a_k, total charge Q -> Q + t dQ
    tD_ij = d_ij . (v_i - v_j) / D_ij + d_ij^T E d_ij / D_ij       d_ij the image of r_i - r_j (constant image shifts)
    te_ij = de/dD * tD_ij;  ta_i = [0 | th_i | tq_i];  a Dense layer maps (z, tz) -> (relu(z W + b), [z W + b > kink_shift] tz W)

The geometry goes through tests/cell_ref.py for all three kinds: open molecules are the all-zero cell, a box is its diagonal cell.
The masks (near, node mask) are constants and come from the float32 edge tensor, as in the oracle.  ReLU kinks are bracketed with
kink_shift like the other references.
"""
from __future__ import annotations

import numpy as np

import cell_ref


def cell_of(box=None, cell=None):
    """The (3, 3) float32 cell of the three geometries: open (zeros), box (3,) (diagonal), cell (3, 3)."""
    if box is not None and cell is not None:
        raise ValueError("box and cell are two descriptions of the same thing: give one of them")
    if cell is not None:
        return np.asarray(cell, dtype=np.float32).reshape(3, 3)
    if box is not None:
        return np.diag(np.asarray(box, dtype=np.float32).reshape(3)).astype(np.float32)
    return np.zeros((3, 3), dtype=np.float32)


def near_flags(xyz, cell, h_dim=48, cutoff=3.0, eta=2.0, near_tol=1e-5):
    """is_near of charge_gn.py:90-94 from the float32 edge tensor (n, n) bool."""
    e32, _ = cell_ref.get_init_edges_cell(xyz, cell, num=h_dim, cutoff=cutoff, eta=eta)
    tol = np.float32(near_tol)
    return np.clip(e32, tol, np.float32(1e5)).max(-1) != tol


_CUT_TE = None        # tests/grad_noise_ref.py: a function applied to the edge tangent te as the MLPs see it (a defect model)


def _cast(weights, dtype=np.float64):
    c = lambda m: [(np.asarray(W, dtype), np.asarray(b, dtype)) for W, b in m]
    return {"msg": [c(m) for m in weights["msg"]], "upd": c(weights["upd"]), "pas": [c(m) for m in weights["pas"]]}


def _mlp(X, tX, layers, s):
    for W, b in layers[:-1]:
        pre = X @ W + b
        tX = (tX @ W) * (pre > s)
        X = np.maximum(pre, 0)
    W, b = layers[-1]
    return X @ W + b, tX @ W


def model_jvp(e, te, near, x, q0, tq0, weights, N, kink_shift=0.0, dtype=np.float64):
    """(q (n,), tq (n,)) from float64 edges e, te (n, n, c), near (n, n) bool, x (n, nx), q0 and tq0 (scalars: Q / n, dQ / n).
    dtype=np.float32: the float32 model of the device's tangent kernels -- weights, e and te as the MLPs see them, activations, the
    tangents th and tq and every Dense product and sum in float32, the result rounded to float32; e and te themselves come from the
    float64 geometry either way."""
    w = _cast(weights, dtype)
    s = float(kink_shift)
    n, nx = x.shape
    nh = e.shape[-1]
    E = np.zeros((n, N, nh), dtype=dtype)
    tE = np.zeros((n, N, nh), dtype=dtype)
    E[:, :n] = e
    tE[:, :n] = te
    if _CUT_TE is not None:
        tE = _CUT_TE(tE)
    xs = np.zeros((N, nx), dtype=dtype)
    xs[:n] = x
    real = np.zeros((N, 1), dtype=dtype)
    real[:n] = 1.0
    q = real * np.asarray(q0, dtype=dtype)
    tq = real * np.asarray(tq0, dtype=dtype)
    h = np.zeros((N, nh), dtype=dtype)
    th = np.zeros((N, nh), dtype=dtype)
    T = len(w["msg"])

    def rows(a, b, ee):
        F = a.shape[-1]
        return np.concatenate([np.broadcast_to(a[:, None, :], (a.shape[0], b.shape[0], F)),
                               np.broadcast_to(b[None, :, :], (a.shape[0], b.shape[0], F)), ee], -1).reshape(a.shape[0] * b.shape[0], -1)

    zx = np.zeros_like(xs)
    for t in range(T):
        a = np.concatenate([xs, h, q], -1)
        ta = np.concatenate([zx, th, tq], -1)
        m, tm = _mlp(rows(a[:n], a, E), rows(ta[:n], ta, tE), w["msg"][t], s)       # every real atom with all N partners
        M, tM = m.reshape(n, N, -1).sum(1), tm.reshape(n, N, -1).sum(1)
        hn, thn = _mlp(np.concatenate([h[:n], M], 1), np.concatenate([th[:n], tM], 1), w["upd"], s)
        h = np.zeros((N, nh), dtype=dtype)
        th = np.zeros((N, nh), dtype=dtype)
        h[:n], th[:n] = hn, thn                                                     # (the node mask keeps padded rows at zero)
    wgt = near.astype(dtype)
    half = np.asarray(0.5, dtype=dtype)
    en, ten = E[:, :n], tE[:, :n]
    for t in range(T):
        a = np.concatenate([xs, h, q], -1)[:n]
        ta = np.concatenate([zx, th, tq], -1)[:n]
        fN, tfN = _mlp(rows(a, a, en), rows(ta, ta, ten), w["pas"][t], s)
        fN, tfN = fN.reshape(n, n), tfN.reshape(n, n)
        # the rows [a_j | a_i | e_ij] are the transposed evaluation (e_ij == e_ji)
        q = q.copy()
        tq = tq.copy()
        q[:n, 0] += (half * (fN - fN.T) * wgt).sum(1)
        tq[:n, 0] += (half * (tfN - tfN.T) * wgt).sum(1)
    return q[:n, 0].astype(np.float64), tq[:n, 0].astype(np.float64)


def edge_tangents(r, a, v=None, strain=None, num=48, cutoff=3.0, eta=2.0):
    """(e, te) (n, n, num) for float64 coordinates r and a float64 cell a taken as they are."""
    e, de, d, D = cell_ref.edges64_at(r, a, num, cutoff, eta)
    tnum = np.zeros_like(D)
    if v is not None:
        v = np.asarray(v, dtype=np.float64)
        tnum = tnum + (d * (v[:, None, :] - v[None, :, :])).sum(-1)
    if strain is not None:
        tnum = tnum + np.einsum("ija,ac,ijc->ij", d, np.asarray(strain, dtype=np.float64), d)
    tD = np.where(D > 0, tnum / np.where(D > 0, D, 1.0), 0.0)
    return e, de * tD[:, :, None]


def jvp64(xyz, x, Q, weights, N=None, v=None, strain=None, dQ=None, box=None, cell=None, h_dim=48, cutoff=3.0, eta=2.0,
          kink_shift=0.0, near_tol=1e-5, dtype=np.float64):
    """(q (n,), tq (n,)) of one molecule padded to N: open, in the box (3,) or in the cell (3, 3); v (n, 3), strain (3, 3), dQ a
    scalar, each or all None (= 0).  dtype: model_jvp's."""
    c = cell_of(box, cell)
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    n = x.shape[0]
    N = n if N is None else N
    r = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    e, te = edge_tangents(r, cell_ref.duals(c)[0], v, strain, h_dim, cutoff, eta)
    q0 = np.float64(np.float32(np.float32(Q) / np.float32(n)))
    tq0 = 0.0 if dQ is None else float(dQ) / n
    return model_jvp(e, te, near_flags(xyz, c, h_dim, cutoff, eta, near_tol), x, q0, tq0, weights, N, kink_shift, dtype)


def forward64_at(r, a, x, Q, near, weights, N, h_dim=48, cutoff=3.0, eta=2.0):
    """(n,) charges for float64 coordinates r, a float64 cell a and a float64 total charge Q taken as they are, with the given near
    flags: what central differences of the forward evaluate."""
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    e = cell_ref.edges64_at(np.asarray(r, dtype=np.float64), a, h_dim, cutoff, eta)[0]
    return model_jvp(e, np.zeros_like(e), near, x, float(Q) / x.shape[0], 0.0, weights, N)[0]


def jvp64_factorised(xyz, x, Q, weights, N=None, v=None, strain=None, dQ=None, box=None, cell=None, h_dim=48, cutoff=3.0, eta=2.0,
                     near_tol=1e-5):
    """jvp64 in the form the kernels of epnn_jvp.hip.h run it (float64): per-atom rows P, R, tP, tR; the all-pairs sweep on
    z1 = max(P_i, -R_j), Yb_j = b2 + W2^T R_j and tz1 = [P_i > -R_j] (tP_i + tR_j); the listed pairs as correction rows (with G minus
    without G) of S and tS; the (N - n) padded partners in closed form; EPN steps over the listed pairs only."""
    from grad_large_ref import pair_list, _split_first
    w = _cast(weights)
    c = cell_of(box, cell)
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    n, nx = x.shape
    N = n if N is None else N
    F = nx + h_dim + 1
    pl = pair_list(xyz, h_dim, cutoff, eta, cell=c, near_tol=near_tol)
    pi, pj, rev, e, d, D = pl["i"], pl["j"], pl["rev"], pl["e"], pl["d"], pl["D"]
    tnum = np.zeros(len(pi))
    if v is not None:
        vv = np.asarray(v, dtype=np.float64)
        tnum = tnum + (d * (vv[pi] - vv[pj])).sum(-1)
    if strain is not None:
        tnum = tnum + np.einsum("ka,ac,kc->k", d, np.asarray(strain, dtype=np.float64), d)
    te = pl["de"] * (tnum / D)[:, None]
    relu = lambda z: np.maximum(z, 0.0)
    scat = lambda idx, rows: (lambda out: (np.add.at(out, idx, rows), out)[1])(np.zeros((n,) + rows.shape[1:]))
    q0 = np.full((n, 1), np.float64(np.float32(np.float32(Q) / np.float32(n))))
    tq0 = np.full((n, 1), 0.0 if dQ is None else float(dQ) / n)
    h, th = np.zeros((n, h_dim)), np.zeros((n, h_dim))
    zx = np.zeros_like(x)
    upd = w["upd"]
    for layers in w["msg"]:
        Wi, Wj, We, b1, W2, b2, W3, b3 = _split_first(layers, F)
        a, ta = np.concatenate([x, h, q0], 1), np.concatenate([zx, th, tq0], 1)
        P, R, tP, tR = a @ Wi + b1, a @ Wj, ta @ Wi, ta @ Wj
        Yb = b2 + R @ W2
        z2pre = np.maximum(P[:, None, :], -R[None, :, :]) @ W2 + Yb[None]
        tz1 = (tP[:, None, :] + tR[None, :, :]) * (P[:, None, :] > -R[None, :, :])
        S = relu(z2pre).sum(1)
        tS = ((tz1 @ W2) * (z2pre > 0)).sum(1)
        zp = relu(P) @ W2 + b2
        S += (N - n) * relu(zp)
        tS += (N - n) * (zp > 0) * ((tP * (P > 0)) @ W2)
        base, tb, G, tG = P[pi] + R[pj], tP[pi] + tR[pj], e @ We, te @ We
        z2g, z2n = relu(base + G) @ W2 + b2, relu(base) @ W2 + b2
        t2g, t2n = ((tb + tG) * (base + G > 0)) @ W2, (tb * (base > 0)) @ W2
        S += scat(pi, relu(z2g) - relu(z2n))
        tS += scat(pi, t2g * (z2g > 0) - t2n * (z2n > 0))
        u, tu = np.concatenate([h, S @ W3 + N * b3], 1), np.concatenate([th, tS @ W3], 1)
        h, th = _mlp(u, tu, upd, 0.0)
    wk = pl["near"].astype(np.float64)
    q, tq = q0, tq0
    for layers in w["pas"]:
        Wi, Wj, We, b1, W2, b2, W3, b3 = _split_first(layers, F)
        a, ta = np.concatenate([x, h, q], 1), np.concatenate([zx, th, tq], 1)
        z1 = (a @ Wi + b1)[pi] + (a @ Wj)[pj] + e @ We
        tz1 = ((ta @ Wi)[pi] + (ta @ Wj)[pj] + te @ We) * (z1 > 0)
        z2 = relu(z1) @ W2 + b2
        f, tf = (relu(z2) @ W3)[:, 0], (((tz1 @ W2) * (z2 > 0)) @ W3)[:, 0]
        q = q + scat(pi, 0.5 * (f - f[rev]) * wk)[:, None]
        tq = tq + scat(pi, 0.5 * (tf - tf[rev]) * wk)[:, None]
    return q[:, 0], tq[:, 0]
