"""Float64 restatement of the pair-list form of the charge gradients (epnn_charges_vjp_xyz[_pbc|_cell], grad_path = 2). Test helper.

tests/xyz_grad_ref.py runs the literal backward on (N, N, .) tensors.  This file is the factorised form of DESIGN.md section 2 run
backwards, on per-atom rows and the list of pairs under the cutoff, a block of rows at a time: memory O(block * n * 32).

* checkpoints: h_t and S_t per GNN step, q_t per EPN step; everything else is recomputed;
* EPN stack: listed pairs only, both orders of the pass MLP, seed +-0.5 w (gq_i - gq_j);
* GNN step t >= 1: update MLP backward -> dS_i = W3 dM_i (the fold of W3), then the all-pairs backward sweep as a ROW pass
  (dP_i = sum_j dz1_ij, tile of i resident, relu(P + R) = max(P, -R) + R, the (N - n) padded partners in closed form) and a
  COLUMN pass (dR_j = sum_i dz1_ij, tile of j resident, relu(P + R) = max(R, -P) + P), near pairs as corrections
  (dz1 with G minus dz1 without it);
* GNN step 0: a_i = [x_i | 0 | Q/n] does not depend on the coordinates: only the listed pairs' dG, no sweep;
* edges to coordinates per listed pair, open / box (minimum image) / cell (image rule of include/epnn.h) displacements, and the
  strain sum beside them.
"""
from __future__ import annotations

import numpy as np


def _image(box=None, cell=None):
    """The displacement rule: float64 (..., 3) r_i - r_j -> its image."""
    if cell is not None:
        import cell_ref
        a, gd = cell_ref.duals(cell)
        return lambda d: cell_ref.mic64(d, a, gd)
    if box is not None:
        import periodic_ref
        return lambda d: periodic_ref.mic(d, box)
    return lambda d: d


def pair_list(xyz, num, cutoff=3.0, eta=2.0, box=None, cell=None, block=256, near_tol=1e-5):
    """Every ORDERED pair (i, j), j != i, with D < cutoff, sorted by (i, j): dict of i, j, rev (index of (j, i)), e and de/dD
    (float64, num channels), d = image of r_i - r_j, D, near (the float32 decision of charge_gn.py:90-94)."""
    r = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    n = r.shape[0]
    img = _image(box, cell)
    mu = np.linspace(0.1, cutoff, num=num)
    I, J, DV = [], [], []
    for i0 in range(0, n, block):
        i1 = min(n, i0 + block)
        d = img(r[i0:i1, None, :] - r[None, :, :])
        D = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
        ii, jj = np.nonzero(D < cutoff)
        keep = jj != ii + i0
        ii, jj = ii[keep], jj[keep]
        I.append(ii + i0)
        J.append(jj)
        DV.append(d[ii, jj])
    I, J, d = np.concatenate(I), np.concatenate(J), np.concatenate(DV)
    D = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    key = I.astype(np.int64) * n + J
    rev = np.searchsorted(key, J.astype(np.int64) * n + I)
    assert np.array_equal(key[rev], J.astype(np.int64) * n + I), "the pair list is not symmetric"
    C = (np.cos(np.pi * D / cutoff) + 1.0) / 2.0
    dC = -0.5 * (np.pi / cutoff) * np.sin(np.pi * D / cutoff)
    C[D <= 0.0] = 1.0
    dC[D <= 0.0] = 0.0
    u = D[:, None] - mu[None, :]
    ex = np.exp(-eta * u * u)
    e = C[:, None] * ex
    de = (dC[:, None] - 2.0 * eta * u * C[:, None]) * ex
    near = e.astype(np.float32).max(-1) > np.float32(near_tol)
    return {"i": I, "j": J, "rev": rev, "e": e, "de": de, "d": d, "D": D, "near": near, "n": n}


def _relu(z):
    return np.maximum(z, 0.0)


def _scatter(idx, rows, n):
    out = np.zeros((n,) + rows.shape[1:])
    np.add.at(out, idx, rows)
    return out


def _split_first(layers, F):
    (W1, b1), (W2, b2), (W3, b3) = layers
    return W1[:F], W1[F:2 * F], W1[2 * F:], b1, W2, b2, W3, b3


def _cast(weights):
    c = lambda m: [(np.asarray(W, np.float64), np.asarray(b, np.float64)) for W, b in m]
    return {"msg": [c(m) for m in weights["msg"]], "upd": c(weights["upd"]), "pas": [c(m) for m in weights["pas"]]}


def _sweep_forward(P, R, W2, b2, pl, G, N, block):
    """S_i = sum over all N partners of relu(W2^T relu(P_i + R_j + G_ij) + b2): rows a block at a time, the forward's
    max(P, -R) + R form, listed pairs as corrections, the padded partners (R = 0, G = 0) in closed form."""
    n = P.shape[0]
    Yb = b2 + R @ W2
    S = np.empty_like(P)
    for i0 in range(0, n, block):
        i1 = min(n, i0 + block)
        z2 = _relu(np.maximum(P[i0:i1, None, :], -R[None, :, :]) @ W2 + Yb[None])
        S[i0:i1] = z2.sum(1)
    S += (N - n) * _relu(_relu(P) @ W2 + b2)
    i, j = pl["i"], pl["j"]
    with_g = _relu(_relu(P[i] + R[j] + G) @ W2 + b2)
    without = _relu(_relu(P[i] + R[j]) @ W2 + b2)
    return S + _scatter(i, with_g - without, n)


def _dz1(z1pre, dS, W2, b2, s):
    d2 = dS * ((_relu(z1pre) @ W2 + b2) > s)
    return (d2 @ W2.T) * (z1pre > s)


def _sweep_backward(P, R, dS, W2, b2, pl, G, N, s, block):
    """(dP, dR, dz1 of the listed pairs) of one GNN step t >= 1: row pass and column pass, each on its own form of
    relu(P + R), near pairs as corrections."""
    n = P.shape[0]
    dP = np.empty_like(P)
    dR = np.empty_like(P)
    Yb = b2 + R @ W2                                   # row pass: z2pre = W2^T max(P_i, -R_j) + Yb_j
    for i0 in range(0, n, block):
        i1 = min(n, i0 + block)
        z2pre = np.maximum(P[i0:i1, None, :], -R[None, :, :]) @ W2 + Yb[None]
        d2 = dS[i0:i1, None, :] * (z2pre > s)
        dz1 = (d2 @ W2.T) * ((P[i0:i1, None, :] + R[None, :, :]) > s)
        dP[i0:i1] = dz1.sum(1)
    dP += (N - n) * _dz1(P, dS, W2, b2, s)            # padded partners: R = 0, G = 0, (N - n) times
    Yc = b2 + P @ W2                                   # column pass: z2pre = W2^T max(R_j, -P_i) + Yc_i
    for j0 in range(0, n, block):
        j1 = min(n, j0 + block)
        z2pre = np.maximum(R[None, j0:j1, :], -P[:, None, :]) @ W2 + Yc[:, None, :]
        d2 = dS[:, None, :] * (z2pre > s)
        dz1 = (d2 @ W2.T) * ((P[:, None, :] + R[None, j0:j1, :]) > s)
        dR[j0:j1] = dz1.sum(0)
    i, j = pl["i"], pl["j"]
    with_g = _dz1(P[i] + R[j] + G, dS[i], W2, b2, s)
    corr = with_g - _dz1(P[i] + R[j], dS[i], W2, b2, s)
    return dP + _scatter(i, corr, n), dR + _scatter(j, corr, n), with_g


def vjp64_large(xyz, x, Q, g, weights, N=None, box=None, cell=None, strain=False, h_dim=48, cutoff=3.0, eta=2.0,
                kink_shift=0.0, block=64, near_tol=1e-5):
    """(q (n,), gxyz (n, 3)[, gstrain (3, 3)]) of one molecule padded to N: open, in the box (3,) or in the cell (3, 3)."""
    w = _cast(weights)
    s = float(kink_shift)
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    n, nx = x.shape
    N = n if N is None else N
    nh = h_dim
    F = nx + nh + 1
    pl = pair_list(xyz, h_dim, cutoff, eta, box, cell, near_tol=near_tol)
    pi, pj, rev, e = pl["i"], pl["j"], pl["rev"], pl["e"]
    q0 = np.full((n, 1), np.float64(np.float32(np.float32(Q) / np.float32(n))))
    T = len(w["msg"])
    upd = w["upd"]

    def upd_forward(h, S, W3, b3):
        acts, pres = [np.concatenate([h, S @ W3 + N * b3], 1)], [None]
        for W, b in upd[:-1]:
            pres.append(acts[-1] @ W + b)
            acts.append(_relu(pres[-1]))
        return acts[-1] @ upd[-1][0] + upd[-1][1], acts, pres

    # ------------------------------------------------------------------ forward with checkpoints
    h = np.zeros((n, nh))
    hs, Ss = [], []
    for t in range(T):
        Wi, Wj, We, b1, W2, b2, W3, b3 = _split_first(w["msg"][t], F)
        a = np.concatenate([x, h, q0], 1)
        S = _sweep_forward(a @ Wi + b1, a @ Wj, W2, b2, pl, e @ We, N, block)
        hs.append(h)
        Ss.append(S)
        h = upd_forward(h, S, W3, b3)[0]
    feats = h
    wk = pl["near"].astype(np.float64)
    q = q0
    qs = []

    def pass_rows(t, qt):
        Wi, Wj, We, b1, W2, b2, W3, b3 = _split_first(w["pas"][t], F)
        a = np.concatenate([x, feats, qt], 1)
        z1pre = (a @ Wi + b1)[pi] + (a @ Wj)[pj] + e @ We
        z2pre = _relu(z1pre) @ W2 + b2
        return z1pre, z2pre, (_relu(z2pre) @ W3 + b3)[:, 0]

    for t in range(T):
        qs.append(q)
        f = pass_rows(t, q)[2]
        q = q + _scatter(pi, 0.5 * (f - f[rev]) * wk, n)[:, None]
    pred = q[:, 0]

    # ------------------------------------------------------------------ backward: EPN stack
    gq = np.asarray(g, dtype=np.float64).copy()
    gfeat = np.zeros((n, nh))
    gE = np.zeros_like(e)
    for t in range(T - 1, -1, -1):
        Wi, Wj, We, b1, W2, b2, W3, b3 = _split_first(w["pas"][t], F)
        z1pre, z2pre, _ = pass_rows(t, qs[t])
        seed = 0.5 * (wk * gq[pi] - wk[rev] * gq[pj])                       # row [a_i | a_j | e_ij]: listed and swapped use
        d2 = (seed[:, None] * W3[:, 0][None, :]) * (z2pre > s)
        dz1 = (d2 @ W2.T) * (z1pre > s)
        ga = _scatter(pi, dz1, n) @ Wi.T + _scatter(pj, dz1, n) @ Wj.T
        gE += dz1 @ We.T
        gfeat += ga[:, nx:nx + nh]
        gq = gq + ga[:, nx + nh]
    # ------------------------------------------------------------------ backward: GNN steps
    gh = gfeat
    for t in range(T - 1, -1, -1):
        Wi, Wj, We, b1, W2, b2, W3, b3 = _split_first(w["msg"][t], F)
        _, acts, pres = upd_forward(hs[t], Ss[t], W3, b3)
        d = gh @ upd[-1][0].T
        for l in range(len(upd) - 2, -1, -1):
            d = (d * (pres[l + 1] > s)) @ upd[l][0].T
        dS = d[:, nh:] @ W3.T
        a = np.concatenate([x, hs[t], q0], 1)
        P, R, G = a @ Wi + b1, a @ Wj, e @ We
        if t == 0:                                                          # h_0 = 0 and q0 are constants: only dG is needed
            gE += _dz1(P[pi] + R[pj] + G, dS[pi], W2, b2, s) @ We.T
            break
        dP, dR, dG = _sweep_backward(P, R, dS, W2, b2, pl, G, N, s, block)
        gE += dG @ We.T
        gh = d[:, :nh] + (dP @ Wi.T + dR @ Wj.T)[:, nx:nx + nh]
    # ------------------------------------------------------------------ edge features -> coordinates
    gD = (gE * pl["de"]).sum(-1)
    Gk = (gD + gD[rev]) / pl["D"]
    gxyz = _scatter(pi, Gk[:, None] * pl["d"], n)
    if not strain:
        return pred, gxyz
    dd = pl["d"]
    gstrain = 0.5 * np.einsum("k,ka,kc->ac", Gk, dd, dd)
    return pred, gxyz, gstrain
