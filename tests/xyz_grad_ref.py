"""Float64 reference for the charge gradients with respect to the coordinates (epnn_charges_vjp_xyz). Test helper.

One molecule padded to N, as epnn_forward_xyz sees it (oracle.epnn_oracle.dense_inputs / model_reduce): per-atom x, h = 0,
q = Q / n, mask 1 on real pairs.  The forward is the oracle's (oracle/epnn_oracle_train.py) with float64 edge features; the
`near` decisions come from the float32 edge tensor, as in the oracle.  The backward is the oracle's training backward seeded
with a cotangent g of the charges instead of the loss gradient, extended by the gradient with respect to the edge features
(the last e_dim columns of every first Dense's input rows) and the backward of get_init_edges (charge_gn.py:122-163).
The masks (near, node mask) are constants.  ReLU kinks are bracketed like loss_and_grads(kink_shift=...).
"""
from __future__ import annotations

import numpy as np

from oracle import epnn_oracle as orc
from oracle import epnn_oracle_train as otr


def edges64(xyz, num, cutoff=3.0, eta=2.0):
    """get_init_edges in float64 (no float32 cast) and its derivative with respect to D: (e, de/dD, r_i - r_j, D)."""
    r = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    mu = np.linspace(0.1, cutoff, num=num)
    d = r[:, None, :] - r[None, :, :]
    D = np.sqrt((d * d).sum(-1))
    C = (np.cos(np.pi * D / cutoff) + 1.0) / 2.0
    dC = -0.5 * (np.pi / cutoff) * np.sin(np.pi * D / cutoff)
    far = D >= cutoff
    C[far] = 0.0
    dC[far] = 0.0
    C[D <= 0.0] = 1.0
    dC[D <= 0.0] = 0.0
    np.fill_diagonal(C, 0.0)
    np.fill_diagonal(dC, 0.0)
    u = D[:, :, None] - mu[None, None, :]
    ex = np.exp(-eta * u * u)
    e = C[:, :, None] * ex
    de = (dC[:, :, None] - 2.0 * eta * u * C[:, :, None]) * ex
    return e, de, d, D


def _inputs(xyz, x, Q, N, h_dim, cutoff, eta, near_tol=1e-5):
    n = x.shape[0]
    e32, _ = orc.get_init_edges(xyz, num=h_dim, cutoff=cutoff, eta=eta)
    e64, de, d, D = edges64(xyz, h_dim, cutoff, eta)
    E = np.zeros((1, N, N, h_dim))
    E[0, :n, :n] = e64
    tol = np.float32(near_tol)
    near32 = np.zeros((N, N), dtype=bool)
    near32[:n, :n] = np.clip(e32, tol, np.float32(1e5)).max(-1) != tol
    xs = np.zeros((1, N, x.shape[1]))
    xs[0, :n] = np.asarray(x, dtype=np.float32)
    q0 = np.zeros((1, N, 1))
    q0[0, :n, 0] = np.float32(np.float32(Q) / np.float32(n))
    mask = np.zeros((1, N, N))
    mask[0, :n, :n] = 1.0
    return E, de, d, D, near32, xs, q0, mask


def forward64(xyz, x, Q, weights, N=None, h_dim=48, cutoff=3.0, eta=2.0, near_tol=1e-5):
    """(N,) charges from the float64 forward with float64 edges."""
    return vjp64(xyz, x, Q, np.zeros(x.shape[0]), weights, N, h_dim, cutoff, eta, near_tol=near_tol)[0]


_CUT_GE = None        # tests/grad_noise_ref.py: a function applied to the edge cotangent gE before its contraction (a defect model)


def vjp64(xyz, x, Q, g, weights, N=None, h_dim=48, cutoff=3.0, eta=2.0, kink_shift=0.0, kink_where="all", near_tol=1e-5,
          dtype=np.float64):
    """(q (N,), gxyz (n, 3) = sum_i g[i] dq_i/dxyz) for one molecule padded to N.  dtype=np.float32: the float32 model of the
    device's derivative kernels -- weights, the edge tensor as the MLPs see it, activations, tapes, gE and every Dense product and
    sweep sum in float32; the geometry (image, D, de/dD, the contraction of gE with de/dD and the displacement) stays in float64
    and the result is rounded to float32, where the device stores it.  near flags and masks are the same for both."""
    otr._KINK_SHIFT, otr._KINK_WHERE = float(kink_shift), kink_where
    try:
        return _vjp64(xyz, x, Q, g, weights, N, h_dim, cutoff, eta, near_tol, dtype)
    finally:
        otr._KINK_SHIFT, otr._KINK_WHERE = 0.0, "all"


def _vjp64(xyz, x_at, Q, g, weights, N, h_dim, cutoff, eta, near_tol=1e-5, dtype=np.float64):
    n = x_at.shape[0]
    N = n if N is None else N
    w = otr._cast(weights, dtype)
    e, de, dvec, Dm, near32, x, q0, mask = _inputs(xyz, x_at, Q, N, h_dim, cutoff, eta, near_tol)
    f64 = np.dtype(dtype) == np.float64
    if not f64:
        e, x, q0, mask = (t.astype(dtype) for t in (e, x, q0, mask))
    B = 1
    nm = np.clip(mask.sum(axis=1), 0, 1)[..., None]                         # (1,N,1)
    h0 = np.zeros((1, N, h_dim), dtype=dtype)
    T = len(w["msg"])
    tape_g = []
    h = h0
    for t in range(T):
        a = np.concatenate([x, h, q0], -1)
        F = a.shape[-1]
        X = np.concatenate([np.broadcast_to(a[:, :, None, :], (B, N, N, F)),
                            np.broadcast_to(a[:, None, :, :], (B, N, N, F)), e], -1).reshape(B * N * N, -1)
        m, acts = otr._mlp_fwd(X, w["msg"][t])
        M = m.reshape(B, N, N, -1).sum(2)
        U0 = np.concatenate([h, M], 2) * nm
        hn, uacts = otr._mlp_fwd(U0.reshape(B * N, -1), w["upd"])
        tape_g.append((acts, uacts, F))
        h = hn.reshape(B, N, -1) * nm
    feats = h
    wgt = mask * near32[None].astype(dtype)
    q = q0
    tape_e = []
    for t in range(T):
        a = np.concatenate([x, feats, q], -1)
        F = a.shape[-1]
        ai = np.broadcast_to(a[:, :, None, :], (B, N, N, F))
        aj = np.broadcast_to(a[:, None, :, :], (B, N, N, F))
        fN, actsN = otr._mlp_fwd(np.concatenate([ai, aj, e], -1).reshape(B * N * N, -1), w["pas"][t])
        fT, actsT = otr._mlp_fwd(np.concatenate([aj, ai, e], -1).reshape(B * N * N, -1), w["pas"][t])
        anti = np.asarray(0.5, dtype=dtype) * (fN.reshape(B, N, N) - fT.reshape(B, N, N)) * wgt
        q = q + anti.sum(2)[..., None]
        tape_e.append((actsN, actsT, F))
    pred = q[0, :, 0]

    # ------------------------------------------------------------------ backward, seeded with g
    gq = np.zeros((B, N, 1), dtype=dtype)
    gq[0, :n, 0] = g
    gE = np.zeros((B, N, N, h_dim), dtype=dtype)
    half = np.asarray(0.5, dtype=dtype)
    gfeat = np.zeros_like(feats)
    nh = feats.shape[-1]
    nx = x.shape[-1]
    for t in range(T - 1, -1, -1):
        actsN, actsT, F = tape_e[t]
        ganti = np.broadcast_to(gq, (B, N, N)) * wgt
        dXN, _ = otr._mlp_bwd((half * ganti).reshape(-1, 1), actsN, w["pas"][t], "listed")
        dXT, _ = otr._mlp_bwd((-half * ganti).reshape(-1, 1), actsT, w["pas"][t], "swapped")
        dXN = dXN.reshape(B, N, N, -1)
        dXT = dXT.reshape(B, N, N, -1)
        ga = dXN[..., :F].sum(2) + dXN[..., F:2 * F].sum(1) + dXT[..., :F].sum(1) + dXT[..., F:2 * F].sum(2)
        gE += dXN[..., 2 * F:] + dXT[..., 2 * F:]
        gfeat = gfeat + ga[..., nx:nx + nh]
        gq = gq + ga[..., nx + nh:nx + nh + 1]
    gh = gfeat
    for t in range(T - 1, -1, -1):
        acts, uacts, F = tape_g[t]
        dhn = (gh * nm).reshape(B * N, -1)
        dU0, _ = otr._mlp_bwd(dhn, uacts, w["upd"])
        dU0 = dU0.reshape(B, N, -1) * nm
        gh_prev = dU0[..., :nh]
        gM = dU0[..., nh:]
        dm = np.broadcast_to(gM[:, :, None, :], (B, N, N, gM.shape[-1])).reshape(B * N * N, -1)
        dX, _ = otr._mlp_bwd(dm, acts, w["msg"][t])
        dX = dX.reshape(B, N, N, -1)
        ga = dX[..., :F].sum(2) + dX[..., F:2 * F].sum(1)
        gE += dX[..., 2 * F:]
        gh = gh_prev + ga[..., nx:nx + nh]
    # ------------------------------------------------------------------ edge features -> coordinates
    if _CUT_GE is not None:
        gE = _CUT_GE(gE)
    gD = (gE[0, :n, :n].astype(np.float64) * de).sum(-1)                    # (n,n), float64 geometry whatever dtype is
    G = gD + gD.T
    with np.errstate(divide="ignore", invalid="ignore"):
        Wm = np.where(Dm > 0, G / np.where(Dm > 0, Dm, 1.0), 0.0)
    gxyz = (Wm[:, :, None] * dvec).sum(1)                                   # sum_j G_ij (r_i - r_j) / D_ij
    if not f64:                                                             # (columns past the third: cell_ref's strain terms, summed first)
        pred = pred.astype(np.float64)
        gxyz[:, :3] = gxyz[:, :3].astype(np.float32)
    return pred, gxyz
