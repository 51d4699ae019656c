"""Float64 restatement of the pair-list training step (epnn_train_step_xyz_cell, train_path = 2). Test helper.

tests/grad_large_ref.py runs the factorised form of DESIGN.md section 2 backwards for the gradient with respect to the coordinates.
This file runs the same algebra for the gradient of loss = sum (y - q)^2 with respect to every weight, on per-atom rows and the list
of pairs under the cutoff, a block of rows at a time: memory O(block * n * 32).

* seed gq = 2 (q - y); checkpoints and the EPN / GNN backward as in grad_large_ref;
* per atom: the update MLP (all T steps add: it is shared), W3 and N b3 of a message MLP, the Wi / Wj blocks of a first Dense as
  a_i (x) dP_i and a_j (x) dR_j, b1 = sum dP_i, and the (N - n) padded partners' share of W2 / b2 in closed form;
* per listed pair: the We block as e_ij (x) dz1_ij, the near-pair corrections' share of W2 / b2 (with G minus without), and W2, b2, W3,
  b3 of the pass MLPs for both orders of a pair;
* all pairs: dW2 = sum_ij z1_ij (x) d2_ij and db2 = sum_ij d2_ij of every message MLP, z1 = relu(P_i + R_j) without G, in the row pass;
* step 0 runs like every other step: a_i of step 0 is constant with respect to the coordinates, not to the weights.

Returns the oracle's structures (oracle/epnn_oracle_train.py: loss, predictions, {"msg", "upd", "pas"} of (dW, db) lists), so the
two can be compared entry by entry (tests/test_train_large_ref.py)."""
from __future__ import annotations

import numpy as np

from grad_large_ref import _cast, _relu, _scatter, _split_first, _sweep_forward, pair_list


def _zero_like(w):
    z = lambda m: [[np.zeros_like(W), np.zeros_like(b)] for W, b in m]
    return {"msg": [z(m) for m in w["msg"]], "upd": z(w["upd"]), "pas": [z(m) for m in w["pas"]]}


def _sweep_backward_w(P, R, dS, W2, b2, pl, G, N, s, block):
    """(dP, dR, dz1 of the listed pairs, dW2, db2) of one GNN step: the row pass also adds up z1 (x) d2 over all pairs, the column
    pass gives dR; listed pairs as corrections (with G minus without), the (N - n) padded partners in closed form."""
    n = P.shape[0]
    dP = np.empty_like(P)
    dR = np.zeros_like(P)
    dW2 = np.zeros_like(W2)
    db2 = np.zeros_like(b2)
    for i0 in range(0, n, block):
        i1 = min(n, i0 + block)
        z1pre = P[i0:i1, None, :] + R[None, :, :]
        z1 = _relu(z1pre)
        d2 = dS[i0:i1, None, :] * ((z1 @ W2 + b2) > s)
        dz1 = (d2 @ W2.T) * (z1pre > s)
        dP[i0:i1] = dz1.sum(1)
        dR += dz1.sum(0)
        dW2 += np.einsum("ijk,ijm->km", z1, d2)
        db2 += d2.sum((0, 1))
    zp = _relu(P)                                                          # padded partners: R = 0, G = 0, (N - n) times
    d2p = dS * ((zp @ W2 + b2) > s)
    dP += (N - n) * ((d2p @ W2.T) * (P > s))
    dW2 += (N - n) * (zp.T @ d2p)
    db2 += (N - n) * d2p.sum(0)
    i, j = pl["i"], pl["j"]

    def rows(z1pre):
        z1 = _relu(z1pre)
        d2 = dS[i] * ((z1 @ W2 + b2) > s)
        return z1, d2, (d2 @ W2.T) * (z1pre > s)

    z1g, d2g, dzg = rows(P[i] + R[j] + G)
    z1n, d2n, dzn = rows(P[i] + R[j])
    dW2 += z1g.T @ d2g - z1n.T @ d2n
    db2 += d2g.sum(0) - d2n.sum(0)
    corr = dzg - dzn
    return dP + _scatter(i, corr, n), dR + _scatter(j, corr, n), dzg, dW2, db2


def loss_and_grads_large(xyz, x, Q, y, weights, N=None, box=None, cell=None, h_dim=48, cutoff=3.0, eta=2.0, kink_shift=0.0, block=64,
                         near_tol=1e-5):
    """(loss, q (n,), grads) of one molecule padded to N: open, in the box (3,) or in the cell (3, 3)."""
    w = _cast(weights)
    s = float(kink_shift)
    x = np.asarray(x, dtype=np.float32).astype(np.float64)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    n, nx = x.shape
    N = n if N is None else N
    nh = h_dim
    F = nx + nh + 1
    pl = pair_list(xyz, h_dim, cutoff, eta, box, cell, near_tol=near_tol)
    pi, pj, rev = pl["i"], pl["j"], pl["rev"]
    # the edge features are an INPUT of the model, float32 (get_init_edges and the library's front-end round them): the same
    # expression as cell_ref._edge_rows_cell, rounded, so that this file and the dense oracle differentiate the same function
    mu = np.linspace(0.1, cutoff, num=h_dim)
    C = (np.cos(np.pi * (pl["D"] - 0.0) / cutoff) + 1.0) / 2.0
    C[pl["D"] <= 0.0] = 1.0
    e = (C[:, None] * np.exp(-eta * (pl["D"][:, None] - mu[None, :]) ** 2)).astype(np.float32).astype(np.float64)
    q0 = np.full((n, 1), np.float64(np.float32(np.float32(Q) / np.float32(n))))
    T = len(w["msg"])
    upd = w["upd"]
    g = _zero_like(w)

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
        return a, z1pre, z2pre, (_relu(z2pre) @ W3 + b3)[:, 0]

    for t in range(T):
        qs.append(q)
        f = pass_rows(t, q)[3]
        q = q + _scatter(pi, 0.5 * (f - f[rev]) * wk, n)[:, None]
    pred = q[:, 0]
    loss = float(((y - pred) ** 2).sum())

    # ------------------------------------------------------------------ backward: EPN stack
    gq = 2.0 * (pred - y)
    gfeat = np.zeros((n, nh))
    for t in range(T - 1, -1, -1):
        Wi, Wj, We, b1, W2, b2, W3, b3 = _split_first(w["pas"][t], F)
        a, z1pre, z2pre = pass_rows(t, qs[t])[:3]
        seed = 0.5 * (wk * gq[pi] - wk[rev] * gq[pj])                       # row [a_i | a_j | e_ij]: listed and swapped use
        z2 = _relu(z2pre)
        d2 = (seed[:, None] * W3[:, 0][None, :]) * (z2pre > s)
        z1 = _relu(z1pre)
        dz1 = (d2 @ W2.T) * (z1pre > s)
        dPa, dRa = _scatter(pi, dz1, n), _scatter(pj, dz1, n)
        G0, G1, G2 = g["pas"][t]
        G2[0] += (z2 * seed[:, None]).sum(0)[:, None]
        G2[1] += np.array([(seed + seed[rev]).sum() / 2])                   # a pair's two orders cancel term by term: exactly 0
        G1[0] += z1.T @ d2
        G1[1] += d2.sum(0)
        G0[0][:F] += a.T @ dPa
        G0[0][F:2 * F] += a.T @ dRa
        G0[0][2 * F:] += e.T @ dz1
        G0[1] += dPa.sum(0)
        ga = dPa @ Wi.T + dRa @ Wj.T
        gfeat += ga[:, nx:nx + nh]
        gq = gq + ga[:, nx + nh]
    # ------------------------------------------------------------------ backward: GNN steps
    gh = gfeat
    for t in range(T - 1, -1, -1):
        Wi, Wj, We, b1, W2, b2, W3, b3 = _split_first(w["msg"][t], F)
        _, acts, pres = upd_forward(hs[t], Ss[t], W3, b3)
        g["upd"][-1][0] += acts[-1].T @ gh
        g["upd"][-1][1] += gh.sum(0)
        d = gh @ upd[-1][0].T
        for l in range(len(upd) - 2, -1, -1):
            d = d * (pres[l + 1] > s)
            g["upd"][l][0] += acts[l].T @ d
            g["upd"][l][1] += d.sum(0)
            d = d @ upd[l][0].T
        dM = d[:, nh:]
        G0, G1, G2 = g["msg"][t]
        G2[0] += Ss[t].T @ dM
        G2[1] += N * dM.sum(0)
        dS = dM @ W3.T
        a = np.concatenate([x, hs[t], q0], 1)
        P, R, G = a @ Wi + b1, a @ Wj, e @ We
        dP, dR, dG, dW2, db2 = _sweep_backward_w(P, R, dS, W2, b2, pl, G, N, s, block)
        G1[0] += dW2
        G1[1] += db2
        G0[0][:F] += a.T @ dP
        G0[0][F:2 * F] += a.T @ dR
        G0[0][2 * F:] += e.T @ dG
        G0[1] += dP.sum(0)
        gh = d[:, :nh] + (dP @ Wi.T + dR @ Wj.T)[:, nx:nx + nh]
    grads = {k: ([[(W, b) for W, b in m] for m in g[k]] if k != "upd" else [(W, b) for W, b in g[k]]) for k in g}
    return loss, pred, grads


def batch_loss_and_grads_large(offsets, xyz, x, Q, y, weights, N, cells=None, **kw):
    """The same for a flat batch (cells: one (3, 3) cell or None per molecule): losses and gradients add, q (A,)."""
    from oracle import epnn_oracle_train as ot
    total, qs, acc = 0.0, [], None
    for b in range(len(offsets) - 1):
        a0, a1 = int(offsets[b]), int(offsets[b + 1])
        loss, q, g = loss_and_grads_large(xyz[a0:a1], x[a0:a1], Q[b], y[a0:a1], weights, N=N, cell=None if cells is None else cells[b], **kw)
        total += loss
        qs.append(q)
        flat = ot.flatten(g)
        acc = flat if acc is None else acc + flat
    return total, np.concatenate(qs), acc
