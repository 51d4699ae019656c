"""Float64 reference for periodic cells (epnn_forward_xyz_pbc, epnn_charges_vjp_xyz_pbc, epnn_edges_pbc). Test helper.

The reference has no periodic boundaries.  Its model sees the geometry only through the pair distances of get_init_edges
(charge_gn.py:122-163), so the periodic model is the oracle's own layer functions (orc.model_forward / gnn_layer / epn_layer)
run on minimum-image edges: per axis d = x_j - x_i in float64, on a periodic axis (L > 0) d - L rint(d / L), then the
oracle's edge formula and its float32 cast.  For cells too large for dense tensors EdgeRowsPBC produces the edge rows a
block at a time, as the oracle's EdgeRows does.  vjp64_pbc is tests/xyz_grad_ref.py with its edges replaced by
minimum-image ones (that file is used as it is).
"""
from __future__ import annotations

import contextlib

import numpy as np

from oracle import epnn_oracle as orc
import xyz_grad_ref as xgr


def box_rows(box, B):
    box = np.asarray(box, dtype=np.float32)
    return np.tile(box, (B, 1)) if box.shape == (3,) else box.reshape(B, 3)


def mic(d, L):
    """Minimum image of float64 displacements d (..., 3) in the cell L (3,) (float32 lengths; 0 = open axis)."""
    L = np.asarray(L, dtype=np.float32).astype(np.float64)
    out = np.array(d, dtype=np.float64, copy=True)
    for k in range(3):
        if L[k] > 0:
            out[..., k] = out[..., k] - L[k] * np.rint(out[..., k] / L[k])
    return out


def _edge_rows_pbc(xyz64, box, i0, i1, num, cutoff, eta):
    """orc._edge_rows with minimum-image distances (d = x_j - x_i, the device's order; D does not depend on the sign)."""
    mu = np.linspace(0.1, cutoff, num=num)
    d = mic(xyz64[None, :, :] - xyz64[i0:i1, None, :], box)
    D = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    C = (np.cos(np.pi * (D - 0.0) / cutoff) + 1.0) / 2.0
    C[D >= cutoff] = 0.0
    C[D <= 0.0] = 1.0
    idx = np.arange(i0, i1)
    C[idx - i0, idx] = 0.0
    e = (C[:, :, None] * np.exp(-eta * (D[:, :, None] - mu[None, None, :]) ** 2)).astype(np.float32)
    return e, C


def get_init_edges_pbc(xyz, box, num=48, cutoff=3.0, eta=2.0):
    """(e float32 (n,n,num), C float64 (n,n)) of one system in the cell box (3,)."""
    xyz64 = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    return _edge_rows_pbc(xyz64, box, 0, xyz64.shape[0], num, cutoff, eta)


class EdgeRowsPBC(orc.EdgeRows):
    """orc.EdgeRows with minimum-image edges."""

    def __init__(self, xyz, box, num=48, cutoff=3.0, eta=2.0):
        super().__init__(xyz, num, cutoff, eta)
        self.box = np.asarray(box, dtype=np.float32)

    def rows(self, i0, i1):
        key = (i0, min(i1, self.shape[1]))
        if key not in self._blocks:
            self._blocks[key] = _edge_rows_pbc(self.xyz, self.box, key[0], key[1], self.num, self.cutoff, self.eta)[0][None]
        return self._blocks[key]


def forward_pbc(xyz, x, Q, box, weights, N=None, dtype=np.float64, h_dim=48, cutoff=3.0, eta=2.0, near_tol=1e-5):
    """One molecule padded to N in the cell box (3,): orc.dense_inputs with periodic edges, orc.model_forward.  (N,) charges."""
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[0]
    N = n if N is None else N
    h_p, e_p, x_p, q_p, mask = orc.dense_inputs(xyz, x, Q, N, h_dim=h_dim, e_dim=h_dim, cutoff=cutoff, eta=eta)
    e, _ = get_init_edges_pbc(xyz, box, num=h_dim, cutoff=cutoff, eta=eta)
    e_p[:n, :n] = e
    return orc.model_forward(h_p[None], e_p[None], x_p[None], q_p[None], mask[None], weights, dtype, near_tol=near_tol)[0, :, 0]


def forward_large_pbc(xyz, x, Q, box, weights, dtype=np.float64, cutoff=3.0, eta=2.0, near_tol=1e-5):
    """orc.forward_xyz_large in the cell box (3,): one unpadded system, edge rows a block at a time."""
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[0]
    h = np.zeros((1, n, 48), dtype=dtype)
    q = np.full((1, n, 1), np.float32(np.float32(Q) / np.float32(n)), dtype=dtype)
    mask = np.ones((1, n, 1, 1), dtype=dtype)
    e = EdgeRowsPBC(xyz, box, 48, cutoff, eta)
    xx = x[None].astype(dtype)
    feats = orc.gnn_layer(h, e, xx, q, mask, weights["msg"], weights["upd"], dtype)
    return orc.epn_layer(feats, e, xx, q, mask, weights["pas"], dtype, near_tol=near_tol)[0, :, 0]


def forward_batch_pbc(offsets, xyz, x, Q, box, weights, N, dtype=np.float64, **kw):
    """A flat batch, molecule by molecule: (A,) charges."""
    rows = box_rows(box, len(offsets) - 1)
    out = []
    for b in range(len(offsets) - 1):
        a0, a1 = int(offsets[b]), int(offsets[b + 1])
        out.append(forward_pbc(xyz[a0:a1], x[a0:a1], Q[b], rows[b], weights, N, dtype, **kw)[:a1 - a0])
    return np.concatenate(out)


def pairs_pbc(xyz, box, cutoff=3.0, eta=2.0, tol=1e-5, num=48, block=64):
    """The pair list epnn_debug_pairs reports for one system: (i, j, near) for every i < j with D < cutoff (float64 test on the
    minimum-image displacement), near = max_k e_k > tol in float32 (charge_gn.py:90-94).  Exact, a block of rows at a time."""
    r = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    n = r.shape[0]
    I, J, W = [], [], []
    mu = np.linspace(0.1, cutoff, num=num)
    for i0 in range(0, n, block):
        i1 = min(n, i0 + block)
        d = mic(r[None, :, :] - r[i0:i1, None, :], box)
        D2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        D = np.sqrt(D2)
        ii, jj = np.nonzero(D < cutoff)
        ii = ii + i0
        keep = jj > ii
        ii, jj = ii[keep], jj[keep]
        Dp = D[ii - i0, jj]
        C = (np.cos(np.pi * Dp / cutoff) + 1.0) / 2.0
        C[Dp <= 0.0] = 1.0
        e = (C[:, None] * np.exp(-eta * (Dp[:, None] - mu[None, :]) ** 2)).astype(np.float32)
        I.append(ii)
        J.append(jj)
        W.append(e.max(-1) > np.float32(tol))
    I, J, W = np.concatenate(I), np.concatenate(J), np.concatenate(W)
    o = np.lexsort((J, I))
    return I[o], J[o], W[o]


def _edges64_pbc(box):
    def edges64(xyz, num, cutoff=3.0, eta=2.0):
        """xgr.edges64 on minimum-image displacements: (e, de/dD, r_i - r_j, D)."""
        r = np.asarray(xyz, dtype=np.float32).astype(np.float64)
        mu = np.linspace(0.1, cutoff, num=num)
        d = mic(r[:, None, :] - r[None, :, :], box)
        D = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
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
        return C[:, :, None] * ex, (dC[:, :, None] - 2.0 * eta * u * C[:, :, None]) * ex, d, D
    return edges64


class _OrcPBC:
    """orc with get_init_edges replaced by its minimum-image form (what xgr._inputs calls)."""

    def __init__(self, box):
        self.box = box

    def get_init_edges(self, xyz, num=48, cutoff=3.0, eta=2.0):
        return get_init_edges_pbc(xyz, self.box, num, cutoff, eta)


@contextlib.contextmanager
def _periodic_grad_ref(box):
    saved = xgr.edges64, xgr.orc
    xgr.edges64, xgr.orc = _edges64_pbc(box), _OrcPBC(box)
    try:
        yield
    finally:
        xgr.edges64, xgr.orc = saved


def vjp64_pbc(xyz, x, Q, g, box, weights, N=None, h_dim=48, cutoff=3.0, eta=2.0, kink_shift=0.0, near_tol=1e-5, dtype=np.float64):
    """(q (N,), gxyz (n, 3)) of one molecule in the cell box (3,): xgr.vjp64 on minimum-image edges (dtype: its float32 model)."""
    with _periodic_grad_ref(box):
        return xgr.vjp64(xyz, x, Q, g, weights, N, h_dim, cutoff, eta, kink_shift=kink_shift, near_tol=near_tol, dtype=dtype)


def forward64_pbc(xyz, x, Q, box, weights, N=None, h_dim=48, cutoff=3.0, eta=2.0, near_tol=1e-5):
    with _periodic_grad_ref(box):
        return xgr.forward64(xyz, x, Q, weights, N, h_dim, cutoff, eta, near_tol=near_tol)


def random_cell(rng, n, L, min_sep=0.9):
    """n atoms uniform in the cell L (3,) with a minimum-image separation of min_sep; an open axis (L = 0) spans [0, 6) A."""
    L = np.asarray(L, dtype=np.float32)
    span = np.where(L > 0, L.astype(np.float64), 6.0)
    pts = []
    while len(pts) < n:
        p = rng.uniform(0, 1, 3) * span
        if all(np.sum(mic(p - q, L) ** 2) >= min_sep ** 2 for q in pts):
            pts.append(p)
    return np.array(pts, dtype=np.float32)
