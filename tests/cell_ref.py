"""Float64 reference for general (triclinic) cells (epnn_forward_xyz_cell, epnn_charges_vjp_xyz_cell, epnn_edges_cell). Test helper.

Built like tests/periodic_ref.py: the model sees the geometry only through the pair distances of get_init_edges, so the model
in a general cell is the oracle's own layer functions on edges whose distances come from the image rule of include/epnn.h:

    d = r_j - r_i;  n_k = rint(g_k . d) on every periodic axis;  d' = ((d - n_0 a_0) - n_1 a_1) - n_2 a_2;
    D = sqrt((dx'^2 + dy'^2) + dz'^2)

all in float64 from the float32 inputs, g_k the dual vector of a_k inside the span of the periodic (non-zero) rows.
tests/xyz_grad_ref.py is used as it is (its edges replaced, as tests/periodic_ref.py does it); strain64 is the strain derivative of
sum_i g_i q_i formed from xyz_grad_ref's dF/dD.
"""
from __future__ import annotations

import contextlib

import numpy as np

from oracle import epnn_oracle as orc
import xyz_grad_ref as xgr


def cell_rows(cell, B):
    cell = np.asarray(cell, dtype=np.float32)
    return np.tile(cell, (B, 1, 1)) if cell.shape == (3, 3) else cell.reshape(B, 3, 3)


def duals(cell):
    """(a (3,3) float64, g (3,3) float64) of the float32 cell: g[k] . a[l] = delta_kl over the periodic rows, zero rows for open
    axes."""
    return duals64(np.asarray(cell, dtype=np.float32).astype(np.float64))


def duals64(a):
    """duals of a float64 cell taken as it is (finite differences deform the cell off the float32 grid)."""
    a = np.asarray(a, dtype=np.float64).reshape(3, 3)
    per = [k for k in range(3) if np.any(a[k] != 0.0)]
    g = np.zeros((3, 3))
    if len(per) == 3:
        det = np.dot(a[0], np.cross(a[1], a[2]))
        g[0], g[1], g[2] = np.cross(a[1], a[2]) / det, np.cross(a[2], a[0]) / det, np.cross(a[0], a[1]) / det
    elif len(per) == 2:
        p, q = per
        n = np.cross(a[p], a[q])
        g[p], g[q] = np.cross(a[q], n) / np.dot(n, n), np.cross(n, a[p]) / np.dot(n, n)
    elif len(per) == 1:
        p = per[0]
        g[p] = a[p] / np.dot(a[p], a[p])
    return a, g


def widths(cell):
    """Perpendicular widths 1 / |g_k| of the periodic axes (inf for an open axis)."""
    _, g = duals(cell)
    n = np.sqrt((g * g).sum(1))
    return np.where(n > 0, 1.0 / np.where(n > 0, n, 1.0), np.inf)


def mic(d, cell):
    """The image of float64 displacements d (..., 3) that the cell contract names."""
    return mic64(d, *duals(cell))


def mic64(d, a, g):
    d = np.asarray(d, dtype=np.float64)
    n = [np.rint((g[k, 0] * d[..., 0] + g[k, 1] * d[..., 1]) + g[k, 2] * d[..., 2]) for k in range(3)]
    out = np.empty_like(d)
    for c in range(3):
        out[..., c] = ((d[..., c] - n[0] * a[0, c]) - n[1] * a[1, c]) - n[2] * a[2, c]
    return out


def _dist(d):
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def _edge_rows_cell(xyz64, cell, i0, i1, num, cutoff, eta):
    mu = np.linspace(0.1, cutoff, num=num)
    D = _dist(mic(xyz64[None, :, :] - xyz64[i0:i1, None, :], cell))
    C = (np.cos(np.pi * (D - 0.0) / cutoff) + 1.0) / 2.0
    C[D >= cutoff] = 0.0
    C[D <= 0.0] = 1.0
    idx = np.arange(i0, i1)
    C[idx - i0, idx] = 0.0
    e = (C[:, :, None] * np.exp(-eta * (D[:, :, None] - mu[None, None, :]) ** 2)).astype(np.float32)
    return e, C


def get_init_edges_cell(xyz, cell, num=48, cutoff=3.0, eta=2.0):
    """(e float32 (n,n,num), C float64 (n,n)) of one system in the cell (3,3)."""
    xyz64 = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    return _edge_rows_cell(xyz64, cell, 0, xyz64.shape[0], num, cutoff, eta)


class EdgeRowsCell(orc.EdgeRows):
    """orc.EdgeRows with the cell's image distances."""

    def __init__(self, xyz, cell, num=48, cutoff=3.0, eta=2.0):
        super().__init__(xyz, num, cutoff, eta)
        self.cell = np.asarray(cell, dtype=np.float32)

    def rows(self, i0, i1):
        key = (i0, min(i1, self.shape[1]))
        if key not in self._blocks:
            self._blocks[key] = _edge_rows_cell(self.xyz, self.cell, key[0], key[1], self.num, self.cutoff, self.eta)[0][None]
        return self._blocks[key]


def forward_cell(xyz, x, Q, cell, weights, N=None, dtype=np.float64, h_dim=48, cutoff=3.0, eta=2.0, near_tol=1e-5):
    """One molecule padded to N in the cell (3,3): orc.dense_inputs with the cell's edges, orc.model_forward.  (N,) charges."""
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[0]
    N = n if N is None else N
    h_p, e_p, x_p, q_p, mask = orc.dense_inputs(xyz, x, Q, N, h_dim=h_dim, e_dim=h_dim, cutoff=cutoff, eta=eta)
    e, _ = get_init_edges_cell(xyz, cell, num=h_dim, cutoff=cutoff, eta=eta)
    e_p[:n, :n] = e
    return orc.model_forward(h_p[None], e_p[None], x_p[None], q_p[None], mask[None], weights, dtype, near_tol=near_tol)[0, :, 0]


def forward_large_cell(xyz, x, Q, cell, weights, dtype=np.float64, cutoff=3.0, eta=2.0, near_tol=1e-5):
    """orc.forward_xyz_large in the cell (3,3): one unpadded system, edge rows a block at a time."""
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[0]
    h = np.zeros((1, n, 48), dtype=dtype)
    q = np.full((1, n, 1), np.float32(np.float32(Q) / np.float32(n)), dtype=dtype)
    mask = np.ones((1, n, 1, 1), dtype=dtype)
    e = EdgeRowsCell(xyz, cell, 48, cutoff, eta)
    xx = x[None].astype(dtype)
    feats = orc.gnn_layer(h, e, xx, q, mask, weights["msg"], weights["upd"], dtype)
    return orc.epn_layer(feats, e, xx, q, mask, weights["pas"], dtype, near_tol=near_tol)[0, :, 0]


def pairs_cell(xyz, cell, cutoff=3.0, eta=2.0, tol=1e-5, num=48, block=64):
    """The pair list epnn_debug_pairs reports for one system: (i, j, near) for every i < j with D < cutoff, near = max_k e_k > tol
    in float32.  Exact, a block of rows at a time."""
    r = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    n = r.shape[0]
    I, J, W = [], [], []
    mu = np.linspace(0.1, cutoff, num=num)
    for i0 in range(0, n, block):
        i1 = min(n, i0 + block)
        D = _dist(mic(r[None, :, :] - r[i0:i1, None, :], cell))
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


def _edges64_cell(cell, outer=False):
    def edges64(xyz, num, cutoff=3.0, eta=2.0):
        """xgr.edges64 on the cell's image displacements: (e, de/dD, r_i - r_j, D).  outer: the displacement is followed by its
        nine products d_a d_c, so that xgr's last line, sum_j (dF/dD_ij / D_ij) * (...), forms the strain sum beside gxyz."""
        return edges64_at(np.asarray(xyz, dtype=np.float32).astype(np.float64), duals(cell)[0], num, cutoff, eta, outer)
    return edges64


def edges64_at(r, a, num, cutoff=3.0, eta=2.0, outer=False):
    """_edges64_cell's result for float64 coordinates r and a float64 cell a, both taken as they are."""
    mu = np.linspace(0.1, cutoff, num=num)
    d = mic64(r[:, None, :] - r[None, :, :], *duals64(a))
    D = _dist(d)
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
    if outer:
        d = np.concatenate([d, (d[:, :, :, None] * d[:, :, None, :]).reshape(d.shape[0], d.shape[1], 9)], -1)
    return C[:, :, None] * ex, (dC[:, :, None] - 2.0 * eta * u * C[:, :, None]) * ex, d, D


class _OrcCell:
    """orc with get_init_edges replaced by its cell form (what xgr._inputs calls)."""

    def __init__(self, cell):
        self.cell = cell

    def get_init_edges(self, xyz, num=48, cutoff=3.0, eta=2.0):
        return get_init_edges_cell(xyz, self.cell, num, cutoff, eta)


@contextlib.contextmanager
def _cell_grad_ref(cell, outer=False):
    saved = xgr.edges64, xgr.orc
    xgr.edges64, xgr.orc = _edges64_cell(cell, outer), _OrcCell(cell)
    try:
        yield
    finally:
        xgr.edges64, xgr.orc = saved


def vjp64_cell(xyz, x, Q, g, cell, weights, N=None, h_dim=48, cutoff=3.0, eta=2.0, kink_shift=0.0, near_tol=1e-5, dtype=np.float64):
    """(q (N,), gxyz (n, 3)) of one molecule in the cell (3,3): xgr.vjp64 on the cell's edges (dtype: its float32 model)."""
    with _cell_grad_ref(cell):
        return xgr.vjp64(xyz, x, Q, g, weights, N, h_dim, cutoff, eta, kink_shift=kink_shift, near_tol=near_tol, dtype=dtype)


def strain64(xyz, x, Q, g, cell, weights, N=None, h_dim=48, cutoff=3.0, eta=2.0, kink_shift=0.0, near_tol=1e-5, dtype=np.float64):
    """(q (N,), gxyz (n, 3), gstrain (3, 3)): gstrain[a][c] = d(sum_i g_i q_i)/d eps_ac under r -> (1 + eps) r, a_k -> (1 + eps) a_k,
    = sum over pairs i < j with D < cutoff of (dF/dD_ij) d'_a d'_c / D_ij.  xgr sums over ordered pairs: half of it.  dtype:
    xgr.vjp64's float32 model; the strain sum stays in float64 and is rounded to float32 at its end."""
    with _cell_grad_ref(cell, outer=True):
        q, ext = xgr.vjp64(xyz, x, Q, g, weights, N, h_dim, cutoff, eta, kink_shift=kink_shift, near_tol=near_tol, dtype=dtype)
    gs = 0.5 * ext[:, 3:].sum(0).reshape(3, 3)
    return q, ext[:, :3], gs if np.dtype(dtype) == np.float64 else gs.astype(np.float32).astype(np.float64)


def forward64_cell(xyz, x, Q, cell, weights, N=None, h_dim=48, cutoff=3.0, eta=2.0, near_tol=1e-5):
    with _cell_grad_ref(cell):
        return xgr.forward64(xyz, x, Q, weights, N, h_dim, cutoff, eta, near_tol=near_tol)


def random_cell(rng, n, cell, min_sep=0.9):
    """n atoms uniform in the cell (3,3) with an image separation of min_sep; an open axis (zero row) spans 6 A along the
    Cartesian axis of its index."""
    a, _ = duals(cell)
    span = a.copy()
    for k in range(3):
        if not np.any(a[k] != 0.0):
            span[k, k] = 6.0
    pts = []
    while len(pts) < n:
        p = rng.uniform(0, 1, 3) @ span
        if all(np.sum(mic(p - q, cell) ** 2) >= min_sep ** 2 for q in pts):
            pts.append(p)
    return np.array(pts, dtype=np.float32)


# the cells of the GPU tests (widths at cutoff 3 beside them)
SHEARED = np.float32([[8, 0, 0], [3, 7.5, 0], [-2.5, 2, 7]])                                    # 6.81, 7.21, 7.00
HEX120 = np.float32([[7, 0, 0], [-3.5, 7 * np.sqrt(3) / 2, 0], [0, 0, 6.5]])                   # 6.06, 6.06, 6.5
HEX60 = np.float32([[7.5, 0, 0], [3.75, 7.5 * np.sqrt(3) / 2, 0], [0, 0, 6.5]])                # 6.50, 6.50, 6.5
RHOMB = np.float32([[9, 1.5, 1.5], [1.5, 9, 1.5], [1.5, 1.5, 9]])                               # 8.40 each
HEX_SLAB = np.float32([[7.5, 0, 0], [3.75, 7.5 * np.sqrt(3) / 2, 0], [0, 0, 0]])               # 6.50, 6.50
WIRE = np.float32([[0, 0, 0], [0, 0, 0], [2, 1, 6.5]])                                          # 6.87
THIN = np.float32([[6.5, 0, 0], [5, 6.5, 0], [0, 0, 7]])                                        # width 5.15: refused
BASIS_A = np.float32([[12, 0, 0], [4, 11, 0], [-3, 2.5, 10.5]])                                 # 10.6, 10.7, 10.5
BASIS_B = np.float32([[12, 0, 0], [16, 11, 0], [-3, 2.5, 10.5]])                                # 6.4, 10.7, 10.5 (b + a for b)
