"""Thin object wrapper over the C ABI: one Engine == one epnn_handle == one GPU."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import W_MSG, W_PAS, W_UPD, EpnnConfig, EpnnError, check, fptr, iptr

KE_EV_ANGSTROM = 14.3996454784255      # e^2 / (4 pi eps0) in eV Angstrom: coulomb_xyz's default ke (332.0637: kcal/mol)
_WHICH = {"msg": W_MSG, "upd": W_UPD, "pas": W_PAS}
_FORWARD_SHAPES = "forward_xyz: shapes xyz {xyz} x {x} Q {Q} do not match offsets (A={A}, B={B}, nx={nx})"


def _box_rows(box, B):
    """A periodic cell argument -> (B, 3) float32 rows: shape (3,) applies to every molecule, (B, 3) gives one row each.  Lengths
    > 0 are periodic axes, 0 open ones (include/epnn.h); the library checks the values."""
    box = np.asarray(box, dtype=np.float32)
    if box.shape == (3,):
        return np.ascontiguousarray(np.tile(box, (B, 1)))
    if box.shape != (B, 3):
        raise ValueError(f"box must have shape (3,) or ({B}, 3), got {box.shape}")
    return np.ascontiguousarray(box)


def _cell_rows(cell, B):
    """A general cell argument -> (B, 3, 3) float32: shape (3, 3) applies to every molecule, (B, 3, 3) gives one cell each.  Row k
    is lattice vector a_k, a row of zeros an open axis (include/epnn.h); the library checks the values."""
    cell = np.asarray(cell, dtype=np.float32)
    if cell.shape == (3, 3):
        return np.ascontiguousarray(np.tile(cell, (B, 1, 1)))
    if cell.shape != (B, 3, 3):
        raise ValueError(f"cell must have shape (3, 3) or ({B}, 3, 3), got {cell.shape}")
    return np.ascontiguousarray(cell)


def _slab_box(where, box, cell):
    """A slab's box has exactly one zero, the open axis."""
    if box is not None and cell is None:
        rows = np.asarray(box, dtype=np.float32)
        if rows.shape[-1:] != (3,) or ((rows.reshape(-1, 3) == 0).sum(1) != 1).any():
            raise ValueError(f"{where}: box must have exactly one zero, the open axis (none: coulomb_xyz_cell)")


def _one_periodic_argument(box, cell):
    if box is not None and cell is not None:
        raise ValueError("box and cell are two descriptions of the same thing: give one of them")


def _geometry(box, cell, B, cells_only=False):
    """box= / cell= (at most one: _one_periodic_argument) -> what the C entry of that geometry is named after and takes: ("", None),
    ("_pbc", (B, 3) rows) or ("_cell", (B, 3, 3) rows).  cells_only (entries that take a cell or nothing): a box becomes its diagonal cell."""
    if box is not None:
        box = _box_rows(box, B)
        if not cells_only:
            return "_pbc", box
        cell = np.zeros((B, 3, 3), dtype=np.float32)
        cell[:, [0, 1, 2], [0, 1, 2]] = box
    if cell is not None:
        return "_cell", _cell_rows(cell, B)
    return "", None


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class DeviceArray:
    """A device allocation owned by an Engine (used by bench.py to keep inputs resident in HBM)."""

    def __init__(self, eng, nbytes):
        self.eng = eng
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(eng.lib.epnn_dev_alloc(eng.h, self.nbytes, C.byref(p)), eng.lib)
        self.ptr = p

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        check(self.eng.lib.epnn_memcpy_h2d(self.eng.h, self.ptr, arr.ctypes.data_as(C.c_void_p), arr.nbytes), self.eng.lib)
        return self

    def download(self, shape, dtype=np.float32):
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        check(self.eng.lib.epnn_memcpy_d2h(self.eng.h, out.ctypes.data_as(C.c_void_p), self.ptr, out.nbytes), self.eng.lib)
        return out

    def free(self):
        if self.ptr is not None and self.eng.h:
            self.eng.lib.epnn_dev_free(self.eng.h, self.ptr)
        self.ptr = None



def _exclusion_lists(where, exclusions):
    """(pairs, scale) -> the three contiguous lists of the _excl entries: int32 (P,), int32 (P,), float32 (P,)."""
    try:
        pairs, scale = exclusions
    except (TypeError, ValueError):
        raise ValueError(f"{where}: exclusions must be (pairs, scale)") from None
    pairs = np.asarray(pairs)
    if pairs.size == 0:
        pairs = np.zeros((0, 2), dtype=np.int64)
    if pairs.ndim != 2 or pairs.shape[1] != 2 or not np.issubdtype(pairs.dtype, np.integer):
        raise ValueError(f"{where}: exclusion pairs must be an integer array of shape (P, 2), got {pairs.dtype} {pairs.shape}")
    P = pairs.shape[0]
    if P and (pairs.min() < -2 ** 31 or pairs.max() >= 2 ** 31):
        raise ValueError(f"{where}: an exclusion index does not fit 32 bits")
    scale = np.asarray(scale, dtype=np.float32)
    if scale.ndim == 0:
        scale = np.full((P,), scale, dtype=np.float32)
    if scale.shape != (P,):
        raise ValueError(f"{where}: exclusion scale must be a scalar or have shape ({P},), got {scale.shape}")
    return (np.ascontiguousarray(pairs[:, 0], dtype=np.int32), np.ascontiguousarray(pairs[:, 1], dtype=np.int32),
            np.ascontiguousarray(scale))


def per_element(Z, table, default=None):
    """A per-atom float32 array (A,) for coulomb_xyz_site's sigma, chi and hardness from a table by element: Z (A,) the atomic numbers
    (x[:, 0] of the flat batch), table a dict {Z: value}.  An element the table lacks takes default; with default None it raises,
    naming the element."""
    Z = np.asarray(Z)
    if Z.ndim != 1:
        raise ValueError(f"per_element: Z must have shape (A,), got {Z.shape}")
    zi = np.rint(Z).astype(np.int64)
    if Z.size and np.abs(np.asarray(Z, dtype=np.float64) - zi).max() != 0.0:
        raise ValueError("per_element: Z must hold whole atomic numbers")
    out = np.empty(zi.shape, dtype=np.float32)
    for z in np.unique(zi):
        if int(z) in table:
            out[zi == z] = table[int(z)]
        elif default is not None:
            out[zi == z] = default
        else:
            raise KeyError(f"per_element: the table has no value for element Z = {int(z)}")
    return out


def bonded_exclusions(bonds, n_atoms, scale12=0.0, scale13=0.0, scale14=0.5):
    """The exclusion list of a force field from a bond list: bonds (nb, 2) int, flat atom indices below n_atoms -> (pairs (P, 2) int32,
    scale (P,) float32) for coulomb_xyz_excl and coulomb_xyz_cell_excl.  Every pair at graph distance 1, 2 or 3 once, i < j, sorted;
    its factor is that of its shortest path (in a ring a pair that is both 1-3 and 1-4 counts as 1-3); pairs whose factor is 1 are
    dropped.  Pure numpy, no GPU."""
    n = int(n_atoms)
    bonds = np.asarray(bonds, dtype=np.int64).reshape(-1, 2)
    if bonds.size and (bonds.min() < 0 or bonds.max() >= n):
        raise ValueError(f"bonded_exclusions: a bond names an atom outside [0, {n})")
    if (bonds[:, 0] == bonds[:, 1]).any():
        raise ValueError("bonded_exclusions: a bond from an atom to itself")
    both = np.unique(np.concatenate([bonds, bonds[:, ::-1]]), axis=0)               # directed, duplicates gone, sorted by (i, j)
    key = lambda p: p[:, 0] * n + p[:, 1]
    found, frontier, out = key(both), both, []
    for depth, factor in enumerate((scale12, scale13, scale14)):
        fwd = frontier[frontier[:, 0] < frontier[:, 1]]
        out.append((fwd, np.full(len(fwd), factor, dtype=np.float32)))
        if depth == 2 or not len(frontier):
            break
        # one bond further from every end j: (i, k) for the bonds (j, k), less what a shorter path reached already
        start = np.searchsorted(both[:, 0], frontier[:, 1], "left")
        cnt = np.searchsorted(both[:, 0], frontier[:, 1], "right") - start
        src = np.repeat(np.arange(len(frontier)), cnt)
        idx = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(start, cnt)
        nxt = np.unique(np.stack([frontier[src, 0], both[idx, 1]], 1), axis=0) if len(src) else np.zeros((0, 2), dtype=np.int64)
        nxt = nxt[(nxt[:, 0] != nxt[:, 1]) & ~np.isin(key(nxt), found)]
        found = np.concatenate([found, key(nxt)])
        frontier = nxt
    pairs = np.concatenate([p for p, _ in out]) if out else np.zeros((0, 2), dtype=np.int64)
    scale = np.concatenate([f for _, f in out]) if out else np.zeros((0,), dtype=np.float32)
    keep = scale != 1.0
    pairs, scale = pairs[keep], scale[keep]
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    return pairs[order].astype(np.int32), scale[order]


class Engine:
    def __init__(self, nx=9, h_dim=48, e_dim=48, T=5, hidden=32, cutoff=3.0, eta=2.0, near_tol=1e-5, device=0, fused_only=False):
        """fused_only: epnn_create_fused -- nx up to 13, and with nx > 10 only forward_xyz* on molecules of at most 64 atoms."""
        self.lib = _lib.load()
        self.cfg = EpnnConfig(nx, h_dim, e_dim, T, hidden, cutoff, eta, near_tol)
        self.nx, self.h_dim, self.e_dim, self.T = nx, h_dim, e_dim, T
        self.device = device
        h = C.c_void_p()
        check((self.lib.epnn_create_fused if fused_only else self.lib.epnn_create)(C.byref(self.cfg), device, C.byref(h)), self.lib)
        self.h = h
        self._upd_layers = [hidden, hidden]              # hidden widths of the update MLP (set_update_layers)

    def close(self):
        if getattr(self, "h", None):
            self.lib.epnn_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ weights
    def weight_shape(self, group, t, layer):
        a, b = C.c_int32(), C.c_int32()
        check(self.lib.epnn_weight_shape(self.h, _WHICH[group], t, layer, C.byref(a), C.byref(b)), self.lib)
        return a.value, b.value

    def set_layer(self, group, t, layer, kernel, bias):
        shp = self.weight_shape(group, t, layer)
        kernel, bias = _f32(kernel), _f32(bias)
        if kernel.shape != shp or bias.shape != (shp[1],):
            raise EpnnError(f"{group}[{t}] layer {layer}: expected kernel {shp} / bias ({shp[1]},), "
                            f"got {kernel.shape} / {bias.shape}")
        check(self.lib.epnn_set_weights(self.h, _WHICH[group], t, layer, fptr(kernel), fptr(bias)), self.lib)

    def get_layer(self, group, t, layer):
        shp = self.weight_shape(group, t, layer)
        k = np.empty(shp, dtype=np.float32)
        b = np.empty((shp[1],), dtype=np.float32)
        check(self.lib.epnn_get_weights(self.h, _WHICH[group], t, layer, fptr(k), fptr(b)), self.lib)
        return k, b

    def set_update_layers(self, widths):
        """make_model(layers, ...): hidden widths of the update MLP (charge_gn.py:371); [32, 32] is the default and the tuned shape."""
        widths = [int(w) for w in widths]
        if widths != self._upd_layers:
            arr = np.ascontiguousarray(widths, dtype=np.int32)
            check(self.lib.epnn_set_update_layers(self.h, len(widths), iptr(arr)), self.lib)
            self._upd_layers = widths

    def set_weights(self, weights):
        """weights = {"msg": [T][3](W,b), "upd": [n_hidden + 1](W,b), "pas": [T][3](W,b)} (checkpoint.load_epnn_weights); the update
        MLP's hidden widths follow the kernels' shapes."""
        if len(weights["msg"]) != self.T or len(weights["pas"]) != self.T:
            raise EpnnError(f"checkpoint has T={len(weights['msg'])}, engine was built with T={self.T}")
        self.set_update_layers([np.asarray(k).shape[1] for k, _ in weights["upd"][:-1]])
        for t in range(self.T):
            for l in range(3):
                self.set_layer("msg", t, l, *weights["msg"][t][l])
                self.set_layer("pas", t, l, *weights["pas"][t][l])
        for l in range(len(weights["upd"])):
            self.set_layer("upd", 0, l, *weights["upd"][l])

    def get_weights(self):
        return {"msg": [[self.get_layer("msg", t, l) for l in range(3)] for t in range(self.T)],
                "upd": [self.get_layer("upd", 0, l) for l in range(len(self._upd_layers) + 1)],
                "pas": [[self.get_layer("pas", t, l) for l in range(3)] for t in range(self.T)]}

    # ------------------------------------------------------------------ compute
    def edges(self, xyz):
        xyz = _f32(xyz)
        n = xyz.shape[0]
        out = np.empty((n, n, self.e_dim), dtype=np.float32)
        check(self.lib.epnn_edges(self.h, n, fptr(xyz), fptr(out)), self.lib)
        return out

    def edges_ex(self, xyz, num, cutoff=3.0, eta=2.0, box=None, cell=None):
        """get_init_edges with its own parameters: (e float32 (n,n,num), C float64 (n,n)) from the device kernel.  box (3,):
        minimum-image distances in that periodic cell; cell (3, 3): in that general cell (include/epnn.h)."""
        _one_periodic_argument(box, cell)
        xyz = _f32(xyz)
        n = xyz.shape[0]
        e = np.empty((n, n, int(num)), dtype=np.float32)
        c = np.empty((n, n), dtype=np.float64)
        if cell is not None:
            cell = np.asarray(cell, dtype=np.float32)
            if cell.shape != (3, 3):
                raise ValueError(f"edges_ex: cell must have shape (3, 3), got {cell.shape}")
            cell = np.ascontiguousarray(cell)
            check(self.lib.epnn_edges_cell(self.h, n, fptr(xyz), fptr(cell), int(num), float(cutoff), float(eta), fptr(e),
                                           c.ctypes.data_as(C.POINTER(C.c_double))), self.lib)
        elif box is None:
            check(self.lib.epnn_edges_ex(self.h, n, fptr(xyz), int(num), float(cutoff), float(eta), fptr(e),
                                         c.ctypes.data_as(C.POINTER(C.c_double))), self.lib)
        else:
            box = np.asarray(box, dtype=np.float32)
            if box.shape != (3,):
                raise ValueError(f"edges_ex: box must have shape (3,), got {box.shape}")
            box = np.ascontiguousarray(box)
            check(self.lib.epnn_edges_pbc(self.h, n, fptr(xyz), fptr(box), int(num), float(cutoff), float(eta), fptr(e),
                                          c.ctypes.data_as(C.POINTER(C.c_double))), self.lib)
        return e, c

    def forward_xyz(self, offsets, xyz, x, Q, N, box=None, cell=None):
        """Flat batch: offsets (B+1,), xyz (A,3), x (A,nx), Q (B,) -> q (A,) float32.  box (3,) or (B, 3): periodic cells
        (include/epnn.h: > 0 periodic length, 0 open axis).  cell (3, 3) or (B, 3, 3): general (triclinic) cells, row k the
        lattice vector a_k, a zero row an open axis."""
        _one_periodic_argument(box, cell)
        offsets, xyz, x, Q, _, B, A = self._flat_batch(_FORWARD_SHAPES, offsets, xyz, x, Q)
        suffix, rows = _geometry(box, cell, B)
        out = np.empty((A,), dtype=np.float32)
        check(getattr(self.lib, "epnn_forward_xyz" + suffix)(self.h, B, int(N), iptr(offsets), fptr(xyz), fptr(x), fptr(Q),
                                                            *([] if rows is None else [fptr(rows)]), fptr(out)), self.lib)
        return out

    def _flat_batch(self, message, offsets, xyz, x, Q, per_atom=None):
        """A flat batch as the C entries take it: offsets int32 (B+1,), xyz (A, 3), x (A, nx), Q (B,), a per-atom array (A,) where the method
        has one, float32 and contiguous -> (offsets, xyz, x, Q, per_atom, B, A); message: the method's text for shapes that do not match."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        xyz, x, Q = _f32(xyz), _f32(x), _f32(Q)
        per_atom = None if per_atom is None else _f32(per_atom)
        B, A = len(offsets) - 1, int(offsets[-1])
        if xyz.shape != (A, 3) or x.shape != (A, self.nx) or Q.shape != (B,) or (per_atom is not None and per_atom.shape != (A,)):
            raise EpnnError(message.format(xyz=xyz.shape, x=x.shape, Q=Q.shape, A=A, B=B, nx=self.nx))
        return offsets, xyz, x, Q, per_atom, B, A

    def forward_xyz_begin(self, offsets, xyz, x, Q, N):
        """First half of forward_xyz: returns as soon as the work is queued (the arrays may be reused at once).  Until
        forward_xyz_end, this engine refuses another begin and forward_xyz; its other methods are served and leave the begun forward's
        result alone, new weights and options counting from the next forward on (include/epnn.h at epnn_forward_xyz_begin)."""
        offsets, xyz, x, Q, _, B, A = self._flat_batch(_FORWARD_SHAPES, offsets, xyz, x, Q)
        check(self.lib.epnn_forward_xyz_begin(self.h, B, int(N), iptr(offsets), fptr(xyz), fptr(x), fptr(Q)), self.lib)
        self._begun = A

    def forward_xyz_end(self):
        """Second half: waits for the forward begun on this engine and returns its charges q (A,) float32."""
        A = getattr(self, "_begun", None)
        if A is None:
            raise EpnnError("forward_xyz_end: no forward was begun on this engine")
        self._begun = None
        out = np.empty((A,), dtype=np.float32)
        check(self.lib.epnn_forward_xyz_end(self.h, fptr(out)), self.lib)
        return out

    def _dense_args(self, B, N, tensors, chans):
        out = []
        for t, ch in zip(tensors, chans):
            t = _f32(t)
            if t.ndim == len(ch) + 1 - 1 and ch[-1] == 1 and t.shape == (B,) + ch[:-1]:
                t = t.reshape((B,) + ch)          # rank-3 mask -> rank 4 like Keras does
            if t.shape != (B,) + ch:
                raise EpnnError(f"expected shape {(B,) + ch}, got {t.shape}")
            out.append(t)
        return out

    def model_forward_dense(self, h_inp, e_inp, x_inp, q_inp, mask_inp):
        e_inp = _f32(e_inp)
        B, N = e_inp.shape[0], e_inp.shape[1]
        h_inp, e_inp, x_inp, q_inp, mask_inp = self._dense_args(
            B, N, (h_inp, e_inp, x_inp, q_inp, mask_inp),
            ((N, N, self.h_dim), (N, N, self.e_dim), (N, N, self.nx), (N, N, 1), (N, N, 1)))
        out = np.empty((B, N, 1), dtype=np.float32)
        check(self.lib.epnn_model_forward_dense(self.h, B, N, fptr(h_inp), fptr(e_inp), fptr(x_inp), fptr(q_inp),
                                                fptr(mask_inp), fptr(out)), self.lib)
        return out

    def _layer(self, fn, h, e, x, q, mask, out_ch):
        e = _f32(e)
        B, N = e.shape[0], e.shape[1]
        h, e, x, q, mask = self._dense_args(
            B, N, (h, e, x, q, mask), ((N, self.h_dim), (N, N, self.e_dim), (N, self.nx), (N, 1), (N, N, 1)))
        out = np.empty((B, N, out_ch), dtype=np.float32)
        check(fn(self.h, B, N, fptr(h), fptr(e), fptr(x), fptr(q), fptr(mask), fptr(out)), self.lib)
        return out

    def gnn_forward(self, h, e, x, q, mask):
        return self._layer(self.lib.epnn_gnn_forward, h, e, x, q, mask, self.h_dim)

    def epn_forward(self, h, e, x, q, mask):
        return self._layer(self.lib.epnn_epn_forward, h, e, x, q, mask, 1)

    ACTIVATIONS = {"relu": 0, None: 1, "linear": 1, "tanh": 2, "sigmoid": 3}

    def mlp_forward_layers(self, rows, layers, activation="relu"):
        """MLP_layer(nodes, out_dim, activation).call for any `nodes`: rows (R, n_in) through [(W,b), ...], `activation` after all
        but the last layer ('relu', None / 'linear', 'tanh', 'sigmoid': charge_gn.py:38-39)."""
        if activation not in self.ACTIVATIONS:
            raise EpnnError(f"mlp_forward_layers: activation {activation!r} is not built (relu, None / linear, tanh, sigmoid)")
        rows = _f32(rows)
        ws = [(_f32(k), _f32(b)) for k, b in layers]
        dims = [rows.shape[1]] + [k.shape[1] for k, _ in ws]
        for l, (k, b) in enumerate(ws):
            if k.shape != (dims[l], dims[l + 1]) or b.shape != (dims[l + 1],):
                raise EpnnError(f"mlp_forward_layers: layer {l} has kernel {k.shape} / bias {b.shape}, expected {(dims[l], dims[l + 1])}")
        n = len(ws)
        FP = C.POINTER(C.c_float)
        Wp = (FP * n)(*[fptr(k) for k, _ in ws])
        bp = (FP * n)(*[fptr(b) for _, b in ws])
        darr = np.ascontiguousarray(dims, dtype=np.int32)
        out = np.empty((rows.shape[0], dims[-1]), dtype=np.float32)
        check(self.lib.epnn_mlp_forward_layers(self.h, rows.shape[0], n, iptr(darr), Wp, bp, fptr(rows), fptr(out), self.ACTIVATIONS[activation]), self.lib)
        return out

    def mlp_forward(self, rows, layers):
        """MLP_layer.call: rows (R, n_in) through [(W1,b1),(W2,b2),(W3,b3)] with hidden width 32."""
        rows = _f32(rows)
        (W1, b1), (W2, b2), (W3, b3) = [(_f32(k), _f32(b)) for k, b in layers]
        if W1.shape != (rows.shape[1], 32) or W2.shape != (32, 32) or W3.shape[0] != 32:
            raise EpnnError(f"mlp_forward: unsupported layer shapes {W1.shape} {W2.shape} {W3.shape}")
        out = np.empty((rows.shape[0], W3.shape[1]), dtype=np.float32)
        check(self.lib.epnn_mlp_forward(self.h, rows.shape[0], rows.shape[1], W3.shape[1], fptr(W1), fptr(b1), fptr(W2),
                                        fptr(b2), fptr(W3), fptr(b3), fptr(rows), fptr(out)), self.lib)
        return out

    # ------------------------------------------------------------------ training (charge_gn.py:393-402)
    def train_init(self, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-7):
        check(self.lib.epnn_train_init(self.h, lr, beta1, beta2, eps), self.lib)

    def param_count(self):
        n = C.c_int64()
        check(self.lib.epnn_param_count(self.h, C.byref(n)), self.lib)
        return n.value

    def train_step_dense(self, h_inp, e_inp, x_inp, q_inp, mask_inp, y, apply=True):
        """Returns (predictions (B,N,1), summed loss)."""
        e_inp = _f32(e_inp)
        B, N = e_inp.shape[0], e_inp.shape[1]
        h_inp, e_inp, x_inp, q_inp, mask_inp = self._dense_args(
            B, N, (h_inp, e_inp, x_inp, q_inp, mask_inp),
            ((N, N, self.h_dim), (N, N, self.e_dim), (N, N, self.nx), (N, N, 1), (N, N, 1)))
        y = _f32(np.asarray(y).reshape(B, N, 1))
        pred = np.empty((B, N, 1), dtype=np.float32)
        loss = C.c_float()
        check(self.lib.epnn_train_step_dense(self.h, B, N, fptr(h_inp), fptr(e_inp), fptr(x_inp), fptr(q_inp), fptr(mask_inp),
                                             fptr(y), fptr(pred), C.byref(loss), int(bool(apply))), self.lib)
        return pred, loss.value

    def train_step_xyz(self, offsets, xyz, x, Q, y, N, apply=True, box=None, cell=None):
        """Flat batch; y per real atom (A,). Returns (q (A,), summed loss).  box (3,) or (B, 3): periodic cells, cell (3, 3) or
        (B, 3, 3): general cells, as in forward_xyz; with one of them the step runs epnn_train_step_xyz_cell, whose implementation
        set_option("train_path", v) chooses: 0 (default) the dense path while B N^2 <= 2^22 and the pair-list path (per-atom rows and
        the pairs under the cutoff only: large systems) above that, 1 / 2 force one of them.  Without box and cell it is the dense
        step of epnn_train_step_xyz at any size."""
        _one_periodic_argument(box, cell)
        offsets, xyz, x, Q, y, B, A = self._flat_batch("train_step_xyz: array shapes do not match offsets", offsets, xyz, x, Q, y)
        q = np.empty((A,), dtype=np.float32)
        loss = C.c_float()
        suffix, cell = _geometry(box, cell, B, cells_only=True)
        check(getattr(self.lib, "epnn_train_step_xyz" + suffix)(self.h, B, int(N), iptr(offsets), fptr(xyz), fptr(x), fptr(Q),
                                                               *([] if cell is None else [fptr(cell)]), fptr(y), fptr(q), C.byref(loss),
                                                               int(bool(apply))), self.lib)
        return q, loss.value

    def charges_vjp_xyz(self, offsets, xyz, x, Q, g, N, box=None, cell=None, strain=False):
        """Flat batch and a cotangent g (A,) of the charges -> (q (A,), gxyz (A, 3) = sum_i g[i] dq_i/dxyz).  Touches no
        training state; works without train_init.  box (3,) or (B, 3): periodic cells, as in forward_xyz; cell (3, 3) or
        (B, 3, 3): general cells.  strain=True (with cell, or with neither: open molecules) returns (q, gxyz, gstrain) with
        gstrain (B, 3, 3) the derivative of sum_i g[i] q_i with respect to a homogeneous strain of coordinates and cell
        (include/epnn.h: dF/dH = inv(H).T @ gstrain for the cell matrix H at fixed fractional coordinates).
        set_option("grad_path", v) chooses the implementation: 0 (default) the dense path while B N^2 <= 2^22 and the pair-list
        path (per-atom rows and the pairs under the cutoff only: large systems) above that, 1 / 2 force one of them."""
        _one_periodic_argument(box, cell)
        if strain and box is not None:
            raise ValueError("charges_vjp_xyz: strain=True takes the cell as cell= (np.diag(box) for an orthorhombic one)")
        offsets, xyz, x, Q, g, B, A = self._flat_batch("charges_vjp_xyz: array shapes do not match offsets", offsets, xyz, x, Q, g)
        q = np.empty((A,), dtype=np.float32)
        gxyz = np.empty((A, 3), dtype=np.float32)
        suffix, rows = _geometry(box, np.zeros((3, 3), np.float32) if strain and cell is None else cell, B)
        gs = np.empty((B, 3, 3), dtype=np.float32) if strain else None
        check(getattr(self.lib, "epnn_charges_vjp_xyz" + suffix)(self.h, B, int(N), iptr(offsets), fptr(xyz), fptr(x), fptr(Q),
                                                                *([] if rows is None else [fptr(rows)]), fptr(g), fptr(q), fptr(gxyz),
                                                                *([fptr(gs) if strain else None] if suffix == "_cell" else [])), self.lib)
        return (q, gxyz, gs) if strain else (q, gxyz)

    def charges_jvp_xyz(self, offsets, xyz, x, Q, N, v=None, strain=None, dQ=None, box=None, cell=None):
        """Forward mode: flat batch and a direction -> (q (A,), tq (A,)), tq the derivative of the charges along it
        (epnn_charges_jvp_xyz_cell): v (A, 3) a tangent of the coordinates (an MD velocity: tq = dq/dt), strain (3, 3) or
        (B, 3, 3) a homogeneous strain E of coordinates and cell (the one gstrain of charges_vjp_xyz is the derivative for),
        dQ a scalar or (B,) a tangent of the total charges (dQ = 1 alone: dq/dQ, the condensed Fukui function).  Each may be
        None (= 0); the three add up.  box (3,) or (B, 3), cell (3, 3) or (B, 3, 3) as in forward_xyz; neither: open molecules.
        One call costs about one forward of the pair-list gradient path, whose charges q has bit for bit; it touches no training
        state and works without train_init."""
        _one_periodic_argument(box, cell)
        offsets, xyz, x, Q, _, B, A = self._flat_batch("charges_jvp_xyz: array shapes do not match offsets", offsets, xyz, x, Q)
        _, cell = _geometry(box, cell, B, cells_only=True)
        if v is not None:
            v = _f32(v)
            if v.shape != (A, 3):
                raise ValueError(f"charges_jvp_xyz: v must have shape ({A}, 3), got {v.shape}")
        if strain is not None:
            strain = np.asarray(strain, dtype=np.float32)
            if strain.shape == (3, 3):
                strain = np.tile(strain, (B, 1, 1))
            if strain.shape != (B, 3, 3):
                raise ValueError(f"charges_jvp_xyz: strain must have shape (3, 3) or ({B}, 3, 3), got {strain.shape}")
            strain = np.ascontiguousarray(strain)
        if dQ is not None:
            dQ = np.asarray(dQ, dtype=np.float32)
            if dQ.shape == ():
                dQ = np.full((B,), dQ, dtype=np.float32)
            if dQ.shape != (B,):
                raise ValueError(f"charges_jvp_xyz: dQ must be a scalar or have shape ({B},), got {dQ.shape}")
            dQ = np.ascontiguousarray(dQ)
        opt = lambda a: None if a is None else fptr(a)
        q = np.empty((A,), dtype=np.float32)
        tq = np.empty((A,), dtype=np.float32)
        check(self.lib.epnn_charges_jvp_xyz_cell(self.h, B, int(N), iptr(offsets), fptr(xyz), fptr(x), fptr(Q), opt(cell), opt(v),
                                                 opt(strain), opt(dQ), fptr(q), fptr(tq)), self.lib)
        return q, tq

    def charges_jvp_xyz_multi(self, offsets, xyz, x, Q, N, v=None, strain=None, dQ=None, box=None, cell=None):
        """Forward mode along K directions in one pass (epnn_charges_jvp_multi_xyz_cell): (q (A,), tq (K, A)), row k being
        charges_jvp_xyz's tq for the k-th slices, bit for bit, whatever K and the other rows are.  v (K, A, 3), strain (K, 3, 3)
        or (K, B, 3, 3), dQ (K,) or (K, B); each may be None (= 0 for every direction), at least one must be given, and those
        given must agree on K (1..16).  The primal, the pair list and every per-pair and per-atom primal statement run once;
        box and cell as in charges_jvp_xyz."""
        _one_periodic_argument(box, cell)
        offsets, xyz, x, Q, _, B, A = self._flat_batch("charges_jvp_xyz_multi: array shapes do not match offsets", offsets, xyz, x, Q)
        _, cell = _geometry(box, cell, B, cells_only=True)
        Ks = {}
        if v is not None:
            v = _f32(v)
            if v.ndim != 3 or v.shape[1:] != (A, 3):
                raise ValueError(f"charges_jvp_xyz_multi: v must have shape (K, {A}, 3), got {v.shape}")
            Ks["v"] = v.shape[0]
        if strain is not None:
            strain = np.asarray(strain, dtype=np.float32)
            if strain.ndim == 3 and strain.shape[1:] == (3, 3):
                strain = np.repeat(strain[:, None], B, axis=1)
            if strain.ndim != 4 or strain.shape[1:] != (B, 3, 3):
                raise ValueError(f"charges_jvp_xyz_multi: strain must have shape (K, 3, 3) or (K, {B}, 3, 3), got {strain.shape}")
            strain = np.ascontiguousarray(strain)
            Ks["strain"] = strain.shape[0]
        if dQ is not None:
            dQ = np.asarray(dQ, dtype=np.float32)
            if dQ.ndim == 1:
                dQ = np.repeat(dQ[:, None], B, axis=1)
            if dQ.ndim != 2 or dQ.shape[1] != B:
                raise ValueError(f"charges_jvp_xyz_multi: dQ must have shape (K,) or (K, {B}), got {dQ.shape}")
            dQ = np.ascontiguousarray(dQ)
            Ks["dQ"] = dQ.shape[0]
        if not Ks:
            raise ValueError("charges_jvp_xyz_multi: give at least one of v, strain and dQ (they carry K)")
        if len(set(Ks.values())) != 1:
            raise ValueError("charges_jvp_xyz_multi: the tangents disagree on K: " + ", ".join(f"{k} has {n}" for k, n in Ks.items()))
        K = next(iter(Ks.values()))
        opt = lambda a: None if a is None else fptr(a)
        q = np.empty((A,), dtype=np.float32)
        tq = np.empty((max(K, 1), A), dtype=np.float32)
        check(self.lib.epnn_charges_jvp_multi_xyz_cell(self.h, B, int(N), iptr(offsets), fptr(xyz), fptr(x), fptr(Q), opt(cell), int(K),
                                                       opt(v), opt(strain), opt(dQ), fptr(q), fptr(tq)), self.lib)
        return q, tq

    def charges_vjp_xyz_multi(self, offsets, xyz, x, Q, g, N, box=None, cell=None, strain=False):
        """Reverse mode for K cotangents in one pass (epnn_charges_vjp_multi_xyz_cell): g (K, A) -> (q (A,), gxyz (K, A, 3)), with
        strain=True also gstrain (K, B, 3, 3); row k has the bits charges_vjp_xyz gives for g[k] on "grad_path" 2, whatever K and
        the other rows are.  K is 1..16.  The call always runs from the pair list; the set-up, the pair list, the checkpointed
        forward and every primal statement of the backward run once.  box (3,) or (B, 3) is taken as its diagonal cell; cell
        (3, 3) or (B, 3, 3); neither: open molecules (with strain=True an all-zero cell, as in charges_vjp_xyz)."""
        _one_periodic_argument(box, cell)
        offsets, xyz, x, Q, _, B, A = self._flat_batch("charges_vjp_xyz_multi: array shapes do not match offsets", offsets, xyz, x, Q)
        g = _f32(g)
        if g.ndim != 2 or g.shape[1] != A:
            raise ValueError(f"charges_vjp_xyz_multi: g must have shape (K, {A}), got {g.shape}")
        K = g.shape[0]
        _, rows = _geometry(box, np.zeros((3, 3), np.float32) if strain and cell is None and box is None else cell, B, cells_only=True)
        q = np.empty((A,), dtype=np.float32)
        gxyz = np.empty((max(K, 1), A, 3), dtype=np.float32)
        gs = np.empty((max(K, 1), B, 3, 3), dtype=np.float32) if strain else None
        opt = lambda a: None if a is None else fptr(a)
        check(self.lib.epnn_charges_vjp_multi_xyz_cell(self.h, B, int(N), iptr(offsets), fptr(xyz), fptr(x), fptr(Q), opt(rows), int(K),
                                                       fptr(g), fptr(q), fptr(gxyz), opt(gs)), self.lib)
        return (q, gxyz, gs) if strain else (q, gxyz)

    def dipole_xyz(self, offsets, xyz, x, Q, N, origin=None):
        """Dipoles and atomic polar tensors of open molecules from one K = 3 call of charges_vjp_xyz_multi:
        (q (A,), mu (B, 3) float64, apt (A, 3, 3) float32).  With o_b the origin of molecule b -- origin (3,) or (B, 3); by default
        the molecule's unweighted centroid, taken in float64 and treated as a fixed point --
            mu_b        = sum_k q_k (r_k - o_b)                         in float64,
            seeds       g_a[k] = float32(r_ka - o_a),   a = x, y, z,
            apt[i][a][b] = d mu_a / d r_ib = q_i delta_ab + gxyz[a][i][b]    (one float32 add on the diagonal).
        In exact arithmetic sum_i apt[i] = Q_b I over a molecule's atoms (moving the whole molecule moves the dipole by Q_b times
        the displacement), and the APT does not depend on o: the model conserves charge under translation, sum_k dq_k/dr_ib = 0, so
        a shift of o adds nothing.  box / cell are not arguments: a cell's dipole is not a function of the positions."""
        offsets, xyz, x, Q, _, B, A = self._flat_batch("dipole_xyz: array shapes do not match offsets", offsets, xyz, x, Q)
        r = xyz.astype(np.float64)
        counts = np.diff(offsets)
        mol = np.repeat(np.arange(B), counts)
        if origin is None:
            o = np.stack([r[offsets[b]:offsets[b + 1]].mean(axis=0) for b in range(B)])
        else:
            o = np.asarray(origin, dtype=np.float64)
            if o.shape == (3,):
                o = np.tile(o, (B, 1))
            if o.shape != (B, 3):
                raise ValueError(f"dipole_xyz: origin must have shape (3,) or ({B}, 3), got {o.shape}")
        rel = r - o[mol]
        g = np.ascontiguousarray(rel.T.astype(np.float32))
        q, gxyz = self.charges_vjp_xyz_multi(offsets, xyz, x, Q, g, N)
        mu = np.stack([(q[offsets[b]:offsets[b + 1]].astype(np.float64)[:, None] * rel[offsets[b]:offsets[b + 1]]).sum(axis=0)
                       for b in range(B)])
        apt = np.ascontiguousarray(gxyz.transpose(1, 0, 2))
        for a in range(3):
            apt[:, a, a] += q
        return q, mu, apt

    def coulomb_xyz(self, offsets, xyz, x, Q, N, ke=KE_EV_ANGSTROM, alpha=0.0, parts=False):
        """Electrostatics of the predicted charges in one call (epnn_coulomb_xyz): flat batch -> (q (A,), phi (A,), E (B,) float64,
        F (A, 3)) with phi_i = ke sum_{j != i} q_j kappa(D_ij) = dE/dq_i, E = 1/2 sum_i q_i phi_i per molecule and F = -dE/dxyz in
        total: the part at fixed charges plus the part through dq/dxyz.  kappa(D) = 1 / D for alpha = 0 (bare Coulomb) and
        erf(alpha D) / D for alpha > 0 (Gaussian charges of width sigma, alpha = 1 / (2 sigma)); ke is the unit constant
        (KE_EV_ANGSTROM, the default: eV, Angstrom, e; 332.0637: kcal/mol).  parts=True appends ffix (A, 3) and fq (A, 3),
        F = ffix + fq; fq is -gxyz of charges_vjp_xyz(g=phi) on "grad_path" 2, bit for bit, and q has that path's bits.  Open
        systems only (fully periodic cells: coulomb_xyz_cell), no self-energy term; bonded exclusions: coulomb_xyz_excl.  One
        call costs about one gradient call of the pair-list path; it touches no training state and works without train_init."""
        return self._coulomb("coulomb_xyz", offsets, xyz, x, Q, N, ke, alpha, parts)

    def ewald_params(self, cell, alpha=0.0, tol=1e-6):
        """The Ewald parameters coulomb_xyz_cell runs at for one cell (3, 3) (epnn_ewald_params, host only): float64 (6,) = beta,
        rc, kc, M0, M1, M2 with s = sqrt(-ln tol), rc = w_min / 2, beta = s / rc capped at alpha (then rc = 0: no real-space
        part), kc = 2 beta s, M_k = ceil(kc |a_k| / 2 pi).  Refuses open axes, tol outside (0, 1) and k boxes above 2^18 slots."""
        return self._ewald_rule("ewald_params", cell, alpha, tol)

    def _ewald_rule(self, entry, cell, alpha, tol):
        """ewald_params and ewald_slab_params: one cell (3, 3) through the host-only C entry epnn_<entry>"""
        cell = np.ascontiguousarray(cell, dtype=np.float32)
        if cell.shape != (3, 3):
            raise ValueError(f"{entry}: cell must have shape (3, 3), got {cell.shape}")
        out = np.empty((6,), dtype=np.float64)
        check(getattr(self.lib, "epnn_" + entry)(fptr(cell), float(alpha), float(tol), out.ctypes.data_as(C.POINTER(C.c_double))), self.lib)
        return out

    def coulomb_xyz_cell(self, offsets, xyz, x, Q, N, cell=None, box=None, ke=KE_EV_ANGSTROM, alpha=0.0, tol=1e-6, ewald=None, parts=False,
                         strain=False):
        """coulomb_xyz in fully periodic cells, by an Ewald sum (epnn_coulomb_xyz_cell): flat batch -> (q (A,), phi (A,), E (B,)
        float64 per cell, F (A, 3)); strain=True appends gstrain (B, 3, 3), the total dE/d eps under a homogeneous strain of
        coordinates and cell (the convention of charges_vjp_xyz(strain=True)).  cell (3, 3) or (B, 3, 3), or box (3,) or (B, 3)
        for its diagonal cell; every axis periodic.  phi includes the self term of the split and the neutralising background of
        a charged cell (include/epnn.h has the sum).  ewald (6,) or (B, 6) float64: the parameters beta, rc, kc, M0, M1, M2 the
        call runs at; None: ewald_params(cell, alpha, tol) per cell.  parts=True appends ffix and fq (F = ffix + fq) and, with
        strain=True, gstrain_fix and gstrain_q behind them (gstrain = gstrain_fix + gstrain_q); fq and gstrain_q are -gxyz and gs
        of charges_vjp_xyz(g=phi, cell=, strain=True) on "grad_path" 2, bit for bit.  Bonded exclusions: coulomb_xyz_cell_excl.
        Partially periodic cells and PME are not built."""
        return self._coulomb("coulomb_xyz_cell", offsets, xyz, x, Q, N, ke, alpha, parts, periodic=(cell, box, tol, ewald, strain))

    def coulomb_xyz_excl(self, offsets, xyz, x, Q, N, ke=KE_EV_ANGSTROM, alpha=0.0, parts=False, exclusions=None):
        """coulomb_xyz with bonded exclusions and pair scaling (epnn_coulomb_xyz_excl).  exclusions=None is coulomb_xyz itself, the
        plain entry; otherwise (pairs, scale): pairs an int array (P, 2) of flat atom indices, each unordered pair once, scale a
        scalar or (P,).  A listed pair counts with weight scale instead of 1 in phi, E and ffix (0 excludes, 0.5 or 0.8333 scales),
        and phi with these weights seeds fq.  bonded_exclusions(bonds, n_atoms) makes the list from a bond list.  The outputs do
        not depend on the order of the list; refused by name: an index out of range, i == j, atoms of two molecules, a pair listed
        twice, a factor that is not finite."""
        return self._coulomb("coulomb_xyz_excl", offsets, xyz, x, Q, N, ke, alpha, parts, exclusions=exclusions)

    def coulomb_xyz_cell_excl(self, offsets, xyz, x, Q, N, cell=None, box=None, ke=KE_EV_ANGSTROM, alpha=0.0, tol=1e-6, ewald=None, parts=False,
                              strain=False, exclusions=None):
        """coulomb_xyz_cell with bonded exclusions and pair scaling (epnn_coulomb_xyz_cell_excl).  exclusions=None is coulomb_xyz_cell
        itself; otherwise (pairs, scale) as in coulomb_xyz_excl.  The Ewald sum runs over all pairs and images as before; the one
        nearest image of every listed pair is corrected by (scale - 1) times its bare term, whatever beta, rc and kc are.  A listed
        pair farther apart than half the smallest perpendicular width of its cell is refused by name."""
        return self._coulomb("coulomb_xyz_cell_excl", offsets, xyz, x, Q, N, ke, alpha, parts, periodic=(cell, box, tol, ewald, strain),
                             exclusions=exclusions)

    def coulomb_xyz_site(self, offsets, xyz, x, Q, N, ke=KE_EV_ANGSTROM, alpha=0.0, sigma=None, chi=None, hardness=None, self_energy=True,
                         exclusions=None, parts=False):
        """The energy of a charge-model potential in one call (epnn_coulomb_xyz_site): coulomb_xyz_excl with per-atom Gaussian widths,
        the Gaussians' self-energy and on-site terms -> (q (A,), phi (A,), mu (A,), E (B,) float64, F (A, 3)),
            E = sum_i (chi_i q_i + 1/2 J_i q_i^2) + [self_energy] ke sum_i gamma_ii q_i^2 / sqrt(pi)
                + ke sum_{i<j} w_ij q_i q_j erf(gamma_ij D_ij) / D_ij,   gamma_ij = 1 / sqrt(2 (sigma_i^2 + sigma_j^2)),
        mu = dE/dq = chi + J q + phi, the seed of the part of F through dq/dxyz.  sigma, chi, hardness: float arrays (A,), one value
        per real atom (per_element makes them from a table by element), each may be None.  sigma=None: every pair uses alpha, as in
        coulomb_xyz; with sigma alpha must be 0 (equal widths sigma are alpha = 1 / (2 sigma)), and gamma_ii = 1 / (2 sigma_i), or alpha.
        chi and hardness are in the caller's energy units and are not multiplied by ke.  self_energy=True needs sigma or alpha > 0 (a
        point charge's self-energy is infinite).  exclusions = (pairs, scale) as in coulomb_xyz_excl, or None.  parts=True appends ffix
        and fq; fq is -gxyz of charges_vjp_xyz(g=mu) on "grad_path" 2, bit for bit.  With nothing given and self_energy=False the
        outputs have the bits of coulomb_xyz_excl and mu is phi."""
        return self._coulomb("coulomb_xyz_site", offsets, xyz, x, Q, N, ke, alpha, parts, exclusions=exclusions,
                             site=(sigma, chi, hardness, self_energy))

    def coulomb_xyz_cell_site(self, offsets, xyz, x, Q, N, cell=None, box=None, ke=KE_EV_ANGSTROM, alpha=0.0, tol=1e-6, ewald=None,
                              sigma=None, chi=None, hardness=None, self_energy=True, exclusions=None, parts=False, strain=False):
        """coulomb_xyz_site in fully periodic cells (epnn_coulomb_xyz_cell_site): the Ewald sum of coulomb_xyz_cell_excl with gamma_ij in
        its real-space term, the background of a charged cell worked out per pair, the self-energy and the on-site terms -> (q, phi,
        mu, E, F[, gstrain][, ffix, fq[, gstrain_fix, gstrain_q]]).  ewald=None: ewald_params(cell, alpha, tol) per cell (alpha is 0
        with sigma).  A cell whose widest Gaussian does not fit the split, sigma_max > 1 / (2 beta), is refused by name: a larger
        tol, or an ewald row with a smaller beta, moves the limit."""
        return self._coulomb("coulomb_xyz_cell_site", offsets, xyz, x, Q, N, ke, alpha, parts, periodic=(cell, box, tol, ewald, strain),
                             exclusions=exclusions, site=(sigma, chi, hardness, self_energy))

    def ewald_slab_params(self, cell, alpha=0.0, tol=1e-6):
        """The parameters coulomb_xyz_slab runs at for one slab cell (3, 3) with one row of zeros (epnn_ewald_slab_params, host only):
        float64 (6,) = beta, rc, kc, M0, M1, M2 by the rule of ewald_params over the two periodic rows; M of the open row is 0.
        Refuses three periodic rows (ewald_params), fewer than two, dependent rows, tol outside (0, 1) and k boxes above 2^16 slots."""
        return self._ewald_rule("ewald_slab_params", cell, alpha, tol)

    def coulomb_xyz_slab(self, offsets, xyz, x, Q, N, cell=None, box=None, ke=KE_EV_ANGSTROM, alpha=0.0, tol=1e-6, ewald=None, parts=False,
                         exclusions=None):
        """coulomb_xyz in slab cells, two periodic axes and one open one, by the exact two-dimensional Ewald sum
        (epnn_coulomb_xyz_slab): flat batch -> (q (A,), phi (A,), E (B,) float64 per cell, F (A, 3)).  cell (3, 3) or (B, 3, 3) with
        exactly one row of zeros, the open axis, or box (3,) or (B, 3) with exactly one zero.  phi includes the self term of the
        split; a charged slab (the model conserves Q, which need not be 0) gets the finite part of a charged sheet's potential and no
        neutralising background, which does not exist in two dimensions (include/epnn.h has the sum).  ewald (6,) or (B, 6) float64:
        the parameters the call runs at; None: ewald_slab_params(cell, alpha, tol) per cell.  parts=True appends ffix and fq
        (F = ffix + fq); fq is -gxyz of charges_vjp_xyz(g=phi, cell=) on "grad_path" 2, bit for bit.  exclusions = (pairs, scale) as
        in coulomb_xyz_excl: the nearest image of every listed pair counts with weight scale; None: no list.  The strain
        derivative: coulomb_xyz_slab_strain.  One periodic axis (wires) is not built."""
        _slab_box("coulomb_xyz_slab", box, cell)
        return self._coulomb("coulomb_xyz_slab", offsets, xyz, x, Q, N, ke, alpha, parts, periodic=(cell, box, tol, ewald, False),
                             exclusions=exclusions, slab=True)

    def coulomb_xyz_slab_strain(self, offsets, xyz, x, Q, N, cell=None, box=None, ke=KE_EV_ANGSTROM, alpha=0.0, tol=1e-6, ewald=None,
                                parts=False, exclusions=None):
        """coulomb_xyz_slab with the strain derivative of the slab sum (epnn_coulomb_xyz_slab_strain): (q, phi, E, F, gstrain), gstrain
        (B, 3, 3) the total dE/d eps under a homogeneous strain of coordinates and the two periodic rows (the convention of
        charges_vjp_xyz(strain=True); beta, rc, kc, the k slots and the in-range pairs held fixed).  parts=True appends ffix, fq,
        gstrain_fix and gstrain_q (gstrain = gstrain_fix + gstrain_q); gstrain_q is gs of charges_vjp_xyz(g=phi, cell=, strain=True)
        on "grad_path" 2, bit for bit.  q, phi, E, F, ffix and fq have the bits of coulomb_xyz_slab on the same arguments, which all
        mean what they mean there.  INTEGRATION.md, "Slabs", has the in-plane stress and the surface tension in terms of gstrain."""
        _slab_box("coulomb_xyz_slab_strain", box, cell)
        return self._coulomb("coulomb_xyz_slab_strain", offsets, xyz, x, Q, N, ke, alpha, parts, periodic=(cell, box, tol, ewald, True),
                             exclusions=exclusions, slab=True)

    def coulomb_xyz_slab_site(self, offsets, xyz, x, Q, N, cell=None, box=None, ke=KE_EV_ANGSTROM, alpha=0.0, tol=1e-6, ewald=None,
                              sigma=None, chi=None, hardness=None, self_energy=True, exclusions=None, parts=False, strain=False):
        """coulomb_xyz_site in slab cells (epnn_coulomb_xyz_slab_site, with strain=True epnn_coulomb_xyz_slab_strain_site): the exact
        two-dimensional Ewald sum of coulomb_xyz_slab with gamma_ij in its real-space term and in the listed pairs' term, the
        Gaussians' self-energy and the on-site terms -> (q, phi, mu, E, F[, gstrain][, ffix, fq[, gstrain_fix, gstrain_q]]).  No
        background term and no per-pair k = 0 correction, for charged slabs too: the Gaussians' sum differs from the point charges'
        by a short-ranged real-space sum alone.  ewald=None: ewald_slab_params(cell, alpha, tol) per cell (alpha is 0 with sigma).  A
        cell whose widest Gaussian does not fit the split, sigma_max > 1 / (2 beta), is refused by name.  fq and gstrain_q are -gxyz
        and gstrain of charges_vjp_xyz(g=mu, cell=, strain=True) on "grad_path" 2, bit for bit.  With nothing given and
        self_energy=False the outputs have the bits of coulomb_xyz_slab / coulomb_xyz_slab_strain and mu is phi."""
        where = "coulomb_xyz_slab_strain_site" if strain else "coulomb_xyz_slab_site"
        _slab_box(where, box, cell)
        return self._coulomb(where, offsets, xyz, x, Q, N, ke, alpha, parts, periodic=(cell, box, tol, ewald, bool(strain)),
                             exclusions=exclusions, slab=True, site=(sigma, chi, hardness, self_energy))

    def _coulomb(self, where, offsets, xyz, x, Q, N, ke, alpha, parts, periodic=None, exclusions=None, slab=False, site=None):
        """The coulomb_xyz* methods: where names the method in an error, periodic = (cell, box, tol, ewald, strain) or None for open
        molecules, exclusions = (pairs, scale) or None for the plain C entry (an _excl method without a list is its plain method).
        slab: the two slab entries, which always take a list (None: an empty one) and their own rule; the plain one has no strain
        rows, the other one is chosen by its name.  site = (sigma, chi, hardness, self_energy): the two _site entries, which always
        take a list too and return mu behind phi."""
        if exclusions is None:
            where = where.replace("_excl", "")
            if slab or site is not None:
                exclusions = (np.zeros((0, 2), dtype=np.int32), 1.0)
        strain = False
        if periodic is not None:
            cell, box, tol, ewald, strain = periodic
            _one_periodic_argument(box, cell)
            if box is None and cell is None:
                raise ValueError(f"{where}: give cell= or box= (open molecules: {where.replace('_cell', '')})")
        offsets, xyz, x, Q, _, B, A = self._flat_batch(where + ": array shapes do not match offsets", offsets, xyz, x, Q)
        dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
        opt = lambda a: None if a is None else fptr(a)
        args = [float(ke), float(alpha)]
        if site is not None:
            sigma, chi, hardness, self_energy = site
            rows = []
            for name, a in (("sigma", sigma), ("chi", chi), ("hardness", hardness)):
                if a is not None:
                    a = np.ascontiguousarray(a, dtype=np.float32)
                    if a.shape != (A,):
                        raise ValueError(f"{where}: {name} must have shape ({A},), one value per real atom, got {a.shape}")
                rows.append(a)
            if rows[0] is not None and float(alpha) > 0.0:
                raise ValueError(f"{where}: both sigma and alpha = {alpha} are given: per-atom widths take alpha = 0")
            if self_energy and rows[0] is None and not float(alpha) > 0.0:
                raise ValueError(f"{where}: self_energy=True with neither sigma nor alpha > 0: the self-energy of a point charge is infinite")
            args += [opt(rows[0]), opt(rows[1]), opt(rows[2]), 1 if self_energy else 0]
        if periodic is not None:
            _, cell = _geometry(box, cell, B, cells_only=True)
            if ewald is None:
                rule = self.ewald_slab_params if slab else self.ewald_params
                ewald = np.stack([rule(cell[b], alpha, tol) for b in range(B)])
            ewald = np.asarray(ewald, dtype=np.float64)
            if ewald.shape == (6,):
                ewald = np.tile(ewald, (B, 1))
            if ewald.shape != (B, 6):
                raise ValueError(f"{where}: ewald must have shape (6,) or ({B}, 6), got {ewald.shape}")
            ewald = np.ascontiguousarray(ewald)
            args = [fptr(cell), dptr(ewald)] + args
        if exclusions is not None:
            ei, ej, es = _exclusion_lists(where, exclusions)
            args += [len(es), iptr(ei), iptr(ej), fptr(es)]
        q = np.empty((A,), dtype=np.float32)
        phi = np.empty((A,), dtype=np.float32)
        E = np.empty((B,), dtype=np.float64)
        F = np.empty((A, 3), dtype=np.float32)
        ffix, fq = (np.empty((A, 3), dtype=np.float32) if parts else None for _ in range(2))
        outs = [fptr(q), fptr(phi), dptr(E), fptr(F), opt(ffix), opt(fq)]
        if periodic is not None and (strain or not slab):
            gs = np.empty((B, 3, 3), dtype=np.float32)
            gs_fix, gs_q = (np.empty((B, 3, 3), dtype=np.float32) if parts else None for _ in range(2))
            outs = outs[:4] + [fptr(gs)] + outs[4:] + [opt(gs_fix), opt(gs_q)]
        if site is not None:
            mu = np.empty((A,), dtype=np.float32)
            outs = outs[:2] + [fptr(mu)] + outs[2:]
        check(getattr(self.lib, "epnn_" + where)(self.h, B, int(N), iptr(offsets), fptr(xyz), fptr(x), fptr(Q), *args, *outs), self.lib)
        out = (q, phi) + ((mu,) if site is not None else ()) + (E, F) + ((gs,) if strain else ())
        if parts:
            out += (ffix, fq) + ((gs_fix, gs_q) if strain else ())
        return out

    def get_gradients(self):
        g = np.empty((self.param_count(),), dtype=np.float32)
        check(self.lib.epnn_get_gradients(self.h, fptr(g), g.size), self.lib)
        return g

    def set_gradients(self, g):
        g = _f32(g)
        check(self.lib.epnn_set_gradients(self.h, fptr(g), g.size), self.lib)

    def train_apply(self):
        check(self.lib.epnn_train_apply(self.h), self.lib)

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == 128
        check(self.lib.epnn_comm_init(self.h, unique_id, rank, world), self.lib)

    def debug_pairs(self, cap):
        """(pi, pj, near weight) of the pair list the last forward built outside the fused kernel (tests)"""
        pi, pj, w = np.zeros(cap, np.int32), np.zeros(cap, np.int32), np.zeros(cap, np.float32)
        n = C.c_int64(0)
        check(self.lib.epnn_debug_pairs(self.h, iptr(pi), iptr(pj), fptr(w), cap, C.byref(n)), self.lib)
        k = min(int(n.value), cap)
        return pi[:k], pj[:k], w[:k], int(n.value)

    def comm_count(self):
        """ranks that joined this engine's RCCL communicator"""
        n = C.c_int32(0)
        check(self.lib.epnn_comm_count(self.h, C.byref(n)), self.lib)
        return int(n.value)

    def comm_allreduce(self, values, op="sum"):
        """all-reduce of a few host doubles over the engine's RCCL communicator (barrier / MAX over ranks of a driver)"""
        buf = (C.c_double * len(values))(*[float(v) for v in values])
        check(self.lib.epnn_comm_allreduce(self.h, buf, len(values), {"sum": 0, "max": 1}[op]), self.lib)
        return [float(v) for v in buf]

    @staticmethod
    def comm_unique_id():
        lib = _lib.load()
        buf = C.create_string_buffer(128)
        check(lib.epnn_comm_unique_id(buf), lib)
        return buf.raw

    # ------------------------------------------------------------------ device-resident plumbing
    def alloc(self, nbytes):
        return DeviceArray(self, nbytes)

    def to_device(self, arr):
        arr = np.ascontiguousarray(arr)
        return DeviceArray(self, arr.nbytes).upload(arr)

    def set_partition(self, rank, world, exchange=None):
        """One large system on `world` processes: this engine computes the all-pairs sums of its own
        rows of atoms and `exchange(d_rows_ptr, row_len, n_rows, row_lo, row_hi) -> None` completes the others' after
        every GNN step (shard.make_row_exchange builds one on torch.distributed).  With exchange=None and world > 1 the
        engine's RCCL communicator (comm_init with the same rank / world) exchanges the rows on the engine's stream -- the
        multi-GPU form, no host synchronisation inside the forward.  world = 1 switches the partition off."""
        if world > 1 and exchange is not None:

            def _cb(ctx, d_rows, row_len, n_rows, row_lo, row_hi):
                try:
                    exchange(d_rows, row_len, n_rows, row_lo, row_hi)
                    return 0
                except Exception:                           # an exception must not cross the C frames: report it here,
                    import traceback                        # the forward then fails with the library's own message
                    traceback.print_exc()
                    return 1

            self._exchange_cb = _lib.EXCHANGE_FN(_cb)       # keep the thunk alive as long as the handle uses it
            fn = C.cast(self._exchange_cb, C.c_void_p)
        else:
            self._exchange_cb = None
            fn = None
        check(self.lib.epnn_set_partition(self.h, int(rank), int(world), fn, None), self.lib)

    def copy_rows_to_host(self, d_ptr, row_len, row_lo, row_hi):
        """rows [row_lo, row_hi) of a device array [..][row_len] float32 -> NumPy (used by exchange functions)."""
        out = np.empty((row_hi - row_lo, row_len), dtype=np.float32)
        if out.size:
            check(self.lib.epnn_memcpy_d2h(self.h, out.ctypes.data_as(C.c_void_p), C.c_void_p(d_ptr + 4 * row_len * row_lo),
                                           out.nbytes), self.lib)
        return out

    def copy_rows_to_device(self, d_ptr, row_len, row_lo, rows):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        if rows.size:
            check(self.lib.epnn_memcpy_h2d(self.h, C.c_void_p(d_ptr + 4 * row_len * row_lo), rows.ctypes.data_as(C.c_void_p),
                                           rows.nbytes), self.lib)

    def forward_xyz_dev(self, offsets, d_xyz, d_x, d_Q, d_q, N, box=None, cell=None):
        _one_periodic_argument(box, cell)
        offsets = np.ascontiguousarray(offsets, dtype=np.int32)
        B = len(offsets) - 1
        if box is None and cell is None:                           # (a trajectory's or a benchmark's loop: nothing else per call)
            check(self.lib.epnn_forward_xyz_dev(self.h, B, int(N), iptr(offsets), d_xyz.ptr, d_x.ptr, d_Q.ptr, d_q.ptr), self.lib)
            return
        suffix, rows = _geometry(box, cell, B)
        check(getattr(self.lib, "epnn_forward_xyz" + suffix + "_dev")(self.h, B, int(N), iptr(offsets), d_xyz.ptr, d_x.ptr, d_Q.ptr,
                                                                     fptr(rows), d_q.ptr), self.lib)

    def sync(self):
        check(self.lib.epnn_sync(self.h), self.lib)

    def timer_begin(self):
        check(self.lib.epnn_timer_begin(self.h), self.lib)

    def timer_end(self):
        ms = C.c_float()
        check(self.lib.epnn_timer_end(self.h, C.byref(ms)), self.lib)
        return ms.value

    def set_option(self, name, value):
        check(self.lib.epnn_set_option(self.h, name.encode(), int(value)), self.lib)

    def last_timing(self):
        out = np.zeros(4, dtype=np.float32)
        check(self.lib.epnn_last_timing(self.h, fptr(out)), self.lib)
        return out

    def timing_at(self, idx):
        out = np.zeros(4, dtype=np.float32)
        check(self.lib.epnn_timing_at(self.h, int(idx), fptr(out)), self.lib)
        return out

    def stream_class(self):
        """(class, priority) of the handle's stream: class 0 normal, 1 high, 2 low -- where epnn_create placed it so that handles
        used side by side get a hardware queue each (include/epnn.h) --, priority as the HIP runtime reports it."""
        cls, prio = C.c_int(), C.c_int()
        check(self.lib.epnn_stream_class(self.h, C.byref(cls), C.byref(prio)), self.lib)
        return cls.value, prio.value

    def last_stats(self):
        out = np.zeros(4, dtype=np.int64)
        check(self.lib.epnn_last_stats(self.h, out.ctypes.data_as(C.POINTER(C.c_int64))), self.lib)
        return out


def reserve_null_stream(device=0, on=True):
    """Say that this process uses the null (default) stream of `device` -- PyTorch work on its default stream, hipMemcpy, a launch
    without a stream: the runtime then holds one normal hardware queue for it, and the handles created AFTERWARDS leave that place
    free (include/epnn.h, epnn_reserve_null_stream; the same as EPNN_NULL_STREAM_PLACE=1 in the environment).  No HIP call."""
    lib = _lib.load()
    check(lib.epnn_reserve_null_stream(int(device), 1 if on else 0), lib)


class Pipeline:
    """Keeps `depth` batches in flight on one GPU: `depth` handles (each with its own HIP stream and workspace) take
    the calls round robin.  The fused kernel runs one wavefront per molecule and an MI355X holds 2048 of them
    (8 per CU), so one batch of 1024 molecules fills half the machine and its largest molecules finish long after
    the smallest: the wavefronts of the next batches fill those slots.  A launch lasts as long as its largest molecule
    (~3x the mean under load), so six to ten batches in flight keep every slot busy (default 8); each needs its own hardware queue
    (GPU_MAX_HW_QUEUES, raised to 16 in _lib.load() unless the caller set it).  Where the caller did set it, to fewer queues than
    lanes, the library spreads the lanes' streams over the runtime's stream priority classes, each of which has that many queues of
    its own (include/epnn.h at epnn_create, `Engine.stream_class()`, switch EPNN_STREAM_CLASSES=0).  A
    pipeline keeps one place of the normal class for the process's null stream unless it is told otherwise (`null_stream_place`
    below): with 4, eight lanes are 3 normal + 4 high + 1 low, fourteen 3 + 4 + 4 and three that share -- the placement that was
    measured (profiles/r11_lane_queues.txt) and that tests/test_gpu_stream_classes.py holds a pipeline to.  The library itself
    never uses the null stream, so a process that does not either can give the pipeline every normal queue: `null_stream_place=0`
    or EPNN_NULL_STREAM_PLACE=0 make it 4 normal + 4 high, and 4 + 4 + 4 and two that share.
    A process that shares its GPU with other jobs should set the switch: queue priority counts across processes.
    Lanes of different classes are served in priority
    order, so lanes may finish in another order than they were called; `map` collects in call order and results do not change.
    All handles carry the same weights.  Results of call k are complete after `sync()`."""

    def __init__(self, depth=8, queue_stride=None, null_stream_place=None, **engine_kwargs):
        """queue_stride: hardware queues from one lane's to the next (the HIP runtime deals streams onto its hardware queues in
        creation order).  Measured on MI355X: up to eight lanes run 3 % faster on every other queue (stride 2, the default there);
        more lanes than that need every queue (stride 1).
        null_stream_place: 1 keeps one normal hardware queue free for the process's null stream, 0 does not (`reserve_null_stream`:
        it holds for the device from here on).  None: what EPNN_NULL_STREAM_PLACE says; without the variable, 1."""
        depth = max(1, int(depth))
        if null_stream_place is None and os.environ.get("EPNN_NULL_STREAM_PLACE") is None:
            null_stream_place = 1
        if null_stream_place is not None:
            reserve_null_stream(int(engine_kwargs.get("device", 0)), bool(null_stream_place))
        if queue_stride is None:
            # every other queue only while the lanes still get a queue each: with a user-set GPU_MAX_HW_QUEUES of 4 or 8 a stride of
            # 2 would fold eight lanes onto 2 or 4 queues (kernels of streams that share a queue serialise)
            _lib.load()                                       # (sets GPU_MAX_HW_QUEUES to 16 unless the caller decided otherwise)
            try:
                queues = int(os.environ.get("GPU_MAX_HW_QUEUES", "4"))
            except ValueError:
                queues = 4
            queue_stride = 2 if depth <= 8 and 2 * depth <= queues else 1
        self.engines = []
        self._device = int(engine_kwargs.get("device", 0))
        self._skipped = False
        for k in range(depth):
            self.engines.append(Engine(**engine_kwargs))
            if queue_stride > 1 and k + 1 < depth:
                # (the placement is defined for the first pipeline of a process: later streams land where the runtime's round robin is)
                check(self.engines[0].lib.epnn_skip_hw_queues(self._device, int(queue_stride) - 1), self.engines[0].lib)
                self._skipped = True
        self._next = 0
        if len(self.engines) > 1:
            # batches side by side fill the GPU: every molecule on one wavefront (the split over two is for a lone batch)
            self.set_option("wave2", 0)

    def set_weights(self, weights):
        for e in self.engines:
            e.set_weights(weights)

    def set_option(self, name, value):
        for e in self.engines:
            e.set_option(name, value)

    def lane(self):
        e = self.engines[self._next % len(self.engines)]
        self._next += 1
        return e

    def map(self, batches, N, workers=None):
        """Charges of every batch of `batches` (an iterable of (offsets, xyz, x, Q) host arrays), in order, with up to
        `depth` batches in flight: while the GPU works on some, the host stages the next and collects the oldest.
        workers: host threads that run the first half of a call (the batch's plan, its copy into page-locked staging and the
        queueing: ~85 us for 1024 molecules, what bounds this entry, not the GPU) while this thread collects results -- the C
        entry points release the GIL and every lane is a handle of its own.  Measured on the bench batch (MI355X box, 16 cores):
        inline 184-186 M atoms/s, one worker 209-218 M, two or more no better than one (the first halves of different lanes
        do not overlap: the HIP runtime's copies and launches serialise).  Default 1 with more than one lane; 0 = everything on
        the calling thread.
        The arrays of a batch: `map` is done with them when it asks `batches` for the next item (or ends it), as
        `forward_xyz_begin` is when it returns -- a loader may refill one set of buffers in place for every batch.  (With workers the
        first half runs later, on another thread: the calling thread takes its own copy of the four arrays first.  That costs: on
        tools/bench_e2e.py's map line, 15 passes per process, medians of 127-176 M atoms/s against 202-248 M for the map that did not
        copy and returned wrong charges to such a loader; holding the loader back until each first half has returned instead gave
        131-167 M: profiles/r22_pipeline_contract.txt.)
        Errors: the first one in call order reaches the caller, as raised (a batch whose arrays do not convert, a failed first or
        second half, the loader's own); whatever else is in flight is collected first, its errors dropped, so that every lane takes
        the next call.  The same holds when the caller stops iterating."""
        if workers is None:
            workers = 1 if len(self.engines) > 1 else 0
        if workers <= 0:
            yield from self._map_inline(batches, N)
            return
        from concurrent.futures import ThreadPoolExecutor
        busy = []                                   # (engine, future of its forward_xyz_begin), oldest first
        pool = ThreadPoolExecutor(max_workers=int(workers))
        taking = False                              # an error now is the loader's or the new batch's: behind all that is in flight
        try:
            batches = iter(batches)
            while True:
                taking = True
                try:
                    offsets, xyz, x, Q = next(batches)
                except StopIteration:
                    break
                # the worker reads the arrays after the loader has been asked for the next batch: its own copies
                offsets = np.array(offsets, dtype=np.int32, order="C")
                xyz, x, Q = (np.array(a, dtype=np.float32, order="C") for a in (xyz, x, Q))
                taking = False
                e = self.lane()
                if busy and busy[0][0] is e:        # the lane's previous forward is collected before it takes the next
                    e0, f0 = busy.pop(0)
                    f0.result()
                    yield e0.forward_xyz_end()
                busy.append((e, pool.submit(e.forward_xyz_begin, offsets, xyz, x, Q, N)))
            taking = False
            while busy:
                e0, f0 = busy.pop(0)
                f0.result()
                yield e0.forward_xyz_end()
        except Exception:
            first = self._collect(busy)
            if taking and first is not None:
                raise first
            raise
        finally:                                    # (the caller stopped iterating)
            self._collect(busy)
            pool.shutdown(wait=True)

    @staticmethod
    def _collect(busy):
        """Abandoned half way (error, or the caller stopped iterating): collect what is in flight, oldest first, so that the engines can
        be used again -> the first error met.  A lane whose first half failed has begun nothing: no second half for it."""
        first = None
        while busy:
            e0, f0 = busy.pop(0)
            try:
                f0.result()
                e0.forward_xyz_end()
            except Exception as err:
                if first is None:
                    first = err
        return first

    def _map_inline(self, batches, N):
        busy = []                                   # engines with a begun forward, oldest first
        try:
            for offsets, xyz, x, Q in batches:
                e = self.lane()
                if busy and busy[0] is e:
                    yield busy.pop(0).forward_xyz_end()
                e.forward_xyz_begin(offsets, xyz, x, Q, N)     # (done with the arrays when it returns; a failed one has begun nothing)
                busy.append(e)
            while busy:
                yield busy.pop(0).forward_xyz_end()
        finally:
            while busy:                             # abandoned half way (error, or the caller stopped iterating): collect what is in
                try:                                # flight so that the engines can be used again; the error under way is the one kept
                    busy.pop(0).forward_xyz_end()
                except Exception:
                    pass

    def sync(self):
        for e in self.engines:
            e.sync()

    def close(self):
        lib = self.engines[0].lib if self.engines else None
        for e in self.engines:
            e.close()
        if self._skipped and lib is not None:
            lib.epnn_skip_hw_queues(self._device, 0)          # the placeholder streams between the lanes
            self._skipped = False
