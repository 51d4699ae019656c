"""The float32 pre-test of the general-cell front-end (front_scan_row with PBC = 2, constants from check_cell) run in NumPy with
the kernel's arithmetic, against the float64 rule of tests/cell_ref.py: it must never reject a pair the float64 test accepts --
for the cells of the GPU tests, cells at the width limit, long thin cells, tilted slabs and wires, atoms many cells outside the
cell and far out along open directions.  An emulation: it pins the derivation down, the kernel itself runs in test_gpu_cell.py.
CPU only."""
import numpy as np
import pytest

import cell_ref as cr

f32 = np.float32
U = 2.0 ** -24
SKIP = f32(1e30)


def constants(cell, cutoff=3.0):
    """check_cell: (pre_ext, pre_eps, pre_margin)"""
    a, g = cr.duals(cell)
    per = [k for k in range(3) if np.any(a[k] != 0)]
    S = sum(np.sqrt((a[k] ** 2).sum()) for k in per)
    X = S + (1024.0 if len(per) < 3 else 0.0)
    r = U * X / cutoff
    wmin = min((cr.widths(cell)[k] for k in per), default=1.0)
    eps = f32(min(0.5, 32.0 * U * X / wmin * 1.000001)) if per else f32(0)
    return f32(X), eps, f32((1.0001 + r * (96.0 + 1024.0 * r)) * 1.000001)


def pretest(cell, xyz, cutoff=3.0):
    """(passed (n, n) bool, untested (n, n) bool): the kernel's decision for every ordered pair."""
    a, g = cr.duals(cell)
    ext, eps, margin = constants(cell, cutoff)
    r = np.asarray(xyz, f32).astype(np.float64)
    w = (r - np.floor(r @ g.T) @ a).astype(f32)                                 # epnn_wrap_cell
    skip = np.abs(w).max(1) > ext
    w[skip, 0] = SKIP
    gf, af = g.astype(f32), a.astype(f32)
    with np.errstate(over="ignore", invalid="ignore"):
        f = w[None, :, :] - w[:, None, :]
        p = [(gf[k, 0] * f[..., 0] + gf[k, 1] * f[..., 1] + gf[k, 2] * f[..., 2]).astype(f32) for k in range(3)]
        n = [np.rint(pk) for pk in p]
        frac = np.maximum(np.abs(p[0] - n[0]), np.maximum(np.abs(p[1] - n[1]), np.abs(p[2] - n[2])))
        untested = ~(frac < (f32(0.5) - eps)) | (np.maximum(np.abs(w[None, :, 0]), np.abs(w[:, None, 0])) > f32(0.5) * SKIP)
        fp = [(f[..., c] - n[0] * af[0, c] - n[1] * af[1, c] - n[2] * af[2, c]).astype(f32) for c in range(3)]
        d2 = (fp[0] * fp[0] + fp[1] * fp[1] + fp[2] * fp[2]).astype(f32)
        passed = untested | (d2 < f32(cutoff * cutoff * float(margin)))
    return passed, untested


CELLS = {"sheared": cr.SHEARED, "hex120": cr.HEX120, "hex60": cr.HEX60, "rhomb": cr.RHOMB, "slab": cr.HEX_SLAB, "wire": cr.WIRE,
         "basis_a": cr.BASIS_A, "basis_b": cr.BASIS_B, "open": np.zeros((3, 3), f32), "cubic6": np.diag(f32([6, 6, 6])),
         "limit": f32([[6.9283, 0, 0], [-3.46415, 6.0001, 0], [0, 0, 6]]),                    # widths 6.0001, 6.0001, 6
         "long": f32([[900, 0, 0], [400, 6.0, 0], [0, 0, 6.0]]), "big": f32([[100, 0, 0], [30, 100, 0], [-20, 25, 100]]),
         "tilted_wire": f32([[0, 0, 0], [2.1, 1.3, 6.7], [0, 0, 0]]), "tilted_slab": f32([[7.7, 0, 1.3], [3.7, 6.9, -2.1], [0, 0, 0]])}


def _atoms(rng, cell, n, cells_out, open_offset):
    """n atoms dense enough for many pairs: fractional coordinates over `cells_out` cells around a few centres, open directions
    (the complement of the periodic rows) spread over 6 A around `open_offset`."""
    a, _ = cr.duals(cell)
    per = [k for k in range(3) if np.any(a[k] != 0)]
    q, _ = np.linalg.qr(np.concatenate([a[per], np.eye(3)]).T)                   # orthonormal: span of the periodic rows first
    open_dirs = q[:, len(per):3].T
    frac = rng.uniform(0, 1, (n, len(per))) * (0.3 if cell is CELLS["big"] or cell is CELLS["long"] else 1.0)
    frac = frac + rng.integers(-cells_out, cells_out + 1, (n, len(per)))
    r = frac @ a[per] if per else np.zeros((n, 3))
    if len(open_dirs):
        r = r + (open_offset + rng.uniform(0, 6, (n, len(open_dirs)))) @ open_dirs
    return r.astype(f32)


@pytest.mark.parametrize("name", sorted(CELLS))
@pytest.mark.parametrize("cells_out,open_offset", [(0, 0.0), (3, 0.0), (40, 500.0), (3, 3000.0), (3, 2e4), (3, 1e5)])
def test_pretest_never_rejects_an_accepted_pair(name, cells_out, open_offset):
    cell = CELLS[name]
    if cr.widths(cell).min() < 6.0:
        pytest.fail("not a valid cell")
    rng = np.random.default_rng(7)
    xyz = _atoms(rng, cell, 700, cells_out, open_offset)
    r = xyz.astype(np.float64)
    D = cr._dist(cr.mic(r[None] - r[:, None], cell))
    np.fill_diagonal(D, 9.0)
    accepted = D < 3.0
    assert accepted.sum() > 1000
    passed, untested = pretest(cell, xyz)
    assert not (accepted & ~passed).any(), int((accepted & ~passed).sum())
    if open_offset <= 500.0 and name not in ("long",):
        # ... and it still is a test: few candidates reach the float64 evaluation that it does not accept
        assert (passed & ~accepted).sum() - len(xyz) <= 0.05 * accepted.sum() + 0.001 * passed.size
