"""General (triclinic) cells on the GPU (epnn_forward_xyz_cell[_dev], epnn_charges_vjp_xyz_cell, epnn_edges_cell) against the
float64 reference of tests/cell_ref.py, test for test what tests/test_gpu_periodic.py does for orthorhombic boxes, with its
tolerances: diagonal cells give the bits of the box entries, small general cells on every route, a rotated orthorhombic cell,
large sheared cells' pair lists and charges, invariances, mixed batches, the device-resident entry, dq/dxyz and the strain
derivative, the dense route, a partitioned handle and the error paths.  GPU only."""
import os

import numpy as np
import pytest

from conftest import load_molecules, random_weights
import cell_ref as cr
import periodic_ref as pr

pytestmark = pytest.mark.gpu

TOL = 1e-5

GENERAL = {"sheared": cr.SHEARED, "hex120": cr.HEX120, "hex60": cr.HEX60, "rhomb": cr.RHOMB, "slab": cr.HEX_SLAB, "wire": cr.WIRE}


def _features(rng, n):
    x = np.zeros((n, 9), np.float32)
    el = rng.integers(0, 4, n)
    x[:, 0] = np.array([1, 6, 7, 8])[el]
    x[np.arange(n), 1 + el] = 1
    return x


def _cell(seed, n, cell):
    rng = np.random.default_rng(seed)
    xyz = cr.random_cell(rng, n, cell)
    return xyz, _features(rng, n)


def _box_cell(seed, n, L):
    """the cells of tests/test_gpu_periodic.py"""
    rng = np.random.default_rng(seed)
    xyz = pr.random_cell(rng, n, L)
    return xyz, _features(rng, n)


def _batch(mols):
    offsets = np.zeros(len(mols) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([m[0].shape[0] for m in mols])
    return offsets, np.concatenate([m[0] for m in mols]), np.concatenate([m[1] for m in mols])


def _pair_set(eng, cap):
    pi, pj, w, n = eng.debug_pairs(cap)
    assert n <= cap
    o = np.lexsort((pj, pi))
    return pi[o], pj[o], w[o]


# ------------------------------------------------------------------------------------------------ 1. diagonal and all-zero cells
def test_zero_cells_give_the_bits_of_the_open_entries(gpu_engine_factory, weights_decay, val_dir, val_names, val_gold):
    """All-zero cells on the 871 validation molecules at N = 41: the bits of forward_xyz with "wave_front" 0 and of all-zero boxes,
    the stored TensorFlow charges to 1e-5; charges_vjp_xyz with zero cells the bits of charges_vjp_xyz on a subset."""
    mols, offsets, xyz, x, Q = load_molecules(val_dir, val_names)
    eng = gpu_engine_factory(nx=9, T=5)
    eng.set_weights(weights_decay)
    q = eng.forward_xyz(offsets, xyz, x, Q, 41, cell=np.zeros((3, 3), np.float32))
    assert np.array_equal(q, eng.forward_xyz(offsets, xyz, x, Q, 41, box=np.zeros(3, np.float32)))
    eng.set_option("wave_front", 0)
    assert np.array_equal(q, eng.forward_xyz(offsets, xyz, x, Q, 41))
    eng.set_option("wave_front", 1)
    for b, m in enumerate(mols):
        n = m[1].shape[0]
        assert np.abs(q[offsets[b]:offsets[b + 1]] - val_gold[b, :n]).max() <= TOL
    sub = offsets[:41]
    A = int(sub[-1])
    g = np.random.default_rng(0).normal(size=A).astype(np.float32)
    q0, g0 = eng.charges_vjp_xyz(sub, xyz[:A], x[:A], Q[:40], g, 41)
    q1, g1 = eng.charges_vjp_xyz(sub, xyz[:A], x[:A], Q[:40], g, 41, cell=np.zeros((40, 3, 3), np.float32))
    assert np.array_equal(q0, q1) and np.array_equal(g0, g1)


@pytest.mark.parametrize("N,ns,L", [(32, [4, 9, 17, 32], [6.0, 6.0, 6.0]), (40, [33, 24, 7], [7.5, 9.0, 12.0]),
                                    (64, [64, 50], [8.0, 9.5, 8.5]), (96, [96, 70], [10.0, 10.5, 11.0]),
                                    (24, [20, 12], [6.5, 0.0, 7.0]), (24, [18, 10], [0.0, 0.0, 6.0])])
def test_diagonal_cells_give_the_bits_of_the_box_entries(gpu_engine_factory, N, ns, L):
    """The cells of test_small_cells_on_every_route, slabs and wires included, as cell=diag(L): forward, gxyz and edges_ex
    bit for bit what box=L gives."""
    w = random_weights(9, 3, seed=7, scale=0.35)
    mols = [_box_cell(100 * N + k, n, L) for k, n in enumerate(ns)]
    offsets, xyz, x = _batch(mols)
    Q = np.array([(-1, 0, 2)[k % 3] for k in range(len(ns))], np.float32)
    eng = gpu_engine_factory(nx=9, T=3)
    eng.set_weights(w)
    L = np.float32(L)
    cell = np.diag(L)
    assert np.array_equal(eng.forward_xyz(offsets, xyz, x, Q, N, cell=cell), eng.forward_xyz(offsets, xyz, x, Q, N, box=L))
    g = np.random.default_rng(1).normal(size=int(offsets[-1])).astype(np.float32)
    q0, g0 = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, box=L)
    q1, g1 = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, cell=cell)
    assert np.array_equal(q0, q1) and np.array_equal(g0, g1)
    e0, C0 = eng.edges_ex(mols[0][0], 48, box=L)
    e1, C1 = eng.edges_ex(mols[0][0], 48, cell=cell)
    assert np.array_equal(e0, e1) and np.array_equal(C0, C1)


def test_diagonal_cell_of_a_large_system_gives_the_bits_of_the_box_entry(gpu_engine_factory):
    """The tiled route and the staged float32 pre-test: the 1500-atom cubic cell as a cell, front_bits 1 and 0."""
    from epnn_amd import synth
    offsets, xyz, x, Q, N, box = synth.periodic_box_system(1500, seed=11)
    eng = gpu_engine_factory(nx=9, T=2)
    eng.set_weights(random_weights(9, 2, seed=2, scale=0.35))
    for bits in (1, 0):
        eng.set_option("front_bits", bits)
        q0 = eng.forward_xyz(offsets, xyz, x, Q, N, box=box)
        p0 = _pair_set(eng, 8 * 1500)
        q1 = eng.forward_xyz(offsets, xyz, x, Q, N, cell=np.diag(box[0]))
        p1 = _pair_set(eng, 8 * 1500)
        assert np.array_equal(q0, q1)
        assert all(np.array_equal(a, b) for a, b in zip(p0, p1))


# ------------------------------------------------------------------------------------------------ 2. small general cells
@pytest.mark.parametrize("name", sorted(GENERAL))
@pytest.mark.parametrize("N,ns", [(32, [4, 9, 17, 32]), (40, [33, 24, 7]), (64, [64, 50]), (96, [96, 70])])
def test_small_general_cells_on_every_route(gpu_engine_factory, name, N, ns):
    """Cells of 4..96 atoms (the fused kernel on the front-end's list up to 32 atoms, the tiled kernels above), a live GNN, Q in
    {-1, 0, 2}, N > n: the float64 reference within max(TOL, 3 x the float32 reference's own noise); total charge conserved."""
    cell = GENERAL[name]
    w = random_weights(9, 3, seed=7, scale=0.35)
    mols = [_cell(100 * N + k, n, cell) for k, n in enumerate(ns)]
    offsets, xyz, x = _batch(mols)
    Q = np.array([(-1, 0, 2)[k % 3] for k in range(len(ns))], np.float32)
    eng = gpu_engine_factory(nx=9, T=3)
    eng.set_weights(w)
    q = eng.forward_xyz(offsets, xyz, x, Q, N, cell=cell)
    crossing = 0
    for b, (mx, mxx) in enumerate(mols):
        a0, a1 = offsets[b], offsets[b + 1]
        ref = cr.forward_cell(mx, mxx, Q[b], cell, w, N, np.float64)[:a1 - a0]
        ref32 = cr.forward_cell(mx, mxx, Q[b], cell, w, N, np.float32)[:a1 - a0]
        tol = max(TOL, 3 * float(np.abs(ref32 - ref).max()))
        assert np.abs(q[a0:a1] - ref).max() <= tol, (b, float(np.abs(q[a0:a1] - ref).max()), tol)
        assert abs(float(q[a0:a1].sum(dtype=np.float64)) - float(Q[b])) < 5e-5
        r = mx.astype(np.float64)
        crossing += int(((cr._dist(cr.mic(r[None] - r[:, None], cell)) < 3.0) & (np.sqrt(((r[None] - r[:, None]) ** 2).sum(-1)) >= 3.0)).sum())
    assert crossing > 0                                           # pairs that exist only through the cell


# ------------------------------------------------------------------------------------------------ 3. a rotated orthorhombic cell
def test_rotated_orthorhombic_cell(gpu_engine_factory):
    """Cell rows and coordinates rotated in float64, then rounded to float32: the reference on those inputs within TOL; the
    distance from the box run of the unrotated system is at most what the float64 reference shows between the two inputs (the
    rounding of the rotated coordinates) plus 2 TOL."""
    w = random_weights(9, 3, seed=7, scale=0.35)
    L = np.float32([8.0, 9.5, 8.5])
    ns = [64, 50, 20]
    mols = [_box_cell(900 + k, n, L) for k, n in enumerate(ns)]
    R, _ = np.linalg.qr(np.random.default_rng(5).normal(size=(3, 3)))
    cell = (np.diag(L.astype(np.float64)) @ R.T).astype(np.float32)
    rot = [((m[0].astype(np.float64) @ R.T).astype(np.float32), m[1]) for m in mols]
    offsets, xyz, x = _batch(mols)
    _, rxyz, _ = _batch(rot)
    Q = np.float32([0, 1, -1])
    eng = gpu_engine_factory(nx=9, T=3)
    eng.set_weights(w)
    q_box = eng.forward_xyz(offsets, xyz, x, Q, 64, box=L)
    q_rot = eng.forward_xyz(offsets, rxyz, x, Q, 64, cell=cell)
    for b in range(3):
        a0, a1 = offsets[b], offsets[b + 1]
        ref_rot = cr.forward_cell(rot[b][0], rot[b][1], Q[b], cell, w, 64)[:a1 - a0]
        ref_box = pr.forward_pbc(mols[b][0], mols[b][1], Q[b], L, w, 64)[:a1 - a0]
        assert np.abs(q_rot[a0:a1] - ref_rot).max() <= TOL
        assert np.abs(q_rot[a0:a1] - q_box[a0:a1]).max() <= np.abs(ref_rot - ref_box).max() + 2 * TOL


# ------------------------------------------------------------------------------------------------ 4, 5. large sheared cells
@pytest.mark.parametrize("n_atoms,bits", [(1500, 1), (1500, 0), (20000, 1)])
def test_large_cell_pair_lists(gpu_engine_factory, n_atoms, bits):
    """The device pair list of a sheared cell equals the host's float64 pairs exactly, near flags included (1500 atoms: the
    front_bits walk and, with front_bits 0, the second scan; 20 000 atoms: a full second scan)."""
    from epnn_amd import synth
    offsets, xyz, x, Q, N, cell = synth.triclinic_cell_system(n_atoms, seed=11)
    eng = gpu_engine_factory(nx=9, T=1)
    eng.set_weights(random_weights(9, 1, seed=2, scale=0.35))
    eng.set_option("front_bits", bits)
    eng.forward_xyz(offsets, xyz, x, Q, N, cell=cell)
    I, J, W = cr.pairs_cell(xyz, cell[0])
    pi, pj, w = _pair_set(eng, 8 * n_atoms)
    assert np.array_equal(pi, I) and np.array_equal(pj, J)
    assert np.array_equal(w, W.astype(np.float32))
    assert 10.5 < 2 * len(I) / n_atoms < 12.0


def test_large_cell_charges(gpu_engine_factory):
    """1500-atom sheared cell, T = 1: the blocked float64 reference; front_bits 0 gives the same bits."""
    from epnn_amd import synth
    offsets, xyz, x, Q, N, cell = synth.triclinic_cell_system(1500, seed=11)
    w = random_weights(9, 1, seed=2, scale=0.35)
    eng = gpu_engine_factory(nx=9, T=1)
    eng.set_weights(w)
    q = eng.forward_xyz(offsets, xyz, x, Q, N, cell=cell)
    eng.set_option("front_bits", 0)
    assert np.array_equal(q, eng.forward_xyz(offsets, xyz, x, Q, N, cell=cell))
    ref = cr.forward_large_cell(xyz, x, Q[0], cell[0], w)
    assert np.abs(q - ref).max() <= 2e-5, float(np.abs(q - ref).max())


# ------------------------------------------------------------------------------------------------ 6. invariances
def test_translation_and_lattice_shift_invariance(gpu_engine_factory):
    from epnn_amd import synth
    offsets, xyz, x, Q, N, cell = synth.triclinic_cell_system(1500, seed=12)
    eng = gpu_engine_factory(nx=9, T=2)
    eng.set_weights(random_weights(9, 2, seed=3, scale=0.35))
    q0 = eng.forward_xyz(offsets, xyz, x, Q, N, cell=cell)
    p0 = _pair_set(eng, 8 * 1500)
    rng = np.random.default_rng(4)
    moved = [(xyz + np.float32([1.7, -3.2, 5.9])).astype(np.float32)]
    w = xyz.astype(np.float64)
    sel = rng.choice(1500, 300, replace=False)
    w[sel] += rng.choice([-3, -2, -1, 1, 2, 3], (300, 3)) @ cell[0].astype(np.float64)
    moved.append(w.astype(np.float32))
    for m in moved:
        q1 = eng.forward_xyz(offsets, m, x, Q, N, cell=cell)
        p1 = _pair_set(eng, 8 * 1500)
        assert np.array_equal(p0[0], p1[0]) and np.array_equal(p0[1], p1[1])
        assert np.abs(q1 - q0).max() <= TOL


def test_two_bases_of_one_lattice(gpu_engine_factory):
    """(12,0,0),(4,11,0),(-3,2.5,10.5) and the same lattice with b + a for b: same pair set, charges within TOL."""
    w = random_weights(9, 3, seed=4, scale=0.35)
    xyz, x = _cell(8, 120, cr.BASIS_A)
    off = np.int32([0, 120])
    eng = gpu_engine_factory(nx=9, T=3)
    eng.set_weights(w)
    qa = eng.forward_xyz(off, xyz, x, np.float32([-1]), 120, cell=cr.BASIS_A)
    pa = _pair_set(eng, 8 * 120)
    qb = eng.forward_xyz(off, xyz, x, np.float32([-1]), 120, cell=cr.BASIS_B)
    pb = _pair_set(eng, 8 * 120)
    assert np.array_equal(pa[0], pb[0]) and np.array_equal(pa[1], pb[1]) and np.array_equal(pa[2], pb[2])
    I, J, W = cr.pairs_cell(xyz, cr.BASIS_B)
    assert np.array_equal(pb[0], I) and np.array_equal(pb[1], J)
    assert np.abs(qa - qb).max() <= TOL


# ------------------------------------------------------------------------------------------------ 7. mixed batches
def test_mixed_batch_gives_each_molecules_bits(gpu_engine_factory):
    """An open molecule, a diagonal cell and general cells in one call: every molecule has the bits of its own call; the diagonal
    one those of its box call, the open one those of the open entry on the same route."""
    from epnn_amd import synth
    w = random_weights(9, 3, seed=8, scale=0.35)
    so, sxyz, sx, _, _ = synth.qm9_like_batch(B=6, seed=3)
    mols = [_cell(1, 20, cr.SHEARED), (sxyz[so[0]:so[1]], sx[so[0]:so[1]]), _box_cell(2, 60, [8.0, 8.0, 9.0]),
            _cell(3, 40, cr.RHOMB), _cell(4, 12, cr.WIRE), _cell(5, 30, cr.HEX_SLAB)]
    cells = np.stack([cr.SHEARED, np.zeros((3, 3), np.float32), np.diag(np.float32([8, 8, 9])), cr.RHOMB, cr.WIRE, cr.HEX_SLAB])
    offsets, xyz, x = _batch(mols)
    Q = np.float32([0, 1, -1, 0, 2, 0])
    eng = gpu_engine_factory(nx=9, T=3)
    eng.set_weights(w)
    q = eng.forward_xyz(offsets, xyz, x, Q, 64, cell=cells)
    g = np.random.default_rng(2).normal(size=int(offsets[-1])).astype(np.float32)
    _, gx, gs = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 64, cell=cells, strain=True)
    for b, (mx, mxx) in enumerate(mols):
        one = np.int32([0, len(mx)])
        alone = eng.forward_xyz(one, mx, mxx, Q[b:b + 1], 64, cell=cells[b])
        assert np.array_equal(q[offsets[b]:offsets[b + 1]], alone), b
        _, gx1, gs1 = eng.charges_vjp_xyz(one, mx, mxx, Q[b:b + 1], g[offsets[b]:offsets[b + 1]], 64, cell=cells[b], strain=True)
        assert np.array_equal(gx[offsets[b]:offsets[b + 1]], gx1) and np.array_equal(gs[b], gs1[0]), b
    b = 2
    assert np.array_equal(q[offsets[b]:offsets[b + 1]],
                          eng.forward_xyz(np.int32([0, 60]), mols[b][0], mols[b][1], Q[b:b + 1], 64, box=np.float32([8, 8, 9])))
    b = 1
    eng.set_option("wave_front", 0)
    assert np.array_equal(q[offsets[b]:offsets[b + 1]], eng.forward_xyz(np.int32([0, len(mols[b][0])]), mols[b][0], mols[b][1], Q[b:b + 1], 64))


# ------------------------------------------------------------------------------------------------ 8. device-resident entry
def test_device_entry_with_a_changing_cell(gpu_engine_factory):
    """Repeated device-resident calls on the same buffers, the cell changed in between (a flexible-cell run): each gives the
    blocking entry's result for its cell."""
    w = random_weights(9, 3, seed=9, scale=0.35)
    mols = [_cell(5 + k, n, cr.SHEARED) for k, n in enumerate([30, 40, 20])]
    offsets, xyz, x = _batch(mols)
    Q = np.float32([0, 1, 0])
    eng = gpu_engine_factory(nx=9, T=3)
    eng.set_weights(w)
    A = int(offsets[-1])
    dx, dX, dQ, dq = eng.to_device(xyz), eng.to_device(x), eng.to_device(Q), eng.alloc(A * 4)
    sheared2 = (cr.SHEARED + np.float32([[0.3, 0, 0], [0.2, -0.1, 0], [0.1, 0.3, 0.2]])).astype(np.float32)
    cells = [cr.SHEARED, cr.SHEARED, sheared2, np.float32(1.1) * cr.SHEARED, np.float32(1.1) * cr.SHEARED]
    want = [eng.forward_xyz(offsets, xyz, x, Q, 64, cell=c) for c in cells]
    got = []
    for c in cells:
        eng.forward_xyz_dev(offsets, dx, dX, dQ, dq, 64, cell=c)
        eng.sync()
        got.append(dq.download((A,)))
    for c in cells:                                            # back to back, no wait in between
        eng.forward_xyz_dev(offsets, dx, dX, dQ, dq, 64, cell=c)
    eng.sync()
    last = dq.download((A,))
    eng.forward_xyz_dev(offsets, dx, dX, dQ, dq, 64, box=np.float32([8, 8, 8]))      # a box after a cell on the same buffers
    eng.sync()
    boxed = dq.download((A,))
    for a in (dx, dX, dQ, dq):
        a.free()
    for k in range(len(cells)):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(last, want[-1])
    assert not np.array_equal(want[0], want[2])
    assert np.array_equal(boxed, eng.forward_xyz(offsets, xyz, x, Q, 64, box=np.float32([8, 8, 8])))


def test_one_handle_through_every_geometry(gpu_engine_factory):
    """One handle and one set of device buffers, forward_xyz_dev as open molecules, in a box, in the diagonal cell of that box, in a
    sheared cell and as open molecules again: every result has the bits of the same call on a fresh handle, the first and the last
    are equal.  Once with a wait behind every call and once for every prefix of the sequence back to back, where the handle decides
    from the kind and the rows of the forward before whether the next one is the same forward enqueued ahead."""
    w = random_weights(9, 2, seed=12, scale=0.35)
    box = np.float32([13.0, 12.0, 12.5])
    mols = [_cell(70 + k, n, cr.SHEARED) for k, n in enumerate([9, 20])]
    offsets, xyz, x = _batch(mols)
    Q = np.float32([0, -1])
    A = int(offsets[-1])
    geos = [{}, {"box": box}, {"cell": np.diag(box).astype(np.float32)}, {"cell": cr.SHEARED}, {}]

    def handle():
        eng = gpu_engine_factory(nx=9, T=2)
        eng.set_weights(w)
        return eng, (eng.to_device(xyz), eng.to_device(x), eng.to_device(Q), eng.alloc(A * 4))

    want = []
    for geo in geos:
        fresh, (dx, dX, dQ, dq) = handle()
        fresh.forward_xyz_dev(offsets, dx, dX, dQ, dq, 24, **geo)
        fresh.sync()
        want.append(dq.download((A,)))
    eng, (dx, dX, dQ, dq) = handle()
    for k, geo in enumerate(geos):
        eng.forward_xyz_dev(offsets, dx, dX, dQ, dq, 24, **geo)
        eng.sync()
        assert np.array_equal(dq.download((A,)), want[k]), k
    for k in range(len(geos)):
        for geo in geos[:k + 1]:                               # back to back, no wait in between
            eng.forward_xyz_dev(offsets, dx, dX, dQ, dq, 24, **geo)
        eng.sync()
        assert np.array_equal(dq.download((A,)), want[k]), k
    assert np.array_equal(want[0], want[4])
    assert not np.array_equal(want[1], want[3])                # (the atoms fill the sheared cell: its images are other neighbours than the box's)


# ------------------------------------------------------------------------------------------------ 9. gradients and strain
@pytest.mark.parametrize("N,ns,name", [(24, [20, 9], "sheared"), (96, [40], "slab"), (100, [40, 30], "sheared"), (24, [18, 10], "open")])
def test_charge_gradients_and_strain_in_cells(gpu_engine_factory, N, ns, name):
    """q, dq/dxyz and the strain derivative against the float64 reference (row-fused up to N = 96, layer-by-layer above; "open":
    open molecules through all-zero cells); sum_a gxyz = 0 per molecule; gstrain symmetric; a second call gives the same bits;
    without strain the same gxyz bits; the training state untouched."""
    cell = np.zeros((3, 3), np.float32) if name == "open" else GENERAL[name]
    w = random_weights(9, 2, seed=6, scale=0.5)
    if name == "open":
        mols = [((m[0] * np.float32(0.5)).astype(np.float32), m[1]) for m in (_box_cell(300 + k, n, [0.0, 0.0, 0.0]) for k, n in enumerate(ns))]
    else:
        mols = [_cell(300 + k, n, cell) for k, n in enumerate(ns)]
    offsets, xyz, x = _batch(mols)
    Q = np.float32([(0, 1)[k % 2] for k in range(len(ns))])
    eng = gpu_engine_factory(nx=9, T=2)
    eng.set_weights(w)
    eng.train_init()
    before = eng.get_gradients()
    w_before = eng.get_weights()
    g = np.random.default_rng(1).normal(size=int(offsets[-1])).astype(np.float32)
    kw = {} if name == "open" else {"cell": cell}
    q, gx, gs = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, strain=True, **kw)
    q2, gx2, gs2 = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, strain=True, **kw)
    assert np.array_equal(q, q2) and np.array_equal(gx, gx2) and np.array_equal(gs, gs2)
    q3, gx3 = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, **kw)
    assert np.array_equal(q, q3) and np.array_equal(gx, gx3)
    assert gs.shape == (len(ns), 3, 3) and gs.dtype == np.float32
    for b, (mx, mxx) in enumerate(mols):
        a0, a1 = offsets[b], offsets[b + 1]
        gb = g[a0:a1].astype(np.float64)
        q_ref, ref, W = cr.strain64(mx, mxx, Q[b], gb, cell, w, N=N)
        _, lo, Wlo = cr.strain64(mx, mxx, Q[b], gb, cell, w, N=N, kink_shift=2e-5)
        _, hi, Whi = cr.strain64(mx, mxx, Q[b], gb, cell, w, N=N, kink_shift=-2e-5)
        dq, dg, dW = np.abs(q[a0:a1] - q_ref[:a1 - a0]).max(), np.abs(gx[a0:a1] - ref).max(), np.abs(gs[b] - W).max()
        print(f"{name} N={N} mol {b}: |dq| {dq:.2e}  |dgxyz| {dg:.2e} of {np.abs(ref).max():.2e} (kink {np.abs(lo - hi).max():.1e})  "
              f"|dgstrain| {dW:.2e} of {np.abs(W).max():.2e} (kink {np.abs(Wlo - Whi).max():.1e})")
        assert dq <= 2e-4
        assert dg <= 2e-4 * np.abs(ref).max() + np.abs(lo - hi).max(), (b, dg)
        assert dW <= 2e-4 * np.abs(W).max() + np.abs(Wlo - Whi).max(), (b, dW)
        assert np.abs(gx[a0:a1].astype(np.float64).sum(0)).max() <= 1e-4 * max(1.0, np.abs(ref).max())
        assert np.array_equal(gs[b], gs[b].T)                     # the output layout: six sums mirrored into nine slots
        assert np.abs(W - W.T).max() <= 1e-12 * np.abs(W).max()   # (the reference forms all nine products: symmetric to rounding)
        assert np.abs(W).max() > 1e-4
    assert np.array_equal(eng.get_gradients(), before)
    after = eng.get_weights()
    for t in range(2):
        for l in range(3):
            assert np.array_equal(after["msg"][t][l][0], w_before["msg"][t][l][0])


def test_training_state_untouched(gpu_engine_factory):
    """Gradients, weights and the Adam state of a training handle: a twin handle that never made the gradient call takes the
    same optimizer step, bit for bit."""
    from oracle import epnn_oracle_train as otr
    w = random_weights(9, 2, seed=6, scale=0.5)
    mols = [_cell(400 + k, n, cr.SHEARED) for k, n in enumerate([14, 9])]
    offsets, xyz, x = _batch(mols)
    Q = np.float32([0, 1])
    A = int(offsets[-1])
    y = np.random.default_rng(3).normal(size=A).astype(np.float32) * 0.1
    g = np.random.default_rng(7).normal(size=A).astype(np.float32)
    eng, twin = gpu_engine_factory(nx=9, T=2), gpu_engine_factory(nx=9, T=2)
    for e in (eng, twin):
        e.set_weights(w)
        e.train_init()
        e.train_step_xyz(offsets, xyz, x, Q, y, 16, apply=False)
    grads = eng.get_gradients()
    weights = otr.flatten(eng.get_weights())
    eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 16, cell=cr.SHEARED, strain=True)
    assert np.array_equal(eng.get_gradients(), grads)
    assert np.array_equal(otr.flatten(eng.get_weights()), weights)
    for e in (eng, twin):
        e.train_apply()
    assert np.array_equal(otr.flatten(eng.get_weights()), otr.flatten(twin.get_weights()))


# ------------------------------------------------------------------------------------------------ 10. jacobian, dense route, partition
def test_charge_jacobian_in_a_cell(gpu_engine_factory):
    from epnn_amd.charge_gn import make_model
    w = random_weights(9, 2, seed=6, scale=0.5)
    xyz, x = _cell(77, 14, cr.SHEARED)
    model = make_model([32, 32], 48, 2, 9, 16)
    model.set_weights_dict(w)
    q, J = model.charge_jacobian_xyz(xyz, x, 1.0, cell=cr.SHEARED)
    for i in (0, 5, 13):
        g = np.zeros(14)
        g[i] = 1.0
        ref = cr.vjp64_cell(xyz, x, np.float32(1.0), g, cr.SHEARED, w, N=16)[1]
        assert np.abs(J[i] - ref).max() <= 2e-4 * max(1.0, np.abs(ref).max()) + 1e-6


def test_dense_route(gpu_engine_factory):
    """edges_ex(cell=...) equals the reference's float32 edges to 1e-7 with identical near flags, C to 1e-12; get_init_edges passes
    the cell on; a dense make_model call on them agrees with predict_xyz(cell=...) to 1e-5."""
    from epnn_amd.charge_gn import get_init_edges, make_model
    w = random_weights(9, 3, seed=10, scale=0.35)
    for cell in (cr.SHEARED, cr.HEX_SLAB):
        xyz, x = _cell(21, 24, cell)
        eng = gpu_engine_factory(nx=9, T=3)
        e, C = eng.edges_ex(xyz, 48, cell=cell)
        er, Cr = cr.get_init_edges_cell(xyz, cell)
        assert np.abs(e - er).max() <= 1e-7
        assert np.array_equal(e.max(-1) > 1e-5, er.max(-1) > 1e-5)
        assert np.abs(C - Cr).max() <= 1e-12
        e2, C2 = get_init_edges(xyz, np.zeros((0,)), num=48, cell=cell)
        assert np.array_equal(e2, e) and np.array_equal(C2[:, :, 0], C)
        N = 24
        model = make_model([32, 32], 48, 3, 9, N)
        model.set_weights_dict(w)
        h = np.zeros((1, N, N, 48), np.float32)
        xx = np.broadcast_to(x[None, None], (1, N, N, 9)).copy()
        q0 = np.full((1, N, N, 1), np.float32(np.float32(0.0) / np.float32(N)), np.float32)
        mask = np.ones((1, N, N, 1), np.float32)
        dense = model([h, e[None], xx, q0, mask])[0, :, 0]
        q = model.predict_xyz(np.int32([0, N]), xyz, x, np.float32([0.0]), N=N, cell=cell)
        assert np.abs(dense - q).max() <= 1e-5


_PART_WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import torch.distributed as dist
from epnn_amd import shard, synth
from epnn_amd.engine import Engine
from conftest import random_weights
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
off, xyz, x, Q, N, cell = synth.triclinic_cell_system(1500, seed=11)
eng = Engine(nx=9, T=3)
eng.set_weights(random_weights(9, 3, seed=5, scale=0.35))
whole = eng.forward_xyz(off, xyz, x, Q, N, cell=cell)
eng.set_partition(rank, world, shard.make_row_exchange(eng, dist, rank, world))
part = eng.forward_xyz(off, xyz, x, Q, N, cell=cell)
assert np.array_equal(part, whole), (rank, float(np.abs(part - whole).max()))
eng.close()
dist.barrier()
if rank == 0:
    print("PARTITION_OK")
'''


def test_partitioned_sheared_cell(tmp_path):
    """The sheared 1500-atom cell over three processes sharing the GPU (gloo exchange): every rank bit-identical to the
    unpartitioned run."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "worker.py"
    script.write_text(_PART_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29543", OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3",
                          "--master-addr", "127.0.0.1", "--master-port", "29543", str(script), root],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    assert "PARTITION_OK" in out.stdout


# ------------------------------------------------------------------------------------------------ 11. errors
def test_errors_leave_the_handle_intact(gpu_engine_factory):
    from epnn_amd._lib import EpnnError
    w = random_weights(9, 3, seed=9, scale=0.35)
    mols = [_cell(50, 20, cr.SHEARED), _cell(51, 30, cr.SHEARED)]
    offsets, xyz, x = _batch(mols)
    Q = np.float32([0, 1])
    eng = gpu_engine_factory(nx=9, T=3)
    eng.set_weights(w)
    q = eng.forward_xyz(offsets, xyz, x, Q, 32, cell=cr.SHEARED)
    g = np.ones(int(offsets[-1]), np.float32)
    nan_cell, inf_cell = cr.SHEARED.copy(), cr.SHEARED.copy()
    nan_cell[1, 0], inf_cell[2, 2] = np.nan, np.inf
    dependent3 = np.float32([[8, 0, 0], [3, 7.5, 0], [11, 7.5, 0]])
    dependent2 = np.float32([[8, 1, 0], [0, 0, 0], [16, 2, 0]])
    for bad, msg in ((cr.THIN, "width"), (dependent3, "dependent"), (dependent2, "dependent"), (nan_cell, "finite"), (inf_cell, "finite"),
                     (np.diag(np.float32([5.9, 7, 7])), "width")):
        with pytest.raises(EpnnError, match=msg):
            eng.forward_xyz(offsets, xyz, x, Q, 32, cell=bad)
        with pytest.raises(EpnnError, match=msg):
            eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 32, cell=bad, strain=True)
        with pytest.raises(EpnnError, match=msg):
            eng.edges_ex(xyz[:20], 48, cell=bad)
    with pytest.raises(EpnnError, match=r"cell\[1\].*molecule 1.*axis 0"):              # names molecule and axis
        eng.forward_xyz(offsets, xyz, x, Q, 32, cell=np.stack([cr.SHEARED, cr.THIN]))
    for shape in ((3,), (2, 3), (1, 3, 3), (3, 3, 3)):
        with pytest.raises(ValueError, match="cell must have shape"):
            eng.forward_xyz(offsets, xyz, x, Q, 32, cell=np.full(shape, 7.0, np.float32))
    with pytest.raises(ValueError, match="cell must have shape"):
        eng.edges_ex(xyz[:20], 48, cell=np.zeros((1, 3, 3), np.float32))
    with pytest.raises(ValueError, match="box and cell"):
        eng.forward_xyz(offsets, xyz, x, Q, 32, box=np.float32([7, 7, 7]), cell=cr.SHEARED)
    with pytest.raises(ValueError, match="box must have shape"):
        eng.forward_xyz(offsets, xyz, x, Q, 32, box=np.full((3, 3), 7.0, np.float32))
    from epnn_amd._lib import fptr, iptr
    out = np.empty(int(offsets[-1]), np.float32)
    assert eng.lib.epnn_forward_xyz_cell(eng.h, 2, 32, iptr(offsets), fptr(xyz), fptr(x), fptr(Q), None, fptr(out)) != 0
    assert b"null cell" in eng.lib.epnn_last_error()
    assert np.array_equal(eng.forward_xyz(offsets, xyz, x, Q, 32, cell=cr.SHEARED), q)
    # coincident images: an atom and another one shifted by a lattice vector
    twin = xyz[:20].copy()
    twin[1] = (twin[0].astype(np.float64) + cr.SHEARED[1].astype(np.float64) - cr.SHEARED[2].astype(np.float64)).astype(np.float32)
    twin = (np.round(twin * 64) / 64).astype(np.float32)          # dyadic coordinates: the shift is exact
    twin[1] = twin[0] + cr.SHEARED[1] - cr.SHEARED[2]
    with pytest.raises(EpnnError, match="coincide"):
        eng.charges_vjp_xyz(np.int32([0, 20]), twin, x[:20], Q[:1], g[:20], 32, cell=cr.SHEARED)
    assert np.array_equal(eng.forward_xyz(offsets, xyz, x, Q, 32, cell=cr.SHEARED), q)
