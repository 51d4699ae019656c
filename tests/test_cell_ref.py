"""The float64 reference for general cells (tests/cell_ref.py) checked against things that do not share its code: a search over
5^3 images, tests/periodic_ref.py for diagonal cells, a rigid rotation, a replication of the cell, a second basis of the lattice,
and central differences for the coordinate and the strain derivative.  Also the pure-Python argument checks of cell=.  CPU only."""
import numpy as np
import pytest

from conftest import random_weights
import cell_ref as cr
import periodic_ref as pr
import xyz_grad_ref as xgr

CELLS = {"sheared": cr.SHEARED, "hex120": cr.HEX120, "hex60": cr.HEX60, "rhomb": cr.RHOMB, "slab": cr.HEX_SLAB, "wire": cr.WIRE,
         "basis_a": cr.BASIS_A, "basis_b": cr.BASIS_B}


def _mol(seed, n, cell):
    rng = np.random.default_rng(seed)
    xyz = cr.random_cell(rng, n, cell)
    x = np.zeros((n, 9), np.float32)
    el = rng.integers(0, 4, n)
    x[:, 0] = np.array([1, 6, 7, 8])[el]
    x[np.arange(n), 1 + el] = 1
    return xyz, x


def _rotation(seed):
    q, _ = np.linalg.qr(np.random.default_rng(seed).normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def test_widths_are_the_ones_the_cells_were_chosen_for():
    want = {"sheared": (6.81, 7.21, 7.00), "hex120": (6.06, 6.06, 6.5), "hex60": (6.50, 6.50, 6.5), "rhomb": (8.40, 8.40, 8.40),
            "basis_a": (10.6, 10.7, 10.5), "basis_b": (6.4, 10.7, 10.5)}
    for k, w in want.items():
        assert np.abs(cr.widths(CELLS[k]) - np.array(w)).max() < 0.05, k
        assert cr.widths(CELLS[k]).min() >= 6.0
    assert np.allclose(cr.widths(cr.HEX_SLAB)[:2], 6.495, atol=1e-2) and np.isinf(cr.widths(cr.HEX_SLAB)[2])
    assert abs(cr.widths(cr.WIRE)[2] - 6.87) < 0.01
    assert abs(cr.widths(cr.THIN).min() - 5.15) < 0.01 and np.sqrt((cr.THIN.astype(float) ** 2).sum(1)).min() > 6.0
    for cell in CELLS.values():                                   # the dual vectors: g_k . a_l = delta_kl on the periodic rows
        a, g = cr.duals(cell)
        per = [k for k in range(3) if np.any(a[k] != 0)]
        assert np.abs((g @ a.T)[np.ix_(per, per)] - np.eye(len(per))).max() < 1e-14


@pytest.mark.parametrize("name", sorted(CELLS))
def test_distances_against_a_search_over_images(name):
    """200 random atoms, anywhere up to a few cells outside: every pair with an image within 3 A gets that distance, no pair has
    two images within 3 A, every other distance the rule returns is >= 3 A (it need not be the shortest one)."""
    cell = CELLS[name]
    rng = np.random.default_rng(3)
    a, _ = cr.duals(cell)
    span = a + np.diag([0.0 if np.any(a[k] != 0) else 6.0 for k in range(3)])
    r = ((rng.uniform(-2, 3, (200, 3)) @ span).astype(np.float32)).astype(np.float64)
    D = cr._dist(cr.mic(r[None] - r[:, None], cell))
    rngs = [range(-4, 5) if np.any(a[k] != 0) else range(0, 1) for k in range(3)]       # 9^3 images on periodic axes
    d0 = r[None] - r[:, None]
    for k in range(3):                                           # bring the difference near the origin first (any integers do)
        if np.any(a[k] != 0):
            d0 = d0 - np.rint(d0 @ np.linalg.pinv(a)[:, k])[..., None] * a[k]
    best = np.full(D.shape, np.inf)
    count = np.zeros(D.shape, int)
    for i0 in rngs[0]:
        for i1 in rngs[1]:
            for i2 in rngs[2]:
                dd = np.sqrt(((d0 + i0 * a[0] + i1 * a[1] + i2 * a[2]) ** 2).sum(-1))
                best = np.minimum(best, dd)
                count += dd < 3.0
    off = ~np.eye(200, dtype=bool)
    close = (best < 3.0) & off
    assert close.sum() > 100
    assert np.abs(D[close] - best[close]).max() < 1e-11
    assert count[off].max() == 1
    assert (D[~close & off] >= 3.0).all()
    assert (D[off] >= best[off] - 1e-11).all()


@pytest.mark.parametrize("L", [[7.0, 6.5, 8.25], [6.5, 0.0, 7.0], [0.0, 0.0, 6.0], [0.0, 0.0, 0.0]])
def test_diagonal_cells_equal_the_periodic_reference(L):
    w = random_weights(9, 2, seed=1, scale=0.35)
    L = np.float32(L)
    xyz, x = _mol(2, 16, np.diag(L))
    cell = np.diag(L)
    e0, C0 = pr.get_init_edges_pbc(xyz, L)
    e1, C1 = cr.get_init_edges_cell(xyz, cell)
    assert np.array_equal(e0, e1) and np.array_equal(C0, C1)
    assert np.array_equal(pr.forward_pbc(xyz, x, np.float32(1.0), L, w, N=18), cr.forward_cell(xyz, x, np.float32(1.0), cell, w, N=18))
    for a, b in zip(pr.pairs_pbc(xyz, L), cr.pairs_cell(xyz, cell)):
        assert np.array_equal(a, b)
    g = np.random.default_rng(0).normal(size=16)
    q0, g0 = pr.vjp64_pbc(xyz, x, np.float32(1.0), g, L, w, N=18)
    q1, g1 = cr.vjp64_cell(xyz, x, np.float32(1.0), g, cell, w, N=18)
    assert np.array_equal(q0, q1) and np.array_equal(g0, g1)


def test_a_rotated_orthorhombic_cell():
    """Cell rows and coordinates rotated in float64, then rounded to float32: the charges equal those of the unrotated system up to
    that rounding, which is bounded by running the reference on the rotated inputs before rounding."""
    w = random_weights(9, 3, seed=2, scale=0.35)
    L = np.float32([6.5, 7.25, 8.0])
    xyz, x = _mol(4, 18, np.diag(L))
    R = _rotation(1)
    r_rot, a_rot = xyz.astype(np.float64) @ R.T, np.diag(L.astype(np.float64)) @ R.T
    q_box = pr.forward64_pbc(xyz, x, np.float32(0.0), L, w)
    q_f32 = cr.forward64_cell(r_rot.astype(np.float32), x, np.float32(0.0), a_rot.astype(np.float32), w)

    # the rotated system in float64, nothing rounded: edges64_at on (r_rot, a_rot); near flags from the unrotated system
    saved = xgr.edges64, xgr.orc
    xgr.edges64, xgr.orc = (lambda _x, num, cutoff=3.0, eta=2.0: cr.edges64_at(r_rot, a_rot, num, cutoff, eta)), pr._OrcPBC(L)
    try:
        q_f64 = xgr.forward64(xyz, x, np.float32(0.0), w)
    finally:
        xgr.edges64, xgr.orc = saved
    assert np.abs(q_f64 - q_box).max() <= 1e-12                 # a rotation changes no distance
    rounding = np.abs(q_f32 - q_f64).max()
    assert rounding <= 1e-5                                      # float32 coordinates of ~8 A: 5e-7 A
    assert np.abs(q_f32 - q_box).max() <= rounding + 1e-12


def test_a_replicated_cell():
    """A sheared cell with 30 atoms doubled along every axis (240 atoms, cell rows doubled).  The model itself is not local (a
    message is formed for every pair of a molecule, with zero edge features beyond the cutoff), so the comparison is made on the
    edges: in the doubled cell exactly one of the eight copies of j carries the edge i-j of the small cell, the others and the
    seven other copies of i itself carry none."""
    cell = cr.SHEARED
    xyz, _ = _mol(6, 30, cell)
    xyz = (np.round(xyz * 256) / 256).astype(np.float32)          # dyadic: the shifted copies are exact in float32
    a = cell.astype(np.float64)
    reps = [i * a[0] + j * a[1] + k * a[2] for i in (0, 1) for j in (0, 1) for k in (0, 1)]
    big64 = np.concatenate([xyz.astype(np.float64) + s for s in reps])
    big = big64.astype(np.float32)
    assert np.array_equal(big.astype(np.float64), big64)
    e1, C1 = cr.get_init_edges_cell(xyz, cell)
    e8, C8 = cr.get_init_edges_cell(big, 2 * cell)
    e8, C8 = e8.reshape(8, 30, 8, 30, 48), C8.reshape(8, 30, 8, 30)
    assert (C1 > 0).sum() > 60                                     # (two partners per atom would already do)
    for c in range(8):
        assert np.array_equal(e8[c].sum(1), e1) and np.array_equal(C8[c].sum(1), C1)
        assert ((C8[c] > 0).sum(1) <= 1).all()


def test_two_bases_of_one_lattice():
    w = random_weights(9, 3, seed=4, scale=0.35)
    xyz, x = _mol(8, 60, cr.BASIS_A)
    Ia, Ja, Wa = cr.pairs_cell(xyz, cr.BASIS_A)
    Ib, Jb, Wb = cr.pairs_cell(xyz, cr.BASIS_B)
    assert np.array_equal(Ia, Ib) and np.array_equal(Ja, Jb) and np.array_equal(Wa, Wb)
    qa = cr.forward_cell(xyz, x, np.float32(-1.0), cr.BASIS_A, w)
    qb = cr.forward_cell(xyz, x, np.float32(-1.0), cr.BASIS_B, w)
    assert np.abs(qa - qb).max() <= 1e-12
    ra = xyz.astype(np.float64)
    Da, Db = cr._dist(cr.mic(ra[None] - ra[:, None], cr.BASIS_A)), cr._dist(cr.mic(ra[None] - ra[:, None], cr.BASIS_B))
    assert (Da != Db).any()                                       # beyond the cutoff the two bases may return different images


@pytest.mark.parametrize("name,n", [("sheared", 9), ("slab", 8), ("open", 6)])
def test_gradient_and_strain_match_central_differences(name, n):
    """gxyz: atoms displaced; gstrain: atoms and cell deformed together, r -> (1 + eps) r, a_k -> (1 + eps) a_k.  Float64
    coordinates and cells as they are (edges64_at), the near flags of the undeformed system (constants, as in
    tests/test_xyz_grad_ref.py)."""
    cell = np.zeros((3, 3), np.float32) if name == "open" else CELLS[name]
    w = random_weights(9, 2, seed=7, scale=0.7)
    if name == "open":
        xyz, x = _mol(11, n, cell)                                # (random_cell spans 6 A on open axes)
        xyz = (xyz * 0.45).astype(np.float32)                     # an open molecule 2.7 A across: most pairs within the cutoff
    else:
        xyz, x = _mol(11, n, cell)
    g = np.random.default_rng(1).normal(size=n)
    Q = np.float32(1.0)
    N = n + 2
    q, gx, W = cr.strain64(xyz, x, Q, g, cell, w, N=N)
    q2, gx2 = cr.vjp64_cell(xyz, x, Q, g, cell, w, N=N)
    assert np.array_equal(q, q2) and np.array_equal(gx, gx2)
    assert np.abs(W - W.T).max() <= 1e-12 * max(1.0, np.abs(W).max()) and np.abs(W).max() > 1e-6
    r0, a0 = xyz.astype(np.float64), cr.duals(cell)[0]
    if name != "open":
        Dm, Do = cr._dist(cr.mic(r0[None] - r0[:, None], cell)), np.sqrt(((r0[None] - r0[:, None]) ** 2).sum(-1))
        assert ((Dm < 3.0) & (Do >= 3.0)).any()                   # pairs across the faces take part

    def f(r, a):
        saved = xgr.edges64, xgr.orc
        xgr.edges64, xgr.orc = (lambda _x, num, cutoff=3.0, eta=2.0: cr.edges64_at(r, a, num, cutoff, eta)), cr._OrcCell(cell)
        try:
            return xgr.forward64(xyz, x, Q, w, N=N)[:n] @ g
        finally:
            xgr.edges64, xgr.orc = saved

    h = 1e-4
    fd = np.zeros((n, 3))
    for i in range(n):
        for c in range(3):
            rp, rm = r0.copy(), r0.copy()
            rp[i, c] += h
            rm[i, c] -= h
            fd[i, c] = (f(rp, a0) - f(rm, a0)) / (2 * h)
    assert np.abs(gx - fd).max() <= 1e-6 + 1e-5 * np.abs(fd).max(), (np.abs(gx - fd).max(), np.abs(fd).max())
    h = 1e-5
    fs = np.zeros((3, 3))
    for a in range(3):
        for c in range(3):
            eps = np.zeros((3, 3))
            eps[a, c] = h
            Fp, Fm = np.eye(3) + eps, np.eye(3) - eps              # r_a -> r_a + eps_ac r_c
            fs[a, c] = (f(r0 @ Fp.T, a0 @ Fp.T) - f(r0 @ Fm.T, a0 @ Fm.T)) / (2 * h)
    assert np.abs(W - fs).max() <= 1e-6 + 1e-5 * np.abs(fs).max(), (W, fs)
    if name != "open":
        # derivative with respect to the lattice vectors at fixed fractional coordinates: dF/dH = G^T W, G = H^-1
        per = [k for k in range(3) if np.any(a0[k] != 0)]
        Hm = a0 + np.diag([0.0 if k in per else 1.0 for k in range(3)])       # open axes: any completion, their rows do not move
        frac = r0 @ np.linalg.inv(Hm)
        dH = np.linalg.inv(Hm).T @ W
        for k in per:
            for c in range(3):
                Hp, Hn = Hm.copy(), Hm.copy()
                Hp[k, c] += h
                Hn[k, c] -= h
                ap, an = a0.copy(), a0.copy()
                ap[k, c] += h
                an[k, c] -= h
                num = (f(frac @ Hp, ap) - f(frac @ Hn, an)) / (2 * h)
                assert abs(dH[k, c] - num) <= 1e-6 + 1e-5 * np.abs(dH).max(), (k, c, dH[k, c], num)


def test_orthorhombic_length_derivative():
    """dF/dL_k = W_kk / L_k for an orthorhombic cell, against central differences of the periodic reference's own distances."""
    w = random_weights(9, 2, seed=7, scale=0.7)
    L = np.float32([6.0, 6.5, 7.0])
    cell = np.diag(L)
    xyz, x = _mol(12, 8, cell)
    g = np.random.default_rng(2).normal(size=8)
    _, _, W = cr.strain64(xyz, x, np.float32(0.0), g, cell, w)
    r0, a0 = xyz.astype(np.float64), cell.astype(np.float64)
    frac = r0 / L.astype(np.float64)

    def f(a):
        saved = xgr.edges64, xgr.orc
        xgr.edges64, xgr.orc = (lambda _x, num, cutoff=3.0, eta=2.0: cr.edges64_at(frac * np.diag(a), a, num, cutoff, eta)), pr._OrcPBC(L)
        try:
            return xgr.forward64(xyz, x, np.float32(0.0), w)[:8] @ g
        finally:
            xgr.edges64, xgr.orc = saved

    h = 1e-5
    for k in range(3):
        ap, am = a0.copy(), a0.copy()
        ap[k, k] += h
        am[k, k] -= h
        num = (f(ap) - f(am)) / (2 * h)
        assert abs(W[k, k] / float(L[k]) - num) <= 1e-6 + 1e-5 * np.abs(W).max() / 6.0, (k, W[k, k] / float(L[k]), num)


def test_python_argument_checks():
    """cell shapes and box-with-cell are refused in Python, before anything reaches the library (no GPU needed)."""
    from epnn_amd import engine
    assert engine._cell_rows(cr.SHEARED, 4).shape == (4, 3, 3)
    assert engine._cell_rows(np.tile(cr.SHEARED, (3, 1, 1)), 3).shape == (3, 3, 3)
    assert engine._cell_rows(cr.SHEARED, 3).shape == (3, 3, 3) and np.array_equal(engine._cell_rows(cr.SHEARED, 3)[2], cr.SHEARED)
    for shape in ((3,), (9,), (2, 3, 3), (1, 3), (3, 3, 1)):
        with pytest.raises(ValueError, match="cell must have shape"):
            engine._cell_rows(np.ones(shape, np.float32), 4)
    with pytest.raises(ValueError, match="box must have shape"):
        engine._box_rows(np.ones((3, 3), np.float32), 4)
    eng = object.__new__(engine.Engine)                           # no handle: the argument checks come first
    off = np.int32([0, 2])
    xyz, x = np.zeros((2, 3), np.float32), np.zeros((2, 9), np.float32)
    for call in (lambda: eng.forward_xyz(off, xyz, x, np.float32([0]), 2, box=np.float32([7, 7, 7]), cell=cr.SHEARED),
                 lambda: eng.charges_vjp_xyz(off, xyz, x, np.float32([0]), np.zeros(2, np.float32), 2, box=np.float32([7, 7, 7]), cell=cr.SHEARED),
                 lambda: eng.edges_ex(xyz, 48, box=np.float32([7, 7, 7]), cell=cr.SHEARED),
                 lambda: eng.forward_xyz_dev(off, None, None, None, None, 2, box=np.float32([7, 7, 7]), cell=cr.SHEARED)):
        with pytest.raises(ValueError, match="box and cell"):
            call()
    with pytest.raises(ValueError, match="strain"):
        eng.charges_vjp_xyz(off, xyz, x, np.float32([0]), np.zeros(2, np.float32), 2, box=np.float32([7, 7, 7]), strain=True)


def test_triclinic_cell_system():
    from epnn_amd import synth
    off, xyz, x, Q, N, cell = synth.triclinic_cell_system(3000, seed=2)
    assert cell.shape == (1, 3, 3) and cell.dtype == np.float32 and xyz.shape == (3000, 3) and N == 3000
    _, _, _, _, _, box = synth.periodic_box_system(8, seed=0)
    assert abs(abs(np.linalg.det(cell[0].astype(np.float64))) - 3000 / 0.1) < 1.0       # the density of periodic_box_system
    assert np.count_nonzero(cell[0] - np.diag(np.diag(cell[0]))) == 3 and cr.widths(cell[0]).min() > 6.0
    I, J, W = cr.pairs_cell(xyz, cell[0])
    assert 10.5 < 2 * len(I) / 3000 < 12.0
    r = xyz.astype(np.float64)
    D = cr._dist(cr.mic(r[J] - r[I], cell[0]))
    assert D.min() >= 0.9 - 1e-5                                   # the separation holds across the faces (float32 coordinates)
    a, g = cr.duals(cell[0])
    assert ((np.abs(np.rint((r[J] - r[I]) @ g.T)).sum(1)) > 0).mean() > 0.1             # many pairs cross a face
