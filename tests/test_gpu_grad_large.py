"""Charge gradients from the pair list (option "grad_path" = 2, automatic above B N^2 = 2^22) on the GPU: against the float64
references, against the dense path, on large periodic systems, determinism, special cases, the untouched training state, error
paths and routing. GPU only.  Every test sets "grad_path", which a library without the pair-list path refuses."""
import numpy as np
import pytest

import cell_ref
import periodic_ref
from cell_ref import strain64, vjp64_cell
from conftest import load_molecules, random_weights
from grad_large_ref import vjp64_large
from periodic_ref import vjp64_pbc
from xyz_grad_ref import vjp64

pytestmark = pytest.mark.gpu

TAU = 2e-5           # ReLU-kink bracket of the references


def _features(rng, n, nx):
    x = np.zeros((n, nx), dtype=np.float32)
    el = rng.integers(0, nx - 1, n)
    x[np.arange(n), 1 + el] = 1.0
    x[:, 0] = np.array([1, 6, 7, 8, 9, 15, 16, 17, 35])[el % 9]
    return x, np.float32(rng.integers(-1, 2))


def _lattice_molecule(n, nx, seed):
    """n atoms on a jittered 1.15 A lattice (no two closer than ~0.9 A), one-hot x like parse_xyz, Q in {-1, 0, 1}."""
    rng = np.random.default_rng(seed)
    k = int(np.ceil(n ** (1 / 3)))
    grid = np.array([(a, b, c) for a in range(k) for b in range(k) for c in range(k)], dtype=np.float64)[:n] * 1.15
    xyz = (grid + rng.uniform(-0.1, 0.1, grid.shape)).astype(np.float32)
    return (xyz,) + _features(rng, n, nx)


def _batch(mols):
    offsets = np.zeros(len(mols) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([m[0].shape[0] for m in mols])
    return (offsets, np.concatenate([m[0] for m in mols]), np.concatenate([m[1] for m in mols]),
            np.array([m[2] for m in mols], dtype=np.float32))


def _open(w):
    return lambda xyz, x, Q, g, **kw: vjp64(xyz, x, Q, g, w, **kw)


def _engine(factory, w, nx, path=2, **kw):
    eng = factory(nx=nx, T=len(w["msg"]), **kw)
    eng.set_weights(w)
    eng.set_option("grad_path", path)
    return eng


def _reference(ref_fn, mol, g, N, h_dim):
    """(q, gxyz, kink) of one molecule from a literal float64 reference ref_fn(xyz, x, Q, g, N=, h_dim=, kink_shift=)."""
    mx, mxx, mQ = mol
    q_ref, ref = ref_fn(mx, mxx, mQ, g, N=N, h_dim=h_dim)[:2]
    lo = ref_fn(mx, mxx, mQ, g, N=N, h_dim=h_dim, kink_shift=+TAU)[1]
    hi = ref_fn(mx, mxx, mQ, g, N=N, h_dim=h_dim, kink_shift=-TAU)[1]
    return q_ref, ref, np.abs(lo - hi).max()


def _check(eng, mols, N, ref_fns, h_dim=48, seed=0, both_paths=True, **geo):
    """The tolerances of test_gpu_xyz_grad._check_against_reference on the pair-list path: per molecule |gxyz - ref| <= 2e-4 max |ref|
    + kink bracket, q within 2e-4 of forward_xyz and of the reference; and the two paths agree to twice that."""
    offsets, xyz, x, Q = _batch(mols)
    g = np.random.default_rng(seed).normal(size=int(offsets[-1])).astype(np.float32)
    eng.set_option("grad_path", 2)
    q, gxyz = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, **geo)
    q_fwd = eng.forward_xyz(offsets, xyz, x, Q, N, **geo)
    print(f"q vs forward_xyz {np.abs(q - q_fwd).max():.3e}")
    assert np.abs(q - q_fwd).max() <= 2e-4
    if both_paths:
        eng.set_option("grad_path", 1)
        q_d, gxyz_d = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, **geo)
        eng.set_option("grad_path", 2)
    for b, mol in enumerate(mols):
        a0, a1 = offsets[b], offsets[b + 1]
        q_ref, ref, kink = _reference(ref_fns[b], mol, g[a0:a1].astype(np.float64), N, h_dim)
        scale = np.abs(ref).max()
        err = np.abs(gxyz[a0:a1] - ref).max()
        print(f"molecule {b} (n = {a1 - a0}): q {np.abs(q[a0:a1] - q_ref[:a1 - a0]).max():.3e}; gxyz {err:.3e} of {scale:.3e}, kink {kink:.3e}")
        assert np.abs(q[a0:a1] - q_ref[:a1 - a0]).max() <= 2e-4
        assert scale > 0
        assert err <= 2e-4 * scale + kink, (b, err, scale, kink)
        if both_paths:
            dd = np.abs(gxyz[a0:a1] - gxyz_d[a0:a1]).max()
            print(f"    dense path vs pair-list path {dd:.3e}")
            assert dd <= 4e-4 * np.abs(gxyz_d[a0:a1]).max() + kink, (b, dd, kink)
            assert np.abs(q[a0:a1] - q_d[a0:a1]).max() <= 2e-4


# ---------------------------------------------------------------------------------------------------- against the float64 references
@pytest.mark.parametrize("n,N", [(40, 40), (97, 97), (150, 150), (300, 300), (300, 320)])
def test_lattice_molecules(gpu_engine_factory, n, N):
    w = random_weights(9, 2, seed=5, scale=0.6)
    eng = _engine(gpu_engine_factory, w, 9)
    _check(eng, [_lattice_molecule(n, 9, seed=n)], N, [_open(w)])


def test_batch_of_three_sizes(gpu_engine_factory):
    w = random_weights(10, 3, seed=6, scale=0.6)
    eng = _engine(gpu_engine_factory, w, 10)
    _check(eng, [_lattice_molecule(n, 10, seed=n) for n in (70, 33, 120)], 128, [_open(w)] * 3)


def test_model_weights_on_the_validation_split(gpu_engine_factory, val_dir, val_names, weights_full):
    mols = load_molecules(val_dir, val_names[:6], nx=10)[0]
    eng = _engine(gpu_engine_factory, weights_full, 10)
    _check(eng, mols, 41, [_open(weights_full)] * 6)


def test_small_h_dim(gpu_engine_factory):
    w = random_weights(9, 2, seed=8, scale=0.6, h_dim=20)
    eng = _engine(gpu_engine_factory, w, 9, h_dim=20, e_dim=20)
    _check(eng, [_lattice_molecule(n, 9, seed=20 + n) for n in (50, 64)], 70, [_open(w)] * 2, h_dim=20)


@pytest.mark.parametrize("L,n,N", [([13.0, 12.0, 12.5], 200, 200), ([12.0, 0.0, 13.0], 180, 192)])
def test_periodic_boxes(gpu_engine_factory, L, n, N):
    w = random_weights(9, 2, seed=11, scale=0.6)
    eng = _engine(gpu_engine_factory, w, 9)
    rng = np.random.default_rng(n)
    L = np.float32(L)
    mol = (periodic_ref.random_cell(rng, n, L),) + _features(rng, n, 9)
    ref = lambda xyz, x, Q, g, **kw: vjp64_pbc(xyz, x, Q, g, L, w, **kw)
    _check(eng, [mol], N, [ref], box=L)


@pytest.mark.parametrize("name,n,N", [("BASIS_A", 200, 200), ("HEX_SLAB", 60, 64)])
def test_cells_and_strain(gpu_engine_factory, name, n, N):
    w = random_weights(10, 2, seed=13, scale=0.6)
    eng = _engine(gpu_engine_factory, w, 10)
    cell = getattr(cell_ref, name)
    rng = np.random.default_rng(n)
    mol = (cell_ref.random_cell(rng, n, cell),) + _features(rng, n, 10)
    ref = lambda xyz, x, Q, g, **kw: vjp64_cell(xyz, x, Q, g, cell, w, **kw)
    _check(eng, [mol], N, [ref], cell=cell)
    g = np.random.default_rng(1).normal(size=n).astype(np.float32)
    off = np.int32([0, n])
    q, gx, gs = eng.charges_vjp_xyz(off, mol[0], mol[1], np.float32([mol[2]]), g, N, cell=cell, strain=True)
    _, ref_x, ref_s = strain64(mol[0], mol[1], mol[2], g.astype(np.float64), cell, w, N=N)
    lo = strain64(mol[0], mol[1], mol[2], g.astype(np.float64), cell, w, N=N, kink_shift=+TAU)[2]
    hi = strain64(mol[0], mol[1], mol[2], g.astype(np.float64), cell, w, N=N, kink_shift=-TAU)[2]
    err, scale, kink = np.abs(gs[0] - ref_s).max(), np.abs(ref_s).max(), np.abs(lo - hi).max()
    print(f"gstrain {err:.3e} of {scale:.3e}, kink {kink:.3e}")
    assert err <= 2e-4 * scale + kink
    # gstrain_out = NULL: the same q and gxyz bits
    q2, gx2 = eng.charges_vjp_xyz(off, mol[0], mol[1], np.float32([mol[2]]), g, N, cell=cell)
    assert np.array_equal(q, q2) and np.array_equal(gx, gx2)
    eng.set_option("grad_path", 1)
    _, _, gs_d = eng.charges_vjp_xyz(off, mol[0], mol[1], np.float32([mol[2]]), g, N, cell=cell, strain=True)
    assert np.abs(gs - gs_d).max() <= 4e-4 * scale + kink


# ---------------------------------------------------------------------------------------------------- the two paths on 1500 atoms
def _paths_agree(eng, offsets, xyz, x, Q, g, N, kink, **geo):
    eng.set_option("grad_path", 1)
    q1, g1 = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, **geo)
    eng.set_option("grad_path", 2)
    q2, g2 = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, **geo)
    dd, scale = np.abs(g2 - g1).max(), np.abs(g1).max()
    print(f"pair-list path vs dense path: gxyz {dd:.3e} of {scale:.3e} (kink {kink:.3e}); q {np.abs(q2 - q1).max():.3e}")
    assert scale > 0 and dd <= 4e-4 * scale + kink
    assert np.abs(q2 - q1).max() <= 2e-4
    return q2, g2


def _weights_large(nx, seed, div):
    """random weights whose all-pairs sums over thousands of partners keep |h| at O(1), as in a trained model"""
    w = random_weights(nx, 2, seed=seed, scale=0.35)
    for t in range(2):
        w["msg"][t][2] = (w["msg"][t][2][0] / div, w["msg"][t][2][1] / div)
    return w


def test_paths_agree_on_a_1500_atom_cluster(gpu_engine_factory):
    from epnn_amd import synth
    offsets, xyz, x, Q, N = synth.box_system(n_atoms=1500, seed=0)
    w = random_weights(9, 2, seed=21, scale=0.35)
    eng = _engine(gpu_engine_factory, w, 9)
    g = np.random.default_rng(3).normal(size=1500).astype(np.float32)
    g64 = g.astype(np.float64)
    lo = vjp64_large(xyz, x, Q[0], g64, w, kink_shift=+TAU)[1]
    hi = vjp64_large(xyz, x, Q[0], g64, w, kink_shift=-TAU)[1]
    q2, g2 = _paths_agree(eng, offsets, xyz, x, Q, g, N, np.abs(lo - hi).max())
    q_ref, ref = vjp64_large(xyz, x, Q[0], g64, w)
    assert np.abs(q2 - q_ref).max() <= 2e-4
    assert np.abs(g2 - ref).max() <= 2e-4 * np.abs(ref).max() + np.abs(lo - hi).max()


def test_paths_agree_on_a_1500_atom_sheared_cell(gpu_engine_factory):
    from epnn_amd import synth
    offsets, xyz, x, Q, N, cell = synth.triclinic_cell_system(n_atoms=1500, seed=1)
    cell = np.asarray(cell, np.float32).reshape(3, 3)
    w = random_weights(9, 2, seed=22, scale=0.35)
    eng = _engine(gpu_engine_factory, w, 9)
    g = np.random.default_rng(4).normal(size=1500).astype(np.float32)
    g64 = g.astype(np.float64)
    lo = vjp64_large(xyz, x, Q[0], g64, w, cell=cell, kink_shift=+TAU)[1]
    hi = vjp64_large(xyz, x, Q[0], g64, w, cell=cell, kink_shift=-TAU)[1]
    _paths_agree(eng, offsets, xyz, x, Q, g, N, np.abs(lo - hi).max(), cell=cell)


# ---------------------------------------------------------------------------------------------------- larger systems
def test_box_4096_against_the_blocked_reference(gpu_engine_factory):
    """A 4096-atom periodic box against tests/grad_large_ref.py (its output for exactly these inputs is cached under tests/golden,
    keyed by a hash of the inputs; recomputed here when they differ)."""
    from golden import make_grad_large_fixtures as fx
    xyz, x, Q, box, g, w = fx.box4096_case()
    z = fx.load(xyz, x, Q, box, g, w)
    q_ref, ref, lo, hi = z if z is not None else fx.compute(xyz, x, Q, box, g, w)
    eng = _engine(gpu_engine_factory, w, 9)
    off = np.int32([0, 4096])
    q, gxyz = eng.charges_vjp_xyz(off, xyz, x, Q, g, 4096, box=box)
    q_fwd = eng.forward_xyz(off, xyz, x, Q, 4096, box=box)
    scale, kink, err = np.abs(ref).max(), np.abs(lo - hi).max(), np.abs(gxyz - ref).max()
    print(f"4096-atom box: q vs forward {np.abs(q - q_fwd).max():.3e}, vs reference {np.abs(q - q_ref).max():.3e}; "
          f"gxyz {err:.3e} of {scale:.3e}, kink {kink:.3e}")
    assert np.abs(q - q_fwd).max() <= 2e-4 and np.abs(q - q_ref).max() <= 2e-4
    assert scale > 0 and err <= 2e-4 * scale + kink


@pytest.mark.parametrize("kind", ["box", "cell"])
def test_20000_atoms_with_automatic_routing(gpu_engine_factory, kind):
    """A 20 000-atom periodic cell (800 M pair rows: the dense path would need 150 GB for gE alone) with grad_path = 0: the
    bounds of test_gpu_xyz_grad.test_invariants."""
    from epnn_amd import synth
    n = 20_000
    if kind == "box":
        offsets, xyz, x, Q, N, box = synth.periodic_box_system(n_atoms=n, seed=2)
        geo = {"box": np.asarray(box, np.float32).reshape(3)}
    else:
        offsets, xyz, x, Q, N, cell = synth.triclinic_cell_system(n_atoms=n, seed=2)
        geo = {"cell": np.asarray(cell, np.float32).reshape(3, 3)}
    w = _weights_large(9, 25, 256.0)
    eng = _engine(gpu_engine_factory, w, 9, path=0)
    g = np.random.default_rng(2).normal(size=n).astype(np.float32)
    strain = {"strain": True} if kind == "cell" else {}
    out = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N, **geo, **strain)
    q, gr = out[0], out[1]
    q_fwd = eng.forward_xyz(offsets, xyz, x, Q, N, **geo)
    print(f"{kind}: q vs forward_xyz {np.abs(q - q_fwd).max():.3e}; max |gxyz| {np.abs(gr).max():.3e}")
    assert np.isfinite(gr).all() and np.abs(q - q_fwd).max() <= 2e-4
    g1 = eng.charges_vjp_xyz(offsets, xyz, x, Q, np.ones(n, np.float32), N, **geo)[1]
    scale = np.abs(gr).max()
    assert scale > 0
    assert np.abs(g1).max() <= 1e-4 * scale
    assert np.abs(gr.astype(np.float64).sum(0)).max() <= 1e-4 * n * scale
    if kind == "cell":
        gs = out[2][0]
        assert np.abs(gs).max() > 0 and np.abs(gs - gs.T).max() <= 1e-6 * np.abs(gs).max()


# ---------------------------------------------------------------------------------------------------- contract
def _random_case(factory, nx=9, N=80, ns=(70, 45, 80), seed=11, path=2):
    w = random_weights(nx, 2, seed=seed, scale=0.6)
    mols = [_lattice_molecule(n, nx, seed=seed + n) for n in ns]
    return _engine(factory, w, nx, path=path), w, mols, _batch(mols)


def test_deterministic_and_batch_independent(gpu_engine_factory):
    eng, w, mols, (offsets, xyz, x, Q) = _random_case(gpu_engine_factory)
    g = np.random.default_rng(4).normal(size=int(offsets[-1])).astype(np.float32)
    q1, g1 = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 80)
    q2, g2 = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 80)
    assert np.array_equal(g1, g2) and np.array_equal(q1, q2)
    for b in range(len(mols)):
        a0, a1 = offsets[b], offsets[b + 1]
        qa, ga = eng.charges_vjp_xyz(np.int32([0, a1 - a0]), xyz[a0:a1], x[a0:a1], Q[b:b + 1], g[a0:a1], 80)
        assert np.array_equal(ga, g1[a0:a1]) and np.array_equal(qa, q1[a0:a1]), b


def test_diagonal_cell_is_the_box_and_zero_cell_is_open(gpu_engine_factory):
    w = random_weights(9, 2, seed=17, scale=0.6)
    eng = _engine(gpu_engine_factory, w, 9)
    rng = np.random.default_rng(4)
    L = np.float32([10.0, 9.0, 0.0])
    n = 100
    xyz = periodic_ref.random_cell(rng, n, L)
    x, Q = _features(rng, n, 9)
    g = rng.normal(size=n).astype(np.float32)
    off, Qa = np.int32([0, n]), np.float32([Q])
    qb, gb = eng.charges_vjp_xyz(off, xyz, x, Qa, g, n, box=L)
    qc, gc = eng.charges_vjp_xyz(off, xyz, x, Qa, g, n, cell=np.diag(L))
    assert np.array_equal(qb, qc) and np.array_equal(gb, gc)
    qo, go = eng.charges_vjp_xyz(off, xyz, x, Qa, g, n)
    qz, gz = eng.charges_vjp_xyz(off, xyz, x, Qa, g, n, cell=np.zeros((3, 3), np.float32))
    assert np.array_equal(qo, qz) and np.array_equal(go, gz)
    assert np.abs(go - gb).max() > 0


def test_training_state_untouched(gpu_engine_factory):
    from oracle import epnn_oracle_train as otr
    eng, w, mols, (offsets, xyz, x, Q) = _random_case(gpu_engine_factory, N=16, ns=(12, 9, 16))
    twin = gpu_engine_factory(nx=9, T=2)
    twin.set_weights(w)
    A = int(offsets[-1])
    y = np.random.default_rng(6).normal(size=A).astype(np.float32) * 0.2
    g = np.random.default_rng(7).normal(size=A).astype(np.float32)
    for e in (eng, twin):
        e.train_init()
        e.train_step_xyz(offsets, xyz, x, Q, y, 16, apply=False)
    grads = eng.get_gradients()
    weights = otr.flatten(eng.get_weights())
    q, gx = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 16)
    assert np.array_equal(eng.get_gradients(), grads)
    assert np.array_equal(otr.flatten(eng.get_weights()), weights)
    for e in (eng, twin):
        e.train_apply()
    assert np.array_equal(otr.flatten(eng.get_weights()), otr.flatten(twin.get_weights()))
    # Adam moments: a second step lands on the same weights in both
    for e in (eng, twin):
        e.train_step_xyz(offsets, xyz, x, Q, y, 16)
    assert np.array_equal(otr.flatten(eng.get_weights()), otr.flatten(twin.get_weights()))
    # after the updates the call uses the new weights, like the forward
    q2, _ = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 16)
    assert np.abs(q2 - eng.forward_xyz(offsets, xyz, x, Q, 16)).max() <= 2e-4
    assert np.abs(q2 - q).max() > 0


def test_errors_leave_the_handle_usable(gpu_engine_factory):
    from epnn_amd._lib import EpnnError
    eng, w, mols, (offsets, xyz, x, Q) = _random_case(gpu_engine_factory, N=16, ns=(12, 9, 16))
    A = int(offsets[-1])
    g = np.ones(A, np.float32)
    twin = xyz.copy()
    twin[5] = twin[2]
    with pytest.raises(EpnnError, match="coincide"):
        eng.charges_vjp_xyz(offsets, twin, x, Q, g, 16)
    L = np.float32([7.0, 7.0, 7.0])
    image = xyz[:12].copy()
    image[1] = np.float32([0.5, 0.25, 0.5])                     # (exact in float32 with the shift below)
    image[3] = np.float32([7.5, 0.25, -6.5])
    with pytest.raises(EpnnError, match="coincide"):
        eng.charges_vjp_xyz(np.int32([0, 12]), image, x[:12], Q[:1], g[:12], 16, box=L)
    with pytest.raises(EpnnError, match="grad_path"):
        eng.set_option("grad_path", 3)
    q, gx = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 16)
    assert np.isfinite(gx).all()
    assert np.abs(q - eng.forward_xyz(offsets, xyz, x, Q, 16)).max() <= 2e-4
    # a partitioned handle: refused on grad_path = 2, the dense path under automatic routing
    eng.set_partition(0, 2, exchange=lambda *a: None)
    with pytest.raises(EpnnError, match="partition"):
        eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 16)
    eng.set_option("grad_path", 0)
    q0, gx0 = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 16)
    eng.set_partition(0, 1)
    eng.set_option("grad_path", 2)
    q1, gx1 = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 16)
    assert np.array_equal(q1, q) and np.array_equal(gx1, gx)
    assert np.isfinite(gx0).all() and np.abs(q0 - q).max() <= 2e-4


def test_other_update_layers_are_refused(gpu_engine_factory):
    from epnn_amd._lib import EpnnError
    w = random_weights(9, 2, seed=9, scale=0.6)
    rng = np.random.default_rng(3)

    def dense(i, o):
        lim = 0.6 * np.sqrt(6.0 / (i + o))
        return rng.uniform(-lim, lim, (i, o)).astype(np.float32), rng.uniform(-0.1, 0.1, (o,)).astype(np.float32)

    w["upd"] = [dense(48 + 32, 64), dense(64, 48)]
    mols = [_lattice_molecule(n, 9, seed=30 + n) for n in (7, 10)]
    offsets, xyz, x, Q = _batch(mols)
    g = np.ones(int(offsets[-1]), np.float32)
    eng = gpu_engine_factory(nx=9, T=2)
    eng.set_weights(w)
    eng.set_option("grad_path", 2)
    with pytest.raises(EpnnError, match=r"\[32, 32\]"):
        eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 12)
    eng.set_option("grad_path", 0)
    q, gx = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 12)
    assert np.isfinite(gx).all() and np.abs(q - eng.forward_xyz(offsets, xyz, x, Q, 12)).max() <= 2e-4


def test_routing_below_the_threshold_is_the_dense_path(gpu_engine_factory):
    eng, w, mols, (offsets, xyz, x, Q) = _random_case(gpu_engine_factory, path=0)
    g = np.random.default_rng(8).normal(size=int(offsets[-1])).astype(np.float32)
    q0, g0 = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 80)
    eng.set_option("grad_path", 1)
    q1, g1 = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 80)
    assert np.array_equal(q0, q1) and np.array_equal(g0, g1)
    eng.set_option("grad_path", 2)
    q2, g2 = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 80)
    assert not np.array_equal(g2, g1)


def test_three_entries_share_one_handle(gpu_engine_factory):
    """The gradient call, the JVP and the pair-list train step share the handle's GradLarge buffers: a smaller call after a larger
    one, and one entry after another, see nothing of the previous call.  Four calls on one engine against the same four on a fresh
    engine each: every output bit and the listed pairs."""
    from test_gpu_train_cell import _batch as _train_batch, _periodic_case
    nx, w, mols, cells, N = _periodic_case("batch")
    t_off, t_xyz, t_x, t_Q, t_y, t_cell = _train_batch(mols, cells)
    big, small = _lattice_molecule(300, nx, seed=300), _lattice_molecule(17, nx, seed=17)
    rng = np.random.default_rng(12)
    g300, g17, v17 = (rng.normal(size=s).astype(np.float32) for s in (300, 17, (17, 3)))

    def vjp(eng, mol, g, N):
        return eng.charges_vjp_xyz(np.int32([0, len(g)]), mol[0], mol[1], np.float32([mol[2]]), g, N)

    def step(eng):
        q, loss = eng.train_step_xyz(t_off, t_xyz, t_x, t_Q, t_y, N, apply=False, cell=t_cell)
        return q, np.float32(loss), eng.get_gradients()

    calls = [lambda e: vjp(e, big, g300, 300),
             lambda e: e.charges_jvp_xyz(np.int32([0, 17]), small[0], small[1], np.float32([small[2]]), 24, v=v17, dQ=1.0),
             step,
             lambda e: vjp(e, small, g17, 24)]

    def engine():
        eng = _engine(gpu_engine_factory, w, nx)
        eng.set_option("train_path", 2)
        eng.train_init()
        return eng

    shared = engine()
    for k, call in enumerate(calls):
        got, pairs = call(shared), int(shared.last_stats()[0])
        fresh = engine()
        want = call(fresh)
        assert pairs == int(fresh.last_stats()[0]) and pairs > 0, k
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want)), k


def test_reverse_entries_share_one_backward(gpu_engine_factory):
    """The train step, the single VJP, the Coulomb call and the K = 3 VJP run one set of backward kernels on one scratch buffer, with
    tape pointers (the train step) or without, one cotangent or three.  On one handle: train step, VJP, Coulomb, VJP at K = 3, then the
    first three again; each call gives the bits of the same call on a fresh handle.  Molecules of 1, 2 (atoms 50 A apart: no listed
    pair), 17 and 40 atoms in one batch."""
    from test_gpu_train_cell import ZERO
    w = random_weights(9, 2, seed=5, scale=0.6)
    far = _lattice_molecule(2, 9, seed=2)
    far[0][1] = far[0][0] + np.float32([50.0, 0.0, 0.0])
    offsets, xyz, x, Q = _batch([_lattice_molecule(1, 9, seed=1), far, _lattice_molecule(17, 9, seed=17), _lattice_molecule(40, 9, seed=40)])
    A, N = int(offsets[-1]), 40
    rng = np.random.default_rng(27)
    g, y = rng.normal(size=(3, A)).astype(np.float32), rng.normal(scale=0.3, size=A).astype(np.float32)

    def step(eng):
        q, loss = eng.train_step_xyz(offsets, xyz, x, Q, y, N, apply=False, cell=ZERO)
        return q, np.float32(loss), eng.get_gradients()

    first = [step,
             lambda e: e.charges_vjp_xyz(offsets, xyz, x, Q, g[0], N),
             lambda e: e.coulomb_xyz(offsets, xyz, x, Q, N, parts=True)]
    calls = first + [lambda e: e.charges_vjp_xyz_multi(offsets, xyz, x, Q, g, N, strain=True)] + first

    def engine():
        eng = _engine(gpu_engine_factory, w, 9)
        eng.set_option("train_path", 2)
        eng.train_init()
        return eng

    shared = engine()
    wants = {}
    for k, call in enumerate(calls):
        got, stats = call(shared), shared.last_stats()
        if call not in wants:
            fresh = engine()
            wants[call] = (call(fresh), fresh.last_stats())
        want, want_stats = wants[call]
        assert int(stats[0]) > 0 and int(stats[0]) == int(want_stats[0]), k
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want)), k
        assert all(np.isfinite(np.asarray(a, dtype=np.float64)).all() for a in got), k


def test_box_rows_on_the_pair_list_path(gpu_engine_factory):
    """The single VJP with box= on the pair-list path (the box instance of the coordinate kernel, K = 1 only) on a 20-atom box against
    the periodic float64 VJP, at the tolerance of test_gpu_periodic.test_charge_gradients_in_cells: q within 2e-4, gxyz within
    2e-4 max |ref| + the ReLU-kink bracket."""
    w = random_weights(9, 2, seed=6, scale=0.5)
    eng = _engine(gpu_engine_factory, w, 9)
    rng = np.random.default_rng(320)
    L = np.float32([6.0, 6.5, 7.0])
    mol = (periodic_ref.random_cell(rng, 20, L),) + _features(rng, 20, 9)
    ref = lambda xyz, x, Q, g, **kw: vjp64_pbc(xyz, x, Q, g, L, w, **kw)
    _check(eng, [mol], 24, [ref], both_paths=False, box=L)
