"""epnn_charges_vjp_multi_xyz_cell (Engine.charges_vjp_xyz_multi, dipole_xyz) on the GPU: every row bit for bit the single entry's on
"grad_path" 2, independence of K, position, the other rows and the rest of the batch, the float64 reference on 1500 atoms, the
adjoint identity against charges_jvp_xyz_multi as a matrix, edge cases, the contract, the scratch formula, dipoles and atomic polar
tensors.  GPU only.  No tolerance of its own: bit equality, or the rule an existing test applies to the single entry."""
import functools

import numpy as np
import pytest

import cell_ref
from conftest import random_weights
from grad_large_ref import vjp64_large
from test_gpu_grad_large import TAU, _batch, _lattice_molecule
from test_gpu_jvp import _case, _engine, _engine_for

pytestmark = pytest.mark.gpu

CASES = ["lattice-2-8", "lattice-15-16", "lattice-16-16", "lattice-17-24", "lattice-33-40", "slab", "box", "batch3", "hdim20"]
KS = (1, 2, 3, 5, 16)


@functools.lru_cache(maxsize=None)
def _cotangents(name):
    offsets = _batch(_case(name)[2])[0]
    return np.random.default_rng(500 + len(name)).normal(size=(16, int(offsets[-1]))).astype(np.float32)


def _cell_geo(geo):
    """strain=True takes the cell as cell=: a box as its diagonal cell (the bits of the box entry by the contract of include/epnn.h)"""
    return {"cell": np.diag(geo["box"])} if "box" in geo else geo


def _singles(eng, offsets, xyz, x, Q, g, N, geo, strain=True):
    """charges_vjp_xyz per row of g on grad_path 2: q, gxyz (K, A, 3)[, gstrain (K, B, 3, 3)]"""
    outs = [eng.charges_vjp_xyz(offsets, xyz, x, Q, gk, N, strain=strain, **geo) for gk in g]
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0])
    return (outs[0][0],) + tuple(np.stack([o[k] for o in outs]) for k in range(1, len(outs[0])))


# ---------------------------------------------------------------------------------------------------- 1, 2: row bits
@pytest.mark.parametrize("name", CASES)
def test_row_bits(gpu_engine_factory, name):
    w, nx, mols, N, geo, _ = _case(name)
    offsets, xyz, x, Q = _batch(mols)
    g = _cotangents(name)
    eng = _engine_for(gpu_engine_factory, name)
    cg = _cell_geo(geo)
    q1, gx1, gs1 = _singles(eng, offsets, xyz, x, Q, g, N, cg)
    assert gx1.any() and gs1.any() and all(gx1[k].any() for k in range(16))
    for K in KS:
        q, gx, gs = eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, g[:K], N, strain=True, **cg)
        assert gx.shape == (K, int(offsets[-1]), 3) and gs.shape == (K, len(mols), 3, 3)
        assert np.array_equal(q, q1), K
        for k in range(K):
            assert np.array_equal(gx[k], gx1[k]) and np.array_equal(gs[k], gs1[k]), (K, k)
    if "box" in geo:                                               # box= is its diagonal cell; the single box entry's bits
        q, gx = eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, g[:3], N, **geo)
        for k in range(3):
            qb, gb = eng.charges_vjp_xyz(offsets, xyz, x, Q, g[k], N, **geo)
            assert np.array_equal(q, qb) and np.array_equal(gx[k], gb), k


@pytest.mark.parametrize("name", ["lattice-17-24", "slab", "batch3"])
def test_without_strain_the_same_bits(gpu_engine_factory, name):
    w, nx, mols, N, geo, _ = _case(name)
    offsets, xyz, x, Q = _batch(mols)
    g = _cotangents(name)[:5]
    eng = _engine_for(gpu_engine_factory, name)
    q, gx, gs = eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, g, N, strain=True, **geo)
    q2, gx2 = eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, g, N, **geo)
    assert np.array_equal(q, q2) and np.array_equal(gx, gx2) and gx.any()
    q1, gx1 = _singles(eng, offsets, xyz, x, Q, g, N, geo, strain=False)
    assert np.array_equal(q, q1) and np.array_equal(gx, gx1)


# ---------------------------------------------------------------------------------------------------- 3: independence
def test_rows_do_not_depend_on_K_position_neighbours_repeats_or_the_batch(gpu_engine_factory):
    w, nx, mols, N, geo, _ = _case("batch3")
    offsets, xyz, x, Q = _batch(mols)
    g = _cotangents("batch3")
    eng = _engine_for(gpu_engine_factory, "batch3")
    call = lambda rows: eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, rows, N, strain=True)
    q, gx, gs = call(g[:7])                                        # (chunks 4 + 2 + 1)
    assert all(gx[k].any() and gs[k].any() for k in range(7))
    q2, gx2, gs2 = call(g[:7])
    assert np.array_equal(q, q2) and np.array_equal(gx, gx2) and np.array_equal(gs, gs2)
    perm = np.array([4, 0, 6, 2, 5, 1, 3])
    qp, gxp, gsp = call(g[perm])
    assert np.array_equal(qp, q) and np.array_equal(gxp, gx[perm]) and np.array_equal(gsp, gs[perm])
    for K in (1, 2, 4, 16):                                        # row 3 first, among other rows, in every chunk width
        rows = np.concatenate([g[3:4], g[8:8 + K - 1]])
        _, gxk, gsk = call(rows)
        assert np.array_equal(gxk[0], gx[3]) and np.array_equal(gsk[0], gs[3]), K
    other = g[:7].copy()
    other[[0, 1, 2, 4, 5, 6]] *= np.float32(-3.5)                  # what the other rows hold
    _, gxo, gso = call(other)
    assert np.array_equal(gxo[3], gx[3]) and np.array_equal(gso[3], gs[3])
    for b in range(len(mols)):                                     # each molecule alone at the same N
        a0, a1 = offsets[b], offsets[b + 1]
        qa, gxa, gsa = eng.charges_vjp_xyz_multi(np.int32([0, a1 - a0]), xyz[a0:a1], x[a0:a1], Q[b:b + 1], g[:7, a0:a1], N, strain=True)
        assert np.array_equal(qa, q[a0:a1]) and np.array_equal(gxa, gx[:, a0:a1]) and np.array_equal(gsa[:, 0], gs[:, b]), b


# ---------------------------------------------------------------------------------------------------- 4: 1500 atoms
@pytest.mark.parametrize("kind", ["cluster", "cell"])
def test_1500_atoms_row_bits_and_the_float64_reference(gpu_engine_factory, kind):
    """Many tiles, all pieces in use.  Row 0 under the rule of test_gpu_grad_large.py for the single entry there:
    |gxyz - ref| <= 2e-4 max |ref| + kink bracket, q within 2e-4."""
    from epnn_amd import synth
    if kind == "cluster":
        offsets, xyz, x, Q, N = synth.box_system(n_atoms=1500, seed=0)
        geo, w = {}, random_weights(9, 2, seed=21, scale=0.35)
    else:
        offsets, xyz, x, Q, N, cell = synth.triclinic_cell_system(n_atoms=1500, seed=1)
        geo, w = {"cell": np.asarray(cell, np.float32).reshape(3, 3)}, random_weights(9, 2, seed=22, scale=0.35)
    eng = _engine(gpu_engine_factory, w, 9)
    g = np.random.default_rng(3 if kind == "cluster" else 4).normal(size=(3, 1500)).astype(np.float32)
    q, gx, gs = eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, g, N, strain=True, **geo)
    q1, gx1, gs1 = _singles(eng, offsets, xyz, x, Q, g, N, geo)
    assert np.array_equal(q, q1) and np.array_equal(gx, gx1) and np.array_equal(gs, gs1)
    assert all(gx[k].any() and gs[k].any() for k in range(3))
    g64 = g[0].astype(np.float64)
    q_ref, ref = vjp64_large(xyz, x, Q[0], g64, w, **geo)
    lo = vjp64_large(xyz, x, Q[0], g64, w, kink_shift=+TAU, **geo)[1]
    hi = vjp64_large(xyz, x, Q[0], g64, w, kink_shift=-TAU, **geo)[1]
    err, scale, kink = np.abs(gx[0] - ref).max(), np.abs(ref).max(), np.abs(lo - hi).max()
    print(f"{kind}: q {np.abs(q - q_ref).max():.3e}; gxyz row 0 {err:.3e} of {scale:.3e}, kink {kink:.3e}")
    assert np.abs(q - q_ref).max() <= 2e-4
    assert scale > 0 and err <= 2e-4 * scale + kink


# ---------------------------------------------------------------------------------------------------- 5: the adjoint identity
@pytest.mark.parametrize("name", ["batch3", "basis_a"])
def test_adjoint_identity_as_a_matrix(gpu_engine_factory, name):
    """sum_i g[k][i] tq[m][i] = gxyz[k] . v[m] + gstrain[k] : E[m] for all nine (k, m), per molecule, under the bound of
    test_gpu_jvp._adjoint on each entry; the dQ tangents are zero (dF/dQ, the adjoint of vQ, is not an output of the entry)."""
    w, nx, mols, N, geo, _ = _case(name)
    offsets, xyz, x, Q = _batch(mols)
    A, B = int(offsets[-1]), len(mols)
    rng = np.random.default_rng(77)
    g = rng.normal(size=(3, A)).astype(np.float32)
    v = rng.normal(size=(3, A, 3)).astype(np.float32)
    E = (0.3 * rng.normal(size=(3, B, 3, 3))).astype(np.float32)
    eng = _engine_for(gpu_engine_factory, name)
    q, gx, gs = eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, g, N, strain=True, **geo)
    q2, tq = eng.charges_jvp_xyz_multi(offsets, xyz, x, Q, N, v=v, strain=E, dQ=np.zeros((3, B), np.float32), **geo)
    assert np.array_equal(q, q2)
    g64, t64, gx64, gs64, v64, E64 = (a.astype(np.float64) for a in (g, tq, gx, gs, v, E))
    for b in range(B):
        a0, a1 = offsets[b], offsets[b + 1]
        for k in range(3):
            for m in range(3):
                lhs = g64[k, a0:a1] @ t64[m, a0:a1]
                rhs = (gx64[k, a0:a1] * v64[m, a0:a1]).sum() + (gs64[k, b] * E64[m, b]).sum()
                bound = 2e-4 * (np.abs(g64[k, a0:a1]).sum() * np.abs(t64[m, a0:a1]).max() +
                                np.abs(v64[m, a0:a1]).sum() * np.abs(gx64[k, a0:a1]).max() + np.abs(E64[m, b]).sum() * np.abs(gs64[k, b]).max())
                print(f"molecule {b}, (k, m) = ({k}, {m}): g.tq {lhs:.6e}, gxyz.v + gstrain:E {rhs:.6e}, difference {abs(lhs - rhs):.3e}, bound {bound:.3e}")
                assert abs(lhs - rhs) <= bound and abs(lhs) > 0, (b, k, m, lhs, rhs, bound)


# ---------------------------------------------------------------------------------------------------- 6: edge cases
def test_a_lone_atom_and_two_atoms_without_a_listed_pair(gpu_engine_factory):
    w = random_weights(9, 2, seed=5, scale=0.6)
    eng = _engine(gpu_engine_factory, w, 9)
    xyz, x, Q = _lattice_molecule(1, 9, seed=1)
    g = np.float32([[1.5], [-2.0], [0.25]])
    q, gx, gs = eng.charges_vjp_xyz_multi(np.int32([0, 1]), xyz, x, np.float32([Q]), g, 4, strain=True)
    assert q[0] == Q and gx.shape == (3, 1, 3) and not gx.any() and not gs.any()
    xyz, x, Q = _lattice_molecule(2, 9, seed=2)
    xyz = np.float32([[0.0, 0.0, 0.0], [10.0, 0.0, 0.0]])
    off, Qa = np.int32([0, 2]), np.float32([Q])
    g = np.random.default_rng(8).normal(size=(3, 2)).astype(np.float32)
    q, gx, gs = eng.charges_vjp_xyz_multi(off, xyz, x, Qa, g, 8, strain=True)
    assert int(eng.last_stats()[0]) == 0
    q1, gx1, gs1 = _singles(eng, off, xyz, x, Qa, g, 8, {})
    assert np.array_equal(q, q1) and np.array_equal(gx, gx1) and np.array_equal(gs, gs1)


def test_a_batch_mixing_an_all_zero_cell_with_a_sheared_cell(gpu_engine_factory):
    w = random_weights(10, 2, seed=13, scale=0.6)
    eng = _engine(gpu_engine_factory, w, 10)
    rng = np.random.default_rng(90)
    from test_gpu_grad_large import _features
    mols = [_lattice_molecule(33, 10, seed=33), (cell_ref.random_cell(rng, 60, cell_ref.SHEARED),) + _features(rng, 60, 10)]
    offsets, xyz, x, Q = _batch(mols)
    cells = np.stack([np.zeros((3, 3), np.float32), np.asarray(cell_ref.SHEARED, np.float32)])
    g = rng.normal(size=(3, int(offsets[-1]))).astype(np.float32)
    q, gx, gs = eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, g, 64, cell=cells, strain=True)
    q1, gx1, gs1 = _singles(eng, offsets, xyz, x, Q, g, 64, {"cell": cells})
    assert np.array_equal(q, q1) and np.array_equal(gx, gx1) and np.array_equal(gs, gs1)
    assert all(gs[k, b].any() for k in range(3) for b in range(2))


# ---------------------------------------------------------------------------------------------------- 7: contract
def _random_case(factory, nx=9, ns=(12, 9, 16), seed=11):
    w = random_weights(nx, 2, seed=seed, scale=0.6)
    mols = [_lattice_molecule(n, nx, seed=seed + n) for n in ns]
    return _engine(factory, w, nx), w, mols, _batch(mols)


def test_refusals_leave_the_handle_usable(gpu_engine_factory):
    from epnn_amd._lib import EpnnError, check, fptr, iptr
    eng, w, mols, (offsets, xyz, x, Q) = _random_case(gpu_engine_factory)
    A = int(offsets[-1])
    g = np.random.default_rng(3).normal(size=(17, A)).astype(np.float32)
    q, gx = eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, g[:3], 16)

    def still_serves():
        q1, gx1 = eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, g[:3], 16)
        assert np.array_equal(q1, q) and np.array_equal(gx1, gx)

    for K in (0, 17):
        with pytest.raises(EpnnError, match=r"epnn_charges_vjp_multi_xyz_cell: K must be in 1\.\.16"):
            eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, g[:K], 16)
        still_serves()
    out_q, out_g = np.empty(A, np.float32), np.empty((3, A, 3), np.float32)
    with pytest.raises(EpnnError, match="epnn_charges_vjp_multi_xyz_cell: null"):          # (a null g, through the binding)
        check(eng.lib.epnn_charges_vjp_multi_xyz_cell(eng.h, 3, 16, iptr(offsets), fptr(xyz), fptr(x), fptr(Q), None, 3, None, fptr(out_q),
                                                      fptr(out_g), None), eng.lib)
    still_serves()
    twin = xyz.copy()
    twin[5] = twin[2]
    with pytest.raises(EpnnError, match="epnn_charges_vjp_multi_xyz_cell.*coincide"):
        eng.charges_vjp_xyz_multi(offsets, twin, x, Q, g[:3], 16)
    still_serves()
    with pytest.raises(EpnnError, match="does not fit"):
        eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, g[:3], 12)
    with pytest.raises(EpnnError, match="offsets"):
        eng.charges_vjp_xyz_multi(np.int32([1, 12, 21, 37]), xyz, x, Q, g[:3], 16)
    with pytest.raises(ValueError, match=r"g must have shape \(K, 37\)"):
        eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, g[0], 16)
    with pytest.raises(ValueError, match=r"g must have shape \(K, 37\)"):
        eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, g[:3, :30], 16)
    still_serves()
    eng.set_partition(0, 2, exchange=lambda *a: None)
    with pytest.raises(EpnnError, match="epnn_charges_vjp_multi_xyz_cell.*partition"):
        eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, g[:3], 16)
    eng.set_partition(0, 1)
    still_serves()
    eng.set_option("grad_path", 1)                                 # the entry runs from the pair list whatever grad_path says
    still_serves()
    assert np.abs(q - eng.forward_xyz(offsets, xyz, x, Q, 16)).max() <= 2e-4


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
    eng = gpu_engine_factory(nx=9, T=2)
    eng.set_weights(w)
    with pytest.raises(EpnnError, match=r"epnn_charges_vjp_multi_xyz_cell.*\[32, 32\]"):
        eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, np.ones((2, 17), np.float32), 12)
    assert np.isfinite(eng.forward_xyz(offsets, xyz, x, Q, 12)).all()


def test_training_state_untouched(gpu_engine_factory):
    """test_gpu_grad_large.test_training_state_untouched with the K-cotangent call in the single call's place"""
    from oracle import epnn_oracle_train as otr
    eng, w, mols, (offsets, xyz, x, Q) = _random_case(gpu_engine_factory)
    twin = gpu_engine_factory(nx=9, T=2)
    twin.set_weights(w)
    A = int(offsets[-1])
    y = np.random.default_rng(6).normal(size=A).astype(np.float32) * 0.2
    g = np.random.default_rng(7).normal(size=(3, A)).astype(np.float32)
    for e in (eng, twin):
        e.train_init()
        e.train_step_xyz(offsets, xyz, x, Q, y, 16, apply=False)
    grads = eng.get_gradients()
    weights = otr.flatten(eng.get_weights())
    q, gx = eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, g, 16)
    assert np.array_equal(eng.get_gradients(), grads)
    assert np.array_equal(otr.flatten(eng.get_weights()), weights)
    for e in (eng, twin):
        e.train_apply()
    assert np.array_equal(otr.flatten(eng.get_weights()), otr.flatten(twin.get_weights()))
    for e in (eng, twin):                                          # Adam moments: a second step lands on the same weights in both
        e.train_step_xyz(offsets, xyz, x, Q, y, 16)
    assert np.array_equal(otr.flatten(eng.get_weights()), otr.flatten(twin.get_weights()))
    q2, gx2 = eng.charges_vjp_xyz_multi(offsets, xyz, x, Q, g, 16)   # the new weights, like the forward
    assert np.abs(q2 - eng.forward_xyz(offsets, xyz, x, Q, 16)).max() <= 2e-4
    assert np.abs(q2 - q).max() > 0 and np.abs(gx2 - gx).max() > 0


def test_served_between_forward_begin_and_end(gpu_engine_factory):
    eng, w, mols, (offsets, xyz, x, Q) = _random_case(gpu_engine_factory)
    g = np.random.default_rng(9).normal(size=(3, int(offsets[-1]))).astype(np.float32)
    want_q = eng.forward_xyz(offsets, xyz, x, Q, 16)
    want = eng.charges_vjp_xyz_multi(offsets[:2], xyz[:12], x[:12], Q[:1], g[:, :12], 16)
    eng.forward_xyz_begin(offsets, xyz, x, Q, 16)
    got = eng.charges_vjp_xyz_multi(offsets[:2], xyz[:12], x[:12], Q[:1], g[:, :12], 16)
    assert np.array_equal(eng.forward_xyz_end(), want_q)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[1].any()


def test_the_model_method(gpu_engine_factory):
    from epnn_amd import charge_gn
    w = random_weights(9, 2, seed=5, scale=0.6)
    xyz, x, Q = _lattice_molecule(17, 9, seed=17)
    model = charge_gn.make_model([32, 32], 48, 2, 9, 24)
    model.set_weights_dict(w)
    off, Qa = np.int32([0, 17]), np.float32([Q])
    g = np.random.default_rng(117).normal(size=(2, 17)).astype(np.float32)
    q, gx, gs = model.charges_vjp_xyz_multi(off, xyz, x, Qa, g, strain=True)
    eng = _engine(gpu_engine_factory, w, 9)
    q2, gx2, gs2 = eng.charges_vjp_xyz_multi(off, xyz, x, Qa, g, 24, strain=True)
    assert np.array_equal(q, q2) and np.array_equal(gx, gx2) and np.array_equal(gs, gs2) and gx.any()


# ---------------------------------------------------------------------------------------------------- 8: scratch
BUFFERS = 43      # 14 staged inputs and counts, 10 of the pair list, 19 rows (11 of them K-fold): 256 bytes each


def _formula(ns, nx, T, pairs, K, B):
    """include/epnn.h: bytes = A (744 + 4 nx + 324 T + pieces + K (580 + 256 pieces)) + (268 + 848 K) listed pairs + 36 K B + 13 KB"""
    pieces = max(min(16, max(1, -(-2048 // -(-n // 16)))) for n in ns)
    return sum(ns) * (744 + 4 * nx + 324 * T + pieces + K * (580 + 256 * pieces)) + (268 + 848 * K) * pairs + 36 * K * B + 13 * 1024


def test_scratch_follows_the_formula(gpu_engine_factory):
    w = random_weights(9, 2, seed=5, scale=0.6)
    eng = _engine(gpu_engine_factory, w, 9)
    xyz, x, Q = _lattice_molecule(304, 9, seed=300)
    off, Qa = np.int32([0, 304]), np.float32([Q])
    g = np.random.default_rng(1).normal(size=(16, 304)).astype(np.float32)
    eng.charges_vjp_xyz(off, xyz, x, Qa, g[0], 304)
    pairs = int(eng.last_stats()[0])
    for K in (1, 3, 16):
        eng.charges_vjp_xyz_multi(off, xyz, x, Qa, g[:K], 304, strain=True)
        st = eng.last_stats()
        want = _formula([304], 9, 2, pairs, K, 1)
        print(f"304 atoms, K = {K}: {st[0]} pairs, {st[2]} bytes, formula {want}, difference {int(st[2]) - want}")
        assert st[0] == pairs and pairs > 0 and st[1] == 0
        assert abs(int(st[2]) - want) <= 256 * BUFFERS


# ---------------------------------------------------------------------------------------------------- 9: dipoles and polar tensors
def _charged():
    xyz, x, _ = _lattice_molecule(17, 9, seed=17)
    return [(xyz, x, np.float32(2.0))]


@pytest.mark.parametrize("name", ["batch3", "charged"])
def test_dipole_xyz(gpu_engine_factory, name):
    if name == "charged":
        w, nx, mols, N = random_weights(9, 2, seed=5, scale=0.6), 9, _charged(), 24
        eng = _engine(gpu_engine_factory, w, nx)
    else:
        w, nx, mols, N = _case(name)[:4]
        eng = _engine_for(gpu_engine_factory, name)
    offsets, xyz, x, Q = _batch(mols)
    B, A = len(mols), int(offsets[-1])
    mol = np.repeat(np.arange(B), np.diff(offsets))
    r = xyz.astype(np.float64)
    cen = np.stack([r[offsets[b]:offsets[b + 1]].mean(axis=0) for b in range(B)])
    for origin in (None, np.array([0.5, -1.0, 2.0]), cen + 0.25):
        o = cen if origin is None else np.broadcast_to(np.asarray(origin, np.float64), (B, 3))
        q, mu, apt = eng.dipole_xyz(offsets, xyz, x, Q, N, origin=origin)
        assert q.dtype == np.float32 and mu.dtype == np.float64 and mu.shape == (B, 3) and apt.dtype == np.float32 and apt.shape == (A, 3, 3)
        rel = r - o[mol]
        seeds = rel.T.astype(np.float32)
        single = np.zeros((A, 3, 3), np.float32)
        for a in range(3):
            q1, gx1 = eng.charges_vjp_xyz(offsets, xyz, x, Q, seeds[a], N)
            assert np.array_equal(q, q1)
            single[:, a, :] = gx1
            single[:, a, a] += q1
        assert np.array_equal(apt, single) and apt.any()
        for b in range(B):
            a0, a1 = offsets[b], offsets[b + 1]
            assert np.array_equal(mu[b], (q[a0:a1].astype(np.float64)[:, None] * rel[a0:a1]).sum(axis=0)), b
            rule = np.abs(apt[a0:a1].astype(np.float64).sum(0) - float(Q[b]) * np.eye(3)).max()
            rule1 = np.abs(single[a0:a1].astype(np.float64).sum(0) - float(Q[b]) * np.eye(3)).max()
            print(f"{name}, molecule {b} (n = {a1 - a0}, Q = {Q[b]}): |sum_i apt[i] - Q I| {rule:.3e} (three single calls: {rule1:.3e}), |mu| {np.abs(mu[b]).max():.3e}")
            assert rule <= rule1
    with pytest.raises(TypeError):
        eng.dipole_xyz(offsets, xyz, x, Q, N, box=np.float32([12.0, 12.0, 12.0]))
    with pytest.raises(ValueError, match="origin"):
        eng.dipole_xyz(offsets, xyz, x, Q, N, origin=np.zeros((B + 1, 3)))
    from epnn_amd import charge_gn
    if name == "charged":
        model = charge_gn.make_model([32, 32], 48, 2, 9, N)
        model.set_weights_dict(w)
        qm, mum, aptm = model.dipole_xyz(offsets, xyz, x, Q)
        q, mu, apt = eng.dipole_xyz(offsets, xyz, x, Q, N)
        assert np.array_equal(qm, q) and np.array_equal(mum, mu) and np.array_equal(aptm, apt)
