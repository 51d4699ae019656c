"""Training steps on periodic cells and from the pair list (epnn_train_step_xyz_cell, option "train_path") on the GPU: against the
float64 oracle on both paths, the pair-list path at its tile edges, 600-atom systems against a stored float64 reference, an Adam
trajectory, bit identities, the interface and its refusals, and a 20 000-atom cell under automatic routing.  GPU only.  Without the
feature every test fails: train_step_xyz takes no box= / cell= and there is no "train_path".

Gradient tolerance everywhere (the rule of test_gpu_train.test_gradients_match_oracle_at_config3_shape): per parameter tensor
err <= max(2e-4, 4 noise) + 2 kink of the tensor's largest float64 entry, noise = the float32 oracle against the float64 one, kink =
the ReLU bracket at tau = 2e-6 (summed over the oracle's three row sets); exact zeros where the oracle's are zero; loss to 2e-5
relative, predictions to 2e-5."""
import numpy as np
import pytest

import cell_ref
from conftest import load_molecules, random_weights
from oracle import epnn_oracle as orc
from oracle import epnn_oracle_train as ot

pytestmark = pytest.mark.gpu

TAU = 2e-6
ZERO = np.zeros((3, 3), np.float32)
CUBIC = np.diag(np.float32([6.5, 6.5, 6.5]))
SLAB = np.float32([[7.0, 0, 0], [1.0, 6.8, 0], [0, 0, 0]])                  # one zero row: periodic in the plane, open along z


def _features(rng, n, nx):
    x = np.zeros((n, nx), dtype=np.float32)
    el = rng.integers(0, nx - 1, n)
    x[np.arange(n), 1 + el] = 1.0
    x[:, 0] = np.array([1, 6, 7, 8, 9, 15, 16, 17, 35])[el % 9]
    return x, np.float32(rng.integers(-1, 2))


def _system(n, nx, cell, seed):
    """(xyz, x, Q, y) of n atoms: random positions in the cell, or (all-zero cell) a jittered lattice."""
    rng = np.random.default_rng(seed)
    if np.any(cell):
        xyz = cell_ref.random_cell(rng, n, cell)
    else:
        k = int(np.ceil(n ** (1 / 3)))
        grid = np.array([(a, b, c) for a in range(k) for b in range(k) for c in range(k)], dtype=np.float64)[:n] * 1.2
        xyz = (grid + rng.uniform(-0.15, 0.15, grid.shape)).astype(np.float32)
    x, Q = _features(rng, n, nx)
    return xyz, x, Q, rng.normal(scale=0.3, size=n).astype(np.float32)


def _batch(mols, cells):
    offsets = np.zeros(len(mols) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([m[0].shape[0] for m in mols])
    return (offsets, np.concatenate([m[0] for m in mols]), np.concatenate([m[1] for m in mols]),
            np.array([m[2] for m in mols], dtype=np.float32), np.concatenate([m[3] for m in mols]).astype(np.float32),
            np.stack([np.asarray(c, np.float32) for c in cells]))


def _dense(mols, cells, N, h_dim=48):
    """The dense make_model inputs of the batch padded to N, with the cells' minimum-image edges."""
    parts, yd = [], np.zeros((len(mols), N, 1))
    for b, ((xyz, x, Q, y), cell) in enumerate(zip(mols, cells)):
        n = x.shape[0]
        d = list(orc.dense_inputs(xyz, x, Q, N, h_dim=h_dim, e_dim=h_dim))
        d[1][:n, :n] = cell_ref.get_init_edges_cell(xyz, cell, num=h_dim)[0]
        parts.append(d)
        yd[b, :n, 0] = y
    return [np.stack([p[k] for p in parts]) for k in range(5)] + [yd]


_ORACLE = {}


def _oracle(key, mols, cells, N, w, h_dim=48):
    """(loss, predictions (B, N), flat gradient, flat float32-oracle gradient, flat kink band), computed once per case."""
    if key not in _ORACLE:
        h, e, x, q, mask, y = _dense(mols, cells, N, h_dim)
        loss, pred, g = ot.loss_and_grads(h, e, x, q, mask, y, w)
        gr = ot.flatten(g)
        g32 = ot.flatten(ot.loss_and_grads(h, e, x, q, mask, y, w, dtype=np.float32)[2]).astype(np.float64)
        band = np.zeros_like(gr)
        for where in ("gnn", "listed", "swapped"):
            lo = ot.flatten(ot.loss_and_grads(h, e, x, q, mask, y, w, kink_shift=+TAU, kink_where=where)[2])
            hi = ot.flatten(ot.loss_and_grads(h, e, x, q, mask, y, w, kink_shift=-TAU, kink_where=where)[2])
            band += np.abs(hi - lo)
        _ORACLE[key] = (loss, pred[:, :, 0], gr, g32, band)
    return _ORACLE[key]


def _tensor_slices(w):
    pos = 0
    for m in [w["upd"]] + list(w["msg"]) + list(w["pas"]):
        for W, b in m:
            for arr in (W, b):
                yield slice(pos, pos + arr.size)
                pos += arr.size


def _check_gradient(g, w, gr, g32=None, band=None, what=""):
    g = np.asarray(g, np.float64)
    assert g.shape == gr.shape
    worst, zeros = 0.0, 0
    for k, sl in enumerate(_tensor_slices(w)):
        scale = np.abs(gr[sl]).max()
        if scale == 0:
            zeros += 1
            assert np.all(g[sl] == 0), (what, k)
            continue
        noise = 0.0 if g32 is None else np.abs(g32[sl] - gr[sl]).max() / scale
        kink = 0.0 if band is None else band[sl].max() / scale
        err = np.abs(g[sl] - gr[sl]).max() / scale
        worst = max(worst, err)
        assert err <= max(2e-4, 4 * noise) + 2 * kink, (what, k, err, noise, kink)
    print(f"{what}: worst per-tensor relative gradient error {worst:.2e}; {zeros} tensors with zero gradient")


def _engine(factory, w, nx, path, fused=1, h_dim=48):
    eng = factory(nx=nx, T=len(w["msg"]), h_dim=h_dim, e_dim=h_dim)
    eng.set_weights(w)
    eng.set_option("train_path", path)
    eng.set_option("train_fused", fused)
    eng.train_init()
    return eng


def _step_against_oracle(factory, key, mols, cells, N, w, nx, path, fused=1, h_dim=48):
    offsets, xyz, x, Q, y, cell = _batch(mols, cells)
    loss_ref, pred_ref, gr, g32, band = _oracle(key, mols, cells, N, w, h_dim)
    eng = _engine(factory, w, nx, path, fused, h_dim)
    q, loss = eng.train_step_xyz(offsets, xyz, x, Q, y, N, apply=False, cell=cell)
    for b in range(len(mols)):
        a0, a1 = offsets[b], offsets[b + 1]
        assert np.abs(q[a0:a1] - pred_ref[b, :a1 - a0]).max() <= 2e-5, b
    assert abs(loss - loss_ref) <= 2e-5 * max(1.0, abs(loss_ref))
    _check_gradient(eng.get_gradients(), w, gr, g32, band, f"{key} train_path={path} train_fused={fused}")
    assert np.array_equal(ot.flatten(eng.get_weights()), ot.flatten(w).astype(np.float32))      # apply=False: weights untouched
    return eng


# ---------------------------------------------------------------------------------------------------- 1. periodic steps, both paths
PERIODIC = {
    # name: (nx, T, [(n, cell)], N)
    "cubic24": (9, 5, [(24, CUBIC)], 24),
    "cubic24_N29": (10, 1, [(24, CUBIC)], 29),
    "sheared20": (10, 5, [(20, cell_ref.SHEARED)], 20),
    "slab": (9, 1, [(22, SLAB)], 26),
    "batch": (9, 5, [(13, ZERO), (24, CUBIC), (18, cell_ref.SHEARED)], 24),
}


def _periodic_case(name):
    nx, T, systems, N = PERIODIC[name]
    w = random_weights(nx, T, seed=13, scale=0.4)
    mols = [_system(n, nx, c, seed=7 * n + T) for n, c in systems]
    return nx, w, mols, [c for _, c in systems], N


@pytest.mark.parametrize("path,fused", [(1, 1), (1, 0), (2, 1)])
@pytest.mark.parametrize("name", list(PERIODIC))
def test_periodic_step_matches_oracle(gpu_engine_factory, name, path, fused):
    nx, w, mols, cells, N = _periodic_case(name)
    gr = _oracle(name, mols, cells, N, w)[2]
    # the geometry matters: the same atoms as open molecules have another gradient, by far more than the tolerance
    g_open = _oracle(name + "/open", mols, [ZERO] * len(mols), N, w)[2]
    assert np.abs(gr - g_open).max() > 100 * 2e-4 * np.abs(gr).max()
    _step_against_oracle(gpu_engine_factory, name, mols, cells, N, w, nx, path, fused)


# ---------------------------------------------------------------------------------------------------- 2. pair-list path, open molecules
@pytest.mark.parametrize("pad", [0, 7])
@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 33, 41, 64])
def test_pair_list_open_molecules_at_tile_edges(gpu_engine_factory, n, pad):
    w = random_weights(9, 2, seed=14, scale=0.4)
    mols = [_system(n, 9, ZERO, seed=n)]
    _step_against_oracle(gpu_engine_factory, f"open{n}+{pad}", mols, [ZERO], n + pad, w, 9, 2)


def test_pair_list_batch_of_three_sizes(gpu_engine_factory):
    w = random_weights(10, 3, seed=15, scale=0.4)
    mols = [_system(n, 10, ZERO, seed=40 + n) for n in (33, 9, 50)]
    _step_against_oracle(gpu_engine_factory, "open-batch", mols, [ZERO] * 3, 52, w, 10, 2)


def test_pair_list_with_the_shipped_checkpoint(gpu_engine_factory, val_dir, val_names, golden_dir, weights_decay):
    """decay_model_weights on real molecules with their stored labels: the collapsed GNN gives exact-zero tensors on both sides."""
    import os
    names = [val_names[i] for i in (val_names.index("dsgdb9nsd_081300"), val_names.index("SSI-081ILE-085ARG-1-dimer"))]
    labs = np.load(os.path.join(golden_dir, "test_lab_charges.npy"))
    raw = load_molecules(val_dir, names, 9)[0]
    mols = [(m[0].astype(np.float32), m[1].astype(np.float32), np.float32(m[2]),
             labs[val_names.index(nm), :m[1].shape[0]].astype(np.float32)) for m, nm in zip(raw, names)]
    _step_against_oracle(gpu_engine_factory, "decay", mols, [ZERO] * 2, 41, weights_decay, 9, 2)
    assert sum(np.abs(_ORACLE["decay"][2][sl]).max() == 0 for sl in _tensor_slices(weights_decay)) > 1


# ---------------------------------------------------------------------------------------------------- 3. more than one piece per tile
@pytest.mark.parametrize("path", [2, 1])
@pytest.mark.parametrize("kind", ["cluster", "cell"])
def test_600_atoms_against_the_fixture(gpu_engine_factory, kind, path):
    """A 600-atom cluster and a 600-atom sheared cell (38 tiles of 16 atoms, several pieces of the partner range each) against
    tests/train_large_ref.py, whose output for exactly these inputs is cached under tests/golden (recomputed when they differ).  The
    dense path on the same input is held to the same numbers: that is how the two paths are shown to agree.  No float32 oracle at
    this size: the tolerance is 2e-4 + 2 kink."""
    from golden import make_train_large_fixtures as fx
    inputs = fx.case(kind)
    xyz, x, Q, cell, y, w = inputs
    z = fx.load(kind, inputs)
    loss_ref, q_ref, gr, band = z if z is not None else fx.compute(*inputs)
    eng = _engine(gpu_engine_factory, w, 9, path)
    off = np.int32([0, fx.N_ATOMS])
    q, loss = eng.train_step_xyz(off, xyz, x, np.float32([Q]), y, fx.N_ATOMS, apply=False, cell=ZERO if cell is None else cell)
    print(f"{kind} train_path={path}: q {np.abs(q - q_ref).max():.3e}, loss {loss:.6f} vs {loss_ref:.6f}")
    assert np.abs(q - q_ref).max() <= 2e-5
    assert abs(loss - loss_ref) <= 2e-5 * max(1.0, abs(loss_ref))
    _check_gradient(eng.get_gradients(), w, gr, None, band.astype(np.float64), f"{kind} train_path={path}")
    if path == 2:
        pairs, _, scratch, _ = eng.last_stats()
        assert pairs > 0 and scratch > 0


# ---------------------------------------------------------------------------------------------------- 4. Adam trajectory
def test_adam_trajectory_on_the_pair_list_path(gpu_engine_factory):
    """Ten optimizer steps over periodic cells on the pair-list path vs the oracle's Adam in float64 (the tolerances of
    test_gpu_train.test_adam_trajectory_matches_oracle); then inference and the gradient entry see the trained weights."""
    nx, T, N = 9, 2, 20
    w = random_weights(nx, T, seed=8, scale=0.5)
    cases = [(_system(n, nx, c, seed=s), c) for s, (n, c) in enumerate([(18, CUBIC), (20, cell_ref.SHEARED), (16, SLAB)])]
    eng = _engine(gpu_engine_factory, w, nx, 2)
    theta = ot.flatten(w)
    opt = ot.Adam(theta.size)
    losses, losses_ref = [], []
    for step in range(10):
        mol, cell = cases[step % 3]
        h, e, x, q, mask, y = _dense([mol], [cell], N)
        lr, _, g = ot.loss_and_grads(h, e, x, q, mask, y, ot.unflatten(theta, w))
        theta = opt.step(theta, ot.flatten(g))
        losses_ref.append(lr)
        n = mol[0].shape[0]
        losses.append(eng.train_step_xyz(np.int32([0, n]), mol[0], mol[1], np.float32([mol[2]]), mol[3], N, apply=True, cell=cell)[1])
    wt = eng.get_weights()
    got = ot.flatten(wt)
    print("loss curve", np.round(losses, 5), "ref", np.round(losses_ref, 5))
    assert np.abs(np.array(losses) - np.array(losses_ref)).max() < 1e-3 * max(losses_ref)
    assert np.abs(got - theta).max() < 2.5e-3
    assert np.mean(np.abs(got - theta) < 2e-4) > 0.97
    assert np.abs(got - ot.flatten(w)).max() > 5e-3                          # (ten steps of lr 1e-3 did move the weights)
    mol, cell = cases[1]
    n = mol[0].shape[0]
    off, Qa = np.int32([0, n]), np.float32([mol[2]])
    pred = eng.forward_xyz(off, mol[0], mol[1], Qa, N, cell=cell)
    ref = cell_ref.forward_cell(mol[0], mol[1], mol[2], cell, wt, N=N)
    assert np.abs(pred - ref[:n]).max() <= 2e-5
    for path in (2, 1):
        eng.set_option("grad_path", path)
        qv, gx = eng.charges_vjp_xyz(off, mol[0], mol[1], Qa, np.ones(n, np.float32), N, cell=cell)
        assert np.isfinite(gx).all() and np.abs(qv - ref[:n]).max() <= 2e-4


# ---------------------------------------------------------------------------------------------------- 5. bits
BITS_L = np.float32([7.0, 6.5, 0.0])


def _bits_batch(ns=(21, 12)):
    mols = [_system(n, 9, np.diag(BITS_L), seed=60 + n) for n in ns]
    return _batch(mols, [ZERO] * len(ns))[:5]


def _bits_case(factory, path, N=24, fused=1):
    """An engine on random weights and `step(**geo)`: one apply=False step of the two-molecule batch -> (q, loss, gradient)."""
    offsets, xyz, x, Q, y = _bits_batch()
    eng = _engine(factory, random_weights(9, 2, seed=19, scale=0.4), 9, path, fused)

    def step(**geo):
        q, loss = eng.train_step_xyz(offsets, xyz, x, Q, y, N, apply=False, **geo)
        return q, loss, eng.get_gradients()

    return eng, BITS_L, step


def _same(a, b):
    return np.array_equal(a[0], b[0]) and a[1] == b[1] and np.array_equal(a[2], b[2])


@pytest.mark.parametrize("path,fused", [(1, 1), (1, 0), (2, 1)])
def test_bit_identities(gpu_engine_factory, path, fused):
    eng, L, step = _bits_case(gpu_engine_factory, path, fused=fused)
    boxed = step(box=L)
    assert _same(boxed, step(box=L))                                         # the same step twice
    assert _same(boxed, step(cell=np.diag(L)))                               # box = its diagonal cell
    opened = step()                                                          # no cell: the unchanged epnn_train_step_xyz
    assert np.abs(opened[2] - boxed[2]).max() > 0
    zero = step(cell=ZERO)
    if path == 1:
        assert _same(zero, opened)                                           # dense path: an all-zero cell is no cell
        return
    # pair-list path: an all-zero cell gives the bits of cell = NULL through the new entry
    import ctypes as C
    from epnn_amd._lib import check, fptr, iptr
    offsets, xyz, x, Q, y = _bits_batch()
    q = np.empty_like(y)
    loss = C.c_float()
    check(eng.lib.epnn_train_step_xyz_cell(eng.h, 2, 24, iptr(offsets), fptr(xyz), fptr(x), fptr(Q), None, fptr(y), fptr(q),
                                           C.byref(loss), 0), eng.lib)
    assert _same(zero, (q, loss.value, eng.get_gradients()))
    # a call without a cell takes the dense path under every train_path value
    eng.set_option("train_path", 1)
    assert _same(opened, step())


def test_automatic_routing_below_the_threshold_is_the_dense_path(gpu_engine_factory):
    eng, L, step = _bits_case(gpu_engine_factory, 0)
    auto = step(cell=np.diag(L))
    auto_open = step()
    eng.set_option("train_path", 1)
    assert _same(auto, step(cell=np.diag(L))) and _same(auto_open, step())
    eng.set_option("train_path", 2)
    assert _same(auto_open, step())
    listed = step(cell=np.diag(L))
    assert not np.array_equal(listed[2], auto[2])                            # (another summation order: the pair-list path did run)
    assert np.abs(listed[2] - auto[2]).max() <= 1e-3 * np.abs(auto[2]).max()


# ---------------------------------------------------------------------------------------------------- 6. interface
def test_gradient_round_trip_after_a_pair_list_step(gpu_engine_factory):
    eng, L, step = _bits_case(gpu_engine_factory, 2)
    twin, _, _ = _bits_case(gpu_engine_factory, 2)
    g = step(box=L)[2]
    assert g.shape == (eng.param_count(),) and np.abs(g).max() > 0
    twin.set_gradients(g)
    assert np.array_equal(twin.get_gradients(), g)
    eng.train_apply()
    twin.train_apply()
    assert np.array_equal(ot.flatten(eng.get_weights()), ot.flatten(twin.get_weights()))
    # ... and equals one apply=True step
    third, _, _ = _bits_case(gpu_engine_factory, 2)
    offsets, xyz, x, Q, y = _bits_batch()
    third.train_step_xyz(offsets, xyz, x, Q, y, 24, apply=True, box=L)
    assert np.array_equal(ot.flatten(eng.get_weights()), ot.flatten(third.get_weights()))


@pytest.mark.parametrize("path", [2, 1])
def test_small_h_dim(gpu_engine_factory, path):
    w = random_weights(9, 2, seed=21, scale=0.4, h_dim=20)
    mols = [_system(n, 9, c, seed=80 + n) for n, c in ((19, CUBIC), (11, ZERO))]
    eng = _step_against_oracle(gpu_engine_factory, "h20", mols, [CUBIC, ZERO], 22, w, 9, path, h_dim=20)
    assert eng.get_gradients().shape == (ot.flatten(w).size,)


def test_refusals_leave_the_handle_usable(gpu_engine_factory):
    from epnn_amd._lib import EpnnError
    nx, N = 9, 24
    w = random_weights(nx, 2, seed=19, scale=0.4)
    mols = [_system(21, nx, CUBIC, seed=5)]
    offsets, xyz, x, Q, y, cell = _batch(mols, [CUBIC])
    eng = gpu_engine_factory(nx=nx, T=2)
    eng.set_weights(w)
    eng.set_option("train_path", 2)
    with pytest.raises(EpnnError, match="epnn_train_init"):                 # as the existing entry fails
        eng.train_step_xyz(offsets, xyz, x, Q, y, N, apply=False, cell=cell)
    with pytest.raises(EpnnError, match="epnn_train_init"):
        eng.train_step_xyz(offsets, xyz, x, Q, y, N, apply=False)
    eng.train_init()
    good = eng.train_step_xyz(offsets, xyz, x, Q, y, N, apply=False, cell=cell), eng.get_gradients()

    def still_good():
        q, loss = eng.train_step_xyz(offsets, xyz, x, Q, y, N, apply=False, cell=cell)
        assert np.array_equal(q, good[0][0]) and loss == good[0][1] and np.array_equal(eng.get_gradients(), good[1])

    with pytest.raises(EpnnError, match="width"):                           # narrower than 2 * cutoff
        eng.train_step_xyz(offsets, xyz, x, Q, y, N, apply=False, cell=cell_ref.THIN)
    still_good()
    with pytest.raises(EpnnError, match="width"):
        eng.train_step_xyz(offsets, xyz, x, Q, y, N, apply=False, box=np.float32([5.0, 7.0, 7.0]))
    with pytest.raises(ValueError):
        eng.train_step_xyz(offsets, xyz, x, Q, y, N, apply=False, box=np.float32([7, 7, 7]), cell=cell)
    with pytest.raises(EpnnError, match="train_path"):
        eng.set_option("train_path", 3)
    still_good()
    eng.set_partition(0, 2, exchange=lambda *a: None)
    with pytest.raises(EpnnError, match="partition"):
        eng.train_step_xyz(offsets, xyz, x, Q, y, N, apply=False, cell=cell)
    eng.set_partition(0, 1)
    still_good()
    loss_ref, pred_ref, gr, g32, band = _oracle("refusals", mols, [CUBIC], N, w)
    _check_gradient(good[1], w, gr, g32, band, "after the refusals")


def test_other_update_layers_are_refused_by_name(gpu_engine_factory):
    from epnn_amd._lib import EpnnError
    w = random_weights(9, 2, seed=9, scale=0.4)
    rng = np.random.default_rng(3)

    def dense(i, o):
        lim = 0.4 * np.sqrt(6.0 / (i + o))
        return rng.uniform(-lim, lim, (i, o)).astype(np.float32), rng.uniform(-0.1, 0.1, (o,)).astype(np.float32)

    w["upd"] = [dense(48 + 32, 64), dense(64, 32), dense(32, 48)]
    mols = [_system(14, 9, CUBIC, seed=3)]
    offsets, xyz, x, Q, y, cell = _batch(mols, [CUBIC])
    eng = gpu_engine_factory(nx=9, T=2)
    eng.set_weights(w)                                                      # (sets the update layers [64, 32] from the kernels' shapes)
    eng.train_init()
    eng.set_option("train_path", 2)
    with pytest.raises(EpnnError, match=r"\[32, 32\]"):
        eng.train_step_xyz(offsets, xyz, x, Q, y, 16, apply=False, cell=cell)
    eng.set_option("train_path", 0)                                         # stays on the dense path, which takes these layers
    q, loss = eng.train_step_xyz(offsets, xyz, x, Q, y, 16, apply=False, cell=cell)
    loss_ref, pred_ref, gr, g32, band = _oracle("upd64", mols, [CUBIC], 16, w)
    assert np.abs(q - pred_ref[0, :14]).max() <= 2e-5
    _check_gradient(eng.get_gradients(), w, gr, g32, band, "update layers [64, 32], dense path with a cell")


# ---------------------------------------------------------------------------------------------------- 7. size
def _weights_large(nx, seed, down):
    w = random_weights(nx, 2, seed=seed, scale=0.35)
    for t in range(2):                       # all-pairs sums over thousands of partners: |h| stays O(1), as in a trained model
        w["msg"][t][2] = (w["msg"][t][2][0] / down, w["msg"][t][2][1] / down)
    return w


def test_20000_atoms_with_automatic_routing(gpu_engine_factory):
    """A 20 000-atom sheared cell with train_path = 0 (400 M pair rows: nothing of that size may exist): routed to the pair list,
    consistent loss, finite gradient, and scratch that grows with the atoms: at most 2.1 times that of 10 000 atoms at the same
    density."""
    from epnn_amd import synth
    w = _weights_large(9, 25, 256.0)
    eng = _engine(gpu_engine_factory, w, 9, 0)
    scratch = {}
    for n in (10_000, 20_000):
        offsets, xyz, x, Q, N, cell = synth.triclinic_cell_system(n_atoms=n, seed=2)
        cell = np.asarray(cell, np.float32).reshape(3, 3)
        y = np.random.default_rng(n).normal(scale=0.3, size=n).astype(np.float32)
        q, loss = eng.train_step_xyz(offsets, xyz, x, Q, y, N, apply=False, cell=cell)
        pairs, fused_mols, scratch[n], _ = eng.last_stats()
        print(f"{n} atoms: {pairs} listed pairs, {scratch[n] / 2**20:.1f} MiB of scratch, loss {loss:.4f}")
        assert pairs > n and fused_mols == 0 and scratch[n] > 0            # the pair-list path's statistics
        g = eng.get_gradients()
        assert np.isfinite(g).all() and np.abs(g).max() > 0
        ref = ((y.astype(np.float64) - q.astype(np.float64)) ** 2).sum()
        assert abs(loss - ref) <= 1e-5 * ref
        assert np.abs(q - eng.forward_xyz(offsets, xyz, x, Q, N, cell=cell)).max() <= 2e-4
    assert scratch[20_000] <= 2.1 * scratch[10_000]
