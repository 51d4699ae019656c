"""The pair-list restatement of the training step (tests/train_large_ref.py) against the literal float64 oracle
(oracle.epnn_oracle_train.loss_and_grads on the dense inputs of cell_ref.get_init_edges_cell): every weight gradient of the factorised
form -- the all-pairs W2 sums, the near pairs' corrections, the padded partners' closed form, step 0 -- per parameter tensor. CPU only.

Bound: the first run gave at most 1.3e-14 of a tensor's largest entry (float64 sums of a few thousand terms in two orders: n = 20, N = 24, sheared); REL is
ten times that, far below the 1e-9 the GPU tests' reference has to be good for."""
import numpy as np
import pytest

import cell_ref
from conftest import random_weights
from oracle import epnn_oracle as orc
from oracle import epnn_oracle_train as ot
from train_large_ref import batch_loss_and_grads_large, loss_and_grads_large

REL = 1.3e-13
ZERO = np.zeros((3, 3), np.float32)
CUBIC = np.diag(np.float32([6.5, 6.5, 6.5]))
SLAB = np.float32([[7.0, 0, 0], [1.0, 6.8, 0], [0, 0, 0]])


def _features(rng, n, nx):
    x = np.zeros((n, nx), dtype=np.float32)
    el = rng.integers(0, nx - 1, n)
    x[np.arange(n), 1 + el] = 1.0
    x[:, 0] = np.array([1, 6, 7, 8, 9, 15, 16, 17, 35])[el % 9]
    return x, np.float32(rng.integers(-1, 2))


def _system(n, nx, cell, seed):
    rng = np.random.default_rng(seed)
    if np.any(cell):
        xyz = cell_ref.random_cell(rng, n, cell)
    else:                                                                   # an open cluster: a jittered lattice
        k = int(np.ceil(n ** (1 / 3)))
        grid = np.array([(a, b, c) for a in range(k) for b in range(k) for c in range(k)], dtype=np.float64)[:n] * 1.2
        xyz = (grid + rng.uniform(-0.15, 0.15, grid.shape)).astype(np.float32)
    x, Q = _features(rng, n, nx)
    return xyz, x, Q, rng.normal(scale=0.3, size=n)


def oracle_dense(xyz, x, Q, y, cell, w, N, h_dim=48, **kw):
    """loss_and_grads of one molecule padded to N with the cell's edges."""
    n = x.shape[0]
    h_p, e_p, x_p, q_p, mask = orc.dense_inputs(xyz, x, Q, N, h_dim=h_dim, e_dim=h_dim)
    e_p[:n, :n] = cell_ref.get_init_edges_cell(xyz, cell, num=h_dim)[0]
    yp = np.zeros((1, N, 1))
    yp[0, :n, 0] = y
    return ot.loss_and_grads(h_p[None], e_p[None], x_p[None], q_p[None], mask[None], yp, w, **kw)


def _compare(got, ref, what):
    worst = 0.0
    for k, (a, b) in enumerate(zip(_tensors(got), _tensors(ref))):
        scale = np.abs(b).max()
        err = np.abs(a - b).max()
        if scale == 0:
            assert err == 0, (what, k)
            continue
        worst = max(worst, err / scale)
        assert err <= REL * scale, (what, k, err, scale)
    return worst


def _tensors(g):
    out = []
    for m in [g["upd"]] + list(g["msg"]) + list(g["pas"]):
        for W, b in m:
            out += [np.asarray(W), np.asarray(b)]
    return out


@pytest.mark.parametrize("name,cell", [("cubic", CUBIC), ("sheared", cell_ref.SHEARED), ("slab", SLAB), ("open", ZERO)])
@pytest.mark.parametrize("n,N,nx,T,h_dim", [(6, 6, 9, 2, 48), (13, 17, 10, 3, 48), (20, 20, 9, 2, 20), (20, 24, 9, 1, 48)])
def test_weight_gradients_match_the_dense_oracle(name, cell, n, N, nx, T, h_dim):
    w = random_weights(nx, T, seed=7 + n, scale=0.5, h_dim=h_dim)
    xyz, x, Q, y = _system(n, nx, cell, seed=n + T)
    loss_ref, pred_ref, g_ref = oracle_dense(xyz, x, Q, y, cell, w, N, h_dim=h_dim)
    loss, q, g = loss_and_grads_large(xyz, x, Q, y, w, N=N, cell=cell if np.any(cell) else None, h_dim=h_dim, block=7)
    assert abs(loss - loss_ref) <= 1e-12 * max(loss_ref, 1.0)
    assert np.abs(q - pred_ref[0, :n, 0]).max() <= 1e-12
    assert np.abs(pred_ref[0, n:, 0]).max(initial=0.0) == 0
    worst = _compare(g, g_ref, name)
    print(f"{name} n={n} N={N}: worst tensor error {worst:.2e} of its largest entry")


def test_kink_shift_moves_both_alike():
    """The bracket of the GPU tests: kink_shift means the same in both."""
    w = random_weights(9, 2, seed=3, scale=0.5)
    xyz, x, Q, y = _system(16, 9, cell_ref.SHEARED, seed=1)
    for shift in (2e-6, -2e-6, 1e-2):
        ref = oracle_dense(xyz, x, Q, y, cell_ref.SHEARED, w, 18, kink_shift=shift)[2]
        got = loss_and_grads_large(xyz, x, Q, y, w, N=18, cell=cell_ref.SHEARED, kink_shift=shift)[2]
        _compare(got, ref, shift)
    a = ot.flatten(oracle_dense(xyz, x, Q, y, cell_ref.SHEARED, w, 18, kink_shift=1e-2)[2])
    assert np.abs(a - ot.flatten(oracle_dense(xyz, x, Q, y, cell_ref.SHEARED, w, 18)[2])).max() > 0


def test_the_cell_changes_the_gradient_and_a_batch_adds_up():
    w = random_weights(9, 2, seed=5, scale=0.5)
    xyz, x, Q, y = _system(12, 9, CUBIC, seed=9)
    g_cell = ot.flatten(loss_and_grads_large(xyz, x, Q, y, w, cell=CUBIC)[2])
    g_open = ot.flatten(loss_and_grads_large(xyz, x, Q, y, w)[2])
    assert np.abs(g_cell - g_open).max() > 1e-3 * np.abs(g_cell).max()
    xyz2, x2, Q2, y2 = _system(7, 9, ZERO, seed=2)
    off = np.int32([0, 12, 19])
    loss, q, flat = batch_loss_and_grads_large(off, np.concatenate([xyz, xyz2]), np.concatenate([x, x2]), np.float32([Q, Q2]),
                                               np.concatenate([y, y2]), w, 14, cells=[CUBIC, None])
    one = loss_and_grads_large(xyz, x, Q, y, w, N=14, cell=CUBIC)
    two = loss_and_grads_large(xyz2, x2, Q2, y2, w, N=14)
    assert loss == one[0] + two[0] and np.array_equal(q, np.concatenate([one[1], two[1]]))
    assert np.array_equal(flat, ot.flatten(one[2]) + ot.flatten(two[2]))


@pytest.mark.parametrize("kind", ["cluster", "cell"])
def test_cached_600_atom_fixtures_were_made_from_the_current_inputs(kind):
    """tests/golden/train_large_{cluster,cell}600.npz (the cached output of loss_and_grads_large for the GPU test's 600-atom systems)
    carry the hash of today's inputs, and their arrays are consistent: the charges sum to Q, the loss is sum (y - q)^2."""
    from golden import make_train_large_fixtures as fx
    inputs = fx.case(kind)
    z = fx.load(kind, inputs)
    assert z is not None, "run tests/golden/make_train_large_fixtures.py"
    loss, q, grad, band = z
    xyz, x, Q, cell, y, w = inputs
    assert q.shape == (fx.N_ATOMS,) and grad.shape == band.shape == ot.flatten(w).shape
    assert abs(q.sum() - float(Q)) <= 1e-9 * fx.N_ATOMS
    assert abs(loss - ((y.astype(np.float64) - q) ** 2).sum()) <= 1e-12 * loss
    assert np.isfinite(grad).all() and np.abs(grad).max() > 0 and (band >= 0).all()
