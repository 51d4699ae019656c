"""The pair-list restatement of the charge gradients (tests/grad_large_ref.py) against the literal float64 references
(xyz_grad_ref.vjp64, periodic_ref.vjp64_pbc, cell_ref.vjp64_cell / strain64): the step-0 shortcut, the padded partners' closed
form, the row and column passes and the fold of W3, to 1e-9 relative. CPU only."""
import numpy as np
import pytest

import cell_ref
import periodic_ref
from conftest import random_weights
from grad_large_ref import pair_list, vjp64_large
from xyz_grad_ref import vjp64

REL = 1e-9


def _lattice_molecule(n, nx, seed):
    """n atoms on a jittered 1.15 A lattice, one-hot x like parse_xyz, Q in {-1, 0, 1}."""
    rng = np.random.default_rng(seed)
    k = int(np.ceil(n ** (1 / 3)))
    grid = np.array([(a, b, c) for a in range(k) for b in range(k) for c in range(k)], dtype=np.float64)[:n] * 1.15
    xyz = (grid + rng.uniform(-0.1, 0.1, grid.shape)).astype(np.float32)
    return (xyz,) + _features(rng, n, nx)


def _features(rng, n, nx):
    x = np.zeros((n, nx), dtype=np.float32)
    el = rng.integers(0, nx - 1, n)
    x[np.arange(n), 1 + el] = 1.0
    x[:, 0] = np.array([1, 6, 7, 8, 9, 15, 16, 17, 35])[el % 9]
    return x, np.float32(rng.integers(-1, 2))


def _close(got, ref, what):
    scale = np.abs(ref).max()
    assert scale > 0, what
    err = np.abs(got - ref).max()
    assert err <= REL * scale, (what, err, scale)


@pytest.mark.parametrize("nx,h_dim,T,n,N", [(9, 48, 2, 20, 20), (10, 48, 3, 60, 64), (9, 20, 2, 45, 50), (10, 48, 2, 150, 150),
                                            (9, 48, 3, 97, 101)])
def test_open_molecules(nx, h_dim, T, n, N):
    w = random_weights(nx, T, seed=3 + T, scale=0.6, h_dim=h_dim)
    xyz, x, Q = _lattice_molecule(n, nx, seed=n)
    g = np.random.default_rng(n).normal(size=n)
    q_ref, ref = vjp64(xyz, x, Q, g, w, N=N, h_dim=h_dim)
    q, gxyz = vjp64_large(xyz, x, Q, g, w, N=N, h_dim=h_dim, block=32)
    _close(q, q_ref[:n], "q")
    _close(gxyz, ref, "gxyz")
    assert np.abs(q_ref[n:]).max(initial=0.0) == 0


def test_kink_shift_moves_both_alike():
    """The bracket of the GPU tests: kink_shift means the same in both references."""
    w = random_weights(9, 2, seed=5, scale=0.6)
    xyz, x, Q = _lattice_molecule(40, 9, seed=2)
    g = np.random.default_rng(0).normal(size=40)
    for shift in (2e-5, -2e-5, 1e-2):
        ref = vjp64(xyz, x, Q, g, w, N=44, kink_shift=shift)[1]
        got = vjp64_large(xyz, x, Q, g, w, N=44, kink_shift=shift)[1]
        _close(got, ref, shift)
    assert np.abs(vjp64(xyz, x, Q, g, w, N=44, kink_shift=1e-2)[1] - vjp64(xyz, x, Q, g, w, N=44)[1]).max() > 0


@pytest.mark.parametrize("T,n,N,L", [(2, 80, 80, [9.0, 9.5, 10.0]), (3, 50, 56, [8.0, 0.0, 8.5]), (2, 120, 128, [11.0, 11.0, 11.0])])
def test_periodic_boxes(T, n, N, L):
    w = random_weights(9, T, seed=11, scale=0.6)
    rng = np.random.default_rng(n)
    L = np.float32(L)
    xyz = periodic_ref.random_cell(rng, n, L)
    x, Q = _features(rng, n, 9)
    g = rng.normal(size=n)
    q_ref, ref = periodic_ref.vjp64_pbc(xyz, x, Q, g, L, w, N=N)
    q, gxyz = vjp64_large(xyz, x, Q, g, w, N=N, box=L)
    _close(q, q_ref[:n], "q")
    _close(gxyz, ref, "gxyz")
    # the list is the one the forward's front-end reports
    pl = pair_list(xyz, 48, box=L)
    I, J, W = periodic_ref.pairs_pbc(xyz, L)
    up = pl["i"] < pl["j"]
    assert np.array_equal(pl["i"][up], I) and np.array_equal(pl["j"][up], J) and np.array_equal(pl["near"][up], W)


@pytest.mark.parametrize("T,n,N,name", [(2, 60, 60, "SHEARED"), (3, 40, 48, "HEX_SLAB"), (2, 20, 24, "WIRE"), (2, 150, 150, "BASIS_A")])
def test_cells_and_strain(T, n, N, name):
    w = random_weights(10, T, seed=13, scale=0.6)
    cell = getattr(cell_ref, name)
    rng = np.random.default_rng(n)
    xyz = cell_ref.random_cell(rng, n, cell)
    x, Q = _features(rng, n, 10)
    g = rng.normal(size=n)
    q_ref, ref, gs_ref = cell_ref.strain64(xyz, x, Q, g, cell, w, N=N)
    q, gxyz, gs = vjp64_large(xyz, x, Q, g, w, N=N, cell=cell, strain=True)
    _close(q, q_ref[:n], "q")
    _close(gxyz, ref, "gxyz")
    _close(gs, gs_ref, "gstrain")
    assert np.abs(gs - gs.T).max() <= 1e-12 * np.abs(gs).max()
    q2, gxyz2 = vjp64_large(xyz, x, Q, g, w, N=N, cell=cell)
    assert np.array_equal(q2, q) and np.array_equal(gxyz2, gxyz)
    _close(gxyz, cell_ref.vjp64_cell(xyz, x, Q, g, cell, w, N=N)[1], "gxyz (vjp64_cell)")


def test_diagonal_cell_is_the_box_and_zero_cell_is_open():
    w = random_weights(9, 2, seed=17, scale=0.6)
    rng = np.random.default_rng(4)
    L = np.float32([8.0, 9.0, 0.0])
    xyz = periodic_ref.random_cell(rng, 40, L)
    x, Q = _features(rng, 40, 9)
    g = rng.normal(size=40)
    box = vjp64_large(xyz, x, Q, g, w, box=L)[1]
    _close(vjp64_large(xyz, x, Q, g, w, cell=np.diag(L))[1], box, "diagonal cell")
    _close(vjp64_large(xyz, x, Q, g, w, cell=np.zeros((3, 3), np.float32))[1], vjp64_large(xyz, x, Q, g, w)[1], "zero cell")


def test_cached_box4096_fixture_was_made_from_the_current_inputs():
    """tests/golden/grad_large_box4096.npz (the cached output of vjp64_large for the GPU test's 4096-atom box) carries the hash of
    today's inputs, and its arrays are consistent: the charges sum to Q and the gradient sums to zero over the atoms."""
    from golden import make_grad_large_fixtures as fx
    case = fx.box4096_case()
    z = fx.load(*case)
    assert z is not None, "run tests/golden/make_grad_large_fixtures.py"
    q, ref, lo, hi = z
    assert q.shape == (4096,) and ref.shape == lo.shape == hi.shape == (4096, 3)
    assert abs(q.sum() - float(case[2][0])) <= 1e-9 * 4096
    assert np.abs(ref.sum(0)).max() <= 1e-9 * 4096 * np.abs(ref).max()
