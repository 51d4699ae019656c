"""The references at edge constants other than the reference's own (the near_tol keyword of oracle/ and tests/*_ref.py, the sets and
the flips of tests/edge_constants.py): the flips against the oracle's own flag, the keyword against central differences of the
float64 forward with the flags held fixed, the factorised references against the literal ones.  CPU only."""
import numpy as np
import pytest

import cell_ref as cr
import edge_constants as ec
import jvp_ref as jr
import xyz_grad_ref as xr
from conftest import random_weights
from grad_large_ref import pair_list, vjp64_large
from oracle import epnn_oracle as orc
from oracle import epnn_oracle_train as ot
from test_train_large_ref import _compare, _system
from test_xyz_grad_ref import _edges_at
from train_large_ref import loss_and_grads_large

ZERO = np.zeros((3, 3), np.float32)
CELL = np.float32([[8, 0, 0], [2.5, 7.8, 0], [-2, 1.5, 7.6]])             # widths 7.27, 7.65, 7.60: twice the cutoff of every set
NON_DEFAULT = ["B", "C"]


def _mol(n, seed, cell=None):
    """n atoms on a jittered 1.15 A lattice (in a cell: its second layer one lattice vector away, so that pairs cross a face)."""
    rng = np.random.default_rng(seed)
    k = int(np.ceil(n ** (1 / 3)))
    grid = np.array([(a, b, c) for a in range(k) for b in range(k) for c in range(k)], dtype=np.float64)[:n] * 1.15
    xyz = grid + rng.uniform(-0.1, 0.1, grid.shape) + 0.4
    if cell is not None:
        xyz[grid[:, 2] > 0] -= np.asarray(cell, dtype=np.float64)[0]
    x = np.zeros((n, 9), np.float32)
    el = rng.integers(0, 4, n)
    x[:, 0] = np.array([1, 6, 7, 8])[el]
    x[np.arange(n), 1 + el] = 1
    return xyz.astype(np.float32), x, np.float32(rng.integers(-1, 2))


def _oracle_flag(D, s):
    """The flag of a pair at distance D as the oracle's EPN layer decides it: from get_init_edges' float32 rows of a two-atom molecule."""
    return bool(jr.near_flags(np.float32([[0, 0, 0], [D, 0, 0]]), ZERO, s.h_dim, s.cutoff, s.eta, s.near_tol)[0, 1])


def test_flips_of_the_named_sets():
    assert np.allclose(ec.near_flips(*ec.SET_C), [2.1037, 2.2983, 2.5347], atol=1e-4)
    assert len(ec.near_flips(*ec.SET_A)) == len(ec.near_flips(*ec.SET_B)) == 1
    assert np.allclose(ec.near_flips(*ec.DEFAULT), [2.99396], atol=1e-5)          # (test_cutoff_and_is_near_edges_on_every_path)
    for s in list(ec.SETS.values()) + [ec.DEFAULT]:
        flips = ec.near_flips(*s)
        want = True                                                              # near from 0 up to the first flip, alternating after it
        for lo, hi in zip(np.concatenate([[0.5], flips]), np.concatenate([flips, [s.cutoff]])):
            for D in (lo + 2e-5, 0.5 * (lo + hi), hi - 2e-5):
                assert _oracle_flag(D, s) == want == bool(ec.flag(np.float64(np.float32(D)), *s)), (s, D)
            want = not want
        assert not _oracle_flag(s.cutoff + 2e-5, s)


def test_the_default_keyword_changes_no_bit():
    w = random_weights(9, 2, seed=4, scale=0.7)
    xyz, x, Q = _mol(9, 1)
    for dtype in (np.float32, np.float64):
        a = orc.forward_xyz(xyz, x, Q, w, N=11, dtype=dtype)
        assert np.array_equal(a, orc.forward_xyz(xyz, x, Q, w, N=11, dtype=dtype, near_tol=1e-5))
    g = np.random.default_rng(2).normal(size=9)
    assert np.array_equal(xr.vjp64(xyz, x, Q, g, w, N=11)[1], xr.vjp64(xyz, x, Q, g, w, N=11, near_tol=1e-5)[1])
    assert np.array_equal(vjp64_large(xyz, x, Q, g, w, N=11)[1], vjp64_large(xyz, x, Q, g, w, N=11, near_tol=1e-5)[1])
    assert np.array_equal(pair_list(xyz, 48)["near"], pair_list(xyz, 48, near_tol=1e-5)["near"])


@pytest.mark.parametrize("name", NON_DEFAULT)
def test_every_reference_has_the_oracles_forward_and_the_tolerance_matters(name):
    s = ec.SETS[name]
    kw = ec.ref_kwargs(s)
    w = random_weights(9, 2, seed=4, scale=0.7, h_dim=s.h_dim)
    n, N = 17, 20
    xyz, x, Q = _mol(n, 17)
    ec.assert_admissible([(xyz,)], s, least=3 if name == "C" else 1, what=f"set {name}")
    ref = orc.forward_xyz(xyz, x, Q, w, N=N, dtype=np.float64, **kw)
    g = np.zeros(n)
    got = {"forward64": xr.forward64(xyz, x, Q, w, N=N, **kw), "vjp64_large": vjp64_large(xyz, x, Q, g, w, N=N, **kw)[0],
           "jvp64": jr.jvp64(xyz, x, Q, w, N=N, **kw)[0], "jvp64_factorised": jr.jvp64_factorised(xyz, x, Q, w, N=N, **kw)[0],
           "forward_cell": cr.forward_cell(xyz, x, Q, ZERO, w, N, **kw)}
    for what, q in got.items():
        assert np.abs(q[:n] - ref[:n]).max() <= 2e-6, what               # (float64 edges against the oracle's float32 ones)
    other = orc.forward_xyz(xyz, x, Q, w, N=N, dtype=np.float64, h_dim=s.h_dim, cutoff=s.cutoff, eta=s.eta)
    assert np.abs(other - ref).max() > 1e-3                              # near_tol alone


def test_the_block_wise_and_periodic_forwards_pass_the_tolerance_down():
    """forward_xyz_large, forward_large_pbc / _cell, forward_batch_pbc and forward64_pbc / _cell (48 channels: set B) against the dense
    forwards at the same constants, and away from them at the default tolerance."""
    import periodic_ref as pr
    s = ec.SET_B
    kw = dict(cutoff=s.cutoff, eta=s.eta, near_tol=s.near_tol)
    w = random_weights(9, 2, seed=4, scale=0.7)
    n = 17
    box = np.float32([7.5, 7.0, 7.2])
    xyz, x, Q = _mol(n, 17)
    xyc, xc, Qc = _mol(n, 18, CELL)
    xyb, xb, Qb = _mol(n, 19, np.diag(box))
    ec.assert_admissible([(xyz,), (xyc,), (xyb,)], s, [None, CELL, np.diag(box)], least=3, what="set B")
    pairs = {
        "forward_xyz_large": (orc.forward_xyz_large, (xyz, x, Q, w), orc.forward_xyz(xyz, x, Q, w, dtype=np.float64, **kw)),
        "forward_large_cell": (cr.forward_large_cell, (xyc, xc, Qc, CELL, w), cr.forward_cell(xyc, xc, Qc, CELL, w, **kw)),
        "forward_large_pbc": (pr.forward_large_pbc, (xyb, xb, Qb, box, w), pr.forward_pbc(xyb, xb, Qb, box, w, **kw)),
        "forward64_cell": (cr.forward64_cell, (xyc, xc, Qc, CELL, w), cr.forward_cell(xyc, xc, Qc, CELL, w, **kw)),
        "forward64_pbc": (pr.forward64_pbc, (xyb, xb, Qb, box, w), pr.forward_pbc(xyb, xb, Qb, box, w, **kw)),
        "forward_batch_pbc": (lambda *a, **k: pr.forward_batch_pbc(np.int32([0, n]), *a, n, **k), (xyb, xb, np.float32([Qb]), box, w),
                              pr.forward_pbc(xyb, xb, Qb, box, w, **kw)),
    }
    for what, (fn, args, ref) in pairs.items():
        assert np.abs(fn(*args, **kw) - ref).max() <= 2e-6, what                                  # (float64 edges against float32 ones)
        assert np.abs(fn(*args, cutoff=s.cutoff, eta=s.eta) - ref).max() > 1e-3, what             # near_tol alone
    assert np.abs(cr.forward_cell(xyb, xb, Qb, np.diag(box), w, **kw) - pairs["forward_large_pbc"][2]).max() <= 1e-12


@pytest.mark.parametrize("name", NON_DEFAULT)
def test_vjp_equals_central_differences(name):
    """test_xyz_grad_ref's check at another set: the flags are those of the undisplaced molecule at the set's near_tol."""
    s = ec.SETS[name]
    kw = ec.ref_kwargs(s)
    w = random_weights(9, 2, seed=7, scale=0.7, h_dim=s.h_dim)
    n, N = 10, 12
    xyz, x, Q = _mol(n, 10 + n)
    ec.assert_admissible([(xyz,)], s, least=1, what=f"set {name}")
    g = np.random.default_rng(1).normal(size=n)
    q, gxyz = xr.vjp64(xyz, x, Q, g, w, N=N, **kw)
    base = xyz.astype(np.float64)
    orig = xr.edges64

    def f(r):
        xr.edges64 = lambda _xyz, num, cutoff=3.0, eta=2.0: _edges_at(r, num, cutoff, eta)
        try:
            return xr.forward64(xyz, x, Q, w, N=N, **kw)[:n] @ g
        finally:
            xr.edges64 = orig

    step = 1e-4
    fd = np.zeros_like(base)
    for i in range(n):
        for c in range(3):
            rp, rm = base.copy(), base.copy()
            rp[i, c] += step
            rm[i, c] -= step
            fd[i, c] = (f(rp) - f(rm)) / (2 * step)
    assert np.abs(fd).max() > 1e-3
    assert np.abs(gxyz - fd).max() <= 1e-6 + 1e-5 * np.abs(fd).max(), (np.abs(gxyz - fd).max(), np.abs(fd).max())
    # with the default tolerance the gradient is another one
    assert np.abs(xr.vjp64(xyz, x, Q, g, w, N=N, h_dim=s.h_dim, cutoff=s.cutoff, eta=s.eta)[1] - gxyz).max() > 1e-3 * np.abs(gxyz).max()


@pytest.mark.parametrize("name", list(ec.SETS))
def test_the_coulomb_cases_are_usable(name):
    """The Coulomb call's case of tests/test_gpu_edge_constants.py at sets A, B and C: admissible, fq a usable derivative case that the
    constants move; the reference's keywords reach both of its halves (q by forward64, fq by vjp64 at the same constants)."""
    from coulomb_ref import coulomb64
    from test_gpu_coulomb import KE
    from test_gpu_edge_constants import COULOMB_ALPHA, _coulomb_case
    s, w, mol, N, q, phi, fq, kink = _coulomb_case(name)
    kw = ec.ref_kwargs(s)
    n = len(q)
    assert np.array_equal(q, xr.forward64(*mol, w, N=N, **kw)[:n])
    assert np.array_equal(phi, coulomb64(mol[0], q, KE, COULOMB_ALPHA)[0])
    assert np.array_equal(fq, -xr.vjp64(*mol, phi, w, N=N, **kw)[1]) and np.abs(fq).max() > 0


@pytest.mark.parametrize("geo", ["open", "cell"])
@pytest.mark.parametrize("name", NON_DEFAULT)
def test_the_factorised_gradient_is_the_literal_one(name, geo):
    s = ec.SETS[name]
    kw = ec.ref_kwargs(s)
    w = random_weights(9, 2, seed=7, scale=0.7, h_dim=s.h_dim)
    n, N = 17, 19
    g = np.random.default_rng(3).normal(size=n)
    if geo == "open":
        xyz, x, Q = _mol(n, 30)
        q, gx = xr.vjp64(xyz, x, Q, g, w, N=N, **kw)
        qf, gf = vjp64_large(xyz, x, Q, g, w, N=N, **kw)
    else:
        xyz, x, Q = _mol(n, 31, CELL)
        q, gx, gs = cr.strain64(xyz, x, Q, g, CELL, w, N=N, **kw)
        qf, gf, gsf = vjp64_large(xyz, x, Q, g, w, N=N, cell=CELL, strain=True, **kw)
        assert np.abs(gs - gsf).max() <= 1e-10 * np.abs(gs).max()
        assert np.abs(cr.vjp64_cell(xyz, x, Q, g, CELL, w, N=N, **kw)[1] - gx).max() == 0
    assert np.abs(q[:n] - qf).max() <= 1e-12 and np.abs(gx).max() > 1e-3
    assert np.abs(gx - gf).max() <= 1e-10 * np.abs(gx).max(), np.abs(gx - gf).max()


@pytest.mark.parametrize("geo", ["open", "cell"])
@pytest.mark.parametrize("name", NON_DEFAULT)
def test_jvp_equals_central_differences_and_its_factorised_form(name, geo):
    """test_jvp_ref's checks at another set: v, strain and dQ at once, the flags of the undeformed system at the set's near_tol."""
    s = ec.SETS[name]
    kw = ec.ref_kwargs(s)
    geo_kw = {} if geo == "open" else {"cell": CELL}
    cell = jr.cell_of(**geo_kw)
    w = random_weights(9, 2, seed=7, scale=0.7, h_dim=s.h_dim)
    n, N = 9, 11
    xyz, x, Q = _mol(n, 11, None if geo == "open" else CELL)
    rng = np.random.default_rng(20 + n)
    v, E, dQ = rng.normal(size=(n, 3)), 0.3 * rng.normal(size=(3, 3)), float(rng.normal())
    q, tq = jr.jvp64(xyz, x, Q, w, N=N, v=v, strain=E, dQ=dQ, **geo_kw, **kw)
    qf, tf = jr.jvp64_factorised(xyz, x, Q, w, N=N, v=v, strain=E, dQ=dQ, **geo_kw, **kw)
    assert np.abs(q - qf).max() <= 1e-12 and np.abs(tq - tf).max() <= 1e-11 * max(1.0, np.abs(tq).max())
    r0, a0 = xyz.astype(np.float64), cr.duals(cell)[0]
    near = jr.near_flags(xyz, cell, **kw)
    assert near.any() and (near != jr.near_flags(xyz, cell, s.h_dim, s.cutoff, s.eta)).any()          # (the tolerance decides some pairs)
    Q0 = float(Q)

    def f(t):
        F = np.eye(3) + t * E
        return jr.forward64_at((r0 + t * v) @ F.T, a0 @ F.T, x, Q0 + t * dQ, near, w, N, **{k: kw[k] for k in ("h_dim", "cutoff", "eta")})

    h = 1e-5
    fd = (f(h) - f(-h)) / (2 * h)
    assert np.abs(fd).max() > 1e-3
    assert np.abs(tq - fd).max() <= 1e-6 + 1e-5 * np.abs(fd).max(), (np.abs(tq - fd).max(), np.abs(fd).max())


@pytest.mark.parametrize("cell", [ZERO, CELL], ids=["open", "cell"])
@pytest.mark.parametrize("name", NON_DEFAULT)
def test_training_gradients_literal_factorised_and_central_differences(name, cell):
    s = ec.SETS[name]
    kw = ec.ref_kwargs(s)
    w = random_weights(9, 2, seed=9, scale=0.5, h_dim=s.h_dim)
    n, N = 14, 16
    xyz, x, Q, y = _system(n, 9, cell, seed=n + 2)
    ec.assert_admissible([(xyz,)], s, [cell], least=1, what=f"set {name}")
    geo = {"cell": cell} if np.any(cell) else {}
    h_p, e_p, x_p, q_p, mask = orc.dense_inputs(xyz, x, Q, N, h_dim=s.h_dim, e_dim=s.h_dim, cutoff=s.cutoff, eta=s.eta)
    e_p[:n, :n] = cr.get_init_edges_cell(xyz, cell, num=s.h_dim, cutoff=s.cutoff, eta=s.eta)[0]
    yp = np.zeros((1, N, 1))
    yp[0, :n, 0] = y
    loss_ref, pred_ref, g_ref = ot.loss_and_grads(h_p[None], e_p[None], x_p[None], q_p[None], mask[None], yp, w, near_tol=s.near_tol)
    loss, q, g = loss_and_grads_large(xyz, x, Q, y, w, N=N, **geo, **kw)
    assert abs(loss - loss_ref) <= 1e-12 * max(loss_ref, 1.0) and np.abs(q - pred_ref[0, :n, 0]).max() <= 1e-12
    _compare(g, g_ref, name)
    at_default = ot.flatten(ot.loss_and_grads(h_p[None], e_p[None], x_p[None], q_p[None], mask[None], yp, w)[2])
    flat = ot.flatten(g)
    assert np.abs(at_default - flat).max() > 1e-3 * np.abs(flat).max()                              # near_tol alone
    # central differences of the loss along random directions of the whole parameter vector (the flags do not depend on the weights)
    theta = ot.flatten(w)
    rng = np.random.default_rng(4)
    for _ in range(3):
        d = rng.normal(size=theta.size)
        d /= np.linalg.norm(d)
        h = 1e-5
        lp = loss_and_grads_large(xyz, x, Q, y, ot.unflatten(theta + h * d, w), N=N, **geo, **kw)[0]
        lm = loss_and_grads_large(xyz, x, Q, y, ot.unflatten(theta - h * d, w), N=N, **geo, **kw)[0]
        fd = (lp - lm) / (2 * h)
        assert abs(fd) > 1e-4 and abs(fd - flat @ d) <= 1e-6 + 1e-5 * abs(fd), (fd, flat @ d)
