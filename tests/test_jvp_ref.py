"""The float64 forward-mode reference (tests/jvp_ref.py) checked against things that do not share its code: the reverse-mode
references (adjoint identity g . tq = gxyz . v + gstrain : E), central differences of the float64 forward along (v, E, dQ), and
charge conservation sum tq = dQ.  CPU only."""
import numpy as np
import pytest

from conftest import random_weights
import cell_ref as cr
import jvp_ref as jr
import periodic_ref as pr
import xyz_grad_ref as xgr

BOX = np.float32([7.0, 6.5, 0.0])
GEOS = {"open": {}, "box": {"box": BOX}, "cell": {"cell": cr.SHEARED}}


def _mol(seed, n, cell):
    """n atoms, most pairs within the cutoff: a jittered 1.15 A lattice (it fits every cell used here), x as in test_cell_ref."""
    rng = np.random.default_rng(seed)
    k = int(np.ceil(n ** (1 / 3)))
    grid = np.array([(a, b, c) for a in range(k) for b in range(k) for c in range(k)], dtype=np.float64)[:n] * 1.15
    xyz = grid + rng.uniform(-0.1, 0.1, grid.shape) + 0.4
    xyz[grid[:, 2] > 0] -= np.asarray(cell, dtype=np.float64)[0]                    # (the second layer one lattice vector away: pairs cross a face)
    xyz = xyz.astype(np.float32)
    x = np.zeros((n, 9), np.float32)
    el = rng.integers(0, 4, n)
    x[:, 0] = np.array([1, 6, 7, 8])[el]
    x[np.arange(n), 1 + el] = 1
    return xyz, x


def _direction(seed, n):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 3)), 0.3 * rng.normal(size=(3, 3)), float(rng.normal())


@pytest.mark.parametrize("geo", ["open", "box", "cell"])
@pytest.mark.parametrize("n", [2, 5, 17])
def test_adjoint_identity_against_the_reverse_mode_references(geo, n):
    kw = GEOS[geo]
    cell = jr.cell_of(**kw)
    w = random_weights(9, 2, seed=7, scale=0.7)
    xyz, x = _mol(3 + n, n, cell)
    Q, N = np.float32(1.0), n + 3
    v, E, _ = _direction(n, n)
    g = np.random.default_rng(50 + n).normal(size=n)
    q, tq = jr.jvp64(xyz, x, Q, w, N=N, v=v, strain=E, **kw)
    if geo == "open":
        q_r, gx = xgr.vjp64(xyz, x, Q, g, w, N=N)
    elif geo == "box":
        q_r, gx = pr.vjp64_pbc(xyz, x, Q, g, BOX, w, N=N)
    else:
        q_r, gx = cr.vjp64_cell(xyz, x, Q, g, cell, w, N=N)
    q_s, gx_s, W = cr.strain64(xyz, x, Q, g, cell, w, N=N)
    assert np.abs(q - q_r[:n]).max() <= 1e-12 and np.abs(gx - gx_s).max() <= 1e-12 * max(1.0, np.abs(gx).max())
    lhs, rhs = g @ tq, (gx * v).sum() + (W * E).sum()
    scale = np.abs(g) @ np.abs(tq) + np.abs(gx * v).sum() + np.abs(W * E).sum()
    assert scale > 1e-6
    assert abs(lhs - rhs) <= 1e-9 * scale, (lhs, rhs, scale)
    # each kind alone, and linearity
    tv = jr.jvp64(xyz, x, Q, w, N=N, v=v, **kw)[1]
    ts = jr.jvp64(xyz, x, Q, w, N=N, strain=E, **kw)[1]
    assert abs(g @ tv - (gx * v).sum()) <= 1e-9 * scale and abs(g @ ts - (W * E).sum()) <= 1e-9 * scale
    assert np.abs(tv + ts - tq).max() <= 1e-12 * max(1.0, np.abs(tq).max())


@pytest.mark.parametrize("geo,n", [("open", 7), ("box", 8), ("cell", 9)])
def test_central_differences_of_the_forward(geo, n):
    """Atoms displaced along v, atoms and cell deformed together by E, Q moved by dQ, all at once: float64 coordinates and cells
    as they are (edges64_at), the near flags of the undeformed system (constants, as in tests/test_cell_ref.py)."""
    kw = GEOS[geo]
    cell = jr.cell_of(**kw)
    w = random_weights(9, 2, seed=7, scale=0.7)
    xyz, x = _mol(11, n, cell)
    Q, N = 1.0, n + 2
    v, E, dQ = _direction(20 + n, n)
    q, tq = jr.jvp64(xyz, x, Q, w, N=N, v=v, strain=E, dQ=dQ, **kw)
    r0, a0 = xyz.astype(np.float64), cr.duals(cell)[0]
    near = jr.near_flags(xyz, cell)
    if geo != "open":
        Dm, Do = cr._dist(cr.mic(r0[None] - r0[:, None], cell)), np.sqrt(((r0[None] - r0[:, None]) ** 2).sum(-1))
        assert ((Dm < 3.0) & (Do >= 3.0)).any()                   # pairs across the faces take part
    assert np.abs(jr.forward64_at(r0, a0, x, Q, near, w, N) - q).max() <= 1e-7   # (jvp64 rounds Q / n to float32, as the library does)

    def f(t):
        F = np.eye(3) + t * E                                     # r_a -> r_a + t E_ac r_c
        return jr.forward64_at((r0 + t * v) @ F.T, a0 @ F.T, x, Q + t * dQ, near, w, N)

    h = 1e-5
    fd = (f(h) - f(-h)) / (2 * h)
    assert np.abs(fd).max() > 1e-3
    assert np.abs(tq - fd).max() <= 1e-6 + 1e-5 * np.abs(fd).max(), (np.abs(tq - fd).max(), np.abs(fd).max())
    # the same for each kind alone
    for one in ({"v": v}, {"strain": E}, {"dQ": dQ}):
        t1 = jr.jvp64(xyz, x, Q, w, N=N, **one, **kw)[1]
        vv, EE, dd = one.get("v", 0 * v), one.get("strain", 0 * E), one.get("dQ", 0.0)

        def f1(t):
            F = np.eye(3) + t * EE
            return jr.forward64_at((r0 + t * vv) @ F.T, a0 @ F.T, x, Q + t * dd, near, w, N)

        fd1 = (f1(h) - f1(-h)) / (2 * h)
        assert np.abs(t1 - fd1).max() <= 1e-6 + 1e-5 * np.abs(fd1).max(), (list(one), np.abs(t1 - fd1).max())


@pytest.mark.parametrize("geo", ["open", "box", "cell"])
def test_the_tangent_conserves_the_charge(geo):
    kw = GEOS[geo]
    w = random_weights(9, 2, seed=7, scale=0.7)
    n = 12
    xyz, x = _mol(5, n, jr.cell_of(**kw))
    v, E, dQ = _direction(9, n)
    q, tq = jr.jvp64(xyz, x, np.float32(-1.0), w, N=n + 1, v=v, strain=E, dQ=dQ, **kw)
    assert abs(q.sum() + 1.0) <= 1e-6 and abs(tq.sum() - dQ) <= 1e-12 * max(1.0, np.abs(tq).sum())
    assert np.abs(tq - dQ / n).max() > 1e-3                       # (not just the uniform share)
    q0, t0 = jr.jvp64(xyz, x, np.float32(-1.0), w, N=n + 1, **kw)
    assert np.array_equal(q0, q) and not t0.any()
    # a lone atom: no pairs, tq = dQ and q = Q
    q1, t1 = jr.jvp64(xyz[:1], x[:1], np.float32(1.0), w, N=4, v=v[:1], strain=E, dQ=dQ, **kw)
    assert q1[0] == 1.0 and t1[0] == dQ


@pytest.mark.parametrize("geo", ["open", "box", "cell"])
@pytest.mark.parametrize("n,N", [(1, 4), (2, 8), (17, 24), (33, 33)])
def test_the_factorised_form_of_the_kernels(geo, n, N):
    """The form epnn_jvp.hip.h runs (per-atom rows, max(P, -R) sweep, correction rows, closed-form padded partners, listed pairs in the
    EPN steps) is the literal model: same q and tq in float64."""
    kw = GEOS[geo]
    w = random_weights(9, 2, seed=7, scale=0.7)
    xyz, x = _mol(40 + n, n, jr.cell_of(**kw))
    v, E, dQ = _direction(60 + n, n)
    q, tq = jr.jvp64(xyz, x, np.float32(1.0), w, N=N, v=v, strain=E, dQ=dQ, **kw)
    qf, tf = jr.jvp64_factorised(xyz, x, np.float32(1.0), w, N=N, v=v, strain=E, dQ=dQ, **kw)
    assert np.abs(q - qf).max() <= 1e-12 * max(1.0, np.abs(q).max())
    assert np.abs(tq - tf).max() <= 1e-11 * max(1.0, np.abs(tq).max()), np.abs(tq - tf).max()
