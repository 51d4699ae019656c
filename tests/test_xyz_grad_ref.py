"""The float64 reference of the charge gradients with respect to the coordinates (tests/xyz_grad_ref.py) against the oracle's
forward and against central finite differences of itself. CPU only."""
import numpy as np
import pytest

from conftest import random_weights
from xyz_grad_ref import forward64, vjp64


def _molecule(n, nx, seed):
    """n atoms at least 0.9 apart inside a 2.4 Å box (most pairs within the 3 Å cutoff), one-hot x like parse_xyz."""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < n:
        p = rng.uniform(0.0, 2.4, 3)
        if all(np.linalg.norm(p - q) > 0.9 for q in pts) or len(pts) == 0:
            pts.append(p)
    xyz = np.array(pts, dtype=np.float32)
    x = np.zeros((n, nx), dtype=np.float32)
    el = rng.integers(0, nx - 1, n)
    x[np.arange(n), 1 + el] = 1.0
    x[:, 0] = np.array([1, 6, 7, 8, 9, 15, 16, 17, 35])[el % 9]
    return xyz, x, np.float32(rng.integers(-1, 2))


@pytest.mark.parametrize("nx,h_dim,n,N", [(9, 48, 6, 6), (10, 48, 5, 8), (10, 20, 6, 9)])
def test_forward_equals_the_oracle(nx, h_dim, n, N):
    from oracle import epnn_oracle as orc
    w = random_weights(nx, 2, seed=4, scale=0.7, h_dim=h_dim)
    xyz, x, Q = _molecule(n, nx, seed=n)
    ref = orc.forward_xyz(xyz, x, Q, w, N=N, dtype=np.float64, h_dim=h_dim)
    got = forward64(xyz, x, Q, w, N=N, h_dim=h_dim)
    assert np.abs(got - ref).max() <= 2e-6


@pytest.mark.parametrize("nx,h_dim,n,N", [(9, 48, 5, 7), (10, 48, 6, 6), (10, 20, 5, 8)])
def test_vjp_equals_central_differences(nx, h_dim, n, N):
    """g^T dq/dxyz against central differences of the float64 forward (step 1e-4 Å on float64 coordinates).  Random
    non-degenerate weights, padding N > n where given, both atom-feature widths, h_dim 48 and 20."""
    import xyz_grad_ref as xr
    w = random_weights(nx, 2, seed=7, scale=0.7, h_dim=h_dim)
    xyz, x, Q = _molecule(n, nx, seed=10 + n)
    g = np.random.default_rng(1).normal(size=n)
    q, gxyz = vjp64(xyz, x, Q, g, w, N=N, h_dim=h_dim)
    assert np.isfinite(gxyz).all() and np.abs(gxyz).max() > 1e-6

    # finite differences on float64 coordinates (the helper's forward casts to float32 first: patch it for the check)
    base = xyz.astype(np.float64)
    orig = xr.edges64

    def f(r):
        xr.edges64 = lambda _xyz, num, cutoff=3.0, eta=2.0: _edges_at(r, num, cutoff, eta)
        try:
            return forward64(xyz, x, Q, w, N=N, h_dim=h_dim)[:n] @ g
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
    assert np.abs(gxyz - fd).max() <= 1e-6 + 1e-5 * np.abs(fd).max(), (np.abs(gxyz - fd).max(), np.abs(fd).max())


def _edges_at(r, num, cutoff, eta):
    """edges64 on float64 coordinates as given."""
    mu = np.linspace(0.1, cutoff, num=num)
    d = r[:, None, :] - r[None, :, :]
    D = np.sqrt((d * d).sum(-1))
    C = (np.cos(np.pi * D / cutoff) + 1.0) / 2.0
    C[D >= cutoff] = 0.0
    np.fill_diagonal(C, 0.0)
    u = D[:, :, None] - mu[None, None, :]
    e = C[:, :, None] * np.exp(-eta * u * u)
    return e, np.zeros_like(e), d, D
