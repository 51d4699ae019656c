"""The dipole and the atomic polar tensor (APT) of dipole_xyz, pinned independently of the device: with tests/grad_large_ref.py in
float64 the APT assembled as apt[i][a][b] = q_i delta_ab + gxyz_a[i][b], gxyz_a the reference's VJP for the seed g_a[k] = r_ka - o_a,
against central differences of the reference's own mu(r) = sum_k q_k(r) (r_k - o) with the origin o held fixed; the sum rule
sum_i apt[i] = Q I; and the entry epnn_charges_vjp_multi_xyz_cell exported by the built library and bound in epnn_amd/_lib.py.
CPU only.

Step and bound are those of the other references' checks against central differences (test_xyz_grad_ref.py, test_coulomb_ref.py):
step 1e-4 A on float64 coordinates, |apt - fd| <= 1e-6 + 1e-5 max |fd| on every component; a component whose central difference
changes by more than that when the step is halved (a ReLU changes sign inside the step) is held to the same bound at the first
halved step whose own half agrees with it, none below 1e-6 (test_coulomb_ref.py's rule)."""
import ctypes as C
import inspect

import numpy as np
import pytest

import grad_large_ref as glr
from conftest import random_weights
from test_grad_large_ref import _lattice_molecule

NAME = "epnn_charges_vjp_multi_xyz_cell"
CASES = [(9, 12, None), (17, 24, 2.0)]            # (n, N, Q or the molecule's own); the second one is charged: Q = +2


def _pair_list_at(r):
    """grad_large_ref.pair_list with the listed pairs of the float32 coordinates and the geometry of the float64 coordinates r as
    given (the reference casts its coordinates to float32 first: a step of 1e-4 would be rounded)."""
    orig = glr.pair_list

    def pair_list(xyz, num, cutoff=3.0, eta=2.0, box=None, cell=None, block=256, near_tol=1e-5):
        pl = dict(orig(xyz, num, cutoff, eta, box, cell, block, near_tol))
        d = r[pl["i"]] - r[pl["j"]]
        D = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        mu = np.linspace(0.1, cutoff, num=num)
        Cc = (np.cos(np.pi * D / cutoff) + 1.0) / 2.0
        dC = -0.5 * (np.pi / cutoff) * np.sin(np.pi * D / cutoff)
        u = D[:, None] - mu[None, :]
        ex = np.exp(-eta * u * u)
        pl.update(d=d, D=D, e=Cc[:, None] * ex, de=(dC[:, None] - 2.0 * eta * u * Cc[:, None]) * ex)
        return pl
    return orig, pair_list


def _vjp_at(r, xyz, x, Q, g, w, N):
    orig, patched = _pair_list_at(r)
    glr.pair_list = patched
    try:
        return glr.vjp64_large(xyz, x, Q, g, w, N=N)
    finally:
        glr.pair_list = orig


def _mu_at(r, o, xyz, x, Q, w, N):
    q = _vjp_at(r, xyz, x, Q, np.zeros(r.shape[0]), w, N)[0]
    return (q[:, None] * (r - o)).sum(0)


def _central(i, b, step, base, o, *args):
    rp, rm = base.copy(), base.copy()
    rp[i, b] += step
    rm[i, b] -= step
    return (_mu_at(rp, o, *args) - _mu_at(rm, o, *args)) / (2 * step)


@pytest.mark.parametrize("n,N,Q", CASES)
def test_apt_equals_central_differences_of_the_dipole_and_sums_to_the_charge(n, N, Q):
    w = random_weights(9, 2, seed=5, scale=0.6)
    xyz, x, Q0 = _lattice_molecule(n, 9, seed=n)
    Q = float(Q0) if Q is None else Q
    base = xyz.astype(np.float64)
    o = base.mean(0)                                                # the fixed origin: the unweighted centroid
    rel = base - o
    q = None
    apt = np.zeros((n, 3, 3))
    for a in range(3):
        q, gx = _vjp_at(base, xyz, x, Q, rel[:, a], w, N)
        apt[:, a, :] = gx
    apt[:, [0, 1, 2], [0, 1, 2]] += q[:, None]
    assert abs(q.sum() - Q) <= 1e-9 * n
    args = (xyz, x, Q, w, N)
    step = 1e-4
    fd = np.zeros((n, 3, 3))
    half = np.zeros((n, 3, 3))
    for i in range(n):
        for b in range(3):
            fd[i, :, b] = _central(i, b, step, base, o, *args)
            half[i, :, b] = _central(i, b, step / 2, base, o, *args)
    tol = 1e-6 + 1e-5 * np.abs(fd).max()
    halved = 0
    for i, b in sorted(set(zip(*np.nonzero(np.abs(fd - half).max(1) > tol)))):
        h, coarse, fine = step / 2, fd[i, :, b], half[i, :, b]
        while np.abs(coarse - fine).max() > tol:
            h, coarse = h / 2, fine
            assert h >= 1e-6, (i, b, "no step down to 1e-6 at which the central difference settles")
            fine = _central(i, b, h, base, o, *args)
        fd[i, :, b] = coarse
        halved += 1
    err = np.abs(apt - fd).max()
    total = apt.sum(0)
    print(f"n = {n}, Q = {Q}: |apt - fd| {err:.3e} of {np.abs(fd).max():.3e}, {halved} of {3 * n} columns at a halved step; "
          f"|sum_i apt - Q I| {np.abs(total - Q * np.eye(3)).max():.3e}")
    assert halved <= 0.1 * 3 * n + 1
    assert np.abs(apt).max() > 1e-3 and err <= tol, (err, np.abs(fd).max())
    assert np.abs(total - Q * np.eye(3)).max() <= tol


def test_apt_does_not_depend_on_the_origin():
    """sum_k dq_k/dr_ib = 0 (charge conservation): another origin changes the seeds by a constant per molecule and the APT by nothing."""
    w = random_weights(9, 2, seed=5, scale=0.6)
    xyz, x, Q = _lattice_molecule(9, 9, seed=9)
    base = xyz.astype(np.float64)
    got = []
    for o in (base.mean(0), np.array([3.0, -2.0, 1.0])):
        got.append(np.stack([glr.vjp64_large(xyz, x, Q, (base - o)[:, a], w, N=12)[1] for a in range(3)], 1))
    assert np.abs(got[0] - got[1]).max() <= 1e-9 * np.abs(got[0]).max()


def test_the_entry_is_exported_bound_and_wrapped():
    from epnn_amd import _lib, charge_gn, engine
    lib = _lib.load()
    assert hasattr(lib, NAME), f"{NAME} is not exported by the built library"
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
    res, args = _lib.SIGNATURES[NAME]
    # (h, B, N, offsets, xyz, x, Q, cell, K, g, q_out, gxyz_out, gstrain_out)
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_int, ip, fp, fp, fp, fp, C.c_int, fp, fp, fp, fp]
    assert getattr(lib, NAME).argtypes == args
    for cls, n_default in ((engine.Engine, inspect.Parameter.empty), (charge_gn.EPNNModel, None)):
        p = inspect.signature(cls.charges_vjp_xyz_multi).parameters
        assert list(p)[1:] == ["offsets", "xyz", "x", "Q", "g", "N", "box", "cell", "strain"] and p["N"].default is n_default
        p = inspect.signature(cls.dipole_xyz).parameters
        assert list(p)[1:] == ["offsets", "xyz", "x", "Q", "N", "origin"] and p["N"].default is n_default
