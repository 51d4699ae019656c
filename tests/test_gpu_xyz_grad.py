"""Charge gradients with respect to the coordinates on the GPU (epnn_charges_vjp_xyz) against the float64 reference of
tests/xyz_grad_ref.py, their invariants, determinism, the Jacobian, the untouched training state and the error paths. GPU only."""
import os

import numpy as np
import pytest

from conftest import ROOT, load_molecules, random_weights
from xyz_grad_ref import vjp64

pytestmark = pytest.mark.gpu

TAU = 2e-5           # ReLU-kink bracket of the reference (loss_and_grads(kink_shift=...))


def _lattice_molecule(n, nx, seed):
    """n atoms on a jittered 1.15 Å lattice (no two closer than ~0.9 Å), one-hot x like parse_xyz, Q in {-1, 0, 1}."""
    rng = np.random.default_rng(seed)
    k = int(np.ceil(n ** (1 / 3)))
    grid = np.array([(a, b, c) for a in range(k) for b in range(k) for c in range(k)], dtype=np.float64)[:n] * 1.15
    xyz = (grid + rng.uniform(-0.1, 0.1, grid.shape)).astype(np.float32)
    x = np.zeros((n, nx), dtype=np.float32)
    el = rng.integers(0, nx - 1, n)
    x[np.arange(n), 1 + el] = 1.0
    x[:, 0] = np.array([1, 6, 7, 8, 9, 15, 16, 17, 35])[el % 9]
    return xyz, x, np.float32(rng.integers(-1, 2))


def _batch(mols):
    offsets = np.zeros(len(mols) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([m[0].shape[0] for m in mols])
    return (offsets, np.concatenate([m[0] for m in mols]), np.concatenate([m[1] for m in mols]),
            np.array([m[2] for m in mols], dtype=np.float32))


def _check_against_reference(eng, mols, w, N, h_dim=48, seed=0):
    """Per molecule: max |gxyz - ref| <= 2e-4 max |ref| (+ the spread of the kink bracket).  q against epnn_forward_xyz and the
    float64 reference <= 2e-4: the inference forward runs its Dense layers on the bf16 pipe in split form, the train path's in f32."""
    offsets, xyz, x, Q = _batch(mols)
    g = np.random.default_rng(seed).normal(size=int(offsets[-1])).astype(np.float32)
    q, gxyz = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, N)
    q_fwd = eng.forward_xyz(offsets, xyz, x, Q, N)
    assert np.abs(q - q_fwd).max() <= 2e-4
    worst = 0.0
    for b, (mx, mxx, mQ) in enumerate(mols):
        a0, a1 = offsets[b], offsets[b + 1]
        q_ref, ref = vjp64(mx, mxx, mQ, g[a0:a1].astype(np.float64), w, N=N, h_dim=h_dim)
        assert np.abs(q[a0:a1] - q_ref[:a1 - a0]).max() <= 2e-4
        lo = vjp64(mx, mxx, mQ, g[a0:a1].astype(np.float64), w, N=N, h_dim=h_dim, kink_shift=+TAU)[1]
        hi = vjp64(mx, mxx, mQ, g[a0:a1].astype(np.float64), w, N=N, h_dim=h_dim, kink_shift=-TAU)[1]
        scale = np.abs(ref).max()
        kink = np.abs(lo - hi).max()
        err = np.abs(gxyz[a0:a1] - ref).max()
        assert scale > 0
        assert err <= 2e-4 * scale + kink, (b, err, scale, kink)
        worst = max(worst, err / scale)
    return worst


@pytest.mark.parametrize("fused", [1, 0])
def test_model_weights_on_the_validation_split(gpu_engine_factory, val_dir, val_names, weights_full, fused):
    """models/model_weights (nx = 10, a live GNN) on real molecules of the recorded validation split, padded to 41."""
    names = val_names[:6]
    mols = load_molecules(val_dir, names, nx=10)[0]
    eng = gpu_engine_factory(nx=10, T=len(weights_full["msg"]))
    eng.set_option("train_fused", fused)
    eng.set_weights(weights_full)
    _check_against_reference(eng, mols, weights_full, 41)


@pytest.mark.parametrize("N,ns", [(8, [6, 8]), (12, [10, 4, 12]), (41, [30, 17])])
def test_random_weights_with_padding(gpu_engine_factory, N, ns):
    w = random_weights(9, 2, seed=5, scale=0.6)
    mols = [_lattice_molecule(n, 9, seed=n) for n in ns]
    eng = gpu_engine_factory(nx=9, T=2)
    eng.set_weights(w)
    _check_against_reference(eng, mols, w, N)


@pytest.mark.parametrize("N,ns", [(96, [90]), (97, [93])])
def test_both_implementations_at_their_border(gpu_engine_factory, N, ns):
    """N = 96 is the last size of the row-fused kernels, N = 97 the first of the layer-by-layer ones."""
    w = random_weights(10, 2, seed=6, scale=0.6)
    mols = [_lattice_molecule(n, 10, seed=n) for n in ns]
    eng = gpu_engine_factory(nx=10, T=2)
    eng.set_weights(w)
    _check_against_reference(eng, mols, w, N)


def test_small_h_dim(gpu_engine_factory):
    w = random_weights(9, 2, seed=8, scale=0.6, h_dim=20)
    mols = [_lattice_molecule(n, 9, seed=20 + n) for n in (9, 12)]
    eng = gpu_engine_factory(nx=9, T=2, h_dim=20, e_dim=20)
    eng.set_weights(w)
    _check_against_reference(eng, mols, w, 14, h_dim=20)


def test_other_update_layers(gpu_engine_factory):
    """make_model(layers=[64]): the update MLP is not [32, 32], every size takes the layer-by-layer kernels."""
    w = random_weights(9, 2, seed=9, scale=0.6)
    rng = np.random.default_rng(3)

    def dense(i, o):
        lim = 0.6 * np.sqrt(6.0 / (i + o))
        return rng.uniform(-lim, lim, (i, o)).astype(np.float32), rng.uniform(-0.1, 0.1, (o,)).astype(np.float32)

    w["upd"] = [dense(48 + 32, 64), dense(64, 48)]
    mols = [_lattice_molecule(n, 9, seed=30 + n) for n in (7, 10)]
    eng = gpu_engine_factory(nx=9, T=2)
    eng.set_weights(w)
    _check_against_reference(eng, mols, w, 12)


def _random_case(gpu_engine_factory, nx=9, N=16, ns=(12, 9, 16), seed=11):
    w = random_weights(nx, 2, seed=seed, scale=0.6)
    mols = [_lattice_molecule(n, nx, seed=seed + n) for n in ns]
    eng = gpu_engine_factory(nx=nx, T=2)
    eng.set_weights(w)
    return eng, w, mols, _batch(mols)


def test_invariants(gpu_engine_factory):
    """Total charge is conserved: the all-ones cotangent gives max |gxyz| <= 1e-4 max |gxyz of a random g|.  q depends on
    distances only: |sum_k gxyz_k| and |sum_k r_k x gxyz_k| <= 1e-4 n max |gxyz| (max |r| for the torque) per molecule."""
    eng, w, mols, (offsets, xyz, x, Q) = _random_case(gpu_engine_factory)
    A = int(offsets[-1])
    g = np.random.default_rng(2).normal(size=A).astype(np.float32)
    _, gr = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 16)
    _, g1 = eng.charges_vjp_xyz(offsets, xyz, x, Q, np.ones(A, np.float32), 16)
    for b in range(len(mols)):
        a0, a1 = offsets[b], offsets[b + 1]
        n = a1 - a0
        scale = np.abs(gr[a0:a1]).max()
        assert scale > 0
        assert np.abs(g1[a0:a1]).max() <= 1e-4 * scale
        r = xyz[a0:a1].astype(np.float64)
        gg = gr[a0:a1].astype(np.float64)
        assert np.abs(gg.sum(0)).max() <= 1e-4 * n * scale
        assert np.abs(np.cross(r, gg).sum(0)).max() <= 1e-4 * n * scale * np.abs(r).max()


def test_deterministic_and_batch_independent(gpu_engine_factory):
    eng, w, mols, (offsets, xyz, x, Q) = _random_case(gpu_engine_factory)
    A = int(offsets[-1])
    g = np.random.default_rng(4).normal(size=A).astype(np.float32)
    q1, g1 = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 16)
    q2, g2 = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 16)
    assert np.array_equal(g1, g2) and np.array_equal(q1, q2)
    for b in range(len(mols)):
        a0, a1 = offsets[b], offsets[b + 1]
        off1 = np.array([0, a1 - a0], dtype=np.int32)
        qa, ga = eng.charges_vjp_xyz(off1, xyz[a0:a1], x[a0:a1], Q[b:b + 1], g[a0:a1], 16)
        assert np.array_equal(ga, g1[a0:a1]), b
    eng.set_option("train_fused", 0)
    q0, g0 = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 16)
    assert np.abs(g0 - g1).max() <= 1e-4 * np.abs(g1).max()
    assert np.abs(q0 - q1).max() <= 1e-5


def test_jacobian(gpu_engine_factory, val_dir, val_names, weights_full):
    """J from one call on n copies: J contracted with g equals the VJP of g to rounding.  A central difference of the shipped
    inference forward (epnn_forward_xyz, step 1e-2 Å) is within 2 % of max |J| of J, beyond what the same difference of the
    float64 reference forward is from J (kinks and is_near switches inside the step), and its median error is within 2 %."""
    from epnn_amd import charge_gn
    mols = load_molecules(val_dir, [nm for nm in val_names if nm.startswith("dsgdb9nsd")][:1], nx=10)[0]
    mxyz, mx, mQ = mols[0]
    n = mxyz.shape[0]
    model = charge_gn.make_model([32, 32], 48, len(weights_full["msg"]), 10, 29)
    model.set_weights_dict(weights_full)
    q, J = model.charge_jacobian_xyz(mxyz, mx, mQ)
    assert J.shape == (n, n, 3)
    g = np.random.default_rng(5).normal(size=n).astype(np.float32)
    off = np.array([0, n], dtype=np.int32)
    qv, gv = model.charges_vjp_xyz(off, mxyz, mx, np.array([mQ], np.float32), g)
    assert np.abs(q - qv).max() == 0
    assert np.abs(np.einsum("i,ikc->kc", g, J) - gv).max() <= 1e-4 * np.abs(gv).max()
    # A step of 1e-2 Å crosses ReLU kinks and is_near switches of a live GNN (the derivative jumps there; the forward itself jumps
    # at an is_near switch): the same central difference of the float64 reference forward measures how far that takes a
    # difference quotient from the derivative at the point, and the inference forward's may differ from J by that much more.
    from xyz_grad_ref import forward64
    h = 1e-2
    fd = np.zeros_like(J)
    fd_ref = np.zeros_like(J)
    for k in range(n):
        for c in range(3):
            xp, xm = mxyz.copy(), mxyz.copy()
            xp[k, c] += h
            xm[k, c] -= h
            qp = model.predict_xyz(off, xp, mx, np.array([mQ], np.float32))
            qm = model.predict_xyz(off, xm, mx, np.array([mQ], np.float32))
            fd[:, k, c] = (qp - qm) / (2 * h)
            fd_ref[:, k, c] = (forward64(xp, mx, mQ, weights_full, N=29)[:n] - forward64(xm, mx, mQ, weights_full, N=29)[:n]) / (2 * h)
    excess = np.abs(fd - J) - np.abs(fd_ref - J)
    assert excess.max() <= 2e-2 * np.abs(J).max(), (excess.max(), np.abs(J).max())
    assert np.median(np.abs(fd - J)) <= 2e-2 * np.abs(J).max()


def test_training_state_untouched(gpu_engine_factory):
    from oracle import epnn_oracle_train as otr
    eng, w, mols, (offsets, xyz, x, Q) = _random_case(gpu_engine_factory)
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
    # after the update the call uses the new weights, like the forward
    q2, _ = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 16)
    assert np.abs(q2 - eng.forward_xyz(offsets, xyz, x, Q, 16)).max() <= 2e-4
    assert np.abs(q2 - q).max() > 0


def test_errors_leave_the_handle_usable(gpu_engine_factory):
    from epnn_amd._lib import EpnnError
    eng, w, mols, (offsets, xyz, x, Q) = _random_case(gpu_engine_factory)
    A = int(offsets[-1])
    g = np.ones(A, np.float32)
    with pytest.raises(EpnnError):
        eng.charges_vjp_xyz(offsets, xyz, x, Q, g[:-1], 16)
    with pytest.raises(EpnnError, match="does not fit"):
        eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 12)
    bad = offsets.copy()
    bad[0] = 1
    with pytest.raises(EpnnError, match="offsets"):
        eng.charges_vjp_xyz(bad, xyz, x, Q, g, 16)
    q, gx = eng.charges_vjp_xyz(offsets, xyz, x, Q, g, 16)
    assert np.isfinite(gx).all()
    assert np.abs(q - eng.forward_xyz(offsets, xyz, x, Q, 16)).max() <= 2e-4
