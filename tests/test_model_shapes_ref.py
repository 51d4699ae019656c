"""Every (nx, T) of tests/model_shapes.py on the float64 references alone: the chosen cases meet the conditions that make them usable
(so that an edit of a reference or of a seed cannot quietly empty tests/test_gpu_model_shapes.py), and the independent references
agree with each other at every shape: the pair-list gradient with the literal one, the forward-mode reference with its factorised form
and (adjoint identity) with the reverse-mode one, the pair-list training reference with the dense training oracle.  CPU only.

The bounds are those of test_grad_large_ref.py (1e-9 of the gradient's scale), test_jvp_ref.py (1e-12 on q, 1e-11 on tq, 1e-9 of the
adjoint identity's terms) and test_train_large_ref.py (1.3e-13 per tensor).  The 150-atom forward is asserted in the GPU file only,
before the device is consulted: its references cost seconds per shape."""
import numpy as np
import pytest

import jvp_ref
import model_shapes as ms
from grad_large_ref import vjp64_large
from oracle import epnn_oracle_train as ot
from test_gpu_train_cell import _batch as _train_batch, _dense
from test_train_large_ref import _compare
from train_large_ref import batch_loss_and_grads_large
from xyz_grad_ref import vjp64

REL = 1e-9           # tests/test_grad_large_ref.py
shapes = pytest.mark.parametrize("shape", ms.SHAPES, ids=ms.IDS)
SIZED = [(s, "small") for s in ms.SHAPES] + [(s, "large") for s in ms.OPEN_LARGE]           # 17 atoms at N = 24; 33 atoms at N = 40
sized = pytest.mark.parametrize("shape,size", SIZED, ids=[f"nx{s[0]}-T{s[1]}-{size}" for s, size in SIZED])


def test_the_shapes_cover_the_limits():
    assert sorted(nx for nx, T in ms.SHAPES) == list(range(1, 11))
    assert {T for nx, T in ms.SHAPES} == {1, 4, 6, 7, 8}
    assert {-(-(nx + 49) // 4) for nx, T in ms.SHAPES} == {13, 14, 15}                  # K-steps of the fused training kernel
    assert {(nx % 2, T % 2) for nx, T in ms.SHAPES} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for table in (ms.OPEN_LARGE, ms.JVP_LARGE):
        nxs = [nx for nx, T in table]
        assert len(nxs) >= 3 and 1 in nxs and any(nx % 2 and nx > 1 for nx in nxs) and any(nx % 2 == 0 for nx in nxs)
    assert {ms.PERIODIC[s][0] for s in ms.SHAPES} == {"box", "cell"}


@pytest.mark.parametrize("nx", range(1, 14))
def test_features_fill_the_columns(nx):
    for n in (1, 2, 5, 17, 33):
        x, Q = ms.features(np.random.default_rng(n), n, nx)
        ms.assert_columns(x)
        assert x.shape == (n, nx) and x.dtype == np.float32 and (x[:, 0] >= 1).all() and Q in (-1.0, 0.0, 1.0)
        if nx >= 2:
            assert ((x[:, 1:] != 0).sum(1) == 1).all() and set(np.unique(x[:, 1:])) <= {0.0, 1.0}


@shapes
@pytest.mark.parametrize("group", ["N32", "N64"])
def test_forward_cases_are_usable(shape, group):
    ms.forward_case(shape, group)


@sized
def test_open_gradient_cases_are_usable_and_the_references_agree(shape, size):
    """The open case against vjp64 meets the conditions; vjp64_large gives the same q and gxyz."""
    w, mol, N, g, q, gxyz, kink, _, fig = ms.open_case(shape, size)
    g64 = g.astype(np.float64)
    n = len(g)
    qf, gf = vjp64_large(mol[0], mol[1], mol[2], g64, w, N=N)
    assert np.abs(q[:n] - qf).max() <= REL * np.abs(q).max() and np.abs(gxyz - gf).max() <= REL * np.abs(gxyz).max()


@shapes
def test_coulomb_cases_are_usable(shape):
    """The Coulomb call's case meets the derivative conditions for fq = -vjp64(g = phi); its parts add up and fq is that gradient."""
    from coulomb_ref import coulomb_forces64
    w, mol, N, q, phi, fq, kink, _, fig = ms.coulomb_case(shape)
    n = len(q)
    assert np.abs(q).max() > 0.01 and np.abs(phi).max() > 0
    assert np.array_equal(fq, -vjp64(mol[0], mol[1], mol[2], phi, w, N=N)[1])
    full = coulomb_forces64(mol[0], mol[1], mol[2], w, N, ms.KE, ms.COULOMB_ALPHA)
    assert np.array_equal(full[3], full[4] + full[5]) and np.array_equal(full[5], fq) and full[0].shape == (n,)


@shapes
def test_cell_gradient_cases_are_usable_and_the_references_agree(shape):
    """The box / cell case against strain64 meets the conditions; vjp64_large gives the same q, gxyz and gstrain."""
    w, mol, N, cell, g, q, gx, gs, kink_x, kink_s, _, figs = ms.periodic_case(shape)
    g64 = g.astype(np.float64)
    n = len(g)
    qf, gf, gsf = vjp64_large(mol[0], mol[1], mol[2], g64, w, N=N, cell=cell, strain=True)
    assert np.abs(q[:n] - qf).max() <= REL * np.abs(q).max()
    assert np.abs(gx - gf).max() <= REL * np.abs(gx).max() and np.abs(gs - gsf).max() <= REL * np.abs(gs).max()


@sized
def test_forward_mode_cases_are_usable_and_the_references_agree(shape, size):
    """The case with v, strain and dQ together meets the conditions; jvp64_factorised gives the same q and tq; g . tq = gxyz . v between
    jvp64 (v alone) and vjp64."""
    w, mol, N, tan, q, tq, kink, fig = ms.jvp_case(shape, size)
    kw = dict(N=N, v=tan["v"], strain=tan["strain"], dQ=float(tan["dQ"]))
    qf, tf = jvp_ref.jvp64_factorised(mol[0], mol[1], mol[2], w, **kw)
    assert np.abs(q - qf).max() <= 1e-12 * max(1.0, np.abs(q).max())
    assert np.abs(tq - tf).max() <= 1e-11 * max(1.0, np.abs(tq).max()), np.abs(tq - tf).max()
    n = len(q)
    g = np.random.default_rng(50 + n).normal(size=n)
    v = tan["v"].astype(np.float64)
    tv = jvp_ref.jvp64(mol[0], mol[1], mol[2], w, N=N, v=v)[1]
    q_r, gx = vjp64(mol[0], mol[1], mol[2], g, w, N=N)
    assert np.abs(q - q_r[:n]).max() <= 1e-12
    lhs, rhs = g @ tv, (gx * v).sum()
    scale = np.abs(g) @ np.abs(tv) + np.abs(gx * v).sum()
    assert scale > 1e-6 and abs(lhs - rhs) <= 1e-9 * scale, (lhs, rhs, scale)


@shapes
def test_training_case_is_usable_and_the_references_agree(shape):
    """The x rows of every first-layer weight gradient are non-zero in the dense training oracle; train_large_ref gives the same loss,
    charges and gradient per tensor."""
    w, mols, cells, N = ms.train_case(shape)
    D = _dense(mols, cells, N)
    loss_ref, pred_ref, g_ref = ot.loss_and_grads(*D, w)
    ms.train_conditions(shape, g_ref, f"nx = {shape[0]}, T = {shape[1]}, training")
    off, xyz, x, Q, y, cell = _train_batch(mols, cells)
    loss, q, g = batch_loss_and_grads_large(off, xyz, x, Q, y, w, N, cells=cells)
    assert abs(loss - loss_ref) <= 1e-12 * max(loss_ref, 1.0)
    for b in range(len(mols)):
        assert np.abs(q[off[b]:off[b + 1]] - pred_ref[b, :off[b + 1] - off[b], 0]).max() <= 1e-12
    _compare(ot.unflatten(g, w), g_ref, str(shape))
