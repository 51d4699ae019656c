"""Every entry at nx = 1..10 and T = 1..8 (the ten (nx, T) pairs of tests/model_shapes.py) against the float64 references run at the same
shape: the forward on its five routes and on the tiled kernels' row tiles, the dense entries, both gradient paths with strain, the
forward mode (single and K = 5), the Coulomb call (coulomb_xyz), the three training routes, and the scratch the pair-list entries
report at T = 1 and T = 8.  GPU only.

No tolerance of its own: the forward within TOL = 1e-5 (tests/test_gpu_parity.py); the layer calls within max(TOL, 3 x float32-oracle
noise) (tests/test_gpu_api.py); derivatives within 2e-4 max |ref| + the ReLU-kink bracket at TAU = 2e-5, here per component
(|got - ref|_i <= 2e-4 max |ref| + kink_i) beside the whole-array bound of test_gpu_grad_large._check; the adjoint identity within
test_gpu_jvp._adjoint's bound; training gradients by the per-tensor rule of tests/test_gpu_train_cell.py, which the x rows of each
first-layer gradient also meet on their own; scratch within 1 % of the formulas of include/epnn.h; the Coulomb call's phi, ffix and E
within BOUND = 2e-6 of their absolute sums on the device charges (tests/test_gpu_coulomb.py), its fq by the derivatives' rule.

Every case first passes the conditions of tests/model_shapes.py on the references alone.  The chosen seeds and what they measure:
forward (weight seed, scale): float32 noise and the smallest of the three sensitivities (last step, column 0, column nx - 1) in q
for the batches at N = 32 / N = 64 / the 150-atom molecule; derivatives (weight seed, scale, molecule seed): share of the components
(atoms for tq) inside the bracket, largest bracket / scale, smallest sensitivity in bounds of the components inside (> 100 asked);
training (weights seed 13, scale 0.4): the smallest x row of a first-layer gradient over its tensor's largest entry; coulomb: fq of
the Coulomb call at alpha = 0.3, the same three figures.

  nx = 1, T = 8
    forward (17, 0.25): noise 4.4e-07 / 4.9e-07 / 1.2e-06; sensitivity 3.3e-01 / 4.9e-01 / 9.3e-01
    gxyz, open (17, 24) (8, 0.6, 43): 92 %, 3.5e-04, 2424;  tq (17, 24) (5, 0.6, 40): 100 %, 1.3e-04, 1594
    gxyz, open (33, 40) (6, 0.6, 44): 85 %, 6.3e-03, 1019;  tq (33, 40) (9, 0.6, 43): 85 %, 8.9e-04, 1356
    box (20, 24) (7, 0.6, 41): gxyz 100 %, 2.1e-08, 2527; gstrain 100 %, 7.6e-09, 2338;  training x rows 5.0e-01
    coulomb fq, open (17, 24) (8, 0.6, 43): 92 %, 3.7e-04, 2503
  nx = 2, T = 1
    forward (18, 0.35): noise 7.4e-07 / 6.7e-07 / 8.6e-07; sensitivity 3.9e-02 / 7.9e-02 / 1.2e-01
    gxyz, open (17, 24) (5, 0.6, 44): 100 %, 0.0e+00, 2284;  tq (17, 24) (5, 0.6, 45): 100 %, 0.0e+00, 1090
    cell (20, 24) (5, 0.6, 42): gxyz 100 %, 0.0e+00, 1567; gstrain 100 %, 0.0e+00, 1387;  training x rows 4.8e-02
    coulomb fq, open (17, 24) (5, 0.6, 44): 100 %, 0.0e+00, 750
  nx = 3, T = 6
    forward (17, 0.35): noise 2.4e-07 / 3.3e-07 / 1.0e-06; sensitivity 3.7e-02 / 4.4e-02 / 2.4e-02
    gxyz, open (17, 24) (9, 0.35, 42): 90 %, 3.2e-03, 1236;  tq (17, 24) (9, 0.35, 42): 88 %, 3.4e-03, 794
    box (20, 24) (8, 0.6, 43): gxyz 100 %, 1.1e-04, 1767; gstrain 100 %, 1.3e-04, 1412;  training x rows 2.6e-02
    coulomb fq, open (17, 24) (9, 0.35, 42): 84 %, 3.8e-03, 1110
  nx = 4, T = 7
    forward (17, 0.35): noise 4.4e-07 / 7.5e-07 / 8.2e-07; sensitivity 1.1e-01 / 2.1e-01 / 3.4e-01
    gxyz, open (17, 24) (5, 0.6, 40): 71 %, 5.0e-03, 560;  tq (17, 24) (8, 0.35, 45): 76 %, 1.7e-02, 1156
    cell (20, 24) (6, 0.6, 43): gxyz 100 %, 1.3e-06, 1123; gstrain 100 %, 5.0e-06, 3838;  training x rows 2.4e-02
    coulomb fq, open (17, 24) (5, 0.6, 41): 75 %, 7.8e-03, 1634
  nx = 5, T = 4
    forward (17, 0.35): noise 3.4e-07 / 6.1e-07 / 8.0e-07; sensitivity 1.5e-01 / 2.7e-01 / 3.8e-01
    gxyz, open (17, 24) (7, 0.6, 40): 100 %, 1.6e-04, 552;  tq (17, 24) (7, 0.6, 40): 100 %, 1.1e-05, 437
    gxyz, open (33, 40) (7, 0.6, 40): 90 %, 2.8e-02, 609;  tq (33, 40) (9, 0.6, 42): 82 %, 5.9e-03, 1018
    box (20, 24) (5, 0.6, 40): gxyz 100 %, 9.3e-06, 1288; gstrain 100 %, 5.9e-06, 2017;  training x rows 1.1e-02
    coulomb fq, open (17, 24) (7, 0.6, 40): 100 %, 8.5e-05, 397
  nx = 6, T = 8
    forward (17, 0.35): noise 6.0e-07 / 1.7e-06 / 1.4e-06; sensitivity 9.3e-02 / 2.1e-01 / 2.4e-01
    gxyz, open (17, 24) (6, 0.6, 43): 92 %, 7.0e-03, 1065;  tq (17, 24) (6, 0.6, 43): 88 %, 3.1e-03, 1051
    cell (20, 24) (5, 0.6, 42): gxyz 100 %, 1.6e-07, 1020; gstrain 100 %, 1.2e-07, 723;  training x rows 9.3e-03
    coulomb fq, open (17, 24) (6, 0.6, 43): 84 %, 2.4e-02, 329
  nx = 7, T = 1
    forward (17, 0.35): noise 2.8e-07 / 2.9e-07 / 6.0e-07; sensitivity 9.3e-02 / 1.8e-01 / 2.4e-01
    gxyz, open (17, 24) (5, 0.6, 42): 100 %, 0.0e+00, 1014;  tq (17, 24) (5, 0.6, 42): 100 %, 0.0e+00, 1641
    box (20, 24) (5, 0.6, 40): gxyz 100 %, 0.0e+00, 299; gstrain 100 %, 0.0e+00, 482;  training x rows 5.9e-03
    coulomb fq, open (17, 24) (5, 0.6, 42): 100 %, 0.0e+00, 957
  nx = 8, T = 6
    forward (17, 0.35): noise 6.0e-07 / 9.6e-07 / 1.6e-06; sensitivity 1.4e-01 / 2.0e-01 / 3.3e-01
    gxyz, open (17, 24) (7, 0.6, 42): 92 %, 1.7e-03, 715;  tq (17, 24) (8, 0.6, 45): 100 %, 2.9e-05, 779
    gxyz, open (33, 40) (6, 0.6, 44): 83 %, 7.3e-04, 299;  tq (33, 40) (6, 0.6, 44): 76 %, 2.4e-03, 624
    cell (20, 24) (5, 0.6, 41): gxyz 100 %, 9.4e-05, 1175; gstrain 100 %, 8.1e-05, 1498;  training x rows 4.4e-03
    coulomb fq, open (17, 24) (7, 0.6, 42): 88 %, 5.4e-03, 1127
  nx = 9, T = 7
    forward (17, 0.35): noise 7.6e-07 / 1.1e-06 / 1.5e-06; sensitivity 8.1e-02 / 1.2e-01 / 2.0e-01
    gxyz, open (17, 24) (5, 0.6, 43): 100 %, 1.3e-04, 472;  tq (17, 24) (5, 0.6, 43): 88 %, 9.9e-04, 831
    box (20, 24) (7, 0.6, 42): gxyz 100 %, 8.0e-06, 1194; gstrain 100 %, 1.2e-05, 801;  training x rows 2.7e-03
    coulomb fq, open (17, 24) (5, 0.6, 43): 88 %, 1.1e-03, 971
  nx = 10, T = 8
    forward (18, 0.3): noise 4.8e-07 / 1.5e-06 / 1.7e-06; sensitivity 2.0e-02 / 2.8e-02 / 4.5e-02
    gxyz, open (17, 24) (6, 0.6, 43): 96 %, 3.1e-04, 121;  tq (17, 24) (6, 0.6, 43): 94 %, 1.1e-03, 117
    cell (20, 24) (5, 0.6, 41): gxyz 100 %, 7.5e-08, 121; gstrain 100 %, 4.8e-08, 105;  training x rows 1.5e-03
    coulomb fq, open (17, 24) (6, 0.6, 43): 96 %, 2.1e-03, 121

Measured on an MI355X (worst over the ten shapes): forward |dq| 1.6e-6 on the five routes and 2.0e-6 on the tiled kernels at 150 atoms; make_model 6.7e-7, GNN_layer 3.7e-8 and
EPN_layer 7.0e-7 (float32-oracle noise 2.3e-8 and 5.7e-7); gxyz 8.0e-7, gstrain 8.6e-7 and tq 3.8e-7 of their scale, every component
inside its own bound by at least 9e-6 of absolute slack; training gradients 1.7e-5 per tensor and 1.3e-5 on the x rows alone (the
float32 oracle's own noise); scratch within 0.02 % (forward mode) and 0.23 % (gradient call) of the formulas; the Coulomb call's
phi 1.1e-7, ffix 1.9e-7 and E 3.3e-8 of their absolute sums, its q within 3.8e-6 and its fq within 1.3e-6 of its scale, every
component inside its own bound by at least 1.3e-5 of absolute slack.  No shape failed: no kernel or host driver needed a change.
"""

import numpy as np
import pytest

import edge_constants as ec
import model_shapes as ms
from conftest import random_weights
from oracle import epnn_oracle as orc
from oracle import epnn_oracle_train as ot
from test_gpu_coulomb import _check_call
from test_gpu_edge_constants import IN_KERNEL, ROUTES
from test_gpu_grad_large import _batch, _check
from test_gpu_jvp import _adjoint, _formula
from test_gpu_jvp_multi import _formula_multi
from test_gpu_train_cell import _oracle, _step_against_oracle

pytestmark = pytest.mark.gpu

TOL = ms.TOL
TAU = ms.TAU
shapes = pytest.mark.parametrize("shape", ms.SHAPES, ids=ms.IDS)
SIZED = [(s, "small") for s in ms.SHAPES] + [(s, "large") for s in ms.OPEN_LARGE]
SIZED_IDS = [f"nx{s[0]}-T{s[1]}-{size}" for s, size in SIZED]


def _engine(factory, shape, w, **options):
    eng = factory(nx=shape[0], T=shape[1])
    eng.set_weights(w)
    for k, v in options.items():
        eng.set_option(k, v)
    return eng


def _components(got, ref, kink, what):
    """The per-component rule: |got - ref|_i <= 2e-4 max |ref| + kink_i."""
    scale = np.abs(ref).max()
    err = np.abs(np.asarray(got, np.float64) - ref)
    print(f"{what}: max error {err.max():.3e} of {scale:.3e}, worst excess over the component's bound {(err - 2e-4 * scale - kink).max():.3e}")
    assert scale > 0 and (err <= 2e-4 * scale + kink).all(), (what, np.argmax(err - kink), err.max(), scale)


# ---------------------------------------------------------------------------------------------------- forward
@shapes
@pytest.mark.parametrize("group", ["N32", "N64"])
def test_forward_on_every_route(gpu_engine_factory, shape, group):
    """2, 15, 16, 17 and 32 atoms at N = 32, 33, 48 and 64 atoms at N = 64 on the five routes of test_gpu_edge_constants against
    orc.forward_xyz in float64; every route reports the reference's listed pairs, the in-kernel routes keep every molecule on the
    fused kernels."""
    w, mols, N, ref, fig = ms.forward_case(shape, group)
    off, xyz, x, Q = _batch(mols)
    counts = [ec.pair_counts(m[0], ec.DEFAULT) for m in mols]
    listed, near = sum(c[0] for c in counts), sum(c[1] for c in counts)
    for name, opts in ROUTES:
        eng = _engine(gpu_engine_factory, shape, w, **opts)
        q = eng.forward_xyz(off, xyz, x, Q, N=N)
        st = eng.last_stats()
        err = max(float(np.abs(q[off[k]:off[k + 1]] - ref[k][:len(m[0])]).max()) for k, m in enumerate(mols))
        print(f"{shape} {group}, {name}: worst |dq| {err:.2e}; stats {tuple(int(v) for v in st[:3])}; the reference lists {listed} pairs")
        assert st[0] == listed, (name, st[0], listed)
        if name in IN_KERNEL:
            assert st[1] == len(mols), (name, st)
        else:
            pi, pj, wt, npairs = eng.debug_pairs(listed + 8)
            assert npairs == listed and int((wt != 0).sum()) == near, (name, npairs, listed, near)
        assert err <= TOL, (name, err)


@shapes
@pytest.mark.parametrize("dedupe", [1, 0])
def test_forward_150_atoms_on_the_tiled_kernels(gpu_engine_factory, shape, dedupe):
    """One 150-atom lattice molecule on force_path = 2: more than one row tile, the first step by types (large_dedupe = 1) and by
    the sweep (0)."""
    w, mols, N, ref, fig = ms.forward_case(shape, "n150")
    off, xyz, x, Q = _batch(mols)
    listed, near = ec.pair_counts(mols[0][0], ec.DEFAULT)
    eng = _engine(gpu_engine_factory, shape, w, force_path=2, large_dedupe=dedupe)
    q = eng.forward_xyz(off, xyz, x, Q, N=N)
    st = eng.last_stats()
    err = float(np.abs(q - ref[0][:150]).max())
    pi, pj, wt, npairs = eng.debug_pairs(listed + 8)
    print(f"{shape} 150 atoms, large_dedupe = {dedupe}: |dq| {err:.2e}; {npairs} pairs listed, the reference {listed}")
    assert st[0] == listed and npairs == listed and int((wt != 0).sum()) == near
    assert err <= TOL


# ---------------------------------------------------------------------------------------------------- dense entries
@shapes
def test_dense_entries(gpu_engine_factory, shape):
    """make_model(...)([h, e, x, q, mask]) and the GNN_layer / EPN_layer calls of tests/test_gpu_api.py on orc.dense_inputs of three
    molecules (20, 13 and 7 atoms at N = 20) against the float64 oracle."""
    from epnn_amd import charge_gn
    nx, T = shape
    w = ms.forward_case(shape, "N32")[0]
    N = 20
    mols = [ms.lattice_molecule(n, nx, seed=n) for n in (20, 13, 7)]
    ref_mols, fig = ms.forward_conditions(shape, w, mols, N, f"{shape} dense entries")
    parts = [orc.dense_inputs(m[0], m[1], m[2], N) for m in mols]
    h, e, x, q, mask = (np.stack([p[k] for p in parts]).astype(np.float32) for k in range(5))
    ref = orc.model_forward(h, e, x, q, mask, w, dtype=np.float64)
    assert np.abs(ref[:, :, 0] - np.stack(ref_mols)).max() <= 1e-12            # (the batch against forward_xyz per molecule)
    model = charge_gn.make_model([32, 32], 48, T, nx, N)
    model.set_weights_dict(w)
    pred = model([h, e, x, q, mask])
    err = float(np.abs(pred - ref).max())
    print(f"{shape} make_model: |dq| {err:.2e}")
    assert pred.shape == (3, N, 1) and err <= TOL
    for b, m in enumerate(mols):
        assert np.all(pred[b, len(m[0]):] == 0)
    # the layer calls, with non-trivial h and q as in test_layer_calls_vs_oracle
    rng = np.random.default_rng(1)
    hx, xx, qx, m4 = orc.model_reduce(h, x, q, mask)
    hx = (rng.normal(size=hx.shape) * 0.2 * (xx[..., :1] != 0)).astype(np.float32)
    qx = (qx + 0.05 * rng.normal(size=qx.shape) * (xx[..., :1] != 0)).astype(np.float32)
    gnn = charge_gn.GNN_layer(charge_gn.MLP_layer, charge_gn.MLP_layer([32, 32], out_dim=48), T)
    for t in range(T):
        gnn.message_fns[t].set_weights(w["msg"][t])
    gnn.update_fn.set_weights(w["upd"])
    h_gpu = gnn.call(hx, e, xx, qx, m4)
    h_ref = orc.gnn_layer(hx, e, xx, qx, m4, w["msg"], w["upd"], dtype=np.float64)
    noise = np.abs(orc.gnn_layer(hx, e, xx, qx, m4, w["msg"], w["upd"], dtype=np.float32) - h_ref).max()
    err = np.abs(h_gpu - h_ref).max()
    print(f"{shape} GNN_layer.call: |dh| {err:.3e} (noise {noise:.3e}, |h| up to {np.abs(h_ref).max():.2f})")
    assert np.abs(h_ref).max() > 100 * TOL and err <= max(TOL, 3 * noise)
    epn = charge_gn.EPN_layer(charge_gn.MLP_layer, T=T)
    for t in range(T):
        epn.pass_fns[t].set_weights(w["pas"][t])
    h32 = h_ref.astype(np.float32)
    q_gpu = epn.call(h32, e, xx, qx, m4)
    q_ref = orc.epn_layer(h32, e, xx, qx, m4, w["pas"], dtype=np.float64)
    noise = np.abs(orc.epn_layer(h32, e, xx, qx, m4, w["pas"], dtype=np.float32) - q_ref).max()
    err = np.abs(q_gpu - q_ref).max()
    print(f"{shape} EPN_layer.call: |dq| {err:.3e} (noise {noise:.3e})")
    assert np.abs(q_ref - qx).max() > 100 * TOL and err <= max(TOL, 3 * noise)


# ---------------------------------------------------------------------------------------------------- gradients
@pytest.mark.parametrize("shape,size", SIZED, ids=SIZED_IDS)
def test_gradients_of_the_open_case(gpu_engine_factory, shape, size):
    """charges_vjp_xyz on the dense path (row-fused and layer-by-layer kernels) and on the pair-list path against vjp64:
    test_gpu_grad_large._check's whole-array bounds and the per-component rule.  17 atoms at N = 24; for nx = 1, 5 and 8 also 33 atoms
    at N = 40 (three 16-row tiles of the pair-list kernels)."""
    w, mol, N, g, q_ref, gxyz, kink, (lo, hi), fig = ms.open_case(shape, size)
    off, xyz, x, Q = _batch([mol])
    by_shift = {0.0: gxyz, +TAU: lo, -TAU: hi}
    ref_fn = lambda xyz, x, Q, g, N, h_dim, kink_shift=0.0: (q_ref, by_shift[kink_shift])
    for fused in (1, 0):
        eng = _engine(gpu_engine_factory, shape, w, train_fused=fused)
        _check(eng, [mol], N, [ref_fn])
        for path in (1, 2):
            eng.set_option("grad_path", path)
            q, gx = eng.charges_vjp_xyz(off, xyz, x, Q, g, N)
            assert np.abs(q - q_ref[:len(q)]).max() <= 2e-4
            _components(gx, gxyz, kink, f"{shape} {size} gxyz, train_fused = {fused}, grad_path = {path}")


@shapes
def test_gradients_and_strain_in_a_cell(gpu_engine_factory, shape):
    """strain=True on both paths (the dense one with both kernel sets) for 20 atoms at N = 24 in the box 7.5 x 7.0 x 7.2 (as
    cell=np.diag(box); box= itself without strain) or in the sheared cell, alternating over the shapes, against strain64."""
    w, mol, N, cell, g, q_ref, gxyz, gstrain, kink_x, kink_s, (lo, hi), figs = ms.periodic_case(shape)
    off, xyz, x, Q = _batch([mol])
    kind = ms.PERIODIC[shape][0]
    by_shift = {0.0: gxyz, +TAU: lo[0], -TAU: hi[0]}
    ref_fn = lambda xyz, x, Q, g, N, h_dim, kink_shift=0.0: (q_ref, by_shift[kink_shift])
    scale = np.abs(gstrain).max()
    for fused in (1, 0):
        eng = _engine(gpu_engine_factory, shape, w, train_fused=fused)
        _check(eng, [mol], N, [ref_fn], cell=cell)
        gs = {}
        for path in (2, 1):
            eng.set_option("grad_path", path)
            what = f"{shape} {kind}, train_fused = {fused}, grad_path = {path}"
            q, gx, gs[path] = eng.charges_vjp_xyz(off, xyz, x, Q, g, N, strain=True, cell=cell)
            assert np.abs(q - q_ref[:len(q)]).max() <= 2e-4
            _components(gx, gxyz, kink_x, what + " gxyz")
            _components(gs[path][0], gstrain, kink_s, what + " gstrain")
            if kind == "box":
                qb, gb = eng.charges_vjp_xyz(off, xyz, x, Q, g, N, box=ms.BOX)
                assert np.abs(qb - q_ref[:len(q)]).max() <= 2e-4
                _components(gb, gxyz, kink_x, what + " gxyz with box=")
        assert np.abs(gs[2] - gs[1]).max() <= 4e-4 * scale + kink_s.max()


# ---------------------------------------------------------------------------------------------------- the Coulomb call
@shapes
def test_coulomb(gpu_engine_factory, shape):
    """coulomb_xyz at alpha = 0.3 on the 17-atom open molecule at N = 24: phi, ffix and E against coulomb64 on the device charges at
    test_gpu_coulomb's BOUND, the bits of charges_vjp_xyz(g=phi) on the pair-list path, q within 2e-4 of the reference and fq =
    -vjp64(g = phi_ref) by the per-component rule."""
    w, mol, N, q_ref, phi_ref, fq_ref, kink, _, fig = ms.coulomb_case(shape)
    eng = _engine(gpu_engine_factory, shape, w, grad_path=2)
    q, phi, E, F, ffix, fq = _check_call(eng, mol, N, ms.COULOMB_ALPHA, f"{shape} coulomb")
    print(f"{shape} coulomb: q {np.abs(q - q_ref).max():.3e}, phi {np.abs(phi - phi_ref).max():.3e} of {np.abs(phi_ref).max():.3e}")
    assert np.abs(q - q_ref).max() <= 2e-4
    _components(fq, fq_ref, kink, f"{shape} coulomb fq")


# ---------------------------------------------------------------------------------------------------- forward mode
@pytest.mark.parametrize("shape,size", SIZED, ids=SIZED_IDS)
def test_forward_mode(gpu_engine_factory, shape, size):
    """charges_jvp_xyz with v, strain and dQ together against jvp64, per atom; charges_jvp_xyz_multi at K = 5 (v, strain, dQ, all
    three, twice v: one launch of four and one of one): every row carries the bits of the single call; the primal bits of the
    pair-list gradient call and the adjoint identity (test_gpu_jvp._adjoint)."""
    w, mol, N, tan, q_ref, ref, kink, fig = ms.jvp_case(shape, size)
    off, xyz, x, Q = _batch([mol])
    eng = _engine(gpu_engine_factory, shape, w, grad_path=2)
    q, tq = eng.charges_jvp_xyz(off, xyz, x, Q, N, **tan)
    assert np.abs(q - q_ref).max() <= 2e-4
    _components(tq, ref, kink, f"{shape} {size} tq")
    v, E, t = tan["v"], tan["strain"], np.float32([tan["dQ"]])
    zv, zE, zt = np.zeros_like(v), np.zeros_like(E), np.zeros_like(t)
    rows = [(v, zE, zt), (zv, E, zt), (zv, zE, t), (v, E, t), (2 * v, zE, zt)]
    qm, tm = eng.charges_jvp_xyz_multi(off, xyz, x, Q, N, v=np.stack([r[0] for r in rows]), strain=np.stack([r[1] for r in rows]),
                                       dQ=np.stack([r[2] for r in rows]))
    assert np.array_equal(qm, q) and np.array_equal(tm[3], tq)
    for k, (rv, rE, rt) in enumerate(rows):
        q1, t1 = eng.charges_jvp_xyz(off, xyz, x, Q, N, v=rv, strain=rE, dQ=rt)
        assert np.array_equal(q1, q) and np.array_equal(t1, tm[k]), k
        assert np.abs(t1).max() > 0
    _adjoint(eng, off, xyz, x, Q, N, {}, {"v": v, "strain": E[None]}, seed=41)


# ---------------------------------------------------------------------------------------------------- training
def _x_block(vec, w, nx, part, t):
    """The rows of x (0..nx-1 and F..F+nx-1) of the first-layer kernel of msg[t] / pas[t] in a flat parameter vector."""
    return np.asarray(ot.unflatten(np.asarray(vec, np.float64), w)[part][t][0][0])[ms.x_rows(nx)]


@pytest.mark.parametrize("path,fused", [(1, 1), (1, 0), (2, 1)])
@shapes
def test_train_step(gpu_engine_factory, shape, path, fused):
    """train_step_xyz without the optimizer on one open 13-atom molecule and 24 atoms in a 6.5 A cubic cell (N = 24): the dense
    row-fused and layer-by-layer kernels and the pair-list path against the training oracle (test_gpu_train_cell's per-tensor rule),
    and the rows of x of every first-layer weight gradient by the same rule on their own."""
    nx, T = shape
    w, mols, cells, N = ms.train_case(shape)
    key = f"model shape {nx} {T}"
    loss_ref, pred_ref, gr, g32, band = _oracle(key, mols, cells, N, w)
    ms.train_conditions(shape, ot.unflatten(gr, w), key)
    eng = _step_against_oracle(gpu_engine_factory, key, mols, cells, N, w, nx, path, fused)
    g = eng.get_gradients()
    worst = 0.0
    for t in range(T):
        for part in ("msg", "pas"):
            got, ref, r32, bd = (_x_block(a, w, nx, part, t) for a in (g, gr, g32, band))
            scale = np.abs(ref).max()
            assert scale > 0
            noise, kink, err = np.abs(r32 - ref).max() / scale, bd.max() / scale, np.abs(got - ref).max() / scale
            worst = max(worst, err)
            assert err <= max(2e-4, 4 * noise) + 2 * kink, (part, t, err, noise, kink)
    print(f"{key} train_path={path} train_fused={fused}: worst relative error of the x rows {worst:.2e}")


# ---------------------------------------------------------------------------------------------------- scratch
def _formula_vjp(ns, nx, T, pairs):
    """include/epnn.h: bytes = A (1324 + 4 nx + 324 T + 257 pieces) + 1120 listed pairs + 13 KB"""
    pieces = max(min(16, max(1, -(-2048 // -(-n // 16)))) for n in ns)
    return sum(ns) * (1324 + 4 * nx + 324 * T + 257 * pieces) + 1120 * pairs + 13 * 1024


@pytest.mark.parametrize("shape", [s for s in ms.SHAPES if s[1] in (1, 8)], ids=[i for i, s in zip(ms.IDS, ms.SHAPES) if s[1] in (1, 8)])
def test_scratch_follows_the_formulas(gpu_engine_factory, shape):
    """The bytes last_stats() reports for the 150-atom molecule at T = 1 and T = 8: the forward mode (single and K = 5) keeps no
    checkpoints and its formula no T; the gradient call keeps h, S and q of every step."""
    nx, T = shape
    w = random_weights(nx, T, seed=5, scale=0.35)
    xyz, x, Q = ms.lattice_molecule(150, nx, seed=150)
    off, Qa = np.int32([0, 150]), np.float32([Q])
    listed = ec.pair_counts(xyz, ec.DEFAULT)[0]
    v = np.random.default_rng(1).normal(size=(5, 150, 3)).astype(np.float32)
    eng = _engine(gpu_engine_factory, shape, w, grad_path=2)
    eng.charges_jvp_xyz(off, xyz, x, Qa, 150, v=v[0])
    st, want = eng.last_stats(), _formula([150], nx, listed, True)
    print(f"{shape} forward mode: {st[0]} pairs, {st[2]} bytes, formula {want}")
    assert st[0] == listed and st[1] == 0 and abs(int(st[2]) - want) <= 0.01 * want
    eng = _engine(gpu_engine_factory, shape, w, grad_path=2)
    eng.charges_jvp_xyz_multi(off, xyz, x, Qa, 150, v=v)
    st, want = eng.last_stats(), _formula_multi([150], nx, listed, 5, True)
    print(f"{shape} forward mode, K = 5: {st[0]} pairs, {st[2]} bytes, formula {want}")
    assert st[0] == listed and st[1] == 0 and abs(int(st[2]) - want) <= 0.01 * want
    eng = _engine(gpu_engine_factory, shape, w, grad_path=2)
    eng.charges_vjp_xyz(off, xyz, x, Qa, v[0, :, 0].copy(), 150)
    st, want = eng.last_stats(), _formula_vjp([150], nx, T, listed)
    print(f"{shape} gradient call: {st[0]} pairs, {st[2]} bytes, formula {want}")
    assert st[0] == listed and st[1] == 0 and abs(int(st[2]) - want) <= 0.01 * want
