"""cutoff, eta and near_tol away from the reference's 3.0 / 2.0 / 1e-5 on every kernel family, against the float64 references run at
the same constants (tests/edge_constants.py: the sets A, B, C and what makes an input a usable case): the forward on its routes, open
and periodic, the dense entries, both gradient paths with strain, the Coulomb call (coulomb_xyz), the forward mode and the training
steps.  GPU only.

No tolerance of its own: the forward within TOL = 1e-5 (tests/test_gpu_parity.py); derivatives within 2e-4 max |ref| + the ReLU-kink
bracket at TAU = 2e-5 (tests/test_gpu_grad_large.py, per atom for the forward mode as in tests/test_gpu_jvp.py); training gradients by
the per-tensor rule of tests/test_gpu_train_cell.py; the adjoint identity within test_gpu_jvp._adjoint's bound; the Coulomb call's
phi, ffix and E within BOUND = 2e-6 of their absolute sums on the device charges (tests/test_gpu_coulomb.py), its fq = -vjp(g = phi) by
the derivatives' rule per component.

Every case first passes, on the references alone: no listed pair within 1e-5 (relative, in max_k e_k / near_tol) of a flip of the near
flag; for set C at least 5 listed pairs in each of the four flag intervals; the reference at the set differs from the reference at the
default constants (same weights) by more than 100 times the bound the comparison really grants (for gradients 2e-4 max |ref| + the
largest bracket; in the forward mode, whose bound is per atom, over the atoms inside the bracket); derivative cases have at least
70 % of their components (gradients, strain) or atoms (forward mode) with a bracket <= 2e-4 max |ref|.  Measured on the references (margin; pairs per flag interval; sensitivity):

  forward, N = 32 (2, 15, 16, 17, 32 atoms) and N = 64 (33, 48, 64 atoms), weights seed 17 scale 0.35:
    A  9.1e-1; 492 / 1        and 1.2e-2; 1269 / 10;            0.14 and 0.27 in q
    B  1.5e-2; 679 / 41       and 6.6e-3; 2082 / 301;           2.9e-2 and 3.7e-2
    C  1.8e-3; 396/37/74/213  and 1.0e-4; 962/118/275/1028;     7.2e-2 and 0.23
  flip edges (set C, 16 molecules): margin 3.3e-5; 10 / 8 / 6 / 6 listed pairs, the two far pairs beyond the cutoff not listed
  forward-mode cases (share of atoms inside the bracket, largest bracket / scale), weights seed 5 scale 0.6:
    A lattice (40, 40): v 95 %, 4.6e-2; v + strain + dQ 95 %, 6.1e-2
    B lattice (33, 40): v 94 %, 8.2e-4; v + strain + dQ 82 %, 1.4e-3
    C lattice (33, 40): v 91 %, 8.3e-4; v + strain + dQ 94 %, 5.4e-4     C lattice (17, 24): v 100 %, 3.6e-5
  gradients (share of the components inside the bracket; largest bracket / scale; sensitivity / (2e-4 scale + largest bracket)):
    open  A lattice (48, 48) seed 148: 100 %, 1.8e-4, 3013;  B (33, 40): 98 %, 6.3e-4, 874;  C (33, 40): 90 %, 9.8e-4, 433
    box   A seed 42: 100 %, 1.1e-5, 4936;  B seed 40: 98 %, 6.9e-4, 719;  C seed 40: 100 %, 6.1e-5, 1424
    cell  (seed 42) gxyz A 100 %, 1.9e-4, 2600;  B 100 %, 1.9e-4, 2730;  C 100 %, 8.6e-6, 2236
          gstrain   A 100 %, 1.3e-4, 2258;  B 100 %, 1.6e-4, 799;   C 100 %, 1.5e-5, 4148
    (set A on the lattice (40, 40) and in the box with seed 40 has brackets of 2.9e-2 and 7.2e-2 of the scale and a sensitivity of
    only 34 and 18 bounds: not usable, replaced by the cases above)
  coulomb, alpha = 0.3, on the open molecules of the gradients (margin; pairs per flag interval; q against the default constants; fq:
    share inside the bracket, largest bracket / scale, sensitivity in bounds of the components inside):
    A (48, 48)  9.4e-1; 423 / 2;            q 2.19;    fq 95 %, 5.1e-4, 3044
    B (33, 40)  1.1e-2; 349 / 31;           q 0.137;   fq 94 %, 2.3e-3, 1197
    C (33, 40)  1.0e-4; 186/17/41/136;      q 1.19;    fq 98 %, 7.7e-4, 830
  training (one open 13-atom molecule and 24 atoms in a 7.0 x 7.2 x 7.5 cell, N = 24): margins 4.8e-2 / 3.9e-3 / 4.9e-3; set C
    63 / 16 / 23 / 80 pairs per interval; the gradient differs from the default constants' by 744 .. 4770 tolerances

Measured on an MI355X: set C edge basis residual 8.2e-11; forward worst |dq| 5.3e-7 over all sets and routes; gxyz, gstrain and tq
errors below 1e-6 of their scale; training gradients below 1e-6 per tensor; the Coulomb call's phi / ffix / E 3.3e-8 / 6.1e-8 /
1.2e-9 (A), 5.1e-8 / 8.7e-8 / 9.7e-9 (B) and 3.7e-8 / 8.5e-8 / 6.2e-9 (C) of their absolute sums, q within 1.7e-6, fq within 3.3e-7,
5.3e-7 and 7.6e-7 of its scale.
"""
import functools

import numpy as np
import pytest

import cell_ref
import edge_constants as ec
import jvp_ref
import periodic_ref
from cell_ref import strain64
from conftest import random_weights
from grad_large_ref import vjp64_large
from oracle import epnn_oracle as orc
from oracle import epnn_oracle_train as ot
from periodic_ref import vjp64_pbc
from test_gpu_grad_large import _batch, _check, _features, _lattice_molecule
from test_gpu_jvp import _adjoint
from test_gpu_train_cell import _check_gradient
from train_large_ref import batch_loss_and_grads_large
from xyz_grad_ref import vjp64

pytestmark = pytest.mark.gpu

TOL = 1e-5           # tests/test_gpu_parity.py
TAU = 2e-5           # ReLU-kink bracket of the derivative references
TAU_TRAIN = 2e-6     # ... of the training oracle (tests/test_gpu_train_cell.py)
NX = 9

# the routes of test_gpu_parity.test_cutoff_and_is_near_edges_on_every_path
ROUTES = (("one wavefront per molecule", {"wave2": 0}), ("block per wavefront", {"wave2": 17}),
          ("separate front-end, fused kernel", {"wave_front": 0, "wave2": 0}), ("tiled kernels", {"force_path": 2}),
          ("tiled kernels, sweep in the first step", {"force_path": 2, "large_dedupe": 0}))
IN_KERNEL = ("one wavefront per molecule", "block per wavefront")

BOX = np.float32([7.5, 7.0, 7.2])                                          # every length >= 2 x 3.4
SHEARED = np.float32([[8, 0, 0], [2.5, 7.8, 0], [-2, 1.5, 7.6]])           # cell_ref.BASIS_A's shape; widths 7.27, 7.65, 7.60
ZERO = np.zeros((3, 3), np.float32)
DERIV = {"A": (40, 40), "B": (33, 40), "C": (33, 40)}                      # (n, N) of the lattice molecule of the derivative cases


def _engine(factory, s, w, **options):
    eng = factory(nx=NX, T=len(w["msg"]), **ec.engine_kwargs(s))
    eng.set_weights(w)
    for k, v in options.items():
        eng.set_option(k, v)
    return eng


def _fwd_kwargs(s):
    return dict(dtype=np.float64, cutoff=s.cutoff, eta=s.eta, near_tol=s.near_tol, h_dim=s.h_dim)


def _forward_routes(factory, s, w, mols, N, ref, what, front="in-kernel"):
    """The batch through the five routes: charges within TOL of ref, the listed pairs every route reports, the listed and near
    pairs of the device's own list where a route builds one."""
    off, xyz, x, Q = _batch(mols)
    counts = [ec.pair_counts(m[0], s) for m in mols]
    listed, near = sum(c[0] for c in counts), sum(c[1] for c in counts)
    worst = {}
    for name, opts in ROUTES:
        eng = _engine(factory, s, w, **opts)
        q = eng.forward_xyz(off, xyz, x, Q, N=N)
        st = eng.last_stats()
        err = max(float(np.abs(q[off[k]:off[k + 1]] - ref[k][:len(m[0])]).max()) for k, m in enumerate(mols))
        worst[name] = err
        print(f"{what}, {name}: worst |dq| {err:.2e}; stats {tuple(int(v) for v in st[:3])}; the reference lists {listed} pairs, {near} near")
        assert st[0] == listed, (what, name, st[0], listed)
        if name in IN_KERNEL and front == "in-kernel":
            assert st[1] == len(mols), (what, name, st)
        if name in IN_KERNEL and front == "fallback" and N > 32:
            assert st[1] == 0 and st[2] == len(mols), (what, name, st)
        if "wave_front" in opts or "force_path" in opts:
            pi, pj, wt, npairs = eng.debug_pairs(listed + 8)
            assert npairs == listed and int((wt != 0).sum()) == near, (what, name, npairs, int((wt != 0).sum()), listed, near)
        assert err <= TOL, (what, name, err)
    return worst


# ---------------------------------------------------------------------------------------------------- forward
@functools.lru_cache(maxsize=None)
def _forward_case(name, N):
    s = ec.SETS[name]
    w = random_weights(NX, 2, seed=17, scale=0.35, h_dim=s.h_dim)
    mols = [_lattice_molecule(n, NX, seed=n) for n in ((2, 15, 16, 17, 32) if N == 32 else (33, 48, 64))]
    ec.assert_admissible(mols, s, least=5 if name == "C" else 0, what=f"set {name}, N = {N}")
    ref = [orc.forward_xyz(m[0], m[1], m[2], w, N=N, **_fwd_kwargs(s)) for m in mols]
    dflt = [orc.forward_xyz(m[0], m[1], m[2], w, N=N, dtype=np.float64, h_dim=s.h_dim) for m in mols]
    ec.assert_sensitive(np.concatenate(ref), np.concatenate(dflt), TOL, f"set {name}, N = {N}")
    return s, w, mols, ref


@pytest.mark.parametrize("N", [32, 64])
@pytest.mark.parametrize("name", list(ec.SETS))
def test_forward_on_every_route(gpu_engine_factory, name, N):
    """2, 15, 16, 17 and 32 atoms at N = 32 (one wavefront, or a share of one), 33, 48 and 64 atoms at N = 64 (the three- and
    four-wavefront kernels) on the five routes, against orc.forward_xyz in float64 at the set's constants.  Set C must really run
    the three-flip count of the in-kernel front-end: the edge basis reproduces the five-Gaussian family (residual < 1e-8) and every
    molecule of the in-kernel routes stays on the fused kernels.  Which front-end ran is asserted for every set: B and C have a
    residual < 1e-8 and, at N = 64 (where only the in-kernel front-end feeds the 33..64-atom kernels), all molecules on the fused
    kernels; set A's residual is >= 1e-8, the library falls back to the 48-channel front-end and sends 33..64 atoms to the tiled kernels."""
    s, w, mols, ref = _forward_case(name, N)
    eng = _engine(gpu_engine_factory, s, w)
    res = float(eng.lib.epnn_edge_basis_residual(eng.h))
    print(f"set {name}: edge basis residual {res:.2e}")
    assert (res >= 1e-8) if name == "A" else (0.0 < res < 1e-8), (name, res)
    _forward_routes(gpu_engine_factory, s, w, mols, N, ref, f"set {name}, N = {N}", front="fallback" if name == "A" else "in-kernel")


@functools.lru_cache(maxsize=None)
def _flip_case():
    """test_gpu_parity.test_cutoff_and_is_near_edges_on_every_path where the flag has four transitions: 2- and 3-atom molecules whose
    far pair sits 2e-5 A on either side of each of set C's three flips and of the cutoff."""
    s = ec.SET_C
    w = random_weights(NX, 2, seed=77, scale=0.5, h_dim=s.h_dim)
    flips = ec.near_flips(*s)
    assert len(flips) == 3
    mols = []
    for k, edge in enumerate(list(flips) + [s.cutoff]):
        for D in (edge - 2e-5, edge + 2e-5):
            for third in (False, True):
                xyz = np.array([[0.0, 0.0, 0.0], [float(np.float32(D)), 0.0, 0.0]] + ([[0.3, 1.1, 0.2]] if third else []), np.float32)
                n = len(xyz)
                x = np.zeros((n, NX), np.float32)
                x[:, 0] = [6, 8, 1][:n]
                x[np.arange(n), [2, 4, 1][:n]] = 1
                mols.append((xyz, x, np.float32(k % 3 - 1)))
    ec.assert_admissible(mols, s, least=4, what="flip edges")
    # the far pair's own flag alternates along the list of distances: near | not | not near ... as the flips say, none beyond the cutoff
    far = [float(np.float32(m[0][1, 0])) for m in mols[::2]]
    want = [True, False, False, True, True, False, False, False]
    assert [bool(ec.flag(np.float64(D), *s)) for D in far] == want and [D < s.cutoff for D in far] == [True] * 7 + [False]
    ref = [orc.forward_xyz(m[0], m[1], m[2], w, N=5, **_fwd_kwargs(s)) for m in mols]
    dflt = [orc.forward_xyz(m[0], m[1], m[2], w, N=5, dtype=np.float64, h_dim=s.h_dim) for m in mols]
    ec.assert_sensitive(np.concatenate(ref), np.concatenate(dflt), TOL, "flip edges")
    return s, w, mols, ref


def test_flip_edges_on_every_route(gpu_engine_factory):
    s, w, mols, ref = _flip_case()
    _forward_routes(gpu_engine_factory, s, w, mols, 5, ref, "flip edges (set C)")


# ---------------------------------------------------------------------------------------------------- box and cell forward
def _periodic_mols(seed, ns, cell):
    out = []
    for k, n in enumerate(ns):
        rng = np.random.default_rng(seed + k)
        out.append((cell_ref.random_cell(rng, n, cell),) + _features(rng, n, NX))
    return out


@functools.lru_cache(maxsize=None)
def _cell_forward_case(name, kind):
    s = ec.SETS[name]
    w = random_weights(NX, 2, seed=7, scale=0.35, h_dim=s.h_dim)
    cell = np.diag(BOX).astype(np.float32) if kind == "box" else SHEARED
    assert (cell_ref.widths(cell) >= 2 * s.cutoff).all()
    mols = _periodic_mols(300, (4, 20, 32, 40, 64), cell)          # up to 32 atoms: the fused kernel on the front-end's list; above: tiled
    ec.assert_admissible(mols, s, [cell] * len(mols), least=5 if name == "C" else 0, what=f"set {name}, {kind}")
    if kind == "box":
        ref = [periodic_ref.forward_pbc(m[0], m[1], m[2], BOX, w, 64, np.float64, **ec.ref_kwargs(s)) for m in mols]
        dflt = [periodic_ref.forward_pbc(m[0], m[1], m[2], BOX, w, 64, np.float64, h_dim=s.h_dim) for m in mols]
    else:
        ref = [cell_ref.forward_cell(m[0], m[1], m[2], cell, w, 64, np.float64, **ec.ref_kwargs(s)) for m in mols]
        dflt = [cell_ref.forward_cell(m[0], m[1], m[2], cell, w, 64, np.float64, h_dim=s.h_dim) for m in mols]
    ec.assert_sensitive(np.concatenate(ref), np.concatenate(dflt), TOL, f"set {name}, {kind}")
    return s, w, mols, cell, ref


@pytest.mark.parametrize("kind", ["box", "sheared"])
@pytest.mark.parametrize("name", list(ec.SETS))
def test_box_and_cell_forward(gpu_engine_factory, name, kind):
    """Cells of 4..64 atoms at N = 64 (the routes of test_small_cells_on_every_route / test_small_general_cells_on_every_route: the
    fused kernel on the front-end's list up to 32 atoms, the tiled kernels above), every periodic width at least twice the set's
    cutoff, against forward_pbc / forward_cell."""
    s, w, mols, cell, ref = _cell_forward_case(name, kind)
    off, xyz, x, Q = _batch(mols)
    eng = _engine(gpu_engine_factory, s, w)
    geo = {"box": BOX} if kind == "box" else {"cell": cell}
    q = eng.forward_xyz(off, xyz, x, Q, 64, **geo)
    counts = [ec.pair_counts(m[0], s, cell) for m in mols]
    listed, near = sum(c[0] for c in counts), sum(c[1] for c in counts)
    err = max(float(np.abs(q[off[k]:off[k + 1]] - ref[k][:len(m[0])]).max()) for k, m in enumerate(mols))
    pi, pj, wt, npairs = eng.debug_pairs(listed + 8)
    print(f"set {name}, {kind}: worst |dq| {err:.2e}; the device lists {npairs} pairs, {int((wt != 0).sum())} near; the reference {listed}, {near}")
    assert npairs == listed and int((wt != 0).sum()) == near
    assert err <= TOL


def test_a_box_is_judged_by_the_engines_own_cutoff(gpu_engine_factory):
    """A 6.5 A box is accepted at cutoff 3.0 and refused by name at 3.4; the refusing handle stays usable."""
    from epnn_amd._lib import EpnnError
    w = random_weights(NX, 2, seed=7, scale=0.35)
    L = np.float32([6.5, 6.5, 6.5])
    rng = np.random.default_rng(12)
    mol = (periodic_ref.random_cell(rng, 20, L),) + _features(rng, 20, NX)
    off, xyz, x, Q = _batch([mol])
    eng = _engine(gpu_engine_factory, ec.DEFAULT, w)
    ref = periodic_ref.forward_pbc(mol[0], mol[1], mol[2], L, w, 24, np.float64)
    assert np.abs(eng.forward_xyz(off, xyz, x, Q, 24, box=L) - ref[:20]).max() <= TOL
    s = ec.EdgeSet(48, 3.4, 2.0, 1e-5)
    eng = _engine(gpu_engine_factory, s, w)
    g = np.ones(20, np.float32)
    for call in (lambda: eng.forward_xyz(off, xyz, x, Q, 24, box=L), lambda: eng.forward_xyz(off, xyz, x, Q, 24, cell=np.diag(L)),
                 lambda: eng.charges_vjp_xyz(off, xyz, x, Q, g, 24, box=L), lambda: eng.charges_jvp_xyz(off, xyz, x, Q, 24, dQ=1.0, box=L)):
        with pytest.raises(EpnnError, match="twice the cutoff"):
            call()
    big = np.float32([6.8, 6.8, 6.8])
    ref = periodic_ref.forward_pbc(mol[0], mol[1], mol[2], big, w, 24, np.float64, **ec.ref_kwargs(s))
    assert np.abs(eng.forward_xyz(off, xyz, x, Q, 24, box=big) - ref[:20]).max() <= TOL


# ---------------------------------------------------------------------------------------------------- dense entries
def test_dense_entries_at_another_tolerance(gpu_engine_factory):
    """model_forward_dense and epn_forward on an engine with near_tol = 0.15: featurised molecules, and an arbitrary e whose rows'
    largest entries sit below, exactly at (not near: the flag is a strict >) and above the tolerance."""
    s = ec.EdgeSet(48, 3.0, 2.0, 0.15)
    T, N = 2, 20
    w = random_weights(NX, T, seed=19, scale=0.35)
    mols = [_lattice_molecule(n, NX, seed=n) for n in (20, 13, 7)]
    ec.assert_admissible(mols, s, what="dense entries")
    parts = [orc.dense_inputs(m[0], m[1], m[2], N) for m in mols]
    h, e, x, q, mask = (np.stack([p[k] for p in parts]) for k in range(5))
    ref = orc.model_forward(h, e, x, q, mask, w, np.float64, near_tol=s.near_tol)
    ec.assert_sensitive(ref, orc.model_forward(h, e, x, q, mask, w, np.float64), TOL, "dense entries")
    eng = _engine(gpu_engine_factory, s, w)
    out = eng.model_forward_dense(h, e, x, q, mask)
    print(f"model_forward_dense at near_tol 0.15: worst |dq| {np.abs(out - ref).max():.2e}")
    assert np.abs(out - ref).max() <= TOL
    # arbitrary e: a third of the pairs each with max_k e_k = 0.05 .. 0.14, = float32(0.15), = 0.16 .. 0.3; symmetric like the model's
    rng = np.random.default_rng(5)
    B = 2
    tol32 = np.float32(s.near_tol)
    top = rng.choice(3, size=(B, N, N))
    top = np.triu(top, 1) + np.transpose(np.triu(top, 1), (0, 2, 1))
    peak = np.where(top == 0, rng.uniform(0.05, 0.14, (B, N, N)), np.where(top == 1, tol32, rng.uniform(0.16, 0.3, (B, N, N)))).astype(np.float32)
    peak = np.triu(peak, 1) + np.transpose(np.triu(peak, 1), (0, 2, 1))
    shape = rng.uniform(0.0, 1.0, (B, N, N, 48)).astype(np.float32)
    shape = np.triu(shape.transpose(0, 3, 1, 2), 1).transpose(0, 2, 3, 1)
    shape = shape + shape.transpose(0, 2, 1, 3)
    shape[..., 7] = 1.0
    ea = (shape * peak[..., None]).astype(np.float32)
    ea[..., 7] = peak                                          # (the largest entry is peak itself, bit for bit)
    assert int((ea.max(-1) == tol32).sum()) >= B * N and int((ea.max(-1) > tol32).sum()) >= B * N
    ha = rng.normal(scale=0.3, size=(B, N, 48)).astype(np.float32)
    xa = np.stack([_features(rng, N, NX)[0] for _ in range(B)])
    qa = rng.normal(scale=0.2, size=(B, N, 1)).astype(np.float32)
    ma = np.ones((B, N, N, 1), np.float32)
    ma[1, 15:, :] = 0.0
    ma[1, :, 15:] = 0.0
    ref = orc.epn_layer(ha, ea, xa, qa, ma, w["pas"], np.float64, near_tol=s.near_tol)
    at_tol = orc.epn_layer(ha, ea, xa, qa, ma, w["pas"], np.float64, near_tol=float(np.nextafter(tol32, np.float32(0))))
    ec.assert_sensitive(ref, orc.epn_layer(ha, ea, xa, qa, ma, w["pas"], np.float64), TOL, "epn_forward, arbitrary e")
    ec.assert_sensitive(ref, at_tol, TOL, "epn_forward, the entries at the tolerance")
    out = eng.epn_forward(ha, ea, xa, qa, ma)
    print(f"epn_forward at near_tol 0.15, arbitrary e: worst |dq| {np.abs(out - ref).max():.2e}")
    assert np.abs(out - ref).max() <= TOL


# ---------------------------------------------------------------------------------------------------- gradients
GRAD_OPEN = {"A": (48, 48, 148), "B": (33, 40, 33), "C": (33, 40, 33)}     # (n, N, seed) of the open lattice molecule
GRAD_BOX_SEED = {"A": 42, "B": 40, "C": 40}                                # 40 atoms in BOX
GRAD_CELL_SEED = 42                                                        # 40 atoms in SHEARED


def _deriv_weights(s):
    return random_weights(NX, 2, seed=5, scale=0.6, h_dim=s.h_dim)


@functools.lru_cache(maxsize=None)
def _gradient_case(name, kind):
    """(s, w, molecule, N, geometry keywords, ref_fn(xyz, x, Q, g, **kw) at the set's constants) of a gradient case, admitted on
    the reference alone: margin, flag intervals, and for gxyz (and gstrain in the cell) the kink rule per component and the
    sensitivity against the bound test_gpu_grad_large._check really grants, 2e-4 max |ref| + the largest bracket."""
    s = ec.SETS[name]
    w = _deriv_weights(s)
    if kind == "open":
        n, N, seed = GRAD_OPEN[name]
        mol, cell, geo = _lattice_molecule(n, NX, seed=seed), None, {}
        fn = lambda xyz, x, Q, g, **k: vjp64(xyz, x, Q, g, w, **k)
    elif kind == "box":
        rng = np.random.default_rng(GRAD_BOX_SEED[name])
        mol, N, cell, geo = (periodic_ref.random_cell(rng, 40, BOX),) + _features(rng, 40, NX), 44, np.diag(BOX), {"box": BOX}
        fn = lambda xyz, x, Q, g, **k: vjp64_pbc(xyz, x, Q, g, BOX, w, **k)
    else:
        rng = np.random.default_rng(GRAD_CELL_SEED)
        mol, N, cell, geo = (cell_ref.random_cell(rng, 40, SHEARED),) + _features(rng, 40, NX), 44, SHEARED, {"cell": SHEARED}
        fn = lambda xyz, x, Q, g, **k: strain64(xyz, x, Q, g, SHEARED, w, **k)
    what = f"set {name}, gradients, {kind}"
    ec.assert_admissible([mol], s, [cell], least=5 if name == "C" else 0, what=what)
    g = np.random.default_rng(0).normal(size=mol[0].shape[0]).astype(np.float32).astype(np.float64)    # (_check's cotangent)
    kw = dict(N=N, **ec.ref_kwargs(s))
    at, lo, hi = fn(*mol, g, **kw), fn(*mol, g, kink_shift=+TAU, **kw), fn(*mol, g, kink_shift=-TAU, **kw)
    dflt = fn(*mol, g, N=N, h_dim=s.h_dim)
    for k, part in ((1, "gxyz"), (2, "gstrain"))[:len(at) - 1]:
        whole, _ = ec.assert_derivative_case(at[k], np.abs(lo[k] - hi[k]), dflt[k], f"{what}, {part}")
        assert whole > 100, (what, part, whole)
    kws = dict(cutoff=s.cutoff, eta=s.eta, near_tol=s.near_tol)
    return s, w, mol, N, geo, lambda xyz, x, Q, g, **k: fn(xyz, x, Q, g, **kws, **k)


@pytest.mark.parametrize("kind", ["open", "box", "cell"])
@pytest.mark.parametrize("name", list(ec.SETS))
def test_gradients(gpu_engine_factory, name, kind):
    """charges_vjp_xyz on both paths against vjp64 / vjp64_pbc / vjp64_cell, the two paths within the 4e-4 rule
    (test_gpu_grad_large._check); open molecules on the pair-list path against vjp64_large too."""
    s, w, mol, N, geo, ref_fn = _gradient_case(name, kind)
    eng = _engine(gpu_engine_factory, s, w)
    _check(eng, [mol], N, [lambda *a, **k: ref_fn(*a, **k)[:2]], h_dim=s.h_dim, **geo)
    if kind == "open":
        kws = dict(cutoff=s.cutoff, eta=s.eta, near_tol=s.near_tol)
        _check(eng, [mol], N, [lambda xyz, x, Q, g, **k: vjp64_large(xyz, x, Q, g, w, **kws, **k)], h_dim=s.h_dim, both_paths=False)


@pytest.mark.parametrize("name", list(ec.SETS))
def test_gradient_strain(gpu_engine_factory, name):
    """test_gpu_grad_large.test_cells_and_strain at the set's constants: strain=True on both paths against strain64."""
    s, w, mol, N, geo, ref_fn = _gradient_case(name, "cell")
    n = mol[0].shape[0]
    g = np.random.default_rng(0).normal(size=n).astype(np.float32)
    g64 = g.astype(np.float64)
    off, Qa = np.int32([0, n]), np.float32([mol[2]])
    ref_s = ref_fn(*mol, g64, N=N, h_dim=s.h_dim)[2]
    lo = ref_fn(*mol, g64, N=N, h_dim=s.h_dim, kink_shift=+TAU)[2]
    hi = ref_fn(*mol, g64, N=N, h_dim=s.h_dim, kink_shift=-TAU)[2]
    scale, kink = np.abs(ref_s).max(), np.abs(lo - hi).max()
    eng = _engine(gpu_engine_factory, s, w)
    gs = {}
    for path in (2, 1):
        eng.set_option("grad_path", path)
        gs[path] = eng.charges_vjp_xyz(off, mol[0], mol[1], Qa, g, N, strain=True, **geo)[2][0]
        err = np.abs(gs[path] - ref_s).max()
        print(f"set {name}, grad_path {path}: gstrain {err:.3e} of {scale:.3e}, kink {kink:.3e}")
        assert err <= 2e-4 * scale + kink
    assert np.abs(gs[2] - gs[1]).max() <= 4e-4 * scale + kink


# ---------------------------------------------------------------------------------------------------- the Coulomb call
COULOMB_ALPHA = 0.3


@functools.lru_cache(maxsize=None)
def _coulomb_case(name):
    """(s, w, molecule, N, q, phi, fq, kink per component) of the Coulomb call on the open molecule of the gradient tests, the
    reference (coulomb_forces64) at the set's constants and h_dim; admitted on the reference alone: margin and flag intervals, the kink
    rule per component for fq = -vjp64(g = phi), and its sensitivity to the constants over the components inside the bracket (the
    comparison's bound is per component)."""
    from coulomb_ref import coulomb_forces64
    from test_gpu_coulomb import KE
    s = ec.SETS[name]
    w = _deriv_weights(s)
    n, N, seed = GRAD_OPEN[name]
    mol = _lattice_molecule(n, NX, seed=seed)
    what = f"set {name}, coulomb ({n}, {N})"
    ec.assert_admissible([mol], s, least=5 if name == "C" else 0, what=what)
    kw = ec.ref_kwargs(s)
    q, phi, E, f, ffix, fq = coulomb_forces64(*mol, w, N, KE, COULOMB_ALPHA, **kw)
    lo = coulomb_forces64(*mol, w, N, KE, COULOMB_ALPHA, kink_shift=+TAU, **kw)[5]
    hi = coulomb_forces64(*mol, w, N, KE, COULOMB_ALPHA, kink_shift=-TAU, **kw)[5]
    dflt = coulomb_forces64(*mol, w, N, KE, COULOMB_ALPHA, h_dim=s.h_dim)
    kink = np.abs(lo - hi)
    ec.assert_sensitive(q, dflt[0], 2e-4, f"{what}, q")
    _, inside = ec.assert_derivative_case(fq, kink, dflt[5], f"{what}, fq")
    assert inside > 100, (what, inside)
    return s, w, mol, N, q, phi, fq, kink


@pytest.mark.parametrize("name", list(ec.SETS))
def test_coulomb(gpu_engine_factory, name):
    """coulomb_xyz at alpha = 0.3 at the set's constants: phi, ffix and E against coulomb64 on the device charges at test_gpu_coulomb's
    BOUND, the bits of charges_vjp_xyz(g=phi) on the pair-list path, q within 2e-4 of the reference and fq per component."""
    from test_gpu_coulomb import _check_call
    s, w, mol, N, q_ref, phi_ref, fq_ref, kink = _coulomb_case(name)
    eng = _engine(gpu_engine_factory, s, w, grad_path=2)
    q, phi, E, F, ffix, fq = _check_call(eng, mol, N, COULOMB_ALPHA, f"set {name} coulomb")
    scale, err = np.abs(fq_ref).max(), np.abs(fq - fq_ref)
    print(f"set {name}: q {np.abs(q - q_ref).max():.3e}, phi {np.abs(phi - phi_ref).max():.3e} of {np.abs(phi_ref).max():.3e}; fq max error "
          f"{err.max():.3e} of {scale:.3e}, worst excess over the component's bound {(err - 2e-4 * scale - kink).max():.3e}")
    assert np.abs(q - q_ref).max() <= 2e-4
    assert scale > 0 and (err <= 2e-4 * scale + kink).all(), (np.argmax(err - kink), err.max(), scale)


# ---------------------------------------------------------------------------------------------------- forward mode
@functools.lru_cache(maxsize=None)
def _jvp_case(name, n, N, which):
    """(s, w, molecule, tangents, q, tq, kink per atom) of a lattice molecule: which = "v" or "all" (v, strain and dQ together)."""
    s = ec.SETS[name]
    w = _deriv_weights(s)
    mol = _lattice_molecule(n, NX, seed=n)
    rng = np.random.default_rng(100 + n)
    tan = {"v": rng.normal(size=(n, 3)).astype(np.float32), "strain": None, "dQ": None}
    if which == "all":
        tan["strain"] = (0.3 * rng.normal(size=(3, 3))).astype(np.float32)
        tan["dQ"] = np.float32(rng.normal())
    ec.assert_admissible([mol], s, least=5 if name == "C" else 0, what=f"set {name}, forward mode ({n}, {N}) {which}")
    kw = dict(N=N, v=tan["v"], strain=tan["strain"], dQ=None if tan["dQ"] is None else float(tan["dQ"]))
    q, tq = jvp_ref.jvp64(*mol, w, **kw, **ec.ref_kwargs(s))
    lo = jvp_ref.jvp64(*mol, w, kink_shift=+TAU, **kw, **ec.ref_kwargs(s))[1]
    hi = jvp_ref.jvp64(*mol, w, kink_shift=-TAU, **kw, **ec.ref_kwargs(s))[1]
    kink = np.abs(lo - hi)
    # the bound is per atom: the sensitivity is asked of the atoms inside the bracket, whose bound is at most 4e-4 max |ref|
    _, inside = ec.assert_derivative_case(tq, kink, jvp_ref.jvp64(*mol, w, h_dim=s.h_dim, **kw)[1], f"set {name} ({n}, {N}) {which}")
    assert inside > 100, (name, n, N, which, inside)
    return s, w, mol, tan, q, tq, kink


JVP_CASES = [(nm,) + DERIV[nm] + (which,) for nm in ec.SETS for which in ("v", "all")] + [("C", 17, 24, "v")]


@pytest.mark.parametrize("name,n,N,which", JVP_CASES)
def test_forward_mode_against_the_float64_reference(gpu_engine_factory, name, n, N, which):
    s, w, mol, tan, q_ref, ref, kink = _jvp_case(name, n, N, which)
    off, xyz, x, Q = _batch([mol])
    eng = _engine(gpu_engine_factory, s, w, grad_path=2)
    q, tq = eng.charges_jvp_xyz(off, xyz, x, Q, N, **tan)
    scale, err = np.abs(ref).max(), np.abs(tq - ref)
    print(f"q vs reference {np.abs(q - q_ref).max():.3e}; tq max error {err.max():.3e} of {scale:.3e}, worst excess over the bound "
          f"{(err - 2e-4 * scale - kink).max():.3e}")
    assert np.abs(q - q_ref).max() <= 2e-4
    assert (err <= 2e-4 * scale + kink).all(), (np.argmax(err - kink), err.max(), scale)


@pytest.mark.parametrize("name", list(ec.SETS))
def test_forward_mode_multi_and_adjoint(gpu_engine_factory, name):
    """charges_jvp_xyz_multi at K = 5 (v, strain, dQ, all three, twice v): every row carries the bits of the single call, the row of
    all three is within the bound of jvp64; the adjoint identity against charges_vjp_xyz(strain=True) on the same engine."""
    n, N = DERIV[name]
    s, w, mol, tan, q_ref, ref, kink = _jvp_case(name, n, N, "all")
    off, xyz, x, Q = _batch([mol])
    eng = _engine(gpu_engine_factory, s, w, grad_path=2)
    v, E, t = tan["v"], tan["strain"], np.float32([tan["dQ"]])
    zv, zE, zt = np.zeros_like(v), np.zeros_like(E), np.zeros_like(t)
    rows = [(v, zE, zt), (zv, E, zt), (zv, zE, t), (v, E, t), (2 * v, zE, zt)]
    q, tq = eng.charges_jvp_xyz_multi(off, xyz, x, Q, N, v=np.stack([r[0] for r in rows]), strain=np.stack([r[1] for r in rows]),
                                      dQ=np.stack([r[2] for r in rows]))
    for k, (rv, rE, rt) in enumerate(rows):
        q1, t1 = eng.charges_jvp_xyz(off, xyz, x, Q, N, v=rv, strain=rE, dQ=rt)
        assert np.array_equal(q1, q) and np.array_equal(t1, tq[k]), k
        assert np.abs(t1).max() > 0
    scale, err = np.abs(ref).max(), np.abs(tq[3] - ref)
    print(f"set {name}: multi row of all three, max error {err.max():.3e} of {scale:.3e}, worst excess {(err - 2e-4 * scale - kink).max():.3e}")
    assert (err <= 2e-4 * scale + kink).all()
    _adjoint(eng, off, xyz, x, Q, N, {}, {"v": v, "strain": E[None]}, seed=41)


# ---------------------------------------------------------------------------------------------------- training
TRAIN_CELL = np.diag(np.float32([7.0, 7.2, 7.5]))


def _train_oracle(D, w, s):
    """(loss, predictions (B, N), flat gradient, flat float32-oracle gradient, flat kink band): test_gpu_train_cell._oracle with near_tol."""
    loss, pred, g = ot.loss_and_grads(*D, w, near_tol=s.near_tol)
    gr = ot.flatten(g)
    g32 = ot.flatten(ot.loss_and_grads(*D, w, dtype=np.float32, near_tol=s.near_tol)[2]).astype(np.float64)
    band = np.zeros_like(gr)
    for where in ("gnn", "listed", "swapped"):
        lo = ot.flatten(ot.loss_and_grads(*D, w, kink_shift=+TAU_TRAIN, kink_where=where, near_tol=s.near_tol)[2])
        hi = ot.flatten(ot.loss_and_grads(*D, w, kink_shift=-TAU_TRAIN, kink_where=where, near_tol=s.near_tol)[2])
        band += np.abs(hi - lo)
    return loss, pred[:, :, 0], gr, g32, band


@functools.lru_cache(maxsize=None)
def _train_case(name):
    """One open 13-atom molecule and 24 atoms in a 7.0 x 7.2 x 7.5 cell at N = 24: the dense inputs, the oracle (gradient, float32
    noise, kink band) and the pair-list reference, all at the set's constants."""
    from test_gpu_train_cell import _system
    s = ec.SETS[name]
    w = random_weights(NX, 2, seed=13, scale=0.4, h_dim=s.h_dim)
    N = 24
    cells = [ZERO, TRAIN_CELL]
    mols = [_system(13, NX, ZERO, seed=28), _system(24, NX, TRAIN_CELL, seed=170)]
    ec.assert_admissible(mols, s, cells, least=5 if name == "C" else 0, what=f"set {name}, training")

    def dense(c):
        parts, yd = [], np.zeros((len(mols), N, 1))
        for b, ((xyz, x, Q, y), cell) in enumerate(zip(mols, cells)):
            d = list(orc.dense_inputs(xyz, x, Q, N, h_dim=c.h_dim, e_dim=c.h_dim, cutoff=c.cutoff, eta=c.eta))
            d[1][:len(x), :len(x)] = cell_ref.get_init_edges_cell(xyz, cell, num=c.h_dim, cutoff=c.cutoff, eta=c.eta)[0]
            parts.append(d)
            yd[b, :len(x), 0] = y
        return [np.stack([p[k] for p in parts]) for k in range(5)] + [yd]

    D = dense(s)
    oracle = _train_oracle(D, w, s)
    gr = oracle[2]
    g_dflt = ot.flatten(ot.loss_and_grads(*dense(ec.EdgeSet(s.h_dim, 3.0, 2.0, 1e-5)), w)[2])
    ec.assert_sensitive(gr, g_dflt, 2e-4 * np.abs(gr).max(), f"set {name}, training gradient")
    off, xyz, x, Q = _batch(mols)
    y = np.concatenate([m[3] for m in mols]).astype(np.float32)
    large = batch_loss_and_grads_large(off, xyz, x, Q, y, w, N, cells=cells, **ec.ref_kwargs(s))
    return s, w, mols, np.stack(cells), N, D, oracle, large, _train_oracle([a[:1] for a in D], w, s)


def _check_step(eng, w, off, q, loss, oracle, what):
    loss_ref, pred_ref, gr, g32, band = oracle
    for b in range(len(off) - 1):
        assert np.abs(q[b] - pred_ref[b, :len(q[b])]).max() <= 2e-5, (what, b)
    assert abs(loss - loss_ref) <= 2e-5 * max(1.0, abs(loss_ref)), (what, loss, loss_ref)
    _check_gradient(eng.get_gradients(), w, gr, g32, band, what)
    assert np.array_equal(ot.flatten(eng.get_weights()), ot.flatten(w).astype(np.float32))          # apply=False: weights untouched


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("name", list(ec.SETS))
def test_train_step_dense(gpu_engine_factory, name, fused):
    s, w, mols, cells, N, D, oracle, large, alone = _train_case(name)
    eng = _engine(gpu_engine_factory, s, w, train_fused=fused)
    eng.train_init()
    pred, loss = eng.train_step_dense(*D, apply=False)
    off = _batch(mols)[0]
    _check_step(eng, w, off, [pred[b, :len(m[0]), 0] for b, m in enumerate(mols)], loss, oracle, f"set {name}, dense step, train_fused={fused}")


@pytest.mark.parametrize("path", [1, 2])
@pytest.mark.parametrize("name", list(ec.SETS))
def test_train_step_xyz(gpu_engine_factory, name, path):
    """train_step_xyz through the cell entry on both paths (the open molecule as the all-zero cell) against the dense oracle; the
    pair-list path against the pair-list reference too; and the open molecule alone through the entry without a cell."""
    s, w, mols, cells, N, D, oracle, large, alone = _train_case(name)
    off, xyz, x, Q = _batch(mols)
    y = np.concatenate([m[3] for m in mols]).astype(np.float32)
    eng = _engine(gpu_engine_factory, s, w, train_path=path)
    eng.train_init()
    q, loss = eng.train_step_xyz(off, xyz, x, Q, y, N, apply=False, cell=cells)
    what = f"set {name}, train_path={path}"
    _check_step(eng, w, off, [q[off[b]:off[b + 1]] for b in range(len(mols))], loss, oracle, what)
    if path == 2:
        _check_gradient(eng.get_gradients(), w, large[2], oracle[3] - oracle[2] + large[2], oracle[4], what + " vs the pair-list reference")
    # the open molecule alone: through the cell entry as the all-zero cell, and through epnn_train_step_xyz without a cell
    n0 = int(off[1])
    for geo in ({"cell": ZERO}, {}):
        q, loss = eng.train_step_xyz(off[:2], xyz[:n0], x[:n0], Q[:1], y[:n0], N, apply=False, **geo)
        _check_step(eng, w, off[:2], [q], loss, alone, what + (", alone as the all-zero cell" if geo else ", alone without a cell"))
