"""Electrostatics of the predicted charges in fully periodic cells (epnn_coulomb_xyz_cell, Engine.coulomb_xyz_cell) on the GPU: the
fixed-charge parts against the float64 Ewald sum on the device's own charges at the parameters the call ran at, the composition
with the pair-list gradient call bit for bit, the totals against the full float64 reference, images, invariants and refusals.
GPU only.

Measured worst shares of the bounds below (MI355X, the 40 cases of test 1 and the 20 pairs of test 4): phi 0.031 (the lone atom of
the batch, beta == alpha), ffix 0.012 (a pair across a face), E 0.007, the fixed-charge strain 0.020; from 17 atoms on all four are
at most 0.010, from 30 atoms on at most 0.008.  The bounds count worst-case roundings per term; the errors of a sum's terms do not add up in phase."""
import math

import numpy as np
import pytest

import cell_ref
from conftest import random_weights
from ewald_ref import ewald64, ewald_forces64
from test_gpu_grad_large import TAU, _features

pytestmark = pytest.mark.gpu

KE = 14.3996454784255
U = 2.0 ** -24
BOUND = 2e-6          # real-space terms: the open call's bound (about ten float32 roundings per term, a few ulp of erff / erfcf / expf)
# Reciprocal terms, counted in the kernels as written, in units of 2^-24 of a term's scale c(k) |q_j| (k_ew_sfac) or c(k) |S| (k_ew_atom):
#   the phase 2 pi frac(m . s): frac rounded to float32 (|frac| <= 1/2: pi), the float32 2 pi (1.5) and the product (|angle| <= pi: pi)   7.8
#   sincosf, 2 ulp of a value below 1                                                                                                      2
#   k_ew_sfac: q_j times the cosine or sine                                                                                                1    -> S: 10.8
#   k_ew_atom: the same phase and sincosf (9.8) and S rounded to float32 (1), two products and a sum on cos Sx + sin Sy
#              (3), all on |cos Sx| + |sin Sy| <= sqrt(2) |S|: 13.8 * 1.41 = 19.5; c(k) in float32 and its product (2); for ffix the
#              float32 k and its product (2)                                                                                              23.5
# together 34; E and the strain take S alone (|S|^2: twice 10.8).  The sums over j and k are float64.
BOUND_REC = 34 * U
REST = 2 * U          # the self and background terms are float64: the rounding of the float32 output
ALPHAS = [0.0, 0.5, 2.0]          # at tol = 1e-6 the rule gives beta == alpha for 0.5 in every cell here (no sweep) and beta < alpha for 2.0

CELLS = {"cube8": np.diag(np.float32([8, 8, 8])), "sheared": np.float32([[7, 0, 0], [1.5, 6.5, 0], [-1, 2, 8]]),
         "slab": np.diag(np.float32([6, 6, 20])), "cube14": np.diag(np.float32([14, 14, 14]))}
# (cell, n, N): every boundary of the packing (epnn_coulomb.hip.h: CL_BLOCK 64, CL_MINPIECE 128), the larger sizes in the larger cell
SINGLE = [("cube8", 1, 8), ("cube8", 2, 8), ("sheared", 17, 24), ("cube8", 63, 64), ("sheared", 64, 64), ("slab", 65, 72),
          ("cube14", 128, 128), ("cube14", 129, 136), ("cube14", 257, 264)]
CASES = [f"{c}-{n}-{N}" for c, n, N in SINGLE] + ["batch"]
BATCH = [("cube8", 20), ("sheared", 1), ("slab", 9), ("cube14", 30)]             # 60 atoms: one wavefront of the sweep


def _weights():
    return random_weights(9, 2, seed=5, scale=0.6)


def _system(cell_name, n, seed):
    rng = np.random.default_rng(seed)
    xyz = cell_ref.random_cell(rng, n, CELLS[cell_name])
    x, Q = _features(rng, n, 9)
    return xyz, x, (np.float32(1.0) if n == 1 else Q), CELLS[cell_name]


def _batch(systems):
    offsets = np.zeros(len(systems) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([s[0].shape[0] for s in systems])
    return (offsets, np.concatenate([s[0] for s in systems]), np.concatenate([s[1] for s in systems]),
            np.array([s[2] for s in systems], dtype=np.float32)), np.stack([s[3] for s in systems])


_CASES, _ENGINE, _RUNS = {}, [], {}


def _case(name):
    """(systems, N)"""
    if name not in _CASES:
        if name == "batch":
            _CASES[name] = ([_system(c, n, 700 + n) for c, n in BATCH], 32)
        else:
            c, n, N = name.split("-")
            _CASES[name] = ([_system(c, int(n), int(n))], int(N))
    return _CASES[name]


def _engine(factory):
    if not _ENGINE:
        eng = factory(nx=9, T=2)
        eng.set_weights(_weights())
        eng.set_option("grad_path", 2)
        _ENGINE.append(eng)
    return _ENGINE[0]


def _rows(eng, cells, alpha, tol=1e-6, beta=None):
    """The parameters of every cell: the rule's, or (beta given) rc = w_min / 2 and kc, M by the rule's formulas at that beta."""
    rows = np.stack([eng.ewald_params(c, alpha, tol) for c in cells])
    if beta is not None:
        s = math.sqrt(-math.log(tol))
        for b, c in enumerate(cells):
            a = c.astype(np.float64)
            kc = 2 * beta * s
            rows[b] = [beta, 0.5 * cell_ref.widths(c).min() * (1 - 1e-12), kc, *np.ceil(kc * np.sqrt((a * a).sum(1)) / (2 * math.pi))]
    return rows


PSETS = {"a0": (0.0, None), "a05": (0.5, None), "a2": (2.0, None), "near": (0.5, 0.45)}      # near: a sweep whose two erf almost cancel


def _run(factory, name, pset):
    """The call with parts and strain, once per case: (engine, batch, cells, N, alpha, rows, (q, phi, E, F, gs, ffix, fq, gs_fix, gs_q))."""
    if (name, pset) not in _RUNS:
        systems, N = _case(name)
        eng = _engine(factory)
        batch, cells = _batch(systems)
        alpha, beta = PSETS[pset]
        rows = _rows(eng, cells, alpha, beta=beta)
        if pset == "a05":
            assert (rows[:, 1] == 0).all() and (rows[:, 0] == 0.5).all()
        else:
            assert (rows[:, 1] > 0).all() and (alpha == 0 or (rows[:, 0] < alpha).all())
        out = eng.coulomb_xyz_cell(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, parts=True, strain=True)
        _RUNS[name, pset] = (eng, batch, cells, N, alpha, rows, out)
    return _RUNS[name, pset]


def _bound(s, k=1.0):
    return k * (BOUND * s["real"] + BOUND_REC * s["rec"] + REST * s["rest"])


# ---------------------------------------------------------------------------------------------------- 1: the fixed-charge parts
def _check_fixed_parts(what, alpha, row, xyz, cell, q, phi, Eb, ffix, gs_fix):
    """One cell's phi, ffix, E and fixed-charge strain against ewald64 on its device charges at the row's parameters: each within
    BOUND of its absolute real-space terms plus BOUND_REC of its absolute reciprocal terms.  Returns the errors as shares of that."""
    e = ewald64(xyz, q, cell, KE, alpha, row[0], row[1], row[2], row[3:])
    bp, bf, bE, bs = _bound(e.s_phi), _bound(e.s_ffix), _bound(e.s_E), _bound(e.s_strain)
    ep, ef, eE, es = np.abs(phi - e.phi), np.abs(ffix - e.ffix).max(1), abs(Eb - e.E), np.abs(gs_fix - e.strain)
    with np.errstate(divide="ignore", invalid="ignore"):                      # (an atom of charge 0 has no force terms at all)
        shares = ((ep / bp).max(), np.where(bf > 0, ef / bf, 0.0).max(), eE / bE, (es / bs).max())
    print(f"{what} (n = {len(q)}): phi {shares[0]:.3f}, ffix {shares[1]:.3f}, E {shares[2]:.3f}, strain {shares[3]:.3f} of the bounds "
          f"(|phi| {np.abs(e.phi).max():.3e}, |ffix| {np.abs(e.ffix).max():.3e}, E {e.E:.6e}, |strain| {np.abs(e.strain).max():.3e})")
    assert np.abs(e.phi).max() > 0
    assert (ep <= bp).all() and (ef <= bf).all() and eE <= bE and (es <= bs).all()
    return shares, e


@pytest.mark.parametrize("pset", sorted(PSETS))
@pytest.mark.parametrize("name", CASES)
def test_fixed_charge_parts_against_float64_on_the_device_charges(gpu_engine_factory, name, pset):
    eng, (offsets, xyz, x, Q), cells, N, alpha, rows, (q, phi, E, F, gs, ffix, fq, gs_fix, gs_q) = _run(gpu_engine_factory, name, pset)
    assert E.dtype == np.float64 and E.shape == (len(offsets) - 1,) and gs.shape == (len(offsets) - 1, 3, 3)
    for b in range(len(offsets) - 1):
        a0, a1 = offsets[b], offsets[b + 1]
        _check_fixed_parts(f"{name} {pset}, cell {b}", alpha, rows[b], xyz[a0:a1], cells[b], q[a0:a1], phi[a0:a1], E[b], ffix[a0:a1], gs_fix[b])
        assert np.array_equal(gs_fix[b], gs_fix[b].T)


def test_one_charge_gives_the_wigner_constant(gpu_engine_factory):
    """One atom with Q = 1 in the 8 A cube, alpha = 0: phi = -2.8372974795 ke / L, E half of it, within the device bound and the
    truncation at tol = 1e-6 (tol ke beta |q|, include/epnn.h)."""
    eng, (offsets, xyz, x, Q), cells, N, alpha, rows, (q, phi, E, F, gs, ffix, fq, gs_fix, gs_q) = _run(gpu_engine_factory, "cube8-1-8", "a0")
    assert q[0] == 1.0 and Q[0] == 1.0
    e = ewald64(xyz, q, cells[0], KE, 0.0, rows[0][0], rows[0][1], rows[0][2], rows[0][3:])
    slack = _bound(e.s_phi)[0] + 1e-6 * KE * rows[0][0]
    assert abs(phi[0] + 2.8372974795 * KE / 8.0) <= slack and abs(E[0] + 0.5 * 2.8372974795 * KE / 8.0) <= slack
    assert np.abs(ffix).max() <= _bound(e.s_ffix)[0] and not fq.any()
    # dE/d eps of E = -w ke / (2 L): E / 3 on the diagonal (the charge has no dq/d eps: q == Q)
    assert np.abs(gs[0] - np.eye(3) * (-E[0] / 3.0)).max() <= _bound(e.s_strain).max() + 1e-6 * KE * rows[0][0] and not gs_q.any()


# ---------------------------------------------------------------------------------------------------- 2: composition bits
@pytest.mark.parametrize("pset", sorted(PSETS))
@pytest.mark.parametrize("name", CASES)
def test_composition_with_the_gradient_call_bit_for_bit(gpu_engine_factory, name, pset):
    eng, batch, cells, N, alpha, rows, (q, phi, E, F, gs, ffix, fq, gs_fix, gs_q) = _run(gpu_engine_factory, name, pset)
    q2, gxyz, gstr = eng.charges_vjp_xyz(*batch, phi, N, cell=cells, strain=True)
    assert np.array_equal(q2, q) and np.array_equal(fq, -gxyz) and np.array_equal(gs_q, gstr)
    assert np.array_equal(F, ffix + fq) and F.dtype == np.float32
    assert np.array_equal(gs, gs_fix + gs_q) and gs.dtype == np.float32
    four = eng.coulomb_xyz_cell(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows)
    five = eng.coulomb_xyz_cell(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, strain=True)
    six = eng.coulomb_xyz_cell(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, parts=True)
    assert len(four) == 4 and len(five) == 5 and len(six) == 6
    for got, want in zip(four + five + six, (q, phi, E, F) + (q, phi, E, F, gs) + (q, phi, E, F, ffix, fq)):
        assert np.array_equal(got, want)


def test_default_parameters_are_the_rules_and_a_box_is_its_diagonal_cell(gpu_engine_factory):
    eng, batch, cells, N, alpha, rows, out = _run(gpu_engine_factory, "cube8-63-64", "a0")
    again = eng.coulomb_xyz_cell(*batch, N, box=np.float32([8, 8, 8]), ke=KE, parts=True, strain=True)
    assert all(np.array_equal(a, b) for a, b in zip(again, out))
    assert np.array_equal(eng.ewald_params(cells[0], 0.0, 1e-6), rows[0])


def test_the_model_method(gpu_engine_factory):
    from epnn_amd import charge_gn
    eng, batch, cells, N, alpha, rows, out = _run(gpu_engine_factory, "sheared-17-24", "a2")
    model = charge_gn.make_model([32, 32], 48, 2, 9, 24)
    model.set_weights_dict(_weights())
    got = model.coulomb_xyz_cell(*batch, cell=cells[0], ke=KE, alpha=2.0, parts=True, strain=True)
    assert len(got) == 9 and all(np.array_equal(a, b) for a, b in zip(got, out))


# ---------------------------------------------------------------------------------------------------- 3: end to end
_REF = {}


def _reference(cell_name, n, N, alpha, row):
    key = (cell_name, n, N, alpha)
    if key not in _REF:
        xyz, x, Q, cell = _system(cell_name, n, n)
        w = _weights()
        mid = ewald_forces64(xyz, x, Q, cell, w, N, KE, alpha, row)
        lo = ewald_forces64(xyz, x, Q, cell, w, N, KE, alpha, row, kink_shift=+TAU)
        hi = ewald_forces64(xyz, x, Q, cell, w, N, KE, alpha, row, kink_shift=-TAU)
        _REF[key] = mid + (np.abs(lo[3] - hi[3]).max(), np.abs(lo[4] - hi[4]).max())
    return _REF[key]


@pytest.mark.parametrize("name,pset", [("sheared-17-24", "a0"), ("sheared-17-24", "a05"), ("sheared-17-24", "a2"), ("slab-65-72", "a0"),
                                       ("slab-65-72", "a2")])
def test_total_forces_and_strain_against_the_float64_reference(gpu_engine_factory, name, pset):
    """F and gstrain against ewald_forces64 (charges, Ewald sum and the charges' part all float64), the project's standing rule on
    either part's scale: |F - F_ref| <= 2e-4 max(max |ffix_ref|, max |fq_ref|) + kink, kink = max |ref(+TAU) - ref(-TAU)|, and the same
    for the strain; the bracket may be used only while it is at most 0.05 of that scale, asserted on the reference alone."""
    eng, batch, cells, N, alpha, rows, (q, phi, E, F, gs, ffix, fq, gs_fix, gs_q) = _run(gpu_engine_factory, name, pset)
    c, n, _ = name.split("-")
    q64, phi64, E64, f64, gs64, ffix64, fq64, gsf64, gsq64, kink_f, kink_s = _reference(c, int(n), N, alpha, rows[0])
    sf, ss = max(np.abs(ffix64).max(), np.abs(fq64).max()), max(np.abs(gsf64).max(), np.abs(gsq64).max())
    ef, es = np.abs(F - f64).max(), np.abs(gs[0] - gs64).max()
    print(f"{name} {pset}: q {np.abs(q - q64).max():.3e}, phi {np.abs(phi - phi64).max():.3e} of {np.abs(phi64).max():.3e}, E {abs(E[0] - E64):.3e} "
          f"of {abs(E64):.3e}; F {ef:.3e} of {sf:.3e} (|fq| {np.abs(fq64).max():.3e}, kink {kink_f:.3e}); gstrain {es:.3e} of {ss:.3e} "
          f"(|gs_q| {np.abs(gsq64).max():.3e}, kink {kink_s:.3e})")
    assert sf > 0 and ss > 0 and kink_f <= 0.05 * sf and kink_s <= 0.05 * ss
    assert np.abs(q - q64).max() <= 2e-4
    assert ef <= 2e-4 * sf + kink_f and es <= 2e-4 * ss + kink_s


# ---------------------------------------------------------------------------------------------------- 4: images
def _pair(cell, fa, fb, Qtot):
    """Two atoms at fractional fa, fb on a 2^-10 A grid (a lattice shift of such a position is exact in float32)."""
    xyz = np.round(np.float64([fa, fb]) @ cell.astype(np.float64) * 1024) / 1024
    x = np.zeros((2, 9), dtype=np.float32)
    x[0, 1] = x[1, 3] = 1.0
    x[:, 0] = [1, 8]
    return xyz.astype(np.float32), x, np.float32(Qtot)


IMAGES = [(0.07, 0.5, 0.5, 0.93, 0.5, 0.5), (0.5, 0.07, 0.5, 0.5, 0.93, 0.5), (0.5, 0.5, 0.06, 0.5, 0.5, 0.94), (0.07, 0.07, 0.5, 0.93, 0.93, 0.5),
          (0.06, 0.5, 0.94, 0.94, 0.5, 0.06)]


@pytest.mark.parametrize("alpha", [0.0, 2.0])
@pytest.mark.parametrize("k", range(len(IMAGES)))
def test_pairs_nearest_through_an_image(gpu_engine_factory, k, alpha):
    """Two atoms of the sheared cell whose nearest image lies across a face (each axis in turn), across an edge and along the shear:
    that image's term is the dominant one, which a bound scaled by a sum over many pairs would not see.  Then one atom is moved out
    of the cell by (3, -2, 5) lattice vectors: phi and ffix stay those of the wrapped pair, within the bound."""
    eng = _engine(gpu_engine_factory)
    cell = CELLS["sheared"]
    f = IMAGES[k]
    xyz, x, Q = _pair(cell, f[:3], f[3:], 1.0)
    d = cell_ref.mic(xyz[1].astype(np.float64) - xyz[0].astype(np.float64), cell)
    D = math.sqrt((d * d).sum())
    assert 0.9 <= D <= 1.7 and np.abs(np.rint(cell_ref.duals(cell)[1] @ (xyz[1] - xyz[0]).astype(np.float64))).sum() >= 1
    row = _rows(eng, cell[None], alpha)
    off = np.int32([0, 2])
    moved = xyz.copy()
    moved[1] += (np.float64([3, -2, 5]) @ cell.astype(np.float64)).astype(np.float32)
    assert np.array_equal(moved[1].astype(np.float64) - xyz[1], np.float64([3, -2, 5]) @ cell.astype(np.float64))
    outs = [eng.coulomb_xyz_cell(off, r, x, np.float32([Q]), 8, cell=cell, ke=KE, alpha=alpha, ewald=row, parts=True, strain=True) for r in (xyz, moved)]
    for what, (q, phi, E, F, gs, ffix, fq, gs_fix, gs_q) in zip(("wrapped", "moved"), outs):
        _check_fixed_parts(f"pair {k} {what}, alpha {alpha}, D {D:.3f}", alpha, row[0], xyz, cell, q, phi, E[0], ffix, gs_fix[0])
    assert np.abs(outs[0][0] - outs[1][0]).max() <= 2e-6


# ---------------------------------------------------------------------------------------------------- 5: invariants
@pytest.mark.parametrize("pset", ["a0", "a2"])
def test_invariants(gpu_engine_factory, pset):
    eng, batch, cells, N, alpha, rows, out = _run(gpu_engine_factory, "batch", pset)
    offsets, xyz, x, Q = batch
    q, phi, E, F, gs, ffix, fq, gs_fix, gs_q = out
    again = eng.coulomb_xyz_cell(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, parts=True, strain=True)
    assert all(np.array_equal(a, b) for a, b in zip(out, again))
    rows8 = _rows(eng, cells, alpha, tol=1e-8)
    fine = eng.coulomb_xyz_cell(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows8, parts=True, strain=True)
    shift = np.float32([0.37, -1.21, 2.05])
    moved = eng.coulomb_xyz_cell(offsets, xyz + shift, x, Q, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, parts=True, strain=True)
    for b in range(len(offsets) - 1):
        a0, a1 = offsets[b], offsets[b + 1]
        e = ewald64(xyz[a0:a1], q[a0:a1], cells[b], KE, alpha, rows[b][0], rows[b][1], rows[b][2], rows[b][3:])
        bf = _bound(e.s_ffix)
        # sum_i ffix_i = 0 to the bound on the cell's summed absolute terms; the total force with fq, a float32 backward (sums of
        # some hundred float32 terms: 1e-5 of their size, as test_gpu_coulomb.py takes it)
        assert np.abs(ffix[a0:a1].sum(0, dtype=np.float64)).max() <= bf.sum()
        assert np.abs(F[a0:a1].sum(0, dtype=np.float64)).max() <= bf.sum() + 1e-5 * np.abs(fq[a0:a1]).sum()
        # a translation by no lattice vector: E changes by the float32 rounding of the moved coordinates (2^-24 of up to 32 A each)
        # times the forces, and by the bound on E of either run
        assert abs(moved[2][b] - E[b]) <= 32 * U * np.abs(F[a0:a1]).sum() + 2 * _bound(e.s_E)
        # tol = 1e-6 against tol = 1e-8: the truncation scales of include/epnn.h at 1e-6, and the bounds of the two runs
        beta, Qa, qm = rows[b][0], np.abs(q[a0:a1]).sum(), np.abs(q[a0:a1]).max()
        assert np.abs(fine[0][a0:a1] - q[a0:a1]).max() == 0
        assert np.abs(fine[1][a0:a1] - phi[a0:a1]).max() <= 1e-6 * KE * beta * Qa + 2 * _bound(e.s_phi).max()
        assert abs(fine[2][b] - E[b]) <= 1e-6 * 0.5 * KE * beta * Qa * Qa + 2 * _bound(e.s_E)
        assert np.abs(fine[5][a0:a1] - ffix[a0:a1]).max() <= 1e-6 * KE * beta * beta * Qa * qm + 2 * bf.max()
        # alone at the same N: the same bits
        alone = eng.coulomb_xyz_cell(np.int32([0, a1 - a0]), xyz[a0:a1], x[a0:a1], Q[b:b + 1], N, cell=cells[b], ke=KE, alpha=alpha, ewald=rows[b],
                                     parts=True, strain=True)
        want = (q[a0:a1], phi[a0:a1], E[b:b + 1], F[a0:a1], gs[b:b + 1], ffix[a0:a1], fq[a0:a1], gs_fix[b:b + 1], gs_q[b:b + 1])
        for k, (got, w) in enumerate(zip(alone, want)):
            assert np.array_equal(got, w), (b, k)


# ---------------------------------------------------------------------------------------------------- 6: refusals
def test_refusals_leave_the_handle_usable(gpu_engine_factory):
    from epnn_amd._lib import EpnnError
    eng, batch, cells, N, alpha, rows, first = _run(gpu_engine_factory, "batch", "a0")
    offsets, xyz, x, Q = batch

    def call(**kw):
        args = dict(cell=cells, ke=KE, alpha=0.0, ewald=rows, parts=True, strain=True)
        args.update(kw)
        return eng.coulomb_xyz_cell(*batch, N, **args)

    def still_fine():
        assert all(np.array_equal(a, b) for a, b in zip(call(), first))

    open_z = cells.copy()
    open_z[2, 2] = 0
    for kw, match in (({"cell": open_z}, "open"), ({"cell": open_z, "ewald": None}, "open"),
                      ({"alpha": -1.0}, "alpha must be finite"), ({"alpha": float("nan")}, "alpha must be finite"),
                      ({"alpha": float("inf")}, "alpha must be finite"), ({"ke": float("inf")}, "ke must be finite"),
                      ({"ke": float("nan")}, "ke must be finite"), ({"ewald": None, "tol": float("nan")}, "tol must be finite"),
                      ({"ewald": None, "tol": 0.0}, "tol must be finite"), ({"ewald": None, "tol": 1.5}, "tol must be finite")):
        with pytest.raises(EpnnError, match=match):
            call(**kw)
        still_fine()
    for col, value, match in ((1, 4.5, "rc"), (1, -1.0, "rc"), (1, 0.0, "rc = 0"), (0, 0.0, "beta"), (0, float("nan"), "not finite"),
                              (3, 2.0, "not consistent"), (4, 9.5, "not consistent"), (5, 30000.0, "cap")):
        bad = rows.copy()
        bad[0, col] = value
        with pytest.raises(EpnnError, match=match):
            call(ewald=bad)
        still_fine()
    needle = cells.copy()
    needle[2] = np.diag(np.float32([6, 6, 20000]))
    with pytest.raises(EpnnError, match="cap"):
        call(cell=needle, ewald=None)
    still_fine()
    with pytest.raises(ValueError, match="cell= or box="):
        eng.coulomb_xyz_cell(*batch, N)
    with pytest.raises(EpnnError, match="does not fit N=12"):
        eng.coulomb_xyz_cell(*batch, 12, cell=cells, ewald=rows)
    still_fine()
    # two atoms that coincide through an image: with the sweep (alpha = 0) and without it (beta == alpha)
    twin = xyz.copy()
    twin[2] = np.round(twin[2] * 1024) / 1024                                 # (on a 2^-10 A grid the lattice shift is exact in float32)
    twin[5] = twin[2] + cells[0][0] - cells[0][1]
    assert np.array_equal(twin[5].astype(np.float64) - twin[2], np.float64([8, -8, 0]))
    for kw in ({}, {"alpha": 0.5, "ewald": _rows(eng, cells, 0.5)}):
        with pytest.raises(EpnnError, match="coincide"):
            eng.coulomb_xyz_cell(offsets, twin, x, Q, N, cell=cells, **{"ewald": rows, **kw})
        still_fine()
