"""Bonded exclusions and pair scaling in the Coulomb calls (epnn_coulomb_xyz_excl, epnn_coulomb_xyz_cell_excl; Engine.coulomb_xyz_excl,
Engine.coulomb_xyz_cell_excl) on the GPU: the fixed-charge parts against the weighted float64 references on the device's own charges,
everything excluded, the bits against the plain entries and across list orders, the composition with the gradient call, the totals
against the full float64 reference, invariants, refusals, the Python layer and the scratch.  GPU only.

The lists come from coulomb_excl_ref.exclusion_cases and reach the library shuffled, half of the rows swapped.  The bound is the plain
calls': 2e-6 of the absolute terms actually added -- the all-pairs or real-space terms and the listed pairs' |(s - 1) term| -- plus
34 * 2^-24 of the absolute reciprocal terms in cells (tests/test_gpu_coulomb_cell.py counts the roundings).

Measured worst shares of that bound (MI355X, the 45 cases of test 1): open molecules phi 0.027, ffix 0.076 (both on the 9-atom
molecule of the batch, which has no pairs: the sweep's own error), E 0.008; cells phi 0.037, ffix 0.026, E 0.015, strain 0.056 (all on
the two-atom cell whose one pair is excluded, beta == alpha).  From 17 atoms on: at most 0.029 (ffix, open 17-24)."""
import ctypes as C
import math

import numpy as np
import pytest

import cell_ref
from conftest import random_weights
from coulomb_excl_ref import add_correction, coulomb64_w, excl_correction64, exclusion_cases, list_stats, pair_shifts, shuffled
from coulomb_ref import coulomb64, coulomb_forces64
from ewald_ref import ewald64
from test_gpu_coulomb import _formula
from test_gpu_coulomb_cell import BATCH, BOUND, CELLS, _batch as _cell_batch, _bound, _rows, _system
from test_gpu_grad_large import TAU, _batch, _lattice_molecule
from xyz_grad_ref import forward64, vjp64

pytestmark = pytest.mark.gpu

KE = 14.3996454784255
ALPHAS = [0.0, 0.5, 2.0]          # cells at tol = 1e-6: beta == alpha and rc == 0 for 0.5 (the correction runs with no sweep), a sweep otherwise
OPEN = [(1, 8), (2, 8), (17, 24), (63, 64), (64, 64), (65, 72), (129, 136)]
OPEN_BATCH = (20, 1, 9, 30)       # at N = 32; the one-atom and the 9-atom molecule get no pairs
CELL = [("cube8", 2, 8), ("sheared", 17, 24), ("cube8", 63, 64), ("sheared", 64, 64), ("slab", 65, 72), ("cube14", 129, 136)]
OPEN_CASES = [f"{n}-{N}" for n, N in OPEN] + ["batch"]
CELL_CASES = [f"{c}-{n}-{N}" for c, n, N in CELL] + ["batch"]
BARE = (1, 2)                     # molecules of the two batches without pairs

_CASES, _ENGINE, _RUNS = {}, [], {}


def _case(kind, name):
    """(batch, cells or None, N, (pairs (P, 2) flat and sorted, scale), per-molecule lists)"""
    if (kind, name) not in _CASES:
        if kind == "open":
            if name == "batch":
                mols, N = [_lattice_molecule(n, 9, seed=700 + n) for n in OPEN_BATCH], 32
            else:
                n, N = (int(v) for v in name.split("-"))
                mols = [_lattice_molecule(n, 9, seed=n)]
            batch, cells = _batch(mols), None
        else:
            if name == "batch":
                systems, N = [_system(c, n, 700 + n) for c, n in BATCH], 32
            else:
                c, n, N = name.split("-")
                systems, N = [_system(c, int(n), int(n))], int(N)
            batch, cells = _cell_batch(systems)
        offsets, xyz = batch[0], batch[1]
        per = []
        for b in range(len(offsets) - 1):
            a0, a1 = offsets[b], offsets[b + 1]
            bare = name == "batch" and b in BARE
            per.append(exclusion_cases(xyz[a0:a1][:1] if bare else xyz[a0:a1], None if cells is None else cells[b]))
        pairs = np.concatenate([p + offsets[b] for b, (p, s) in enumerate(per)]).astype(np.int32)
        scale = np.concatenate([s for p, s in per]).astype(np.float32)
        _CASES[kind, name] = (batch, cells, N, (pairs, scale), per)
    return _CASES[kind, name]


def _engine(factory):
    if not _ENGINE:
        eng = factory(nx=9, T=2)
        eng.set_weights(random_weights(9, 2, seed=5, scale=0.6))
        eng.set_option("grad_path", 2)
        _ENGINE.append(eng)
    return _ENGINE[0]


def _call(eng, kind, batch, cells, N, alpha, rows, exclusions):
    """The call with every part: open (q, phi, E, F, ffix, fq), cells (q, phi, E, F, gs, ffix, fq, gs_fix, gs_q)."""
    if kind == "open":
        return eng.coulomb_xyz_excl(*batch, N, ke=KE, alpha=alpha, parts=True, exclusions=exclusions)
    return eng.coulomb_xyz_cell_excl(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, parts=True, strain=True, exclusions=exclusions)


def _run(factory, kind, name, alpha):
    """The _excl call on the shuffled list, once per case: (engine, case, rows, outputs)."""
    if (kind, name, alpha) not in _RUNS:
        case = _case(kind, name)
        batch, cells, N, (pairs, scale), per = case
        eng = _engine(factory)
        rows = None
        if kind == "cell":
            rows = _rows(eng, cells, alpha)
            if alpha == 0.5:
                assert (rows[:, 1] == 0).all() and (rows[:, 0] == 0.5).all()
            else:
                assert (rows[:, 1] > 0).all() and (alpha == 0 or (rows[:, 0] < alpha).all())
        _RUNS[kind, name, alpha] = (eng, case, rows, _call(eng, kind, batch, cells, N, alpha, rows, shuffled(pairs, scale)))
    return _RUNS[kind, name, alpha]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


def test_the_lists_reach_what_they_are_meant_to():
    """The conditions the shapes were chosen for, asserted so that a changed generator cannot hollow them out."""
    most = 0
    for kind, names in (("open", OPEN_CASES), ("cell", CELL_CASES)):
        for name in names:
            (offsets, xyz, x, Q), cells, N, (pairs, scale), per = _case(kind, name)
            for b, (p, s) in enumerate(per):
                n = int(offsets[b + 1] - offsets[b])
                if name == "batch" and b in BARE:
                    assert len(p) == 0
                    continue
                assert len(p) >= (1 if n >= 2 else 0) and (n < 3 or set(s.tolist()) >= {0.0})
                top, none = list_stats(n, p)
                if kind == "cell":
                    most = max(most, top)
                if n >= 17:
                    assert none >= 1, (kind, name, b)
                    if kind == "cell":
                        assert (np.abs(pair_shifts(xyz[offsets[b]:offsets[b + 1]], cells[b], p)).sum(1) > 0).any(), (name, b)
            sh = shuffled(pairs, scale)
            assert len(pairs) < 4 or (not np.array_equal(sh[0], pairs) and (sh[0][:, 0] > sh[0][:, 1]).any())
    assert most >= 8
    assert [len(_case("cell", n)[3][0]) for n in CELL_CASES[:-1]] == [1, 12, 128, 191, 100, 96]


# ---------------------------------------------------------------------------------------------------- 1: the fixed-charge parts
def _shares(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max())


def _check_open(what, alpha, xyz, q, pairs, scale, phi, Eb, ffix):
    phi64, E64, ffix64, sphi, sff = coulomb64_w(xyz, q, KE, alpha, pairs, scale)
    sE = 0.5 * float(np.abs(q.astype(np.float64)) @ sphi)
    sh = (_shares(np.abs(phi - phi64), BOUND * sphi), _shares(np.abs(ffix - ffix64).max(1), BOUND * sff),
          _shares(np.float64(abs(Eb - E64)), np.float64(BOUND * sE)))
    print(f"{what}, alpha {alpha} (n = {len(q)}, {len(pairs)} pairs): phi {sh[0]:.3f}, ffix {sh[1]:.3f}, E {sh[2]:.3f} of the bounds")
    assert max(sh) <= 1.0, sh
    return sh


def _check_cell(what, alpha, row, xyz, cell, q, pairs, scale, phi, Eb, ffix, gs_fix):
    e = add_correction(ewald64(xyz, q, cell, KE, alpha, row[0], row[1], row[2], row[3:]), excl_correction64(xyz, q, cell, KE, alpha, pairs, scale), q)
    sh = (_shares(np.abs(phi - e.phi), _bound(e.s_phi)), _shares(np.abs(ffix - e.ffix).max(1), _bound(e.s_ffix)),
          _shares(np.float64(abs(Eb - e.E)), np.float64(_bound(e.s_E))), _shares(np.abs(gs_fix - e.strain), _bound(e.s_strain)))
    print(f"{what}, alpha {alpha} (n = {len(q)}, {len(pairs)} pairs): phi {sh[0]:.3f}, ffix {sh[1]:.3f}, E {sh[2]:.3f}, strain {sh[3]:.3f} of the bounds")
    assert max(sh) <= 1.0, sh
    return sh, e


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", OPEN_CASES)
def test_fixed_charge_parts_of_open_molecules_against_float64(gpu_engine_factory, name, alpha):
    """phi, ffix and E against coulomb64_w on q_out itself: each within 2e-6 of the absolute terms actually added."""
    eng, ((offsets, xyz, x, Q), cells, N, lists, per), rows, (q, phi, E, F, ffix, fq) = _run(gpu_engine_factory, "open", name, alpha)
    assert E.dtype == np.float64 and E.shape == (len(offsets) - 1,)
    for b, (p, s) in enumerate(per):
        a0, a1 = offsets[b], offsets[b + 1]
        _check_open(f"open {name}, molecule {b}", alpha, xyz[a0:a1], q[a0:a1], p, s, phi[a0:a1], E[b], ffix[a0:a1])
        if a1 - a0 == 1:
            assert not phi[a0:a1].any() and not ffix[a0:a1].any() and E[b] == 0.0 and q[a0] == Q[b]


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", CELL_CASES)
def test_fixed_charge_parts_in_cells_against_float64(gpu_engine_factory, name, alpha):
    """phi, ffix, E and the fixed-charge strain against ewald64 + excl_correction64 on q_out itself at the parameters the call ran at."""
    eng, ((offsets, xyz, x, Q), cells, N, lists, per), rows, out = _run(gpu_engine_factory, "cell", name, alpha)
    q, phi, E, F, gs, ffix, fq, gs_fix, gs_q = out
    for b, (p, s) in enumerate(per):
        a0, a1 = offsets[b], offsets[b + 1]
        _check_cell(f"cell {name}, cell {b}", alpha, rows[b], xyz[a0:a1], cells[b], q[a0:a1], p, s, phi[a0:a1], E[b], ffix[a0:a1], gs_fix[b])
        assert np.array_equal(gs_fix[b], gs_fix[b].T)


# ---------------------------------------------------------------------------------------------------- 2: everything excluded
_PLAIN_REF = {}


def _plain_reference(n, N, alpha):
    if (n, N, alpha) not in _PLAIN_REF:
        xyz, x, Q = _lattice_molecule(n, 9, seed=n)
        _PLAIN_REF[n, N, alpha] = coulomb_forces64(xyz, x, Q, random_weights(9, 2, seed=5, scale=0.6), N, KE, alpha)
    return _PLAIN_REF[n, N, alpha]


@pytest.mark.parametrize("alpha", [0.0, 2.0])
@pytest.mark.parametrize("n,N", [(17, 24), (65, 72)])
def test_all_pairs_of_a_molecule_at_factor_zero(gpu_engine_factory, n, N, alpha):
    """phi, E and ffix are zero within the bound, whose yardstick is then twice the all-pairs absolute sum; fq, the backward of that
    seed, is zero within the charges-part tolerance 2e-4 max |gxyz_ref|, gxyz_ref the float64 reference's charges part of the same
    molecule with nothing excluded (no kink allowance is taken)."""
    eng = _engine(gpu_engine_factory)
    xyz, x, Q = _lattice_molecule(n, 9, seed=n)
    pairs = np.array([(i, j) for i in range(n) for j in range(i + 1, n)], dtype=np.int32)
    q, phi, E, F, ffix, fq = eng.coulomb_xyz_excl(np.int32([0, n]), xyz, x, np.float32([Q]), N, ke=KE, alpha=alpha, parts=True,
                                                  exclusions=shuffled(pairs, np.zeros(len(pairs), np.float32)))
    plain = coulomb64(xyz, q, KE, alpha)
    sphi, sff = coulomb64_w(xyz, q, KE, alpha, pairs, 0.0)[3:]
    assert np.allclose(sphi, 2 * plain[3], rtol=1e-12) and np.allclose(sff, 2 * plain[4], rtol=1e-12)
    sE = 0.5 * float(np.abs(q.astype(np.float64)) @ sphi)
    print(f"n = {n}, alpha {alpha}: |phi| {_shares(np.abs(phi), BOUND * sphi):.3f}, |ffix| {_shares(np.abs(ffix).max(1), BOUND * sff):.3f}, "
          f"|E| {abs(E[0]) / (BOUND * sE):.3f} of the bounds; |fq| {np.abs(fq).max():.3e}")
    assert (np.abs(phi) <= BOUND * sphi).all() and (np.abs(ffix) <= BOUND * sff[:, None]).all() and abs(E[0]) <= BOUND * sE
    scale = np.abs(_plain_reference(n, N, alpha)[5]).max()
    assert scale > 0 and np.abs(fq).max() <= 2e-4 * scale
    assert np.array_equal(F, ffix + fq)


# ---------------------------------------------------------------------------------------------------- 3: bits
def _raw(eng, kind, batch, cells, N, alpha, rows, npairs, ei, ej, es):
    """The C entry itself, so that NULL lists and any npairs can be passed."""
    from epnn_amd._lib import check, fptr, iptr
    offsets, xyz, x, Q = batch
    B, A = len(offsets) - 1, int(offsets[-1])
    dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    opt = lambda a, f: None if a is None else f(a)
    q, phi, E, F, ffix, fq = (np.empty(s, t) for s, t in (((A,), np.float32), ((A,), np.float32), ((B,), np.float64), ((A, 3), np.float32),
                                                         ((A, 3), np.float32), ((A, 3), np.float32)))
    if kind == "open":
        check(eng.lib.epnn_coulomb_xyz_excl(eng.h, B, N, iptr(offsets), fptr(xyz), fptr(x), fptr(Q), KE, float(alpha), npairs, opt(ei, iptr),
                                            opt(ej, iptr), opt(es, fptr), fptr(q), fptr(phi), dptr(E), fptr(F), fptr(ffix), fptr(fq)), eng.lib)
        return q, phi, E, F, ffix, fq
    gs, gsf, gsq = (np.empty((B, 3, 3), np.float32) for _ in range(3))
    cells = np.ascontiguousarray(cells, dtype=np.float32)
    check(eng.lib.epnn_coulomb_xyz_cell_excl(eng.h, B, N, iptr(offsets), fptr(xyz), fptr(x), fptr(Q), fptr(cells), dptr(np.ascontiguousarray(rows)), KE,
                                             float(alpha), npairs, opt(ei, iptr), opt(ej, iptr), opt(es, fptr), fptr(q), fptr(phi), dptr(E), fptr(F),
                                             fptr(gs), fptr(ffix), fptr(fq), fptr(gsf), fptr(gsq)), eng.lib)
    return q, phi, E, F, gs, ffix, fq, gsf, gsq


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("kind,name", [("open", n) for n in OPEN_CASES] + [("cell", n) for n in CELL_CASES])
def test_bits(gpu_engine_factory, kind, name, alpha):
    eng, (batch, cells, N, (pairs, scale), per), rows, out = _run(gpu_engine_factory, kind, name, alpha)
    offsets, xyz, x, Q = batch
    plain = _call(eng, kind, batch, cells, N, alpha, rows, None)
    # no pairs: NULL lists and empty arrays; every factor 1
    assert _same(_raw(eng, kind, batch, cells, N, alpha, rows, 0, None, None, None), plain)
    assert _same(_call(eng, kind, batch, cells, N, alpha, rows, (np.zeros((0, 2), np.int32), np.zeros(0, np.float32))), plain)
    assert _same(_call(eng, kind, batch, cells, N, alpha, rows, (pairs, 1.0)), plain)
    assert np.array_equal(out[0], plain[0])
    if len(pairs):
        assert not np.array_equal(out[1], plain[1])
    # the sorted list, the list reversed with every pair swapped, and a second run
    assert _same(_call(eng, kind, batch, cells, N, alpha, rows, (pairs, scale)), out)
    assert _same(_call(eng, kind, batch, cells, N, alpha, rows, (pairs[::-1, ::-1], scale[::-1])), out)
    assert _same(_call(eng, kind, batch, cells, N, alpha, rows, shuffled(pairs, scale)), out)
    # a molecule alone at the same N: the rows it has inside the batch
    if name == "batch":
        for b, (p, s) in enumerate(per):
            a0, a1 = offsets[b], offsets[b + 1]
            alone = _call(eng, kind, (np.int32([0, a1 - a0]), xyz[a0:a1], x[a0:a1], Q[b:b + 1]), None if cells is None else cells[b:b + 1], N, alpha,
                          None if rows is None else rows[b:b + 1], shuffled(p, s, seed=3))
            per_atom = (0, 1, 3, 5, 6) if kind == "cell" else (0, 1, 3, 4, 5)
            for k, (got, want) in enumerate(zip(alone, out)):
                assert np.array_equal(got, want[a0:a1] if k in per_atom else want[b:b + 1]), (b, k)


# ---------------------------------------------------------------------------------------------------- 4: composition
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("kind,name", [("open", n) for n in OPEN_CASES] + [("cell", n) for n in CELL_CASES])
def test_composition_with_the_gradient_call_bit_for_bit(gpu_engine_factory, kind, name, alpha):
    eng, (batch, cells, N, lists, per), rows, out = _run(gpu_engine_factory, kind, name, alpha)
    if kind == "open":
        q, phi, E, F, ffix, fq = out
        q2, gxyz = eng.charges_vjp_xyz(*batch, phi, N)
        plain_q = eng.coulomb_xyz(*batch, N, ke=KE, alpha=alpha)[0]
    else:
        q, phi, E, F, gs, ffix, fq, gs_fix, gs_q = out
        q2, gxyz, gstr = eng.charges_vjp_xyz(*batch, phi, N, cell=cells, strain=True)
        assert np.array_equal(gs_q, gstr) and np.array_equal(gs, gs_fix + gs_q) and gs.dtype == np.float32
        plain_q = eng.coulomb_xyz_cell(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows)[0]
    assert np.array_equal(q2, q) and np.array_equal(fq, -gxyz)
    assert np.array_equal(F, ffix + fq) and F.dtype == np.float32
    assert np.array_equal(q, plain_q)


# ---------------------------------------------------------------------------------------------------- 5: totals
@pytest.mark.parametrize("alpha", [0.0, 2.0])
def test_total_forces_of_an_open_molecule_against_the_float64_reference(gpu_engine_factory, alpha):
    """(17, 24): q from forward64, the fixed parts from coulomb64_w on those charges, fq = -vjp64(g = phi) with the ReLU-kink bracket.
    The rule of test_the_charges_part_against_the_float64_reference: |fq - fq_ref| <= 2e-4 max |gxyz_ref| + kink, usable only while
    kink <= 0.05 of it; and F on either part's scale, as the periodic test takes it."""
    eng, ((offsets, xyz, x, Q), cells, N, (pairs, scale), per), rows, (q, phi, E, F, ffix, fq) = _run(gpu_engine_factory, "open", "17-24", alpha)
    w = random_weights(9, 2, seed=5, scale=0.6)
    q64 = forward64(xyz, x, Q[0], w, N=N)[:17]
    phi64, E64, ffix64 = coulomb64_w(xyz, q64, KE, alpha, pairs, scale)[:3]
    fq64, lo, hi = (-vjp64(xyz, x, Q[0], phi64, w, N=N, kink_shift=s)[1] for s in (0, +TAU, -TAU))
    kink, sq = np.abs(lo - hi).max(), np.abs(fq64).max()
    sf = max(np.abs(ffix64).max(), sq)
    print(f"open 17-24, alpha {alpha}: q {np.abs(q - q64).max():.3e}, phi {np.abs(phi - phi64).max():.3e} of {np.abs(phi64).max():.3e}, "
          f"fq {np.abs(fq - fq64).max():.3e} of {sq:.3e}, F {np.abs(F - (ffix64 + fq64)).max():.3e} of {sf:.3e}, kink {kink:.3e}")
    assert sq > 0 and kink <= 0.05 * sq
    assert np.abs(q - q64).max() <= 2e-4
    assert np.abs(fq - fq64).max() <= 2e-4 * sq + kink
    assert np.abs(F - (ffix64 + fq64)).max() <= 2e-4 * sf + kink


@pytest.mark.parametrize("alpha", [0.0, 2.0])
def test_total_forces_and_strain_in_a_cell_against_the_float64_reference(gpu_engine_factory, alpha):
    """sheared-17-24: q from forward64_cell, the fixed parts from ewald64 + excl_correction64 on those charges, fq and gstrain_q from
    strain64 at g = phi.  The rule of test_total_forces_and_strain_against_the_float64_reference: |F - F_ref| <= 2e-4 max(max
    |ffix_ref|, max |fq_ref|) + kink and the same for the strain, usable only while kink <= 0.05 of that scale."""
    eng, ((offsets, xyz, x, Q), cells, N, (pairs, scale), per), rows, out = _run(gpu_engine_factory, "cell", "sheared-17-24", alpha)
    q, phi, E, F, gs, ffix, fq, gs_fix, gs_q = out
    w = random_weights(9, 2, seed=5, scale=0.6)
    cell, row = cells[0], rows[0]
    q64 = cell_ref.forward64_cell(xyz, x, Q[0], cell, w, N=N)[:17]
    e = add_correction(ewald64(xyz, q64, cell, KE, alpha, row[0], row[1], row[2], row[3:]), excl_correction64(xyz, q64, cell, KE, alpha, pairs, scale), q64)
    (gx, gq), (gxl, gql), (gxh, gqh) = (cell_ref.strain64(xyz, x, Q[0], e.phi, cell, w, N=N, kink_shift=s)[1:] for s in (0.0, +TAU, -TAU))
    f64, gs64 = e.ffix - gx, e.strain + gq
    kink_f, kink_s = np.abs(gxl - gxh).max(), np.abs(gql - gqh).max()
    sf, ss = max(np.abs(e.ffix).max(), np.abs(gx).max()), max(np.abs(e.strain).max(), np.abs(gq).max())
    ef, es = np.abs(F - f64).max(), np.abs(gs[0] - gs64).max()
    print(f"sheared-17-24, alpha {alpha}: q {np.abs(q - q64).max():.3e}, phi {np.abs(phi - e.phi).max():.3e} of {np.abs(e.phi).max():.3e}; F {ef:.3e} of "
          f"{sf:.3e} (kink {kink_f:.3e}); gstrain {es:.3e} of {ss:.3e} (kink {kink_s:.3e})")
    assert sf > 0 and ss > 0 and kink_f <= 0.05 * sf and kink_s <= 0.05 * ss
    assert np.abs(q - q64).max() <= 2e-4
    assert ef <= 2e-4 * sf + kink_f and es <= 2e-4 * ss + kink_s


# ---------------------------------------------------------------------------------------------------- 6: invariants
@pytest.mark.parametrize("alpha", [0.0, 2.0])
@pytest.mark.parametrize("kind", ["open", "cell"])
def test_the_fixed_charge_forces_of_a_molecule_add_up_to_zero(gpu_engine_factory, kind, alpha):
    eng, ((offsets, xyz, x, Q), cells, N, lists, per), rows, out = _run(gpu_engine_factory, kind, "batch", alpha)
    q, ffix = out[0], out[5 if kind == "cell" else 4]
    for b, (p, s) in enumerate(per):
        a0, a1 = offsets[b], offsets[b + 1]
        if kind == "open":
            bound = BOUND * coulomb64_w(xyz[a0:a1], q[a0:a1], KE, alpha, p, s)[4].sum()
        else:
            row = rows[b]
            e = add_correction(ewald64(xyz[a0:a1], q[a0:a1], cells[b], KE, alpha, row[0], row[1], row[2], row[3:]),
                               excl_correction64(xyz[a0:a1], q[a0:a1], cells[b], KE, alpha, p, s), q[a0:a1])
            bound = _bound(e.s_ffix).sum()
            assert np.array_equal(out[7][b], out[7][b].T)
        assert np.abs(ffix[a0:a1].sum(0, dtype=np.float64)).max() <= bound


@pytest.mark.parametrize("alpha", ALPHAS)
def test_a_listed_atom_moved_by_a_lattice_vector(gpu_engine_factory, alpha):
    """sheared-17-24 on a 2^-10 A grid (a lattice shift of such a position is exact in float32): the partner of atom 0's first listed
    pair moved by (3, -2, 5) lattice vectors.  phi, ffix, E and the strain stay those of the wrapped system, within the bound."""
    eng = _engine(gpu_engine_factory)
    xyz, x, Q, cell = _system("sheared", 17, 17)
    xyz = (np.round(xyz.astype(np.float64) * 1024) / 1024).astype(np.float32)
    pairs, scale = exclusion_cases(xyz, cell)
    j = int(pairs[0, 1])
    assert pairs[0, 0] == 0 and scale[0] == 0.0
    moved = xyz.copy()
    moved[j] += (np.float64([3, -2, 5]) @ cell.astype(np.float64)).astype(np.float32)
    assert np.array_equal(moved[j].astype(np.float64) - xyz[j], np.float64([3, -2, 5]) @ cell.astype(np.float64))
    rows = _rows(eng, cell[None], alpha)
    outs = [eng.coulomb_xyz_cell_excl(np.int32([0, 17]), r, x, np.float32([Q]), 24, cell=cell, ke=KE, alpha=alpha, ewald=rows, parts=True, strain=True,
                                      exclusions=shuffled(pairs, scale)) for r in (xyz, moved)]
    for what, (q, phi, E, F, gs, ffix, fq, gs_fix, gs_q) in zip(("wrapped", "moved"), outs):
        _check_cell(f"lattice shift, {what}", alpha, rows[0], xyz, cell, q, pairs, scale, phi, E[0], ffix, gs_fix[0])
        assert np.array_equal(gs_fix[0], gs_fix[0].T)
    assert np.abs(outs[0][0] - outs[1][0]).max() <= 2e-6


# ---------------------------------------------------------------------------------------------------- 7: refusals
def _far_pair_system():
    """Two atoms of the 8 A cube 0.55 w_min apart along a face diagonal (each component below half the edge, so this is the nearest
    image and it lies beyond half the width)."""
    s = 0.55 * 8.0 / math.sqrt(2.0)
    xyz = np.float32([[1.0, 1.0, 1.0], [1.0 + s, 1.0 + s, 1.0]])
    x = np.zeros((2, 9), dtype=np.float32)
    x[0, 1] = x[1, 3] = 1.0
    x[:, 0] = [1, 8]
    d = cell_ref.mic(xyz[1].astype(np.float64) - xyz[0], CELLS["cube8"])
    assert abs(math.sqrt((d * d).sum()) - 4.4) < 1e-5
    return np.int32([0, 2]), xyz, x, np.float32([0.0])


@pytest.mark.parametrize("kind", ["open", "cell"])
def test_refusals_leave_the_handle_usable(gpu_engine_factory, kind):
    from epnn_amd._lib import EpnnError
    eng, (batch, cells, N, (pairs, scale), per), rows, first = _run(gpu_engine_factory, kind, "batch", 0.0)
    offsets = batch[0]
    A = int(offsets[-1])
    entry = "epnn_coulomb_xyz_excl" if kind == "open" else "epnn_coulomb_xyz_cell_excl"
    good = shuffled(pairs, scale)

    def still_fine():
        assert _same(_call(eng, kind, batch, cells, N, 0.0, rows, good), first)

    def listed(k, i, j, s=None):
        p, f = pairs.copy(), scale.copy()
        p[k] = (i, j)
        if s is not None:
            f[k] = s
        return p, f

    in0, in3 = int(offsets[0]) + 3, int(offsets[3]) + 3
    for ex, match in ((listed(2, A, in0), r"pair 2 = .*outside \[0, %d\)" % A), (listed(5, in0, -1), "pair 5 = .*outside"),
                      (listed(4, in3, in3), "pair 4 = .*paired with itself"), (listed(1, in0, in3), "pair 1 = .*different molecules"),
                      (listed(3, int(offsets[1]), in0), "pair 3 = .*different molecules"),
                      (listed(7, *pairs[0]), "pair 7 = .*listed twice: pair 0"), (listed(7, *pairs[0][::-1]), "pair 7 = .*listed twice: pair 0"),
                      (listed(6, *pairs[6], s=np.nan), "pair 6 = .*not finite"), (listed(0, *pairs[0], s=np.inf), "pair 0 = .*not finite"),
                      (listed(0, *pairs[0], s=-np.inf), "pair 0 = .*not finite")):
        with pytest.raises(EpnnError, match=entry + ": exclusion " + match):
            _call(eng, kind, batch, cells, N, 0.0, rows, ex)
        still_fine()
    ei, ej, es = (np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1]), scale)
    for npairs, lists, match in ((-1, (ei, ej, es), "npairs = -1 is negative"), (2 ** 30, (ei, ej, es), r"2 npairs must not exceed 2\^31 - 1"),
                                 (len(es), (None, ej, es), "NULL exclusion list"), (len(es), (ei, None, es), "NULL exclusion list"),
                                 (len(es), (ei, ej, None), "NULL exclusion list")):
        with pytest.raises(EpnnError, match=entry + ": .*" + match):
            _raw(eng, kind, batch, cells, N, 0.0, rows, npairs, *lists)
        still_fine()
    with pytest.raises(ValueError, match=r"shape \(P, 2\)"):
        _call(eng, kind, batch, cells, N, 0.0, rows, (pairs.astype(np.float32), scale))
    with pytest.raises(ValueError, match="scale must be a scalar or have shape"):
        _call(eng, kind, batch, cells, N, 0.0, rows, (pairs, scale[:-1]))
    # the plain entry's refusals are the _excl entry's too
    with pytest.raises(EpnnError, match=entry + ": alpha must be finite"):
        _call(eng, kind, batch, cells, N, -1.0, rows, good)
    still_fine()
    if kind == "cell":
        off2, xyz2, x2, Q2 = _far_pair_system()
        cube = CELLS["cube8"]
        for alpha in (0.0, 0.5):                                 # with the sweep and without it
            row = _rows(eng, cube[None], alpha)
            with pytest.raises(EpnnError, match=entry + ": exclusion pair 0 = .*beyond half the smallest perpendicular width"):
                eng.coulomb_xyz_cell_excl(off2, xyz2, x2, Q2, 8, cell=cube, ke=KE, alpha=alpha, ewald=row, exclusions=(np.int32([[1, 0]]), 0.0))
            still_fine()
            # the same two atoms unlisted, or nearer than half the width through an image, are served
            eng.coulomb_xyz_cell_excl(off2, xyz2, x2, Q2, 8, cell=cube, ke=KE, alpha=alpha, ewald=row, exclusions=(np.zeros((0, 2), np.int32), 0.0))
            near = xyz2.copy()
            near[1] = [1.0 + 4.4, 1.0, 1.0]                       # 4.4 along an edge is 3.6 through the face
            eng.coulomb_xyz_cell_excl(off2, near, x2, Q2, 8, cell=cube, ke=KE, alpha=alpha, ewald=row, exclusions=(np.int32([[0, 1]]), 0.0))
    # two listed atoms that coincide
    twin = batch[1].copy()
    i, j = (int(v) for v in pairs[0])
    twin[j] = twin[i]
    with pytest.raises(EpnnError, match="coincide"):
        _call(eng, kind, (offsets, twin, batch[2], batch[3]), cells, N, 0.0, rows, good)
    still_fine()


# ---------------------------------------------------------------------------------------------------- 8: the Python layer
def test_no_exclusions_is_the_plain_entry_and_a_scalar_broadcasts(gpu_engine_factory):
    for kind in ("open", "cell"):
        eng, (batch, cells, N, (pairs, scale), per), rows, out = _run(gpu_engine_factory, kind, "batch", 2.0)
        if kind == "open":
            plain = eng.coulomb_xyz(*batch, N, ke=KE, alpha=2.0, parts=True)
        else:
            plain = eng.coulomb_xyz_cell(*batch, N, cell=cells, ke=KE, alpha=2.0, ewald=rows, parts=True, strain=True)
        plain_bytes = int(eng.last_stats()[2])
        assert _same(_call(eng, kind, batch, cells, N, 2.0, rows, None), plain)
        assert int(eng.last_stats()[2]) == plain_bytes                          # the old entry: none of the _excl entry's buffers
        _call(eng, kind, batch, cells, N, 2.0, rows, (pairs, scale))
        assert int(eng.last_stats()[2]) > plain_bytes
        assert _same(_call(eng, kind, batch, cells, N, 2.0, rows, (pairs, 0.5)),
                     _call(eng, kind, batch, cells, N, 2.0, rows, (pairs.astype(np.int64), np.full(len(pairs), 0.5))))
    eng, (batch, cells, N, lists, per), rows, out = _run(gpu_engine_factory, "open", "batch", 2.0)
    four = eng.coulomb_xyz_excl(*batch, N, ke=KE, alpha=2.0, exclusions=lists)
    assert len(four) == 4 and _same(four, out[:4])


def test_the_model_method_on_a_water_cluster(gpu_engine_factory):
    """Four waters, their bonds through bonded_exclusions: every intramolecular pair is 1-2 or 1-3 and drops out; phi, ffix and E
    against coulomb64_w on the device's charges; EPNNModel and Engine agree."""
    from epnn_amd import charge_gn
    from epnn_amd.engine import bonded_exclusions
    o = np.float64([[0, 0, 0], [3.1, 0.2, 0], [0.1, 3.0, 0.3], [3.0, 3.2, 2.9]])
    xyz = np.concatenate([[c, c + [0.96, 0, 0], c + [-0.24, 0.93, 0]] for c in o]).astype(np.float32)
    x = np.zeros((12, 9), dtype=np.float32)
    x[:, 0] = [8, 1, 1] * 4
    x[np.arange(12), [4, 1, 1] * 4] = 1.0
    bonds = np.array([(3 * m, 3 * m + k) for m in range(4) for k in (1, 2)])
    pairs, scale = bonded_exclusions(bonds, 12)
    assert len(pairs) == 12 and not scale.any()
    off, Q = np.int32([0, 12]), np.float32([0.0])
    model = charge_gn.make_model([32, 32], 48, 2, 9, 16)
    model.set_weights_dict(random_weights(9, 2, seed=5, scale=0.6))
    got = model.coulomb_xyz_excl(off, xyz, x, Q, alpha=0.0, parts=True, exclusions=(pairs, scale))
    want = _engine(gpu_engine_factory).coulomb_xyz_excl(off, xyz, x, Q, 16, alpha=0.0, parts=True, exclusions=(pairs, scale))
    assert len(got) == 6 and _same(got, want)
    q, phi, E, F, ffix, fq = got
    _check_open("water cluster", 0.0, xyz, q, pairs, scale, phi, E[0], ffix)
    plain = model.coulomb_xyz(off, xyz, x, Q, alpha=0.0, parts=True)
    assert _same(model.coulomb_xyz_excl(off, xyz, x, Q, alpha=0.0, parts=True), plain)
    assert np.abs(phi).max() < 0.5 * np.abs(plain[1]).max()                      # the 1 A terms are gone


# ---------------------------------------------------------------------------------------------------- 9: scratch
@pytest.mark.parametrize("kind", ["open", "cell"])
def test_scratch_follows_the_formula(gpu_engine_factory, kind):
    """epnn_last_stats out[2] of an _excl call on a fresh handle: the plain entry's bytes plus (A + 1) 4 + 16 P + 32 A (open) or
    (A + 1) 4 + 16 P + 80 A (cells), two buffers, each rounded up to 256."""
    batch, cells, N, (pairs, scale), per = _case(kind, "batch")
    rows = None if kind == "open" else _rows(_engine(gpu_engine_factory), cells, 0.0)
    A, P = int(batch[0][-1]), len(pairs)
    stats = []
    for ex in (None, (pairs, scale)):
        eng = gpu_engine_factory(nx=9, T=2)
        eng.set_weights(random_weights(9, 2, seed=5, scale=0.6))
        _call(eng, kind, batch, cells, N, 0.0, rows, ex)
        stats.append(eng.last_stats())
        eng.close()
    gain = (A + 1) * 4 + 16 * P + A * (32 if kind == "open" else 80)
    got = int(stats[1][2]) - int(stats[0][2])
    print(f"{kind}: A = {A}, P = {P}: {int(stats[1][2])} bytes, {got} more than the plain entry, formula {gain}")
    assert stats[1][0] == stats[0][0] and gain <= got < gain + 2 * 256
    if kind == "open":                                           # 60 atoms: one task of the sweep; 44 buffers of the plain entry and two more
        want = _formula(OPEN_BATCH, 9, 2, int(stats[1][0]), 1) + gain
        assert want <= int(stats[1][2]) < want + 46 * 256
