"""Per-atom Gaussian widths, self-energy and on-site terms in the slab Coulomb calls (epnn_coulomb_xyz_slab_site,
epnn_coulomb_xyz_slab_strain_site, Engine.coulomb_xyz_slab_site) on the GPU: the fixed-charge parts and the fixed-charge strain against
the float64 reference on the device's own charges at the rows the call ran at, the composition with the gradient call and the
reduction to the slab entries bit for bit, equal widths against the alpha route, the totals against the full float64 reference,
invariants, refusals (the width check among them), the model method and the scratch.  GPU only.

Cells and sizes are those of tests/test_gpu_coulomb_slab.py that reach every packing and piece boundary: a lone atom with Q = 1 (its
energy is its self and on-site terms alone), two atoms, 17 in the sheared cell, 65 in the tilted one (cut into blocks), 129 in the 14 A
square (pieces of the partner range), the 60-atom batch with three different open rows in one wavefront, and a charged sheared slab of
20 atoms with Q = 1.  Widths are drawn in [0.4, 1.0] of 1 / (2 beta) of each cell's own row at tol = 1e-6, alpha = 0, so every case
passes the width check.  The bounds are the slab tests' own, imported: 2e-6 of the absolute real-space and listed terms, 41 * 2^-24 of
the reciprocal terms (43 * 2^-24 for the strain), 16 * 2^-24 of the k = 0 terms, 2 * 2^-24 of "rest" (the split's and the Gaussians'
self terms and, for mu and E, the on-site terms), and for the strain 2 * 2^-24 of its own size.

Measured worst shares of those bounds (MI355X, the 14 runs of test 1, which prints them): phi 0.068, mu 0.025 and E 0.048 (all on the
lone atom, whose values are its self and on-site terms alone), ffix 0.010, strain 0.010; from 17 atoms on at most 0.010.
"""
import ctypes as C
import re

import numpy as np
import pytest

import cell_ref
from coulomb_excl_ref import exclusion_cases, shuffled
from slab_ref import slab_geometry64
from slab_site_ref import slab_site64, slab_site_forces64
from test_gpu_coulomb_slab import BATCH, KE, U, _batch, _bound, _cl_pieces, _rows, _system, _weights
from test_gpu_coulomb_slab_strain import _bound as _bound_strain
from test_gpu_grad_large import TAU

pytestmark = pytest.mark.gpu

CASES = ["sq65-1-8", "sq65-2-8", "sheared-17-24", "tilted-65-72", "sq14-129-136", "batch", "charged"]
TOTALS = ["sheared-17-24", "charged", "tilted-65-72"]
_CASES, _ENGINE, _RUNS, _WORST = {}, [], {}, {}


def _host():
    """An Engine without a handle: the host-only rule epnn_ewald_slab_params needs none, so the cases are the same with and without a device."""
    from epnn_amd import _lib
    from epnn_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.lib, eng.h = _lib.load(), None
    return eng


def _engine(factory):
    if not _ENGINE:
        eng = factory(nx=9, T=2)
        eng.set_weights(_weights())
        eng.set_option("grad_path", 2)
        _ENGINE.append(eng)
    return _ENGINE[0]


def _case(name):
    """(batch, cells, N, rows at tol = 1e-6 and alpha = 0, (sigma, chi, J), (pairs, scale), per-cell lists)"""
    if name not in _CASES:
        if name == "batch":
            systems, N = [_system(c, n, 700 + n) for c, n in BATCH], 32
        elif name == "charged":
            xyz, x, Q, cell = _system("sheared", 20, 20)
            systems, N = [(xyz, x, np.float32(1.0), cell)], 24
        else:
            c, n, N = name.split("-")
            systems, N = [_system(c, int(n), int(n))], int(N)
        batch, cells = _batch(systems)
        offsets, xyz = batch[0], batch[1]
        rows = _rows(_host(), cells, 0.0)
        A = int(offsets[-1])
        rng = np.random.default_rng(2600 + A)
        sigma = np.concatenate([(rng.uniform(0.4, 1.0, int(offsets[b + 1] - offsets[b])) * 0.5 / rows[b][0]).astype(np.float32)
                                for b in range(len(cells))])
        chi = rng.normal(size=A).astype(np.float32)
        site = (sigma, chi, np.abs(rng.normal(size=A)).astype(np.float32) * 3)
        per = [exclusion_cases(xyz[offsets[b]:offsets[b + 1]], cells[b]) for b in range(len(cells))]
        pairs = np.concatenate([p + offsets[b] for b, (p, s) in enumerate(per)]).astype(np.int32).reshape(-1, 2)
        scale = np.concatenate([s for p, s in per]).astype(np.float32)
        _CASES[name] = (batch, cells, N, rows, site, (pairs, scale), per)
    return _CASES[name]


def _call(eng, case, full, **kw):
    batch, cells, N, rows, (sigma, chi, J), (pairs, scale), per = case
    args = dict(cell=cells, ke=KE, ewald=rows, parts=True, strain=True, sigma=sigma, chi=chi)
    args.update(dict(hardness=J, self_energy=True, exclusions=shuffled(pairs, scale)) if full else dict(self_energy=False))
    args.update(kw)
    return eng.coulomb_xyz_slab_site(*batch, N, **args)


def _run(factory, name, full):
    """The strain call with parts, once per case.  full: widths, chi, J, the self term and the shuffled list; otherwise widths and chi
    alone.  (engine, case, (q, phi, mu, E, F, gs, ffix, fq, gs_fix, gs_q))."""
    if (name, full) not in _RUNS:
        case = _case(name)
        eng = _engine(factory)
        _RUNS[name, full] = (eng, case, _call(eng, case, full))
    return _RUNS[name, full]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


def _shares(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max())


def _check(what, ref, phi, mu, Eb, ffix, gs_fix, k=1.0):
    sh = (_shares(np.abs(phi - ref.phi), _bound(ref.s_phi, k)), _shares(np.abs(mu - ref.mu), _bound(ref.s_mu, k)),
          _shares(np.abs(ffix - ref.ffix).max(1), _bound(ref.s_ffix, k)), _shares(np.float64(abs(Eb - ref.E)), np.float64(_bound(ref.s_E, k))),
          _shares(np.abs(gs_fix - ref.strain), k * _bound_strain(ref.strain, ref.s_strain)))
    print(f"{what} (n = {len(phi)}): phi {sh[0]:.3f}, mu {sh[1]:.3f}, ffix {sh[2]:.3f}, E {sh[3]:.3f}, strain {sh[4]:.3f} of the bounds")
    assert max(sh) <= 1.0, sh
    return sh


def _ref(case, b, q, full):
    (offsets, xyz, x, Q), cells, N, rows, (sigma, chi, J), lists, per = case
    a0, a1 = offsets[b], offsets[b + 1]
    r = rows[b]
    return slab_site64(xyz[a0:a1], q[a0:a1], cells[b], KE, 0.0, sigma[a0:a1], chi[a0:a1], J[a0:a1] if full else None, int(full), r[0], r[1], r[2],
                       r[3:], pairs=per[b][0] if full else None, scale=per[b][1] if full else None)


# ---------------------------------------------------------------------------------------------------- 0: the cases
def test_the_cases_pass_the_width_check_and_reach_what_they_are_meant_to():
    sizes = {name: [int(v) for v in np.diff(_case(name)[0][0])] for name in CASES}
    assert sizes["sq65-1-8"] == [1] and sizes["sq65-2-8"] == [2] and sizes["batch"] == [20, 1, 9, 30] and sum(sizes["batch"]) <= 64
    assert 64 < sizes["tilted-65-72"][0] <= 128 < sizes["sq14-129-136"][0] and _cl_pieces(129) > 1
    assert _case("charged")[0][3][0] == 1.0 and _case("sq65-1-8")[0][3][0] == 1.0
    assert len({slab_geometry64(c)[3] for c in _case("batch")[1]}) == 3                       # three different open rows
    for name in CASES:
        batch, cells, N, rows, (sigma, chi, J), (pairs, scale), per = _case(name)
        for b in range(len(cells)):
            s = sigma[batch[0][b]:batch[0][b + 1]]
            assert (s > 0.19 / rows[b][0]).all() and (0.5 / s.astype(np.float64) >= rows[b][0]).all() and rows[b][1] > 0
        big = sigma if name != "batch" else sigma[:20]
        assert len(big) < 17 or (big.max() > 1.5 * big.min() and len(pairs) >= 3)
    assert all(sizes[name][0] >= 17 for name in TOTALS)


# ---------------------------------------------------------------------------------------------------- 1: the fixed-charge parts
@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_fixed_charge_parts_against_float64_on_the_device_charges(gpu_engine_factory, name, full):
    """phi, mu, ffix, E and the nine components of gstrain_fix against slab_site64 on q_out itself at the rows the call ran at."""
    eng, case, (q, phi, mu, E, F, gs, ffix, fq, gs_fix, gs_q) = _run(gpu_engine_factory, name, full)
    offsets = case[0][0]
    assert E.dtype == np.float64 and E.shape == (len(offsets) - 1,) and gs.shape == (len(offsets) - 1, 3, 3) and mu.shape == q.shape
    for b in range(len(offsets) - 1):
        a0, a1 = offsets[b], offsets[b + 1]
        ref = _ref(case, b, q, full)
        sh = _check(f"{name} full={full}, cell {b}", ref, phi[a0:a1], mu[a0:a1], E[b], ffix[a0:a1], gs_fix[b])
        for k, v in zip(("phi", "mu", "ffix", "E", "strain"), sh):
            _WORST[k] = max(_WORST.get(k, 0.0), v)
        assert np.array_equal(gs_fix[b], gs_fix[b].T) and np.array_equal(gs[b], gs[b].T)
        if a1 - a0 == 1 and full:                                # the lone atom: no pair terms, E is its self and on-site terms alone
            assert not ref.s_E["real"] and abs(ref.E) > 0
    print("worst shares so far: " + ", ".join(f"{k} {v:.3f}" for k, v in _WORST.items()))
    assert not np.array_equal(mu, phi)


# ---------------------------------------------------------------------------------------------------- 2: bits
def _raw(eng, case, strain, alpha, sigma, chi, J, self_term, lists, rows=None, optional=True):
    """The C entries themselves, so that NULL outputs and NULL lists can be passed."""
    from epnn_amd._lib import check, fptr, iptr
    (offsets, xyz, x, Q), cells, N, rows0 = case[:4]
    B, A = len(offsets) - 1, int(offsets[-1])
    dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    opt = lambda a, f=fptr: None if a is None else f(a)
    q, phi, mu = (np.empty((A,), np.float32) for _ in range(3))
    F, ffix, fq = (np.empty((A, 3), np.float32) for _ in range(3))
    gs, gsf, gsq = (np.empty((B, 3, 3), np.float32) for _ in range(3))
    E = np.empty((B,), np.float64)
    cells, rows = np.ascontiguousarray(cells, dtype=np.float32), np.ascontiguousarray(rows0 if rows is None else rows)
    npairs, ei, ej, es = (0, None, None, None) if lists is None else (len(lists[1]), np.ascontiguousarray(lists[0][:, 0]),
                                                                      np.ascontiguousarray(lists[0][:, 1]), lists[1])
    on = lambda a: fptr(a) if optional else None
    head = (eng.h, B, N, iptr(offsets), fptr(xyz), fptr(x), fptr(Q), fptr(cells), dptr(rows), KE, float(alpha), opt(sigma), opt(chi), opt(J),
            int(self_term), npairs, opt(ei, iptr), opt(ej, iptr), opt(es), fptr(q), fptr(phi), on(mu), dptr(E), fptr(F))
    if strain:
        check(eng.lib.epnn_coulomb_xyz_slab_strain_site(*head, fptr(gs), on(ffix), on(fq), on(gsf), on(gsq)), eng.lib)
        return q, phi, mu, E, F, gs, ffix, fq, gsf, gsq
    check(eng.lib.epnn_coulomb_xyz_slab_site(*head, on(ffix), on(fq)), eng.lib)
    return q, phi, mu, E, F, ffix, fq


@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_composition_with_the_gradient_call_bit_for_bit(gpu_engine_factory, name, full):
    eng, case, out = _run(gpu_engine_factory, name, full)
    batch, cells, N, rows, (sigma, chi, J), (pairs, scale), per = case
    q, phi, mu, E, F, gs, ffix, fq, gs_fix, gs_q = out
    q2, gxyz, gstr = eng.charges_vjp_xyz(*batch, mu, N, cell=cells, strain=True)
    assert np.array_equal(q2, q) and np.array_equal(fq, -gxyz) and np.array_equal(gs_q, gstr)
    assert np.array_equal(F, ffix + fq) and np.array_equal(gs, gs_fix + gs_q) and F.dtype == np.float32 and gs.dtype == np.float32
    for b in range(len(cells)):
        assert np.array_equal(gs_fix[b], gs_fix[b].T) and np.array_equal(gs[b], gs[b].T)
    # the plain site entry: the strain entry's q, phi, mu, E, F, ffix, fq
    seven = _call(eng, case, full, strain=False)
    assert len(seven) == 7 and _same(seven, out[:5] + out[6:8])
    six = _call(eng, case, full, parts=False)
    assert len(six) == 6 and _same(six, out[:6])
    five = _call(eng, case, full, parts=False, strain=False)
    assert len(five) == 5 and _same(five, out[:5])
    # NULL optional outputs change no other bit; the list's order and direction reach no bit
    lists = shuffled(pairs, scale) if full else None
    bare = _raw(eng, case, True, 0.0, sigma, chi, J if full else None, full, lists, optional=False)
    assert _same([bare[k] for k in (0, 1, 3, 4, 5)], [out[k] for k in (0, 1, 3, 4, 5)])
    bare = _raw(eng, case, False, 0.0, sigma, chi, J if full else None, full, lists, optional=False)
    assert _same([bare[k] for k in (0, 1, 3, 4)], [out[k] for k in (0, 1, 3, 4)])
    assert _same(_raw(eng, case, True, 0.0, sigma, chi, J if full else None, full, lists), out)
    if full and len(pairs):
        assert _same(_call(eng, case, True, exclusions=(pairs, scale)), out)
        assert _same(_call(eng, case, True, exclusions=(pairs[::-1, ::-1], scale[::-1])), out)
    if full and len(pairs) >= 3:
        assert not np.array_equal(_call(eng, case, True, exclusions=None)[1], out[1])


@pytest.mark.parametrize("alpha", [0.0, 0.5, 2.0])
@pytest.mark.parametrize("name", ["batch", "tilted-65-72"])
def test_nothing_given_is_the_slab_entry_bit_for_bit(gpu_engine_factory, name, alpha):
    """alpha = 0.5: beta == alpha and no sweep (rc == 0); 2.0: a sweep with beta < alpha"""
    batch, cells, N, _, site, (pairs, scale), per = _case(name)
    eng = _engine(gpu_engine_factory)
    rows = _rows(eng, cells, alpha)
    assert ((rows[:, 1] == 0).all() and (rows[:, 0] == 0.5).all()) if alpha == 0.5 else (rows[:, 1] > 0).all()
    for ex in (None, shuffled(pairs, scale)):
        want = eng.coulomb_xyz_slab_strain(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, parts=True, exclusions=ex)
        got = eng.coulomb_xyz_slab_site(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, self_energy=False, exclusions=ex, parts=True, strain=True)
        assert len(got) == 10 and _same([got[k] for k in (0, 1, 3, 4, 5, 6, 7, 8, 9)], want)
        assert np.array_equal(got[2], got[1])                    # mu == phi
        want = eng.coulomb_xyz_slab(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, parts=True, exclusions=ex)
        got = eng.coulomb_xyz_slab_site(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, self_energy=False, exclusions=ex, parts=True)
        assert len(got) == 7 and _same([got[k] for k in (0, 1, 3, 4, 5, 6)], want) and np.array_equal(got[2], got[1])
    # on-site terms and the self term through alpha, no widths, where the sweep is skipped (rc == 0) and where it runs
    if alpha > 0:
        sigma, chi, J = site
        q, phi, mu, E, F, gs, ffix, fq, gs_fix, gs_q = eng.coulomb_xyz_slab_site(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, chi=chi,
                                                                               hardness=J, parts=True, strain=True)
        offsets, xyz = batch[0], batch[1]
        for b in range(len(cells)):
            a0, a1 = offsets[b], offsets[b + 1]
            r = rows[b]
            ref = slab_site64(xyz[a0:a1], q[a0:a1], cells[b], KE, alpha, None, chi[a0:a1], J[a0:a1], 1, r[0], r[1], r[2], r[3:])
            _check(f"{name} alpha={alpha} without widths, cell {b}", ref, phi[a0:a1], mu[a0:a1], E[b], ffix[a0:a1], gs_fix[b])


# ---------------------------------------------------------------------------------------------------- 3: equal widths
@pytest.mark.parametrize("name", ["batch", "sheared-17-24", "tilted-65-72", "sq14-129-136"])
def test_equal_widths_against_the_alpha_route(gpu_engine_factory, name):
    """sigma_i = 0.6 / (2 beta_max) in every cell against coulomb_xyz_slab_strain(alpha = 1 / (2 sigma)) at the same rows: two float32
    routes (one takes rsqrtf per pair: not the same bits), each within the bound of test 1 of the float64 value, so within the sum
    of both bounds of each other; the charges are the same bits."""
    case = _case(name)
    batch, cells, N, rows, site, (pairs, scale), per = case
    offsets, xyz = batch[0], batch[1]
    eng = _engine(gpu_engine_factory)
    sg = np.full(int(offsets[-1]), 0.6 * 0.5 / rows[:, 0].max(), dtype=np.float32)
    alpha = 0.5 / float(sg[0])
    assert (alpha > rows[:, 0]).all()
    ex = shuffled(pairs, scale)
    q, phi, mu, E, F, gs, ffix, fq, gs_fix, gs_q = eng.coulomb_xyz_slab_site(*batch, N, cell=cells, ke=KE, ewald=rows, sigma=sg, self_energy=False,
                                                                           exclusions=ex, parts=True, strain=True)
    q2, phi2, E2, F2, gs2, ffix2, fq2, gsf2, gsq2 = eng.coulomb_xyz_slab_strain(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, exclusions=ex,
                                                                              parts=True)
    assert np.array_equal(q, q2) and np.array_equal(mu, phi)
    for b, (p, s) in enumerate(per):
        a0, a1 = offsets[b], offsets[b + 1]
        r = rows[b]
        ref = slab_site64(xyz[a0:a1], q[a0:a1], cells[b], KE, 0.0, sg[a0:a1], None, None, 0, r[0], r[1], r[2], r[3:], pairs=p, scale=s)
        ref.phi = ref.mu = phi2[a0:a1].astype(np.float64)
        ref.E, ref.ffix, ref.strain = E2[b], ffix2[a0:a1].astype(np.float64), gsf2[b].astype(np.float64)
        _check(f"equal widths {name}, cell {b}", ref, phi[a0:a1], mu[a0:a1], E[b], ffix[a0:a1], gs_fix[b], k=2.0)


# ---------------------------------------------------------------------------------------------------- 4: totals
_TOTAL = {}


def _total(name):
    """The float64 model of one single-cell case: (q, e, f, fq, gstrain, gstrain_q, kink_f, kink_s), the kink bracket at +-TAU."""
    if name not in _TOTAL:
        (offsets, xyz, x, Q), cells, N, rows, (sigma, chi, J), (pairs, scale), per = _case(name)
        kw = dict(sigma=sigma, chi=chi, hard=J, self_term=1, pairs=per[0][0], scale=per[0][1])
        mid, lo, hi = (slab_site_forces64(xyz, x, Q[0], cells[0], _weights(), N, KE, 0.0, rows[0], kink_shift=s, **kw) for s in (0.0, +TAU, -TAU))
        _TOTAL[name] = mid + (np.abs(lo[3] - hi[3]).max(), np.abs(lo[5] - hi[5]).max())
    return _TOTAL[name]


@pytest.mark.parametrize("name", TOTALS)
def test_total_forces_and_strain_against_the_float64_reference(gpu_engine_factory, name):
    """q from forward64_cell, the fixed parts from slab_site64 on those charges, fq and gstrain_q from strain64 at g = mu.  The rule of
    test_gpu_coulomb_slab.py: |F - F_ref| <= 2e-4 max(max |ffix_ref|, max |fq_ref|) + kink, kink = max |ref(+TAU) - ref(-TAU)|, and the
    same for the strain; the bracket may be used only while it is at most 0.05 of that scale, asserted on the reference alone (the
    seeds of these three cases meet it, checked on the CPU: the bracket is 0.0002 to 0.005 of the scale)."""
    q64, e, f64, fq64, gs64, gsq64, kink_f, kink_s = _total(name)
    sf, ss = max(np.abs(e.ffix).max(), np.abs(fq64).max()), max(np.abs(e.strain).max(), np.abs(gsq64).max())
    assert sf > 0 and ss > 0 and kink_f <= 0.05 * sf and kink_s <= 0.05 * ss
    eng, case, (q, phi, mu, E, F, gs, ffix, fq, gs_fix, gs_q) = _run(gpu_engine_factory, name, True)
    ef, es = np.abs(F - f64).max(), np.abs(gs[0] - gs64).max()
    print(f"{name}: q {np.abs(q - q64).max():.3e}, mu {np.abs(mu - e.mu).max():.3e} of {np.abs(e.mu).max():.3e}; F {ef:.3e} of {sf:.3e} (kink "
          f"{kink_f:.3e}); gstrain {es:.3e} of {ss:.3e} (kink {kink_s:.3e})")
    assert np.abs(q - q64).max() <= 2e-4
    assert ef <= 2e-4 * sf + kink_f and es <= 2e-4 * ss + kink_s


# ---------------------------------------------------------------------------------------------------- 5: invariants
def test_invariants(gpu_engine_factory):
    """Two calls; a cell alone at the same N; sum f in the plane."""
    eng, case, out = _run(gpu_engine_factory, "batch", True)
    (offsets, xyz, x, Q), cells, N, rows, (sigma, chi, J), (pairs, scale), per = case
    q, F, ffix, fq = out[0], out[4], out[6], out[7]
    assert _same(_call(eng, case, True), out)
    for b, (p, s) in enumerate(per):
        a0, a1 = offsets[b], offsets[b + 1]
        # sum_i ffix_i = 0 to the bound on the cell's summed absolute terms (all three components: Newton's third law pair by pair);
        # f = ffix + fq, and fq sums to zero in the plane (the charges do not change under an in-plane translation) within the grade the
        # total-forces rule gives every atom's fq, 2e-4 of the larger of max |ffix| and max |fq|
        bf = _bound(_ref(case, b, q, True).s_ffix).sum()
        assert np.abs(ffix[a0:a1].sum(0, dtype=np.float64)).max() <= bf
        nhat = slab_geometry64(cells[b])[5]
        tot = F[a0:a1].sum(0, dtype=np.float64)
        inplane = tot - (tot @ nhat) * nhat
        scale_f = max(np.abs(ffix[a0:a1]).max(), np.abs(fq[a0:a1]).max())
        assert np.abs(inplane).max() <= bf + (a1 - a0) * 2e-4 * scale_f
        alone = eng.coulomb_xyz_slab_site(np.int32([0, a1 - a0]), xyz[a0:a1], x[a0:a1], Q[b:b + 1], N, cell=cells[b], ke=KE, ewald=rows[b],
                                          sigma=sigma[a0:a1], chi=chi[a0:a1], hardness=J[a0:a1], exclusions=shuffled(p, s, seed=3), parts=True,
                                          strain=True)
        for k, (got, want) in enumerate(zip(alone, out)):
            assert np.array_equal(got, want[b:b + 1] if k in (3, 5, 8, 9) else want[a0:a1]), (b, k)


def test_a_constant_added_to_chi_of_a_charged_slab(gpu_engine_factory):
    """chi -> chi + c on the charged slab (Q = 1): ffix keeps its bits (it does not see chi); mu shifts by the constant itself, within
    the float32 rounding of both values (phi is the same float64 in both runs); E shifts by sum_i q_i d_i, d the shift as float32 took
    it, within the float64 roundings of two sums of A terms (2^-44 of E's absolute terms); fq = -sum_k mu_k dq_k/dr changes by
    c sum_k dq_k/dr = 0 (Q is conserved), within the total-forces rule's 2e-4 of the larger of max |ffix| and max |fq|."""
    eng, case, out = _run(gpu_engine_factory, "charged", True)
    (offsets, xyz, x, Q), cells, N, rows, (sigma, chi, J), (pairs, scale), per = case
    q, phi, mu, E, F, gs, ffix, fq, gs_fix, gs_q = out
    chi2 = (chi + np.float32(0.5)).astype(np.float32)
    d = chi2.astype(np.float64) - chi
    q2, phi2, mu2, E2, F2, gs2, ffix2, fq2, gs_fix2, gs_q2 = _call(eng, case, True, chi=chi2)
    assert np.array_equal(q2, q) and np.array_equal(phi2, phi) and np.array_equal(ffix2, ffix) and np.array_equal(gs_fix2, gs_fix)
    assert (np.abs(mu2.astype(np.float64) - mu - d) <= U * (np.abs(mu) + np.abs(mu2))).all()
    ref = _ref(case, 0, q, True)
    s_E = sum(ref.s_E.values()) + float(np.abs(q * d).sum())
    shift = float(q.astype(np.float64) @ d)
    assert abs(shift - 0.5) <= 1e-5 and abs((E2[0] - E[0]) - shift) <= 2.0 ** -44 * s_E
    sf = max(np.abs(ffix).max(), np.abs(fq).max())
    print(f"chi + 0.5: E shifts by {E2[0] - E[0]:.9f} (sum q d = {shift:.9f}), |dfq| {np.abs(fq2 - fq).max():.3e} of {sf:.3e}")
    assert np.abs(fq2 - fq).max() <= 2e-4 * sf and np.abs(gs_q2 - gs_q).max() <= 2e-4 * max(np.abs(gs_fix).max(), np.abs(gs_q).max())


# ---------------------------------------------------------------------------------------------------- 6: refusals
def test_refusals_leave_the_handle_usable(gpu_engine_factory):
    from epnn_amd._lib import EpnnError
    eng, case, first = _run(gpu_engine_factory, "batch", True)
    batch, cells, N, rows, (sigma, chi, J), (pairs, scale), per = case
    offsets, xyz = batch[0], batch[1]
    A = int(offsets[-1])

    def still_fine():
        assert _same(_call(eng, case, True), first)

    def with_value(a, k, v):
        a = a.copy()
        a[k] = v
        return a

    for strain, entry in ((True, "epnn_coulomb_xyz_slab_strain_site: "), (False, "epnn_coulomb_xyz_slab_site: ")):
        # the width check: cell 3's widest Gaussian made 1.25 / (2 beta); named with the cell, sigma_max and the limit
        a3 = int(offsets[3])
        wide = with_value(sigma, a3 + 2, np.float32(1.25 * 0.5 / rows[3][0]))
        with pytest.raises(EpnnError, match=entry + r"cell 3: sigma_max = \S+ is above the largest width 1 / \(2 beta\) = \S+ ") as err:
            _call(eng, case, True, sigma=wide, strain=strain)
        named = [float(v) for v in re.search(r"sigma_max = (\S+) .* 1 / \(2 beta\) = (\S+) ", str(err.value)).groups()]
        assert np.allclose(named, [float(wide[a3 + 2]), 0.5 / rows[3][0]], rtol=1e-5, atol=0)
        with pytest.raises(EpnnError, match=entry + "both sigma and alpha"):
            _raw(eng, case, strain, 0.5, sigma, None, None, 0, None)
        with pytest.raises(EpnnError, match=entry + "self_term = 1 with neither sigma nor alpha > 0"):
            _raw(eng, case, strain, 0.0, None, chi, None, 1, None)
        with pytest.raises(EpnnError, match=entry + "self_term = 2 must be 0 or 1"):
            _raw(eng, case, strain, 0.0, sigma, chi, None, 2, None)
        still_fine()
        for bad in (0.0, -0.5, np.nan, np.inf, 1e-30):
            with pytest.raises(EpnnError, match=entry + r"sigma\[7\]"):
                _call(eng, case, True, sigma=with_value(sigma, 7, bad), strain=strain)
        for bad in (np.nan, np.inf):
            with pytest.raises(EpnnError, match=entry + r"chi\[3\] .*not finite"):
                _call(eng, case, True, chi=with_value(chi, 3, bad), strain=strain)
            with pytest.raises(EpnnError, match=entry + r"hard\[%d\] .*not finite" % (A - 1)):
                _call(eng, case, True, hardness=with_value(J, A - 1, bad), strain=strain)
        still_fine()
        # wires and cubes, as today; the row checks; the list's checks
        cube, wire = cells.copy(), cells.copy()
        cube[0, 2, 2] = 6.5
        wire[0, 1] = 0
        for kw, match in (({"cell": cube}, "use epnn_coulomb_xyz_cell"), ({"cell": wire}, "not built"), ({"ke": np.nan}, "ke must be finite")):
            with pytest.raises(EpnnError, match=entry + ".*" + match):
                _call(eng, case, True, strain=strain, **kw)
        bad = rows.copy()
        bad[0, 1] = 4.5
        with pytest.raises(EpnnError, match=entry + ".*rc"):
            _call(eng, case, True, ewald=bad, strain=strain)
        p = pairs.copy()
        p[2] = (A, 3)
        with pytest.raises(EpnnError, match=entry + r"exclusion pair 2 = .*outside \[0, %d\)" % A):
            _call(eng, case, True, exclusions=(p, scale), strain=strain)
        p[2] = pairs[0][::-1]
        with pytest.raises(EpnnError, match=entry + "exclusion pair 2 = .*listed twice: pair 0"):
            _call(eng, case, True, exclusions=(p, scale), strain=strain)
        still_fine()
        # a listed pair beyond half the smaller width (cell 3, the 14 A square: half of it is 7 A), after the device pass
        r3 = xyz[a3:].astype(np.float64)
        d = cell_ref.mic64(r3[:, None, :] - r3[None, :, :], *cell_ref.duals64(cells[3].astype(np.float64)))
        i, j = np.argwhere(np.sqrt((d * d).sum(-1)) > 7.2)[0]
        with pytest.raises(EpnnError, match=entry + r"exclusion pair 0 = \(%d, %d\): its atoms are \S+ apart, beyond half the smallest" % (a3 + i, a3 + j)):
            _call(eng, case, True, exclusions=(np.int32([[a3 + i, a3 + j]]), 0.5), strain=strain)
        still_fine()
    for kw in ({"sigma": sigma[:-1]}, {"chi": chi[1:]}, {"hardness": np.concatenate([J, J])}):
        with pytest.raises(ValueError, match=r"must have shape \(%d,\)" % A):
            _call(eng, case, True, **kw)
    # the same cells with the caller's own row of a smaller beta in cell 3 are served, and right
    wide = with_value(sigma, int(offsets[3]) + 2, np.float32(1.25 * 0.5 / rows[3][0]))
    own = rows.copy()
    own[3] = _rows(eng, cells[3:4], 0.0, beta=0.75 * rows[3][0])[0]
    q, phi, mu, E, F, gs, ffix, fq, gs_fix, gs_q = _call(eng, case, True, sigma=wide, ewald=own)
    case3 = (batch, cells, N, own, (wide, chi, J), (pairs, scale), per)
    a3 = int(offsets[3])
    _check("own row, cell 3", _ref(case3, 3, q, True), phi[a3:], mu[a3:], E[3], ffix[a3:], gs_fix[3])
    still_fine()


# ---------------------------------------------------------------------------------------------------- 7: the model method, the scratch
def test_the_model_method_and_the_default_rows(gpu_engine_factory):
    """EPNNModel.coulomb_xyz_slab_site: the engine's call with N = natom; ewald=None is ewald_slab_params(cell, 0, tol) per cell."""
    from epnn_amd import charge_gn
    eng, case, out = _run(gpu_engine_factory, "sheared-17-24", True)
    batch, cells, N, rows, (sigma, chi, J), (pairs, scale), per = case
    model = charge_gn.make_model([32, 32], 48, 2, 9, N)
    model.set_weights_dict(_weights())
    got = model.coulomb_xyz_slab_site(*batch, cell=cells[0], sigma=sigma, chi=chi, hardness=J, exclusions=shuffled(pairs, scale), parts=True, strain=True)
    assert len(got) == 10 and _same(got, out)
    got = model.coulomb_xyz_slab_site(*batch, cell=cells[0], sigma=sigma, chi=chi, hardness=J, exclusions=shuffled(pairs, scale), parts=True)
    assert len(got) == 7 and _same(got, out[:5] + out[6:8])


def _r256(v):
    return (v + 255) // 256 * 256


@pytest.mark.parametrize("strain", [False, True])
@pytest.mark.parametrize("with_list", [False, True])
@pytest.mark.parametrize("name", ["batch", "sq14-129-136"])
def test_scratch_follows_the_formula(gpu_engine_factory, name, with_list, strain):
    """epnn_last_stats out[2] of a site call on a fresh handle against the slab entry's on the same batch and list: 16 A of staged rows,
    a buffer of its own rounded up to 256, and 4 A of mu at the end of the outputs' buffer ([A] phi | [A][3] ffix | flag | [B] E at 8 |
    strain: [B][9]); no per-cell sum.  Within 256 bytes per buffer of 20 A, and to the byte once the two roundings are written out."""
    batch, cells, N, rows, (sigma, chi, J), (pairs, scale), per = _case(name)
    A, B = int(batch[0][-1]), len(cells)
    ex = (pairs, scale) if with_list else None
    stats = []
    for site in (False, True):
        eng = gpu_engine_factory(nx=9, T=2)
        eng.set_weights(_weights())
        if site:
            eng.coulomb_xyz_slab_site(*batch, N, cell=cells, ke=KE, ewald=rows, sigma=sigma, chi=chi, hardness=J, exclusions=ex, strain=strain)
        elif strain:
            eng.coulomb_xyz_slab_strain(*batch, N, cell=cells, ke=KE, ewald=rows, exclusions=ex)
        else:
            eng.coulomb_xyz_slab(*batch, N, cell=cells, ke=KE, ewald=rows, exclusions=ex)
        stats.append(eng.last_stats())
        eng.close()
    co = ((4 * A + 1) * 4 + 7) // 8 * 8 + 8 * B + (36 * B if strain else 0)
    want = _r256(16 * A) + _r256(co + 4 * A) - _r256(co)
    got = int(stats[1][2]) - int(stats[0][2])
    print(f"{name}: A = {A}, B = {B}, list {with_list}, strain {strain}: {int(stats[1][2])} bytes, {got} more than the slab entry, stated {want} "
          f"(20 A = {20 * A})")
    assert stats[1][0] == stats[0][0] and abs(got - 20 * A) < 2 * 256 and got == want
