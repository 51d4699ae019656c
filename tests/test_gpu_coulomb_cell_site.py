"""Per-atom Gaussian widths, self-energy and on-site terms in the periodic Coulomb call (epnn_coulomb_xyz_cell_site,
Engine.coulomb_xyz_cell_site) on the GPU: the fixed-charge parts and the fixed-charge strain against the float64 reference on the
device's own charges at the parameters the call ran at, the composition with the gradient call and the reduction to the _cell_excl
entry bit for bit, equal widths against the alpha route, the totals against the full float64 reference, images, invariants, refusals
(the width check among them) and the scratch.  GPU only.

Cells and sizes are those of tests/test_gpu_coulomb_cell.py: the packed batch of cells under 64 atoms (one of them a lone atom with
Q = 1), a cell above 64 atoms and one above 128, the sheared cell, a charged cell and pairs nearest through an image.  Widths are drawn
in [0.4, 1.0] of 1 / (2 beta) of each cell's own rule at tol = 1e-6, so every case passes the width check.  The bound is the periodic
tests': 2e-6 of the absolute real-space and listed terms, plus 34 * 2^-24 of the reciprocal ones, plus 2 * 2^-24 of the rest (the
split's and the Gaussians' self terms, the background, and for mu the on-site terms).

Measured worst shares of that bound (MI355X, the 10 runs of test 1, the image pairs and the caller's own row): phi 0.044, mu 0.072, E 0.038
(all on the lone atom of the batch), ffix 0.013 and strain 0.008 (pairs nearest through an image); from 17 atoms on at most 0.006."""
import ctypes as C
import re

import numpy as np
import pytest

import cell_ref
from coulomb_excl_ref import exclusion_cases, shuffled
from site_ref import ewald_site64
from test_gpu_coulomb_cell import BATCH, CELLS, IMAGES, KE, U, _batch, _bound, _pair, _rows, _system, _weights
from test_gpu_coulomb import _cl_pieces
from test_gpu_grad_large import TAU

pytestmark = pytest.mark.gpu

CASES = ["batch", "sheared-17-24", "slab-65-72", "cube14-129-136", "charged"]
_CASES, _ENGINE, _RUNS = {}, [], {}


def _engine(factory):
    if not _ENGINE:
        eng = factory(nx=9, T=2)
        eng.set_weights(_weights())
        eng.set_option("grad_path", 2)
        _ENGINE.append(eng)
    return _ENGINE[0]


def _widths(rng, n, beta):
    return (rng.uniform(0.4, 1.0, n) * 0.5 / beta).astype(np.float32)


def _case(factory, name):
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
        rows = _rows(_engine(factory), cells, 0.0)
        A = int(offsets[-1])
        rng = np.random.default_rng(2000 + A)
        sigma = np.concatenate([_widths(rng, int(offsets[b + 1] - offsets[b]), rows[b][0]) for b in range(len(cells))])
        site = (sigma, rng.normal(size=A).astype(np.float32), np.abs(rng.normal(size=A)).astype(np.float32) * 3)
        per = [exclusion_cases(xyz[offsets[b]:offsets[b + 1]], cells[b]) for b in range(len(cells))]
        pairs = np.concatenate([p + offsets[b] for b, (p, s) in enumerate(per)]).astype(np.int32)
        scale = np.concatenate([s for p, s in per]).astype(np.float32)
        _CASES[name] = (batch, cells, N, rows, site, (pairs, scale), per)
    return _CASES[name]


def _call(eng, case, full, **kw):
    batch, cells, N, rows, (sigma, chi, J), (pairs, scale), per = case
    args = dict(cell=cells, ke=KE, ewald=rows, parts=True, strain=True, sigma=sigma, chi=chi)
    args.update(dict(hardness=J, self_energy=True, exclusions=shuffled(pairs, scale)) if full else dict(self_energy=False))
    args.update(kw)
    return eng.coulomb_xyz_cell_site(*batch, N, **args)


def _run(factory, name, full):
    """The call with parts and strain, once per case.  full: widths, chi, J, the self term and the shuffled list; otherwise widths and
    chi alone.  (engine, case, (q, phi, mu, E, F, gs, ffix, fq, gs_fix, gs_q))."""
    if (name, full) not in _RUNS:
        case = _case(factory, name)
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
          _shares(np.abs(gs_fix - ref.strain), _bound(ref.s_strain, k)))
    print(f"{what} (n = {len(phi)}): phi {sh[0]:.3f}, mu {sh[1]:.3f}, ffix {sh[2]:.3f}, E {sh[3]:.3f}, strain {sh[4]:.3f} of the bounds")
    assert max(sh) <= 1.0, sh
    return sh


def _ref(case, b, q, full, xyz=None):
    (offsets, xyz0, x, Q), cells, N, rows, (sigma, chi, J), lists, per = case
    a0, a1 = offsets[b], offsets[b + 1]
    r = rows[b]
    return ewald_site64((xyz0 if xyz is None else xyz)[a0:a1], q[a0:a1], cells[b], KE, 0.0, sigma[a0:a1], chi[a0:a1], J[a0:a1] if full else None,
                        int(full), r[0], r[1], r[2], r[3:], pairs=per[b][0] if full else None, scale=per[b][1] if full else None)


# ---------------------------------------------------------------------------------------------------- 1: the fixed-charge parts
def test_the_cases_reach_what_they_are_meant_to(gpu_engine_factory):
    sizes = {name: [int(v) for v in np.diff(_case(gpu_engine_factory, name)[0][0])] for name in CASES}
    assert max(sizes["batch"]) < 64 and sum(sizes["batch"]) <= 64 and 1 in sizes["batch"]
    assert 64 < sizes["slab-65-72"][0] <= 128 < sizes["cube14-129-136"][0]
    assert _case(gpu_engine_factory, "charged")[0][3][0] == 1.0 and (_case(gpu_engine_factory, "batch")[0][3] != 0).any()
    for name in CASES:
        batch, cells, N, rows, (sigma, chi, J), (pairs, scale), per = _case(gpu_engine_factory, name)
        for b in range(len(cells)):
            s = sigma[batch[0][b]:batch[0][b + 1]]
            assert (s > 0.19 / rows[b][0]).all() and (s <= 0.5 / rows[b][0]).all() and rows[b][1] > 0
        assert len(pairs) >= 3 and (s.max() > 1.5 * s.min() or len(s) == 1)


@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_fixed_charge_parts_against_float64_on_the_device_charges(gpu_engine_factory, name, full):
    """phi, mu, ffix, E and the nine components of gstrain_fix against ewald_site64 on q_out itself at the rows the call ran at."""
    eng, case, (q, phi, mu, E, F, gs, ffix, fq, gs_fix, gs_q) = _run(gpu_engine_factory, name, full)
    offsets = case[0][0]
    assert E.dtype == np.float64 and E.shape == (len(offsets) - 1,) and gs.shape == (len(offsets) - 1, 3, 3) and mu.shape == q.shape
    for b in range(len(offsets) - 1):
        a0, a1 = offsets[b], offsets[b + 1]
        _check(f"{name} full={full}, cell {b}", _ref(case, b, q, full), phi[a0:a1], mu[a0:a1], E[b], ffix[a0:a1], gs_fix[b])
        assert np.array_equal(gs_fix[b], gs_fix[b].T)
    assert not np.array_equal(mu, phi)


# ---------------------------------------------------------------------------------------------------- 2: composition bits
def _raw(eng, case, alpha, sigma, chi, J, self_term, lists, optional=True):
    """The C entry itself, so that NULL outputs and NULL lists can be passed."""
    from epnn_amd._lib import check, fptr, iptr
    (offsets, xyz, x, Q), cells, N, rows = case[:4]
    B, A = len(offsets) - 1, int(offsets[-1])
    dptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    opt = lambda a, f=fptr: None if a is None else f(a)
    q, phi, mu = (np.empty((A,), np.float32) for _ in range(3))
    F, ffix, fq = (np.empty((A, 3), np.float32) for _ in range(3))
    gs, gsf, gsq = (np.empty((B, 3, 3), np.float32) for _ in range(3))
    E = np.empty((B,), np.float64)
    cells, rows = np.ascontiguousarray(cells, dtype=np.float32), np.ascontiguousarray(rows)
    npairs, ei, ej, es = (0, None, None, None) if lists is None else (len(lists[1]), np.ascontiguousarray(lists[0][:, 0]),
                                                                      np.ascontiguousarray(lists[0][:, 1]), lists[1])
    on = lambda a: fptr(a) if optional else None
    check(eng.lib.epnn_coulomb_xyz_cell_site(eng.h, B, N, iptr(offsets), fptr(xyz), fptr(x), fptr(Q), fptr(cells), dptr(rows), KE, float(alpha),
                                             opt(sigma), opt(chi), opt(J), int(self_term), npairs, opt(ei, iptr), opt(ej, iptr), opt(es), fptr(q),
                                             fptr(phi), on(mu), dptr(E), fptr(F), fptr(gs), on(ffix), on(fq), on(gsf), on(gsq)), eng.lib)
    return q, phi, mu, E, F, gs, ffix, fq, gsf, gsq


@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_composition_with_the_gradient_call_bit_for_bit(gpu_engine_factory, name, full):
    eng, case, out = _run(gpu_engine_factory, name, full)
    batch, cells, N, rows, (sigma, chi, J), (pairs, scale), per = case
    q, phi, mu, E, F, gs, ffix, fq, gs_fix, gs_q = out
    q2, gxyz, gstr = eng.charges_vjp_xyz(*batch, mu, N, cell=cells, strain=True)
    assert np.array_equal(q2, q) and np.array_equal(fq, -gxyz) and np.array_equal(gs_q, gstr)
    assert np.array_equal(F, ffix + fq) and np.array_equal(gs, gs_fix + gs_q) and F.dtype == np.float32 and gs.dtype == np.float32
    assert np.array_equal(q, eng.coulomb_xyz_cell(*batch, N, cell=cells, ke=KE, ewald=rows)[0])
    six = _call(eng, case, full, parts=False)
    assert len(six) == 6 and _same(six, out[:6])
    five = _call(eng, case, full, parts=False, strain=False)
    assert len(five) == 5 and _same(five, out[:5])
    lists = shuffled(pairs, scale) if full else None
    bare = _raw(eng, case, 0.0, sigma, chi, J if full else None, full, lists, optional=False)
    assert _same([bare[k] for k in (0, 1, 3, 4, 5)], [out[k] for k in (0, 1, 3, 4, 5)])
    assert _same(_raw(eng, case, 0.0, sigma, chi, J if full else None, full, lists), out)


# ---------------------------------------------------------------------------------------------------- 3: reduction bits
@pytest.mark.parametrize("alpha", [0.0, 0.5, 2.0])
@pytest.mark.parametrize("name", ["batch", "slab-65-72"])
def test_nothing_given_is_the_cell_excl_entry_bit_for_bit(gpu_engine_factory, name, alpha):
    """alpha = 0.5: beta == alpha and no sweep; 2.0: a sweep with beta < alpha"""
    case = _case(gpu_engine_factory, name)
    batch, cells, N, _, site, (pairs, scale), per = case
    eng = _engine(gpu_engine_factory)
    rows = _rows(eng, cells, alpha)
    for ex in (None, shuffled(pairs, scale)):
        want = eng.coulomb_xyz_cell_excl(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, parts=True, strain=True, exclusions=ex)
        got = eng.coulomb_xyz_cell_site(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, self_energy=False, exclusions=ex, parts=True, strain=True)
        assert len(got) == 10 and _same([got[k] for k in (0, 1, 3, 4, 5, 6, 7, 8, 9)], want)
        assert np.array_equal(got[2], got[1])                    # mu == phi


# ---------------------------------------------------------------------------------------------------- 4: equal widths
@pytest.mark.parametrize("name", ["batch", "sheared-17-24", "slab-65-72", "cube14-129-136"])
def test_equal_widths_against_the_alpha_route(gpu_engine_factory, name):
    """sigma_i = 0.6 / (2 beta_max) in every cell against coulomb_xyz_cell_excl(alpha = 1 / (2 sigma)) at the same rows (alpha > beta: the
    rule's rows for that alpha are those of alpha = 0): two float32 routes, each within the bound of test 1 of the float64 value,
    so within twice that bound of each other; the charges are the same bits."""
    case = _case(gpu_engine_factory, name)
    batch, cells, N, rows, site, (pairs, scale), per = case
    offsets, xyz = batch[0], batch[1]
    eng = _engine(gpu_engine_factory)
    sg = np.full(int(offsets[-1]), 0.6 * 0.5 / rows[:, 0].max(), dtype=np.float32)
    alpha = 0.5 / float(sg[0])
    assert np.array_equal(_rows(eng, cells, alpha), rows)
    ex = shuffled(pairs, scale)
    q, phi, mu, E, F, gs, ffix, fq, gs_fix, gs_q = eng.coulomb_xyz_cell_site(*batch, N, cell=cells, ke=KE, ewald=rows, sigma=sg, self_energy=False,
                                                                           exclusions=ex, parts=True, strain=True)
    q2, phi2, E2, F2, gs2, ffix2, fq2, gsf2, gsq2 = eng.coulomb_xyz_cell_excl(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, exclusions=ex,
                                                                            parts=True, strain=True)
    assert np.array_equal(q, q2) and np.array_equal(mu, phi)
    for b, (p, s) in enumerate(per):
        a0, a1 = offsets[b], offsets[b + 1]
        r = rows[b]
        ref = ewald_site64(xyz[a0:a1], q[a0:a1], cells[b], KE, 0.0, sg[a0:a1], None, None, 0, r[0], r[1], r[2], r[3:], pairs=p, scale=s)
        ref.phi = ref.mu = phi2[a0:a1].astype(np.float64)
        ref.E, ref.ffix, ref.strain = E2[b], ffix2[a0:a1].astype(np.float64), gsf2[b].astype(np.float64)
        _check(f"equal widths {name}, cell {b}", ref, phi[a0:a1], mu[a0:a1], E[b], ffix[a0:a1], gs_fix[b], k=2.0)


# ---------------------------------------------------------------------------------------------------- 5: totals
@pytest.mark.parametrize("name", ["sheared-17-24", "charged"])
def test_total_forces_and_strain_against_the_float64_reference(gpu_engine_factory, name):
    """q from forward64_cell, the fixed parts from ewald_site64 on those charges, fq and gstrain_q from strain64 at g = mu.  The
    standing rule: |F - F_ref| <= 2e-4 max(max |ffix_ref|, max |fq_ref|) + kink and the same for the strain, usable only while
    kink <= 0.05 of that scale."""
    eng, case, (q, phi, mu, E, F, gs, ffix, fq, gs_fix, gs_q) = _run(gpu_engine_factory, name, True)
    (offsets, xyz, x, Q), cells, N, rows, (sigma, chi, J), (pairs, scale), per = case
    w, cell = _weights(), cells[0]
    q64 = cell_ref.forward64_cell(xyz, x, Q[0], cell, w, N=N)[:len(q)]
    e = _ref(case, 0, q64, True)
    (gx, gq), (gxl, gql), (gxh, gqh) = (cell_ref.strain64(xyz, x, Q[0], e.mu, cell, w, N=N, kink_shift=s)[1:] for s in (0.0, +TAU, -TAU))
    f64, gs64 = e.ffix - gx, e.strain + gq
    kink_f, kink_s = np.abs(gxl - gxh).max(), np.abs(gql - gqh).max()
    sf, ss = max(np.abs(e.ffix).max(), np.abs(gx).max()), max(np.abs(e.strain).max(), np.abs(gq).max())
    ef, es = np.abs(F - f64).max(), np.abs(gs[0] - gs64).max()
    print(f"{name}: q {np.abs(q - q64).max():.3e}, mu {np.abs(mu - e.mu).max():.3e} of {np.abs(e.mu).max():.3e}; F {ef:.3e} of {sf:.3e} (kink "
          f"{kink_f:.3e}); gstrain {es:.3e} of {ss:.3e} (kink {kink_s:.3e})")
    assert sf > 0 and ss > 0 and kink_f <= 0.05 * sf and kink_s <= 0.05 * ss
    assert np.abs(q - q64).max() <= 2e-4
    assert ef <= 2e-4 * sf + kink_f and es <= 2e-4 * ss + kink_s


# ---------------------------------------------------------------------------------------------------- images
@pytest.mark.parametrize("k", [0, 4])
def test_pairs_nearest_through_an_image(gpu_engine_factory, k):
    """Two atoms of the sheared cell with Q = 1 whose nearest image lies across a face, and along the shear: that image's term is the
    dominant one.  Then one atom is moved out of the cell by (3, -2, 5) lattice vectors: the results stay those of the wrapped pair."""
    eng = _engine(gpu_engine_factory)
    cell = CELLS["sheared"]
    f = IMAGES[k]
    xyz, x, Q = _pair(cell, f[:3], f[3:], 1.0)
    rows = _rows(eng, cell[None], 0.0)
    sigma = np.float32([0.45, 0.95]) * np.float32(0.5 / rows[0][0])
    chi, J = np.float32([0.7, -1.1]), np.float32([4.0, 6.5])
    moved = xyz.copy()
    moved[1] += (np.float64([3, -2, 5]) @ cell.astype(np.float64)).astype(np.float32)
    assert np.array_equal(moved[1].astype(np.float64) - xyz[1], np.float64([3, -2, 5]) @ cell.astype(np.float64))
    r = rows[0]
    outs = []
    for what, pos in (("wrapped", xyz), ("moved", moved)):
        q, phi, mu, E, F, gs, ffix, fq, gs_fix, gs_q = eng.coulomb_xyz_cell_site(np.int32([0, 2]), pos, x, np.float32([Q]), 8, cell=cell, ke=KE, ewald=rows,
                                                                               sigma=sigma, chi=chi, hardness=J, parts=True, strain=True)
        ref = ewald_site64(xyz, q, cell, KE, 0.0, sigma, chi, J, 1, r[0], r[1], r[2], r[3:])
        _check(f"pair {k} {what}", ref, phi, mu, E[0], ffix, gs_fix[0])
        outs.append(q)
    assert np.abs(outs[0] - outs[1]).max() <= 2e-6


# ---------------------------------------------------------------------------------------------------- 6: invariants
def test_invariants(gpu_engine_factory):
    """sum ffix = 0 per cell to the bound; the list's order and direction; a cell alone at the same N; two calls."""
    eng, case, out = _run(gpu_engine_factory, "batch", True)
    (offsets, xyz, x, Q), cells, N, rows, (sigma, chi, J), (pairs, scale), per = case
    q, ffix = out[0], out[6]
    assert _same(_call(eng, case, True), out)
    assert _same(_call(eng, case, True, exclusions=(pairs, scale)), out)
    assert _same(_call(eng, case, True, exclusions=(pairs[::-1, ::-1], scale[::-1])), out)
    assert not np.array_equal(_call(eng, case, True, exclusions=None)[1], out[1])
    for b, (p, s) in enumerate(per):
        a0, a1 = offsets[b], offsets[b + 1]
        assert np.abs(ffix[a0:a1].sum(0, dtype=np.float64)).max() <= _bound(_ref(case, b, q, True).s_ffix).sum()
        alone = eng.coulomb_xyz_cell_site(np.int32([0, a1 - a0]), xyz[a0:a1], x[a0:a1], Q[b:b + 1], N, cell=cells[b], ke=KE, ewald=rows[b],
                                          sigma=sigma[a0:a1], chi=chi[a0:a1], hardness=J[a0:a1], exclusions=shuffled(p, s, seed=3), parts=True,
                                          strain=True)
        for k, (got, want) in enumerate(zip(alone, out)):
            assert np.array_equal(got, want[b:b + 1] if k in (3, 5, 8, 9) else want[a0:a1]), (b, k)


# ---------------------------------------------------------------------------------------------------- 7: refusals
def test_refusals_leave_the_handle_usable(gpu_engine_factory):
    from epnn_amd._lib import EpnnError
    eng, case, first = _run(gpu_engine_factory, "batch", True)
    batch, cells, N, rows, (sigma, chi, J), (pairs, scale), per = case
    offsets = batch[0]
    A = int(offsets[-1])
    entry = "epnn_coulomb_xyz_cell_site: "

    def still_fine():
        assert _same(_call(eng, case, True), first)

    def with_value(a, k, v):
        a = a.copy()
        a[k] = v
        return a

    # the width check: cell 3's widest Gaussian made 1.25 / (2 beta); named with the cell, sigma_max and the limit
    a3 = int(offsets[3])
    wide = with_value(sigma, a3 + 2, np.float32(1.25 * 0.5 / rows[3][0]))
    with pytest.raises(EpnnError, match=entry + r"cell 3: sigma_max = \S+ is above the largest width 1 / \(2 beta\) = \S+ ") as err:
        _call(eng, case, True, sigma=wide)
    named = [float(v) for v in re.search(r"sigma_max = (\S+) .* 1 / \(2 beta\) = (\S+) ", str(err.value)).groups()]
    assert np.allclose(named, [float(wide[a3 + 2]), 0.5 / rows[3][0]], rtol=1e-5, atol=0)
    still_fine()
    # the same cells with the caller's own row of a smaller beta in cell 3 are served, and right
    own = rows.copy()
    own[3] = _rows(eng, cells[3:4], 0.0, beta=0.75 * rows[3][0])[0]
    out = _call(eng, case, True, sigma=wide, ewald=own)
    case3 = (batch, cells, N, own, (wide, chi, J), (pairs, scale), per)
    q, phi, mu, E, F, gs, ffix, fq, gs_fix, gs_q = out
    _check("own row, cell 3", _ref(case3, 3, q, True), phi[a3:], mu[a3:], E[3], ffix[a3:], gs_fix[3])
    still_fine()
    with pytest.raises(EpnnError, match=entry + "both sigma and alpha"):
        _raw(eng, case, 0.5, sigma, None, None, 0, None)
    with pytest.raises(EpnnError, match=entry + "self_term = 1 with neither sigma nor alpha > 0"):
        _raw(eng, case, 0.0, None, chi, None, 1, None)
    still_fine()
    for bad in (0.0, -0.5, np.nan, np.inf, 1e-30):
        with pytest.raises(EpnnError, match=entry + r"sigma\[7\]"):
            _call(eng, case, True, sigma=with_value(sigma, 7, bad))
    still_fine()
    for bad in (np.nan, np.inf):
        with pytest.raises(EpnnError, match=entry + r"chi\[3\] .*not finite"):
            _call(eng, case, True, chi=with_value(chi, 3, bad))
        with pytest.raises(EpnnError, match=entry + r"hard\[%d\] .*not finite" % (A - 1)):
            _call(eng, case, True, hardness=with_value(J, A - 1, bad))
    still_fine()
    for kw in ({"sigma": sigma[:-1]}, {"chi": chi[1:]}, {"hardness": np.concatenate([J, J])}):
        with pytest.raises(ValueError, match=r"must have shape \(%d,\)" % A):
            _call(eng, case, True, **kw)
    # the _cell_excl entry's refusals
    p = pairs.copy()
    p[2] = (A, 3)
    with pytest.raises(EpnnError, match=entry + r"exclusion pair 2 = .*outside \[0, %d\)" % A):
        _call(eng, case, True, exclusions=(p, scale))
    p[2] = pairs[0][::-1]
    with pytest.raises(EpnnError, match=entry + "exclusion pair 2 = .*listed twice: pair 0"):
        _call(eng, case, True, exclusions=(p, scale))
    bad = rows.copy()
    bad[0, 1] = 4.5
    with pytest.raises(EpnnError, match=entry + ".*rc"):
        _call(eng, case, True, ewald=bad)
    with pytest.raises(EpnnError, match=entry + "ke must be finite"):
        _call(eng, case, True, ke=np.nan)
    still_fine()
    twin = batch[1].copy()
    twin[2] = np.round(twin[2] * 1024) / 1024
    twin[5] = twin[2] + cells[0][0] - cells[0][1]
    with pytest.raises(EpnnError, match="coincide"):
        eng.coulomb_xyz_cell_site(offsets, twin, batch[2], batch[3], N, cell=cells, ewald=rows, sigma=sigma)
    still_fine()


def test_the_model_method_and_the_default_rows(gpu_engine_factory):
    """EPNNModel.coulomb_xyz_cell_site: the engine's call with N = natom; ewald=None is ewald_params(cell, 0, tol) per cell."""
    from epnn_amd import charge_gn
    eng, case, out = _run(gpu_engine_factory, "sheared-17-24", True)
    batch, cells, N, rows, (sigma, chi, J), (pairs, scale), per = case
    model = charge_gn.make_model([32, 32], 48, 2, 9, N)
    model.set_weights_dict(_weights())
    got = model.coulomb_xyz_cell_site(*batch, cell=cells[0], sigma=sigma, chi=chi, hardness=J, exclusions=shuffled(pairs, scale), parts=True, strain=True)
    assert len(got) == 10 and _same(got, out)


# ---------------------------------------------------------------------------------------------------- 8: scratch
def _r256(v):
    return (v + 255) // 256 * 256


@pytest.mark.parametrize("with_list", [False, True])
@pytest.mark.parametrize("name", ["batch", "cube14-129-136"])
def test_scratch_follows_the_formula(gpu_engine_factory, name, with_list):
    """epnn_last_stats out[2] of a site call on a fresh handle against the _cell_excl entry's on the same batch and list, to the byte:
    16 A of staged rows, a buffer of its own rounded up to 256; 4 A of mu at the end of the outputs' buffer ([A] phi | [A][3] ffix |
    flag | [B] E at 8 | [B][9] strain); 8 B of per-cell sums at the end of the sweep's buffer (part [cpieces][A][10] | share [A][7] |
    S [slots] at 16 | rec [slots], float64 and 16-byte records).  A buffer that grows moves its rounding to 256, so the difference is
    stated with the roundings and not as a window: an error of 4 A or 8 B in the formula shows on the 129-atom cell (two pieces)."""
    case = _case(gpu_engine_factory, name)
    batch, cells, N, rows, (sigma, chi, J), (pairs, scale), per = case
    A, B = int(batch[0][-1]), len(cells)
    ex = (pairs, scale) if with_list else None
    stats = []
    for site in (False, True):
        eng = gpu_engine_factory(nx=9, T=2)
        eng.set_weights(_weights())
        if site:
            eng.coulomb_xyz_cell_site(*batch, N, cell=cells, ke=KE, ewald=rows, sigma=sigma, chi=chi, hardness=J, exclusions=ex)
        else:
            eng.coulomb_xyz_cell_excl(*batch, N, cell=cells, ke=KE, ewald=rows, exclusions=ex)
        stats.append(eng.last_stats())
        eng.close()
    cp = max(_cl_pieces(int(n)) for n in np.diff(batch[0]))
    slots = int(((2 * rows[:, 3] + 1) * (2 * rows[:, 4] + 1) * (rows[:, 5] + 1)).sum())
    co = ((4 * A + 1) * 4 + 7) // 8 * 8 + 8 * B + 36 * B
    sc = (cp * A * 80 + A * 56 + 15) // 16 * 16 + 32 * slots
    want = _r256(16 * A) + _r256(co + 4 * A) - _r256(co) + _r256(sc + 8 * B) - _r256(sc)
    got = int(stats[1][2]) - int(stats[0][2])
    print(f"{name}: A = {A}, B = {B}, cpieces {cp}, slots {slots}, list {with_list}: {int(stats[1][2])} bytes, {got} more than the _cell_excl entry, "
          f"stated {want} (20 A + 8 B = {20 * A + 8 * B})")
    assert stats[1][0] == stats[0][0] and got == want
    assert abs(want - (20 * A + 8 * B)) < 3 * 256
