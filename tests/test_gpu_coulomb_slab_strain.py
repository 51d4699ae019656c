"""The strain derivative of the slab sum (epnn_coulomb_xyz_slab_strain, Engine.coulomb_xyz_slab_strain) on the GPU: the fixed-charge
strain against the float64 reference on the device's own charges, the composition with the gradient call and with the plain slab call
bit for bit, the total against the full float64 reference, the single charge, invariants, exclusions, refusals and scratch.  GPU only.

The bound of a component W_ab of gstrain_fix (tests/slab_strain_ref.py defines the absolute terms s_real, s_rec, s_k0, s_excl):
    2e-6 (s_real + s_excl) + C_S 2^-24 s_rec + C_0S 2^-24 s_k0 + 2 * 2^-24 |W_ab|
2e-6 is the bound of the real-space sweep and of the listed pairs' kernel, which run unchanged (test_gpu_coulomb_cell.py holds their
virial rows to it).  C_S and C_0S count the roundings of k_sl_sweep_strain as written, in units of 2^-24 of a term's scale, on top of
the counts in the header of test_gpu_coulomb_slab.py, whose values are used here: the phase and sincosf 9.8 (sine or cosine, of a
value below 1); Fs = Fa + Fb 21 units of Fs, and Fa - Fb likewise 21 units OF Fs (20 on Fa + Fb and the difference's rounding), which
is why the reference counts |Fd| as Fs; the weights w, wk 1 each.  Every sum over j and k is float64, and the expansion through g_a,
g_b and nhat in k_sl_atom_strain is float64: an error of a sum in the slot integers' basis is weighed by |g| components, which is why
the reference counts k_a and k_a k_b in that basis.
  -(E_rec + E_k0) (delta_ab - n_a n_b): the sweep's phi sum, per term c Fs |q_j|                                                   34.8
  sum[5], n_a n_b z (wk q_j) cos Fd: wk (1), the cosine (9.8), Fd (21), z rounded from float64 (1), four products (4)              36.8
  sum[6], sum[7], z (w q_j) sin Fs m: w (1), the sine (9.8), Fs (21), z (1), five products, the last with the integer m (5)         38.8
  sum[8..10], (w q_j cos / k) [Fs / k + |z| (Fb - Fa) + G] m m':
      the factor: w (1), cos (9.8), 1 / k rounded from float64 (1), three products (3)                                             14.8
      the bracket, three terms of one sign, in units of their sum Fs / k + |z| Fs + G: Fs / k: Fs (21), 1 / k (1), the product (1):
      23; |z| (Fb - Fa): 21 units of Fs, |z| (1), the product (1): 23; G = cg eg: cg and eg rounded from float64, the product: 3;
      the larger (23) and the two additions (2)                                                                                      25
      factor times bracket (1), times m, times m' (2)                                                                                 3
                                                                                                                                   42.8
  C_S = 43 covers every kind of reciprocal term.
  k = 0: the phi sum's 16 on the bracket times |delta_ab - n_a n_b|; sum[5] -= ((cn q_j) er) |z|: cn (1), beta |z| rounded from float64
      at erf's sensitivity <= 1 (1), erff's 4 ulp (8), |z| (1), three products (3): 14.                                 C_0S = 16
The float64 sums are rounded to float32 once: 1 of the 2 * 2^-24 |W_ab|.

Measured worst share of the bound (MI355X, the 25 cases of test 1, which prints it): 0.025 (the lone atom of the batch, beta == alpha).
The bound counts worst-case roundings per term; the errors of a sum's terms do not add up in phase."""
import ctypes as C

import numpy as np
import pytest

import coulomb_excl_ref as xref
from slab_ref import slab_geometry64
from slab_strain_ref import slab_strain64, slab_strain_forces64
from test_gpu_coulomb_slab import (BATCH, CELLS, KE, PSETS, U, _batch, _cl_pieces, _engine, _formula, _listed_slots, _rows, _system, _water_slab,
                                   _weights)
from test_gpu_grad_large import TAU

pytestmark = pytest.mark.gpu

BOUND = 2e-6
C_S = 43
C_0S = 16
SINGLE = [("sq65", 1, 8), ("sq65", 2, 8), ("sheared", 17, 24), ("tilted", 63, 64), ("sheared", 64, 64), ("tilted", 65, 72), ("sq14", 129, 136)]
CASES = [f"{c}-{n}-{N}" for c, n, N in SINGLE] + ["batch"]
SETS = [(name, pset) for name in CASES for pset in ("a0", "a05", "near")] + [("sheared-17-24", "fine")]

_CASES, _RUNS, _REF64, _WORST = {}, {}, {}, {}


def _case(name):
    if name not in _CASES:
        if name == "batch":
            _CASES[name] = ([_system(c, n, 700 + n) for c, n in BATCH], 32)
        else:
            c, n, N = name.split("-")
            _CASES[name] = ([_system(c, int(n), int(n))], int(N))
    return _CASES[name]


def _run(factory, name, pset):
    """The strain call with parts, once per case: (engine, batch, cells, N, alpha, rows, the nine outputs)."""
    if (name, pset) not in _RUNS:
        systems, N = _case(name)
        eng = _engine(factory)
        batch, cells = _batch(systems)
        alpha, beta, tol = PSETS[pset]
        rows = _rows(eng, cells, alpha, tol, beta)
        assert ((rows[:, 1] == 0).all() and (rows[:, 0] == 0.5).all()) if pset == "a05" else (rows[:, 1] > 0).all()
        out = eng.coulomb_xyz_slab_strain(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, parts=True)
        assert len(out) == 9
        _RUNS[name, pset] = (eng, batch, cells, N, alpha, rows, out)
    return _RUNS[name, pset]


def _ref(key, xyz, q, cell, alpha, row, exclusions=None):
    if key not in _REF64:
        _REF64[key] = slab_strain64(xyz, q, cell, KE, alpha, row[0], row[1], row[2], row[3:], exclusions)
    return _REF64[key]


def _bound(W, s):
    return BOUND * (s["real"] + s.get("excl", 0.0)) + C_S * U * s["rec"] + C_0S * U * s["k0"] + 2 * U * np.abs(W)


def _check(what, got, W, s):
    """One cell's gstrain_fix (3, 3) against the reference, per component; returns the worst share of the bound."""
    b = _bound(W, s)
    err = np.abs(got.astype(np.float64) - W)
    share = float(np.where(b > 0, err / np.where(b > 0, b, 1.0), 0.0).max())      # (a component without terms: 0 within 0)
    print(f"{what}: {share:.3f} of the bound (max |W| {np.abs(W).max():.4e}, worst error {err.max():.3e})")
    assert np.abs(W).max() > 0 and (err <= b).all()
    return share


# ---------------------------------------------------------------------------------------------------- 1: the fixed-charge strain
@pytest.mark.parametrize("name,pset", SETS)
def test_fixed_charge_strain_against_float64_on_the_device_charges(gpu_engine_factory, name, pset):
    eng, (offsets, xyz, x, Q), cells, N, alpha, rows, out = _run(gpu_engine_factory, name, pset)
    q, gs, gs_fix = out[0], out[4], out[7]
    assert gs.shape == gs_fix.shape == (len(offsets) - 1, 3, 3) and gs.dtype == gs_fix.dtype == np.float32
    for b in range(len(offsets) - 1):
        a0, a1 = offsets[b], offsets[b + 1]
        W, s = _ref((name, pset, b), xyz[a0:a1], q[a0:a1], cells[b], alpha, rows[b])
        assert s["rec"].any() and s["k0"].any() and (pset != "a05" or not s["real"].any())
        _WORST["W"] = max(_WORST.get("W", 0.0), _check(f"{name} {pset}, cell {b} (n = {a1 - a0})", gs_fix[b], W, s))
    print(f"worst share so far: {_WORST['W']:.3f}")


def test_one_unit_charge_in_the_square_cell(gpu_engine_factory):
    """One atom with Q = 1 in the 6.5 A square at tol = 1e-10: gstrain_fix = diag(-E/2, -E/2, 0), E = -1/2 ke 3.9002649200 / L (E ~ 1 / L
    and the square's symmetry), within the bound of test 1 plus the truncation at that tol (tol ke beta, include/epnn.h); nothing
    depends on the one charge's position: gstrain_q = 0."""
    eng, batch, cells, N, alpha, rows, out = _run(gpu_engine_factory, "sq65-1-8", "fine")
    q, gs, gs_fix, gs_q = out[0], out[4], out[7], out[8]
    assert q[0] == 1.0 and not gs_q.any() and np.array_equal(gs, gs_fix)
    W, s = _ref(("sq65-1-8", "fine", 0), batch[1], q, cells[0], 0.0, rows[0])
    E1 = -0.5 * KE * 3.9002649200 / 6.5
    want = np.diag([-0.5 * E1, -0.5 * E1, 0.0])
    slack = _bound(want, s) + 1e-10 * KE * rows[0][0]
    assert (np.abs(gs_fix[0] - want) <= slack).all()


# ---------------------------------------------------------------------------------------------------- 2: composition bits
@pytest.mark.parametrize("name,pset", SETS)
def test_composition_bit_for_bit(gpu_engine_factory, name, pset):
    eng, batch, cells, N, alpha, rows, out = _run(gpu_engine_factory, name, pset)
    q, phi, E, F, gs, ffix, fq, gs_fix, gs_q = out
    q2, gxyz, gs2 = eng.charges_vjp_xyz(*batch, phi, N, cell=cells, strain=True)
    assert np.array_equal(q2, q) and np.array_equal(fq, -gxyz) and np.array_equal(gs_q, gs2)
    assert np.array_equal(gs, gs_fix + gs_q) and gs.dtype == np.float32
    for w in (gs, gs_fix, gs_q):
        assert np.array_equal(w, w.transpose(0, 2, 1))
    plain = eng.coulomb_xyz_slab(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, parts=True)
    for k, (got, want) in enumerate(zip((q, phi, E, F, ffix, fq), plain)):
        assert np.array_equal(got, want), k
    again = eng.coulomb_xyz_slab_strain(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, parts=True)
    assert all(np.array_equal(a, b) for a, b in zip(again, out))
    five = eng.coulomb_xyz_slab_strain(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows)
    assert len(five) == 5 and all(np.array_equal(a, b) for a, b in zip(five, (q, phi, E, F, gs)))


def test_the_model_method_and_the_rules_parameters(gpu_engine_factory):
    from epnn_amd import charge_gn
    eng, batch, cells, N, alpha, rows, out = _run(gpu_engine_factory, "sheared-17-24", "a0")
    model = charge_gn.make_model([32, 32], 48, 2, 9, 24)
    model.set_weights_dict(_weights())
    got = model.coulomb_xyz_slab_strain(*batch, cell=cells[0], ke=KE, parts=True)
    assert len(got) == 9 and all(np.array_equal(a, b) for a, b in zip(got, out))
    with pytest.raises(ValueError, match="exactly one zero"):
        eng.coulomb_xyz_slab_strain(*batch, N, box=np.float32([7, 7, 7]))


# ---------------------------------------------------------------------------------------------------- 3: end to end
@pytest.mark.parametrize("name,pset", [("sheared-17-24", "a0"), ("sheared-17-24", "near"), ("tilted-65-72", "a0")])
def test_total_strain_against_the_float64_reference(gpu_engine_factory, name, pset):
    """gstrain against slab_strain_forces64 (charges, the slab sum and the charges' part all float64), by the rule of the slab call's
    total forces: |W - W_ref| <= 2e-4 max(max |fix_ref|, max |q part_ref|) + kink, kink = max |ref(+TAU) - ref(-TAU)|; the bracket may
    be used only while it is at most 0.05 of that scale, asserted on the reference alone."""
    eng, batch, cells, N, alpha, rows, out = _run(gpu_engine_factory, name, pset)
    c, n, _ = name.split("-")
    xyz, x, Q, cell = _system(c, int(n), int(n))
    w = _weights()
    tot, fix, gq = slab_strain_forces64(xyz, x, Q, cell, w, N, KE, alpha, rows[0])
    lo = slab_strain_forces64(xyz, x, Q, cell, w, N, KE, alpha, rows[0], kink_shift=+TAU)[0]
    hi = slab_strain_forces64(xyz, x, Q, cell, w, N, KE, alpha, rows[0], kink_shift=-TAU)[0]
    kink, scale = np.abs(lo - hi).max(), max(np.abs(fix).max(), np.abs(gq).max())
    err = np.abs(out[4][0] - tot).max()
    print(f"{name} {pset}: gstrain {err:.3e} of {scale:.3e} (|fix| {np.abs(fix).max():.3e}, |q part| {np.abs(gq).max():.3e}, kink {kink:.3e})")
    assert scale > 0 and kink <= 0.05 * scale
    assert err <= 2e-4 * scale + kink


# ---------------------------------------------------------------------------------------------------- 4: invariants
def _slack(W, s, other_W, other_s, q, other_q):
    """Two runs' bounds, and what a difference of the charges may move: W is quadratic in q."""
    dq = np.abs(q - other_q).max() / np.abs(q).max()
    return _bound(W, s) + _bound(other_W, other_s) + (2 * dq + dq * dq) * (s["real"] + s["rec"] + s["k0"])


def test_a_cell_alone_has_the_bits_it_has_in_the_batch(gpu_engine_factory):
    eng, (offsets, xyz, x, Q), cells, N, alpha, rows, out = _run(gpu_engine_factory, "batch", "a0")
    for b in range(len(offsets) - 1):
        a0, a1 = offsets[b], offsets[b + 1]
        alone = eng.coulomb_xyz_slab_strain(np.int32([0, a1 - a0]), xyz[a0:a1], x[a0:a1], Q[b:b + 1], N, cell=cells[b], ke=KE, alpha=alpha,
                                            ewald=rows[b], parts=True)
        want = [o[b:b + 1] if k in (2, 4, 7, 8) else o[a0:a1] for k, o in enumerate(out)]
        for k, (got, w) in enumerate(zip(alone, want)):
            assert np.array_equal(got, w), (b, k)


@pytest.mark.parametrize("pset", ["a0", "a05"])
def test_the_open_row_at_another_place_permutes_the_strain(gpu_engine_factory, pset):
    """The sheared slab with its axes renamed cyclically, coordinates, rows and the rows' entries alike: the open row moves from
    place 2 to 0 and to 1, and W'[a][b] = W[p[a]][p[b]] within the two runs' bounds."""
    eng, (offsets, xyz, x, Q), cells, N, alpha, rows, out = _run(gpu_engine_factory, "sheared-17-24", pset)
    W, s = _ref(("sheared-17-24", pset, 0), xyz, out[0], cells[0], alpha, rows[0])
    for p in ([1, 2, 0], [2, 0, 1]):
        cell_p, xyz_p = np.ascontiguousarray(cells[0][p][:, p]), np.ascontiguousarray(xyz[:, p])
        row_p = np.concatenate([rows[0][:3], rows[0][3:][p]])
        assert not cell_p[p.index(2)].any()
        got = eng.coulomb_xyz_slab_strain(offsets, xyz_p, x, Q, N, cell=cell_p, ke=KE, alpha=alpha, ewald=row_p, parts=True)
        Wp, sp = slab_strain64(xyz_p, got[0], cell_p, KE, alpha, row_p[0], row_p[1], row_p[2], row_p[3:])
        _check(f"open row at {p.index(2)}", got[7][0], Wp, sp)
        back = {k: v[np.ix_(np.argsort(p), np.argsort(p))] for k, v in sp.items()}
        assert (np.abs(got[7][0][np.ix_(np.argsort(p), np.argsort(p))] - out[7][0])
                <= _slack(W, s, Wp[np.ix_(np.argsort(p), np.argsort(p))], back, out[0], got[0])).all()


@pytest.mark.parametrize("pset", ["a0", "near"])
def test_a_shift_of_all_atoms_leaves_the_fixed_charge_strain(gpu_engine_factory, pset):
    """Every cell of the batch moved by 3/8 a - 5/8 b in its plane and by 2.5 A along its normal, on a 2^-10 A grid."""
    eng, (offsets, xyz, x, Q), cells, N, alpha, rows, out = _run(gpu_engine_factory, "batch", pset)
    grid = np.round(xyz.astype(np.float64) * 1024) / 1024
    plane, up = grid.copy(), grid.copy()
    for b in range(len(offsets) - 1):
        a, _, per, _, _, nhat = slab_geometry64(cells[b])
        plane[offsets[b]:offsets[b + 1]] += np.round((0.375 * a[per[0]] - 0.625 * a[per[1]]) * 1024) / 1024
        up[offsets[b]:offsets[b + 1]] += np.round(2.5 * nhat * 1024) / 1024
    base, moved, lifted = (eng.coulomb_xyz_slab_strain(offsets, r.astype(np.float32), x, Q, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, parts=True)
                           for r in (grid, plane, up))
    for b in range(len(offsets) - 1):
        a0, a1 = offsets[b], offsets[b + 1]
        W, s = slab_strain64(grid[a0:a1].astype(np.float32), base[0][a0:a1], cells[b], KE, alpha, rows[b][0], rows[b][1], rows[b][2], rows[b][3:])
        _check(f"batch {pset} cell {b} on the grid", base[7][b], W, s)
        for what, run in (("in the plane", moved), ("along nhat", lifted)):
            assert (np.abs(run[7][b] - base[7][b]) <= _slack(W, s, W, s, base[0][a0:a1], run[0][a0:a1])).all(), (b, what)


# ---------------------------------------------------------------------------------------------------- 5: exclusions
def test_exclusions(gpu_engine_factory):
    from epnn_amd import engine
    eng = _engine(gpu_engine_factory)
    xyz, x, Q, bonds = _water_slab()
    cell = CELLS["sq65"]
    off, Qa = np.int32([0, 9]), np.float32([Q])
    pairs, _ = engine.bonded_exclusions(bonds, 9)
    mixed = np.float32([0.0, 0.5, 0.8333] * 3)
    for alpha in (0.0, 0.5):
        rows = _rows(eng, cell[None], alpha)
        plain = eng.coulomb_xyz_slab_strain(off, xyz, x, Qa, 16, cell=cell, ke=KE, alpha=alpha, ewald=rows, parts=True)
        for ex in ((np.zeros((0, 2), np.int32), np.zeros(0, np.float32)), (pairs, 1.0)):
            same = eng.coulomb_xyz_slab_strain(off, xyz, x, Qa, 16, cell=cell, ke=KE, alpha=alpha, ewald=rows, parts=True, exclusions=ex)
            assert all(np.array_equal(a, b) for a, b in zip(same, plain))
        out = eng.coulomb_xyz_slab_strain(off, xyz, x, Qa, 16, cell=cell, ke=KE, alpha=alpha, ewald=rows, parts=True, exclusions=(pairs, mixed))
        shuffled = eng.coulomb_xyz_slab_strain(off, xyz, x, Qa, 16, cell=cell, ke=KE, alpha=alpha, ewald=rows, parts=True,
                                               exclusions=xref.shuffled(pairs, mixed))
        assert all(np.array_equal(a, b) for a, b in zip(shuffled, out))
        with_list = eng.coulomb_xyz_slab(off, xyz, x, Qa, 16, cell=cell, ke=KE, alpha=alpha, ewald=rows, parts=True, exclusions=(pairs, mixed))
        for k, (got, want) in enumerate(zip((out[0], out[1], out[2], out[3], out[5], out[6]), with_list)):
            assert np.array_equal(got, want), k
        assert np.array_equal(out[0], plain[0]) and not np.array_equal(out[7], plain[7])
        W, s = slab_strain64(xyz, out[0], cell, KE, alpha, rows[0][0], rows[0][1], rows[0][2], rows[0][3:], (pairs, mixed))
        assert s["excl"].any()
        _check(f"water slab with bonded exclusions, alpha {alpha}", out[7][0], W, s)
        _, _, gs2 = eng.charges_vjp_xyz(off, xyz, x, Qa, out[1], 16, cell=cell, strain=True)
        assert np.array_equal(out[8], gs2) and np.array_equal(out[4], out[7] + out[8])


# ---------------------------------------------------------------------------------------------------- 6: refusals
def test_refusals_leave_the_handle_usable(gpu_engine_factory):
    from epnn_amd._lib import EpnnError, fptr, iptr
    eng, batch, cells, N, alpha, rows, first = _run(gpu_engine_factory, "batch", "a0")
    offsets, xyz, x, Q = batch

    def call(**kw):
        args = dict(cell=cells, ke=KE, alpha=0.0, ewald=rows, parts=True)
        args.update(kw)
        return eng.coulomb_xyz_slab_strain(*batch, N, **args)

    def still_fine():
        assert all(np.array_equal(a, b) for a, b in zip(call(), first))

    # gstrain_out is required: the C entry with NULL in its place (the other outputs given)
    A, B = len(xyz), len(offsets) - 1
    q, phi, E, F = np.empty(A, np.float32), np.empty(A, np.float32), np.empty(B, np.float64), np.empty((A, 3), np.float32)
    rc = eng.lib.epnn_coulomb_xyz_slab_strain(eng.h, B, N, iptr(offsets), fptr(xyz), fptr(x), fptr(Q), fptr(np.ascontiguousarray(cells)),
                                              rows.ctypes.data_as(C.POINTER(C.c_double)), KE, 0.0, 0, None, None, None, fptr(q), fptr(phi),
                                              E.ctypes.data_as(C.POINTER(C.c_double)), fptr(F), None, None, None, None, None)
    assert rc != 0 and "epnn_coulomb_xyz_slab_strain: null argument" in eng.lib.epnn_last_error().decode(errors="replace")
    still_fine()
    cube, wire, thin = cells.copy(), cells.copy(), cells.copy()
    cube[0, 2, 2] = 6.5
    wire[0, 1] = 0
    thin[0] = np.diag(np.float32([5.5, 6.5, 0]))
    for kw, match in (({"cell": cube}, "use epnn_coulomb_xyz_cell"), ({"cell": cube, "ewald": None}, "use epnn_coulomb_xyz_cell"),
                      ({"cell": wire}, "not built"), ({"cell": wire, "ewald": None}, "not built"), ({"cell": thin}, "below twice the cutoff"),
                      ({"alpha": -1.0}, "alpha must be finite"), ({"ke": float("inf")}, "ke must be finite"),
                      ({"ewald": None, "tol": 0.0}, "tol must be finite")):
        with pytest.raises(EpnnError, match="epnn_coulomb_xyz_slab_strain|epnn_ewald_slab_params") as info:
            call(**kw)
        assert match in str(info.value)
        still_fine()
    for b, col, value, match in ((0, 1, 3.3, "rc"), (0, 1, 0.0, "rc = 0"), (0, 0, 0.0, "beta"), (0, 3, rows[0, 3] - 1, "not consistent"),
                                 (0, 5, 1.0, "is open"), (1, 3, 2.0, "is open"), (0, 4, 40000.0, "cap")):
        bad = rows.copy()
        bad[b, col] = value
        with pytest.raises(EpnnError, match=match):
            call(ewald=bad)
        still_fine()
    with pytest.raises(ValueError, match="cell= or box="):
        eng.coulomb_xyz_slab_strain(*batch, N)
    with pytest.raises(EpnnError, match="does not fit N=12"):
        eng.coulomb_xyz_slab_strain(*batch, 12, cell=cells, ewald=rows)
    still_fine()
    # two atoms that coincide through an image: with the sweep (alpha = 0) and without it (beta == alpha)
    twin = xyz.copy()
    twin[2] = np.round(twin[2] * 1024) / 1024
    twin[5] = twin[2] + cells[0][0] - cells[0][1]
    for kw in ({}, {"alpha": 0.5, "ewald": _rows(eng, cells, 0.5)}):
        with pytest.raises(EpnnError, match="coincide"):
            eng.coulomb_xyz_slab_strain(offsets, twin, x, Q, N, cell=cells, **{"ewald": rows, **kw})
        still_fine()
    far = eng.coulomb_xyz_slab_strain  # a listed pair beyond half the width, by name
    wx, wxx, wQ, _ = _water_slab()
    wx = wx.copy()
    wx[0], wx[3] = [0.2, 0.2, 0.3], [3.2, 3.3, 0.3]
    with pytest.raises(EpnnError, match="beyond half the smallest perpendicular width"):
        far(np.int32([0, 9]), wx, wxx, np.float32([wQ]), 16, cell=CELLS["sq65"], ke=KE, exclusions=(np.int32([[0, 3]]), 0.0))
    still_fine()


# ---------------------------------------------------------------------------------------------------- 7: scratch
@pytest.mark.parametrize("name,ctasks", [("sq14-129-136", 6), ("batch", 1)])
def test_scratch_follows_the_formula(gpu_engine_factory, name, ctasks):
    """epnn_last_stats against the header's formula: the plain slab call's (test_gpu_coulomb_slab.py) plus 48 A cpieces + 48 A + 36 B;
    never below it, above it by less than 256 bytes for each of the 44 buffers (and the 16 of the staged parameters' rounding).
    ctasks: 3 blocks x 2 pieces; the four cells of the batch in one wavefront."""
    eng, batch, cells, N, alpha, rows, out = _run(gpu_engine_factory, name, "a0")
    eng.coulomb_xyz_slab_strain(*batch, N, cell=cells, ke=KE, ewald=rows)
    st = eng.last_stats()
    ns = tuple(int(n) for n in np.diff(batch[0]))
    A, B, cpieces = sum(ns), len(ns), max(_cl_pieces(n) for n in ns)
    slots = sum(_listed_slots(c, r) for c, r in zip(cells, rows))
    want = _formula(ns, 9, 2, int(st[0]), ctasks, slots) + 48 * A * cpieces + 48 * A + 36 * B
    eng.coulomb_xyz_slab(*batch, N, cell=cells, ke=KE, ewald=rows)
    plain = int(eng.last_stats()[2])
    print(f"{name}: {st[0]} pairs, {slots} slots, {st[2]} bytes, formula {want}, the plain call {plain}")
    assert st[0] > 0 and st[1] == 0
    assert want <= int(st[2]) < want + 44 * 256 + 16
    assert plain < int(st[2])
