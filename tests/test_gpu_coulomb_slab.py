"""Electrostatics of the predicted charges in slab cells (epnn_coulomb_xyz_slab, Engine.coulomb_xyz_slab) on the GPU: the fixed-charge
parts against the float64 two-dimensional Ewald sum on the device's own charges at the parameters the call ran at, the composition with
the pair-list gradient call bit for bit, the totals against the full float64 reference, invariants, exclusions, refusals and scratch.
GPU only.

Measured worst shares of the bounds below (MI355X, the 50 cases of test 1, which prints them): phi 0.036 (17 atoms in the sheared cell,
beta == alpha), ffix 0.031 (the 9-atom cell of the batch, beta == alpha), E 0.025 (the lone atom, the near set).  The bounds count
worst-case roundings per term; the errors of a sum's terms do not add up in phase."""
import math

import numpy as np
import pytest

import cell_ref
import coulomb_excl_ref as xref
from conftest import random_weights
from slab_ref import slab64, slab_forces64, slab_geometry64, slab_params64
from test_gpu_grad_large import TAU, _features

pytestmark = pytest.mark.gpu

KE = 14.3996454784255
U = 2.0 ** -24
BOUND = 2e-6          # real-space terms and the listed pairs' correction: the bound of the sweep that runs unchanged (test_gpu_coulomb_cell.py)
# Reciprocal terms, counted in k_sl_sweep as written, in units of 2^-24 of a term's scale w |q_j| [F+ + F-], w = 2 pi / (A k) (the
# cosine and sine count as 1); Fa, Fb: the two of F+- (epnn_ewald_slab.hip.h), 1 ulp of a result up to 2 units relative:
#   the phase 2 pi frac(m0 f0 + m1 f1): float64 up to frac, rounded to float32 (|frac| <= 1/2: pi), the float32 2 pi (1.5) and the
#       product (|angle| <= pi: pi); sincosf, 2 ulp of a value below 1 (2)                                                           9.8
#   Fa = eg erfcxf(u + beta |z|): eg = exp(-beta^2 z^2) rounded from float64 (1); the argument rounded from float64 (1) at a
#       sensitivity |x erfcx'(x) / erfcx(x)| <= 1; erfcxf's 4 ulp (8); the product (1)                                              11
#   Fb, where u >= beta |z|: the same (the argument is the float64 difference, rounded once: no cancellation reaches it)             11
#   Fb otherwise = 2 E - eg erfcxf(beta |z| - u), E = expf(-xh) (1 - xl) with the float64 exponent split exactly into xh + xl:
#       expf's 1 ulp (2), 1 - xl (1), the product (1) on 2 E; 11 on the second term, which is at most E <= Fb; the difference (1):
#       (2 * 4 + 11) E + Fb <= 20 Fb                                                                                                 20
#   Fs = Fa + Fb, Fd = +-(Fa - Fb): 20 on (Fa + Fb) and the sum's rounding (1)                                                       21
#   phi: w with exp(-u^2) folded in, rounded from float64 (1); (w q_j) cos Fs: three products (3); the cosine 9.8; Fs 21             34.8
#   ffix, a component along a unit vector e: the in-plane part (w q_j) sin Fs k_e and the part along nhat (wk q_j) cos Fd n_e, wk
#       rounded from float64.  The absolute errors of sine and cosine weigh |khat . e| + |nhat . e| <= sqrt(2) (13.9); the relative
#       ones, on |sin| |khat . e| + |cos| |nhat . e| <= 1: w or wk (1), Fs or Fd (21), three products (3), the float32 k component
#       and its product (2).  nhat is applied in float64.                                                                            40.9
# The k = 0 terms, in units of 2^-24 of (2 sqrt(pi) / A) |q_j| [exp(-beta^2 z^2) / beta + sqrt(pi) |z| erf(beta |z|)] (both terms >= 0):
#   eg / beta: eg (1), the float32 1 / beta (1), the product (1): 3;  sqrt(pi) |z| erff(beta |z|): |z| and beta |z| rounded from float64
#       (1 + 1, erf's sensitivity <= 1), erff's 4 ulp (8), the float32 sqrt(pi) and two products (3): 13;  the larger of the two (13),
#       their sum (1), the float32 weight (1) and the product with q_j (1)                                                           16
#   ffix: (2 pi / A) q_j erff: 1 + 8 for the erf, the float32 weight (1), two products (2)                                            12
# The sums over j and k are float64 (a float64 add of a float32 term: 2^-53 of the running sum, nothing here).
C_REC = 41
C_0 = 16
BOUND_REC = C_REC * U
BOUND_K0 = C_0 * U
REST = 2 * U          # the self term is float64: the rounding of the float32 output
TILTED = np.float32([[0, 0, 0], [6.8, 1.0, 1.5], [-0.5, 6.0, 3.5]])             # the open row first; widths 6.95, 6.88
CELLS = {"sq65": np.diag(np.float32([6.5, 6.5, 0])), "sheared": np.float32([[7, 0, 0], [2, 6.9, 0], [0, 0, 0]]), "tilted": TILTED,
         "openy": np.float32([[7, 0, 0], [0, 0, 0], [2, 0, 6.9]]), "sq14": np.diag(np.float32([14, 14, 0]))}
# (cell, n, N): every boundary of the packing and the pieces (epnn_coulomb.hip.h: CL_BLOCK 64, CL_MINPIECE 128)
SINGLE = [("sq65", 1, 8), ("sq65", 2, 8), ("sheared", 17, 24), ("tilted", 63, 64), ("sheared", 64, 64), ("tilted", 65, 72),
          ("sq14", 128, 128), ("sq14", 129, 136), ("sq14", 257, 264)]
CASES = [f"{c}-{n}-{N}" for c, n, N in SINGLE] + ["batch"]
BATCH = [("sq65", 20), ("tilted", 1), ("openy", 9), ("sq14", 30)]               # 60 atoms: one wavefront, three different open rows
# (alpha, beta or None for the rule's, tol): near: a sweep whose two erf almost cancel; fine: a second, larger k box
PSETS = {"a0": (0.0, None, 1e-6), "a05": (0.5, None, 1e-6), "a2": (2.0, None, 1e-6), "near": (0.5, 0.45, 1e-6), "fine": (0.0, None, 1e-10)}


def _weights():
    return random_weights(9, 2, seed=5, scale=0.6)


def _place(rng, n, cell, thick, min_sep=0.9):
    """n atoms uniform over the cell's two periodic rows and `thick` along its normal, no two images closer than min_sep."""
    a, _, per, _, _, nhat = slab_geometry64(np.asarray(cell, dtype=np.float32))
    pts = []
    while len(pts) < n:
        f = rng.uniform(0, 1, 3)
        p = f[0] * a[per[0]] + f[1] * a[per[1]] + thick * f[2] * nhat
        if all(np.sum(cell_ref.mic(p - o, cell) ** 2) >= min_sep ** 2 for o in pts):
            pts.append(p)
    return np.array(pts, dtype=np.float32)


def _system(cell_name, n, seed):
    rng = np.random.default_rng(seed)
    xyz = _place(rng, n, CELLS[cell_name], 4.0 + 2.0 * rng.uniform())
    x, Q = _features(rng, n, 9)
    return xyz, x, (np.float32(1.0) if n == 1 else Q), CELLS[cell_name]


def _batch(systems):
    offsets = np.zeros(len(systems) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum([s[0].shape[0] for s in systems])
    return (offsets, np.concatenate([s[0] for s in systems]), np.concatenate([s[1] for s in systems]),
            np.array([s[2] for s in systems], dtype=np.float32)), np.stack([s[3] for s in systems])


_CASES, _ENGINE, _RUNS, _REF64, _WORST = {}, [], {}, {}, {}


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
    rows = np.stack([eng.ewald_slab_params(c, alpha, tol) for c in cells])
    if beta is not None:
        s = math.sqrt(-math.log(tol))
        for b, c in enumerate(cells):
            a = c.astype(np.float64)
            kc = 2 * beta * s
            rows[b] = [beta, 0.5 * cell_ref.widths(c).min() * (1 - 1e-12), kc, *np.ceil(kc * np.sqrt((a * a).sum(1)) / (2 * math.pi))]
    return rows


def _run(factory, name, pset):
    """The call with parts, once per case: (engine, batch, cells, N, alpha, rows, (q, phi, E, F, ffix, fq))."""
    if (name, pset) not in _RUNS:
        systems, N = _case(name)
        eng = _engine(factory)
        batch, cells = _batch(systems)
        alpha, beta, tol = PSETS[pset]
        rows = _rows(eng, cells, alpha, tol, beta)
        for b, c in enumerate(cells):
            want = slab_params64(c, alpha, tol)
            assert beta is not None or (np.array_equal(rows[b][3:], want[3:]) and np.allclose(rows[b][:3], want[:3], rtol=1e-14, atol=0))
        if pset == "a05":
            assert (rows[:, 1] == 0).all() and (rows[:, 0] == 0.5).all()
        else:
            assert (rows[:, 1] > 0).all() and (alpha == 0 or (rows[:, 0] < alpha).all())
        out = eng.coulomb_xyz_slab(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, parts=True)
        _RUNS[name, pset] = (eng, batch, cells, N, alpha, rows, out)
    return _RUNS[name, pset]


def _ref(name, pset, b, xyz, q, cell, alpha, row):
    """slab64 of cell b of a run on the device's charges, computed once and shared."""
    if (name, pset, b) not in _REF64:
        _REF64[name, pset, b] = slab64(xyz, q, cell, KE, alpha, row[0], row[1], row[2], row[3:])
    return _REF64[name, pset, b]


def _bound(s, k=1.0):
    return k * (BOUND * s["real"] + BOUND_REC * s["rec"] + BOUND_K0 * s["k0"] + REST * s["rest"])


# ---------------------------------------------------------------------------------------------------- 1: the fixed-charge parts
def _check_fixed_parts(what, e, q, phi, Eb, ffix):
    """One cell's phi, ffix and E against the reference namespace e: each within BOUND of its absolute real-space terms plus BOUND_REC
    of its absolute reciprocal terms plus BOUND_K0 of its absolute k = 0 terms.  Returns the errors as shares of that."""
    bp, bf, bE = _bound(e.s_phi), _bound(e.s_ffix), _bound(e.s_E)
    ep, ef, eE = np.abs(phi - e.phi), np.abs(ffix - e.ffix).max(1), abs(Eb - e.E)
    with np.errstate(divide="ignore", invalid="ignore"):                      # (an atom of charge 0 has no force terms at all)
        shares = ((ep / bp).max(), np.where(bf > 0, ef / bf, 0.0).max(), eE / bE)
    print(f"{what} (n = {len(q)}): phi {shares[0]:.3f}, ffix {shares[1]:.3f}, E {shares[2]:.3f} of the bounds "
          f"(|phi| {np.abs(e.phi).max():.3e}, |ffix| {np.abs(e.ffix).max():.3e}, E {e.E:.6e})")
    assert np.abs(e.phi).max() > 0
    assert (ep <= bp).all() and (ef <= bf).all() and eE <= bE
    return shares


@pytest.mark.parametrize("pset", sorted(PSETS))
@pytest.mark.parametrize("name", CASES)
def test_fixed_charge_parts_against_float64_on_the_device_charges(gpu_engine_factory, name, pset):
    eng, (offsets, xyz, x, Q), cells, N, alpha, rows, (q, phi, E, F, ffix, fq) = _run(gpu_engine_factory, name, pset)
    assert E.dtype == np.float64 and E.shape == (len(offsets) - 1,) and F.shape == (len(q), 3)
    for b in range(len(offsets) - 1):
        a0, a1 = offsets[b], offsets[b + 1]
        e = _ref(name, pset, b, xyz[a0:a1], q[a0:a1], cells[b], alpha, rows[b])
        sh = _check_fixed_parts(f"{name} {pset}, cell {b}", e, q[a0:a1], phi[a0:a1], E[b], ffix[a0:a1])
        for k, v in zip(("phi", "ffix", "E"), sh):
            _WORST[k] = max(_WORST.get(k, 0.0), float(v))
    print(f"worst shares so far: phi {_WORST['phi']:.3f}, ffix {_WORST['ffix']:.3f}, E {_WORST['E']:.3f}")


def test_one_charge_gives_the_constant_of_the_square_lattice(gpu_engine_factory):
    """One atom with Q = 1 in the 6.5 A square, alpha = 0: phi L / (ke q) = -3.9002649, E half of it, within the device bound plus the
    truncation at tol = 1e-6 (tol ke beta |q|, include/epnn.h)."""
    eng, (offsets, xyz, x, Q), cells, N, alpha, rows, (q, phi, E, F, ffix, fq) = _run(gpu_engine_factory, "sq65-1-8", "a0")
    assert q[0] == 1.0 and Q[0] == 1.0
    e = _ref("sq65-1-8", "a0", 0, xyz, q, cells[0], 0.0, rows[0])
    slack = _bound(e.s_phi)[0] + 1e-6 * KE * rows[0][0]
    assert abs(phi[0] + 3.9002649 * KE / 6.5) <= slack and abs(E[0] + 0.5 * 3.9002649 * KE / 6.5) <= slack
    assert np.abs(ffix).max() <= _bound(e.s_ffix)[0] and not fq.any()


# ---------------------------------------------------------------------------------------------------- 3: composition bits
@pytest.mark.parametrize("pset", sorted(PSETS))
@pytest.mark.parametrize("name", CASES)
def test_composition_with_the_gradient_call_bit_for_bit(gpu_engine_factory, name, pset):
    eng, batch, cells, N, alpha, rows, (q, phi, E, F, ffix, fq) = _run(gpu_engine_factory, name, pset)
    q2, gxyz = eng.charges_vjp_xyz(*batch, phi, N, cell=cells)
    assert np.array_equal(q2, q) and np.array_equal(fq, -gxyz)
    assert np.array_equal(F, ffix + fq) and F.dtype == np.float32
    four = eng.coulomb_xyz_slab(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows)
    assert len(four) == 4
    for got, want in zip(four, (q, phi, E, F)):
        assert np.array_equal(got, want)


def test_default_parameters_are_the_rules_and_a_box_is_its_diagonal_cell(gpu_engine_factory):
    eng, batch, cells, N, alpha, rows, out = _run(gpu_engine_factory, "sq14-128-128", "a0")
    again = eng.coulomb_xyz_slab(*batch, N, box=np.float32([14, 14, 0]), ke=KE, parts=True)
    assert all(np.array_equal(a, b) for a, b in zip(again, out))
    assert np.array_equal(eng.ewald_slab_params(cells[0], 0.0, 1e-6), rows[0])
    for box in (np.float32([14, 14, 14]), np.float32([14, 0, 0])):
        with pytest.raises(ValueError, match="exactly one zero"):
            eng.coulomb_xyz_slab(*batch, N, box=box)


def test_the_model_method(gpu_engine_factory):
    from epnn_amd import charge_gn
    eng, batch, cells, N, alpha, rows, out = _run(gpu_engine_factory, "sheared-17-24", "a2")
    model = charge_gn.make_model([32, 32], 48, 2, 9, 24)
    model.set_weights_dict(_weights())
    got = model.coulomb_xyz_slab(*batch, cell=cells[0], ke=KE, alpha=2.0, parts=True)
    assert len(got) == 6 and all(np.array_equal(a, b) for a, b in zip(got, out))


# ---------------------------------------------------------------------------------------------------- 4: end to end
_TOTAL = {}


def _reference(cell_name, n, N, alpha, row):
    key = (cell_name, n, N, alpha)
    if key not in _TOTAL:
        xyz, x, Q, cell = _system(cell_name, n, n)
        w = _weights()
        mid = slab_forces64(xyz, x, Q, cell, w, N, KE, alpha, row)
        lo = slab_forces64(xyz, x, Q, cell, w, N, KE, alpha, row, kink_shift=+TAU)
        hi = slab_forces64(xyz, x, Q, cell, w, N, KE, alpha, row, kink_shift=-TAU)
        _TOTAL[key] = mid + (np.abs(lo[3] - hi[3]).max(),)
    return _TOTAL[key]


@pytest.mark.parametrize("name,pset", [("sheared-17-24", "a0"), ("sheared-17-24", "a2"), ("tilted-65-72", "a0"), ("tilted-65-72", "a2")])
def test_total_forces_against_the_float64_reference(gpu_engine_factory, name, pset):
    """F against slab_forces64 (charges, the slab sum and the charges' part all float64), the rule of test_gpu_coulomb_cell.py's total
    test: |F - F_ref| <= 2e-4 max(max |ffix_ref|, max |fq_ref|) + kink, kink = max |ref(+TAU) - ref(-TAU)|; the bracket may be used
    only while it is at most 0.05 of that scale, asserted on the reference alone."""
    eng, batch, cells, N, alpha, rows, (q, phi, E, F, ffix, fq) = _run(gpu_engine_factory, name, pset)
    c, n, _ = name.split("-")
    q64, phi64, E64, f64, ffix64, fq64, kink_f = _reference(c, int(n), N, alpha, rows[0])
    sf = max(np.abs(ffix64).max(), np.abs(fq64).max())
    ef = np.abs(F - f64).max()
    print(f"{name} {pset}: q {np.abs(q - q64).max():.3e}, phi {np.abs(phi - phi64).max():.3e} of {np.abs(phi64).max():.3e}, E {abs(E[0] - E64):.3e} "
          f"of {abs(E64):.3e}; F {ef:.3e} of {sf:.3e} (|fq| {np.abs(fq64).max():.3e}, kink {kink_f:.3e})")
    assert sf > 0 and kink_f <= 0.05 * sf
    assert np.abs(q - q64).max() <= 2e-4
    assert ef <= 2e-4 * sf + kink_f


# ---------------------------------------------------------------------------------------------------- 5: invariants
@pytest.mark.parametrize("pset", ["a0", "a2"])
def test_invariants(gpu_engine_factory, pset):
    eng, batch, cells, N, alpha, rows, out = _run(gpu_engine_factory, "batch", pset)
    offsets, xyz, x, Q = batch
    q, phi, E, F, ffix, fq = out
    again = eng.coulomb_xyz_slab(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, parts=True)
    assert all(np.array_equal(a, b) for a, b in zip(out, again))
    fine = eng.coulomb_xyz_slab(*batch, N, cell=cells, ke=KE, alpha=alpha, ewald=_rows(eng, cells, alpha, tol=1e-10), parts=True)
    # every cell moved by a lattice vector of its own (3 a - 2 b), and by 1024 A along its normal: coordinates on a 2^-10 A grid move exactly
    grid = np.round(xyz.astype(np.float64) * 1024) / 1024
    lat, up = grid.copy(), grid.copy()
    for b in range(len(offsets) - 1):
        a, _, per, _, _, nhat = slab_geometry64(cells[b])
        lat[offsets[b]:offsets[b + 1]] += 3 * a[per[0]] - 2 * a[per[1]]
        up[offsets[b]:offsets[b + 1]] += 1024.0 * nhat
    base, moved, lifted = (eng.coulomb_xyz_slab(offsets, r.astype(np.float32), x, Q, N, cell=cells, ke=KE, alpha=alpha, ewald=rows, parts=True)
                           for r in (grid, lat, up))
    for b in range(len(offsets) - 1):
        a0, a1 = offsets[b], offsets[b + 1]
        e = _ref("batch", pset, b, xyz[a0:a1], q[a0:a1], cells[b], alpha, rows[b])
        bp, bf, bE = _bound(e.s_phi), _bound(e.s_ffix), _bound(e.s_E)
        # sum_i ffix_i = 0 to the bound on the cell's summed absolute terms
        assert np.abs(ffix[a0:a1].sum(0, dtype=np.float64)).max() <= bf.sum()
        # shifted coordinates: the fixed-charge parts of each run agree with the reference on that run's own float32 coordinates and
        # charges within the bound of test 1 (the reference is periodic by construction; the lift rounds a coordinate at 1024 A to 2^-14 A)
        for what, run, r in (("base", base, grid), ("lattice shift", moved, lat), ("lift", lifted, up)):
            r32 = r[a0:a1].astype(np.float32)
            ref = slab64(r32, run[0][a0:a1], cells[b], KE, alpha, rows[b][0], rows[b][1], rows[b][2], rows[b][3:])
            _check_fixed_parts(f"batch {pset} cell {b} {what}", ref, run[0][a0:a1], run[1][a0:a1], run[2][b], run[4][a0:a1])
        # tol = 1e-6 against tol = 1e-10: the truncation scales of include/epnn.h at 1e-6, and the bounds of the two runs
        beta, Qa, qm = rows[b][0], np.abs(q[a0:a1]).sum(), np.abs(q[a0:a1]).max()
        assert np.abs(fine[0][a0:a1] - q[a0:a1]).max() == 0
        assert np.abs(fine[1][a0:a1] - phi[a0:a1]).max() <= 1e-6 * KE * beta * Qa + 2 * bp.max()
        assert abs(fine[2][b] - E[b]) <= 1e-6 * 0.5 * KE * beta * Qa * Qa + 2 * bE
        assert np.abs(fine[4][a0:a1] - ffix[a0:a1]).max() <= 1e-6 * KE * beta * beta * Qa * qm + 2 * bf.max()
        # alone at the same N: the same bits
        alone = eng.coulomb_xyz_slab(np.int32([0, a1 - a0]), xyz[a0:a1], x[a0:a1], Q[b:b + 1], N, cell=cells[b], ke=KE, alpha=alpha, ewald=rows[b],
                                     parts=True)
        want = (q[a0:a1], phi[a0:a1], E[b:b + 1], F[a0:a1], ffix[a0:a1], fq[a0:a1])
        for k, (got, w) in enumerate(zip(alone, want)):
            assert np.array_equal(got, w), (b, k)


def test_a_mirror_image_in_the_plane_gives_mirrored_forces(gpu_engine_factory):
    """The sheared slab mirrored in its own plane (z -> -z; the cell is unchanged): the charges stay, within the float32 grade of a
    forward, and phi, ffix and E of each run agree with the reference on its own charges, whose forces are mirrored exactly."""
    eng, (offsets, xyz, x, Q), cells, N, alpha, rows, (q, phi, E, F, ffix, fq) = _run(gpu_engine_factory, "sheared-17-24", "a0")
    flip = np.float32([1, 1, -1])
    qm, phim, Em, Fm, ffixm, fqm = eng.coulomb_xyz_slab(offsets, xyz * flip, x, Q, N, cell=cells, ke=KE, ewald=rows, parts=True)
    assert np.abs(qm - q).max() <= 2e-6
    e = _ref("sheared-17-24", "a0", 0, xyz, q, cells[0], 0.0, rows[0])
    em = slab64(xyz * flip, q, cells[0], KE, 0.0, rows[0][0], rows[0][1], rows[0][2], rows[0][3:])
    assert np.abs(em.ffix - e.ffix * flip).max() <= 1e-12 * np.abs(e.ffix).max() and abs(em.E - e.E) <= 1e-12 * abs(e.E)
    mine = slab64(xyz * flip, qm, cells[0], KE, 0.0, rows[0][0], rows[0][1], rows[0][2], rows[0][3:])
    _check_fixed_parts("mirrored", mine, qm, phim, Em[0], ffixm)
    # and directly: mirrored fixed-charge forces within the two runs' bounds plus the charges' difference times the terms' scale
    slack = 2 * _bound(e.s_ffix) + 2 * np.abs(qm - q).max() / np.abs(q).max() * (e.s_ffix["real"] + e.s_ffix["rec"] + e.s_ffix["k0"])
    assert (np.abs(ffixm - ffix * flip).max(1) <= slack).all()


# ---------------------------------------------------------------------------------------------------- 6: exclusions
def _water_slab():
    """Three water-like molecules in the 6.5 A square slab: O H H each, bonded O-H; 9 atoms."""
    O = np.float64([[1.0, 1.2, 0.3], [4.1, 2.0, 1.9], [2.2, 4.9, 3.4]])
    rng = np.random.default_rng(9)
    xyz, bonds = [], []
    for k, o in enumerate(O):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        v = np.cross(u, rng.normal(size=3))
        v /= np.linalg.norm(v)
        h1 = o + 0.96 * u
        h2 = o + 0.96 * (math.cos(1.824) * u + math.sin(1.824) * v)
        xyz += [o, h1, h2]
        bonds += [(3 * k, 3 * k + 1), (3 * k, 3 * k + 2)]
    x = np.zeros((9, 9), dtype=np.float32)
    for i in range(9):
        x[i, 0], x[i, 4 if i % 3 == 0 else 1] = (8, 1) if i % 3 == 0 else (1, 1)
    return np.array(xyz, dtype=np.float32), x, np.float32(0), np.int32(bonds)


def test_exclusions(gpu_engine_factory):
    from epnn_amd import engine
    from epnn_amd._lib import EpnnError
    eng = _engine(gpu_engine_factory)
    xyz, x, Q, bonds = _water_slab()
    cell = CELLS["sq65"]
    off, Qa = np.int32([0, 9]), np.float32([Q])
    rows = _rows(eng, cell[None], 0.0)
    plain = eng.coulomb_xyz_slab(off, xyz, x, Qa, 16, cell=cell, ke=KE, ewald=rows, parts=True)
    pairs, scale = engine.bonded_exclusions(bonds, 9)
    assert len(pairs) == 9 and (scale == 0).all()                                 # O-H twice and H-H once per molecule, all excluded
    # an empty list and a list of factors 1: the bits of the call without a list
    for ex in ((np.zeros((0, 2), np.int32), np.zeros(0, np.float32)), (pairs, 1.0)):
        same = eng.coulomb_xyz_slab(off, xyz, x, Qa, 16, cell=cell, ke=KE, ewald=rows, parts=True, exclusions=ex)
        assert all(np.array_equal(a, b) for a, b in zip(same, plain))
    mixed = np.float32([0.0, 0.5, 0.8333] * 3)
    out = eng.coulomb_xyz_slab(off, xyz, x, Qa, 16, cell=cell, ke=KE, ewald=rows, parts=True, exclusions=(pairs, mixed))
    shuffled = eng.coulomb_xyz_slab(off, xyz, x, Qa, 16, cell=cell, ke=KE, ewald=rows, parts=True, exclusions=xref.shuffled(pairs, mixed))
    assert all(np.array_equal(a, b) for a, b in zip(shuffled, out))
    q, phi, E, F, ffix, fq = out
    assert np.array_equal(q, plain[0]) and not np.array_equal(phi, plain[1])
    # against slab64 plus the listed pairs' correction, whose absolute terms count at the sweep's bound
    e = slab64(xyz, q, cell, KE, 0.0, rows[0][0], rows[0][1], rows[0][2], rows[0][3:])
    c = xref.excl_correction64(xyz, q, cell, KE, 0.0, pairs, mixed)
    e.phi = e.phi + c.dphi
    e.E = 0.5 * float(q.astype(np.float64) @ e.phi)
    e.ffix = e.ffix + c.dffix
    e.s_phi["real"] = e.s_phi["real"] + c.s_phi
    e.s_ffix["real"] = e.s_ffix["real"] + c.s_ffix
    e.s_E["real"] = e.s_E["real"] + c.s_E
    _check_fixed_parts("water slab with bonded exclusions", e, q, phi, E[0], ffix)
    q2, gxyz = eng.charges_vjp_xyz(off, xyz, x, Qa, phi, 16, cell=cell)
    assert np.array_equal(q2, q) and np.array_equal(fq, -gxyz) and np.array_equal(F, ffix + fq)
    # a pair beyond half the width is refused by name, and the handle stays usable
    far = xyz.copy()
    far[0] = [0.2, 0.2, 0.3]
    far[3] = [3.2, 3.3, 0.3]
    with pytest.raises(EpnnError, match="beyond half the smallest perpendicular width"):
        eng.coulomb_xyz_slab(off, far, x, Qa, 16, cell=cell, ke=KE, ewald=rows, exclusions=(np.int32([[0, 3]]), 0.0))
    again = eng.coulomb_xyz_slab(off, xyz, x, Qa, 16, cell=cell, ke=KE, ewald=rows, parts=True)
    assert all(np.array_equal(a, b) for a, b in zip(again, plain))


# ---------------------------------------------------------------------------------------------------- 7: refusals
def test_refusals_leave_the_handle_usable(gpu_engine_factory):
    from epnn_amd._lib import EpnnError
    eng, batch, cells, N, alpha, rows, first = _run(gpu_engine_factory, "batch", "a0")
    offsets, xyz, x, Q = batch

    def call(**kw):
        args = dict(cell=cells, ke=KE, alpha=0.0, ewald=rows, parts=True)
        args.update(kw)
        return eng.coulomb_xyz_slab(*batch, N, **args)

    def still_fine():
        assert all(np.array_equal(a, b) for a, b in zip(call(), first))

    cube, wire, thin = cells.copy(), cells.copy(), cells.copy()
    cube[0, 2, 2] = 6.5                                                       # three periodic rows
    wire[0, 1] = 0                                                            # one periodic row
    thin[0] = np.diag(np.float32([5.5, 6.5, 0]))                              # a width below twice the cutoff
    for kw, match in (({"cell": cube}, "use epnn_coulomb_xyz_cell"), ({"cell": cube, "ewald": None}, "use epnn_coulomb_xyz_cell"),
                      ({"cell": wire}, "not built"), ({"cell": wire, "ewald": None}, "not built"), ({"cell": thin}, "below twice the cutoff"),
                      ({"alpha": -1.0}, "alpha must be finite"), ({"ke": float("inf")}, "ke must be finite"),
                      ({"ewald": None, "tol": 0.0}, "tol must be finite")):
        with pytest.raises(EpnnError, match=match):
            call(**kw)
        still_fine()
    # cell 0 is the 6.5 A square, open along z (M2 = 0); cell 1 is the tilted one, open row first
    for b, col, value, match in ((0, 1, 3.3, "rc"), (0, 1, -1.0, "rc"), (0, 1, 0.0, "rc = 0"), (0, 0, 0.0, "beta"), (0, 0, float("nan"), "not finite"),
                                 (0, 3, rows[0, 3] - 1, "not consistent"), (0, 4, 9.5, "not consistent"), (0, 5, 1.0, "is open"),
                                 (1, 3, 2.0, "is open"), (0, 4, 40000.0, "cap")):
        bad = rows.copy()
        bad[b, col] = value
        with pytest.raises(EpnnError, match=match):
            call(ewald=bad)
        still_fine()
    needle = cells.copy()
    needle[0] = np.diag(np.float32([6.5, 3e6, 0]))
    with pytest.raises(EpnnError, match="cap"):
        call(cell=needle, ewald=None)
    still_fine()
    with pytest.raises(ValueError, match="cell= or box="):
        eng.coulomb_xyz_slab(*batch, N)
    with pytest.raises(EpnnError, match="does not fit N=12"):
        eng.coulomb_xyz_slab(*batch, 12, cell=cells, ewald=rows)
    still_fine()
    # two atoms that coincide through an image: with the sweep (alpha = 0) and without it (beta == alpha)
    twin = xyz.copy()
    twin[2] = np.round(twin[2] * 1024) / 1024                                 # (on a 2^-10 A grid the lattice shift is exact in float32)
    twin[5] = twin[2] + cells[0][0] - cells[0][1]
    assert np.array_equal(twin[5].astype(np.float64) - twin[2], np.float64([6.5, -6.5, 0]))
    for kw in ({}, {"alpha": 0.5, "ewald": _rows(eng, cells, 0.5)}):
        with pytest.raises(EpnnError, match="coincide"):
            eng.coulomb_xyz_slab(offsets, twin, x, Q, N, cell=cells, **{"ewald": rows, **kw})
        still_fine()


# ---------------------------------------------------------------------------------------------------- 8: scratch
def _gl_pieces(n):
    return min(16, max(1, -(-2048 // -(-n // 16))))


def _cl_pieces(n):
    return 1 if n <= 64 else max(1, min(32, -(-n // 128), -(-2048 // -(-n // 64))))


def _formula(ns, nx, T, pairs, ctasks, slots):
    """include/epnn.h: epnn_coulomb_xyz's bytes = A (1344 + 4 nx + 324 T + 256 pieces + 32 cpieces) + 16 (gtasks + ctasks) +
    1116 max(pairs, 1) + 56 B + 8240, and the slab's on top: 88 A cpieces + 304 B + 56 slots"""
    A, B = sum(ns), len(ns)
    pieces, cpieces = max(_gl_pieces(n) for n in ns), max(_cl_pieces(n) for n in ns)
    gtasks = sum(-(-n // 16) * _gl_pieces(n) for n in ns)
    return (A * (1344 + 4 * nx + 324 * T + 256 * pieces + 32 * cpieces) + 16 * (gtasks + ctasks) + 1116 * max(pairs, 1) + 56 * B + 8240
            + 88 * A * cpieces + 304 * B + 56 * slots)


def _listed_slots(cell, row):
    _, g, per, _, _, _ = slab_geometry64(cell)
    m0, m1 = np.meshgrid(np.arange(-row[3 + per[0]], row[3 + per[0]] + 1), np.arange(0, row[3 + per[1]] + 1), indexing="ij")
    k = 2 * math.pi * np.linalg.norm(m0[..., None] * g[per[0]] + m1[..., None] * g[per[1]], axis=-1)
    return int(((k <= row[2]) & ((m1 > 0) | (m0 > 0))).sum())


@pytest.mark.parametrize("name,ctasks", [("sq14-257-264", 15), ("batch", 1)])
def test_scratch_follows_the_formula(gpu_engine_factory, name, ctasks):
    """epnn_last_stats against the header's formula: never below it, above it by less than 256 bytes for each of the 44 buffers (and the
    16 of the staged parameters' rounding).  ctasks: 5 blocks x 3 pieces; the four cells of the batch in one wavefront."""
    eng, batch, cells, N, alpha, rows, out = _run(gpu_engine_factory, name, "a0")
    eng.coulomb_xyz_slab(*batch, N, cell=cells, ke=KE, ewald=rows)
    st = eng.last_stats()
    ns = tuple(np.diff(batch[0]))
    slots = sum(_listed_slots(c, r) for c, r in zip(cells, rows))
    want = _formula(ns, 9, 2, int(st[0]), ctasks, slots)
    print(f"{name}: {st[0]} pairs, {slots} slots, {st[2]} bytes, formula {want}")
    assert st[0] > 0 and st[1] == 0 and slots >= 100 * len(ns)
    assert want <= int(st[2]) < want + 44 * 256 + 16
