"""Electrostatics of the predicted charges in one call (epnn_coulomb_xyz, Engine.coulomb_xyz) on the GPU: the fixed-charge parts
against float64 on the device's own charges, the composition with the pair-list gradient call bit for bit, the charges' part
against the full float64 reference, invariants, refusals and scratch. GPU only."""
import os

import numpy as np
import pytest

from conftest import random_weights
from coulomb_ref import coulomb64, coulomb_forces64
from test_gpu_grad_large import TAU, _batch, _lattice_molecule

pytestmark = pytest.mark.gpu

KE = 14.3996454784255
ALPHAS = [0.0, 0.5]
BOUND = 2e-6          # about ten float32 roundings per term (10 * 2^-24 = 6e-7) plus a few ulp of erff / expf; the sums are float64

# (n, N) of single lattice molecules.  Beside the sizes every build is held to, one on each side of the kernel's boundaries
# (epnn_coulomb.hip.h):
#   CL_BLOCK = 64       atoms of a task; up to 64 atoms a molecule is one packed task with one piece: 63, 64 | 65
#                       a further block of atoms: 128 | 129 and 192 | 193
#   CL_TILE = 64        partners staged at a time: a piece of 127 is a tile of 64 and one of 63, of 128 two full ones, and the
#                       two pieces of 129 are of 65 and 64 partners: a full tile and one partner more
#   CL_MINPIECE = 128   pieces of the partner range, ceil(n / 128) at these sizes: 1 piece up to 128 | 2 from 129, 2 up to 256 | 3 from 257
#   CL_MAXP, CL_WANT    limit the pieces from 4097 atoms on only; the 2220-atom protein runs 18 pieces of 124 (35 blocks)
#                       (4100 and 8250 atoms, the packing of small molecules and single pairs over alpha and D: test_gpu_coulomb_domain.py)
SIZES = [(1, 8), (2, 8), (17, 24), (63, 64), (64, 64), (65, 72), (129, 136),
         (127, 128), (128, 128), (192, 192), (193, 200), (256, 256), (257, 264)]
CASES = [f"{n}-{N}" for n, N in SIZES] + ["batch", "far", "protein"]
FAR = np.float32([1000.0, -2000.0, 500.0])


def _weights(golden=False):
    if golden:
        from epnn_amd import checkpoint
        return checkpoint.load_epnn_weights(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "models", "decay_model_weights"))
    return random_weights(9, 2, seed=5, scale=0.6)


_CASES, _ENGINES, _RUNS = {}, {}, {}


def _case(name):
    """(engine key, molecules, N)"""
    if name not in _CASES:
        if name == "batch":
            _CASES[name] = ("random", [_lattice_molecule(n, 9, seed=n) for n in (70, 1, 33, 120)], 128)
        elif name == "far":
            xyz, x, Q = _lattice_molecule(65, 9, seed=65)
            _CASES[name] = ("random", [(xyz + FAR, x, Q)], 72)
        elif name == "protein":
            from conftest import GOLDEN
            from oracle import epnn_oracle as orc
            xyz, x, Q = orc.parse_xyz(os.path.join(GOLDEN, "protein", "6qlp_capped.xyz"), 9)
            assert x.shape[0] == 2220
            _CASES[name] = ("protein", [(xyz.astype(np.float32), x.astype(np.float32), np.float32(Q))], 2220)
        else:
            n, N = (int(v) for v in name.split("-"))
            _CASES[name] = ("random", [_lattice_molecule(n, 9, seed=n)], N)
    return _CASES[name]


def _engine(factory, key):
    if key not in _ENGINES:
        w = _weights(golden=key == "protein")
        eng = factory(nx=9, T=len(w["msg"]))
        eng.set_weights(w)
        eng.set_option("grad_path", 2)
        _ENGINES[key] = eng
    return _ENGINES[key]


def _run(factory, name, alpha):
    """The call with parts=True, once per case: (engine, (offsets, xyz, x, Q), N, (q, phi, E, F, ffix, fq))."""
    if (name, alpha) not in _RUNS:
        key, mols, N = _case(name)
        eng = _engine(factory, key)
        batch = _batch(mols)
        _RUNS[name, alpha] = (eng, batch, N, eng.coulomb_xyz(*batch, N, ke=KE, alpha=alpha, parts=True))
    return _RUNS[name, alpha]


# ---------------------------------------------------------------------------------------------------- 1: the fixed-charge parts
def _check_fixed_parts(what, alpha, xyz, Qb, q, phi, Eb, F, ffix, fq):
    """One molecule's phi, ffix and E against coulomb64 on its device charges q: each within BOUND of the sum of its absolute terms;
    a lone atom has zeros and q == Q.  Returns the three errors as shares of the absolute sums."""
    n = len(q)
    phi64, E64, ffix64, sphi, sff = coulomb64(xyz, q, KE, alpha)
    sE = 0.5 * float(np.abs(q.astype(np.float64)) @ sphi)
    ephi, eff, eE = np.abs(phi - phi64), np.abs(ffix - ffix64), abs(Eb - E64)
    with np.errstate(divide="ignore", invalid="ignore"):
        rp = np.where(sphi > 0, ephi / sphi, 0.0).max()
        rf = np.where(sff > 0, eff.max(1) / sff, 0.0).max()
    re = eE / sE if sE else 0.0
    print(f"{what}, alpha {alpha} (n = {n}): phi {rp:.2e}, ffix {rf:.2e}, E {re:.2e} of the absolute sums "
          f"(|phi| {np.abs(phi64).max():.3e}, |ffix| {np.abs(ffix64).max():.3e}, E {E64:.6e})")
    if n == 1:
        assert not phi.any() and not ffix.any() and Eb == 0.0 and not F.any() and not fq.any()
        assert q[0] == Qb
        return rp, rf, re
    assert np.abs(phi64).max() > 0
    assert (ephi <= BOUND * sphi).all()
    assert (eff <= BOUND * sff[:, None]).all()
    assert eE <= BOUND * sE
    return rp, rf, re


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", CASES)
def test_fixed_charge_parts_against_float64_on_the_device_charges(gpu_engine_factory, name, alpha):
    """phi, ffix and E against coulomb64 on q_out itself: each within 2e-6 of the sum of its absolute terms."""
    eng, (offsets, xyz, x, Q), N, (q, phi, E, F, ffix, fq) = _run(gpu_engine_factory, name, alpha)
    assert E.dtype == np.float64 and E.shape == (len(offsets) - 1,)
    for b in range(len(offsets) - 1):
        a0, a1 = offsets[b], offsets[b + 1]
        _check_fixed_parts(f"{name}, molecule {b}", alpha, xyz[a0:a1], Q[b], q[a0:a1], phi[a0:a1], E[b], F[a0:a1], ffix[a0:a1], fq[a0:a1])


# ---------------------------------------------------------------------------------------------------- 2: composition bits
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("name", CASES)
def test_composition_with_the_gradient_call_bit_for_bit(gpu_engine_factory, name, alpha):
    eng, batch, N, (q, phi, E, F, ffix, fq) = _run(gpu_engine_factory, name, alpha)
    A = int(batch[0][-1])
    g = np.random.default_rng(A).normal(size=A).astype(np.float32)
    assert np.array_equal(eng.charges_vjp_xyz(*batch, g, N)[0], q)
    q2, gxyz = eng.charges_vjp_xyz(*batch, phi, N)
    assert np.array_equal(q2, q) and np.array_equal(fq, -gxyz)
    assert np.array_equal(F, ffix + fq) and F.dtype == np.float32
    out = eng.coulomb_xyz(*batch, N, ke=KE, alpha=alpha)
    assert len(out) == 4
    for got, want in zip(out, (q, phi, E, F)):
        assert np.array_equal(got, want)


def _check_call(eng, mol, N, alpha, what):
    """One molecule through the call on an engine of any shape or edge constants, "grad_path" 2 set: the fixed-charge parts against
    coulomb64 on the device charges (test 1) and the composition bits (test 2).  Returns (q, phi, E, F, ffix, fq)."""
    batch = _batch([mol])
    out = eng.coulomb_xyz(*batch, N, ke=KE, alpha=alpha, parts=True)
    q, phi, E, F, ffix, fq = out
    _check_fixed_parts(what, alpha, mol[0], batch[3][0], q, phi, E[0], F, ffix, fq)
    q2, gxyz = eng.charges_vjp_xyz(*batch, phi, N)
    assert np.array_equal(q2, q) and np.array_equal(fq, -gxyz)
    assert np.array_equal(F, ffix + fq) and F.dtype == np.float32
    for got, want in zip(eng.coulomb_xyz(*batch, N, ke=KE, alpha=alpha), (q, phi, E, F)):
        assert np.array_equal(got, want)
    return out


# ---------------------------------------------------------------------------------------------------- 3: the charges' part
_REF = {}


def _reference(n, N, alpha):
    if (n, N, alpha) not in _REF:
        w = _weights()
        xyz, x, Q = _lattice_molecule(n, 9, seed=n)
        mid = coulomb_forces64(xyz, x, Q, w, N, KE, alpha)
        lo = coulomb_forces64(xyz, x, Q, w, N, KE, alpha, kink_shift=+TAU)[5]
        hi = coulomb_forces64(xyz, x, Q, w, N, KE, alpha, kink_shift=-TAU)[5]
        _REF[n, N, alpha] = mid + (np.abs(lo - hi).max(),)
    return _REF[n, N, alpha]


@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("n,N", [(17, 24), (40, 40), (65, 72), (97, 97), (129, 136)])
def test_the_charges_part_against_the_float64_reference(gpu_engine_factory, n, N, alpha):
    """fq = -sum_k phi_k dq_k/dr against the full float64 reference with g = phi_ref, the project's standing rule: |fq + gxyz_ref| <=
    2e-4 max |gxyz_ref| + kink, kink = max |ref(+TAU) - ref(-TAU)|; the bracket may be used only while it is at most 0.05 max
    |gxyz_ref|, asserted on the reference alone.  (The fixed-charge part is 10 to 60 times larger and is held by test 1.)"""
    q64, phi64, E64, f64, ffix64, fq64, kink = _reference(n, N, alpha)
    scale = np.abs(fq64).max()
    print(f"({n}, {N}), alpha {alpha}: |ffix| max {np.abs(ffix64).max():.3e}, |gxyz| max {scale:.3e}, kink {kink:.3e} = {kink / scale:.2e} of it, "
          f"{kink / np.abs(f64).max():.2e} of max |F|")
    assert scale > 0 and kink <= 0.05 * scale
    xyz, x, Q = _lattice_molecule(n, 9, seed=n)
    eng = _engine(gpu_engine_factory, "random")
    q, phi, E, F, ffix, fq = eng.coulomb_xyz(np.int32([0, n]), xyz, x, np.float32([Q]), N, ke=KE, alpha=alpha, parts=True)
    err = np.abs(fq - fq64).max()
    print(f"    q {np.abs(q - q64).max():.3e}, phi {np.abs(phi - phi64).max():.3e} of {np.abs(phi64).max():.3e}, fq {err:.3e}, "
          f"F {np.abs(F - f64).max():.3e} of {np.abs(f64).max():.3e}, E {abs(E[0] - E64):.3e} of {abs(E64):.3e}")
    assert np.abs(q - q64).max() <= 2e-4
    assert err <= 2e-4 * scale + kink, (err, scale, kink)


# ---------------------------------------------------------------------------------------------------- 4: invariants
@pytest.mark.parametrize("alpha", ALPHAS)
def test_invariants(gpu_engine_factory, alpha):
    eng, batch, N, out = _run(gpu_engine_factory, "batch", alpha)
    offsets, xyz, x, Q = batch
    q, phi, E, F, ffix, fq = out
    again = eng.coulomb_xyz(*batch, N, ke=KE, alpha=alpha, parts=True)
    assert all(np.array_equal(a, b) for a, b in zip(out, again))
    unit = eng.coulomb_xyz(*batch, N, ke=1.0, alpha=alpha, parts=True)
    assert np.array_equal(unit[0], q)
    for b in range(len(offsets) - 1):
        a0, a1 = offsets[b], offsets[b + 1]
        # sum_i ffix_i = 0 to the bound of test 1 on the molecule's summed absolute terms
        sff = coulomb64(xyz[a0:a1], q[a0:a1], KE, alpha)[4]
        assert np.abs(ffix[a0:a1].sum(0, dtype=np.float64)).max() <= BOUND * sff.sum()
        # alone at the same N: the same bits
        alone = eng.coulomb_xyz(np.int32([0, a1 - a0]), xyz[a0:a1], x[a0:a1], Q[b:b + 1], N, ke=KE, alpha=alpha, parts=True)
        for k, (got, want) in enumerate(zip(alone, (q[a0:a1], phi[a0:a1], E[b:b + 1], F[a0:a1], ffix[a0:a1], fq[a0:a1]))):
            assert np.array_equal(got, want), (b, k)
    # linear in ke: phi and ffix are one float32 rounding (2^-24) of a float64 product on either side, E is float64; fq is a float32
    # backward of a seed scaled by ke (the ReLU decisions do not depend on the seed): sums of some hundred float32 terms
    eps = 2.0 ** -24
    assert (np.abs(phi - KE * unit[1].astype(np.float64)) <= 2.5 * eps * np.abs(phi)).all()
    assert (np.abs(ffix - KE * unit[4].astype(np.float64)) <= 2.5 * eps * np.abs(ffix)).all()
    assert (np.abs(E - KE * unit[2]) <= 1e-12 * np.abs(E)).all()
    assert np.abs(fq - KE * unit[5].astype(np.float64)).max() <= 1e-5 * np.abs(fq).max() and np.abs(fq).max() > 0


def test_training_state_untouched(gpu_engine_factory):
    from oracle import epnn_oracle_train as otr
    w = _weights()
    mols = [_lattice_molecule(n, 9, seed=40 + n) for n in (12, 9, 16)]
    offsets, xyz, x, Q = _batch(mols)
    eng, twin = (gpu_engine_factory(nx=9, T=2) for _ in range(2))
    y = np.random.default_rng(6).normal(size=int(offsets[-1])).astype(np.float32) * 0.2
    for e in (eng, twin):
        e.set_weights(w)
        e.train_init()
        e.train_step_xyz(offsets, xyz, x, Q, y, 16)
        e.train_step_xyz(offsets, xyz, x, Q, y, 16, apply=False)
    grads, weights = eng.get_gradients(), otr.flatten(eng.get_weights())
    q = eng.coulomb_xyz(offsets, xyz, x, Q, 16)[0]
    assert np.abs(q - eng.forward_xyz(offsets, xyz, x, Q, 16)).max() <= 2e-4
    assert np.array_equal(eng.get_gradients(), grads) and np.array_equal(otr.flatten(eng.get_weights()), weights)
    # the step count and the Adam moments: applying, and one more step, land on the same weights in both
    for e in (eng, twin):
        e.train_apply()
    assert np.array_equal(otr.flatten(eng.get_weights()), otr.flatten(twin.get_weights()))
    for e in (eng, twin):
        e.train_step_xyz(offsets, xyz, x, Q, y, 16)
    assert np.array_equal(otr.flatten(eng.get_weights()), otr.flatten(twin.get_weights()))
    assert np.abs(eng.coulomb_xyz(offsets, xyz, x, Q, 16)[0] - q).max() > 0


# ---------------------------------------------------------------------------------------------------- 5: refusals
def test_refusals_leave_the_handle_usable(gpu_engine_factory):
    from epnn_amd._lib import EpnnError, check, fptr, iptr
    import ctypes as C
    w = _weights()
    eng = gpu_engine_factory(nx=9, T=2)
    eng.set_weights(w)
    mols = [_lattice_molecule(n, 9, seed=50 + n) for n in (12, 9, 16)]
    offsets, xyz, x, Q = _batch(mols)
    first = eng.coulomb_xyz(offsets, xyz, x, Q, 16, parts=True)

    def still_fine():
        assert all(np.array_equal(a, b) for a, b in zip(eng.coulomb_xyz(offsets, xyz, x, Q, 16, parts=True), first))

    for kw, match in (({"alpha": -1.0}, "alpha"), ({"alpha": float("nan")}, "alpha"), ({"alpha": float("inf")}, "alpha"),
                      ({"ke": float("inf")}, "ke"), ({"ke": float("nan")}, "ke")):
        with pytest.raises(EpnnError, match=match + " must be finite"):
            eng.coulomb_xyz(offsets, xyz, x, Q, 16, **kw)
        still_fine()
    q, phi, F = (np.empty(s, np.float32) for s in ((37,), (37,), (37, 3)))
    E = np.empty(3, np.float64)
    with pytest.raises(EpnnError, match="null"):                  # (a null f_out, through the binding)
        check(eng.lib.epnn_coulomb_xyz(eng.h, 3, 16, iptr(offsets), fptr(xyz), fptr(x), fptr(Q), KE, 0.0, fptr(q), fptr(phi),
                                       E.ctypes.data_as(C.POINTER(C.c_double)), None, None, None), eng.lib)
    still_fine()
    with pytest.raises(EpnnError, match="offsets"):
        eng.coulomb_xyz(np.int32([1, 12, 21, 37]), xyz, x, Q, 16)
    with pytest.raises(EpnnError, match="does not fit"):
        eng.coulomb_xyz(np.int32([0, 12, 12, 37]), xyz, x, Q, 16)
    still_fine()
    with pytest.raises(EpnnError, match="does not fit N=12"):
        eng.coulomb_xyz(offsets, xyz, x, Q, 12)
    still_fine()
    twin = xyz.copy()
    twin[5] = twin[2]
    with pytest.raises(EpnnError, match="coincide"):
        eng.coulomb_xyz(offsets, twin, x, Q, 16)
    still_fine()
    eng.set_partition(0, 2, exchange=lambda *a: None)
    with pytest.raises(EpnnError, match="partition"):
        eng.coulomb_xyz(offsets, xyz, x, Q, 16)
    eng.set_partition(0, 1)
    still_fine()
    # update layers other than [32, 32]
    rng = np.random.default_rng(3)

    def dense(i, o):
        lim = 0.6 * np.sqrt(6.0 / (i + o))
        return rng.uniform(-lim, lim, (i, o)).astype(np.float32), rng.uniform(-0.1, 0.1, (o,)).astype(np.float32)

    other = dict(w)
    other["upd"] = [dense(48 + 32, 64), dense(64, 48)]
    eng.set_weights(other)
    with pytest.raises(EpnnError, match=r"\[32, 32\]"):
        eng.coulomb_xyz(offsets, xyz, x, Q, 16)
    assert np.isfinite(eng.forward_xyz(offsets, xyz, x, Q, 16)).all()
    eng.set_weights(w)
    still_fine()


def test_the_model_method(gpu_engine_factory):
    """EPNNModel.coulomb_xyz: the engine's call with N = natom by default."""
    from epnn_amd import charge_gn
    xyz, x, Q = _lattice_molecule(17, 9, seed=17)
    model = charge_gn.make_model([32, 32], 48, 2, 9, 24)
    model.set_weights_dict(_weights())
    off, Qa = np.int32([0, 17]), np.float32([Q])
    got = model.coulomb_xyz(off, xyz, x, Qa, alpha=0.5, parts=True)
    want = _run(gpu_engine_factory, "17-24", 0.5)[3]
    assert len(got) == 6 and all(np.array_equal(a, b) for a, b in zip(got, want))
    assert charge_gn.KE_EV_ANGSTROM == KE


# ---------------------------------------------------------------------------------------------------- 6: scratch
def _gl_pieces(n):
    return min(16, max(1, -(-2048 // -(-n // 16))))


def _cl_pieces(n):
    return 1 if n <= 64 else max(1, min(32, -(-n // 128), -(-2048 // -(-n // 64))))


def _formula(ns, nx, T, pairs, ctasks):
    """include/epnn.h: bytes = A (1344 + 4 nx + 324 T + 256 pieces + 32 cpieces) + 16 (gtasks + ctasks) + 1116 max(pairs, 1) + 56 B + 8240"""
    A, B = sum(ns), len(ns)
    pieces, cpieces = max(_gl_pieces(n) for n in ns), max(_cl_pieces(n) for n in ns)
    gtasks = sum(-(-n // 16) * _gl_pieces(n) for n in ns)
    return A * (1344 + 4 * nx + 324 * T + 256 * pieces + 32 * cpieces) + 16 * (gtasks + ctasks) + 1116 * max(pairs, 1) + 56 * B + 8240


@pytest.mark.parametrize("ns,N,ctasks", [((300,), 300, 15), ((70, 1, 33, 120), 128, 5), ((18,) * 7, 24, 3)])
def test_scratch_follows_the_formula(gpu_engine_factory, ns, N, ctasks):
    """epnn_last_stats against the header's formula: never below it, above it by less than 256 bytes for each of the 44 buffers.
    ctasks: 5 blocks x 3 pieces; 2 blocks, one wavefront for the molecules of 1 and 33 atoms, 2 blocks; three 18-atom molecules to a
    wavefront."""
    eng = _engine(gpu_engine_factory, "random")
    batch = _batch([_lattice_molecule(n, 9, seed=300 + k) for k, n in enumerate(ns)])
    eng.coulomb_xyz(*batch, N)
    st = eng.last_stats()
    want = _formula(ns, 9, 2, int(st[0]), ctasks)
    print(f"{ns}: {st[0]} pairs, {st[2]} bytes, formula {want}")
    assert st[0] > 0 and st[1] == 0
    assert want <= int(st[2]) < want + 44 * 256
