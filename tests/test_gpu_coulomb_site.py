"""Per-atom Gaussian widths, self-energy and on-site terms in the open Coulomb call (epnn_coulomb_xyz_site, Engine.coulomb_xyz_site) on
the GPU: the fixed-charge parts against the float64 reference on the device's own charges, the composition with the gradient call
and the reduction to the _excl entry bit for bit, equal widths against the alpha route, the totals against the full float64
reference, invariants, refusals and the scratch.  GPU only.

Widths are drawn in [0.3, 1.2] A per atom, chi and J of order 1; lists come from coulomb_excl_ref.exclusion_cases and reach the
library shuffled.  The bound: 2e-6 of the absolute pair terms actually added (the sweep's and the listed pairs' |(s - 1) term|) --
the widths mode adds one add, one reciprocal square root and one multiply in front of erff, about 4 * 2^-24 on u, and |u erf'(u)| <=
erf(u) -- plus 2 * 2^-24 of the rest: the self term (gamma_ii rounded to float32, the output rounded to float32) and, for mu, the
on-site terms |chi_i| + |J_i q_i| (exact float64 products of float32 values, then mu's rounding to float32).

Measured worst shares of that bound (MI355X, the 14 runs of test 1 and the model method): phi 0.035, mu 0.034, ffix 0.078 (all on the
two-atom molecule), E 0.213 (the lone atom of the batch, whose energy is its on-site and self terms alone: 2 * 2^-24 of them); from 17
atoms on phi 0.021, mu 0.026, ffix 0.041, E 0.005.  Equal widths against the alpha route: below 0.0005 of twice the bound."""
import ctypes as C

import numpy as np
import pytest

from conftest import random_weights
from coulomb_excl_ref import exclusion_cases, shuffled
from site_ref import coulomb_site64
from test_gpu_coulomb import BOUND, FAR, KE, _formula
from test_gpu_grad_large import TAU, _batch, _lattice_molecule
from xyz_grad_ref import forward64, vjp64

pytestmark = pytest.mark.gpu

REST = 2 * 2.0 ** -24
SIZES = [(2, 8), (17, 24), (64, 64), (65, 72), (129, 136)]       # the block, tile and piece boundaries of epnn_coulomb.hip.h
CASES = [f"{n}-{N}" for n, N in SIZES] + ["batch", "far"]
_CASES, _ENGINE, _RUNS = {}, [], {}


def _weights():
    return random_weights(9, 2, seed=5, scale=0.6)


def _case(name):
    """(batch, N, (sigma, chi, J) per atom in float32, (pairs flat and sorted, scale), per-molecule lists)"""
    if name not in _CASES:
        if name == "batch":
            mols, N = [_lattice_molecule(n, 9, seed=n) for n in (70, 1, 33, 120)], 128
        elif name == "far":
            xyz, x, Q = _lattice_molecule(65, 9, seed=65)
            mols, N = [(xyz + FAR, x, Q)], 72
        else:
            n, N = (int(v) for v in name.split("-"))
            mols = [_lattice_molecule(n, 9, seed=n)]
        batch = _batch(mols)
        offsets, xyz = batch[0], batch[1]
        A = int(offsets[-1])
        rng = np.random.default_rng(1000 + A)
        site = (rng.uniform(0.3, 1.2, A).astype(np.float32), rng.normal(size=A).astype(np.float32),
                np.abs(rng.normal(size=A)).astype(np.float32) * 3)
        per = [exclusion_cases(xyz[offsets[b]:offsets[b + 1]]) for b in range(len(offsets) - 1)]
        pairs = np.concatenate([p + offsets[b] for b, (p, s) in enumerate(per)]).astype(np.int32)
        scale = np.concatenate([s for p, s in per]).astype(np.float32)
        _CASES[name] = (batch, N, site, (pairs, scale), per)
    return _CASES[name]


def _engine(factory):
    if not _ENGINE:
        eng = factory(nx=9, T=2)
        eng.set_weights(_weights())
        eng.set_option("grad_path", 2)
        _ENGINE.append(eng)
    return _ENGINE[0]


def _run(factory, name, full):
    """The call with parts, once per case.  full: widths, chi, J, the self term and the shuffled list; otherwise widths and chi alone,
    no self term, no list.  (engine, case, outputs (q, phi, mu, E, F, ffix, fq))."""
    if (name, full) not in _RUNS:
        case = _case(name)
        batch, N, (sigma, chi, J), (pairs, scale), per = case
        eng = _engine(factory)
        if full:
            out = eng.coulomb_xyz_site(*batch, N, ke=KE, sigma=sigma, chi=chi, hardness=J, self_energy=True, exclusions=shuffled(pairs, scale),
                                       parts=True)
        else:
            out = eng.coulomb_xyz_site(*batch, N, ke=KE, sigma=sigma, chi=chi, self_energy=False, parts=True)
        _RUNS[name, full] = (eng, case, out)
    return _RUNS[name, full]


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(u, v) for u, v in zip(a, b))


def _shares(err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0)).max())


def _bound(s):
    return BOUND * s["real"] + REST * s["rest"]


def _check(what, ref, phi, mu, Eb, ffix, k=1.0):
    sh = (_shares(np.abs(phi - ref.phi), k * _bound(ref.s_phi)), _shares(np.abs(mu - ref.mu), k * _bound(ref.s_mu)),
          _shares(np.abs(ffix - ref.ffix).max(1), k * _bound(ref.s_ffix)), _shares(np.float64(abs(Eb - ref.E)), np.float64(k * _bound(ref.s_E))))
    print(f"{what} (n = {len(phi)}): phi {sh[0]:.3f}, mu {sh[1]:.3f}, ffix {sh[2]:.3f}, E {sh[3]:.3f} of the bounds")
    assert max(sh) <= 1.0, sh
    return sh


# ---------------------------------------------------------------------------------------------------- 1: the fixed-charge parts
@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_fixed_charge_parts_against_float64_on_the_device_charges(gpu_engine_factory, name, full):
    """phi, mu, ffix and E against coulomb_site64 on q_out itself, molecule by molecule."""
    eng, ((offsets, xyz, x, Q), N, (sigma, chi, J), lists, per), (q, phi, mu, E, F, ffix, fq) = _run(gpu_engine_factory, name, full)
    assert E.dtype == np.float64 and E.shape == (len(offsets) - 1,) and mu.dtype == np.float32 and mu.shape == q.shape
    for b, (p, s) in enumerate(per):
        a0, a1 = offsets[b], offsets[b + 1]
        ref = coulomb_site64(xyz[a0:a1], q[a0:a1], KE, sigma=sigma[a0:a1], chi=chi[a0:a1], hard=J[a0:a1] if full else None,
                             self_term=int(full), pairs=p if full else None, scale=s if full else None)
        _check(f"{name} full={full}, molecule {b}", ref, phi[a0:a1], mu[a0:a1], E[b], ffix[a0:a1])
        if a1 - a0 == 1:
            assert not ffix[a0:a1].any() and q[a0] == Q[b]
    assert not np.array_equal(mu, phi)


# ---------------------------------------------------------------------------------------------------- 2: composition bits
def _raw(eng, batch, N, alpha, sigma, chi, J, self_term, lists, mu_out=True, parts=True):
    """The C entry itself, so that NULL outputs and NULL lists can be passed."""
    from epnn_amd._lib import check, fptr, iptr
    offsets, xyz, x, Q = batch
    B, A = len(offsets) - 1, int(offsets[-1])
    opt = lambda a, f=fptr: None if a is None else f(a)
    q, phi, mu = (np.empty((A,), np.float32) for _ in range(3))
    F, ffix, fq = (np.empty((A, 3), np.float32) for _ in range(3))
    E = np.empty((B,), np.float64)
    npairs, ei, ej, es = (0, None, None, None) if lists is None else (len(lists[1]), np.ascontiguousarray(lists[0][:, 0]),
                                                                      np.ascontiguousarray(lists[0][:, 1]), lists[1])
    check(eng.lib.epnn_coulomb_xyz_site(eng.h, B, N, iptr(offsets), fptr(xyz), fptr(x), fptr(Q), KE, float(alpha), opt(sigma), opt(chi), opt(J),
                                        int(self_term), npairs, opt(ei, iptr), opt(ej, iptr), opt(es), fptr(q), fptr(phi),
                                        fptr(mu) if mu_out else None, E.ctypes.data_as(C.POINTER(C.c_double)), fptr(F),
                                        fptr(ffix) if parts else None, fptr(fq) if parts else None), eng.lib)
    return q, phi, mu, E, F, ffix, fq


@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("name", CASES)
def test_composition_with_the_gradient_call_bit_for_bit(gpu_engine_factory, name, full):
    eng, (batch, N, (sigma, chi, J), (pairs, scale), per), out = _run(gpu_engine_factory, name, full)
    q, phi, mu, E, F, ffix, fq = out
    q2, gxyz = eng.charges_vjp_xyz(*batch, mu, N)
    assert np.array_equal(q2, q) and np.array_equal(fq, -gxyz)
    assert np.array_equal(F, ffix + fq) and F.dtype == np.float32
    kw = dict(sigma=sigma, chi=chi, hardness=J, self_energy=True, exclusions=shuffled(pairs, scale)) if full else dict(sigma=sigma, chi=chi,
                                                                                                                      self_energy=False)
    five = eng.coulomb_xyz_site(*batch, N, ke=KE, **kw)
    assert len(five) == 5 and _same(five, out[:5])
    lists = shuffled(pairs, scale) if full else None
    bare = _raw(eng, batch, N, 0.0, sigma, chi, J if full else None, full, lists, mu_out=False, parts=False)
    assert _same([bare[k] for k in (0, 1, 3, 4)], [out[k] for k in (0, 1, 3, 4)])
    assert _same(_raw(eng, batch, N, 0.0, sigma, chi, J if full else None, full, lists), out)


# ---------------------------------------------------------------------------------------------------- 3: reduction bits
@pytest.mark.parametrize("alpha", [0.0, 0.5])
@pytest.mark.parametrize("name", ["17-24", "65-72", "batch"])
def test_nothing_given_is_the_excl_entry_bit_for_bit(gpu_engine_factory, name, alpha):
    batch, N, site, (pairs, scale), per = _case(name)
    eng = _engine(gpu_engine_factory)
    for ex in (None, shuffled(pairs, scale)):
        want = eng.coulomb_xyz_excl(*batch, N, ke=KE, alpha=alpha, parts=True, exclusions=ex)
        got = eng.coulomb_xyz_site(*batch, N, ke=KE, alpha=alpha, self_energy=False, exclusions=ex, parts=True)
        assert len(got) == 7 and _same([got[k] for k in (0, 1, 3, 4, 5, 6)], want)
        assert np.array_equal(got[2], got[1])                    # mu == phi
    assert _same(_raw(eng, batch, N, alpha, None, None, None, 0, None), eng.coulomb_xyz_site(*batch, N, ke=KE, alpha=alpha, self_energy=False, parts=True))


# ---------------------------------------------------------------------------------------------------- 4: equal widths
@pytest.mark.parametrize("name", ["17-24", "65-72", "129-136", "batch"])
def test_equal_widths_against_the_alpha_route(gpu_engine_factory, name):
    """sigma_i = 0.8 against coulomb_xyz_excl(alpha = 1 / (2 sigma)): two float32 routes to the same sums, each within the bound of
    test 1 of the float64 value, so within twice that bound of each other; the charges are the same bits."""
    batch, N, site, (pairs, scale), per = _case(name)
    offsets, xyz = batch[0], batch[1]
    eng = _engine(gpu_engine_factory)
    sg = np.full(int(offsets[-1]), 0.8, dtype=np.float32)
    alpha = 0.5 / float(sg[0])
    ex = shuffled(pairs, scale)
    q, phi, mu, E, F, ffix, fq = eng.coulomb_xyz_site(*batch, N, ke=KE, sigma=sg, self_energy=False, exclusions=ex, parts=True)
    q2, phi2, E2, F2, ffix2, fq2 = eng.coulomb_xyz_excl(*batch, N, ke=KE, alpha=alpha, exclusions=ex, parts=True)
    assert np.array_equal(q, q2) and np.array_equal(mu, phi)
    for b, (p, s) in enumerate(per):
        a0, a1 = offsets[b], offsets[b + 1]
        ref = coulomb_site64(xyz[a0:a1], q[a0:a1], KE, sigma=sg[a0:a1], pairs=p, scale=s)
        ref.phi, ref.mu, ref.E, ref.ffix = phi2[a0:a1].astype(np.float64), phi2[a0:a1].astype(np.float64), E2[b], ffix2[a0:a1].astype(np.float64)
        _check(f"equal widths {name}, molecule {b}", ref, phi[a0:a1], mu[a0:a1], E[b], ffix[a0:a1], k=2.0)


# ---------------------------------------------------------------------------------------------------- 5: totals
@pytest.mark.parametrize("name", ["17-24", "65-72"])
def test_total_forces_against_the_float64_reference(gpu_engine_factory, name):
    """q from forward64, the fixed parts from coulomb_site64 on those charges, fq = -vjp64(g = mu) with the ReLU-kink bracket
    (coulomb_forces64's scheme with the seed mu).  The standing rule: |fq - fq_ref| <= 2e-4 max |fq_ref| + kink, usable only while
    kink <= 0.05 of it; and F on the larger of the two parts' scales."""
    eng, ((offsets, xyz, x, Q), N, (sigma, chi, J), (pairs, scale), per), (q, phi, mu, E, F, ffix, fq) = _run(gpu_engine_factory, name, True)
    n = int(offsets[-1])
    w = _weights()
    q64 = forward64(xyz, x, Q[0], w, N=N)[:n]
    ref = coulomb_site64(xyz, q64, KE, sigma=sigma, chi=chi, hard=J, self_term=1, pairs=pairs, scale=scale)
    fq64, lo, hi = (-vjp64(xyz, x, Q[0], ref.mu, w, N=N, kink_shift=s)[1] for s in (0, +TAU, -TAU))
    kink, sq = np.abs(lo - hi).max(), np.abs(fq64).max()
    sf = max(np.abs(ref.ffix).max(), sq)
    print(f"open {name}: q {np.abs(q - q64).max():.3e}, mu {np.abs(mu - ref.mu).max():.3e} of {np.abs(ref.mu).max():.3e}, fq {np.abs(fq - fq64).max():.3e} "
          f"of {sq:.3e}, F {np.abs(F - (ref.ffix + fq64)).max():.3e} of {sf:.3e}, kink {kink:.3e}")
    assert sq > 0 and kink <= 0.05 * sq
    assert np.abs(q - q64).max() <= 2e-4
    assert np.abs(fq - fq64).max() <= 2e-4 * sq + kink
    assert np.abs(F - (ref.ffix + fq64)).max() <= 2e-4 * sf + kink


# ---------------------------------------------------------------------------------------------------- 6: invariants
def test_invariants(gpu_engine_factory):
    """sum ffix = 0 per molecule to the bound; the list's order and direction; a molecule alone at the same N; two calls."""
    eng, (batch, N, (sigma, chi, J), (pairs, scale), per), out = _run(gpu_engine_factory, "batch", True)
    offsets, xyz, x, Q = batch
    q, ffix = out[0], out[5]
    call = lambda ex: eng.coulomb_xyz_site(*batch, N, ke=KE, sigma=sigma, chi=chi, hardness=J, self_energy=True, exclusions=ex, parts=True)
    assert _same(call(shuffled(pairs, scale)), out)
    assert _same(call((pairs, scale)), out) and _same(call((pairs[::-1, ::-1], scale[::-1])), out)
    assert not np.array_equal(call(None)[1], out[1])
    for b, (p, s) in enumerate(per):
        a0, a1 = offsets[b], offsets[b + 1]
        ref = coulomb_site64(xyz[a0:a1], q[a0:a1], KE, sigma=sigma[a0:a1], chi=chi[a0:a1], hard=J[a0:a1], self_term=1, pairs=p, scale=s)
        assert np.abs(ffix[a0:a1].sum(0, dtype=np.float64)).max() <= _bound(ref.s_ffix).sum()
        alone = eng.coulomb_xyz_site(np.int32([0, a1 - a0]), xyz[a0:a1], x[a0:a1], Q[b:b + 1], N, ke=KE, sigma=sigma[a0:a1], chi=chi[a0:a1],
                                     hardness=J[a0:a1], self_energy=True, exclusions=shuffled(p, s, seed=3), parts=True)
        for k, (got, want) in enumerate(zip(alone, out)):
            assert np.array_equal(got, want[b:b + 1] if k == 3 else want[a0:a1]), (b, k)


# ---------------------------------------------------------------------------------------------------- 7: refusals
def test_refusals_leave_the_handle_usable(gpu_engine_factory):
    from epnn_amd._lib import EpnnError
    eng, (batch, N, (sigma, chi, J), (pairs, scale), per), first = _run(gpu_engine_factory, "batch", True)
    A = int(batch[0][-1])
    good = shuffled(pairs, scale)
    entry = "epnn_coulomb_xyz_site: "

    def still_fine():
        assert _same(eng.coulomb_xyz_site(*batch, N, ke=KE, sigma=sigma, chi=chi, hardness=J, self_energy=True, exclusions=good, parts=True), first)

    def with_value(a, k, v):
        a = a.copy()
        a[k] = v
        return a

    # through the C entry: the Python layer refuses the first two itself
    with pytest.raises(EpnnError, match=entry + "both sigma and alpha"):
        _raw(eng, batch, N, 0.5, sigma, None, None, 0, None)
    still_fine()
    with pytest.raises(EpnnError, match=entry + "self_term = 1 with neither sigma nor alpha > 0"):
        _raw(eng, batch, N, 0.0, None, chi, None, 1, None)
    with pytest.raises(EpnnError, match=entry + "self_term = 2 must be 0 or 1"):
        _raw(eng, batch, N, 0.0, sigma, None, None, 2, None)
    still_fine()
    with pytest.raises(ValueError, match="both sigma and alpha"):
        eng.coulomb_xyz_site(*batch, N, alpha=0.5, sigma=sigma)
    with pytest.raises(ValueError, match="neither sigma nor alpha > 0"):
        eng.coulomb_xyz_site(*batch, N, chi=chi)
    for bad in (0.0, -0.5, np.nan, np.inf, 1e-30, 1e25):
        with pytest.raises(EpnnError, match=entry + r"sigma\[7\]"):
            eng.coulomb_xyz_site(*batch, N, sigma=with_value(sigma, 7, bad))
        still_fine()
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(EpnnError, match=entry + r"chi\[3\] .*not finite"):
            eng.coulomb_xyz_site(*batch, N, sigma=sigma, chi=with_value(chi, 3, bad))
        with pytest.raises(EpnnError, match=entry + r"hard\[%d\] .*not finite" % (A - 1)):
            eng.coulomb_xyz_site(*batch, N, sigma=sigma, hardness=with_value(J, A - 1, bad))
    still_fine()
    for kw in ({"sigma": sigma[:-1]}, {"sigma": sigma, "chi": chi[1:]}, {"sigma": sigma, "hardness": np.concatenate([J, J])},
               {"sigma": sigma.reshape(-1, 1)}):
        with pytest.raises(ValueError, match=r"must have shape \(%d,\)" % A):
            eng.coulomb_xyz_site(*batch, N, **kw)
    # the _excl entry's refusals
    p = pairs.copy()
    p[2] = (A, 3)
    with pytest.raises(EpnnError, match=entry + r"exclusion pair 2 = .*outside \[0, %d\)" % A):
        eng.coulomb_xyz_site(*batch, N, sigma=sigma, exclusions=(p, scale))
    p[2] = pairs[0][::-1]
    with pytest.raises(EpnnError, match=entry + "exclusion pair 2 = .*listed twice: pair 0"):
        eng.coulomb_xyz_site(*batch, N, sigma=sigma, exclusions=(p, scale))
    with pytest.raises(EpnnError, match=entry + "exclusion pair 1 = .*not finite"):
        eng.coulomb_xyz_site(*batch, N, sigma=sigma, exclusions=(pairs, with_value(scale, 1, np.nan)))
    still_fine()
    with pytest.raises(EpnnError, match=entry + "alpha must be finite"):
        eng.coulomb_xyz_site(*batch, N, alpha=-1.0, self_energy=False)
    with pytest.raises(EpnnError, match=entry + "ke must be finite"):
        eng.coulomb_xyz_site(*batch, N, ke=np.inf, sigma=sigma)
    twin = batch[1].copy()
    twin[5] = twin[2]
    with pytest.raises(EpnnError, match="coincide"):
        eng.coulomb_xyz_site(batch[0], twin, batch[2], batch[3], N, sigma=sigma)
    still_fine()


def test_the_model_method_and_per_element(gpu_engine_factory):
    """EPNNModel.coulomb_xyz_site with tables by element through engine.per_element: the engine's call with N = natom."""
    from epnn_amd import charge_gn
    from epnn_amd.engine import per_element
    xyz, x, Q = _lattice_molecule(17, 9, seed=17)
    Z = sorted(set(int(z) for z in x[:, 0]))
    sig = per_element(x[:, 0], {z: 0.4 + 0.05 * k for k, z in enumerate(Z)})
    chi = per_element(x[:, 0], {z: 0.1 * z - 1.0 for z in Z})
    J = per_element(x[:, 0], {}, default=7.5)
    model = charge_gn.make_model([32, 32], 48, 2, 9, 24)
    model.set_weights_dict(_weights())
    off, Qa = np.int32([0, 17]), np.float32([Q])
    got = model.coulomb_xyz_site(off, xyz, x, Qa, sigma=sig, chi=chi, hardness=J, parts=True)
    want = _engine(gpu_engine_factory).coulomb_xyz_site(off, xyz, x, Qa, 24, sigma=sig, chi=chi, hardness=J, parts=True)
    assert len(got) == 7 and _same(got, want)
    q, phi, mu, E, F, ffix, fq = got
    _check("model method", coulomb_site64(xyz, q, KE, sigma=sig, chi=chi, hard=J, self_term=1), phi, mu, E[0], ffix)


# ---------------------------------------------------------------------------------------------------- 8: scratch
def _r256(v):
    return (v + 255) // 256 * 256


@pytest.mark.parametrize("with_list", [False, True])
@pytest.mark.parametrize("name", ["batch", "129-136"])
def test_scratch_follows_the_formula(gpu_engine_factory, name, with_list):
    """epnn_last_stats out[2] of a site call on a fresh handle against the _excl entry's on the same batch and list, to the byte: 16 A of
    staged rows, a buffer of its own rounded up to 256, and 4 A of mu at the end of the outputs' buffer ([A] phi | [A][3] ffix | flag |
    [B] E at 8), whose rounding to 256 moves with it."""
    batch, N, (sigma, chi, J), (pairs, scale), per = _case(name)
    A, B = int(batch[0][-1]), len(batch[0]) - 1
    ex = (pairs, scale) if with_list else None
    stats = []
    for site in (False, True):
        eng = gpu_engine_factory(nx=9, T=2)
        eng.set_weights(_weights())
        if site:
            eng.coulomb_xyz_site(*batch, N, ke=KE, sigma=sigma, chi=chi, hardness=J, exclusions=ex)
        else:
            eng.coulomb_xyz_excl(*batch, N, ke=KE, exclusions=ex)
        stats.append(eng.last_stats())
        eng.close()
    co = ((4 * A + 1) * 4 + 7) // 8 * 8 + 8 * B
    want = _r256(16 * A) + _r256(co + 4 * A) - _r256(co)
    got = int(stats[1][2]) - int(stats[0][2])
    print(f"{name}: A = {A}, list {with_list}: {int(stats[1][2])} bytes, {got} more than the _excl entry, stated {want} (20 A = {20 * A})")
    assert stats[1][0] == stats[0][0] and got == want and abs(want - 20 * A) < 2 * 256
    if name == "batch" and not with_list:                        # (70, 1, 33, 120): 2 + 1 + 2 tasks of the sweep; 44 buffers and one more
        lo = _formula((70, 1, 33, 120), 9, 2, int(stats[1][0]), 5) + 20 * A
        assert lo - 256 < int(stats[1][2]) < lo + 45 * 256
