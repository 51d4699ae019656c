"""epnn_coulomb_xyz over its whole domain: one pair at a time over alpha and D, molecules packed into a wavefront in every way the
packing can go, and the piece counts above 4096 atoms.  The fixtures, the bound and the assertions are tests/test_gpu_coulomb.py's:
BOUND = 2e-6 of the sum of the absolute terms against coulomb64 on the device's own charges, the composition with
charges_vjp_xyz(g=phi) on "grad_path" 2 bit for bit.  No tolerance of its own.  GPU only (the conditions on the inputs alone also run on
the CPU: tests/test_coulomb_ref.py).

Pairs.  A two-atom molecule has one partner per atom: "within BOUND of the sum of the absolute terms" is then the relative error of
that one term, kappa(D) for phi and E and g(alpha D) / D^2 for ffix.  One call per alpha; each call takes 64 distances spaced
geometrically over 0.6 .. 80 A (alpha = 0.5: 32 spaced evenly over 1.8 .. 2.2 A, u = 0.9 .. 1.1 around the branch of cl_g; alpha = 0:
both sets), every fourth of them a second time 1000 A from the origin, two different elements, Q = +1 or -1, a random orientation.
Beyond the cutoff of 3.0 A a molecule has no listed pair, the charges are Q / 2 and their gradient is zero.  Thirty-two such
molecules share a wavefront.  u = alpha D covers (asserted on the inputs): 8 and more values in each of [0.9, 1) and [1, 1.1] and in
every decade from 1e-3 to 1e2; values above 10 at three alphas; 6e-4 .. 320 in all.

Packed batches at N = 128 (the last one at N = 136: it has a molecule of 130 atoms, which N = 128 refuses), alpha in {0, 0.3}; the
wavefronts (tasks of k_cl_sweep) a mirror of cl_build_tasks counts, stated here and held against the reported scratch:
    (32, 32) 1    (63, 1) 1    (33, 31, 1) 2    (64, 1, 1) 2    (1, 64) 2    (20, 20, 20, 20) 2    (1,) * 70 2
    (65, 3, 61, 64, 2, 130, 40, 24) 12 = 2 blocks | 3 + 61 | 64 | 2 | 3 blocks x 2 pieces | 40 + 24

Pieces.  Single lattice clusters of 4100 atoms (65 blocks x 32 pieces of 129 partners, the last of 101; the last block of 4 atoms) and
of 8250 atoms (129 blocks x 16 pieces of 516, the last of 510).  At 8250 atoms the float64 rows are those of the first and the last
block of 64 atoms and of every eighth atom between, and the energy is checked where scipy's erf is there to sum all pairs in seconds.

Measured on an MI355X, as shares of the absolute sums (BOUND = 2e-6); no case exceeded the bound, no kernel or driver changed:
  pairs, worst per-pair error of phi / ffix / E and the u = alpha D where it sits
    alpha 1e-3   2.2e-7 (8.8e-4) / 5.6e-7 (1.3e-2) / 1.8e-7 (4.6e-2)
    alpha 0.02   2.1e-7 (0.27)   / 4.9e-7 (3.6e-2) / 1.7e-7 (0.27)
    alpha 0.3    2.1e-7 (0.53)   / 6.1e-7 (0.53)   / 2.0e-7 (0.53)
    alpha 0.5    1.7e-7 (0.93)   / 3.2e-7 (0.98)   / 1.3e-7 (0.93)
    alpha 1.0    1.3e-7 (0.82)   / 2.9e-7 (0.82)   / 1.1e-7 (2.8)
    alpha 4.0    1.6e-7 (3.3)    / 2.9e-7 (3.5)    / 1.5e-7 (3.3)
    alpha 0      1.5e-7          / 2.8e-7          / 1.3e-7
    (a CPU emulation of cl_g with correctly rounded erf and exp gives 2.3e-7 for g alone; rsqrtf and the three factors of
    g / D^3 add the rest)
  packed batches, worst molecule, phi / ffix / E at alpha 0 and at alpha 0.3
    (32, 32)         2.5e-8 / 5.8e-8 / 5.3e-9    3.7e-8 / 7.8e-8 / 4.7e-9
    (63, 1)          1.8e-8 / 5.2e-8 / 1.8e-9    3.2e-8 / 5.8e-8 / 2.3e-10
    (33, 31, 1)      3.8e-8 / 7.0e-8 / 2.2e-9    4.1e-8 / 6.8e-8 / 4.4e-9
    (64, 1, 1)       2.3e-8 / 3.9e-8 / 1.2e-9    2.6e-8 / 4.7e-8 / 5.3e-10
    (1, 64)          1.5e-8 / 4.1e-8 / 2.2e-9    3.5e-8 / 5.1e-8 / 6.4e-10
    (20,) * 4        3.8e-8 / 7.8e-8 / 3.3e-9    7.8e-8 / 1.0e-7 / 1.1e-8
    (1,) * 70        zeros, q == Q
    (65, 3, .., 24)  9.0e-8 / 1.6e-7 / 7.5e-8    2.1e-7 / 4.1e-7 / 1.8e-7   (its molecules of 2 and 3 atoms: few terms to average over)
  pieces (weights at scale 0.35, |q| up to 0.93 at 4100 atoms and 7.6 at 8250)
    4100 atoms, alpha 0      5.2e-9 / 1.8e-8 / 2.4e-11     134 810 listed pairs, 171 MB of scratch
    4100 atoms, alpha 0.3    4.2e-9 / 9.1e-9 / 5.5e-11
    8250 atoms, alpha 0.3    3.1e-9 / 6.1e-9 / 3.7e-11     1144 rows; 283 433 listed pairs, 346 MB of scratch; 2.6 s, the reference's
  scratch: every case within the header's formula and 44 x 256 bytes above it.
"""
import functools

import numpy as np
import pytest

from conftest import random_weights
from coulomb_ref import coulomb64_rows, coulomb_energy64
from test_gpu_coulomb import BOUND, FAR, KE, _check_fixed_parts, _cl_pieces, _engine, _formula
from test_gpu_grad_large import _batch, _lattice_molecule

pytestmark = pytest.mark.gpu

CUTOFF = 3.0
ELEMENTS = np.array([1, 6, 7, 8, 9, 15, 16, 17, 35])


# ---------------------------------------------------------------------------------------------------- 1: one pair at a time
PAIR_ALPHAS = {1e-3: "geometric", 0.02: "geometric", 0.3: "geometric", 1.0: "geometric", 4.0: "geometric", 0.5: "branch", 0.0: "both"}
PAIR_N = 8


def _distances(kind):
    geometric, branch = np.geomspace(0.6, 80.0, 64), np.linspace(1.8, 2.2, 32)
    return {"geometric": geometric, "branch": branch, "both": np.concatenate([geometric, branch])}[kind]


@functools.lru_cache(maxsize=None)
def two_atom_molecules(kind):
    """The two-atom molecules of a set of distances, and every fourth of them again 1000 A from the origin."""
    rng = np.random.default_rng({"geometric": 1, "branch": 2, "both": 3}[kind])
    mols = []
    for k, D in enumerate(_distances(kind)):
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        first = rng.uniform(-1.0, 1.0, 3)
        xyz = np.stack([first, first + D * axis]).astype(np.float32)
        el = rng.choice(8, size=2, replace=False)
        x = np.zeros((2, 9), np.float32)
        x[np.arange(2), 1 + el] = 1.0
        x[:, 0] = ELEMENTS[el]
        Q = np.float32(rng.choice([-1.0, 1.0]))
        mols.append((xyz, x, Q))
        if k % 4 == 0:
            mols.append((xyz + FAR, x, Q))
    return mols


def pair_distance(mol):
    """The float64 distance of the float32 coordinates."""
    r = mol[0].astype(np.float64)
    return float(np.sqrt(((r[0] - r[1]) ** 2).sum()))


def u_values():
    """{alpha: u = alpha D of its molecules}, alpha > 0."""
    return {alpha: alpha * np.array([pair_distance(m) for m in two_atom_molecules(kind)]) for alpha, kind in PAIR_ALPHAS.items() if alpha > 0}


def assert_u_coverage():
    """The conditions on u = alpha D, and on D itself: both sides of the cutoff and none within 1e-3 A of it."""
    us = u_values()
    u = np.concatenate(list(us.values()))
    count = lambda lo, hi, closed=False: int(((u >= lo) & ((u <= hi) if closed else (u < hi))).sum())
    decades = {f"1e{k}": count(10.0 ** k, 10.0 ** (k + 1)) for k in range(-3, 2)}
    branch = (count(0.9, 1.0), count(1.0, 1.1, closed=True))
    above = [alpha for alpha, v in us.items() if (v > 10).any()]
    print(f"u = alpha D: {u.min():.1e} .. {u.max():.1e}; per decade from 1e-3 {decades}; {branch[0]} in [0.9, 1), {branch[1]} in [1, 1.1]; above 10 at alpha {above}")
    assert min(decades.values()) >= 8 and min(branch) >= 8 and len(above) > 1
    for kind in ("geometric", "branch", "both"):
        D = np.array([pair_distance(m) for m in two_atom_molecules(kind)])
        assert (np.abs(D - CUTOFF) > 1e-3).all()
        assert kind == "branch" or (D.min() < 0.61 and D.max() > 79.9 and (D < CUTOFF).sum() >= 8 and (D > CUTOFF).sum() >= 8)
        assert all(m[1][0, 0] != m[1][1, 0] and abs(m[2]) == 1 for m in two_atom_molecules(kind))
    return u


def test_the_pairs_cover_u():
    assert_u_coverage()


@pytest.mark.parametrize("alpha", list(PAIR_ALPHAS))
def test_one_pair_per_atom(gpu_engine_factory, alpha):
    """Every two-atom molecule of the call at this alpha: phi, ffix and E within BOUND of their single term, F == ffix + fq and the
    bits of charges_vjp_xyz(g=phi); without a listed pair q == Q / 2 and fq == 0 exactly."""
    mols = two_atom_molecules(PAIR_ALPHAS[alpha])
    batch = _batch(mols)
    offsets, xyz, x, Q = batch
    eng = _engine(gpu_engine_factory, "random")
    q, phi, E, F, ffix, fq = eng.coulomb_xyz(*batch, PAIR_N, ke=KE, alpha=alpha, parts=True)
    assert E.dtype == np.float64 and E.shape == (len(mols),)
    worst = np.zeros((len(mols), 3))
    D = np.array([pair_distance(m) for m in mols])
    for b in range(len(mols)):
        s = slice(2 * b, 2 * b + 2)
        worst[b] = _check_fixed_parts(f"pair {b}, D {D[b]:.4f}, u {alpha * D[b]:.3e}", alpha, xyz[s], Q[b], q[s], phi[s], E[b], F[s], ffix[s], fq[s])
        if D[b] > CUTOFF:
            assert (q[s] == Q[b] / np.float32(2)).all() and not fq[s].any(), (b, D[b])
    k = worst.argmax(0)
    print(f"alpha {alpha}: worst per-pair error phi {worst[k[0], 0]:.2e} at u = {alpha * D[k[0]]:.3e}, ffix {worst[k[1], 1]:.2e} at u = {alpha * D[k[1]]:.3e}, "
          f"E {worst[k[2], 2]:.2e} at u = {alpha * D[k[2]]:.3e} (D = {D[k[0]]:.3f}, {D[k[1]]:.3f}, {D[k[2]]:.3f} A)")
    assert np.array_equal(F, ffix + fq) and F.dtype == np.float32
    q2, gxyz = eng.charges_vjp_xyz(*batch, phi, PAIR_N)
    assert np.array_equal(q2, q) and np.array_equal(fq, -gxyz)


# ---------------------------------------------------------------------------------------------------- 2: packing
def cl_tasks(ns):
    """Mirror of cl_build_tasks (epnn_api_coulomb.hip.h): (first atom, atoms, piece, first partner, end of the partners) per wavefront."""
    off = np.concatenate([[0], np.cumsum(ns)])
    tasks, b, B = [], 0, len(ns)
    while b < B:
        lo, hi = int(off[b]), int(off[b + 1])
        n = hi - lo
        if n <= 64:
            b1 = b + 1
            while b1 < B and off[b1 + 1] - off[b1] <= 64 and off[b1 + 1] - lo <= 64:
                b1 += 1
            tasks.append((lo, int(off[b1]) - lo, 0, lo, int(off[b1])))
            b = b1
            continue
        pieces = _cl_pieces(n)
        length = -(-n // pieces)
        for a0 in range(lo, hi, 64):
            for k in range(pieces):
                p0 = min(lo + k * length, hi)
                tasks.append((a0, min(64, hi - a0), k, p0, min(p0 + length, hi)))
        b += 1
    return tasks


# (composition, N, wavefronts)
PACKED = [((32, 32), 128, 1), ((63, 1), 128, 1), ((33, 31, 1), 128, 2), ((64, 1, 1), 128, 2), ((1, 64), 128, 2), ((20, 20, 20, 20), 128, 2),
          ((1,) * 70, 128, 2), ((65, 3, 61, 64, 2, 130, 40, 24), 136, 12)]
PACKED_IDS = ["32+32", "63+1", "33+31+1", "64+1+1", "1+64", "4x20", "70x1", "mixed"]


def test_the_mirror_packs_as_the_names_say():
    for ns, N, wavefronts in PACKED:
        tasks = cl_tasks(ns)
        assert len(tasks) == wavefronts and max(ns) <= N, ns
        covered = np.zeros(sum(ns), int)
        for a0, na, piece, p0, p1 in tasks:
            assert 1 <= na <= 64
            covered[a0:a0 + na] += piece == 0
        assert (covered == 1).all()
    assert [t[1] for t in cl_tasks((33, 31, 1))] == [64, 1] and [t[1] for t in cl_tasks((1,) * 70)] == [64, 6]
    assert [t[1] for t in cl_tasks((64, 1, 1))] == [64, 2] and [t[1] for t in cl_tasks((1, 64))] == [1, 64]
    assert [t[1] for t in cl_tasks((20,) * 4)] == [60, 20]
    assert [(t[1], t[2]) for t in cl_tasks(PACKED[-1][0])] == [(64, 0), (1, 0), (64, 0), (64, 0), (2, 0), (64, 0), (64, 1), (64, 0), (64, 1), (2, 0), (2, 1), (64, 0)]


def packed_molecules(ns):
    """The lattice molecules of a composition (seeds at which no molecule of two or more atoms has vanishing charges in the reference:
    two atoms of one element at Q = 0 have q = 0 exactly; tests/test_coulomb_ref.py)."""
    return [_lattice_molecule(n, 9, seed=900 + 7 * k + n) for k, n in enumerate(ns)]


def _scratch(eng, ns, ctasks, what):
    """test_gpu_coulomb.test_scratch_follows_the_formula's check of epnn_last_stats after a coulomb call (T = 2, nx = 9)."""
    st = eng.last_stats()
    want = _formula(ns, 9, 2, int(st[0]), ctasks)
    print(f"{what}: {st[0]} pairs, {st[2]} bytes, formula {want} with {ctasks} wavefronts")
    assert st[1] == 0
    assert want <= int(st[2]) < want + 44 * 256


@pytest.mark.parametrize("alpha", [0.0, 0.3])
@pytest.mark.parametrize("ns,N,wavefronts", PACKED, ids=PACKED_IDS)
def test_packed_batches(gpu_engine_factory, ns, N, wavefronts, alpha):
    """Every molecule within BOUND of float64 on its device charges and with the bits of the call on it alone at the same N; lone
    atoms give zeros and q == Q; the scratch is that of the wavefronts the mirror counts."""
    mols = packed_molecules(ns)
    batch = _batch(mols)
    offsets, xyz, x, Q = batch
    eng = _engine(gpu_engine_factory, "random")
    out = eng.coulomb_xyz(*batch, N, ke=KE, alpha=alpha, parts=True)
    assert len(cl_tasks(ns)) == wavefronts
    _scratch(eng, ns, wavefronts, f"{ns}")
    q, phi, E, F, ffix, fq = out
    worst = np.zeros(3)
    for b, n in enumerate(ns):
        a0, a1 = offsets[b], offsets[b + 1]
        worst = np.maximum(worst, _check_fixed_parts(f"{ns}, molecule {b}", alpha, xyz[a0:a1], Q[b], q[a0:a1], phi[a0:a1], E[b], F[a0:a1],
                                                     ffix[a0:a1], fq[a0:a1]))
        alone = eng.coulomb_xyz(np.int32([0, n]), xyz[a0:a1], x[a0:a1], Q[b:b + 1], N, ke=KE, alpha=alpha, parts=True)
        for k, (got, want) in enumerate(zip(alone, (q[a0:a1], phi[a0:a1], E[b:b + 1], F[a0:a1], ffix[a0:a1], fq[a0:a1]))):
            assert np.array_equal(got, want), (b, k)
    print(f"{ns}, alpha {alpha}: worst phi {worst[0]:.2e}, ffix {worst[1]:.2e}, E {worst[2]:.2e} of the absolute sums")
    assert np.array_equal(F, ffix + fq)


# ---------------------------------------------------------------------------------------------------- 3: pieces above 4096 atoms
# atoms: (pieces, partners per piece, partners of the last piece, atoms of the last block)
PIECES = {4100: (32, 129, 101, 4), 8250: (16, 516, 510, 58)}


def test_the_piece_counts():
    for n, (pieces, length, last, tail) in PIECES.items():
        assert _cl_pieces(n) == pieces and -(-n // pieces) == length and n - (pieces - 1) * length == last and n - 64 * ((n - 1) // 64) == tail
        tasks = cl_tasks((n,))
        assert len(tasks) == -(-n // 64) * pieces and tasks[-1] == (64 * ((n - 1) // 64), tail, pieces - 1, n - last, n)
        assert {t[4] - t[3] for t in tasks} == {length, last}
    assert [_cl_pieces(m) for m in (4096, 4097, 4224, 4225, 8193, 16448)] == [32, 32, 32, 31, 16, 8]      # 32 while 2048 / blocks rounds up to it


_LARGE = []


def _engine_large(factory):
    """Weights at scale 0.35: the charges of a cluster of thousands of atoms stay below about 1 (at test_gpu_coulomb._weights' scale
    0.6 they reach 4.5e3 at 4100 atoms and 2e4 at 8250)."""
    if not _LARGE:
        eng = factory(nx=9, T=2)
        eng.set_weights(random_weights(9, 2, seed=5, scale=0.35))
        eng.set_option("grad_path", 2)
        _LARGE.append(eng)
    return _LARGE[0]


@pytest.mark.parametrize("n,alpha", [(4100, 0.0), (4100, 0.3), (8250, 0.3)])
def test_piece_counts_above_4096_atoms(gpu_engine_factory, n, alpha):
    """One lattice cluster whose piece count the limits CL_MAXP and CL_WANT decide: the fixed-charge parts against float64 on the device
    charges (all atoms at 4100; at 8250 the first and the last block of 64 and every eighth atom between), composition bits, scratch."""
    pieces = PIECES[n][0]
    xyz, x, Q = _lattice_molecule(n, 9, seed=n)
    batch = (np.int32([0, n]), xyz, x, np.float32([Q]))
    eng = _engine_large(gpu_engine_factory)
    q, phi, E, F, ffix, fq = eng.coulomb_xyz(*batch, n, ke=KE, alpha=alpha, parts=True)
    _scratch(eng, (n,), -(-n // 64) * pieces, f"{n} atoms")
    assert np.isfinite(q).all() and np.abs(q).max() > 0
    rows = np.arange(n) if n == 4100 else np.unique(np.concatenate([np.arange(64), np.arange(64, n - 64, 8), np.arange(n - 64, n)]))
    phi64, ffix64, sphi, sff = coulomb64_rows(xyz, q, KE, alpha, rows)
    ephi, eff = np.abs(phi[rows] - phi64), np.abs(ffix[rows] - ffix64)
    rp, rf = (ephi / sphi).max(), (eff.max(1) / sff).max()
    assert np.abs(phi64).max() > 0 and (ephi <= BOUND * sphi).all() and (eff <= BOUND * sff[:, None]).all()
    if len(rows) == n:
        E64, sE = 0.5 * float(q.astype(np.float64) @ phi64), 0.5 * float(np.abs(q.astype(np.float64)) @ sphi)
    else:
        try:
            import scipy.special  # noqa: F401
            E64, sE = coulomb_energy64(xyz, q, KE, alpha)
        except ImportError:
            E64 = sE = None
    re = abs(E[0] - E64) / sE if sE else float("nan")
    print(f"{n} atoms, alpha {alpha}, {pieces} pieces, {len(rows)} rows: phi {rp:.2e}, ffix {rf:.2e}, E {re:.2e} of the absolute sums "
          f"(|q| up to {np.abs(q).max():.3f}, |phi| {np.abs(phi64).max():.3e}, |ffix| {np.abs(ffix64).max():.3e})")
    assert sE is None or abs(E[0] - E64) <= BOUND * sE
    assert np.array_equal(F, ffix + fq)
    q2, gxyz = eng.charges_vjp_xyz(*batch, phi, n)
    assert np.array_equal(q2, q) and np.array_equal(fq, -gxyz)
