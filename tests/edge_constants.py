"""Edge constants other than the reference's hard-coded cutoff 3.0 / eta 2.0 / near_tol 1e-5: the named sets the tests use, the
distances at which the reference's near flag flips, and the conditions that make an input a usable case.  Test helper.

The flag of a pair at distance D (charge_gn.py:90-94 on the edge features of :148-161) is

    float32(C(D) * max_k exp(-eta (D - mu_k)^2)) > float32(near_tol),   C = (cos(pi D / cutoff) + 1) / 2,   mu = linspace(0.1, cutoff, h_dim)

With 48 centres 0.06 A apart the maximum over k is nearly 1 and the flag follows C: one flip.  With few centres the maximum dips
between them and the flag is not monotone in D: set C has three flips.  Everything here is written from that expression alone (a
dense scan and a bisection in float64), independently of the library's own table of flips.

A case is usable when (all asserted on the float64 references alone, before the device is consulted)
  * no listed pair sits on a flip: min over the pairs of |max_k e_k / near_tol - 1| >= MARGIN (float32 rounding of e is 6e-8
    relative: two orders of magnitude below);
  * every interval between the flips (and the cutoff) holds at least `least` listed pairs, where the test asks for it;
  * the constants matter: the reference at the set differs from the reference at (3.0, 2.0, 1e-5) with the same weights by more
    than 100 times the comparison's tolerance;
  * derivative cases: at least 70 % of the atoms have a ReLU-kink bracket <= 2e-4 max |ref| (the rule of tests/test_gpu_jvp.py).
"""
from __future__ import annotations

import collections

import numpy as np

import cell_ref

EdgeSet = collections.namedtuple("EdgeSet", "h_dim cutoff eta near_tol")

SET_A = EdgeSet(48, 2.5, 4.0, 1e-5)        # narrow Gaussians: 16 basis vectors do not reach 1e-8, the 48-channel front-end runs by itself
SET_B = EdgeSet(48, 3.4, 1.2, 0.05)        # one flip, well inside the cutoff (2.9119 A)
SET_C = EdgeSet(5, 3.4, 6.0, 0.15)         # three flips (2.1037, 2.2983, 2.5347 A) and the zero-padded model_dim < 48 route
SETS = {"A": SET_A, "B": SET_B, "C": SET_C}
DEFAULT = EdgeSet(48, 3.0, 2.0, 1e-5)      # the reference's own constants

MARGIN = 1e-5
KINK_SHARE = 0.70


def engine_kwargs(s):
    """Engine(...) keywords of a set."""
    return dict(h_dim=s.h_dim, e_dim=s.h_dim, cutoff=s.cutoff, eta=s.eta, near_tol=s.near_tol)


def ref_kwargs(s):
    """The references' keywords of a set (those that take h_dim)."""
    return dict(h_dim=s.h_dim, cutoff=s.cutoff, eta=s.eta, near_tol=s.near_tol)


def e_max(D, h_dim, cutoff, eta):
    """max_k e_k of pairs at the float64 distances D (0 < D; 0 from the cutoff on), float64."""
    D = np.asarray(D, dtype=np.float64)
    mu = np.linspace(0.1, cutoff, num=h_dim)
    C = (np.cos(np.pi * D / cutoff) + 1.0) / 2.0
    C = np.where(D >= cutoff, 0.0, C)
    return C * np.exp(-eta * (D[..., None] - mu) ** 2).max(-1)


def flag(D, h_dim, cutoff, eta, near_tol):
    """The reference's float32 decision for pairs at the distances D."""
    return e_max(D, h_dim, cutoff, eta).astype(np.float32) > np.float32(near_tol)


def near_flips(h_dim, cutoff, eta, near_tol, step=1e-4):
    """The distances in (0, cutoff) at which the flag changes, ascending: a scan at `step` (far below the 0.06 A spacing of the
    closest centres the tests use) finds the brackets, a bisection on the float32 decision narrows each to 1e-13."""
    grid = np.arange(step, cutoff, step)
    grid = np.append(grid, np.nextafter(cutoff, 0.0))
    f = flag(grid, h_dim, cutoff, eta, near_tol)
    flips = []
    for k in np.nonzero(f[1:] != f[:-1])[0]:
        lo, hi, flo = grid[k], grid[k + 1], f[k]
        while hi - lo > 1e-13:
            mid = 0.5 * (lo + hi)
            if flag(mid, h_dim, cutoff, eta, near_tol) == flo:
                lo = mid
            else:
                hi = mid
        flips.append(0.5 * (lo + hi))
    return np.array(flips)


def listed_distances(xyz, cutoff, cell=None):
    """Float64 distances (the cell's image rule; None: an open molecule) of the pairs i < j under the cutoff."""
    r = np.asarray(xyz, dtype=np.float32).astype(np.float64)
    c = np.zeros((3, 3), np.float32) if cell is None else np.asarray(cell, np.float32).reshape(3, 3)
    D = cell_ref._dist(cell_ref.mic(r[None, :, :] - r[:, None, :], c))
    iu = np.triu_indices(r.shape[0], 1)
    D = D[iu]
    return D[D < cutoff]


def pair_counts(xyz, s, cell=None):
    """(listed, near) pairs i < j of one molecule as the reference decides them."""
    D = listed_distances(xyz, s.cutoff, cell)
    return int(D.size), int(flag(D, *s).sum())


def margin(xyz, s, cell=None):
    """min over the listed pairs of |max_k e_k / near_tol - 1| (inf without pairs)."""
    D = listed_distances(xyz, s.cutoff, cell)
    if D.size == 0:
        return np.inf
    return float(np.abs(e_max(D, s.h_dim, s.cutoff, s.eta) / s.near_tol - 1.0).min())


def interval_counts(xyz, s, cell=None):
    """Listed pairs in each interval between 0, the flips and the cutoff."""
    D = listed_distances(xyz, s.cutoff, cell)
    edges = np.concatenate([[0.0], near_flips(*s), [s.cutoff]])
    return np.histogram(D, edges)[0]


def assert_admissible(mols, s, cells=None, least=0, what=""):
    """The first two conditions for every molecule (xyz first in each tuple); prints and returns (margin, interval counts)."""
    cells = [None] * len(mols) if cells is None else cells
    m = min(margin(mol[0], s, c) for mol, c in zip(mols, cells))
    counts = sum(interval_counts(mol[0], s, c) for mol, c in zip(mols, cells))
    print(f"{what}: margin to the nearest flip {m:.1e}, listed pairs per flag interval {' / '.join(str(int(c)) for c in counts)}")
    assert m >= MARGIN, (what, m)
    assert (counts >= least).all(), (what, counts, least)
    return m, counts


def assert_sensitive(ref_set, ref_default, tol, what=""):
    """The third condition: the reference at the set against the reference at the default constants."""
    d = float(np.abs(np.asarray(ref_set) - np.asarray(ref_default)).max())
    print(f"{what}: the set against the reference's constants {d:.2e} ({d / tol:.0f} times the tolerance {tol:.1e})")
    assert d > 100 * tol, (what, d, tol)
    return d


def kink_share(ref, kink):
    """(share of the atoms with kink_i <= 2e-4 max |ref|, largest bracket / scale)."""
    scale = np.abs(ref).max()
    return float(np.mean(kink <= 2e-4 * scale)), float(kink.max() / scale)


def assert_derivative_case(ref, kink, ref_default, what=""):
    """The conditions of a derivative case, ref and kink per component (or per atom): the kink rule, and the sensitivity measured
    against the bounds the comparisons really grant.  Returns (sensitivity over all components / (2e-4 scale + largest bracket),
    sensitivity over the components inside the bracket / their largest bound 4e-4 scale): a test with one bound for the whole array
    asks the first to exceed 100, a test with a bound per component the second."""
    ref, kink, ref_default = (np.asarray(a, dtype=np.float64) for a in (ref, kink, ref_default))
    scale = np.abs(ref).max()
    share, worst = kink_share(ref, kink)
    inside = kink <= 2e-4 * scale
    diff = np.abs(ref - ref_default)
    whole = float(diff.max() / (2e-4 * scale + kink.max()))
    tight = float(diff[inside].max() / (4e-4 * scale)) if inside.any() else 0.0
    print(f"{what}: {100 * share:.0f} % of the components within the bracket, largest bracket / scale {worst:.2e}; the set against the "
          f"reference's constants: {whole:.0f} times the whole array's bound, {tight:.0f} times the bound of the components inside")
    assert scale > 0 and share >= KINK_SHARE, (what, share)
    return whole, tight
