"""The float64 reference for bonded exclusions and pair scaling (tests/coulomb_excl_ref.py) against what is known without it: forces
and strain as central differences of its own energy, factor 1 everywhere, one excluded pair in a two-atom cell, the list rule's
counts, and engine.bonded_exclusions against a brute-force breadth-first search.  CPU only."""
import numpy as np
import pytest

import cell_ref
from coulomb_excl_ref import add_correction, coulomb64_w, excl_correction64, exclusion_cases, list_stats, pair_shifts, shuffled
from coulomb_ref import coulomb64, kappa64
from ewald_ref import ewald64
from test_ewald_ref import SHEARED, _system, _tight

KE = 14.4


def _cell_case(n=8, seed=5):
    xyz, q = _system(n, SHEARED, seed)
    pairs, scale = exclusion_cases(xyz, SHEARED, near=3.4, most=2)
    assert len(pairs) >= 4 and len(set(scale.tolist())) == 3
    return xyz, q, pairs, scale


def _ewald_w(xyz, q, cell, alpha, par, pairs, scale):
    return add_correction(ewald64(xyz, q, cell, KE, alpha, *par), excl_correction64(xyz, q, cell, KE, alpha, pairs, scale), q)


@pytest.mark.parametrize("alpha", [0.0, 0.8, 0.2])
def test_forces_and_strain_are_central_differences_of_the_energy(alpha):
    """As tests/test_ewald_ref.py holds ewald64: steps of 1e-5, within 1e-6 of the largest component; open molecule and cell."""
    cell = SHEARED.astype(np.float64)
    xyz, q, pairs, scale = _cell_case()
    par = _tight(cell, alpha)
    h = 1e-5
    for E, ref in ((lambda r, c: _ewald_w(r, q, c, alpha, par, pairs, scale).E, _ewald_w(xyz, q, cell, alpha, par, pairs, scale)),
                   (lambda r, c: coulomb64_w(r, q, KE, alpha, pairs, scale)[1], None)):
        ffix = ref.ffix if ref is not None else coulomb64_w(xyz, q, KE, alpha, pairs, scale)[2]
        fd = np.zeros_like(xyz)
        for i in range(xyz.shape[0]):
            for c in range(3):
                d = np.zeros_like(xyz)
                d[i, c] = h
                fd[i, c] = -(E(xyz + d, cell) - E(xyz - d, cell)) / (2 * h)
        assert np.abs(fd - ffix).max() <= 1e-6 * np.abs(ffix).max(), np.abs(fd - ffix).max()
        assert np.abs(ffix.sum(0)).max() <= 1e-10 * np.abs(ffix).max()
        if ref is None:
            continue
        sd = np.zeros((3, 3))
        for a in range(3):
            for b in range(3):
                eps = np.zeros((3, 3))
                eps[a, b] = h
                up, dn = np.eye(3) + eps, np.eye(3) - eps
                sd[a, b] = (E(xyz @ up.T, cell @ up.T) - E(xyz @ dn.T, cell @ dn.T)) / (2 * h)
        assert np.abs(sd - ref.strain).max() <= 1e-6 * np.abs(ref.strain).max(), np.abs(sd - ref.strain).max()
        assert np.abs(ref.strain - ref.strain.T).max() <= 1e-12 * np.abs(ref.strain).max()


@pytest.mark.parametrize("alpha", [0.0, 0.8])
def test_factor_one_everywhere_reproduces_the_plain_references(alpha):
    cell = SHEARED.astype(np.float64)
    xyz, q, pairs, _ = _cell_case()
    par = _tight(cell, alpha)
    plain, w = ewald64(xyz, q, cell, KE, alpha, *par), _ewald_w(xyz, q, cell, alpha, par, pairs, 1.0)
    for name in ("phi", "E", "ffix", "strain"):
        assert np.array_equal(np.asarray(getattr(plain, name)), np.asarray(getattr(w, name))), name
    assert all(np.array_equal(w.s_phi[p], plain.s_phi[p]) for p in plain.s_phi)
    for a, b in zip(coulomb64(xyz, q, KE, alpha), coulomb64_w(xyz, q, KE, alpha, pairs, np.ones(len(pairs)))):
        assert np.array_equal(np.asarray(a), np.asarray(b))
    # and no list at all
    for a, b in zip(coulomb64(xyz, q, KE, alpha), coulomb64_w(xyz, q, KE, alpha, np.zeros((0, 2), dtype=np.int32), np.zeros(0))):
        assert np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("alpha", [0.0, 0.8])
def test_a_two_atom_cell_with_its_pair_excluded(alpha):
    cell = SHEARED.astype(np.float64)
    xyz = np.array([[0.4, 0.3, 0.2], [6.8, 0.8, 0.6]])                          # nearest through an image
    q = np.array([0.6, -0.35])
    par = _tight(cell, alpha)
    d = cell_ref.mic64(xyz[0] - xyz[1], *cell_ref.duals64(cell))
    D = float(np.sqrt((d * d).sum()))
    assert D < 2.0 and np.abs(pair_shifts(xyz, SHEARED, [[0, 1]])).sum() >= 1
    plain, w = ewald64(xyz, q, cell, KE, alpha, *par), _ewald_w(xyz, q, cell, alpha, par, [[0, 1]], 0.0)
    want = plain.E - KE * q[0] * q[1] * float(kappa64(np.float64(D), alpha)[0])
    assert abs(w.E - want) <= 1e-13 * (abs(plain.E) + abs(want))
    # the yardstick counts the pair's term twice: added by the sum over all pairs, taken away by the correction
    c = excl_correction64(xyz, q, cell, KE, alpha, [[1, 0]], 0.0)
    assert c.s_E == pytest.approx(abs(KE * q[0] * q[1] * float(kappa64(np.float64(D), alpha)[0])), rel=1e-13)
    assert w.s_E["real"] == pytest.approx(plain.s_E["real"] + c.s_E, rel=1e-13)


def test_all_pairs_excluded_leaves_nothing():
    xyz, q = _system(9, SHEARED, 7)
    pairs = np.array([(i, j) for i in range(9) for j in range(i + 1, 9)])
    phi, E, ffix, sp, sf = coulomb64_w(xyz, q, KE, 0.3, pairs, 0.0)
    plain = coulomb64(xyz, q, KE, 0.3)
    assert np.abs(phi).max() <= 1e-13 * sp.max() and abs(E) <= 1e-13 * sp.max() and np.abs(ffix).max() <= 1e-13 * sf.max()
    assert np.allclose(sp, 2 * plain[3], rtol=1e-13) and np.allclose(sf, 2 * plain[4], rtol=1e-13)


def test_the_list_rule():
    """The counts the GPU tests lean on, on the cells of tests/test_gpu_coulomb_cell.py, and the shuffle."""
    cells = {"cube8": np.diag(np.float32([8, 8, 8])), "sheared": SHEARED, "slab": np.diag(np.float32([6, 6, 20])),
             "cube14": np.diag(np.float32([14, 14, 14]))}
    want = {("cube8", 2): (1, 1, 0, 0), ("sheared", 17): (12, 4, 3, 5), ("cube8", 63): (128, 12, 2, 42), ("sheared", 64): (191, 12, 1, 58),
            ("slab", 65): (100, 8, 5, 30), ("cube14", 129): (96, 12, 26, 14)}
    for (c, n), w in want.items():
        xyz = cell_ref.random_cell(np.random.default_rng(n), n, cells[c])
        pairs, scale = exclusion_cases(xyz, cells[c])
        most, none = list_stats(n, pairs)
        assert (len(pairs), most, none, int((np.abs(pair_shifts(xyz, cells[c], pairs)).sum(1) > 0).sum())) == w, (c, n)
        assert (pairs[:, 0] < pairs[:, 1]).all() and len({tuple(p) for p in pairs.tolist()}) == len(pairs)
        assert n < 3 or (pairs != n - 1).all()
        p2, s2 = shuffled(pairs, scale)
        back = {tuple(sorted(p)): s for p, s in zip(p2.tolist(), s2.tolist())}
        assert back == {tuple(p): s for p, s in zip(pairs.tolist(), scale.tolist())}
        assert n < 17 or ((p2[:, 0] > p2[:, 1]).any() and not np.array_equal(np.sort(p2, 1), pairs))
    assert len(exclusion_cases(np.zeros((1, 3)))[0]) == 0


# ---------------------------------------------------------------------------------------------------- bonded_exclusions
def _bfs(bonds, n, factors):
    adj = [set() for _ in range(n)]
    for a, b in bonds:
        adj[a].add(b)
        adj[b].add(a)
    out = {}
    for s in range(n):
        dist = {s: 0}
        layer = [s]
        for depth in (1, 2, 3):
            nxt = []
            for u in layer:
                for v in sorted(adj[u]):
                    if v not in dist:
                        dist[v] = depth
                        nxt.append(v)
            layer = nxt
        for v, dv in dist.items():
            if v > s and factors[dv - 1] != 1.0:
                out[s, v] = factors[dv - 1]
    keys = sorted(out)
    return np.array(keys, dtype=np.int32).reshape(-1, 2), np.array([out[k] for k in keys], dtype=np.float32)


GRAPHS = {
    "chain6": ([(k, k + 1) for k in range(5)], 6),
    "ring4": ([(0, 1), (1, 2), (2, 3), (3, 0)], 4),
    "ring5": ([(0, 1), (1, 2), (2, 3), (3, 4), (4, 0)], 5),
    "two molecules": ([(0, 1), (1, 2), (2, 3), (3, 4), (6, 5), (7, 6), (8, 6), (9, 8)], 11),
    "empty": ([], 4),
    "duplicate bond": ([(0, 1), (1, 0), (1, 2), (0, 1), (2, 3)], 4),
}


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_bonded_exclusions_against_breadth_first_search(name):
    from epnn_amd.engine import bonded_exclusions
    bonds, n = GRAPHS[name]
    for factors in ((0.0, 0.0, 0.5), (0.0, 0.25, 0.8333), (0.0, 0.0, 1.0), (1.0, 0.0, 0.5)):
        pairs, scale = bonded_exclusions(np.array(bonds, dtype=np.int64).reshape(-1, 2), n, *factors)
        wp, ws = _bfs(bonds, n, factors)
        assert pairs.shape == wp.shape and np.array_equal(pairs, wp) and np.array_equal(scale, ws), (name, factors)
        assert pairs.dtype == np.int32 and scale.dtype == np.float32
    if name == "ring4":                                          # opposite corners: 1-3 by either way round, never 1-4
        pairs, scale = bonded_exclusions(bonds, n)
        assert len(pairs) == 6 and not scale.any()
    if name == "ring5":                                          # every pair is 1-2 or 1-3: the 1-4 way round is the longer one
        pairs, scale = bonded_exclusions(bonds, n, 0.0, 0.0, 0.5)
        assert len(pairs) == 10 and not scale.any()
    if name == "chain6":
        pairs, scale = bonded_exclusions(bonds, n)
        assert len(pairs) == 12 and sorted(scale.tolist()).count(0.5) == 3
    if name == "two molecules":
        pairs, _ = bonded_exclusions(bonds, n)
        assert not ((pairs[:, 0] < 5) & (pairs[:, 1] >= 5)).any() and (pairs != 10).all()
