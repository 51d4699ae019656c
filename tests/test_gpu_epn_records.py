"""The per-pair operand table of the fused kernel's EPN blocks (k_wave_forward with the in-kernel front-end, epnn_wave.hip.h):
the bf16 pieces of a pair's edge coordinates, its row addresses and its transfer-matrix store addresses are built once per
molecule and serve every EPN step; pairs whose record does not fit the wavefront's LDS run from their f32 rows as before.

The cases are the smallest at which that code can go wrong: pair counts around the block size of 16, the second column block
(16 / 17 atoms), molecules whose table fits entirely, partly and not at all (by the kernel's own LDS arithmetic, repeated
here), a pair under the cutoff but beyond the near tolerance (weight 0: its entry is never stored) and total charges 0, +1
and -1.  Everything is compared with the float64 oracle within 1e-5 per atom; the float32 oracle's own distance from it is
printed next to the figure.  The two fused kernels must agree to the bit wherever they did before (test_both_fused_kernels_same_bits)."""
import os

import numpy as np
import pytest

from conftest import ROOT, random_weights

TOL = 1e-5   # BASELINE.json north_star: charges within 1e-5 absolute per atom
NX, N = 9, 32
CUTOFF = 3.0
PST, DMS = 36, 36       # EPNN_PST, the transfer matrix' row stride


def _lds_words(wave_lds):
    return (min(max(wave_lds, 16384), 65536) & ~15) // 4


def _epn_free_words(n, wave_lds=20480):
    """Words of the wavefront's LDS budget above the EPN layout's tables (eij | R | P | transfer matrix) of an n-atom molecule."""
    eij_n = n * (n - 1) // 2
    o_r = (((eij_n + 1) >> 1) + 3) & ~3
    o_x = o_r + n * PST
    return _lds_words(wave_lds) - (o_x + n * (PST + DMS))


def _table_pairs(n, pairs, wave_lds=20480):
    """Pairs of the molecule that get a record (16 words in place of the pair's f32 row, 16 more below the rows): all of them, or
    whole blocks of 16 as far as the room below the f32 rows goes."""
    free = _epn_free_words(n, wave_lds)
    rows = min(pairs, free // 16)
    fit = min(rows, max(0, free - 16 * rows) // 16)
    return pairs if fit >= pairs else fit & ~15


def _pairs(xyz, lo=0.0, hi=CUTOFF):
    d = np.linalg.norm(xyz.astype(np.float64)[:, None, :] - xyz.astype(np.float64)[None, :, :], axis=-1)
    iu = np.triu_indices(len(xyz), 1)
    return int(np.count_nonzero((d[iu] >= lo) & (d[iu] < hi)))


def _line(pairs, rng):
    """Atoms along x with `pairs` contacts under the cutoff: gaps of 1.4 (two in a row: a second-neighbour contact at 2.8) and
    then gaps of 1.7 (1.4 + 1.7 and 1.7 + 1.7 are beyond the cutoff), a little off the axis."""
    if pairs == 0:
        return np.zeros((1, 3), dtype=np.float32)
    if pairs == 1:
        m, a = 2, 1
    else:
        m = (pairs + 4) // 2            # (m - 1) + (a - 1) = pairs with a <= m - 1
        a = pairs - (m - 1) + 1
    gaps = [1.4] * a + [1.7] * (m - 1 - a)
    xyz = np.zeros((m, 3))
    xyz[1:, 0] = np.cumsum(gaps)
    xyz[:, 1:] = rng.uniform(-0.04, 0.04, size=(m, 2))
    xyz = xyz.astype(np.float32)
    assert _pairs(xyz) == pairs, (pairs, _pairs(xyz))
    return xyz


def _cluster(rng, n, span):
    """n points in a cube of edge `span`, at least 1.0 apart (bonded hydrogens are about that close)."""
    pts = []
    while len(pts) < n:
        p = rng.uniform(0, span, size=3)
        if all(np.linalg.norm(p - o) > 1.0 for o in pts):
            pts.append(p)
    return np.asarray(pts, dtype=np.float32)


def _features(rng, n):
    """(element rows as the reference builds them -- atomic number and one-hot of H, C, N, O, what decay_model_weights was trained
    on --, dense float32 rows whose every bf16 piece is non-zero, for the random weights)"""
    z = rng.choice(4, size=n, p=[0.5, 0.3, 0.1, 0.1])
    elem = np.zeros((n, NX), dtype=np.float32)
    elem[:, 0] = np.array([1.0, 6.0, 7.0, 8.0], dtype=np.float32)[z]
    elem[np.arange(n), 1 + z] = 1.0
    return elem, rng.uniform(0.05, 1.0, size=(n, NX)).astype(np.float32)


def _build_cases():
    rng = np.random.default_rng(1507)
    cases = {}
    charges = (0.0, 1.0, -1.0)
    for k, p in enumerate((0, 1, 15, 16, 17, 32, 33)):
        xyz = _line(p, rng)
        cases[f"pairs{p}"] = (xyz, _features(rng, len(xyz)), charges[k % 3])
    for k, n in enumerate((16, 17)):
        xyz = _cluster(rng, n, 4.2)
        cases[f"atoms{n}"] = (xyz, _features(rng, n), charges[(k + 1) % 3])
    for k, n in enumerate((29, 32)):
        xyz = _cluster(rng, n, 5.2)
        cases[f"dense{n}"] = (xyz, _features(rng, n), charges[(k + 1) % 3])
    xyz = _cluster(rng, 20, 4.4)
    cases["mid20"] = (xyz, _features(rng, 20), 1.0)
    xyz = _cluster(rng, 25, 5.0)
    cases["mid25"] = (xyz, _features(rng, 25), 0.0)
    # a pair under the cutoff but beyond the near flip (6.0e-3 below the cutoff): listed, weight 0
    xyz = np.array([[0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [1.5, 2.997, 0.0], [0.2, -1.3, 0.4]], dtype=np.float32)
    cases["far_near"] = (xyz, _features(rng, 4), -1.0)
    return cases


_CACHE = {}


def _cases():
    if "cases" not in _CACHE:
        _CACHE["cases"] = _build_cases()
    return _CACHE["cases"]


def _weights(kind):
    """(weights, T): the shipped decay_model_weights, or random non-degenerate ones (every term of the path exercised)."""
    if kind not in _CACHE:
        if kind == "decay":
            from epnn_amd import checkpoint
            _CACHE[kind] = (checkpoint.load_epnn_weights(os.path.join(ROOT, "models", "decay_model_weights")), 5)
        else:
            _CACHE[kind] = (random_weights(NX, 3, seed=77, scale=0.35), 3)
    return _CACHE[kind]


def _refs(kind):
    """name -> (float64 oracle charges, float32 oracle's distance from them), computed once per kind of weights."""
    key = "ref_" + kind
    if key not in _CACHE:
        from oracle import epnn_oracle as orc
        w, _ = _weights(kind)
        out = {}
        for name in _cases():
            xyz, x, Q = _mol(kind, name)
            r64 = orc.forward_xyz(xyz, x, Q, w, N=N, dtype=np.float64)
            r32 = orc.forward_xyz(xyz, x, Q, w, N=N, dtype=np.float32)
            assert np.isfinite(r64).all()
            r64.setflags(write=False)
            out[name] = (r64, float(np.abs(r32 - r64).max()))
        _CACHE[key] = out
    return _CACHE[key]


def _mol(kind, name):
    xyz, (x_elem, x_dense), Q = _cases()[name]
    return xyz, (x_elem if kind == "decay" else x_dense), Q


def _batch(mols):
    off = np.zeros(len(mols) + 1, dtype=np.int32)
    off[1:] = np.cumsum([m[1].shape[0] for m in mols])
    return (off, np.concatenate([m[0] for m in mols]), np.concatenate([m[1] for m in mols]),
            np.array([m[2] for m in mols], dtype=np.float32))


def _engine(kind, **opts):
    from epnn_amd.engine import Engine
    w, T = _weights(kind)
    eng = Engine(nx=NX, T=T)
    eng.set_weights(w)
    eng.set_option("wave2", 0)          # every molecule of up to 32 atoms on k_wave_forward
    for k, v in opts.items():
        eng.set_option(k, v)
    return eng


def _check(eng, kind, names, pairs=None):
    cases, refs = _cases(), _refs(kind)
    off, xyz, x, Q = _batch([_mol(kind, nm) for nm in names])
    q = eng.forward_xyz(off, xyz, x, Q, N=N)
    st = eng.last_stats()
    assert st[1] == len(names) and st[2] == 0, (names, st)
    if pairs is not None:
        assert st[0] == pairs, (names, st, pairs)
    for i, nm in enumerate(names):
        n = cases[nm][0].shape[0]
        ref, noise = refs[nm]
        err = float(np.abs(q[off[i]:off[i + 1]] - ref[:n]).max())
        print(f"{kind} {nm}: |dq| {err:.2e}, float32 oracle noise {noise:.2e}")
        assert err <= TOL, (kind, nm, err, noise)
    return q


def test_layout_arithmetic_of_the_cases():
    """The cases are what their names say (no GPU): the dense clusters cannot hold a record per pair, the 20-atom molecule holds
    all of them in the default budget and only part of them, in whole blocks, in the smallest one."""
    cases = _cases()
    for nm in ("dense29", "dense32"):
        xyz = cases[nm][0]
        n, p = len(xyz), _pairs(xyz)
        assert 28 * p > _epn_free_words(n) and _table_pairs(n, p) < p, (nm, p, _epn_free_words(n))
    xyz = cases["mid20"][0]
    p = _pairs(xyz)
    assert _table_pairs(20, p) == p, p
    part = _table_pairs(20, p, 16384)
    assert 0 < part < p and part % 16 == 0, (p, part)
    xyz = cases["mid25"][0]                       # (the default budget holds its rows and records for some of its blocks)
    part = _table_pairs(25, _pairs(xyz))
    assert 0 < part < _pairs(xyz) and part % 16 == 0, (_pairs(xyz), part)
    for nm in ("atoms16", "atoms17"):
        xyz = cases[nm][0]
        assert _table_pairs(len(xyz), _pairs(xyz)) == _pairs(xyz) > 16
    xyz = cases["far_near"][0]
    assert _pairs(xyz) == _pairs(xyz, 0.0, CUTOFF - 6.0e-3) + 1        # one listed pair beyond the near flip


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["decay", "random"])
def test_pair_counts_around_the_block_size(kind):
    """0, 1, 15, 16, 17, 32 and 33 pairs (blocks of 16; the pipeline's prologue, its loop and its odd last block), each molecule in
    a launch of its own with the listed pairs counted by the library, then all of them in one launch."""
    eng = _engine(kind)
    try:
        names = [f"pairs{p}" for p in (0, 1, 15, 16, 17, 32, 33)]
        for nm, p in zip(names, (0, 1, 15, 16, 17, 32, 33)):
            _check(eng, kind, [nm], pairs=p)
        _check(eng, kind, names, pairs=114)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["decay", "random"])
def test_second_column_block_and_weight_zero_pairs(kind):
    """16 and 17 atoms (the second column block and its own1 stores), and the molecule with a listed pair beyond the near tolerance
    whose transfer-matrix entries must stay unwritten; total charges 0, +1 and -1 among them."""
    eng = _engine(kind)
    try:
        cases = _cases()
        assert {cases[nm][2] for nm in ("atoms16", "atoms17", "far_near", "pairs0")} == {0.0, 1.0, -1.0}
        for nm in ("atoms16", "atoms17", "far_near"):
            _check(eng, kind, [nm], pairs=_pairs(cases[nm][0]))
        _check(eng, kind, ["atoms17", "far_near", "pairs0", "atoms16"])
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["decay", "random"])
@pytest.mark.parametrize("wave_lds", [20480, 16384])
def test_table_that_does_not_fit(kind, wave_lds):
    """Dense 29- and 32-atom clusters (no room for a record per pair: test_layout_arithmetic_of_the_cases) alone and mixed with small
    molecules, in the default LDS budget (where the 25-atom molecule runs its first blocks from records and the others from f32 rows)
    and in the smallest one, where the 20-atom and the 17-atom molecule overflow as well."""
    eng = _engine(kind, wave_lds=wave_lds)
    try:
        for nm in ("dense32", "dense29", "mid25", "mid20"):
            _check(eng, kind, [nm], pairs=_pairs(_cases()[nm][0]))
        _check(eng, kind, ["pairs17", "dense32", "mid20", "pairs0", "dense29", "atoms17", "mid25", "pairs33"])
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["decay", "random"])
def test_both_fused_kernels_same_bits(kind):
    """Molecules of 17..32 atoms: k_wave_forward ("wave2" = 0) and k_wave_forward2 ("wave2" = 17) on the same handle give the same
    bits -- the records hold the pieces the other kernel still splits every step.

    That holds wherever the two kernels add up a message sum in the same order: with the shipped weights (collapsed GNN) at every
    size, with a live GNN from 25 atoms on.  At 17..24 atoms k_wave_forward's second column block holds two or more copies of each
    atom and deals the partners among them, so its message sums are added in another order than k_wave_forward2's: the charges
    then differ in the last bits (measured: up to 1.5e-8 on charges of up to 0.12, by the same amounts before and after the records
    were introduced).  What is asserted there is the bound of such a reordering, 32 float32 terms: 32 x 2^-24 of the largest charge."""
    rng = np.random.default_rng(2932)
    geo = [(_cluster(rng, n, float(rng.choice([4.4, 5.4]))), _features(rng, n), float(rng.choice([-1.0, 0.0, 1.0]))) for n in range(17, 33)]
    mols = [(g[0], g[1][0 if kind == "decay" else 1], g[2]) for g in geo]
    off, xyz, x, Q = _batch(mols)
    eng = _engine(kind)
    try:
        q0 = eng.forward_xyz(off, xyz, x, Q, N=N).copy()
        eng.set_option("wave2", 17)
        q1 = eng.forward_xyz(off, xyz, x, Q, N=N).copy()
        st = eng.last_stats()
        assert st[1] == len(mols) and st[2] == 0, st
        assert np.isfinite(q0).all()
        diff = [float(np.abs(q0[off[i]:off[i + 1]] - q1[off[i]:off[i + 1]]).max()) for i in range(len(mols))]
        print(f"{kind}: largest difference between the kernels per size 17..32: {['%.1e' % d for d in diff]}")
        same_from = 17 if kind == "decay" else 25
        assert np.array_equal(q0[off[same_from - 17]:], q1[off[same_from - 17]:]), diff
        assert max(diff) <= 32 * 2.0 ** -24 * float(np.abs(q0).max()), diff
    finally:
        eng.close()
