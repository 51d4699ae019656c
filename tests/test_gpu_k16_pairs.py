"""The K = 16 products of the fused kernels -- the xq block of every projection, the G tiles, the G term of both EPN block forms --
issued as three v_mfma_f32_16x16x32_bf16 instead of six v_mfma_f32_16x16x16_bf16 (w16_mm_bfk16, epnn_common.h; the arithmetic
and the layout: tests/test_k16_pairs_ref.py).

Inputs under which a wrong pairing cannot hide: features are random float32 numbers with bits in every bf16 piece and the total
charges are non-zero and no bf16 numbers, so every xq value has non-zero second and third pieces (one-hot features and neutral
molecules would make z2 = z3 = 0 and half of the terms vanish); edge coordinates are float32 anyway.  Sizes: 1 atom (no pair),
2 atoms, a chain with exactly 16 pairs, 16 atoms (one column block, full), 17 atoms (the second block, 16 copies), a 21..25-atom
molecule of which some pairs have an EPN record and some do not (both block forms in one molecule), 29 atoms, and 40 atoms
(k_wave_forward2<3>, the same helper).  nx = 1 and nx = 13 (the first and the last xq slot) through epnn_create_fused, nx = 9
elsewhere; T = 1 and T = 5.  Everything against the float64 oracle within 1e-5 per atom, the total charge conserved to 1e-4.

Those inputs go with random weights.  The shipped decay_model_weights take part with the same geometries and charges but with the
element rows they were trained on (atomic number and one-hot): on random feature rows they are out of their domain and float32
itself cannot hold the bound -- the float32 NumPy oracle is 6.4e-5 from the float64 one on the 29-atom cluster and 6.9e-5 on the
40-atom one (1.5e-6 and 3.2e-6 on the 17- and 25-atom molecules), so no float32 implementation can be asked for 1e-5 there."""
import os
import re
import subprocess

import numpy as np
import pytest

import micro_tool
from conftest import ROOT, random_weights
from test_gpu_epn_records import _cluster, _line, _pairs, _table_pairs

TOL = 1e-5       # BASELINE.json north_star: charges within 1e-5 absolute per atom
QTOL = 1e-4      # total charge of a molecule
N = 48
CHARGES = (0.7123, -1.3371, 0.3001)          # non-zero, no bf16 numbers: three non-zero pieces each

_CACHE = {}


def _three_pieces(a):
    """Every value has a non-zero first, second and third truncated bf16 piece."""
    x = np.ascontiguousarray(a, dtype=np.float32)
    for _ in range(3):
        top = (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
        if np.any(top == 0):
            return False
        x = x - top
    return True


def _geometries():
    """name -> xyz, the same for every nx."""
    if "geo" not in _CACHE:
        rng = np.random.default_rng(1811)
        geo = {"atoms1": np.zeros((1, 3), dtype=np.float32), "atoms2": _line(1, rng), "pairs16": _line(16, rng),
               "atoms16": _cluster(rng, 16, 4.2), "atoms17": _cluster(rng, 17, 4.2), "atoms29": _cluster(rng, 29, 5.2),
               "atoms40": _cluster(rng, 40, 6.0)}
        # a molecule of 21..25 atoms whose pairs have a record in part (the kernel's LDS arithmetic: test_gpu_epn_records.py)
        for n in (25, 24, 23, 22, 21) * 4:
            xyz = _cluster(rng, n, 5.0)
            if 0 < _table_pairs(n, _pairs(xyz)) < _pairs(xyz):
                geo["part_records"] = xyz
                break
        _CACHE["geo"] = geo
    return _CACHE["geo"]


def _molecules(nx, kind="random"):
    """name -> (xyz, x, Q): dense random feature rows, or (decay_model_weights) element rows as the reference builds them"""
    key = ("mols", nx, kind)
    if key not in _CACHE:
        rng = np.random.default_rng(1900 + nx)
        mols = {}
        for k, (name, xyz) in enumerate(_geometries().items()):
            if kind == "decay":
                z = rng.choice(4, size=len(xyz), p=[0.5, 0.3, 0.1, 0.1])
                x = np.zeros((len(xyz), nx), dtype=np.float32)
                x[:, 0] = np.array([1.0, 6.0, 7.0, 8.0], dtype=np.float32)[z]
                x[np.arange(len(xyz)), 1 + z] = 1.0
            else:
                x = rng.uniform(0.05, 1.0, size=(len(xyz), nx)).astype(np.float32)
                x.view(np.uint32)[...] |= 0x101                        # bits in the second and in the third piece of every value
            mols[name] = (xyz, x, CHARGES[k % 3])
        _CACHE[key] = mols
    return _CACHE[key]


def _weights(kind, nx, T):
    key = ("w", kind, nx, T)
    if key not in _CACHE:
        if kind == "decay":
            from epnn_amd import checkpoint
            _CACHE[key] = checkpoint.load_epnn_weights(os.path.join(ROOT, "models", "decay_model_weights"))
        else:
            _CACHE[key] = random_weights(nx, T, seed=300 + 16 * nx + T, scale=0.35)
    return _CACHE[key]


def _refs(kind, nx, T):
    """name -> float64 oracle charges, computed once per configuration and read-only."""
    key = ("ref", kind, nx, T)
    if key not in _CACHE:
        from oracle import epnn_oracle as orc
        out = {}
        for name, (xyz, x, Q) in _molecules(nx, kind).items():
            r = orc.forward_xyz(xyz, x, Q, _weights(kind, nx, T), N=N, dtype=np.float64)
            assert np.isfinite(r).all()
            r.setflags(write=False)
            out[name] = r
        _CACHE[key] = out
    return _CACHE[key]


def _batch(mols):
    off = np.zeros(len(mols) + 1, dtype=np.int32)
    off[1:] = np.cumsum([m[1].shape[0] for m in mols])
    return (off, np.concatenate([m[0] for m in mols]), np.concatenate([m[1] for m in mols]),
            np.array([m[2] for m in mols], dtype=np.float32))


def test_the_cases_are_what_their_names_say():
    """(no GPU) pair counts 0, exactly 16 and one with a partial last group of 16; the molecule with records for part of its pairs;
    inputs whose every piece is non-zero."""
    geo = _geometries()
    assert [len(geo[k]) for k in ("atoms1", "atoms2", "atoms16", "atoms17", "atoms29", "atoms40")] == [1, 2, 16, 17, 29, 40]
    assert _pairs(geo["atoms1"]) == 0 and _pairs(geo["atoms2"]) == 1 and _pairs(geo["pairs16"]) == 16
    assert "part_records" in geo and 21 <= len(geo["part_records"]) <= 25
    p = _pairs(geo["part_records"])
    assert 0 < _table_pairs(len(geo["part_records"]), p) < p
    assert any(_pairs(geo[k]) % 16 not in (0,) and _pairs(geo[k]) > 16 for k in ("atoms16", "atoms17", "atoms29"))
    for nx in (1, 9, 13):
        for xyz, x, Q in _molecules(nx).values():
            assert _three_pieces(x) and _three_pieces(np.float32(Q)) and _three_pieces(np.float32(Q / len(xyz)))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,nx,T", [("random", 9, 5), ("random", 9, 1), ("random", 1, 5), ("random", 13, 1), ("decay", 9, 5)])
def test_charges_vs_float64_oracle(kind, nx, T):
    """Every molecule in a launch of its own and all of them in one launch, molecules of up to 32 atoms on k_wave_forward ("wave2" 0),
    then those of 17..32 atoms on k_wave_forward2<2> as well ("wave2" 17); the 40-atom molecule runs on k_wave_forward2<3> either way."""
    from epnn_amd.engine import Engine
    mols, refs = _molecules(nx, kind), _refs(kind, nx, T)
    names = list(mols)
    eng = Engine(nx=nx, T=T, fused_only=True)
    try:
        eng.set_weights(_weights(kind, nx, T))
        for wave2, launches in ((0, [[nm] for nm in names] + [names]), (17, [["atoms17", "part_records", "atoms29", "atoms40"]])):
            eng.set_option("wave2", wave2)
            for sel in launches:
                off, xyz, x, Q = _batch([mols[nm] for nm in sel])
                q = eng.forward_xyz(off, xyz, x, Q, N=N)
                st = eng.last_stats()
                assert st[1] == len(sel) and st[2] == 0, (sel, st)              # every molecule on the fused kernels
                for i, nm in enumerate(sel):
                    qi = q[off[i]:off[i + 1]]
                    err = float(np.abs(qi - refs[nm][:len(qi)]).max())
                    dQ = abs(float(qi.astype(np.float64).sum()) - float(np.float32(mols[nm][2])))
                    print(f"{kind} nx = {nx} T = {T} wave2 = {wave2} {nm}{' (mixed)' if len(sel) > 1 else ''}: |dq| {err:.2e}, |sum q - Q| {dQ:.2e}")
                    assert err <= TOL, (kind, nx, T, wave2, nm, err)
                    assert dQ <= QTOL, (kind, nx, T, wave2, nm, dQ)
    finally:
        eng.close()


@pytest.mark.gpu
def test_micro_paired_form_vs_f32_mfma():
    """tools/micro/bf16x6 k16pairs runs w16_split3k16 and w16_mm_bfk16 themselves (epnn_common.h, under the library's flags) on
    their operand strings (w1 w2 | w3 w1; a = z3|z1, b = a's upper half and z2).  On random operands whose three pieces are all non-zero the paired form's error against float64 is
    not above the f32 MFMA's on the same data (the bar the six-instruction form was held to, profiles/r05_micro_bf16x6.txt), and the
    operand's piece words are those of the v_and / v_sub split.  The end-to-end bound of 1e-5 does not see a third piece (truncating
    x to two pieces moves these charges by 1.5e-6 at most): this case does."""
    out = subprocess.run([micro_tool.bf16x6(), "k16pairs"], check=True, capture_output=True, text=True, timeout=120).stdout
    print(out)
    m = re.search(r"paired \(three K = 32 MFMAs\) ([0-9.e+-]+), six K = 16 MFMAs ([0-9.e+-]+), f32 MFMA ([0-9.e+-]+)", out)
    assert m, out
    paired, six, f32 = (float(v) for v in m.groups())
    assert 0.0 < paired <= f32, out
    # Third-piece level: the distance from the six partial products summed exactly.  The accumulator is rounded to float32 three times,
    # half an ulp of the largest |C| each, and the two-term sums inside the instructions are allowed as much again: 3 ulp.  A third
    # piece in the wrong place moves an output by about 2^-15 |w z| per K slot, some 1e-4 on these operands: forty times the bound.
    m = re.search(r"summed in float64\|: paired ([0-9.e+-]+), six K = 16 MFMAs ([0-9.e+-]+)", out)
    big = re.search(r"largest \|C\| ([0-9.]+)", out)
    assert m and big, out
    import math
    ulp = 2.0 ** (math.floor(math.log2(float(big.group(1)))) - 23)
    assert float(m.group(1)) <= 3 * ulp, out
    m = re.search(r"(\d+) of (\d+) piece words differ", out)
    assert m and int(m.group(1)) == 0 and int(m.group(2)) > 0, out
    assert re.search(r"\d+ of \d+ outputs differ in bits from the six-instruction form", out), out
