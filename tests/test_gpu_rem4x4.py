"""The splits' remainders on v_mfma_f32_4x4x4_16b_bf16 (w16_ident / w16_rem, epnn_common.h; the operand placement without a GPU:
tests/test_rem4x4_ref.py).

Two parts.  The micro tool's sub-command (tools/micro/bf16x6 rem4x4): the piece words of a split with these remainders are those of the
v_and / v_sub form on the tool's 2^22 values of every kind, as many values as there are not reproduced by x1 + x2 + x3 (the tiny ones
whose third piece leaves float32's range, in both forms), and a lane's values stay in the lane and in order.  No timing is asserted.

Then every user of the helper at the smallest shapes that reach it, against the float64 oracle at the bound of
tests/test_gpu_f32_grade.py (its K = 4 times the float32 oracle's own noise, rms and max, over the real atoms of one launch; the largest
error also within the standing 1e-5 per atom, which is the tighter of the two for these weights: their charges reach 3.9):
    n = 3, 16, 17, 32   k_wave_forward, one and two column blocks ("wave2" 0), and the same batch on k_wave_forward2<2> (default)
    n = 33, 49          k_wave_forward2 on three and on four wavefronts
    n = 70              the tiled kernels: the tile-workgroup sweep k_lg_sweep2 and the four-tile sweep k_lg_sweep
with decay_model_weights on the element rows they were trained on (on random rows they leave their domain and no float32 bound holds,
profiles/r18_k16_pairs.txt section 5) and total charges whose three pieces are non-zero; the total charge conserved to 1e-4.
test_the_bound_is_the_kernel_s_not_the_oracle_s (no GPU) holds these inputs to what the bound needs: see there."""
import os
import re
import subprocess

import numpy as np
import pytest

import micro_tool
from conftest import ROOT
from test_gpu_f32_grade import CHARGES, K, TOL, _batch, _cluster, rms, three_pieces

QTOL = 1e-4
NX, T = 9, 5
# name -> (atoms of the batch's molecules, padded size, [(route, options, molecules on the fused kernels?)])
BATCHES = {
    "n3_16_17_32": ((3, 16, 17, 32), 34, [("k_wave_forward", {"wave2": 0}, True), ("k_wave_forward2<2>", {"wave2": -1}, True)]),
    "n33_49":      ((33, 49), 50, [("k_wave_forward2<3> and <4>", {}, True)]),
    "n70":         ((70,), 72, [("tiled, k_lg_sweep2", {"large_sweep_old": 0}, False), ("tiled, k_lg_sweep", {"large_sweep_old": 1}, False)]),
}
_CACHE = {}


def _weights():
    if "w" not in _CACHE:
        from epnn_amd import checkpoint
        _CACHE["w"] = checkpoint.load_epnn_weights(os.path.join(ROOT, "models", "decay_model_weights"))
    return _CACHE["w"]


def _molecules(name):
    """[(xyz, x, Q)]: clusters of test_gpu_f32_grade's density, element rows (atomic number, one-hot of H C N O) as the reference builds them."""
    if ("mols", name) not in _CACHE:
        mols = []
        for k, n in enumerate(BATCHES[name][0]):
            rng = np.random.default_rng(2100 + n)
            xyz = _cluster(rng, n)
            z = rng.choice(4, size=n, p=[0.5, 0.3, 0.1, 0.1])
            x = np.zeros((n, NX), dtype=np.float32)
            x[:, 0] = np.array([1.0, 6.0, 7.0, 8.0], dtype=np.float32)[z]
            x[np.arange(n), 1 + z] = 1.0
            mols.append((xyz, x, float(np.float32(CHARGES[k % 3] * (1.0 if n >= 5 else n / 6.0)))))
        _CACHE[("mols", name)] = mols
    return _CACHE[("mols", name)]


def _references(name):
    """(q64, q32) of the batch's real atoms, concatenated: the float64 and the float32 oracle, once per batch and read-only."""
    if ("ref", name) not in _CACHE:
        from oracle import epnn_oracle as orc
        mols, N = _molecules(name), BATCHES[name][1]
        dense = [orc.dense_inputs(xyz, x, np.float32(Q), N) for xyz, x, Q in mols]
        stacked = [np.stack([d[k] for d in dense]) for k in range(5)]
        refs = []
        for dtype in (np.float64, np.float32):
            out = orc.model_forward(*stacked, _weights(), dtype)
            q = np.concatenate([out[b, :len(m[0]), 0] for b, m in enumerate(mols)]).astype(np.float64)
            assert np.isfinite(q).all()
            q.setflags(write=False)
            refs.append(q)
        _CACHE[("ref", name)] = tuple(refs)
    return _CACHE[("ref", name)]


@pytest.mark.parametrize("name", list(BATCHES))
def test_the_bound_is_the_kernel_s_not_the_oracle_s(name):
    """(no GPU) On exactly these inputs the float32 NumPy oracle itself is inside both bounds of the GPU test -- K times its own noise
    (by the factor K, and the noise is not zero: the bound is no equality) and the project's standing 1e-5 per atom -- so a float32
    implementation can hold them and they test the kernels, not the oracle's noise.  (On random feature rows these weights put the
    float32 oracle 6e-5 from the float64 one.)  The inputs have pieces to lose."""
    q64, q32 = _references(name)
    noise_rms, noise_max = rms(q32 - q64), float(np.abs(q32 - q64).max())
    print(f"REM4X4 {name}: float32 oracle noise rms {noise_rms:.2e} max {noise_max:.2e}; largest |q| {np.abs(q64).max():.2f}")
    assert 0.0 < noise_rms and 0.0 < noise_max <= min(K * noise_max, TOL), (name, noise_rms, noise_max)
    for xyz, x, Q in _molecules(name):
        assert three_pieces(np.float32(Q)) and three_pieces(np.float32(Q) / np.float32(len(xyz)))
    assert [len(m[0]) for m in _molecules(name)] == list(BATCHES[name][0])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(BATCHES))
def test_charges_within_float32_noise(name):
    from epnn_amd.engine import Engine
    sizes, N, routes = BATCHES[name]
    mols = _molecules(name)
    q64, q32 = _references(name)
    noise_rms, noise_max = rms(q32 - q64), float(np.abs(q32 - q64).max())
    off, xyz, x, Q = _batch(mols)
    eng = Engine(nx=NX, T=T)
    try:
        eng.set_weights(_weights())
        for route, options, fused in routes:
            for opt, value in options.items():
                eng.set_option(opt, value)
            q = eng.forward_xyz(off, xyz, x, Q, N=N)
            st = eng.last_stats()
            assert (st[1], st[2]) == ((len(mols), 0) if fused else (0, len(mols))), (name, route, st)
            assert q.shape == q64.shape and np.isfinite(q).all()
            err_rms, err_max = rms(q - q64), float(np.abs(q - q64).max())
            print(f"REM4X4 {name} [{route}]: rms {err_rms:.2e} = {err_rms / (K * noise_rms):.3f} of {K} x {noise_rms:.2e}; "
                  f"max {err_max:.2e} = {err_max / (K * noise_max):.3f} of {K} x {noise_max:.2e}")
            assert err_rms <= K * noise_rms, (name, route, err_rms, noise_rms)
            assert err_max <= min(K * noise_max, TOL), (name, route, err_max, noise_max)
            for i, (_, _, Qi) in enumerate(mols):
                dQ = abs(float(q[off[i]:off[i + 1]].astype(np.float64).sum()) - float(np.float32(Qi)))
                assert dQ <= QTOL, (name, route, sizes[i], dQ)
    finally:
        eng.close()


@pytest.mark.gpu
def test_micro_tool_exactness_and_layout():
    out = subprocess.run([micro_tool.bf16x6(), "rem4x4"], check=True, capture_output=True, text=True, timeout=120).stdout
    print(out)
    m = re.search(r"rem4x4 exactness: (\d+) of (\d+) piece words differ", out)
    assert m and int(m.group(1)) == 0 and int(m.group(2)) >= 6_000_000, out
    m = re.search(r"rem4x4 exactness: (\d+) of (\d+) values not reproduced by x1 \+ x2 \+ x3 \(4x4x4 remainders\), (\d+) \(truncated form\)", out)
    assert m and int(m.group(1)) == int(m.group(3)) and int(m.group(2)) == 1 << 22, out
    probes = re.findall(r"^rem4x4 layout: values in lane +(\d+) .*: (\w+)$", out, re.M)
    assert len(probes) >= 4 and len({int(l) // 4 for l, _ in probes}) >= 4 and {int(l) % 4 for l, _ in probes} == {0, 1, 2, 3}, out
    assert all(verdict == "ok" for _, verdict in probes), out
