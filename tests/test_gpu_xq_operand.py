"""The xq operand of the fused kernels' per-atom chains (node mask, one, charge, x: `wave_xq_slot`, epnn_common.h) as a K = 16
bf16 operand: its slot map, and the charges of molecules whose operand has zero second and third pieces (bf16 features, no
charge), none (float32 features, charged) or only the charge's (bf16 features, Q = -1) -- the three kinds a shortcut for zero
pieces would have to tell apart, alone and mixed in one launch.

The GPU tests compare against the float64 oracle; the slot-map test needs no GPU (a host-only C++ unit)."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, random_weights

TOL = 1e-5   # BASELINE.json north_star: charges within 1e-5 absolute per atom
SIZES = (1, 7, 16, 17, 24, 25, 32,      # one wavefront (k_wave_forward) or a block per wavefront (k_wave_forward2<2>)
         33, 48, 49, 64)                # three and four wavefronts (k_wave_forward2<3>, <4>)
ROUTINGS = ({}, {"wave_front": 0}, {"wave2": 0}, {"wave2": 25})


def test_xq_slot_map_holds_every_input_once(tmp_path):
    """wave_xq_slot over the 16 K slots: every index 0 .. nx + 2 of (mask, x[0..nx-1], charge, one) exactly once, everything
    else -1, for every nx the fused kernel takes; mask, one and charge in lane group 0 (xq_charge() rewrites one dword there)."""
    import __graft_entry__ as g
    src = tmp_path / "xq_slot.cpp"
    src.write_text('#include "epnn_common.h"\n#include <stdio.h>\n'
                   "int main() {\n"
                   "    for (int nx = 1; nx <= 13; ++nx) {\n"
                   "        for (int q = 0; q < 4; ++q)\n"
                   '            for (int s = 0; s < 4; ++s) printf("%d ", wave_xq_slot(q, s, nx));\n'
                   '        printf("\\n");\n'
                   "    }\n"
                   "    return 0;\n"
                   "}\n")
    exe = tmp_path / "xq_slot"
    rocm_inc = os.path.join(os.path.dirname(os.path.dirname(g.HIPCC)), "include")
    subprocess.run([g.HIPCC, "-x", "c++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", g.CSRC, "-I", rocm_inc, str(src), "-o", str(exe)],
                   check=True, capture_output=True, timeout=300)
    rows = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=60).stdout.strip().splitlines()
    assert len(rows) == 13
    for nx, row in zip(range(1, 14), rows):
        slots = [int(v) for v in row.split()]
        assert len(slots) == 16
        assert sorted(v for v in slots if v >= 0) == list(range(nx + 3)), (nx, slots)
        assert all(v == -1 for v in slots if v < 0) and slots.count(-1) == 16 - (nx + 3), (nx, slots)
        assert slots[:3] == [0, nx + 2, nx + 1], (nx, slots)          # lane group 0: mask, one, charge


def _grow(rng, n, span_per_atom):
    """n points in a cube, at least 0.7 apart (sequential insertion)."""
    span = max(1.2, span_per_atom * n ** (1.0 / 3.0) * 1.6)
    pts = []
    while len(pts) < n:
        p = rng.uniform(0, span, size=3)
        if all(np.linalg.norm(p - o) > 0.7 for o in pts):
            pts.append(p)
    return np.asarray(pts, dtype=np.float32)


def _is_bf16(a):
    return not np.any(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & 0xFFFF)


def _molecules(nx, seed):
    """Per size three molecules: features that are not bf16 numbers with a total charge (every piece of the operand counts), bf16
    features and no charge (pieces 2 and 3 are zero), bf16 features and Q = -1 (zero pieces but for the charge's)."""
    rng = np.random.default_rng(seed)
    mols, kinds = [], []
    for n in SIZES:
        dense = rng.uniform(0.05, 1.0, size=(n, nx)).astype(np.float32)
        dense.view(np.uint32)[...] |= 0x101                           # (bits in the second AND the third piece of every value)
        small = rng.integers(0, 10, size=(n, nx)).astype(np.float32)  # element numbers / one-hots: bf16 numbers
        small[:, 0] = np.maximum(small[:, 0], 1.0)
        assert not _is_bf16(dense) and _is_bf16(small)
        for kind, x, Q in (("f32 charged", dense, float(rng.choice([-1.0, 1.0]))), ("bf16 neutral", small, 0.0), ("bf16 Q=-1", small.copy(), -1.0)):
            mols.append((_grow(rng, n, float(rng.choice([0.9, 2.2]))), x, Q))
            kinds.append(kind)
    return mols, kinds


def _batch(mols):
    off = np.zeros(len(mols) + 1, dtype=np.int32)
    off[1:] = np.cumsum([m[1].shape[0] for m in mols])
    return (off, np.concatenate([m[0] for m in mols]), np.concatenate([m[1] for m in mols]),
            np.array([m[2] for m in mols], dtype=np.float32))


@pytest.mark.gpu
@pytest.mark.parametrize("nx", range(1, 14))
def test_xq_operand_every_nx_vs_oracle(nx):
    """Every nx the fused kernels take (nx + 3 <= 16; 13 fills all 16 slots) x the sizes at which the column-block layout and the
    kernel change x the three kinds of _molecules, random non-degenerate weights, on every routing of the size test: each kind in a
    launch of its own and all of them mixed in one launch (state that leaked from one wavefront's products into another's would show
    there), against the float64 oracle within max(TOL, 4 x the float32 oracle's own distance from it).  The sizes above 32 are there
    for k_wave_forward2<3>, <4>: they run on the three routings that reach it (without the in-kernel front-end, "wave_front" = 0,
    such molecules take the tiled kernels).  Every molecule must have run on the fused kernels.

    epnn_create takes nx up to 10 (the tiled kernels' feature image); the handles here come from epnn_create_fused, which takes the
    fused kernels' own limit and, above 10, refuses what would leave them -- checked at the end for a 33-atom molecule on "wave_front" 0."""
    from epnn_amd._lib import EpnnError
    from epnn_amd.engine import Engine
    from oracle import epnn_oracle as orc
    T, N = 2, 66
    w = random_weights(nx, T, seed=100 + nx, scale=0.35)
    mols, kinds = _molecules(nx, seed=200 + nx)
    ref = [orc.forward_xyz(xyz, x, Q, w, N=N, dtype=np.float64) for xyz, x, Q in mols]
    ref32 = [orc.forward_xyz(xyz, x, Q, w, N=N, dtype=np.float32) for xyz, x, Q in mols]
    assert all(np.isfinite(r).all() for r in ref)
    noise = max(float(np.abs(a - b).max()) for a, b in zip(ref32, ref))
    bound = max(TOL, 4 * noise)
    launches = [("f32 charged", [k for k, kd in enumerate(kinds) if kd == "f32 charged"]),
                ("bf16 neutral", [k for k, kd in enumerate(kinds) if kd == "bf16 neutral"]),
                ("mixed", list(range(len(mols))))]
    for opts in ROUTINGS:
        eng = Engine(nx=nx, T=T, fused_only=True)
        top = 32 if opts.get("wave_front", 1) == 0 else 64
        try:
            eng.set_weights(w)
            for k, v in opts.items():
                eng.set_option(k, v)
            for name, sel in launches:
                sel = [k for k in sel if mols[k][1].shape[0] <= top]
                off, xyz, x, Q = _batch([mols[k] for k in sel])
                q = eng.forward_xyz(off, xyz, x, Q, N=N)
                st = eng.last_stats()
                assert st[1] == len(sel) and st[2] == 0, (nx, opts, name, st)
                worst, at = 0.0, None
                for i, k in enumerate(sel):
                    n = mols[k][1].shape[0]
                    err = float(np.abs(q[off[i]:off[i + 1]] - ref[k][:n]).max())
                    if not err <= worst:
                        worst, at = err, (n, kinds[k])
                print(f"nx = {nx} {opts} {name}: worst |dq| {worst:.2e} at {at}; float32 oracle noise {noise:.2e}")
                assert worst <= bound, (nx, opts, name, worst, at, noise)
            if nx > 10 and top == 32:
                big = [m for m in mols if m[1].shape[0] == 33][:1]
                with pytest.raises(EpnnError, match="fused kernels only"):
                    eng.forward_xyz(*_batch(big), N=N)
        finally:
            eng.close()
