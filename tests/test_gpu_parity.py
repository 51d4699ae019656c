"""Parity of the HIP path (through the C ABI) against the golden vectors and the CPU oracle. GPU only."""
import os

import numpy as np
import pytest

from conftest import load_molecules, random_weights

pytestmark = pytest.mark.gpu

TOL = 1e-5   # BASELINE.json north_star: charges within 1e-5 absolute per atom


def test_val_golden_small(gpu_engine_factory, weights_decay, val_dir, val_names, val_gold):
    """Every validation system with n <= 32 atoms (fused kernel) vs the stored TensorFlow predictions (N=41)."""
    eng = gpu_engine_factory(nx=9, T=5)
    eng.set_weights(weights_decay)
    mols, offsets, xyz, x, Q = load_molecules(val_dir, val_names)
    sel = [i for i, m in enumerate(mols) if m[1].shape[0] <= 32]
    assert len(sel) > 400
    mols_s = [mols[i] for i in sel]
    off = np.zeros(len(sel) + 1, dtype=np.int32)
    off[1:] = np.cumsum([m[1].shape[0] for m in mols_s])
    q = eng.forward_xyz(off, np.concatenate([m[0] for m in mols_s]), np.concatenate([m[1] for m in mols_s]),
                        np.array([m[2] for m in mols_s], dtype=np.float32), N=41)
    worst = 0.0
    for k, i in enumerate(sel):
        n = mols[i][1].shape[0]
        d = np.abs(q[off[k]:off[k + 1]] - val_gold[i, :n]).max()
        worst = max(worst, d)
        # total charge conserved (reference's own drift is <= 1.7e-6 on these systems)
        assert abs(float(q[off[k]:off[k + 1]].sum(dtype=np.float64)) - float(mols[i][2])) < 5e-6
    assert worst <= TOL, worst


def _oracle_batch(mols, weights, N, dtype=np.float64):
    from oracle import epnn_oracle as orc
    return [orc.forward_xyz(xyz, x, Q, weights, N=N, dtype=dtype) for xyz, x, Q in mols]


@pytest.mark.parametrize("nx,T,N", [(9, 5, 41), (10, 3, 29), (9, 2, 33)])
def test_small_random_weights_vs_oracle(gpu_engine_factory, val_dir, val_names, nx, T, N):
    """Non-degenerate GNN (random weights, non-zero biases): fused kernel vs the float64 oracle, incl. the
    dependence on the padded size N (charge_gn.py:70 sums over padded partners)."""
    w = random_weights(nx, T, seed=nx + T, scale=0.35)
    eng = gpu_engine_factory(nx=nx, T=T)
    eng.set_weights(w)
    names = [nm for nm in val_names if nm.startswith("dsgdb9nsd")][:24] + val_names[:8]
    mols, offsets, xyz, x, Q = load_molecules(val_dir, names, nx)
    keep = [k for k, m in enumerate(mols) if m[1].shape[0] <= min(N, 32)]
    mols = [mols[k] for k in keep]
    off = np.zeros(len(mols) + 1, dtype=np.int32)
    off[1:] = np.cumsum([m[1].shape[0] for m in mols])
    q = eng.forward_xyz(off, np.concatenate([m[0] for m in mols]), np.concatenate([m[1] for m in mols]),
                        np.array([m[2] for m in mols], dtype=np.float32), N=N)
    ref = _oracle_batch(mols, w, N)
    ref32 = _oracle_batch(mols, w, N, np.float32)
    worst = max(np.abs(q[off[k]:off[k + 1]] - ref[k][:m[1].shape[0]]).max() for k, m in enumerate(mols))
    noise = max(np.abs(ref32[k] - ref[k]).max() for k in range(len(mols)))
    scale = max(np.abs(r).max() for r in ref)
    print(f"nx={nx} T={T} N={N}: worst |dq| {worst:.3e}; float32 oracle noise {noise:.3e}; |q| up to {scale:.3f}")
    # 1e-5 absolute, or the float32 noise of the reference algorithm itself where that is larger
    assert worst <= max(TOL, 3 * noise), (worst, noise)


def _batch(mols):
    off = np.zeros(len(mols) + 1, dtype=np.int32)
    off[1:] = np.cumsum([m[1].shape[0] for m in mols])
    return (off, np.concatenate([m[0] for m in mols]), np.concatenate([m[1] for m in mols]),
            np.array([m[2] for m in mols], dtype=np.float32))


def test_val_golden_all(gpu_engine_factory, weights_decay, val_dir, val_names, val_gold):
    """All 871 validation systems in ONE mixed batch vs the stored TensorFlow predictions: n <= 32 on the two-block fused
    kernel, the 22 systems of 33..38 atoms on three wavefronts of the block-per-wavefront kernel; and once more with those 22 on the tiled kernels
    ("wave3" = 0), which is where every system above 48 atoms goes."""
    mols, offsets, xyz, x, Q = load_molecules(val_dir, val_names)
    nmid = sum(1 for m in mols if m[1].shape[0] > 32)
    assert nmid == 22 and max(m[1].shape[0] for m in mols) == 38
    # (third pass, "wave2" = 28: molecules of 17..27 atoms on one wavefront each in a launch of their own, which the launch of the 22
    #  larger systems runs beside on the handle's side stream)
    for wave3, wave2 in ((1, -1), (0, -1), (1, 28)):
        eng = gpu_engine_factory(nx=9, T=5)
        eng.set_weights(weights_decay)
        eng.set_option("wave3", wave3)
        eng.set_option("wave2", wave2)
        q = eng.forward_xyz(offsets, xyz, x, Q, N=41)
        st = eng.last_stats()
        assert (st[1], st[2]) == ((871, 0) if wave3 else (871 - nmid, nmid)), st
        worst = 0.0
        for i, m in enumerate(mols):
            n = m[1].shape[0]
            qi = q[offsets[i]:offsets[i + 1]]
            worst = max(worst, np.abs(qi - val_gold[i, :n]).max())
            assert abs(float(qi.sum(dtype=np.float64)) - float(m[2])) < 5e-6
            assert np.all(val_gold[i, n:] == 0)      # the reference's padded atoms stay exactly 0
        print(f"871 systems (wave3 = {wave3}, wave2 = {wave2}): worst |dq| vs TF golden {worst:.3e}; fused / tiled = {st[1]} / {st[2]}")
        assert worst <= TOL, worst


def test_protein_golden(gpu_engine_factory, weights_decay, golden_dir):
    """2220-atom Galectin-3C, Q=+2 (BASELINE.json configs[3]) vs the stored TensorFlow prediction."""
    from oracle import epnn_oracle as orc
    eng = gpu_engine_factory(nx=9, T=5)
    eng.set_weights(weights_decay)
    xyz, x, Q = orc.parse_xyz(os.path.join(golden_dir, "protein", "6qlp_capped.xyz"), 9)
    gold = np.load(os.path.join(golden_dir, "protein", "preds.npy")).ravel()
    n = x.shape[0]
    assert n == 2220 and float(Q) == 2.0
    q = eng.forward_xyz(np.array([0, n], dtype=np.int32), xyz, x, np.array([Q], dtype=np.float32), N=n)
    err = np.abs(q - gold).max()
    drift = abs(float(q.sum(dtype=np.float64)) - 2.0)
    print(f"protein: max |dq| {err:.3e}; |sum q - Q| {drift:.3e} (reference's own drift 1.5e-5); pairs {eng.last_stats()[0]}")
    assert err <= TOL, err
    assert drift < 5e-5


@pytest.mark.parametrize("nx,T,N", [(9, 3, 41), (10, 2, 50)])
def test_tiled_random_weights_vs_oracle(gpu_engine_factory, val_dir, val_names, nx, T, N):
    """Tiled kernels in the non-degenerate regime, on molecules of every size (force_path=2), incl. N > n."""
    w = random_weights(nx, T, seed=7 * nx + T, scale=0.35)
    eng = gpu_engine_factory(nx=nx, T=T)
    eng.set_weights(w)
    eng.set_option("force_path", 2)
    names = [nm for nm in val_names if nm.startswith("SSI")][:10] + [nm for nm in val_names if nm.startswith("dsgdb9nsd")][:6]
    mols, offsets, xyz, x, Q = load_molecules(val_dir, names, nx)
    q = eng.forward_xyz(offsets, xyz, x, Q, N=N)
    assert eng.last_stats()[1] == 0
    ref = _oracle_batch(mols, w, N)
    ref32 = _oracle_batch(mols, w, N, np.float32)
    worst = max(np.abs(q[offsets[k]:offsets[k + 1]] - ref[k][:m[1].shape[0]]).max() for k, m in enumerate(mols))
    noise = max(np.abs(ref32[k] - ref[k]).max() for k in range(len(mols)))
    print(f"tiled nx={nx} T={T} N={N}: worst |dq| {worst:.3e}; float32 oracle noise {noise:.3e}")
    assert worst <= max(TOL, 3 * noise), (worst, noise)
    # fused and tiled paths agree on the molecules both can run
    eng2 = gpu_engine_factory(nx=nx, T=T)
    eng2.set_weights(w)
    small = [m for m in mols if m[1].shape[0] <= 32]
    off, xyz_s, x_s, Q_s = _batch(small)
    qa = eng2.forward_xyz(off, xyz_s, x_s, Q_s, N=N)
    eng2.set_option("force_path", 2)
    qb = eng2.forward_xyz(off, xyz_s, x_s, Q_s, N=N)
    assert np.abs(qa - qb).max() <= 2e-6


def test_tile_workgroup_sweep_sizes_vs_oracle(gpu_engine_factory):
    """The tile-workgroup sweep kernel (k_lg_sweep2, systems of up to 4096 atoms) around its boundaries: one tile with a single
    column block (n <= 16 on the tiled path), 32 / 33 atoms (a second tile of one atom), pieces of one partner, a partial last piece,
    several systems in one batch, a piece longer than one staging trip (large_chunks = 1: 321 partners per wavefront) -- each against
    the float64 oracle with non-degenerate weights, and the four-tile kernel (large_sweep_old) within float32 rounding of it."""
    from epnn_amd import synth
    from oracle import epnn_oracle as orc
    nx, T = 9, 2
    w = random_weights(nx, T, seed=41, scale=0.35)
    for t in range(T):                                       # (all-pairs sums over hundreds of partners: keep |h| of order one)
        w["msg"][t][2] = (w["msg"][t][2][0] / 8.0, w["msg"][t][2][1] / 8.0)
    sizes = [5, 16, 17, 32, 33, 64, 65, 97, 129, 161, 257, 321]
    mols = []
    for k, n in enumerate(sizes):
        _, xyz, x, Q, _ = synth.box_system(n_atoms=n, seed=100 + k)
        mols.append((xyz, x, np.float32(Q[0])))
    off, xyz, x, Q = _batch(mols)
    N = 330
    ref = _oracle_batch(mols, w, N)
    ref32 = _oracle_batch(mols, w, N, np.float32)
    noise = max(np.abs(ref32[k] - ref[k]).max() for k in range(len(mols)))
    got = {}
    for name, opts in (("tile workgroups", {}), ("one piece per tile", {"large_chunks": 1}), ("four-tile kernel", {"large_sweep_old": 1})):
        eng = gpu_engine_factory(nx=nx, T=T)
        eng.set_weights(w)
        eng.set_option("force_path", 2)
        for k_, v_ in opts.items():
            eng.set_option(k_, v_)
        q = eng.forward_xyz(off, xyz, x, Q, N=N)
        assert eng.last_stats()[2] == len(mols)
        worst = max(np.abs(q[off[k]:off[k + 1]] - ref[k][:len(m[0])]).max() for k, m in enumerate(mols))
        print(f"{name}: worst |dq| {worst:.3e} over sizes {sizes}; float32 oracle noise {noise:.3e}")
        assert worst <= max(TOL, 3 * noise), (name, worst, noise)
        got[name] = q
        # every system alone gives the bits it has in the batch (its plan depends on its own size only)
        k = sizes.index(97)
        alone = eng.forward_xyz(np.array([0, 97], np.int32), mols[k][0], mols[k][1], np.array([mols[k][2]], np.float32), N=N)
        assert np.array_equal(alone, q[off[k]:off[k + 1]]), name
    assert np.abs(got["tile workgroups"] - got["four-tile kernel"]).max() <= max(TOL, 3 * noise)


def test_sharded_equals_whole_bit_for_bit(gpu_engine_factory, weights_full, val_dir, val_names):
    """molecules are independent, so any partition of the batch (here: the 2-, 3- and
    8-way partitions bench.py / shard.py would use) gives bit-identical charges; also run-to-run determinism.
    Uses model_weights (nx=10, non-collapsed GNN, N-dependent)."""
    from epnn_amd import shard
    eng = gpu_engine_factory(nx=10, T=5)
    eng.set_weights(weights_full)
    names = val_names[:160]
    mols, offsets, xyz, x, Q = load_molecules(val_dir, names, nx=10)
    compute = lambda o, a, b, c, N: eng.forward_xyz(o, a, b, c, N)
    whole = compute(offsets, xyz, x, Q, 41)
    again = compute(offsets, xyz, x, Q, 41)
    assert np.array_equal(whole, again)
    for world in (2, 3, 8):
        out = np.zeros_like(whole)
        parts = shard.partition_molecules(np.diff(offsets), world)
        for idx in parts:
            off, xyz_s, x_s, Q_s, rows = shard.take_molecules(offsets, xyz, x, Q, idx)
            out[rows] = compute(off, xyz_s, x_s, Q_s, 41)
        assert np.array_equal(out, whole), world


def test_model_weights_vs_oracle_noise_scaled(gpu_engine_factory, weights_full, val_dir, val_names):
    """model_weights (nx=10): no stored reference output exists (parity unpinned); |h| reaches
    ~150 so float32 noise of the reference algorithm itself is ~1e-4.  Compare with the float64 oracle at a
    tolerance scaled to the float32 oracle's own noise."""
    eng = gpu_engine_factory(nx=10, T=5)
    eng.set_weights(weights_full)
    names = [nm for nm in val_names if nm.startswith("dsgdb9nsd")][:12]
    mols, offsets, xyz, x, Q = load_molecules(val_dir, names, nx=10)
    q = eng.forward_xyz(offsets, xyz, x, Q, N=41)
    ref = _oracle_batch(mols, weights_full, 41)
    ref32 = _oracle_batch(mols, weights_full, 41, np.float32)
    worst = max(np.abs(q[offsets[k]:offsets[k + 1]] - ref[k][:m[1].shape[0]]).max() for k, m in enumerate(mols))
    noise = max(np.abs(ref32[k] - ref[k]).max() for k in range(len(mols)))
    print(f"model_weights: worst |dq| {worst:.3e}; float32 oracle noise {noise:.3e}")
    assert worst <= max(TOL, 3 * noise)


def test_box_system_vs_oracle(gpu_engine_factory):
    """BASELINE.json configs[4] at a size the oracle finishes in seconds: a 1500-atom piece of the synthetic
    periodic-like box (density 0.1 / A^3, min separation 0.9 A) on the tiled kernels vs the float64 oracle, with
    non-degenerate weights; plus charge conservation of the full-size recipe's statistics."""
    from epnn_amd import synth
    from oracle import epnn_oracle as orc
    from golden import make_oracle_fixtures as fx
    nx, T = 9, 2
    xyz, x, Q, N, w = fx.box1500_case()
    offsets = np.array([0, 1500], np.int32)
    eng = gpu_engine_factory(nx=nx, T=T)
    eng.set_weights(w)
    q = eng.forward_xyz(offsets, xyz, x, Q, N=N)
    st = eng.last_stats()
    assert st[2] == 1 and 6.0 < 2.0 * st[0] / 1500 < 14.0          # ~11 partners within 3 A per atom
    # the oracle's output for exactly these inputs is cached (tests/golden/oracle_box1500.npz: OUR oracle's arrays, keyed by a hash
    # of the inputs; test_oracle_golden.py recomputes it on the CPU); recomputed here only if the inputs have changed
    z = fx.load("oracle_box1500.npz", xyz, x, Q, N, w)
    if z is not None:
        ref, ref32 = z["q_float64"], z["q_float32"]
    else:
        ref = orc.forward_xyz(xyz, x, Q[0], w, N=N, dtype=np.float64, row_block=128)
        ref32 = orc.forward_xyz(xyz, x, Q[0], w, N=N, dtype=np.float32, row_block=128)
    err, noise = np.abs(q - ref).max(), np.abs(ref32 - ref).max()
    print(f"box 1500 atoms: |dq| {err:.3e}; float32 oracle noise {noise:.3e}; sum q {q.sum(dtype=np.float64):.2e}")
    assert err <= max(TOL, 3 * noise)
    assert abs(float(q.sum(dtype=np.float64))) < 1e-4


def test_capacity_regrow_and_launch_variants_are_bit_identical(gpu_engine_factory, weights_full, val_dir, val_names):
    """Internal capacity / launch-shape choices must not change the bits: G rows spilled to HBM (small LDS budget per
    wavefront) with the in-kernel front-end; with the separate front-end kernels the pair-list regrow after an
    overflow and the LDS budget.  The two front-ends differ only in how the float64 edge features are evaluated
    (exp per channel vs. recurrence), the tiled kernels in the summation order: float32 rounding apart."""
    names = val_names[:96]
    mols, offsets, xyz, x, Q = load_molecules(val_dir, names, nx=10)

    def run(opts):
        eng = gpu_engine_factory(nx=10, T=5)
        eng.set_weights(weights_full)
        for k, v in opts.items():
            eng.set_option(k, v)
        q = eng.forward_xyz(offsets, xyz, x, Q, 41)
        st = eng.last_stats()
        q2 = eng.forward_xyz(offsets, xyz, x, Q, 41)      # and again with the grown capacities
        assert np.array_equal(q2, q), opts
        return q, st

    ref, st = run({})
    assert st[3] == 0 and st[0] > 0
    q, st = run({"wave_lds": 16384})
    assert np.array_equal(q, ref), np.abs(q - ref).max()
    ref_list, st_list = run({"wave_front": 0})
    assert st_list[0] == st[0]                            # same number of near pairs from both front-ends
    assert np.abs(ref_list - ref).max() <= 2e-4           # model_weights: |h| ~ 150, float32 noise ~1e-4
    q, st = run({"wave_front": 0, "pair_cap_per_atom": 1})
    assert st[3] >= 1, st                                 # the overflow path really ran
    assert np.array_equal(q, ref_list), np.abs(q - ref_list).max()
    q, st = run({"wave_front": 0, "wave_lds": 16384})
    assert np.array_equal(q, ref_list), np.abs(q - ref_list).max()
    q, st = run({"force_path": 2})
    assert np.abs(q - ref).max() <= 2e-4


def test_repeated_device_resident_forwards_run_one_ahead(gpu_engine_factory, weights_full, val_dir, val_names):
    """epnn_forward_xyz_dev on the same batch and device buffers again (a trajectory, a benchmark loop) enqueues the new
    forward before it looks at the previous one's status ("forward_ahead", default): two status slots, and a forward that
    overflowed a capacity is redone with its successor behind it.  Ten forwards in a row, with the separate front-end and
    a pair capacity of one per atom (the first forward overflows while the second is already behind it) and with the defaults;
    tiled path forced for a second batch: the charges are the bits of the one-at-a-time sequence every time."""
    names = val_names[:48]
    mols, offsets, xyz, x, Q = load_molecules(val_dir, names, nx=10)
    A = int(offsets[-1])
    for opts in ({}, {"wave_front": 0}, {"wave_front": 0, "pair_cap_per_atom": 1}, {"force_path": 2}, {"force_path": 2, "pair_cap_per_atom": 1}):
        outs = {}
        for ahead in (1, 0):
            eng = gpu_engine_factory(nx=10, T=5)
            eng.set_weights(weights_full)
            for k, v in opts.items():
                eng.set_option(k, v)
            eng.set_option("forward_ahead", ahead)
            d = [eng.to_device(a) for a in (xyz, x, Q)]
            dq = eng.alloc(A * 4)
            res = []
            for rep in range(10):
                eng.forward_xyz_dev(offsets, d[0], d[1], d[2], dq, 41)
                if rep in (0, 1, 4, 9):
                    eng.sync()
                    res.append(dq.download((A,)))
            eng.sync()
            outs[ahead] = (res, eng.last_stats())
            for b in d + [dq]:
                b.free()
        for a, b_ in zip(outs[1][0], outs[0][0]):
            assert np.array_equal(a, b_), opts
        assert np.array_equal(outs[1][0][0], outs[1][0][-1])
        if "pair_cap_per_atom" in opts:
            assert outs[1][1][3] >= 1 and outs[0][1][3] >= 1, (opts, outs[1][1], outs[0][1])


def test_fused_kernel_edge_shapes_vs_oracle(gpu_engine_factory):
    """Shapes at the limits of the one-wavefront-per-molecule kernel: single atom (no pairs), two atoms, 31 and 32 atoms
    (every lane owns an atom), and dense clusters in which EVERY pair is under the cutoff (496 near pairs for n = 32:
    the G rows do not fit the wave's LDS budget, both stacks read them back from HBM) -- random non-degenerate weights,
    float64 oracle, both front-ends."""
    from epnn_amd import synth
    nx, T, N = 9, 3, 35
    w = random_weights(nx, T, seed=7, scale=0.35)
    rng = np.random.default_rng(11)
    mols = []
    for n, span in [(1, 1.0), (2, 1.2), (31, 9.0), (32, 9.0), (32, 1.9), (24, 1.6), (17, 6.0)]:
        while True:                      # random points in a cube of edge `span`, minimum separation 0.35 A
            pts = rng.uniform(0, span, size=(n, 3))
            d = np.linalg.norm(pts[:, None] - pts[None], axis=-1) + np.eye(n) * 10
            if d.min() > (0.35 if span < 3 else 0.8):
                break
        sym = rng.choice(["H", "C", "N", "O", "F"], size=n)
        mols.append((pts.astype(np.float32), synth.features(sym), float(rng.integers(-1, 2))))
    # molecules split over two / three wavefronts at both extremes: no pair under the cutoff at all (atoms 3.5 A apart on a
    # line: every pair table is empty, the barriers still have to match), and a 35-atom cluster with most pairs under it
    for n in (20, 35):
        pts = np.stack([np.arange(n) * 3.5, np.zeros(n), np.zeros(n)], axis=1)
        mols.append((pts.astype(np.float32), synth.features(rng.choice(["H", "C", "N", "O"], size=n)), 0.0))
    while True:
        pts = rng.uniform(0, 2.6, size=(35, 3))
        d = np.linalg.norm(pts[:, None] - pts[None], axis=-1) + np.eye(35) * 10
        if d.min() > 0.35:
            break
    mols.append((pts.astype(np.float32), synth.features(rng.choice(["H", "C", "N", "O"], size=35)), 1.0))
    off = np.zeros(len(mols) + 1, dtype=np.int32)
    off[1:] = np.cumsum([m[1].shape[0] for m in mols])
    xyz, x = np.concatenate([m[0] for m in mols]), np.concatenate([m[1] for m in mols])
    Q = np.array([m[2] for m in mols], dtype=np.float32)
    ref = _oracle_batch(mols, w, N)
    ref32 = _oracle_batch(mols, w, N, np.float32)
    noise = max(np.abs(ref32[k] - ref[k]).max() for k in range(len(mols)))
    npairs = sum(int(((np.linalg.norm(m[0][:, None].astype(np.float64) - m[0][None].astype(np.float64), axis=-1) < 3.0).sum()
                      - m[0].shape[0]) // 2) for m in mols)
    for opts in ({}, {"wave_front": 0}, {"wave_lds": 16384}, {"wave2": 0}):
        eng = gpu_engine_factory(nx=nx, T=T)
        eng.set_weights(w)
        for k, v in opts.items():
            eng.set_option(k, v)
        q = eng.forward_xyz(off, xyz, x, Q, N=N)
        st = eng.last_stats()
        tiled = 2 if opts.get("wave_front", 1) == 0 else 0          # without the in-kernel front-end 33..48 atoms run on the tiled kernels
        assert st[0] == npairs and st[1] == len(mols) - tiled and st[2] == tiled, (opts, st, npairs)
        for k, m in enumerate(mols):
            n = m[1].shape[0]
            err = np.abs(q[off[k]:off[k + 1]] - ref[k][:n]).max()
            assert err <= max(TOL, 4 * noise), (opts, k, n, err, noise)
            assert abs(float(q[off[k]:off[k + 1]].sum(dtype=np.float64)) - m[2]) < 2e-5
    print(f"edge shapes: {npairs} near pairs, float32 oracle noise {noise:.2e}")


def test_edge_basis_residual_and_front_end_agreement(gpu_engine_factory, weights_decay, val_dir, val_names, val_gold):
    """The fused kernel's own front-end runs its G products in a 16-dimensional basis of the Gaussian edge features.
    The basis must reproduce the features to 1e-9 (relative to max e = 1), and charges must agree with the K = 48 path
    (separate front-end kernels, exp per channel) far inside the parity tolerance."""
    eng = gpu_engine_factory(nx=9, T=5)
    res = float(eng.lib.epnn_edge_basis_residual(eng.h))
    assert 0.0 < res < 1e-9, res
    eng.set_weights(weights_decay)
    mols, offsets, xyz, x, Q = load_molecules(val_dir, val_names[:200])
    sel = [i for i, m in enumerate(mols) if m[1].shape[0] <= 32]
    ms = [mols[i] for i in sel]
    off = np.zeros(len(ms) + 1, dtype=np.int32)
    off[1:] = np.cumsum([m[1].shape[0] for m in ms])
    args = (off, np.concatenate([m[0] for m in ms]), np.concatenate([m[1] for m in ms]), np.array([m[2] for m in ms], dtype=np.float32))
    q16 = eng.forward_xyz(*args, N=41)
    eng48 = gpu_engine_factory(nx=9, T=5)
    eng48.set_weights(weights_decay)
    eng48.set_option("wave_front", 0)
    q48 = eng48.forward_xyz(*args, N=41)
    d = float(np.abs(q16 - q48).max())
    worst = max(float(np.abs(q16[off[k]:off[k + 1]] - val_gold[i, :ms[k][1].shape[0]]).max()) for k, i in enumerate(sel))
    print(f"edge basis residual {res:.2e}; K=16 vs K=48 charges {d:.2e}; vs stored TensorFlow outputs {worst:.2e}")
    assert d < 3e-6 and worst <= TOL                      # float32 rounding of two different summations


def test_fused_kernel_every_size_vs_oracle(gpu_engine_factory):
    """Every molecule size 1..32 (the column-block / partner-copy layout of the fused kernel changes with n) at two
    densities, random non-degenerate weights, nx = 10 (four xq K steps), float64 oracle; both front-ends."""
    from epnn_amd import synth
    nx, T, N = 10, 2, 34
    w = random_weights(nx, T, seed=3, scale=0.35)
    rng = np.random.default_rng(5)
    names10 = ["H", "C", "N", "O", "F", "S", "Cl", "Br"]
    mols = []
    for n in range(1, 33):
        for span_per_atom in (0.9, 2.2):
            span = max(1.2, span_per_atom * n ** (1.0 / 3.0) * 1.6)
            while True:
                pts = rng.uniform(0, span, size=(n, 3))
                d = np.linalg.norm(pts[:, None] - pts[None], axis=-1) + np.eye(n) * 10
                if d.min() > 0.7:
                    break
            sym = rng.choice(names10[:5], size=n)
            x9 = synth.features(sym)
            x = np.concatenate([x9, rng.uniform(0, 1, size=(n, nx - 9)).astype(np.float32)], axis=1)
            mols.append((pts.astype(np.float32), x, float(rng.integers(-1, 2))))
    off = np.zeros(len(mols) + 1, dtype=np.int32)
    off[1:] = np.cumsum([m[1].shape[0] for m in mols])
    xyz, x = np.concatenate([m[0] for m in mols]), np.concatenate([m[1] for m in mols])
    Q = np.array([m[2] for m in mols], dtype=np.float32)
    ref = _oracle_batch(mols, w, N)
    ref32 = _oracle_batch(mols, w, N, np.float32)
    noise = max(np.abs(ref32[k] - ref[k]).max() for k in range(len(mols)))
    got = {}
    for opts in ({}, {"wave_front": 0}, {"wave2": 0}, {"wave2": 25}):
        eng = gpu_engine_factory(nx=nx, T=T)
        eng.set_weights(w)
        for k, v in opts.items():
            eng.set_option(k, v)
        q = eng.forward_xyz(off, xyz, x, Q, N=N)
        got[tuple(opts.items())] = q
        worst, at = 0.0, -1
        for k, m in enumerate(mols):
            n = m[1].shape[0]
            err = float(np.abs(q[off[k]:off[k + 1]] - ref[k][:n]).max())
            if err > worst:
                worst, at = err, n
        print(f"sizes 1..32 {opts}: worst |dq| {worst:.2e} (n = {at}); float32 oracle noise {noise:.2e}")
        assert worst <= max(TOL, 4 * noise), (opts, worst, at)
    # The block-per-wavefront kernel (default: molecules of 17+ atoms split over two wavefronts, smaller ones in pairs) against
    # the one-wavefront kernel ("wave2" = 0): an unsplit molecule runs the very same instruction sequence (bit-identical); a
    # split one runs the one-block code for the atoms of its second block too, where k_wave_forward has separately compiled
    # two-block code -- same operands, same order of every sum, results within float32 rounding of each other.
    base = got[(("wave2", 0),)]
    for key, thr in (((), 17), ((("wave2", 25),), 25)):
        for k, m in enumerate(mols):
            n = m[1].shape[0]
            a, b = got[key][off[k]:off[k + 1]], base[off[k]:off[k + 1]]
            if n < thr:
                assert np.array_equal(a, b), (key, n)
            else:
                assert np.abs(a - b).max() <= 2e-7, (key, n, np.abs(a - b).max())


def test_pipeline_map_equals_one_call_at_a_time(weights_decay):
    """Pipeline.map (epnn_forward_xyz_begin / _end on several handles, page-locked staging, plans uploaded without
    waiting) returns, in order, bit-for-bit what forward_xyz returns for each batch - also when a batch contains a
    system for the tiled path (its 698 pairs fit the list's first 1024: the regrow deferred into _end is reached in
    tests/test_gpu_pipeline_contract.py)."""
    from epnn_amd import synth
    from epnn_amd.engine import Engine, Pipeline
    batches = [synth.qm9_like_batch(B=40 + 7 * s, seed=s) for s in range(7)]
    N = max(b[4] for b in batches)
    big = synth.qm9_like_batch(B=3, seed=99)
    rng = np.random.default_rng(5)
    nbig = 70                                         # one 70-atom chain: tiled path
    xyz_big = np.cumsum(rng.normal(size=(nbig, 3)) * 0.8, axis=0).astype(np.float32)
    x_big = np.tile(big[2][:1], (nbig, 1))
    off = np.concatenate([big[0], [big[0][-1] + nbig]]).astype(np.int32)
    mixed = (off, np.concatenate([big[1], xyz_big]), np.concatenate([big[2], x_big]), np.concatenate([big[3], [0.0]]).astype(np.float32))
    stream = [b[:4] for b in batches[:3]] + [mixed] + [b[:4] for b in batches[3:]] + [batches[0][:4]]
    Nall = max(N, nbig)
    eng = Engine(nx=9, T=5)
    eng.set_weights(weights_decay)
    ref = [eng.forward_xyz(*b, Nall) for b in stream]
    eng.close()
    pipe = Pipeline(depth=3, nx=9, T=5)
    pipe.set_weights(weights_decay)
    got = list(pipe.map(stream, Nall))
    pipe.close()
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert a.shape == b.shape and np.array_equal(a, b)
    # a caller that stops iterating half way leaves no forward behind: the pipeline can be used again at once
    pipe = Pipeline(depth=3, nx=9, T=5)
    pipe.set_weights(weights_decay)
    it = pipe.map(stream, Nall)
    first = next(it)
    it.close()
    again = list(pipe.map(stream[:2], Nall))
    pipe.close()
    assert np.array_equal(first, ref[0]) and np.array_equal(again[0], ref[0]) and np.array_equal(again[1], ref[1])
    eng = Engine(nx=9, T=5)
    with pytest.raises(Exception):
        eng.forward_xyz_end()
    # One upload per forward: the host entry stages its inputs behind the plan's index arrays.  Every way the staging can
    # meet a plan: built by the device-resident entry (no room for inputs yet) and then reused by the host entry with the
    # same offsets; reused as it is (same batch again); rebuilt for a smaller and for a larger batch.
    eng.set_weights(weights_decay)
    b0, b1, b2 = batches[2], batches[0], batches[6]
    d = [eng.to_device(a) for a in b0[1:4]] + [eng.alloc(int(b0[0][-1]) * 4)]
    eng.forward_xyz_dev(b0[0], d[0], d[1], d[2], d[3], Nall)
    q_dev = d[3].download((int(b0[0][-1]),))
    for b, want in ((b0, ref[2]), (b0, ref[2]), (b1, ref[0]), (b2, ref[7]), (b0, ref[2])):
        assert np.array_equal(eng.forward_xyz(*b[:4], Nall), want)
    assert np.array_equal(q_dev, ref[2])
    eng.close()


@pytest.mark.parametrize("cutoff,eta", [(2.5, 4.0), (3.4, 1.2)])
def test_other_edge_constants_vs_oracle(gpu_engine_factory, val_dir, val_names, cutoff, eta):
    """The C ABI's config carries cutoff and eta (the reference hard-codes 3 and 2, charge_gn.py:148-161).  The fused
    kernel derives everything that depends on them at epnn_create -- edge basis, its interpolation table, the distance
    up to which every pair is a near pair -- so other values must work the same (or, when 16 basis vectors do not reach
    1e-8, fall back to the 48-channel front-end by themselves): both front-end settings vs the float64 oracle."""
    from oracle import epnn_oracle as orc
    nx, T, N = 9, 3, 33
    w = random_weights(nx, T, seed=17, scale=0.35)
    names = [nm for nm in val_names if nm.startswith("dsgdb9nsd")][:20]
    mols, offsets, xyz, x, Q = load_molecules(val_dir, names, nx)
    ref = [orc.forward_xyz(m[0], m[1], m[2], w, N=N, dtype=np.float64, cutoff=cutoff, eta=eta) for m in mols]
    for front in (1, 0):
        eng = gpu_engine_factory(nx=nx, T=T, cutoff=cutoff, eta=eta)
        res = float(eng.lib.epnn_edge_basis_residual(eng.h))   # >= 1e-8 (narrower Gaussians): the kernel's own front-end is not used
        eng.set_weights(w)
        eng.set_option("wave_front", front)
        q = eng.forward_xyz(offsets, xyz, x, Q, N=N)
        assert eng.last_stats()[1] == len(mols)
        worst = max(np.abs(q[offsets[k]:offsets[k + 1]] - ref[k][:m[1].shape[0]]).max() for k, m in enumerate(mols))
        print(f"cutoff {cutoff} eta {eta} front-end {front}: worst |dq| {worst:.2e}, edge basis residual {res:.1e}")
        assert worst <= TOL


@pytest.mark.parametrize("eta,near_tol", [(2.0, 1e-2), (2.0, 0.3), (1.2, 0.05)])
def test_near_flag_at_other_tolerances_fused_front_end_vs_pair_list(gpu_engine_factory, val_dir, val_names, eta, near_tol):
    """`near_tol` is a free constructor argument (the reference hard-codes 1e-5, charge_gn.py:89).  The fused kernel's own
    front-end does not evaluate max_k e_k per pair: epnn_create finds, with the reference's float64 expression, the distances at
    which the flag changes and the kernel counts how many lie below D.  With a large tolerance the change sits well inside the
    cutoff (1.9 .. 2.8 A), where QM9 molecules have many pairs: the charges must equal those of the 48-channel front-end,
    which forms the e rows and takes their maximum like the reference does; and both equal the float64 oracle run at that tolerance."""
    from oracle import epnn_oracle as orc
    nx, T, N = 9, 3, 33
    w = random_weights(nx, T, seed=23, scale=0.35)
    names = [nm for nm in val_names if nm.startswith("dsgdb9nsd")][:40]
    mols, offsets, xyz, x, Q = load_molecules(val_dir, names, nx)
    q = []
    for front in (1, 0):
        eng = gpu_engine_factory(nx=nx, T=T, eta=eta, near_tol=near_tol)
        assert float(eng.lib.epnn_edge_basis_residual(eng.h)) < 1e-8      # (otherwise the kernel's own front-end would not run)
        eng.set_weights(w)
        eng.set_option("wave_front", front)
        q.append(eng.forward_xyz(offsets, xyz, x, Q, N=N))
        assert eng.last_stats()[1] == len(mols)
    # the same run with the reference's tolerance differs by far more than rounding: the flag matters on this input
    eng = gpu_engine_factory(nx=nx, T=T, eta=eta)
    eng.set_weights(w)
    q_ref_tol = eng.forward_xyz(offsets, xyz, x, Q, N=N)
    print(f"eta {eta} near_tol {near_tol}: fused vs pair-list front-end {np.abs(q[0] - q[1]).max():.2e}; effect of the tolerance {np.abs(q[0] - q_ref_tol).max():.2e}")
    assert np.abs(q[0] - q_ref_tol).max() > 1e-3
    assert np.abs(q[0] - q[1]).max() <= 5e-6
    ref = np.concatenate([orc.forward_xyz(m[0], m[1], m[2], w, N=N, dtype=np.float64, eta=eta, near_tol=near_tol)[:m[1].shape[0]] for m in mols])
    print(f"    vs the float64 oracle at that tolerance: fused front-end {np.abs(q[0] - ref).max():.2e}, pair-list front-end {np.abs(q[1] - ref).max():.2e}")
    assert np.abs(q[0] - ref).max() <= TOL and np.abs(q[1] - ref).max() <= TOL


_PART_WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
import torch.distributed as dist
from epnn_amd import shard, synth, checkpoint, charge_gn
from epnn_amd.engine import Engine
from conftest import random_weights
rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
dist.init_process_group("gloo", rank=rank, world_size=world)
ROOT = sys.argv[1]
cases = []
# (a) the 2220-atom protein with the shipped checkpoint: stored TensorFlow output
xyz, x, Q, _ = charge_gn.read_xyz(os.path.join(ROOT, "tests/golden/protein/6qlp_capped.xyz"), 9)
gold = np.load(os.path.join(ROOT, "tests/golden/protein/preds.npy")).astype(np.float32).ravel()
cases.append((checkpoint.load_epnn_weights(os.path.join(ROOT, "models/decay_model_weights")), 5,
              np.array([0, len(x)], np.int32), xyz, x, np.array([Q], np.float32), len(x), gold))
# (b) random non-degenerate weights (the all-pairs sums matter): a 700-atom box, small molecules, a 300-atom box -- the
#     ranges of tile groups dealt out to the processes cross the boundaries between the tiled molecules
offs, bxyz, bx, bQ, bN = synth.box_system(n_atoms=700, seed=3)
_, cxyz, cx, cQ, _ = synth.box_system(n_atoms=300, seed=4)
so, sxyz, sx, sQ, sN = synth.qm9_like_batch(B=5, seed=1)
off = np.concatenate([[0, 700], 700 + so[1:], [700 + so[-1] + 300]]).astype(np.int32)
cases.append((random_weights(9, 3, seed=5, scale=0.35), 3, off, np.concatenate([bxyz, sxyz, cxyz]), np.concatenate([bx, sx, cx]),
              np.concatenate([bQ, sQ, cQ]).astype(np.float32), 700, None))
for w, T, off, xyz, x, Q, N, gold in cases:
    eng = Engine(nx=9, T=T)
    eng.set_weights(w)
    whole = eng.forward_xyz(off, xyz, x, Q, N)
    eng.set_partition(rank, world, shard.make_row_exchange(eng, dist, rank, world))
    part = eng.forward_xyz(off, xyz, x, Q, N)
    assert np.array_equal(part, whole), (rank, float(np.abs(part - whole).max()))
    if gold is not None:
        assert np.abs(part - gold).max() < 1e-5
    eng.set_partition(0, 1)
    assert np.array_equal(eng.forward_xyz(off, xyz, x, Q, N), whole)
    eng.close()
dist.barrier()
if rank == 0:
    print("PARTITION_OK")
'''


def test_row_block_partition_of_one_large_system(tmp_path):
    """SURVEY section 8e, single large system: three processes (sharing this GPU, gloo for the exchange) each compute the
    all-pairs sums of their own rows of atoms and all-gather them after every GNN step; every process ends with charges
    bit-identical to the unpartitioned run (and within 1e-5 of the stored TensorFlow output for the protein)."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = tmp_path / "worker.py"
    script.write_text(_PART_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", OMP_NUM_THREADS="2")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3",
                          "--master-addr", "127.0.0.1", "--master-port", "29533", str(script), root],
                         env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    assert "PARTITION_OK" in out.stdout


@pytest.mark.parametrize("which", ["decay_model_weights", "random"])
def test_bench_batch_vs_oracle(weights_decay, which):
    """The batch bench.py times -- synth.qm9_like_batch(B=1024, seed=0, N=29), BASELINE.json configs[1] -- through the
    entry bench.py uses (Pipeline lanes, forward_xyz_dev on resident inputs): 160 of its molecules, every size that
    occurs among them included, vs the float64 oracle at 1e-5 (charge_gn.py:56-119); total charge of ALL 1024 molecules
    conserved.  With the shipped checkpoint (the bench's weights) and with random non-degenerate weights (the shipped
    GNN is collapsed, so only those see the message sums)."""
    from epnn_amd import synth
    from epnn_amd.engine import Pipeline
    w = weights_decay if which == "decay_model_weights" else random_weights(9, 5, seed=12, scale=0.3)
    offsets, xyz, x, Q, N = synth.qm9_like_batch(B=1024, seed=0, N=29)
    A = int(offsets[-1])
    pipe = Pipeline(depth=3, nx=9, T=5)
    pipe.set_weights(w)
    outs = []
    for e in pipe.engines:                                   # every lane runs the batch, like the bench's round robin
        d = [e.to_device(a) for a in (xyz, x, Q)]
        dq = e.alloc(A * 4)
        e.forward_xyz_dev(offsets, d[0], d[1], d[2], dq, N)
        outs.append((e, d, dq))
    pipe.sync()
    qs = [dq.download((A,)) for _, _, dq in outs]
    for e, d, dq in outs:
        for a in d + [dq]:
            a.free()
    pipe.close()
    assert all(np.array_equal(qs[0], q) for q in qs[1:])
    q = qs[0]
    ns = np.diff(offsets)
    sums = np.add.reduceat(q.astype(np.float64), offsets[:-1])
    assert np.abs(sums - Q).max() < 5e-6
    # sample: the first molecule of every size + the first 140 others
    first = {}
    for b, n in enumerate(ns):
        first.setdefault(int(n), b)
    sample = sorted(set(first.values()) | set(range(1, 141)))
    assert len(sample) >= 128 and set(int(ns[b]) for b in sample) == set(int(n) for n in ns)
    mols = [(xyz[offsets[b]:offsets[b + 1]], x[offsets[b]:offsets[b + 1]], Q[b]) for b in sample]
    ref = _oracle_batch(mols, w, N)
    ref32 = _oracle_batch(mols, w, N, np.float32)
    worst = max(np.abs(q[offsets[b]:offsets[b + 1]] - ref[k][:ns[b]]).max() for k, b in enumerate(sample))
    noise = max(np.abs(ref32[k] - ref[k]).max() for k in range(len(sample)))
    print(f"bench batch ({which}): {len(sample)} molecules, sizes {sorted(first)}; worst |dq| {worst:.3e}; float32 oracle noise {noise:.3e}")
    assert worst <= (TOL if which == "decay_model_weights" else max(TOL, 3 * noise)), (worst, noise)


@pytest.fixture(scope="module")
def box100k():
    from epnn_amd import synth
    return synth.box_system(n_atoms=100_000, seed=0)


def test_box_100k_full_size_properties(gpu_engine_factory, weights_decay, box100k):
    """BASELINE.json configs[4] at FULL size (100 000 atoms, seed 0; 0.9 s on the tiled kernels) through properties that
    do not need an O(n^2) oracle: charges finite, total charge conserved (Q = 0), the pair list the device
    front-end built has exactly the pairs a host count finds under the cutoff (k-d tree candidates, then the reference's
    own float64 distance and compare, charge_gn.py:124,150; how many of them also pass `is_near`, :90-94, is printed --
    that test enters the kernels as the pairs' weights and is covered by the oracle / golden comparisons), and a second
    run gives the same bits."""
    from scipy.spatial import cKDTree
    offsets, xyz, x, Q, N = box100k
    eng = gpu_engine_factory(nx=9, T=5)
    eng.set_weights(weights_decay)
    q = eng.forward_xyz(offsets, xyz, x, Q, N=N)
    st = eng.last_stats()
    assert st[1] == 0 and st[2] == 1
    assert np.isfinite(q).all()
    assert abs(float(q.sum(dtype=np.float64))) < 1e-3
    x64 = xyz.astype(np.float64)
    pr = cKDTree(x64).query_pairs(3.0 + 1e-9, output_type="ndarray")
    d = x64[pr[:, 1]] - x64[pr[:, 0]]
    D = np.sqrt((d * d).sum(-1))                     # charge_gn.py:124 on float32 coordinates promoted to float64
    listed = int((D < 3.0).sum())                    # charge_gn.py:150: C = 0 from D >= cutoff on
    mu = np.linspace(0.1, 3.0, 48)
    C = (np.cos(np.pi * D / 3.0) + 1.0) / 2.0
    C[D >= 3.0] = 0.0
    emax = (C[:, None] * np.exp(-2.0 * (D[:, None] - mu[None]) ** 2)).astype(np.float32).max(axis=1)
    near = int((emax > np.float32(1e-5)).sum())      # charge_gn.py:90-94; the device carries it as the pairs' weights
    print(f"100k box: {listed} pairs under the cutoff on the host, {st[0]} listed on the device ({near} of them pass is_near); "
          f"sum q {q.sum(dtype=np.float64):.2e}; |q| up to {np.abs(q).max():.3f}")
    assert listed == st[0]
    # ... and the device's is_near decisions (the pairs' weights) are the host's, pair by pair
    pi, pj, w, npairs = eng.debug_pairs(listed + 16)
    assert npairs == listed and int((w != 0).sum()) == near
    host = {(int(a), int(b)): bool(f) for (a, b), f in zip(pr[D < 3.0], emax[D < 3.0] > np.float32(1e-5))}
    assert all(host[(int(a), int(b))] == (wt != 0) for a, b, wt in zip(pi, pj, w))
    assert np.array_equal(eng.forward_xyz(offsets, xyz, x, Q, N=N), q)


def test_box_subbox_4096_vs_oracle(gpu_engine_factory, box100k):
    """The oracle comparison SURVEY section 8d names for configs[4]: the 4096 atoms of the 100 000-atom box closest to its
    corner (a sub-box at the box's density, ~11 partners per atom), tiled kernels vs the literal float64 oracle with
    non-degenerate random weights (the all-pairs sums of charge_gn.py:70 matter: 16.8 M pair rows per sweep)."""
    from oracle import epnn_oracle as orc
    from golden import make_oracle_fixtures as fx
    # (weights: all-pairs sums over 4096 partners -- the message MLP's last layer is scaled so that |h| stays O(1) like in a trained model)
    xyz, x, Q1, n, w = fx.subbox4096_case(box100k)
    nx, T = 9, 2
    eng = gpu_engine_factory(nx=nx, T=T)
    eng.set_weights(w)
    off = np.array([0, n], np.int32)
    q = eng.forward_xyz(off, xyz, x, np.array([1.0], np.float32), N=n)
    st = eng.last_stats()
    assert st[2] == 1 and 8.0 < 2.0 * st[0] / n < 13.0
    # cached like the 1500-atom box's (tests/golden/oracle_subbox4096.npz, OUR oracle's output keyed by a hash of the inputs)
    z = fx.load("oracle_subbox4096.npz", xyz, x, Q1, n, w)
    ref = z["q_float64"] if z is not None else orc.forward_xyz_large(xyz, x, np.float32(1.0), w, dtype=np.float64, row_block=64)     # ~2.5 min of host time
    err = np.abs(q - ref).max()
    print(f"sub-box 4096 atoms: |dq| {err:.3e}; |q| up to {np.abs(ref).max():.3f}; sum q {q.sum(dtype=np.float64):.6f}")
    assert err <= TOL
    assert abs(float(q.sum(dtype=np.float64)) - 1.0) < 1e-4


def test_partition_rccl_exchange_in_stream_world1(gpu_engine_factory):
    """The row exchange of a partitioned system through the handle's RCCL communicator (epnn_set_partition with no
    callback): grouped in-place broadcasts on the handle's stream, no host synchronisation.  One GPU here, so a
    world-size-1 communicator with the developer switch that runs the collective anyway: charges bit-identical to the
    unpartitioned forward (separate launches and fused tail are the same arithmetic), also for a batch that mixes tiled
    systems with small molecules."""
    from epnn_amd import synth
    from epnn_amd.engine import Engine
    w = random_weights(9, 3, seed=5, scale=0.35)
    offs, bxyz, bx, bQ, bN = synth.box_system(n_atoms=700, seed=3)
    so, sxyz, sx, sQ, sN = synth.qm9_like_batch(B=5, seed=1)
    off = np.concatenate([[0, 700], 700 + so[1:]]).astype(np.int32)
    xyz, x, Q = np.concatenate([bxyz, sxyz]), np.concatenate([bx, sx]), np.concatenate([bQ, sQ]).astype(np.float32)
    eng = gpu_engine_factory(nx=9, T=3)
    eng.set_weights(w)
    whole = eng.forward_xyz(off, xyz, x, Q, 700)
    eng.comm_init(Engine.comm_unique_id(), 0, 1)
    eng.set_option("part_collective", 1)
    coll = eng.forward_xyz(off, xyz, x, Q, 700)
    assert np.array_equal(coll, whole)
    eng.set_option("part_collective", 0)
    eng.set_option("large_fused", 0)                      # one kernel per stage, no collective
    assert np.array_equal(eng.forward_xyz(off, xyz, x, Q, 700), whole)
    with pytest.raises(Exception, match="exchange function or a communicator"):
        eng.set_partition(0, 2)                           # world 2 with a world-1 communicator and no callback


_RCCL_PART_WORKER = r'''
import os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import numpy as np
from epnn_amd import synth
from epnn_amd.engine import Engine
from epnn_amd.rendezvous import Rendezvous
from conftest import random_weights
r = Rendezvous()
eng = Engine(nx=9, T=3, device=r.rank)
eng.set_weights(random_weights(9, 3, seed=5, scale=0.35))
off, xyz, x, Q, N = synth.box_system(n_atoms=3000, seed=3)
whole = eng.forward_xyz(off, xyz, x, Q, N)
eng.comm_init(r.broadcast(Engine.comm_unique_id() if r.rank == 0 else None, name="id"), r.rank, r.world)
eng.set_partition(r.rank, r.world)                        # no callback: RCCL on the engine's stream
part = eng.forward_xyz(off, xyz, x, Q, N)
assert np.array_equal(part, whole), float(np.abs(part - whole).max())
same = r.all_gather(part.tobytes(), name="q")
assert all(s == same[0] for s in same)
r.barrier(); r.close(); eng.close()
if r.rank == 0:
    print("RCCL_PARTITION_OK", r.world)
'''


def test_partition_rccl_two_gpus(tmp_path):
    """Two processes, one GPU each, the row exchange over RCCL (xGMI) inside the forward: bit-identical to the whole-system
    run on every rank.  Needs two devices (the driver's multi-GPU node); skipped on a one-GPU box, where RCCL cannot join
    two ranks of one device."""
    import subprocess, sys
    from conftest import ROOT
    from epnn_amd import _lib
    if _lib.load().epnn_device_count() < 2:
        pytest.skip("one GPU visible: a multi-rank RCCL communicator needs one device per rank")
    script = tmp_path / "w.py"
    script.write_text(_RCCL_PART_WORKER)
    drv = ("import sys; sys.path.insert(0, sys.argv[1]); from epnn_amd.rendezvous import launch_ranks; "
           "sys.exit(launch_ranks(sys.argv[2], sys.argv[1:2], 2))")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    out = subprocess.run([sys.executable, "-c", drv, ROOT, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "RCCL_PARTITION_OK 2" in out.stdout, (out.stdout[-1500:], out.stderr[-3000:])


def test_all_real_qm9_molecules_vs_oracle(gpu_engine_factory, weights_decay, val_dir, train_dir, val_names, train_names, val_gold):
    """BASELINE.json configs[1] on REAL data ("also run the 1338 real QM9 files if committed as fixtures"):
    every QM9 molecule of the reference's `mixed` set that carries labels (the dsgdb9nsd_* files of the recorded training
    and validation splits) in ONE batch padded to the QM9 directory maximum N = 29, shipped checkpoint, against the float64
    oracle at 1e-5 per atom; the 281 of them that are validation systems also against the stored TensorFlow predictions."""
    where = [(val_dir, nm) for nm in val_names if nm.startswith("dsgdb9nsd")] + [(train_dir, nm) for nm in train_names if nm.startswith("dsgdb9nsd")]
    assert len(where) > 1300
    from oracle import epnn_oracle as orc
    mols = [orc.parse_xyz(os.path.join(d, nm + ".xyz"), 9) for d, nm in where]
    sizes = np.array([m[1].shape[0] for m in mols])
    assert sizes.max() == 29 and sizes.min() >= 3
    off, xyz, x, Q = _batch(mols)
    eng = gpu_engine_factory(nx=9, T=5)
    eng.set_weights(weights_decay)
    q = eng.forward_xyz(off, xyz, x, Q, N=29)
    assert eng.last_stats()[1] == len(mols)
    ref = _oracle_batch(mols, weights_decay, 29)
    worst = max(np.abs(q[off[k]:off[k + 1]] - ref[k][:sizes[k]]).max() for k in range(len(mols)))
    drift = max(abs(float(q[off[k]:off[k + 1]].sum(dtype=np.float64)) - float(mols[k][2])) for k in range(len(mols)))
    nval = sum(1 for d, _ in where if d == val_dir)
    gold_worst = max(np.abs(q[off[k]:off[k + 1]] - val_gold[val_names.index(where[k][1]), :sizes[k]]).max() for k in range(nval))
    print(f"{len(mols)} real QM9 molecules ({int(sizes.sum())} atoms, n = {sizes.min()}..{sizes.max()}): worst |dq| vs float64 oracle {worst:.2e}, "
          f"vs the stored TensorFlow output ({nval} systems) {gold_worst:.2e}; worst |sum q - Q| {drift:.1e}")
    assert worst <= TOL and gold_worst <= TOL and drift < 5e-6


def test_limits_of_the_configuration_vs_oracle(gpu_engine_factory):
    """The largest configuration the C ABI accepts: T = 8 steps (EPNN_MAXT) and nx = 10 atom-feature columns (the reference's
    larger element table; the feature row of the kernels has 59 slots + the constant), random non-degenerate weights with
    arbitrary (not one-hot) values in the feature columns, molecules on all three kernels (1..32 atoms, 40 atoms, 70 atoms tiled),
    N beyond the largest; float64 oracle.  One more column or step is refused at epnn_create."""
    from epnn_amd import synth
    from epnn_amd._lib import EpnnError
    from epnn_amd.engine import Engine
    nx, T, N = 10, 8, 75
    w = random_weights(nx, T, seed=31, scale=0.3)
    rng = np.random.default_rng(8)
    mols = []
    for n in (1, 5, 16, 17, 29, 32, 40, 70):
        span = max(1.5, 1.8 * n ** (1.0 / 3.0))
        while True:
            pts = rng.uniform(0, span, size=(n, 3))
            d = np.linalg.norm(pts[:, None] - pts[None], axis=-1) + np.eye(n) * 10
            if d.min() > 0.75:
                break
        x = np.concatenate([synth.features(rng.choice(["H", "C", "N", "O"], size=n)), rng.uniform(0, 1, size=(n, nx - 9)).astype(np.float32)], axis=1)
        x[:, 1:5] += rng.uniform(0, 0.3, size=(n, 4)).astype(np.float32)
        mols.append((pts.astype(np.float32), x, float(rng.integers(-1, 2))))
    off, xyz, x, Q = _batch(mols)
    eng = gpu_engine_factory(nx=nx, T=T)
    eng.set_weights(w)
    q = eng.forward_xyz(off, xyz, x, Q, N=N)
    st = eng.last_stats()
    assert st[1] == 7 and st[2] == 1                     # 1..32 and 40 on the fused kernels (40: three wavefronts), 70 on the tiled kernels
    ref = _oracle_batch(mols, w, N)
    ref32 = _oracle_batch(mols, w, N, np.float32)
    noise = max(np.abs(ref32[k] - ref[k]).max() for k in range(len(mols)))
    worst = max(np.abs(q[off[k]:off[k + 1]] - ref[k][:m[1].shape[0]]).max() for k, m in enumerate(mols))
    print(f"nx = 10, T = 8: worst |dq| {worst:.2e}; float32 oracle noise {noise:.2e}")
    assert worst <= max(TOL, 4 * noise)
    with pytest.raises(EpnnError, match="nx must be"):
        Engine(nx=11, T=8)
    with pytest.raises(EpnnError, match="T must be"):
        Engine(nx=9, T=9)


def test_three_block_kernel_every_size_vs_oracle(gpu_engine_factory):
    """Molecules of 33..48 atoms through the compact entry run on three wavefronts of the block-per-wavefront kernel
    (epnn_wave2.hip.h, k_wave_forward2<3>; the reference's `mixed` set goes up to 41 atoms).  Every size at two densities (the sparse ones keep
    their G rows in LDS, the dense ones spill them to HBM), random non-degenerate weights, nx = 10, N beyond the largest,
    non-zero total charges; float64 oracle.  The same molecules on the tiled kernels ("wave3" = 0) agree to float32
    rounding, and a batch that mixes all three kernels gives every molecule the bits it gets alone."""
    from epnn_amd import synth
    nx, T, N = 10, 3, 50
    w = random_weights(nx, T, seed=13, scale=0.35)
    rng = np.random.default_rng(17)
    mols = []
    for n in range(33, 49):
        for span_per_atom in (1.0, 2.2):
            span = max(1.2, span_per_atom * n ** (1.0 / 3.0) * 1.6)
            while True:
                pts = rng.uniform(0, span, size=(n, 3))
                d = np.linalg.norm(pts[:, None] - pts[None], axis=-1) + np.eye(n) * 10
                if d.min() > 0.7:
                    break
            x = np.concatenate([synth.features(rng.choice(["H", "C", "N", "O", "F"], size=n)), rng.uniform(0, 1, size=(n, 1)).astype(np.float32)], axis=1)
            mols.append((pts.astype(np.float32), x, float(rng.integers(-1, 2))))
    off, xyz, x, Q = _batch(mols)
    ref = _oracle_batch(mols, w, N)
    ref32 = _oracle_batch(mols, w, N, np.float32)
    noise = max(np.abs(ref32[k] - ref[k]).max() for k in range(len(mols)))
    eng = gpu_engine_factory(nx=nx, T=T)
    eng.set_weights(w)
    q = eng.forward_xyz(off, xyz, x, Q, N=N)
    st = eng.last_stats()
    assert st[1] == len(mols) and st[2] == 0, st                       # all on the fused kernels
    worst, at = 0.0, -1
    for k, m in enumerate(mols):
        n = m[1].shape[0]
        err = float(np.abs(q[off[k]:off[k + 1]] - ref[k][:n]).max())
        assert abs(float(q[off[k]:off[k + 1]].sum(dtype=np.float64)) - m[2]) < 2e-5
        if err > worst:
            worst, at = err, n
    npairs = sum(int(((np.linalg.norm(m[0][:, None].astype(np.float64) - m[0][None].astype(np.float64), axis=-1) < 3.0).sum() - m[0].shape[0]) // 2) for m in mols)
    assert st[0] == npairs
    print(f"sizes 33..48: worst |dq| {worst:.2e} (n = {at}); float32 oracle noise {noise:.2e}; {npairs} pairs")
    assert worst <= max(TOL, 4 * noise), (worst, at)
    # ("wave2" = 0, what a pipeline lane sets: the same kernel for these molecules, on the handle's one stream)
    one = gpu_engine_factory(nx=nx, T=T)
    one.set_weights(w)
    one.set_option("wave2", 0)
    q1 = one.forward_xyz(off, xyz, x, Q, N=N)
    assert one.last_stats()[1] == len(mols)
    worst1 = max(float(np.abs(q1[off[k]:off[k + 1]] - ref[k][:m[1].shape[0]]).max()) for k, m in enumerate(mols))
    print(f"sizes 33..48, one wavefront per molecule: worst |dq| {worst1:.2e}; |split - one wavefront| {np.abs(q1 - q).max():.2e}")
    assert worst1 <= max(TOL, 4 * noise) and np.abs(q1 - q).max() <= max(1e-6, 4 * noise)
    tiled = gpu_engine_factory(nx=nx, T=T)
    tiled.set_weights(w)
    tiled.set_option("wave3", 0)
    qt = tiled.forward_xyz(off, xyz, x, Q, N=N)
    assert tiled.last_stats()[2] == len(mols)
    assert np.abs(qt - q).max() <= max(3e-6, 4 * noise)
    # mixed batch: small, mid (three wavefronts), large (tiled): each molecule's charges do not depend on the others
    so, sxyz, sx9, sQ, _ = synth.qm9_like_batch(B=6, seed=2)
    sx = np.concatenate([sx9, np.zeros((sx9.shape[0], 1), np.float32)], axis=1)
    _, bxyz, bx9, bQ, bn = synth.box_system(n_atoms=90, seed=4)
    bx = np.concatenate([bx9, np.zeros((90, 1), np.float32)], axis=1)
    pick = [0, 7, 31]
    parts = [(sxyz[so[b]:so[b + 1]], sx[so[b]:so[b + 1]], float(sQ[b])) for b in range(6)] + [mols[k] for k in pick] + [(bxyz, bx, 0.0)]
    moff, mxyz, mx, mQ = _batch(parts)
    qm = eng.forward_xyz(moff, mxyz, mx, mQ, N=90)
    st = eng.last_stats()
    assert st[1] == 9 and st[2] == 1, st
    alone = eng.forward_xyz(*_batch([mols[k] for k in pick]), N=90)
    got = np.concatenate([qm[moff[6 + j]:moff[7 + j]] for j in range(3)])
    assert np.array_equal(got, alone)


@pytest.mark.gpu
def test_block_per_wave_kernel_batch_shapes(gpu_engine_factory):
    """The block-per-wavefront kernel (epnn_wave2.hip.h; the default of a lone handle for batches of at most 1024 molecules)
    on every shape of batch its workgroup table can take: only molecules that are split over two wavefronts, only ones that
    share a workgroup in pairs, an odd number of those (one idle wavefront), a single molecule of either kind, a mix with
    three-block and tiled molecules - against the float64 oracle; and where the automatic choice stops."""
    from epnn_amd import synth
    nx, T, N = 9, 2, 70
    w = random_weights(nx, T, seed=21, scale=0.35)
    off, xyz, x, Q, _ = synth.qm9_like_batch(B=48, seed=11, N=29)
    mols = [(xyz[off[k]:off[k + 1]], x[off[k]:off[k + 1]], float(Q[k])) for k in range(48)]
    rng = np.random.default_rng(4)
    for n in (36, 45, 60, 70):                               # three wavefronts (2), four (1) and the tiled path (1)
        pts = np.cumsum(rng.normal(size=(n, 3)) * 0.75, axis=0).astype(np.float32)
        mols.append((pts, synth.features(rng.choice(["H", "C", "N", "O"], size=n)), 0.0))
    ref = _oracle_batch(mols, w, N)
    ref32 = _oracle_batch(mols, w, N, np.float32)
    tol = max(TOL, 4 * max(np.abs(a - b).max() for a, b in zip(ref, ref32)))
    ns = [m[1].shape[0] for m in mols]
    singles = [k for k in range(48) if ns[k] <= 16]
    splits = [k for k in range(48) if ns[k] >= 17]
    assert len(singles) >= 5 and len(splits) >= 5
    eng = gpu_engine_factory(nx=nx, T=T)
    eng.set_weights(w)

    def run(sel):
        o = np.zeros(len(sel) + 1, np.int32)
        o[1:] = np.cumsum([ns[k] for k in sel])
        q = eng.forward_xyz(o, np.concatenate([mols[k][0] for k in sel]), np.concatenate([mols[k][1] for k in sel]),
                            np.array([mols[k][2] for k in sel], np.float32), N)
        return [q[o[i]:o[i + 1]] for i in range(len(sel))]

    cases = {"splits only": splits, "pairs only": singles[:4], "odd number of singles": singles[:5], "one single": singles[:1],
             "one split": splits[:1], "everything": list(range(len(mols))), "reversed": list(range(len(mols)))[::-1]}
    for name, sel in cases.items():
        got = run(sel)
        worst = max(np.abs(g - ref[k][:ns[k]]).max() for g, k in zip(got, sel))
        assert worst <= tol, (name, worst)
        assert int(eng.last_stats()[1]) == sum(1 for k in sel if ns[k] <= 64), name      # fused-path molecules
    # a molecule's charges do not depend on what else is in the batch (same kernel, same wavefront roles)
    whole = run(list(range(len(mols))))
    alone = run(splits[:1]) + run(singles[:1])
    assert np.array_equal(alone[0], whole[splits[0]]) and np.array_equal(alone[1], whole[singles[0]])
    # automatic choice: 1024 molecules still take the kernel, 1025 run one wavefront per molecule ("wave2" = 0)
    sel = [k % 48 for k in range(1025)]
    auto_1025 = np.concatenate(run(sel))
    auto_1024 = np.concatenate(run(sel[:1024]))
    eng.set_option("wave2", 0)
    off_1025 = np.concatenate(run(sel))
    eng.set_option("wave2", 17)
    on_1024 = np.concatenate(run(sel[:1024]))
    assert np.array_equal(auto_1025, off_1025) and np.array_equal(auto_1024, on_1024)
    assert np.abs(auto_1025[:auto_1024.size] - auto_1024).max() <= 2e-7


@pytest.mark.gpu
def test_four_wavefront_sizes_vs_oracle(gpu_engine_factory):
    """Molecules of 49..64 atoms through the compact entry run on FOUR wavefronts of the block-per-wavefront kernel
    (k_wave_forward2<4>; 64 is where its one-lane-per-partner front-end ends, 65 atoms take the tiled kernels).  Sizes at
    both ends and in between, sparse and dense, random non-degenerate weights, float64 oracle; the same molecules on the tiled
    kernels ("wave3" = 0) agree to float32 rounding."""
    from epnn_amd import synth
    nx, T, N = 9, 2, 66
    w = random_weights(nx, T, seed=23, scale=0.35)
    rng = np.random.default_rng(29)
    mols = []
    for n in (49, 50, 53, 56, 60, 63, 64, 65):
        for span_per_atom in (1.0, 2.2):
            span = max(1.2, span_per_atom * n ** (1.0 / 3.0) * 1.6)
            while True:
                pts = rng.uniform(0, span, size=(n, 3))
                d = np.linalg.norm(pts[:, None] - pts[None], axis=-1) + np.eye(n) * 10
                if d.min() > 0.7:
                    break
            mols.append((pts.astype(np.float32), synth.features(rng.choice(["H", "C", "N", "O", "F"], size=n)), float(rng.integers(-1, 2))))
    off, xyz, x, Q = _batch(mols)
    ref = _oracle_batch(mols, w, N)
    ref32 = _oracle_batch(mols, w, N, np.float32)
    noise = max(np.abs(ref32[k] - ref[k]).max() for k in range(len(mols)))
    eng = gpu_engine_factory(nx=nx, T=T)
    eng.set_weights(w)
    q = eng.forward_xyz(off, xyz, x, Q, N=N)
    st = eng.last_stats()
    assert st[1] == len(mols) - 2 and st[2] == 2, st                # the two 65-atom systems on the tiled kernels
    worst = max(float(np.abs(q[off[k]:off[k + 1]] - ref[k][:m[1].shape[0]]).max()) for k, m in enumerate(mols))
    for k, m in enumerate(mols):
        assert abs(float(q[off[k]:off[k + 1]].sum(dtype=np.float64)) - m[2]) < 2e-5
    tiled = gpu_engine_factory(nx=nx, T=T)
    tiled.set_weights(w)
    tiled.set_option("wave3", 0)
    qt = tiled.forward_xyz(off, xyz, x, Q, N=N)
    assert tiled.last_stats()[2] == len(mols)
    print(f"sizes 49..64: worst |dq| {worst:.2e}; float32 oracle noise {noise:.2e}; |four wavefronts - tiled| {np.abs(qt - q).max():.2e}")
    assert worst <= max(TOL, 4 * noise) and np.abs(qt - q).max() <= max(3e-6, 4 * noise)
    # on pipeline lanes ("wave2" = 0) the same kernel, on the lane's one stream
    lane = gpu_engine_factory(nx=nx, T=T)
    lane.set_weights(w)
    lane.set_option("wave2", 0)
    assert np.array_equal(lane.forward_xyz(off, xyz, x, Q, N=N), q)



def test_cutoff_and_is_near_edges_on_every_path(gpu_engine_factory):
    """charge_gn.py:150 (C = 0 from D >= 3.0 on: the pair has e = 0) and :90-94 (is_near from max_k e_k > 1e-5 in float32:
    flips at D = 2.99396) are two different cuts.  Constructed 2- and 3-atom molecules whose far pair sits at distances on
    both sides of both -- 2.9899 / 2.9900 (where the fused kernel's front-end stops assuming is_near), 2.9939 / 2.9940 (the
    flip), 2.99999, the float32 neighbours of 3.0 and 3.0 itself -- through every path: the in-kernel front-end on one
    wavefront per molecule and on the block-per-wavefront kernel, the separate front-end with the fused and with the tiled
    kernels; against the float64 oracle with non-degenerate weights (the transfer over a pair in the gap is excluded, its
    message term is not), and with the number of pairs each path lists."""
    from oracle import epnn_oracle as orc
    nx, T, N = 9, 3, 5
    w = random_weights(nx, T, seed=77, scale=0.5)
    three = np.float32(3.0)
    dists = [2.9899, 2.9900, 2.9939, 2.99395, 2.99397, 2.9940, 2.99999, float(np.nextafter(three, np.float32(0))), 3.0,
             float(np.nextafter(three, np.float32(4)))]
    mols = []
    for k, D in enumerate(dists):
        d32 = np.float32(D)
        for third in (False, True):
            xyz = [[0.0, 0.0, 0.0], [float(d32), 0.0, 0.0]] + ([[0.3, 1.1, 0.2]] if third else [])
            xyz = np.array(xyz, np.float32)
            n = len(xyz)
            x = np.zeros((n, nx), np.float32)
            x[:, 0] = [6, 8, 1][:n]
            x[np.arange(n), [2, 4, 1][:n]] = 1
            mols.append((xyz, x, np.float32(k % 3 - 1)))
    off, xyz, x, Q = _batch(mols)
    ref = _oracle_batch(mols, w, N)
    # the oracle's own count of listed pairs (D < 3.0) and near pairs
    mu = np.linspace(0.1, 3.0, 48)
    listed = near = 0
    for m in mols:
        c = m[0].astype(np.float64)
        for i in range(len(c)):
            for j in range(i + 1, len(c)):
                D = float(np.sqrt(((c[j] - c[i]) ** 2).sum()))
                if D < 3.0:
                    listed += 1
                    e = ((np.cos(np.pi * D / 3.0) + 1.0) / 2.0 * np.exp(-2.0 * (D - mu) ** 2)).astype(np.float32)
                    near += int(e.max() > np.float32(1e-5))
    assert listed > near                                      # some pairs do sit in the gap
    results = {}
    for name, opts in (("one wavefront per molecule", {"wave2": 0}), ("block per wavefront", {"wave2": 17}),
                       ("separate front-end, fused kernel", {"wave_front": 0, "wave2": 0}), ("tiled kernels", {"force_path": 2}),
                       ("tiled kernels, sweep in the first step", {"force_path": 2, "large_dedupe": 0})):
        eng = gpu_engine_factory(nx=nx, T=T)
        eng.set_weights(w)
        for k, v in opts.items():
            eng.set_option(k, v)
        q = eng.forward_xyz(off, xyz, x, Q, N=N)
        err = max(np.abs(q[off[k]:off[k + 1]] - ref[k][:len(m[0])]).max() for k, m in enumerate(mols))
        assert eng.last_stats()[0] == listed, (name, eng.last_stats()[0], listed)
        if "wave_front" in opts or "force_path" in opts:
            pi, pj, wt, npairs = eng.debug_pairs(listed + 8)
            assert npairs == listed and int((wt != 0).sum()) == near, (name, npairs, int((wt != 0).sum()), near)
        results[name] = err
        assert err <= TOL, (name, err)
    print("cutoff / is_near edges, worst |dq| per path:", {k: f"{v:.1e}" for k, v in results.items()})


@pytest.mark.parametrize("script,seed", [("fuzz_forward.py", 301), ("fuzz_dense.py", 302), ("fuzz_model.py", 303), ("fuzz_train.py", 304), ("fuzz_tiled.py", 305)])
def test_randomised_sweeps_with_a_fixed_seed(script, seed):
    """The four randomised sweeps against the float64 oracle (tests/fuzz_*.py; they found round 1's only real defect) with a
    fixed seed and a 12 s budget each, as part of the suite instead of by hand."""
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, script), str(seed), "12"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    assert "fuzz ok" in out.stdout or "0 not explained by a ReLU kink" in out.stdout, out.stdout[-500:]


def test_tiled_path_variants_agree(gpu_engine_factory, weights_full, golden_dir):
    """The tiled path's launch variants on the 2220-atom protein with model_weights (nx = 10, non-collapsed GNN): the merged
    launches of the compact entry (`large_merge`) and the one-kernel-per-stage form (`large_fused` = 0, what a partition runs)
    are the SAME arithmetic as the default -- bit-identical --; the first GNN step by atom types (`large_dedupe`) is an exact
    re-association of the all-pairs sum (count x value instead of repeated adds): float32 rounding apart."""
    from oracle import epnn_oracle as orc
    xyz, x, Q = orc.parse_xyz(os.path.join(golden_dir, "protein", "6qlp_capped.xyz"), 10)
    n = x.shape[0]
    off, Qa = np.array([0, n], np.int32), np.array([Q], np.float32)

    def run(**opts):
        eng = gpu_engine_factory(nx=10, T=5)
        eng.set_weights(weights_full)
        for k, v in opts.items():
            eng.set_option(k, v)
        q = eng.forward_xyz(off, xyz, x, Qa, N=n)
        assert eng.last_stats()[2] == 1 and eng.last_stats()[3] == 0
        return q

    ref = run()
    assert np.isfinite(ref).all()
    assert np.array_equal(run(large_merge=0), ref)
    assert np.array_equal(run(large_fused=0), ref)
    assert np.array_equal(run(large_chunks=14), run(large_chunks=14, large_fused=0))
    sweep = run(large_dedupe=0)
    scale = max(1.0, float(np.abs(ref).max()))
    print(f"protein, model_weights: first step by types vs by sweep: max |dq| {np.abs(sweep - ref).max():.2e} (|q| up to {scale:.2f})")
    assert np.abs(sweep - ref).max() <= 2e-4 * scale          # model_weights: |h| ~ 150, float32 noise of the algorithm itself ~1e-4
    assert np.array_equal(run(large_dedupe=0, large_merge=0), sweep)
    # round 5's front-end forms are the same arithmetic: the fill pass walking the count pass's bits or measuring every distance
    # again, the prefix sums worked out by the fill workgroups or by a launch of their own -- bit-identical
    assert np.array_equal(run(front_bits=0), ref)
    assert np.array_equal(run(front_inline=0), ref)
    assert np.array_equal(run(front_inline=0, front_bits=0, large_merge=0), ref)
    # the four-tile sweep kernel (what systems above 4096 atoms run) sums the partners in other pieces: float32 rounding apart
    old = run(large_sweep_old=1)
    print(f"protein, model_weights: tile-workgroup vs four-tile sweep kernel: max |dq| {np.abs(old - ref).max():.2e}")
    # (model_weights on the protein is the numerically wild case -- |q| ~ 2e4, |h| ~ 150 --: another order of a 2220-term float32 sum
    #  moves the charges by 2e-3 of their size; test_tile_workgroup_sweep_sizes_vs_oracle compares the two kernels where |q| ~ 1)
    assert np.abs(old - ref).max() <= 5e-3 * scale
    assert np.array_equal(run(large_sweep_old=1, large_fused=0), old)


def test_more_atom_types_than_the_table_holds_falls_back_to_the_sweep(gpu_engine_factory):
    """The first GNN step groups the atoms of a tiled molecule by feature row (at most 64 distinct rows).  A molecule whose
    rows are ALL different overflows the table: the device raises the flag, the host repeats the forward with the all-pairs
    sweep and the handle stays on the sweep; a molecule with few types next to it does not change that.  Against the float64
    oracle, and the repeat is counted in the stats."""
    from oracle import epnn_oracle as orc
    nx, T = 9, 2
    w = random_weights(nx, T, seed=5, scale=0.3)
    rng = np.random.default_rng(3)
    mols = []
    for n, distinct in ((90, True), (70, False)):
        pts = rng.uniform(0, 9.0, size=(n, 3)).astype(np.float32)
        x = np.zeros((n, nx), np.float32)
        x[np.arange(n), 1 + rng.integers(0, 4, size=n)] = 1
        x[:, 0] = np.arange(n) * 0.01 + 1.0 if distinct else rng.choice([1.0, 6.0, 8.0], size=n)
        mols.append((pts, x, np.float32(0)))
    off, xyz, x, Q = _batch(mols)
    eng = gpu_engine_factory(nx=nx, T=T)
    eng.set_weights(w)
    q = eng.forward_xyz(off, xyz, x, Q, N=96)
    st = eng.last_stats()
    assert st[2] == 2 and st[3] >= 1, st                       # two tiled molecules, at least one repeat of the forward
    ref = _oracle_batch(mols, w, 96)
    ref32 = _oracle_batch(mols, w, 96, np.float32)
    err = max(np.abs(q[off[k]:off[k + 1]] - ref[k][:len(m[0])]).max() for k, m in enumerate(mols))
    noise = max(np.abs(ref32[k] - ref[k]).max() for k in range(len(mols)))
    assert err <= max(TOL, 3 * noise), (err, noise)
    q2 = eng.forward_xyz(off, xyz, x, Q, N=96)                 # the handle now sweeps: no repeat, same bits
    assert eng.last_stats()[3] == st[3] and np.array_equal(q2, q)
    # few types only: the table serves, and the result agrees with the sweep's to rounding
    eng2 = gpu_engine_factory(nx=nx, T=T)
    eng2.set_weights(w)
    o2 = np.array([0, 70], np.int32)
    qa = eng2.forward_xyz(o2, mols[1][0], mols[1][1], Q[1:], N=96)
    assert eng2.last_stats()[3] == 0
    assert np.abs(qa - q[off[1]:off[2]]).max() <= max(TOL, 3 * noise)


def test_bf16_split_forms_on_the_device():
    """The arithmetic the Dense layers rest on, checked on the device itself (tools/micro/bf16x6, built by __graft_entry__.build
    from the w16_* primitives of epnn_common.h under the library's flags): the three-piece bf16 split with its remainders taken on the matrix pipe (x - piece as D = C - I B, both the K = 32 and the
    K = 16 instruction) gives bit for bit the pieces of the v_and / v_sub form on 4 M float32 values of every kind, and the
    six-product sum of such pieces is at least as close to float64 as the f32 MFMA's own result.  (The kernels no longer issue
    either of the two: they take their remainders on the 4x4x4 instruction, which tests/test_gpu_rem4x4.py holds to the same bits.)"""
    import re
    import subprocess
    import micro_tool
    out = subprocess.run([micro_tool.bf16x6()], capture_output=True, text=True, timeout=300).stdout
    for k in (32, 16):
        m = re.search(r"MFMA remainders \(K = %d\): (\d+) of (\d+) piece words differ" % k, out)
        assert m, out[-2000:]
        assert int(m.group(1)) == 0 and int(m.group(2)) >= 6_000_000, m.group(0)
    bad = {name: int(n) for name, n in re.findall(r"^(truncated|truncated / MFMA remainders|truncated / MFMA remainders, K = 16) pieces: (\d+) of", out, re.M)}
    assert len(bad) == 3 and len(set(bad.values())) == 1, bad            # (only values whose pieces leave the normal float32 range)
    assert bad["truncated"] < 0.01 * 4194304, bad
    m = re.search(r"remainders by MFMA pieces\) ([0-9.e+-]+), f32 MFMA ([0-9.e+-]+)", out)
    assert m and float(m.group(1)) <= float(m.group(2)), out[:600]
