"""The reference's layer/model API (epnn_amd.charge_gn) on the GPU vs the CPU oracle. GPU only."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, random_weights

pytestmark = pytest.mark.gpu
TOL = 1e-5


def _small_state(golden_dir, nx):
    from epnn_amd import charge_gn
    path = os.path.join(golden_dir, "qm9_small") + "/"
    return charge_gn.gen_padded_init_state(path, 48, 48, n_elems=nx)


def _set(model_or_layers, w):
    model_or_layers.set_weights_dict(w)


@pytest.mark.parametrize("nx,T", [(9, 5), (10, 2)])
def test_make_model_dense_vs_oracle(golden_dir, nx, T):
    """model([h,e,x,q,mask]) with the literal (B,N,N,.) tensors: random non-degenerate weights vs float64 oracle."""
    from epnn_amd import charge_gn
    from oracle import epnn_oracle as orc
    x, h, q, e, Q, y, mask, names = _small_state(golden_dir, nx)
    w = random_weights(nx, T, seed=11, scale=0.35)
    model = charge_gn.make_model([32, 32], 48, T, nx, x.shape[1])
    model.set_weights_dict(w)
    pred = model([h, e, x, q, mask])
    assert pred.shape == (x.shape[0], x.shape[1], 1) and pred.dtype == np.float32
    ref = orc.model_forward(h, e, x, q, mask, w, dtype=np.float64)
    ref32 = orc.model_forward(h, e, x, q, mask, w, dtype=np.float32)
    err, noise = np.abs(pred - ref).max(), np.abs(ref32 - ref).max()
    print(f"dense model nx={nx} T={T}: |dq| {err:.3e}, float32 oracle noise {noise:.3e}")
    assert err <= max(TOL, 3 * noise)
    # padded atoms stay exactly zero, like in the reference
    for b in range(x.shape[0]):
        n = int(mask[b].sum(axis=0).max())
        assert np.all(pred[b, n:] == 0)


def test_make_model_golden_row(golden_dir, weights_decay, val_gold, val_names):
    """BASELINE.json configs[0]: QM9 single molecule through the infer.py plumbing vs the stored TF prediction."""
    from epnn_amd import charge_gn
    x, h, q, e, Q, y, mask, names = _small_state(golden_dir, 9)
    model = charge_gn.make_model([32, 32], 48, 5, 9, x.shape[1])
    model.load_weights(os.path.join(ROOT, "models", "decay_model_weights"))
    names = [str(n) for n in names]
    for nm in names:
        if nm not in val_names:
            continue
        k, g = names.index(nm), val_names.index(nm)
        pred = model([h[k:k + 1], e[k:k + 1], x[k:k + 1], q[k:k + 1], mask[k:k + 1]])
        n = int(mask[k].sum(axis=0).max())
        assert np.abs(pred[0, :n, 0] - val_gold[g, :n]).max() <= TOL


def test_layer_calls_vs_oracle(golden_dir):
    """GNN_layer.call and EPN_layer.call stand-alone (charge_gn.py:57,88) with non-trivial h and q inputs."""
    from epnn_amd import charge_gn
    from oracle import epnn_oracle as orc
    nx, T = 9, 3
    x, h, q, e, Q, y, mask, names = _small_state(golden_dir, nx)
    w = random_weights(nx, T, seed=5, scale=0.35)
    rng = np.random.default_rng(1)
    hx, xx, qx, m4 = orc.model_reduce(h, x, q, mask)
    hx = (rng.normal(size=hx.shape) * 0.2 * (xx[..., :1] != 0)).astype(np.float32)     # h only on real atoms
    qx = (qx + 0.05 * rng.normal(size=qx.shape) * (xx[..., :1] != 0)).astype(np.float32)
    gnn = charge_gn.GNN_layer(charge_gn.MLP_layer, charge_gn.MLP_layer([32, 32], out_dim=48), T)
    for t in range(T):
        gnn.message_fns[t].set_weights(w["msg"][t])
    gnn.update_fn.set_weights(w["upd"])
    h_gpu = gnn.call(hx, e, xx, qx, m4)
    h_ref = orc.gnn_layer(hx, e, xx, qx, m4, w["msg"], w["upd"], dtype=np.float64)
    h_r32 = orc.gnn_layer(hx, e, xx, qx, m4, w["msg"], w["upd"], dtype=np.float32)
    err, noise = np.abs(h_gpu - h_ref).max(), np.abs(h_r32 - h_ref).max()
    print(f"GNN_layer.call: |dh| {err:.3e} (noise {noise:.3e}, |h| up to {np.abs(h_ref).max():.2f})")
    assert err <= max(TOL, 3 * noise)
    epn = charge_gn.EPN_layer(charge_gn.MLP_layer, T=T)
    for t in range(T):
        epn.pass_fns[t].set_weights(w["pas"][t])
    q_gpu = epn.call(h_ref.astype(np.float32), e, xx, qx, m4)
    q_ref = orc.epn_layer(h_ref.astype(np.float32), e, xx, qx, m4, w["pas"], dtype=np.float64)
    q_r32 = orc.epn_layer(h_ref.astype(np.float32), e, xx, qx, m4, w["pas"], dtype=np.float32)
    err, noise = np.abs(q_gpu - q_ref).max(), np.abs(q_r32 - q_ref).max()
    print(f"EPN_layer.call: |dq| {err:.3e} (noise {noise:.3e})")
    assert err <= max(TOL, 3 * noise)
    # total charge is conserved by the layer (antisymmetric transfer)
    assert np.abs(q_gpu.sum(axis=(1, 2)) - qx.sum(axis=(1, 2))).max() < 2e-6


def test_small_dense_calls_take_the_short_sequence_with_the_same_bits(golden_dir):
    """model([h,e,x,q,mask]) on one or a few molecules builds its per-atom features, flags, effective atom counts and pair
    list in four launches ("dense_small", default) instead of two memsets, seven kernels and a download; the flags are the
    call's generation number, so no call clears them.  Same bits as the general sequence, call after call on ONE handle, a
    large molecule followed by a small one (stale flags of an earlier generation must not count), batches of one and three."""
    from epnn_amd import charge_gn
    x, h, q, e, Q, y, mask, names = _small_state(golden_dir, 9)
    w = random_weights(9, 3, seed=5, scale=0.35)
    N = x.shape[1]
    sizes = [int(mask[b].sum(axis=0).max()) for b in range(x.shape[0])]
    order = list(np.argsort(sizes)[::-1]) + list(np.argsort(sizes))        # largest first, then smallest first
    model = charge_gn.make_model([32, 32], 48, 3, 9, N)
    model.set_weights_dict(w)
    eng = model.engine()
    eng.set_option("dense_rowfused", 0)                      # (its own test below: a different arithmetic form, not the same bits)
    cases = [[b] for b in order] + [order[:3], order[-3:]]
    outs = {0: [], 1: []}
    for opt in (1, 0):
        eng.set_option("dense_small", opt)
        for sel in cases:
            sel = np.asarray(sel)
            outs[opt].append(model([h[sel], e[sel], x[sel], q[sel], mask[sel]]))
    for a, b_, sel in zip(outs[1], outs[0], cases):
        assert np.array_equal(a, b_), sel
        for r, b in enumerate(sel):
            assert np.all(a[r, sizes[b]:] == 0) and np.any(a[r, :sizes[b]] != 0)


@pytest.mark.parametrize("nx,T", [(9, 5), (10, 2)])
def test_lone_molecules_take_the_row_fused_forward(golden_dir, nx, T):
    """model([h,e,x,q,mask]) on ONE molecule (or a few, B N <= 256) runs the row-fused forward kernels of the training step --
    a workgroup per atom slot, the reference's literal rows -- instead of the fused inference kernel on one CU
    ("dense_rowfused", default): always when the padded size is at most 48 (no effective atom counts needed: no host
    synchronisation inside the call), and beyond that when the largest molecule fills more than 55 % of the padded size.
    Same answers as the float64 oracle to the tolerance of the other dense tests and as the fused kernels to float32 rounding;
    padded atoms exactly zero; epnn_last_stats shows the path (0 molecules on the fused and on the tiled kernels)."""
    from epnn_amd import charge_gn, synth
    from oracle import epnn_oracle as orc
    w = random_weights(nx, T, seed=17, scale=0.35)

    def check(model, ins, sizes, expect_rowfused, tag):
        eng = model.engine()
        eng.set_option("dense_rowfused", 1)
        pred = model(ins)
        st = eng.last_stats()
        assert (int(st[1]) + int(st[2]) == 0) == expect_rowfused, (tag, st)
        eng.set_option("dense_rowfused", 0)
        pred0 = model(ins)
        st0 = eng.last_stats()
        assert int(st0[1]) + int(st0[2]) == len(sizes)
        ref = orc.model_forward(*ins, w, dtype=np.float64)
        ref32 = orc.model_forward(*ins, w, dtype=np.float32)
        err, noise = np.abs(pred - ref).max(), np.abs(ref32 - ref).max()
        print(f"row-fused dense call nx={nx} T={T} {tag}: |dq| {err:.3e} (fused kernels {np.abs(pred0 - ref).max():.3e}, float32 oracle {noise:.3e})")
        assert err <= max(TOL, 3 * noise)
        assert np.abs(pred - pred0).max() <= max(TOL, 3 * noise)
        for r, n in enumerate(sizes):
            assert np.all(pred[r, n:] == 0) and np.any(pred[r, :n] != 0)

    # (a) the golden QM9 molecules padded to N = 26: every call takes the row-fused kernels, whatever the molecule's size
    x, h, q, e, Q, y, mask, names = _small_state(golden_dir, nx)
    N = x.shape[1]
    sizes = [int(mask[b].sum(axis=0).max()) for b in range(x.shape[0])]
    big, small, Np = int(np.argmax(sizes)), int(np.argmin(sizes)), 26

    def pad(a, sel):                                         # (B, N, N, C) -> the selected molecules, zero padded to (Np, Np)
        out = np.zeros((len(sel), Np, Np) + a.shape[3:], a.dtype)
        out[:, :N, :N] = a[sel]
        return out
    model = charge_gn.make_model([32, 32], 48, T, nx, Np)
    model.set_weights_dict(w)
    for sel in ([big], [small], [big, small]):
        check(model, [pad(a, sel) for a in (h, e, x, q, mask)], [sizes[b] for b in sel], True, f"N={Np} molecules {sel}")

    # (b) N = 60: a 40-atom molecule fills two thirds of it (row-fused), a 12-atom one a fifth (the fused kernel as before)
    Nb = 60
    rng = np.random.default_rng(8)
    model = charge_gn.make_model([32, 32], 48, T, nx, Nb)
    model.set_weights_dict(w)

    def synth_batch(ns):
        B = len(ns)
        hh = np.zeros((B, Nb, Nb, 48), np.float32); ee = np.zeros((B, Nb, Nb, 48), np.float32)
        xx = np.zeros((B, Nb, Nb, nx), np.float32); qq = np.zeros((B, Nb, Nb, 1), np.float32); mm = np.zeros((B, Nb, Nb, 1), np.float32)
        for b, n in enumerate(ns):
            span = 1.6 * n ** (1 / 3.0) * 1.3
            while True:
                pts = rng.uniform(0, span, size=(n, 3))
                d = np.linalg.norm(pts[:, None] - pts[None], axis=-1) + np.eye(n) * 10
                if d.min() > 0.8:
                    break
            ee[b, :n, :n] = charge_gn.get_init_edges(pts.astype(np.float32), np.array([]), num=48)[0]
            f = synth.features(rng.choice(["H", "C", "N", "O"], size=n))
            xx[b, :n, :n, :f.shape[1]] = f[None]
            hh[b, :n, :n] = (rng.normal(size=(n, 48)) * 0.2).astype(np.float32)[None]
            qq[b, :n, :n, 0] = np.float32(rng.integers(-1, 2)) / np.float32(n)
            mm[b, :n, :n, 0] = 1
        return [hh, ee, xx, qq, mm]
    for ns, expect in (([40], True), ([12], False), ([40, 12], True)):
        check(model, synth_batch(ns), ns, expect, f"N={Nb} sizes {ns}")


def test_arbitrary_dense_inputs(golden_dir):
    """Inputs gen_padded_init_state never produces: non-symmetric e, non-zero diagonal, fractional and
    non-symmetric masks, atoms with e but no mask.  The pair list must not assume symmetry."""
    from epnn_amd import charge_gn
    from oracle import epnn_oracle as orc
    nx, T, B, N = 9, 2, 3, 12
    rng = np.random.default_rng(3)
    w = random_weights(nx, T, seed=9, scale=0.35)
    n_real = [12, 9, 5]
    e = np.zeros((B, N, N, 48), dtype=np.float32)
    mask = np.zeros((B, N, N, 1), dtype=np.float32)
    x = np.zeros((B, N, nx), dtype=np.float32)
    h = np.zeros((B, N, 48), dtype=np.float32)
    q = np.zeros((B, N, 1), dtype=np.float32)
    for b, n in enumerate(n_real):
        dense = rng.random((n, n)) < 0.5
        ev = (rng.random((n, n, 48)) * 0.3 * dense[..., None]).astype(np.float32)
        sym = rng.random((n, n)) < 0.5                       # half of the pairs symmetric, the rest not
        evs = np.where(sym[..., None] & sym.T[..., None], np.maximum(ev, ev.transpose(1, 0, 2)), ev)
        e[b, :n, :n] = evs
        mask[b, :n, :n, 0] = rng.choice([0.0, 0.5, 1.0], size=(n, n), p=[0.1, 0.2, 0.7])
        x[b, :n, 0] = rng.choice([1, 6, 7, 8], size=n)
        x[b, np.arange(n), 1 + rng.integers(0, 4, size=n)] = 1
        h[b, :n] = rng.normal(size=(n, 48)) * 0.2
        q[b, :n, 0] = rng.normal(size=n) * 0.1
    e[1, 3, 3] = 0.2                                           # diagonal entry
    gnn = charge_gn.GNN_layer(charge_gn.MLP_layer, charge_gn.MLP_layer([32, 32], out_dim=48), T)
    epn = charge_gn.EPN_layer(charge_gn.MLP_layer, T=T)
    for t in range(T):
        gnn.message_fns[t].set_weights(w["msg"][t])
        epn.pass_fns[t].set_weights(w["pas"][t])
    gnn.update_fn.set_weights(w["upd"])
    h_gpu = gnn.call(h, e, x, q, mask)
    h_ref = orc.gnn_layer(h, e, x, q, mask, w["msg"], w["upd"], dtype=np.float64)
    h_r32 = orc.gnn_layer(h, e, x, q, mask, w["msg"], w["upd"], dtype=np.float32)
    assert np.abs(h_gpu - h_ref).max() <= max(TOL, 3 * np.abs(h_r32 - h_ref).max())
    q_gpu = epn.call(h, e, x, q, mask)
    q_ref = orc.epn_layer(h, e, x, q, mask, w["pas"], dtype=np.float64)
    q_r32 = orc.epn_layer(h, e, x, q, mask, w["pas"], dtype=np.float32)
    err, noise = np.abs(q_gpu - q_ref).max(), np.abs(q_r32 - q_ref).max()
    print(f"arbitrary dense inputs: |dq| {err:.3e} (noise {noise:.3e})")
    assert err <= max(TOL, 3 * noise)


def test_mlp_layer_call():
    from epnn_amd import charge_gn
    from oracle import epnn_oracle as orc
    rng = np.random.default_rng(0)
    for n_in, n_out, rows in [(164, 32, 1000), (80, 48, 77), (166, 1, 5)]:
        mlp = charge_gn.MLP_layer([32, 32], out_dim=n_out)
        xs = rng.normal(size=(rows, n_in)).astype(np.float32)
        out = mlp(xs)
        ref = orc.mlp(xs.astype(np.float64), [(k.astype(np.float64), b.astype(np.float64)) for k, b in mlp.get_weights()])
        assert out.shape == (rows, n_out)
        assert np.abs(out - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max())


def test_edges_device_vs_host(golden_dir):
    from epnn_amd import charge_gn
    from epnn_amd.engine import Engine
    fx = np.load(os.path.join(golden_dir, "edges_081300.npz"))
    eng = Engine(nx=9, T=1)
    e_dev = eng.edges(fx["xyz"])
    eng.close()
    assert e_dev.shape == fx["e"].shape
    # float64 cos/exp on the device vs glibc: identical after rounding to float32 except at rounding boundaries
    assert np.abs(e_dev - fx["e"]).max() <= 1e-7
    assert np.mean(e_dev != fx["e"]) < 1e-3
    assert np.array_equal(e_dev > 1e-5, fx["e"] > 1e-5)


def test_infer_entry_point(tmp_path):
    """infer.py flow end to end (BASELINE.json configs[0] plumbing) in a subprocess."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "infer.py"), "--batched", "--repeats", "2"],
                         cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "avg inference time:" in out.stdout and "avg feature time:" in out.stdout
    assert os.path.exists(tmp_path / "test_names.npy")
    piped = [l for l in out.stdout.splitlines() if l.startswith("pipelined compact entry")][0]
    assert float(piped.rsplit(" ", 1)[1]) == 0.0            # bit-identical to the one-call batch
    line = [l for l in out.stdout.splitlines() if l.startswith("batched compact entry")][0]
    assert float(line.rsplit(" ", 1)[1]) <= 2e-6


@pytest.mark.parametrize("launcher", ["self", "torchrun"])
def test_bench_two_ranks_on_this_box(tmp_path, launcher):
    """`python bench.py --gpus 2` WITHOUT a launcher starts its two rank processes itself (fresh children; on a one-GPU box
    they share the device and the timing exchange runs over gloo) and prints ONE valid JSON line with n_gpus = 2, the
    per-rank rates and their sum; the torch.distributed.run form gives the same kind of line."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    args = [os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "40", "--warmup", "6", "--full", "--no-cpu-baseline", "--no-extras"]
    if launcher == "self":
        cmd = [sys.executable] + args
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
               "--master-port", "29541"] + args
    out = subprocess.run(cmd, cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    o = json.loads(lines[0])
    assert o["n_gpus"] == 2 and o["steps"] == 40 and o["unit"] == "atoms/s" and o["scaling"] == "weak" and o["dtype"] == "f32"
    assert o["config"]["workload"] == "qm9_like_b1024_N29" and o["vs_baseline"] is None
    per = o["ranks"]["atoms_per_s_per_rank"]
    assert o["ranks"]["world_size"] == 2 and len(per) == 2
    # one GPU on this box: RCCL refuses two ranks on a device, the timing exchange goes over the rendezvous store; with two
    # devices it is the library's communicator and both ranks must have joined it
    if o["ranks"]["rccl_ranks"] is None:
        assert o["ranks"]["timing_backend"].startswith("rendezvous") and o["ranks"]["ranks_per_device"] == 2
        assert o["ranks"]["hw_queues_per_rank"] <= 4              # ranks that share a device take fewer hardware queues each
    else:
        assert o["ranks"]["timing_backend"].startswith("rccl") and o["ranks"]["rccl_ranks"] == 2
    # max-over-ranks time: value <= sum of the rates; and two ranks sharing the GPU must not fall off the queue cliff of round 2
    # (13.6 M atoms/s in total with 16 hardware queues per rank beside this process's own: gpurun_out/r2_fulltests2.log)
    assert 0.5 * sum(per) < o["value"] <= 1.001 * sum(per) and o["value"] > 5e7
    assert 0 < o["roofline"]["frac"] < 1.0 and o["roofline"]["bound"] == "mfma"
    assert "import torch" not in open(os.path.join(ROOT, "bench.py")).read()          # the timing exchange is the library's own


def test_bench_line_of_the_drivers_command(tmp_path):
    """`python bench.py --gpus 1 --steps 20 --warmup 5 --full`: ONE JSON line on stdout with every field of the contract,
    the roofline and CPU-baseline objects, and this project's extras."""
    import json
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    # the hardware queues the bounds below were set with (bench.py's own choice for one rank per device, _lib.load's default);
    # a smaller count inherited from the environment puts several lanes on one queue and the line reads ~30 % lower
    env["GPU_MAX_HW_QUEUES"] = "16"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--full"],
                         cwd=tmp_path, env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), out.stdout[-2000:]
    o = json.loads(lines[0])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "value_cold", "prewarm_ms"):
        assert key in o, key
    # the cold figure stands beside `value`; the warmed-up timed region is not allowed to read more than 10 % under it (what a host
    # thread that woke up late from the completion interrupt did once in round 4: 172 M against 189 M cold -- sync_spin_us fixed it)
    assert 0.5 * o["value"] < o["value_cold"] and o["value"] >= 0.9 * o["value_cold"] and o["prewarm_ms"] > 10
    assert o["n_gpus"] == 1 and o["steps"] == 20 and o["warmup"] == 5 and o["higher_is_better"] is True
    assert o["unit"] == "atoms/s" and o["dtype"] == "f32" and o["data"] == "synthetic" and o["vs_baseline"] is None
    assert o["config"]["workload"] == "qm9_like_b1024_N29" and "model" not in o["config"]
    assert abs(o["value"] - o["config"]["atoms_per_gpu"] / (o["ms_per_step"] * 1e-3)) <= 1e-6 * o["value"]
    r = o["roofline"]
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in r, key
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-9 and 0.3 < r["frac"] < 1.0
    c = o["cpu_baseline"]
    for key in ("value", "unit", "cores", "kind", "sample"):
        assert key in c, key
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0
    assert o["parity"]["max_abs_dq_vs_reference"] <= 1e-5 and o["parity"]["systems"] == 871
    for key in ("real_data", "host_to_host", "blocking_call", "order"):
        assert key in o, key
    assert o["blocking_call"]["ms"] < o["blocking_call"]["ms_one_wavefront_per_molecule"]


def test_bench_plain_line_and_dumped_outputs(tmp_path, weights_decay):
    """A plain `python bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` (no --full): ONE JSON line with the
    contract's fields and none of the --full measurements; DIR/charges.npy holds the charges of the last timed step of the
    bench batch, the same whichever lane ran that step (K = 20 and K = 7), and equal to a forward of that batch here."""
    import json
    from epnn_amd import synth
    from epnn_amd.engine import Engine
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    dumps = []
    for steps in (20, 7):
        d = tmp_path / f"out{steps}"
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "5",
                              "--dump-outputs", str(d)], cwd=tmp_path, env=env, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        lines = [l for l in out.stdout.splitlines() if l.strip()]
        assert len(lines) == 1 and lines[0].startswith("{"), out.stdout[-2000:]
        o = json.loads(lines[0])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "n_gpus", "steps", "warmup", "config"):
            assert key in o, key
        assert o["steps"] == steps and o["warmup"] == 5 and o["n_gpus"] == 1 and o["higher_is_better"] is True
        assert o["unit"] == "atoms/s" and o["dtype"] == "f32" and o["config"]["workload"] == "qm9_like_b1024_N29"
        assert abs(o["value"] - o["config"]["atoms_per_gpu"] / (o["ms_per_step"] * 1e-3)) <= 1e-6 * o["value"]
        for key in ("roofline", "cpu_baseline", "value_cold", "parity", "real_data", "host_to_host", "blocking_call"):
            assert key not in o, key
        assert sorted(os.listdir(d)) == ["charges.npy"]
        q = np.load(d / "charges.npy")
        assert q.dtype == np.float32 and q.shape == (o["config"]["atoms_per_gpu"],)
        dumps.append(q)
    assert np.array_equal(dumps[0], dumps[1])
    offsets, xyz, x, Q, N = synth.qm9_like_batch(B=1024, seed=0, N=29)
    assert np.isfinite(dumps[0]).all()
    assert np.abs(np.add.reduceat(dumps[0].astype(np.float64), offsets[:-1]) - Q).max() < 1e-4
    eng = Engine(nx=9, T=5)
    eng.set_weights(weights_decay)
    eng.set_option("wave2", 0)                              # the bench's kernel
    ref = eng.forward_xyz(offsets, xyz, x, Q, N)
    eng.close()
    assert np.abs(dumps[0] - ref).max() <= 1e-6


def test_smoke_entry():
    import __graft_entry__ as g
    g.smoke()


def test_error_behaviour_at_the_boundary(weights_decay):
    """Bad calls come back as EpnnError with the C side's message (epnn_last_error), never as a crash or a silent
    result; the handle stays usable afterwards."""
    from epnn_amd import synth
    from epnn_amd._lib import EpnnError
    from epnn_amd.engine import Engine
    eng = Engine(nx=9, T=5)
    eng.set_weights(weights_decay)
    offsets, xyz, x, Q, N = synth.qm9_like_batch(B=8, seed=3)
    good = eng.forward_xyz(offsets, xyz, x, Q, N)
    with pytest.raises(EpnnError, match="padded size"):
        eng.forward_xyz(offsets, xyz, x, Q, 5)                      # a molecule does not fit N
    bad = offsets.copy()
    bad[0] = 1
    with pytest.raises(EpnnError):
        eng.forward_xyz(bad, xyz, x, Q, N)                          # offsets must start at 0
    with pytest.raises(EpnnError, match="shapes"):
        eng.forward_xyz(offsets, xyz[:-1], x, Q, N)                 # arrays do not match the offsets
    bad = offsets.copy()
    bad[3], bad[4] = offsets[4], offsets[3]                         # not ascending: refused before any buffer is sized or
    with pytest.raises(EpnnError, match="atoms"):                   # indexed by an offset
        eng.forward_xyz(bad, xyz, x, Q, N)
    d = [eng.to_device(a) for a in (xyz, x, Q)] + [eng.alloc(int(offsets[-1]) * 4)]
    with pytest.raises(EpnnError, match="atoms"):
        eng.forward_xyz_dev(bad, d[0], d[1], d[2], d[3], N)
    with pytest.raises(EpnnError, match="unknown option"):
        eng.set_option("no_such_option", 1)
    eng.forward_xyz_begin(offsets, xyz, x, Q, N)
    with pytest.raises(EpnnError, match="collect the previous forward"):
        eng.forward_xyz_begin(offsets, xyz, x, Q, N)                # one forward per handle between begin and end
    assert np.array_equal(eng.forward_xyz_end(), good)
    with pytest.raises(EpnnError):
        eng.train_step_xyz(offsets, xyz, x, Q, np.zeros(int(offsets[-1]), np.float32), N)    # train_init not called
    assert np.array_equal(eng.forward_xyz(offsets, xyz, x, Q, N), good)                     # still usable
    eng.close()
    with pytest.raises(EpnnError, match="e_dim"):
        Engine(nx=9, T=5, h_dim=32)                                 # e_dim must equal h_dim (charge_gn.py:377)
    with pytest.raises(EpnnError, match="1..48"):
        Engine(nx=9, T=5, h_dim=64, e_dim=64)                       # the kernels hold 48 channels


def test_layer_calls_on_a_system_for_the_tiled_kernels():
    """GNN_layer.call / EPN_layer.call / the model on dense inputs of a 50-atom system next to a 20-atom one, padded to 56:
    the larger one runs on the tiled kernels (n > 32), with h, q and the node mask coming from the caller."""
    from epnn_amd import charge_gn
    from oracle import epnn_oracle as orc
    nx, T, N = 9, 2, 56
    rng = np.random.default_rng(7)
    mols = []
    for n in (50, 20):
        xyz = (rng.normal(size=(n, 3)) * 2.6).astype(np.float32)
        x = np.zeros((n, nx), np.float32)
        x[np.arange(n), rng.integers(1, nx, size=n)] = 1
        x[:, 0] = rng.integers(1, 10, size=n)
        mols.append(orc.dense_inputs(xyz, x, np.float32(1.0), N))
    h, e, x, q, mask = (np.stack([m[k] for m in mols]) for k in range(5))
    w = random_weights(nx, T, seed=21, scale=0.35)
    hx, xx, qx, m4 = orc.model_reduce(h, x, q, mask)
    hx = (rng.normal(size=hx.shape) * 0.2 * (xx[..., :1] != 0)).astype(np.float32)
    qx = (qx + 0.05 * rng.normal(size=qx.shape) * (xx[..., :1] != 0)).astype(np.float32)
    gnn = charge_gn.GNN_layer(charge_gn.MLP_layer, charge_gn.MLP_layer([32, 32], out_dim=48), T)
    for t in range(T):
        gnn.message_fns[t].set_weights(w["msg"][t])
    gnn.update_fn.set_weights(w["upd"])
    h_gpu = gnn.call(hx, e, xx, qx, m4)
    h_ref = orc.gnn_layer(hx, e, xx, qx, m4, w["msg"], w["upd"], dtype=np.float64)
    h_r32 = orc.gnn_layer(hx, e, xx, qx, m4, w["msg"], w["upd"], dtype=np.float32)
    assert np.abs(h_gpu - h_ref).max() <= max(TOL, 3 * np.abs(h_r32 - h_ref).max())
    epn = charge_gn.EPN_layer(charge_gn.MLP_layer, T=T)
    for t in range(T):
        epn.pass_fns[t].set_weights(w["pas"][t])
    q_gpu = epn.call(h_ref.astype(np.float32), e, xx, qx, m4)
    q_ref = orc.epn_layer(h_ref.astype(np.float32), e, xx, qx, m4, w["pas"], dtype=np.float64)
    q_r32 = orc.epn_layer(h_ref.astype(np.float32), e, xx, qx, m4, w["pas"], dtype=np.float32)
    assert np.abs(q_gpu - q_ref).max() <= max(TOL, 3 * np.abs(q_r32 - q_ref).max())
    assert np.abs(q_gpu.sum(axis=(1, 2)) - qx.sum(axis=(1, 2))).max() < 5e-6
    model = charge_gn.make_model([32, 32], 48, T, nx, N)
    model.set_weights_dict(w)
    p_gpu = model([h, e, x, q, mask])
    p_ref = orc.model_forward(h, e, x, q, mask, w, np.float64)
    p_r32 = orc.model_forward(h, e, x, q, mask, w, np.float32)
    assert np.abs(p_gpu - p_ref).max() <= max(TOL, 3 * np.abs(p_r32 - p_ref).max())


def test_fractional_node_mask():
    """node_mask = clip(sum_i mask[i, j], 0, 1) (charge_gn.py:59) is fractional when an atom's mask column sums to less than
    1 -- tiny systems with fractional masks.  It multiplies the update MLP's input and its output once each (:72, :74).
    (Found by tests/fuzz_dense.py: the h block of the first step used to be masked twice.)"""
    from epnn_amd import charge_gn
    from oracle import epnn_oracle as orc
    nx, T = 9, 2
    rng = np.random.default_rng(2)
    w = random_weights(nx, T, seed=13, scale=0.35)
    e = (rng.random((2, 3, 3, 48)) * 0.3).astype(np.float32)
    mask = np.zeros((2, 3, 3, 1), np.float32)
    mask[0, :2, :2, 0] = [[1.0, 0.5], [1.0, 0.0]]             # node masks 1, 0.5 (and 0 for the padded third atom)
    mask[1, :, :, 0] = [[0.5, 0.0, 0.5], [0.0, 0.0, 0.0], [0.0, 0.5, 0.0]]       # node masks 0.5, 0.5, 0.5
    e[0, 2] = 0
    e[0, :, 2] = 0
    x = np.zeros((2, 3, nx), np.float32)
    x[:, :, 0] = [[7, 1, 0], [6, 8, 1]]
    x[0, :2, 4] = 1
    x[1, :, 2] = 1
    h = (rng.normal(size=(2, 3, 48)) * 0.2).astype(np.float32)
    h[0, 2] = 0
    q = (rng.normal(size=(2, 3, 1)) * 0.1).astype(np.float32)
    q[0, 2] = 0
    gnn = charge_gn.GNN_layer(charge_gn.MLP_layer, charge_gn.MLP_layer([32, 32], out_dim=48), T)
    for t in range(T):
        gnn.message_fns[t].set_weights(w["msg"][t])
    gnn.update_fn.set_weights(w["upd"])
    h_gpu = gnn.call(h, e, x, q, mask)
    h_ref = orc.gnn_layer(h, e, x, q, mask, w["msg"], w["upd"], dtype=np.float64)
    assert np.abs(h_gpu - h_ref).max() < 2e-6, np.abs(h_gpu - h_ref).max()


def test_make_model_every_size_class_on_the_block_per_wave_kernel():
    """model([h,e,x,q,mask]) on molecules of every size class of the block-per-wavefront kernel's dense-input form
    (epnn_wave2.hip.h, !FRONT: pair lists and 48-channel e rows from the dense front-end, h given): two to a workgroup
    (<= 16 atoms), split over two (17..32) and three wavefronts (33..48) -- float64 oracle, non-zero h, and the same call
    with the kernel switched off ("wave2" = 0, "wave3" = 0: k_wave_forward and the tiled kernels)."""
    from epnn_amd import charge_gn, synth
    from oracle import epnn_oracle as orc
    nx, T, N = 9, 3, 48
    sizes = [3, 11, 16, 17, 20, 25, 32, 33, 38, 41, 48]
    rng = np.random.default_rng(31)
    B = len(sizes)
    h = np.zeros((B, N, N, 48), np.float32); e = np.zeros((B, N, N, 48), np.float32)
    x = np.zeros((B, N, N, nx), np.float32); q = np.zeros((B, N, N, 1), np.float32); mask = np.zeros((B, N, N, 1), np.float32)
    for b, n in enumerate(sizes):
        span = 1.6 * n ** (1 / 3.0) * 1.3
        while True:
            pts = rng.uniform(0, span, size=(n, 3))
            d = np.linalg.norm(pts[:, None] - pts[None], axis=-1) + np.eye(n) * 10
            if d.min() > 0.8:
                break
        eb, _ = charge_gn.get_init_edges(pts.astype(np.float32), np.array([]), num=48)
        e[b, :n, :n] = eb
        x[b, :n, :n] = synth.features(rng.choice(["H", "C", "N", "O"], size=n))[None]
        h[b, :n, :n] = (rng.normal(size=(n, 48)) * 0.2).astype(np.float32)[None]
        q[b, :n, :n, 0] = np.float32(rng.integers(-1, 2)) / np.float32(n)
        mask[b, :n, :n, 0] = 1
    w = random_weights(nx, T, seed=17, scale=0.35)
    model = charge_gn.make_model([32, 32], 48, T, nx, N)
    model.set_weights_dict(w)
    pred = model([h, e, x, q, mask])
    ref = orc.model_forward(h, e, x, q, mask, w, dtype=np.float64)
    ref32 = orc.model_forward(h, e, x, q, mask, w, dtype=np.float32)
    err, noise = np.abs(pred - ref).max(), np.abs(ref32 - ref).max()
    st = model.engine().last_stats()
    assert st[1] == B and st[2] == 0, st                         # every molecule on the fused kernels
    model.engine().set_option("wave2", 0)
    model.engine().set_option("wave3", 0)
    other = model([h, e, x, q, mask])
    st = model.engine().last_stats()
    assert st[2] == sum(1 for n in sizes if n > 32), st           # 33..48 on the tiled kernels now
    print(f"dense model, sizes {sizes}: |dq| {err:.3e} (float32 oracle noise {noise:.3e}); |block-per-wave - other kernels| {np.abs(pred - other).max():.2e}")
    assert err <= max(TOL, 4 * noise)
    assert np.abs(other - ref).max() <= max(TOL, 4 * noise) and np.abs(pred - other).max() <= max(2e-6, 4 * noise)


def _upd_layers(widths, seed):
    """Glorot kernels + biases of an update MLP 80 -> widths... -> 48 (charge_gn.py:371)."""
    rng = np.random.default_rng(seed)
    dims = [80] + list(widths) + [48]
    out = []
    for i, o in zip(dims[:-1], dims[1:]):
        lim = 0.35 * np.sqrt(6.0 / (i + o))
        out.append((rng.uniform(-lim, lim, (i, o)).astype(np.float32), rng.uniform(-0.1, 0.1, (o,)).astype(np.float32)))
    return out


@pytest.mark.parametrize("nodes,out_dim", [([16], 5), ([64, 32], 7), ([20, 30, 40], 3), ([], 48), ([256], 1)])
def test_mlp_layer_call_with_any_nodes(nodes, out_dim):
    """MLP_layer(nodes, out_dim).call for other `nodes` than the reference's own [32, 32] (charge_gn.py:31-45): the generic
    Dense stack (epnn_mlp_forward_layers) vs the float64 oracle; `nodes = []` is a single linear Dense."""
    from epnn_amd import charge_gn
    from oracle import epnn_oracle as orc
    rng = np.random.default_rng(len(nodes) + out_dim)
    rows = rng.normal(size=(3, 37, 23)).astype(np.float32)
    m = charge_gn.MLP_layer(nodes, out_dim=out_dim)
    dims = [23] + list(nodes) + [out_dim]
    ws = [((rng.normal(size=(i, o)) / np.sqrt(i)).astype(np.float32), (0.1 * rng.normal(size=(o,))).astype(np.float32))
          for i, o in zip(dims[:-1], dims[1:])]
    m.build(23)
    m.set_weights(ws)
    got = m.call(rows)
    ref = orc.mlp(rows.reshape(-1, 23).astype(np.float64), orc._cast_layers(ws, np.float64)).reshape(3, 37, out_dim)
    assert got.shape == (3, 37, out_dim) and got.dtype == np.float32
    assert np.abs(got - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max())


@pytest.mark.parametrize("activation", [None, "linear", "tanh", "sigmoid", "relu"])
@pytest.mark.parametrize("nodes", [[32, 32], [20]])
def test_mlp_layer_call_with_other_activations(nodes, activation):
    """MLP_layer(nodes, out_dim, activation).call (charge_gn.py:31,38: `activation` goes to every Dense but the last): the Keras names
    None / 'linear', 'tanh', 'sigmoid' next to the default 'relu' vs the float64 oracle; anything else, and any non-relu MLP inside a
    GNN / EPN stack, is refused loudly."""
    from epnn_amd import charge_gn
    from epnn_amd._lib import EpnnError
    from oracle import epnn_oracle as orc
    rng = np.random.default_rng(7 + len(nodes))
    rows = rng.normal(size=(5, 29, 17)).astype(np.float32)
    m = charge_gn.MLP_layer(nodes, out_dim=3, activation=activation)
    dims = [17] + list(nodes) + [3]
    ws = [((rng.normal(size=(i, o)) / np.sqrt(i)).astype(np.float32), (0.1 * rng.normal(size=(o,))).astype(np.float32))
          for i, o in zip(dims[:-1], dims[1:])]
    m.build(17)
    m.set_weights(ws)
    got = m(rows)
    ref = orc.mlp(rows.reshape(-1, 17).astype(np.float64), orc._cast_layers(ws, np.float64), activation).reshape(5, 29, 3)
    assert got.shape == (5, 29, 3) and got.dtype == np.float32
    assert np.abs(got - ref).max() <= 2e-5 * max(1.0, np.abs(ref).max())         # float32 Dense stack + tanhf / expf vs float64
    if activation not in (None, "linear", "relu"):                             # the activation really ran
        lin = orc.mlp(rows.reshape(-1, 17).astype(np.float64), orc._cast_layers(ws, np.float64), None).reshape(5, 29, 3)
        assert np.abs(got - lin).max() > 1e-2
    with pytest.raises(ValueError, match="not built"):
        charge_gn.MLP_layer(nodes, activation="selu")
    if activation != "relu":
        class Tanh(charge_gn.MLP_layer):
            def __init__(self, nodes, out_dim=1):
                super().__init__(nodes, out_dim, activation=activation)
        gnn = charge_gn.GNN_layer(Tanh, charge_gn.MLP_layer([32, 32], out_dim=48), 1)
        z = np.zeros((1, 4, 4, 48), np.float32)
        with pytest.raises(EpnnError, match="built for 'relu'"):
            gnn(np.zeros((1, 4, 48), np.float32), z, np.zeros((1, 4, 9), np.float32), np.zeros((1, 4, 1), np.float32), np.ones((1, 4, 4, 1), np.float32))


@pytest.mark.parametrize("h_dim,layers", [(32, [32, 32]), (20, [64, 32]), (7, [12, 20, 9])])
def test_make_model_with_other_h_dim(golden_dir, val_dir, val_names, tmp_path, h_dim, layers):
    """make_model(layers, h_dim, ...) with h_dim below the 48 of the reference's scripts (charge_gn.py:369-377: h_inp and e_inp have
    h_dim channels, the update MLP ends in h_dim units, gen_padded_init_state(path, h_dim, e_dim) builds e from e_dim Gaussians).
    The library runs such a model as a 48-channel one with zero channels / zero kernel rows and columns (include/epnn.h): every
    tensor and weight at the interface has the model's own shapes.  The literal dense call, the compact entry on the three kernel
    families, GNN_layer.call / EPN_layer.call, get_init_edges, the checkpoint round trip, the training step's gradients (flat vector
    in the model's shapes) and an optimizer step, each vs the float64 oracle on the model as the reference would build it."""
    from epnn_amd import charge_gn, synth
    from epnn_amd._lib import EpnnError
    from epnn_amd.engine import Engine
    from oracle import epnn_oracle as orc
    from oracle import epnn_oracle_train as ot
    from conftest import load_molecules
    nx, T = 9, 3
    w = random_weights(nx, T, seed=41, scale=0.35, h_dim=h_dim)
    dims = [h_dim + 32] + list(layers) + [h_dim]
    rng = np.random.default_rng(h_dim)
    w["upd"] = [(rng.uniform(-1, 1, (i, o)).astype(np.float32) * np.float32(0.35 * np.sqrt(6.0 / (i + o))), rng.uniform(-0.1, 0.1, (o,)).astype(np.float32))
                for i, o in zip(dims[:-1], dims[1:])]
    # (1) the literal make_model call on gen_padded_init_state(path, h_dim, h_dim)
    path = os.path.join(golden_dir, "qm9_small") + "/"
    x, h, q, e, Q, y, mask, names = charge_gn.gen_padded_init_state(path, h_dim, h_dim, n_elems=nx)
    assert h.shape[-1] == h_dim and e.shape[-1] == h_dim
    model = charge_gn.make_model(layers, h_dim, T, nx, x.shape[1])
    model.set_weights_dict(w)
    pred = model([h, e, x, q, mask])
    ref = orc.model_forward(h, e, x, q, mask, w, dtype=np.float64)
    noise = np.abs(orc.model_forward(h, e, x, q, mask, w, dtype=np.float32) - ref).max()
    err = np.abs(pred - ref).max()
    print(f"h_dim {h_dim}, layers {layers}: dense call |dq| {err:.3e} (float32 oracle noise {noise:.3e})")
    assert err <= max(TOL, 3 * noise)
    # (2) weights come back in the model's shapes; checkpoint round trip
    w_back = model.engine().get_weights()
    for key in ("msg", "pas"):
        for t in range(T):
            for (k0, b0), (k1, b1) in zip(w[key][t], w_back[key][t]):
                assert k0.shape == k1.shape and np.array_equal(k0, k1) and np.array_equal(b0, b1)
    for (k0, b0), (k1, b1) in zip(w["upd"], w_back["upd"]):
        assert k0.shape == k1.shape and np.array_equal(k0, k1) and np.array_equal(b0, b1)
    model.save_weights(str(tmp_path / "m"))
    again = charge_gn.make_model(layers, h_dim, T, nx, x.shape[1])
    again.load_weights(str(tmp_path / "m"))
    assert np.array_equal(again([h, e, x, q, mask]), pred)
    # (3) get_init_edges of the handle: e_dim Gaussians
    eng = Engine(nx=nx, T=T, h_dim=h_dim, e_dim=h_dim)
    eng.set_weights(w)
    xyz0 = (np.random.default_rng(3).normal(size=(11, 3)) * 1.5).astype(np.float32)
    e_dev, e_ref = eng.edges(xyz0), orc.get_init_edges(xyz0, num=h_dim)[0]
    assert e_dev.shape == (11, 11, h_dim) and np.abs(e_dev - e_ref).max() <= 1e-6
    # (4) the compact entry: QM9-like molecules, a 40-atom and a 150-atom system in one batch
    mols, offsets, xyz, xx, QQ = load_molecules(val_dir, [nm for nm in val_names][:20], nx)
    for nb, seed in ((40, 10), (150, 9)):
        _, bxyz, bx, bQ, _ = synth.box_system(n_atoms=nb, seed=seed)
        offsets = np.concatenate([offsets, [offsets[-1] + nb]]).astype(np.int32)
        xyz, xx, QQ = np.concatenate([xyz, bxyz]), np.concatenate([xx, bx]), np.concatenate([QQ, bQ]).astype(np.float32)
    N = 150
    got = eng.forward_xyz(offsets, xyz, xx, QQ, N)
    worst = 0.0
    for k in range(len(offsets) - 1):
        sl = slice(offsets[k], offsets[k + 1])
        r = orc.forward_xyz(xyz[sl], xx[sl], QQ[k], w, N=N, dtype=np.float64, h_dim=h_dim)
        worst = max(worst, float(np.abs(got[sl] - r[:offsets[k + 1] - offsets[k]]).max()))
    print(f"h_dim {h_dim}: compact entry worst |dq| {worst:.3e} over {len(offsets) - 1} systems (fused / tiled: {eng.last_stats()[1]} / {eng.last_stats()[2]})")
    assert worst <= TOL
    eng.close()
    # (5) GNN_layer / EPN_layer calls with h of h_dim channels
    hx, x1, qx, m4 = orc.model_reduce(h, x, q, mask)
    hx = (rng.normal(size=hx.shape) * 0.2 * (x1[..., :1] != 0)).astype(np.float32)
    gnn = charge_gn.GNN_layer(charge_gn.MLP_layer, charge_gn.MLP_layer(layers, out_dim=h_dim), T)
    for t in range(T):
        gnn.message_fns[t].set_weights(w["msg"][t])
    gnn.update_fn.set_weights(w["upd"])
    h_gpu = gnn.call(hx, e, x1, qx, m4)
    h_ref = orc.gnn_layer(hx, e, x1, qx, m4, w["msg"], w["upd"], dtype=np.float64)
    h_r32 = orc.gnn_layer(hx, e, x1, qx, m4, w["msg"], w["upd"], dtype=np.float32)
    assert h_gpu.shape == h_ref.shape == hx.shape
    assert np.abs(h_gpu - h_ref).max() <= max(TOL, 3 * np.abs(h_r32 - h_ref).max())
    epn = charge_gn.EPN_layer(charge_gn.MLP_layer, T=T)
    for t in range(T):
        epn.pass_fns[t].set_weights(w["pas"][t])
    q_gpu = epn.call(h_ref.astype(np.float32), e, x1, qx, m4)
    q_ref = orc.epn_layer(h_ref.astype(np.float32), e, x1, qx, m4, w["pas"], dtype=np.float64)
    assert np.abs(q_gpu - q_ref).max() <= TOL
    with pytest.raises(EpnnError, match="out_dim"):
        charge_gn.GNN_layer(charge_gn.MLP_layer, charge_gn.MLP_layer(layers, out_dim=48), T).call(hx, e, x1, qx, m4)
    # (6) the training step: gradients in the model's shapes vs the float64 oracle, then an optimizer step
    yb = (0.05 * rng.normal(size=(x.shape[0], x.shape[1])) * np.asarray(mask).reshape(x.shape[0], x.shape[1], x.shape[1]).max(axis=2)).astype(np.float32)   # (labels of real atoms)
    loss_ref, pred_ref, g_ref = ot.loss_and_grads(h, e, x, q, mask, yb, w)
    engt = Engine(nx=nx, T=T, h_dim=h_dim, e_dim=h_dim)
    engt.set_weights(w)
    engt.train_init()
    predt, losst = engt.train_step_dense(h, e, x, q, mask, yb, apply=False)
    assert np.abs(predt.reshape(pred_ref.shape) - pred_ref).max() < 2e-5 and abs(losst - loss_ref) <= 2e-5 * max(1.0, abs(loss_ref))
    g, gr = engt.get_gradients().astype(np.float64), ot.flatten(g_ref)
    assert g.shape == gr.shape == (engt.param_count(),)
    pos, worst = 0, 0.0
    for m in [w["upd"]] + w["msg"] + w["pas"]:
        for W_, b_ in m:
            for arr in (W_, b_):
                sl = slice(pos, pos + arr.size)
                scale = np.abs(gr[sl]).max()
                if scale > 0:
                    worst = max(worst, np.abs(g[sl] - gr[sl]).max() / scale)
                pos += arr.size
    print(f"h_dim {h_dim}: worst per-tensor relative gradient error {worst:.2e}")
    assert worst <= 2e-4
    # the compact training entry (its own featurisation with e_dim Gaussians): the same gradient for the same molecules
    cm, coff, cxyz, cx, cQ = load_molecules(os.path.join(golden_dir, "qm9_small"), [str(nm) for nm in names], nx)
    cy = np.concatenate([yb[k, :coff[k + 1] - coff[k]] for k in range(len(coff) - 1)])
    qc, lossc = engt.train_step_xyz(coff, cxyz, cx, cQ, cy, x.shape[1], apply=False)
    assert abs(lossc - loss_ref) <= 2e-5 * max(1.0, abs(loss_ref))
    gc = engt.get_gradients().astype(np.float64)
    assert np.abs(gc - gr).max() <= 2e-4 * np.abs(gr).max()
    engt.set_gradients(g.astype(np.float32))
    assert np.array_equal(engt.get_gradients(), g.astype(np.float32))
    engt.train_apply()
    w_after = engt.get_weights()
    assert w_after["upd"][-1][0].shape == w["upd"][-1][0].shape and not np.array_equal(w_after["upd"][0][0], w["upd"][0][0])
    engt.close()


@pytest.mark.parametrize("layers", [[16], [64, 32], [8, 24, 40], [24, 8], [48, 48], [64]])
def test_make_model_with_other_update_layers(golden_dir, val_dir, val_names, tmp_path, layers):
    """make_model(layers, ...) sizes the update MLP from `layers` (charge_gn.py:369-371; the message / pass MLPs are [32, 32] by
    the reference's own constants).  One or two hidden layers of at most 32 units run the tuned kernels of the [32, 32] model on a
    zero-padded copy of the update MLP (a missing second layer = the identity: exact, epnn_set_update_layers); of at most 64 units
    the 64-unit variant of the one-wavefront-per-molecule kernel for molecules of up to 32 atoms (the same embedding into [64, 64])
    and the tiled kernels with the generic update stage for larger ones; anything else the tiled kernels alone.  The literal dense call, the compact entry on molecules of 3..38 atoms and a
    150-atom box, and GNN_layer.call, each vs the float64 oracle; the checkpoint writer / reader round trip keeps the layer count;
    the training step's gradients vs the float64 oracle."""
    from epnn_amd import charge_gn, synth
    from epnn_amd._lib import EpnnError
    from epnn_amd.engine import Engine
    from oracle import epnn_oracle as orc
    from conftest import load_molecules
    nx, T = 9, 3
    w = random_weights(nx, T, seed=31, scale=0.35)
    w["upd"] = _upd_layers(layers, seed=len(layers))
    # (1) the literal make_model call
    x, h, q, e, Q, y, mask, names = _small_state(golden_dir, nx)
    model = charge_gn.make_model(layers, 48, T, nx, x.shape[1])
    model.set_weights_dict(w)
    pred = model([h, e, x, q, mask])
    ref = orc.model_forward(h, e, x, q, mask, w, dtype=np.float64)
    ref32 = orc.model_forward(h, e, x, q, mask, w, dtype=np.float32)
    err, noise = np.abs(pred - ref).max(), np.abs(ref32 - ref).max()
    print(f"layers {layers}: dense call |dq| {err:.3e} (float32 oracle noise {noise:.3e})")
    assert err <= max(TOL, 3 * noise)
    # (2) checkpoint round trip: len(layers) + 1 Dense layers under update_fn/layer_set
    model.save_weights(str(tmp_path / "m"))
    again = charge_gn.make_model(layers, 48, T, nx, x.shape[1])
    again.load_weights(str(tmp_path / "m"))
    w2 = again.weights_dict()
    assert len(w2["upd"]) == len(layers) + 1
    for (k0, b0), (k1, b1) in zip(w["upd"], w2["upd"]):
        assert np.array_equal(k0, k1) and np.array_equal(b0, b1)
    assert np.array_equal(again([h, e, x, q, mask]), pred)
    # (3) the compact entry: QM9-like molecules of every path's sizes + a 150-atom box in one batch
    mnames = [nm for nm in val_names][:30]
    mols, offsets, xyz, xx, QQ = load_molecules(val_dir, mnames, nx)
    for nb, seed in ((40, 10), (150, 9)):      # a 40-atom system (block-per-wavefront kernels) and a 150-atom one (tiled kernels)
        _, bxyz, bx, bQ, _ = synth.box_system(n_atoms=nb, seed=seed)
        offsets = np.concatenate([offsets, [offsets[-1] + nb]]).astype(np.int32)
        xyz, xx, QQ = np.concatenate([xyz, bxyz]), np.concatenate([xx, bx]), np.concatenate([QQ, bQ]).astype(np.float32)
    N = 150
    eng = Engine(nx=nx, T=T)
    eng.set_weights(w)
    got = eng.forward_xyz(offsets, xyz, xx, QQ, N)
    embeds = len(layers) <= 2 and max(layers) <= 32
    wide = len(layers) <= 2 and 32 < max(layers) <= 64
    n_le32 = int((np.diff(offsets) <= 32).sum())
    assert n_le32 == 30
    fused = 31 if embeds else (30 if wide else 0)                # the tuned kernels take such a model's small molecules, or none
    assert eng.last_stats()[1] == fused and eng.last_stats()[2] == 32 - fused
    worst = 0.0
    for k in range(len(offsets) - 1):
        sl = slice(offsets[k], offsets[k + 1])
        r = orc.forward_xyz(xyz[sl], xx[sl], QQ[k], w, N=N, dtype=np.float64)
        worst = max(worst, float(np.abs(got[sl] - r[:offsets[k + 1] - offsets[k]]).max()))
    print(f"layers {layers}: compact entry worst |dq| {worst:.3e} over {len(offsets) - 1} systems")
    assert worst <= TOL
    # the same handle back on the reference's layers: the tuned kernels again
    w32 = random_weights(nx, T, seed=31, scale=0.35)
    eng.set_weights(w32)
    got32 = eng.forward_xyz(offsets[:-2], xyz[:offsets[-3]], xx[:offsets[-3]], QQ[:-2], 41)
    eng_ref = Engine(nx=nx, T=T)
    eng_ref.set_weights(w32)
    assert np.array_equal(got32, eng_ref.forward_xyz(offsets[:-2], xyz[:offsets[-3]], xx[:offsets[-3]], QQ[:-2], 41))
    assert eng.last_stats()[1] > 0
    eng.close(); eng_ref.close()
    # (4) GNN_layer with such an update_fn
    rng = np.random.default_rng(2)
    hx, x1, qx, m4 = orc.model_reduce(h, x, q, mask)
    hx = (rng.normal(size=hx.shape) * 0.2 * (x1[..., :1] != 0)).astype(np.float32)
    gnn = charge_gn.GNN_layer(charge_gn.MLP_layer, charge_gn.MLP_layer(layers, out_dim=48), T)
    for t in range(T):
        gnn.message_fns[t].set_weights(w["msg"][t])
    gnn.update_fn.set_weights(w["upd"])
    h_gpu = gnn.call(hx, e, x1, qx, m4)
    h_ref = orc.gnn_layer(hx, e, x1, qx, m4, w["msg"], w["upd"], dtype=np.float64)
    h_r32 = orc.gnn_layer(hx, e, x1, qx, m4, w["msg"], w["upd"], dtype=np.float32)
    assert np.abs(h_gpu - h_ref).max() <= max(TOL, 3 * np.abs(h_r32 - h_ref).max())
    # (5) the training step: gradient of sum (y - p)^2 (charge_gn.py:397-398) per parameter tensor vs the float64 oracle, then an
    #     optimizer step through the reference-style API (the weights move, the layer count stays)
    from oracle import epnn_oracle_train as ot
    yb = (0.05 * rng.normal(size=(x.shape[0], x.shape[1]))).astype(np.float32)
    loss_ref, pred_ref, g_ref = ot.loss_and_grads(h, e, x, q, mask, yb, w)
    engt = Engine(nx=nx, T=T)
    engt.set_weights(w)
    engt.train_init()
    predt, losst = engt.train_step_dense(h, e, x, q, mask, yb, apply=False)
    assert np.abs(predt.reshape(pred_ref.shape) - pred_ref).max() < 2e-5 and abs(losst - loss_ref) <= 2e-5 * max(1.0, abs(loss_ref))
    g, gr = engt.get_gradients().astype(np.float64), ot.flatten(g_ref)
    assert g.shape == gr.shape == (engt.param_count(),)
    pos, worst = 0, 0.0
    for m in [w["upd"]] + w["msg"] + w["pas"]:
        for W_, b_ in m:
            for arr in (W_, b_):
                sl = slice(pos, pos + arr.size)
                scale = np.abs(gr[sl]).max()
                if scale > 0:
                    worst = max(worst, np.abs(g[sl] - gr[sl]).max() / scale)
                pos += arr.size
    print(f"layers {layers}: worst per-tensor relative gradient error {worst:.2e}")
    assert worst <= 2e-4
    engt.train_apply()
    w_after = engt.get_weights()
    assert len(w_after["upd"]) == len(layers) + 1 and not np.array_equal(w_after["upd"][0][0], w["upd"][0][0])
    engt.close()
