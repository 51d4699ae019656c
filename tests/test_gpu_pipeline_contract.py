"""Pipeline.map and epnn_forward_xyz_begin / _end on the device, driven the way a data loader drives them: one buffer set refilled
in place for every batch, batches that fail, and other entries on a handle between the two halves.  Every result is held, bit for
bit, to the blocking forward_xyz of the same batch on a fresh lone handle with the pipeline's options; that blocking result is held
once per batch to the float64 oracle (tests/test_pipeline_contract.py holds the same contract on stand-in lanes without a GPU)."""
import os
import threading
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import random_weights

pytestmark = pytest.mark.gpu

TOL = 1e-5                                   # the bound of test_bench_batch_vs_oracle
WAIT = 0.2                                   # a begin waits at most this long for the loader to be asked for the next batch
# (molecules, seed) of synth.qm9_like_batch per batch: the one-wavefront sizes 12..29 atoms mixed (lanes run "wave2" = 0).  The seeds are
# the first from 40 on at which the float32 oracle itself stays within TOL / 4 of the float64 one with the shipped weights at N = 70
# (the K = 4 of test_gpu_f32_grade.py; with random_weights it is 1e-7 everywhere).  Every second batch of these sizes holds a molecule
# on which it does not -- 4.2e-5 on molecule 24 of (33, 43), 1.9e-5 in (29, 54) --, and no float32 forward holds 1e-5 there.
BATCHES = [(24, 40), (40, 41), (27, 43), (33, 49), (25, 50), (36, 52), (29, 56)]
MIXED_AT = 3                                 # place of the batch with the 70-atom chain in the stream of 8
NBIG = 70
# A pair list starts with room for max(1024, 16 per atom) pairs and the stream's batch with the 70-atom chain has 698 (chain 428, its
# three small molecules 270): it takes the tiled path, but no regrow.  The regrow deferred into forward_xyz_end is reached with a
# 140-atom chain built the same way (1628 + 270 pairs) on handles whose "pair_cap_per_atom" is 1, i.e. room for 1024 pairs.
NLONG = 140
LONG_AT = 1                                  # its place in the short stream (tiny batch, long batch, tiny batch)
LONG_OPTIONS = {"pair_cap_per_atom": 1}


def _lone(w, **options):
    """A fresh handle with a pipeline lane's options."""
    from epnn_amd.engine import Engine
    eng = Engine(nx=9, T=5)
    eng.set_weights(w)
    for name, value in dict({"wave2": 0}, **options).items():
        eng.set_option(name, value)
    return eng


def _mixed_batch(nbig=NBIG):
    """Three small molecules and a random-walk chain of nbig atoms, as test_pipeline_map_equals_one_call_at_a_time builds it (tiled path)."""
    from epnn_amd import synth
    big = synth.qm9_like_batch(B=3, seed=99)
    rng = np.random.default_rng(5)
    xyz_big = np.cumsum(rng.normal(size=(nbig, 3)) * 0.8, axis=0).astype(np.float32)
    x_big = np.tile(big[2][:1], (nbig, 1))
    off = np.concatenate([big[0], [big[0][-1] + nbig]]).astype(np.int32)
    return (off, np.concatenate([big[1], xyz_big]), np.concatenate([big[2], x_big]), np.concatenate([big[3], [0.0]]).astype(np.float32))


_CASES = {}


def _case(which, weights_decay):
    """The stream of 8 batches (N = 70) and the short one with the regrow (N = 140) and, computed once, the blocking reference of
    each batch on a fresh lone handle."""
    if which not in _CASES:
        from epnn_amd import synth
        w = weights_decay if which == "decay_model_weights" else random_weights(9, 5, 31, scale=0.35)
        batches = [synth.qm9_like_batch(B=B, seed=seed)[:4] for B, seed in BATCHES]
        stream = batches[:MIXED_AT] + [_mixed_batch()] + batches[MIXED_AT:]
        lstream = [synth.qm9_like_batch(B=4, seed=61)[:4], _mixed_batch(NLONG), synth.qm9_like_batch(B=5, seed=62)[:4]]

        def blocking(batches, N, **options):
            ref, stats = [], []
            for b in batches:
                eng = _lone(w, **options)
                ref.append(eng.forward_xyz(*b, N))
                stats.append(eng.last_stats())
                eng.close()
                ref[-1].setflags(write=False)
            return ref, stats

        ref, stats = blocking(stream, NBIG)
        assert [int(s[2]) for s in stats] == [int(k == MIXED_AT) for k in range(8)], stats       # tiled molecules per batch
        lref, lstats = blocking(lstream, NLONG, **LONG_OPTIONS)
        assert [int(s[3]) > 0 for s in lstats] == [k == LONG_AT for k in range(3)], lstats        # regrows per batch
        # a pipeline of one lane leaves "wave2" at its default, the split over two wavefronts: other bits with a GNN that is not collapsed
        ref1, lref1 = blocking(stream, NBIG, wave2=-1)[0], blocking(lstream, NLONG, wave2=-1, **LONG_OPTIONS)[0]
        _CASES[which] = SimpleNamespace(which=which, w=w, stream=stream, ref=ref, N=NBIG, lstream=lstream, lref=lref, lN=NLONG,
                                        ref1=ref1, lref1=lref1)
    return _CASES[which]


@pytest.fixture(scope="module", params=["decay_model_weights", "random"])
def case(request, weights_decay):
    return _case(request.param, weights_decay)


def test_blocking_reference_vs_oracle(case):
    """What every other test of this file compares with, against the float64 oracle: all molecules of all batches of both streams
    at 1e-5, so that a wrong pipeline cannot agree with a reference that is wrong the same way."""
    from oracle import epnn_oracle as orc
    batches = [(b, r, case.N) for b, r in zip(case.stream + case.stream, case.ref + case.ref1)]
    batches += [(b, r, case.lN) for b, r in zip(case.lstream + case.lstream, case.lref + case.lref1)]
    mols = []
    for (off, xyz, x, Q), N in [(b, case.N) for b in case.stream] + [(b, case.lN) for b in case.lstream]:
        mols += [(xyz[off[b]:off[b + 1]], x[off[b]:off[b + 1]], Q[b], N) for b in range(len(Q))]
    with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
        refs = iter(list(pool.map(lambda m: orc.forward_xyz(m[0], m[1], m[2], case.w, N=m[3], dtype=np.float64), mols)))
    oracle = [np.concatenate([next(refs)[:off[b + 1] - off[b]] for b in range(len(Q))]) for off, _, _, Q in case.stream + case.lstream]
    oracle = oracle[:8] + oracle[:8] + oracle[8:] + oracle[8:]
    worst = [float(np.abs(r - o).max()) for (_, r, _), o in zip(batches, oracle)]
    print(f"{case.which}: worst |dq| per batch vs the float64 oracle " + " ".join(f"{v:.2e}" for v in worst))
    assert max(worst) <= TOL, worst


class _Recycler:
    """A loader that owns ONE offsets / xyz / x / Q buffer set, sized for the largest batch: refilled in place for every batch, handed
    out as views, and refilled with `after` (data, never NaN) behind the last batch.  `entered` is set while the loader has been asked
    for the batch after the one it last handed out."""

    def __init__(self, stream, after):
        self.stream, self.after = stream, after
        Bmax = max(len(b[3]) for b in stream + [after])
        Amax = max(int(b[0][-1]) for b in stream + [after])
        nx = stream[0][2].shape[1]
        self.bufs = (np.zeros(Bmax + 1, np.int32), np.zeros((Amax, 3), np.float32), np.zeros((Amax, nx), np.float32), np.zeros(Bmax, np.float32))
        self.entered = threading.Event()

    def _fill(self, b):
        B, A = len(b[3]), int(b[0][-1])
        views = (self.bufs[0][:B + 1], self.bufs[1][:A], self.bufs[2][:A], self.bufs[3][:B])
        for v, a in zip(views, b):
            v[...] = a
        return views

    def __iter__(self):
        try:
            for b in self.stream:
                views = self._fill(b)
                self.entered.clear()
                yield views
                self.entered.set()
        finally:
            self._fill(self.after)
            self.entered.set()


@pytest.fixture
def late_begin(monkeypatch):
    """Every forward_xyz_begin first waits, at most WAIT, for the loader to be asked for the next batch: the worst interleaving for
    a map that lets another thread read the loader's arrays."""
    from epnn_amd.engine import Engine
    real = Engine.forward_xyz_begin
    box = SimpleNamespace(event=None)

    def shim(self, *args):
        if box.event is not None:
            box.event.wait(WAIT)
        return real(self, *args)

    monkeypatch.setattr(Engine, "forward_xyz_begin", shim)
    return box


@pytest.mark.parametrize("depth,workers", [(3, 0), (3, 1), (3, 2), (1, 1)])
def test_recycled_buffers(case, late_begin, depth, workers):
    """The 8 batches from one recycled buffer set: every batch's charges are the bits of its own blocking forward.  Then, on fresh
    lanes, the short stream whose middle batch overflows its lane's pair list: the same, and that lane grew the list (inside
    forward_xyz_end, from the staged copy of arrays the loader has long refilled)."""
    from epnn_amd.engine import Pipeline
    ref, lref = (case.ref, case.lref) if depth > 1 else (case.ref1, case.lref1)
    for stream, ref, N, options, regrow_at in ((case.stream, ref, case.N, {}, None), (case.lstream, lref, case.lN, LONG_OPTIONS, LONG_AT)):
        loader = _Recycler(stream, after=stream[0])
        late_begin.event = loader.entered
        pipe = Pipeline(depth=depth, nx=9, T=5)
        try:
            pipe.set_weights(case.w)
            for name, value in options.items():
                pipe.set_option(name, value)
            got = list(pipe.map(iter(loader), N, workers=workers))
            regrown = [int(e.last_stats()[3]) for e in pipe.engines]
        finally:
            pipe.close()
        assert len(got) == len(ref)
        right = [a.shape == b.shape and np.array_equal(a, b) for a, b in zip(got, ref)]
        assert all(right), f"batches that came back right: {right}"
        assert regrow_at is None or regrown[regrow_at % depth] >= 1, regrown


def test_predict_xyz_stream_recycling_loader(case, late_begin):
    """The shape of infer.py: EPNNModel.predict_xyz_stream over single molecules that a loader hands out from one recycled buffer
    set, against the blocking engine."""
    from epnn_amd import charge_gn
    off, xyz, x, Q = case.stream[1]
    mols = [(np.array([0, off[b + 1] - off[b]], np.int32), xyz[off[b]:off[b + 1]], x[off[b]:off[b + 1]], Q[b:b + 1]) for b in range(12)]
    eng = _lone(case.w)
    ref = [eng.forward_xyz(*m, 29) for m in mols]
    eng.close()
    model = charge_gn.make_model([32, 32], 48, 5, 9, 29)
    model.set_weights_dict(case.w)
    loader = _Recycler(mols, after=mols[0])
    late_begin.event = loader.entered
    got = list(model.predict_xyz_stream(iter(loader), depth=3))
    assert len(got) == len(ref) and all(np.array_equal(a, b) for a, b in zip(got, ref))


@pytest.mark.parametrize("workers", [0, 1, 2])
def test_failures(case, workers):
    """A batch whose x has nx + 1 columns (EpnnError from the shape check), one whose xyz is an object array that does not
    convert (NumPy's error), and the two next to each other in both orders: the first error in call order reaches the caller, every
    lane then answers a following map with the bits of the blocking reference, and no lane is left with a forward begun."""
    from epnn_amd.engine import EpnnError, Pipeline
    g = case.stream
    off, xyz, x, Q = g[4]
    bad_x = (off, xyz, np.concatenate([x, x[:, :1]], axis=1), Q)
    bad_obj = (off, np.full(xyz.shape, "1.0 A", dtype=object), x, Q)
    numpy_error = (TypeError, ValueError)
    runs = [([g[0], bad_x, g[1], g[2]], EpnnError, 1), ([g[0], bad_obj, g[1]], numpy_error, 1),
            ([g[0], g[1], bad_x, bad_obj, g[2]], EpnnError, 2), ([g[0], g[1], bad_obj, bad_x, g[2]], numpy_error, 2)]
    pipe = Pipeline(depth=3, nx=9, T=5)
    try:
        pipe.set_weights(case.w)
        for batches, exc, first_bad in runs:
            got = []
            with pytest.raises(exc) as info:
                for q in pipe.map(iter(batches), case.N, workers=workers):
                    got.append(q)
            assert isinstance(info.value, EpnnError) == (exc is EpnnError), repr(info.value)
            assert len(got) <= first_bad and all(np.array_equal(q, case.ref[k]) for k, q in enumerate(got))
            again = list(pipe.map(iter(g[2:5]), case.N, workers=workers))          # one batch per lane, the 70-atom one among them
            assert len(again) == 3 and all(np.array_equal(q, r) for q, r in zip(again, case.ref[2:5]))
            for e in pipe.engines:
                with pytest.raises(EpnnError, match="no forward was begun"):
                    e.forward_xyz_end()
    finally:
        pipe.close()


# ---------------------------------------------------------------------------- other entries between begin and end on one handle
def _entry_context(weights_decay):
    from epnn_amd import synth
    from oracle import epnn_oracle as orc
    c = _case("random", weights_decay)
    tiny = synth.qm9_like_batch(B=4, seed=21)
    A = int(tiny[0][-1])
    rng = np.random.default_rng(77)
    n0 = int(tiny[0][1])
    dense = tuple(a[None] for a in orc.dense_inputs(tiny[1][:n0], tiny[2][:n0], tiny[3][0], n0))
    return SimpleNamespace(case=c, other=c.stream[1], tiny=tiny[:4], N=tiny[4], g=rng.normal(size=A).astype(np.float32),
                           begun={"small": (c.stream[0], c.ref[0], c.N, {}), "regrow_owed": (c.lstream[LONG_AT], c.lref[LONG_AT], c.lN, LONG_OPTIONS)},
                           v=rng.normal(size=(A, 3)).astype(np.float32), y=(0.1 * rng.normal(size=A)).astype(np.float32),
                           dense=dense, other_w=weights_decay)


def _forward_dev(e, c):
    off, xyz, x, Q = c.other
    A = int(off[-1])
    d = [e.to_device(a) for a in (xyz, x, Q)] + [e.alloc(A * 4)]
    e.forward_xyz_dev(off, d[0], d[1], d[2], d[3], c.case.N)
    q = d[3].download((A,))
    for a in d:
        a.free()
    return [q]


def _vjp(path):
    def run(e, c):
        e.set_option("grad_path", path)
        return list(e.charges_vjp_xyz(*c.tiny, c.g, c.N))
    return run


def _train(e, c):
    e.train_init()
    q, loss = e.train_step_xyz(*c.tiny, c.y, c.N, apply=False)
    return [q, np.float32(loss)]


def _next_forward(e, c):
    return [e.forward_xyz(*c.tiny, c.N)]


# name -> (the entry called between the halves, what is asked of the handle after forward_xyz_end; both -> the outputs compared)
_SERVED = {
    "forward_xyz_dev": (_forward_dev, None),
    "model_forward_dense": (lambda e, c: [e.model_forward_dense(*c.dense)], None),
    "charges_vjp_xyz_grad_path_1": (_vjp(1), None),
    "charges_vjp_xyz_grad_path_2": (_vjp(2), None),
    "charges_jvp_xyz": (lambda e, c: list(e.charges_jvp_xyz(*c.tiny, c.N, v=c.v)), None),
    "coulomb_xyz": (lambda e, c: list(e.coulomb_xyz(*c.tiny, c.N)), None),
    "train_step_xyz": (_train, None),
    "set_weights": (lambda e, c: e.set_weights(c.other_w) or [], _next_forward),
    "set_option_wave2": (lambda e, c: e.set_option("wave2", 17) or [], _next_forward),
    "sync": (lambda e, c: e.sync() or [], None),
}
_FRESH = {}


def _fresh_outputs(name, c):
    """The same call(s) on a fresh handle that has nothing begun."""
    if name not in _FRESH:
        run, after = _SERVED[name]
        e = _lone(c.case.w)
        _FRESH[name] = run(e, c) + (after(e, c) if after else [])
        e.close()
    return _FRESH[name]


@pytest.mark.parametrize("begun", ["small", "regrow_owed"])
@pytest.mark.parametrize("name", sorted(_SERVED))
def test_entry_served_between_begin_and_end(weights_decay, name, begun):
    """Entries that include/epnn.h says are served on a handle with a forward begun: their outputs are the bits of the same call on
    a fresh handle, and forward_xyz_end returns the bits of the begun batch under the weights and options of its begin -- once with
    a plain small batch begun, once with the 140-atom batch on a fresh handle, whose pair-list regrow is still owed then (its redo
    reads the staged inputs, packs weights and builds a plan).  New weights and options count from the next forward on."""
    from epnn_amd.engine import EpnnError
    c = _entry_context(weights_decay)
    want = _fresh_outputs(name, c)
    batch, ref, N, options = c.begun[begun]
    run, after = _SERVED[name]
    e = _lone(c.case.w, **options)
    try:
        e.forward_xyz_begin(*batch, N)
        assert int(e.last_stats()[3]) == 0                     # (the regrow runs in whoever waits for the forward next)
        got = run(e, c)
        q = e.forward_xyz_end()
        regrown = int(e.last_stats()[3])
        if after:
            got += after(e, c)
        with pytest.raises(EpnnError, match="no forward was begun"):
            e.forward_xyz_end()
    finally:
        e.close()
    assert np.array_equal(q, ref), float(np.abs(q - ref).max())
    # (the pair-list calls report their own counters through last_stats)
    assert regrown >= 1 or begun == "small" or name in ("charges_vjp_xyz_grad_path_2", "charges_jvp_xyz", "coulomb_xyz")
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(np.asarray(a), np.asarray(b)), (name, i, float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max()))


@pytest.mark.parametrize("begun", ["small", "regrow_owed"])
def test_entry_refused_between_begin_and_end(weights_decay, begun):
    """A second begin, the blocking forward_xyz and the box / cell host forwards are refused by name on a handle with a forward
    begun, and forward_xyz_end still returns the begun batch's bits."""
    from epnn_amd.engine import EpnnError
    c = _entry_context(weights_decay)
    batch, ref, N, options = c.begun[begun]
    e = _lone(c.case.w, **options)
    try:
        e.forward_xyz_begin(*batch, N)
        for what, kw in (("epnn_forward_xyz_begin", {}), ("epnn_forward_xyz_pbc", {"box": [30.0, 30.0, 30.0]}),
                         ("epnn_forward_xyz_cell", {"cell": 30.0 * np.eye(3)})):
            with pytest.raises(EpnnError, match=what):
                e.forward_xyz(*c.tiny, c.N, **kw)
        with pytest.raises(EpnnError, match="epnn_forward_xyz_begin"):
            e.forward_xyz_begin(*c.tiny, c.N)
        q = e.forward_xyz_end()
    finally:
        e.close()
    assert np.array_equal(q, ref)
