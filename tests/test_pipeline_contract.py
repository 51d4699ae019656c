"""Pipeline.map's scheduling, held to the contract of the C entry it drives, without a GPU: the lanes are stand-ins that keep
epnn_forward_xyz_begin's promises (the arrays are read while `begin` runs and never after, one forward per handle between begin
and end) and hand back exactly what they read.  What a loader may do with its arrays, which error reaches the caller, and the
state every lane is left in."""
import threading

import numpy as np
import pytest

from epnn_amd.engine import EpnnError, Pipeline

# How long a stand-in's `begin` waits for "the loader has been asked for the next batch" before it reads its arrays: the worst
# interleaving for a map that hands the caller's own arrays to another thread.  A map that does not ask for the next batch before
# `begin` has returned just sits the time out (no deadlock).  With everything on the calling thread nobody can re-enter the loader
# while `begin` runs, so there is nothing to wait for.
PATIENCE = 0.2
PATIENCE_INLINE = 0.005

FAIL_EPNN, FAIL_VALUE = -1.0, -2.0           # Q[0] of a batch whose `begin` raises EpnnError / ValueError


def _flatten(offsets, xyz, x, Q):
    """What a stand-in returns for a batch: everything it read, in one row."""
    return np.concatenate([np.asarray(offsets, dtype=np.float64).ravel(), np.asarray(xyz, dtype=np.float64).ravel(),
                           np.asarray(x, dtype=np.float64).ravel(), np.asarray(Q, dtype=np.float64).ravel()])


class Clock:
    """after[k] is set once the loader has been re-entered (or finalised) after it yielded batch k; batch k carries k in xyz[0, 0]."""

    def __init__(self, n):
        self.after = [threading.Event() for _ in range(n)]

    def release(self, upto=None):
        for ev in self.after[:upto]:
            ev.set()


class StandIn:
    """A lane that mimics the C contract of epnn_forward_xyz_begin / _end."""

    def __init__(self, clock, patience):
        self.clock, self.patience = clock, patience
        self.begun = False
        self.snap = None
        self.begin_failed = False            # the last `begin` on this lane raised: an `end` now is one too many
        self.ends_after_failed_begin = 0
        self.refused_begins = 0

    def forward_xyz_begin(self, offsets, xyz, x, Q, N):
        if self.begun:
            self.refused_begins += 1
            raise EpnnError("epnn_forward_xyz_begin: collect the previous forward with epnn_forward_xyz_end first")
        k = int(np.asarray(xyz)[0, 0])
        if 0 <= k < len(self.clock.after):
            self.clock.after[k].wait(self.patience)
        snap = [np.array(a, copy=True) for a in (offsets, xyz, x, Q)]      # as the C entry: read now, never again
        if snap[3][0] == FAIL_EPNN:
            self.begin_failed = True
            raise EpnnError(f"stand-in: batch {k} is refused")
        if snap[3][0] == FAIL_VALUE:
            self.begin_failed = True
            raise ValueError(f"stand-in: batch {k} does not convert")
        self.begin_failed = False
        self.snap = snap
        self.begun = True

    def forward_xyz_end(self):
        if self.begin_failed:
            self.ends_after_failed_begin += 1
        if not self.begun:
            raise EpnnError("forward_xyz_end: no forward was begun on this engine")
        self.begun = False
        return _flatten(*self.snap)


def _pipeline(depth, clock, workers):
    pipe = Pipeline.__new__(Pipeline)        # no handle, no library
    pipe.engines = [StandIn(clock, PATIENCE if workers > 0 else PATIENCE_INLINE) for _ in range(depth)]
    pipe._next = 0
    return pipe


def _data(k, rng, fail=None):
    """Batch k: 2..4 molecules of 1..5 atoms, nx = 3; xyz[0, 0] = k (Clock), Q[0] marks a batch whose `begin` fails."""
    B = int(rng.integers(2, 5))
    offsets = np.concatenate([[0], np.cumsum(rng.integers(1, 6, size=B))]).astype(np.int32)
    A = int(offsets[-1])
    xyz = rng.normal(size=(A, 3)).astype(np.float32)
    xyz[0, 0] = k
    x = rng.normal(size=(A, 3)).astype(np.float32)
    Q = rng.integers(0, 3, size=B).astype(np.float32)
    if fail is not None:
        Q[0] = fail
    return offsets, xyz, x, Q


def _recycling_loader(datas, clock, spoil):
    """One buffer set, refilled in place for every batch and handed out as views; overwritten once more after the last yield."""
    Bmax = max(len(d[3]) for d in datas)
    Amax = max(int(d[0][-1]) for d in datas)
    offsets, xyz, x, Q = (np.zeros(Bmax + 1, np.int32), np.zeros((Amax, 3), np.float32), np.zeros((Amax, 3), np.float32),
                          np.zeros(Bmax, np.float32))
    try:
        for k, d in enumerate(datas):
            B, A = len(d[3]), int(d[0][-1])
            offsets[:B + 1], xyz[:A], x[:A], Q[:B] = d
            yield offsets[:B + 1], xyz[:A], x[:A], Q[:B]
            clock.release(k + 1)             # re-entered: the arrays of batch k are the loader's again
    finally:
        for buf, a in zip((offsets, xyz, x, Q), spoil):
            buf[...] = a[tuple(slice(0, s) for s in buf.shape)]
        clock.release()


def _plain_loader(datas, clock, raise_at=None):
    """Distinct arrays per batch; raise_at: the loader itself fails when asked for that batch."""
    try:
        for k, d in enumerate(datas):
            if k == raise_at:
                raise RuntimeError("loader: no batch %d" % k)
            yield d
            clock.release(k + 1)
    finally:
        clock.release()


def _assert_idle(pipe):
    assert not any(e.begun for e in pipe.engines), "a lane is left begun"
    assert sum(e.ends_after_failed_begin for e in pipe.engines) == 0, "forward_xyz_end on a lane whose begin had failed"
    assert sum(e.refused_begins for e in pipe.engines) == 0, "a lane was given a second begin before its end"


def _assert_two_good_batches(pipe, workers, rng):
    datas = [_data(k, rng) for k in range(2)]
    clock = Clock(2)
    for e in pipe.engines:
        e.clock = clock
    got = list(pipe.map(_plain_loader(datas, clock), 8, workers=workers))
    assert len(got) == 2 and all(np.array_equal(g, _flatten(*d)) for g, d in zip(got, datas))
    _assert_idle(pipe)


@pytest.mark.parametrize("workers", [0, 1, 2, 3])
@pytest.mark.parametrize("depth", [1, 3, 8])
def test_recycled_buffers(depth, workers):
    """A loader that refills ONE offsets / xyz / x / Q buffer set in place for each of 7 batches, as the contract of
    forward_xyz_begin allows ("the arrays may be reused at once"), and overwrites it once more after the last one: every batch's
    result is that of its own data.  Fails for workers >= 1 with the map that submitted the caller's own arrays to the worker
    thread and went straight back to the loader: 1 batch of 7 came back right (all 7 at workers = 0)."""
    rng = np.random.default_rng(100 * depth + workers)
    datas = [_data(k, rng) for k in range(7)]
    spoil = (np.full(16, 3, np.int32), np.full((64, 3), 7.5, np.float32), np.full((64, 3), -7.5, np.float32), np.full(16, 9, np.float32))
    clock = Clock(7)
    pipe = _pipeline(depth, clock, workers)
    got = list(pipe.map(_recycling_loader(datas, clock, spoil), 8, workers=workers))
    assert len(got) == 7
    right = [g.shape == _flatten(*d).shape and np.array_equal(g, _flatten(*d)) for g, d in zip(got, datas)]
    assert all(right), f"batches that came back right: {sum(right)} of 7"
    _assert_idle(pipe)


_FAILURES = {
    "begin_epnn_error": ([None, None, FAIL_EPNN, None, None, None], None, EpnnError, "batch 2 is refused"),
    "begin_value_error": ([None, None, FAIL_VALUE, None, None, None], None, ValueError, "batch 2 does not convert"),
    "two_in_flight_epnn_first": ([None, None, FAIL_EPNN, FAIL_VALUE, None, None], None, EpnnError, "batch 2 is refused"),
    "two_in_flight_value_first": ([None, FAIL_VALUE, FAIL_EPNN, None, None, None], None, ValueError, "batch 1 does not convert"),
    "loader_raises": ([None, None, None, None, None, None], 3, RuntimeError, "loader: no batch 3"),
    "begin_fails_then_loader_raises": ([None, None, FAIL_VALUE, None, None, None], 3, ValueError, "batch 2 does not convert"),
}


@pytest.mark.parametrize("depth,workers", [(3, 0), (3, 1), (3, 2), (3, 3), (1, 1), (8, 2)])
@pytest.mark.parametrize("case", sorted(_FAILURES))
def test_failures(case, depth, workers):
    """One batch whose begin raises EpnnError, one whose begin raises ValueError, two failing batches next to each other (in
    flight together wherever the depth allows) with different exception types, the loader itself raising mid-stream: the caller
    gets the first error in call order, as raised; no lane is left begun; forward_xyz_end is never called on a lane whose begin
    failed; and a following map over two good batches returns them right.  The two-failure cases fail with cleanup that catches
    EpnnError only: there the second lane's ValueError replaced the first error and the lanes behind it stayed begun."""
    marks, raise_at, exc, text = _FAILURES[case]
    rng = np.random.default_rng(7 * depth + workers)
    datas = [_data(k, rng, fail=m) for k, m in enumerate(marks)]
    clock = Clock(len(datas))
    pipe = _pipeline(depth, clock, workers)
    got = []
    with pytest.raises(exc, match=text) as info:
        for q in pipe.map(_plain_loader(datas, clock, raise_at), 8, workers=workers):
            got.append(q)
    assert type(info.value) is exc
    assert all(np.array_equal(g, _flatten(*d)) for g, d in zip(got, datas))      # what was yielded before the error is right
    first_bad = min([k for k, m in enumerate(marks) if m is not None] + ([raise_at] if raise_at is not None else []))
    assert len(got) <= first_bad
    _assert_idle(pipe)
    _assert_two_good_batches(pipe, workers, rng)


@pytest.mark.parametrize("workers", [0, 1, 2])
def test_early_stop(workers):
    """The caller takes the first result and closes the iterator, with recycled buffers and batches in flight: the result is
    that of batch 0, no lane is left begun, and the pipeline serves the next map."""
    rng = np.random.default_rng(40 + workers)
    datas = [_data(k, rng) for k in range(7)]
    spoil = (np.full(16, 3, np.int32), np.full((64, 3), 7.5, np.float32), np.full((64, 3), -7.5, np.float32), np.full(16, 9, np.float32))
    clock = Clock(7)
    pipe = _pipeline(3, clock, workers)
    loader = _recycling_loader(datas, clock, spoil)
    it = pipe.map(loader, 8, workers=workers)
    first = next(it)
    it.close()
    loader.close()
    assert np.array_equal(first, _flatten(*datas[0]))
    _assert_idle(pipe)
    _assert_two_good_batches(pipe, workers, rng)
