"""Placement of the handles' streams in the runtime's priority classes (include/epnn.h at epnn_create) on the GPU: which class
every lane of a pipeline gets, that places are given back, the switch, a process with plentiful queues, and that results do
not depend on the class.  The HIP runtime reads GPU_MAX_HW_QUEUES when it starts, so every case runs in a fresh child process
whose environment is given explicitly."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

_CHILD = r"""
import ctypes as C, json, os, sys
sys.path.insert(0, sys.argv[1])
mode = sys.argv[2]
import numpy as np
from epnn_amd import _lib, checkpoint, synth
from epnn_amd.engine import Engine, Pipeline

lib = _lib.load()
out = {"queues": os.environ.get("GPU_MAX_HW_QUEUES")}
pipe = Pipeline(depth=8, nx=9, T=5)
least, greatest = C.c_int(), C.c_int()
rc = lib.hipDeviceGetStreamPriorityRange(C.byref(least), C.byref(greatest))        # (the HIP runtime the library is linked to)
assert rc == 0, rc
out["range"] = [least.value, greatest.value]
out["lanes"] = [list(e.stream_class()) for e in pipe.engines]
if mode == "limit4":
    # results do not depend on the class: one batch through every lane, and through a lone engine of the switched-off placement
    offsets, xyz, x, Q, N = synth.qm9_like_batch(B=16, seed=3, N=29)
    out["sizes"] = np.diff(offsets).tolist()
    w = checkpoint.load_epnn_weights(os.path.join(sys.argv[1], "models", "decay_model_weights"))
    pipe.set_weights(w)
    qs, pairs = [], []
    for e in pipe.engines:
        qs.append(e.forward_xyz(offsets, xyz, x, Q, N))
        pairs.append(int(e.last_stats()[0]))
    os.environ["EPNN_STREAM_CLASSES"] = "0"
    lone = Engine(nx=9, T=5)
    del os.environ["EPNN_STREAM_CLASSES"]
    out["lone_class"] = lone.stream_class()[0]
    lone.set_weights(w)
    lone.set_option("wave2", 0)                 # the kernel the pipeline's lanes run (Pipeline sets it; a lone engine's default splits molecules)
    q0 = lone.forward_xyz(offsets, xyz, x, Q, N)
    pairs.append(int(lone.last_stats()[0]))
    lone.close()
    out["finite"] = bool(np.isfinite(q0).all() and np.abs(q0).max() > 0)
    out["same_bits"] = [bool(q.tobytes() == q0.tobytes()) for q in qs]
    out["pairs"] = pairs
    # places are given back: lanes 1 (normal) and 5 (high) go, the next two handles take exactly those places
    pipe.engines[1].close()
    pipe.engines[5].close()
    a, b = Engine(nx=9, T=5), Engine(nx=9, T=5)
    out["refill"] = [a.stream_class()[0], b.stream_class()[0]]
    a.close()
    b.close()
    pipe.close()
    p2 = Pipeline(depth=2, nx=9, T=5)
    out["after_close"] = [e.stream_class()[0] for e in p2.engines]
    p2.close()
else:
    pipe.close()
print("RESULT " + json.dumps(out))
"""


def _child(tmp_path_factory, mode, queues, classes=None):
    script = tmp_path_factory.mktemp("stream_classes") / "child.py"
    script.write_text(_CHILD)
    env = {k: v for k, v in os.environ.items() if k != "EPNN_STREAM_CLASSES"}
    env["GPU_MAX_HW_QUEUES"] = str(queues)
    if classes is not None:
        env["EPNN_STREAM_CLASSES"] = str(classes)
    run = subprocess.run([sys.executable, str(script), ROOT, mode], env=env, capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    rows = [l for l in run.stdout.splitlines() if l.startswith("RESULT ")]
    assert len(rows) == 1, run.stdout[-2000:]
    return json.loads(rows[0][len("RESULT "):])


@pytest.fixture(scope="module")
def limit4(tmp_path_factory):
    return _child(tmp_path_factory, "limit4", 4)


def _levels(res):
    least, greatest = res["range"]
    return {0: 0, 1: greatest, 2: least}, (greatest != 0) + (least != 0 and least != greatest)


def test_eight_lanes_are_three_normal_four_high_one_low(limit4):
    assert limit4["queues"] == "4"
    prio, extra = _levels(limit4)
    if extra == 0:
        pytest.skip(f"the device reports a single stream priority level {limit4['range']}: every stream stays normal")
    assert [c for c, _ in limit4["lanes"]] == [0, 0, 0, 1, 1, 1, 1, 2]
    for c, p in limit4["lanes"]:
        assert p == prio[c], (limit4["lanes"], limit4["range"])


def test_places_are_given_back(limit4):
    _, extra = _levels(limit4)
    if extra == 0:
        pytest.skip(f"the device reports a single stream priority level {limit4['range']}: every stream stays normal")
    assert limit4["refill"] == [0, 1]
    assert limit4["after_close"] == [0, 0]


def test_switch_off_keeps_every_stream_normal(tmp_path_factory):
    res = _child(tmp_path_factory, "classes", 4, classes=0)
    assert res["lanes"] == [[0, 0]] * 8


def test_plentiful_queues_keep_every_stream_normal(tmp_path_factory):
    res = _child(tmp_path_factory, "classes", 16)
    assert res["queues"] == "16"
    assert res["lanes"] == [[0, 0]] * 8


def test_results_do_not_depend_on_the_class(limit4):
    sizes = limit4["sizes"]
    assert min(sizes) < 16 < max(sizes), sizes            # synth.qm9_like_batch(B=16, seed=3): 14..29 atoms
    assert limit4["lone_class"] == 0
    assert limit4["finite"]
    assert limit4["same_bits"] == [True] * 8
    assert len(set(limit4["pairs"])) == 1 and limit4["pairs"][0] > 0, limit4["pairs"]
