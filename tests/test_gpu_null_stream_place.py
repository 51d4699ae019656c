"""The null stream's place on the GPU (include/epnn.h, "THE NULL STREAM'S PLACE"): under GPU_MAX_HW_QUEUES=4 eight handles are
four normal + four high by default and 3 + 4 + 1 with EPNN_NULL_STREAM_PLACE=1, and the charges do not depend on it by a bit.  The
HIP runtime reads GPU_MAX_HW_QUEUES when it starts, so every case is a fresh child process with its environment given explicitly."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

SIZES = [3, 7, 12, 16, 17, 19, 24, 29]

_CHILD = r"""
import ctypes as C, json, os, sys
sys.path.insert(0, sys.argv[1])
mode = sys.argv[2]
import numpy as np
from epnn_amd import _lib, checkpoint, synth
from epnn_amd.engine import Engine

lib = _lib.load()
out = {"queues": os.environ.get("GPU_MAX_HW_QUEUES"), "place": os.environ.get("EPNN_NULL_STREAM_PLACE")}
engines = [Engine(nx=9, T=5, device=0) for _ in range(8)]
least, greatest = C.c_int(), C.c_int()
rc = lib.hipDeviceGetStreamPriorityRange(C.byref(least), C.byref(greatest))        # (the HIP runtime the library is linked to)
assert rc == 0, rc
out["range"] = [least.value, greatest.value]
out["lanes"] = [list(e.stream_class()) for e in engines]
if mode == "charges":
    sizes = json.loads(sys.argv[3])
    rng = np.random.default_rng(13)
    offsets = np.zeros(len(sizes) + 1, dtype=np.int32)
    offsets[1:] = np.cumsum(sizes)
    xyz = np.concatenate([synth._grow_molecule(rng, n) for n in sizes]).astype(np.float32)
    names = [e for e, _ in synth.QM9_ELEMS]
    ep = np.array([p for _, p in synth.QM9_ELEMS])
    x = synth.features(rng.choice(names, size=int(offsets[-1]), p=ep / ep.sum()))
    Q = np.zeros(len(sizes), dtype=np.float32)
    w = checkpoint.load_epnn_weights(os.path.join(sys.argv[1], "models", "decay_model_weights"))
    qs = []
    for e in engines:
        e.set_weights(w)
        qs.append(np.ascontiguousarray(e.forward_xyz(offsets, xyz, x, Q, 29), dtype=np.float32))
    out["atoms"] = int(qs[0].size)
    out["finite"] = bool(np.isfinite(qs[0]).all() and np.abs(qs[0]).max() > 0)
    out["same_bits"] = [bool(q.tobytes() == qs[0].tobytes()) for q in qs]
    out["charges"] = qs[0].tobytes().hex()
for e in engines:
    e.close()
print("RESULT " + json.dumps(out))
"""


def _child(tmp_path_factory, mode, place):
    script = tmp_path_factory.mktemp("null_stream_place") / "child.py"
    script.write_text(_CHILD)
    env = {k: v for k, v in os.environ.items() if k not in ("EPNN_STREAM_CLASSES", "EPNN_NULL_STREAM_PLACE")}
    env["GPU_MAX_HW_QUEUES"] = "4"
    if place is not None:
        env["EPNN_NULL_STREAM_PLACE"] = str(place)
    run = subprocess.run([sys.executable, str(script), ROOT, mode, json.dumps(SIZES)], env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    rows = [l for l in run.stdout.splitlines() if l.startswith("RESULT ")]
    assert len(rows) == 1, run.stdout[-2000:]
    return json.loads(rows[0][len("RESULT "):])


@pytest.fixture(scope="module")
def first(tmp_path_factory):            # no place: the default
    return _child(tmp_path_factory, "charges", None)


@pytest.fixture(scope="module")
def third(tmp_path_factory):            # the same call with the place kept
    return _child(tmp_path_factory, "charges", 1)


def _three_classes(res):
    least, greatest = res["range"]
    assert greatest < 0 < least, res["range"]            # gfx950 under this runtime: the three classes the placement is about
    return {0: 0, 1: greatest, 2: least}


def test_eight_handles_are_four_normal_four_high(first):
    assert first["queues"] == "4" and first["place"] is None
    prio = _three_classes(first)
    assert [c for c, _ in first["lanes"]] == [0, 0, 0, 0, 1, 1, 1, 1]
    for c, p in first["lanes"]:
        assert p == prio[c], (first["lanes"], first["range"])


def test_place_kept_gives_three_four_one(tmp_path_factory):
    second = _child(tmp_path_factory, "classes", 1)
    assert second["queues"] == "4" and second["place"] == "1"
    prio = _three_classes(second)
    assert [c for c, _ in second["lanes"]] == [0, 0, 0, 1, 1, 1, 1, 2]
    for c, p in second["lanes"]:
        assert p == prio[c], (second["lanes"], second["range"])


def test_charges_are_the_same_bits_on_every_handle(first):
    assert first["atoms"] == sum(SIZES)
    assert first["finite"]
    assert first["same_bits"] == [True] * 8


def test_charges_are_the_same_bits_with_the_place_kept(first, third):
    assert third["place"] == "1"
    _three_classes(third)
    assert [c for c, _ in third["lanes"]] == [0, 0, 0, 1, 1, 1, 1, 2]
    assert third["finite"] and third["same_bits"] == [True] * 8
    assert len(first["charges"]) == 8 * sum(SIZES)
    assert third["charges"] == first["charges"]
