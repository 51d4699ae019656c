"""epnn_coulomb_xyz through the layers that need no GPU: declared in include/epnn.h, bound in epnn_amd/_lib.py with as many
arguments as the header declares, reachable as Engine.coulomb_xyz and EPNNModel.coulomb_xyz, and its two sources part of the
translation unit."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "epnn_coulomb_xyz"
ARGS = ["offsets", "xyz", "x", "Q", "N", "ke", "alpha", "parts"]
# the handle, B, N, offsets, xyz, x, Q, ke, alpha, and the six outputs q, phi, e, f, ffix, fq
DECLARED = 15


def test_declared_bound_and_wrapped():
    from epnn_amd import _lib, charge_gn, engine
    header = open(os.path.join(ROOT, "include", "epnn.h")).read()
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", header)
    assert m, "include/epnn.h does not declare " + NAME
    declared = [a.strip() for a in m.group(1).split(",")]
    assert len(declared) == DECLARED and declared[0].startswith("epnn_handle") and declared[-1].endswith("fq_out")
    assert [a.split()[-1].lstrip("*") for a in declared[7:9]] == ["ke", "alpha"] and all(a.startswith("double") for a in declared[7:9])
    assert declared[11].replace(" ", "") == "double*e_out"
    assert NAME in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[NAME]
    assert len(args) == len(declared)
    for cls in (engine.Engine, charge_gn.EPNNModel):
        fn = getattr(cls, "coulomb_xyz", None)
        assert fn is not None, f"{cls.__name__}.coulomb_xyz is missing"
        assert list(inspect.signature(fn).parameters)[1:] == ARGS
    assert inspect.signature(charge_gn.EPNNModel.coulomb_xyz).parameters["N"].default is None
    for mod in (engine, charge_gn):
        assert mod.KE_EV_ANGSTROM == 14.3996454784255
        for cls_fn in (engine.Engine.coulomb_xyz, charge_gn.EPNNModel.coulomb_xyz):
            p = inspect.signature(cls_fn).parameters
            assert p["ke"].default == mod.KE_EV_ANGSTROM and p["alpha"].default == 0.0 and p["parts"].default is False
    assert "INTEGRATION.md" in header[header.index("electrostatics of the predicted charges"):m.start()]


def test_the_source_files_are_part_of_the_translation_unit():
    api = open(os.path.join(ROOT, "epnn_amd", "csrc", "epnn_api.hip")).read()
    assert '#include "epnn_api_coulomb.hip.h"' in api
    drv = open(os.path.join(ROOT, "epnn_amd", "csrc", "epnn_api_coulomb.hip.h")).read()
    assert '#include "epnn_coulomb.hip.h"' in drv and 'extern "C" int ' + NAME in drv
    assert os.path.exists(os.path.join(ROOT, "epnn_amd", "csrc", "epnn_coulomb.hip.h"))
