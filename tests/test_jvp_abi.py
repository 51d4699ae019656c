"""epnn_charges_jvp_xyz_cell through the layers that need no GPU: declared in include/epnn.h, bound in epnn_amd/_lib.py with as many
arguments as the header declares, and reachable as Engine.charges_jvp_xyz and EPNNModel.charges_jvp_xyz."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["offsets", "xyz", "x", "Q", "N", "v", "strain", "dQ", "box", "cell"]


def test_declared_bound_and_wrapped():
    from epnn_amd import _lib, charge_gn, engine
    header = open(os.path.join(ROOT, "include", "epnn.h")).read()
    m = re.search(r"\bint\s+epnn_charges_jvp_xyz_cell\s*\(([^;]*)\)\s*;", header)
    assert m, "include/epnn.h does not declare epnn_charges_jvp_xyz_cell"
    declared = [a.strip() for a in m.group(1).split(",")]
    assert len(declared) == 13 and declared[0].startswith("epnn_handle") and declared[-1].endswith("tq_out")
    assert "epnn_charges_jvp_xyz_cell" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["epnn_charges_jvp_xyz_cell"]
    assert len(args) == len(declared)
    for cls, want in ((engine.Engine, ARGS), (charge_gn.EPNNModel, ARGS)):
        fn = getattr(cls, "charges_jvp_xyz", None)
        assert fn is not None, f"{cls.__name__}.charges_jvp_xyz is missing"
        assert list(inspect.signature(fn).parameters)[1:] == want
    assert inspect.signature(charge_gn.EPNNModel.charges_jvp_xyz).parameters["N"].default is None


def test_the_source_files_are_part_of_the_translation_unit():
    api = open(os.path.join(ROOT, "epnn_amd", "csrc", "epnn_api.hip")).read()
    assert '#include "epnn_api_jvp.hip.h"' in api
    drv = open(os.path.join(ROOT, "epnn_amd", "csrc", "epnn_api_jvp.hip.h")).read()
    assert '#include "epnn_jvp.hip.h"' in drv and 'extern "C" int epnn_charges_jvp_xyz_cell' in drv
