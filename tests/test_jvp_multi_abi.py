"""epnn_charges_jvp_multi_xyz_cell through the layers that need no GPU: declared in include/epnn.h with its 14 parameters (the 13 of
epnn_charges_jvp_xyz_cell and K in front of the tangents), bound in epnn_amd/_lib.py with as many, reachable as Engine.charges_jvp_xyz_multi and EPNNModel.charges_jvp_xyz_multi, used by
EPNNModel.charge_strain_response, and defined in the driver beside the single-tangent entry."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "epnn_charges_jvp_multi_xyz_cell"
ARGS = ["offsets", "xyz", "x", "Q", "N", "v", "strain", "dQ", "box", "cell"]


def test_declared_bound_and_wrapped():
    from epnn_amd import _lib, charge_gn, engine
    header = open(os.path.join(ROOT, "include", "epnn.h")).read()
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*)\)\s*;", header)
    assert m, f"include/epnn.h does not declare {NAME}"
    declared = [a.strip() for a in m.group(1).split(",")]
    assert len(declared) == 14 and declared[0].startswith("epnn_handle") and declared[-1].endswith("tq_out")
    assert declared[8] == "int K"
    assert NAME in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[NAME]
    assert len(args) == len(declared)
    for cls in (engine.Engine, charge_gn.EPNNModel):
        fn = getattr(cls, "charges_jvp_xyz_multi", None)
        assert fn is not None, f"{cls.__name__}.charges_jvp_xyz_multi is missing"
        assert list(inspect.signature(fn).parameters)[1:] == ARGS
    assert inspect.signature(engine.Engine.charges_jvp_xyz_multi).parameters["N"].default is inspect.Parameter.empty
    assert inspect.signature(charge_gn.EPNNModel.charges_jvp_xyz_multi).parameters["N"].default is None
    fn = getattr(charge_gn.EPNNModel, "charge_strain_response", None)
    assert fn is not None, "EPNNModel.charge_strain_response is missing"
    assert list(inspect.signature(fn).parameters)[1:] == ["offsets", "xyz", "x", "Q", "N", "box", "cell"]


def test_the_entry_is_defined_in_the_driver():
    drv = open(os.path.join(ROOT, "epnn_amd", "csrc", "epnn_api_jvp.hip.h")).read()
    assert 'extern "C" int ' + NAME in drv and 'extern "C" int epnn_charges_jvp_xyz_cell' in drv
    kernels = open(os.path.join(ROOT, "epnn_amd", "csrc", "epnn_jvp.hip.h")).read()
    for k in ("k_jvm_edge", "k_jvm_proj", "k_jvm_sweep", "k_jvm_gnn_pair", "k_jvm_epn_pair", "k_jvm_gnn_tail"):
        assert re.search(r"\bvoid\s+" + k + r"\b", kernels), k
