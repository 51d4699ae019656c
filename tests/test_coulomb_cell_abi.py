"""epnn_coulomb_xyz_cell and epnn_ewald_params through the layers that need no GPU: declared in include/epnn.h, bound in
epnn_amd/_lib.py with as many arguments as the header declares, reachable as Engine.coulomb_xyz_cell, Engine.ewald_params and
EPNNModel.coulomb_xyz_cell, and their sources part of the translation unit beside the open call's, which stays as it is."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "epnn_coulomb_xyz_cell"
HELPER = "epnn_ewald_params"
ARGS = ["offsets", "xyz", "x", "Q", "N", "cell", "box", "ke", "alpha", "tol", "ewald", "parts", "strain"]
# the handle, B, N, offsets, xyz, x, Q, cell, ewald, ke, alpha, and the nine outputs q, phi, e, f, gstrain, ffix, fq, gstrain_fix, gstrain_q
DECLARED = 20


def _declared(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, "include/epnn.h does not declare " + name
    return m, [a.strip() for a in m.group(1).split(",")]


def test_declared_bound_and_wrapped():
    from epnn_amd import _lib, charge_gn, engine
    header = open(os.path.join(ROOT, "include", "epnn.h")).read()
    m, declared = _declared(header, NAME)
    assert len(declared) == DECLARED and declared[0].startswith("epnn_handle") and declared[-1].endswith("gstrain_q_out")
    assert declared[7].replace(" ", "") == "constfloat*cell" and declared[8].replace(" ", "") == "constdouble*ewald"
    assert [a.split()[-1].lstrip("*") for a in declared[9:11]] == ["ke", "alpha"] and all(a.startswith("double") for a in declared[9:11])
    assert declared[13].replace(" ", "") == "double*e_out" and declared[15].replace(" ", "") == "float*gstrain_out"
    _, helper = _declared(header, HELPER)
    assert [a.replace(" ", "") for a in helper] == ["constfloat*cell", "doublealpha", "doubletol", "double*out"]
    for name, n in ((NAME, DECLARED), (HELPER, 4)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n
    for cls in (engine.Engine, charge_gn.EPNNModel):
        fn = getattr(cls, "coulomb_xyz_cell", None)
        assert fn is not None, f"{cls.__name__}.coulomb_xyz_cell is missing"
        p = inspect.signature(fn).parameters
        assert list(p)[1:] == ARGS
        assert p["cell"].default is None and p["box"].default is None and p["ewald"].default is None
        assert p["ke"].default == engine.KE_EV_ANGSTROM and p["alpha"].default == 0.0 and p["tol"].default == 1e-6
        assert p["parts"].default is False and p["strain"].default is False
    assert inspect.signature(charge_gn.EPNNModel.coulomb_xyz_cell).parameters["N"].default is None
    assert list(inspect.signature(engine.Engine.ewald_params).parameters)[1:] == ["cell", "alpha", "tol"]
    # the open call keeps its own argument list: the periodic call is a method of its own
    assert "cell" not in inspect.signature(engine.Engine.coulomb_xyz).parameters
    start = header.index("electrostatics of the predicted charges in fully periodic cells")
    assert "INTEGRATION.md" in header[start:m.start()] and "tol" in header[start:m.start()]


def test_the_source_files_are_part_of_the_translation_unit():
    api = open(os.path.join(ROOT, "epnn_amd", "csrc", "epnn_api.hip")).read()
    assert '#include "epnn_api_coulomb_cell.hip.h"' in api
    assert api.index('#include "epnn_api_coulomb.hip.h"') < api.index('#include "epnn_api_coulomb_cell.hip.h"')
    drv = open(os.path.join(ROOT, "epnn_amd", "csrc", "epnn_api_coulomb_cell.hip.h")).read()
    assert '#include "epnn_ewald.hip.h"' in drv and 'extern "C" int ' + NAME in drv and 'extern "C" int ' + HELPER in drv
    kernels = open(os.path.join(ROOT, "epnn_amd", "csrc", "epnn_ewald.hip.h")).read()
    for k in ("k_ew_sweep", "k_ew_sfac", "k_ew_atom", "k_ew_energy"):
        assert "void " + k + "(" in kernels
    # the open call's kernels are in their own file and know nothing of the periodic ones
    assert "k_ew_" not in open(os.path.join(ROOT, "epnn_amd", "csrc", "epnn_coulomb.hip.h")).read()
