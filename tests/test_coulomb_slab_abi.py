"""epnn_coulomb_xyz_slab and epnn_ewald_slab_params through the layers that need no GPU: declared in include/epnn.h, bound in
epnn_amd/_lib.py with as many arguments as the header declares, reachable as Engine.coulomb_xyz_slab, Engine.ewald_slab_params and
EPNNModel.coulomb_xyz_slab; the host-only rule against slab_ref.slab_params64 and its refusals by name; the new kernels in a file of
their own, part of the translation unit, beside the open and the periodic call's, which stay as they are."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from slab_ref import slab_params64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "epnn_coulomb_xyz_slab"
HELPER = "epnn_ewald_slab_params"
ARGS = ["offsets", "xyz", "x", "Q", "N", "cell", "box", "ke", "alpha", "tol", "ewald", "parts", "exclusions"]
# the handle, B, N, offsets, xyz, x, Q, cell, ewald, ke, alpha, the list npairs, ex_i, ex_j, ex_scale and the six outputs q, phi, e, f, ffix, fq
DECLARED = 21


def _declared(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, "include/epnn.h does not declare " + name
    return m, [a.strip() for a in m.group(1).split(",")]


def test_declared_bound_and_wrapped():
    from epnn_amd import _lib, charge_gn, engine
    header = open(os.path.join(ROOT, "include", "epnn.h")).read()
    m, declared = _declared(header, NAME)
    assert len(declared) == DECLARED and declared[0].startswith("epnn_handle") and declared[-1].endswith("fq_out")
    assert declared[7].replace(" ", "") == "constfloat*cell" and declared[8].replace(" ", "") == "constdouble*ewald"
    assert [a.split()[-1].lstrip("*") for a in declared[9:11]] == ["ke", "alpha"] and all(a.startswith("double") for a in declared[9:11])
    assert [a.replace(" ", "") for a in declared[11:15]] == ["int64_tnpairs", "constint32_t*ex_i", "constint32_t*ex_j", "constfloat*ex_scale"]
    assert declared[17].replace(" ", "") == "double*e_out"
    _, helper = _declared(header, HELPER)
    assert [a.replace(" ", "") for a in helper] == ["constfloat*cell", "doublealpha", "doubletol", "double*out"]
    for name, n in ((NAME, DECLARED), (HELPER, 4)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n
    for cls in (engine.Engine, charge_gn.EPNNModel):
        fn = getattr(cls, "coulomb_xyz_slab", None)
        assert fn is not None, f"{cls.__name__}.coulomb_xyz_slab is missing"
        p = inspect.signature(fn).parameters
        assert list(p)[1:] == ARGS
        assert p["cell"].default is None and p["box"].default is None and p["ewald"].default is None and p["exclusions"].default is None
        assert p["ke"].default == engine.KE_EV_ANGSTROM and p["alpha"].default == 0.0 and p["tol"].default == 1e-6
        assert p["parts"].default is False
    assert inspect.signature(charge_gn.EPNNModel.coulomb_xyz_slab).parameters["N"].default is None
    sig = inspect.signature(engine.Engine.ewald_slab_params).parameters
    assert list(sig)[1:] == ["cell", "alpha", "tol"] and sig["alpha"].default == 0.0 and sig["tol"].default == 1e-6
    start = header.index("electrostatics of the predicted charges in slab cells")
    doc = header[start:m.start()]
    assert "INTEGRATION.md" in doc and "No neutralising" in doc and "41 * 2^-24" in doc and "16 * 2^-24" in doc
    assert "Still missing: one periodic axis (wires); the strain derivative of the slab sum; PME" in header


def _loaded_lib():
    from epnn_amd import _lib
    return _lib.load()


def _rule(lib, cell, alpha, tol):
    cell = np.ascontiguousarray(cell, dtype=np.float32)
    out = np.full(6, np.nan)
    rc = lib.epnn_ewald_slab_params(cell.ctypes.data_as(C.POINTER(C.c_float)), float(alpha), float(tol), out.ctypes.data_as(C.POINTER(C.c_double)))
    return rc, out


CELLS = [np.float32([[0, 0, 0], [6.8, 1.0, 1.5], [-0.5, 6.0, 3.5]]), np.float32([[6.5, 0, 0], [0, 0, 0], [0, 1, 9]]),
         np.float32([[7, 0, 0], [2, 6.9, 0], [0, 0, 0]])]


@pytest.mark.parametrize("open_row", [0, 1, 2])
def test_the_rule_without_a_gpu_equals_the_reference(open_row):
    lib = _loaded_lib()
    cell = CELLS[open_row]
    assert not cell[open_row].any()
    for alpha, tol in ((0.0, 1e-6), (0.0, 1e-10), (2.0, 1e-6), (0.5, 1e-6)):
        rc, got = _rule(lib, cell, alpha, tol)
        want = slab_params64(cell, alpha, tol)
        assert rc == 0 and got[3 + open_row] == 0
        assert np.array_equal(got[3:], want[3:]) and np.allclose(got[:3], want[:3], rtol=1e-14, atol=0)
    assert _rule(lib, cell, 0.5, 1e-6)[1][1] == 0                                # beta capped at alpha: no real-space part


def test_the_rule_refuses_by_name():
    lib = _loaded_lib()
    good = CELLS[2]
    cube, wire, none = good.copy(), good.copy(), np.zeros((3, 3), np.float32)
    cube[2] = [0, 0, 9]
    wire[1] = 0
    dependent = np.float32([[7, 0, 0], [14, 0, 0], [0, 0, 0]])
    inf = good.copy()
    inf[0, 1] = np.inf
    needle = np.float32([[6, 0, 0], [0, 3e6, 0], [0, 0, 0]])
    for cell, alpha, tol, text in ((cube, 0.0, 1e-6, "use epnn_coulomb_xyz_cell"), (wire, 0.0, 1e-6, "not built"), (none, 0.0, 1e-6, "not built"),
                                   (dependent, 0.0, 1e-6, "linearly dependent"), (inf, 0.0, 1e-6, "not finite"),
                                   (good, -1.0, 1e-6, "alpha must be finite"), (good, float("nan"), 1e-6, "alpha must be finite"),
                                   (good, 0.0, 0.0, "tol must be finite"), (good, 0.0, 1.0, "tol must be finite"),
                                   (good, 0.0, float("nan"), "tol must be finite"), (needle, 0.0, 1e-6, "cap")):
        rc, _ = _rule(lib, cell, alpha, tol)
        said = lib.epnn_last_error().decode(errors="replace")
        assert rc != 0 and text in said, (text, said)
    assert _rule(lib, good, 0.0, 1e-6)[0] == 0


def test_the_source_files_are_part_of_the_translation_unit():
    csrc = os.path.join(ROOT, "epnn_amd", "csrc")
    api = open(os.path.join(csrc, "epnn_api.hip")).read()
    assert '#include "epnn_api_coulomb_slab.hip.h"' in api
    assert api.index('#include "epnn_api_coulomb_cell.hip.h"') < api.index('#include "epnn_api_coulomb_slab.hip.h"')
    assert api.index('#include "epnn_api_coulomb_slab.hip.h"') < api.index('#include "epnn_api_coulomb_run.hip.h"')
    ent = open(os.path.join(csrc, "epnn_api_coulomb_slab.hip.h")).read()
    assert '#include "epnn_ewald_slab.hip.h"' in ent and 'extern "C" int ' + NAME in ent and 'extern "C" int ' + HELPER in ent
    drv = open(os.path.join(csrc, "epnn_api_coulomb_run.hip.h")).read()
    assert "k_ew_sweep<true>" in drv and "gl_grad_forward(" in drv and "gl_grad_backward(" in drv
    kernels = open(os.path.join(csrc, "epnn_ewald_slab.hip.h")).read()
    for k in ("k_sl_sweep", "k_sl_atom", "k_sl_atom_x"):
        assert "void " + k + "(" in kernels
    assert "__launch_bounds__(64) void k_sl_sweep" in kernels and "erfcxf" in kernels
    # the open and the periodic call's kernels are in their own files and know nothing of the slab's
    for other in ("epnn_coulomb.hip.h", "epnn_ewald.hip.h"):
        assert "k_sl_" not in open(os.path.join(csrc, other)).read()


def test_the_six_entries_share_one_forward_and_one_download():
    csrc = os.path.join(ROOT, "epnn_amd", "csrc")
    text = "".join(open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if re.fullmatch(r"epnn_api_coulomb.*\.hip\.h", f))
    assert text.count('extern "C" int epnn_coulomb_xyz') == 6
    assert text.count("gl_grad_forward(") == 1 and text.count("hipMemcpyDeviceToHost") == 1
