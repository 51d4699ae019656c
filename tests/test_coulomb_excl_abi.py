"""epnn_coulomb_xyz_excl and epnn_coulomb_xyz_cell_excl through the layers that need no GPU: declared in include/epnn.h, bound in
epnn_amd/_lib.py with the argument types the header declares, reachable from Engine and EPNNModel, their kernel part of the
translation unit; the plain entries keep their declarations."""
import ctypes as C
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIST = ["int64_t npairs", "const int32_t *ex_i", "const int32_t *ex_j", "const float *ex_scale"]


def _declared(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, "include/epnn.h does not declare " + name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def _ctype(decl):
    t = decl.replace("const ", "")
    t = t[:t.rindex("*") + 1] if "*" in t else t.rsplit(" ", 1)[0]
    return {"epnn_handle *": C.c_void_p, "int": C.c_int, "int64_t": C.c_int64, "double": C.c_double, "int32_t *": C.POINTER(C.c_int32),
            "float *": C.POINTER(C.c_float), "double *": C.POINTER(C.c_double)}[t.strip()]


def test_declared_and_bound_with_matching_types():
    from epnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "epnn.h")).read()
    for name, plain, at in (("epnn_coulomb_xyz_excl", "epnn_coulomb_xyz", 9), ("epnn_coulomb_xyz_cell_excl", "epnn_coulomb_xyz_cell", 11)):
        decl, base = _declared(header, name), _declared(header, plain)
        # the plain entry's arguments with the list between alpha and the outputs
        assert decl == base[:at] + LIST + base[at:], name
        assert base[at - 1] == "double alpha"
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(decl)
        for k, (a, d) in enumerate(zip(args, decl)):
            assert a is _ctype(d), (name, k, d)
        assert _lib.SIGNATURES[plain][1] == args[:at] + args[at + 4:]
    doc = header[header.index("bonded exclusions and pair scaling for the two calls above"):header.index("int epnn_coulomb_xyz_excl")]
    for word in ("INTEGRATION.md", "npairs == 0", "listed twice", "2e-6", "34 * 2^-24", "(A + 1) 4 + 16 P + 32 A", "(A + 1) 4 + 16 P + 80 A"):
        assert word in doc, word


def test_wrapped_and_part_of_the_translation_unit():
    from epnn_amd import charge_gn, engine
    for cls in (engine.Engine, charge_gn.EPNNModel):
        for plain in ("coulomb_xyz", "coulomb_xyz_cell"):
            p, base = inspect.signature(getattr(cls, plain + "_excl")).parameters, inspect.signature(getattr(cls, plain)).parameters
            assert list(p) == list(base) + ["exclusions"] and p["exclusions"].default is None
            assert all(p[k].default == base[k].default for k in base)
    p = inspect.signature(engine.bonded_exclusions).parameters
    assert list(p) == ["bonds", "n_atoms", "scale12", "scale13", "scale14"]
    assert (p["scale12"].default, p["scale13"].default, p["scale14"].default) == (0.0, 0.0, 0.5)
    csrc = os.path.join(ROOT, "epnn_amd", "csrc")
    open_drv, cell_drv = (open(os.path.join(csrc, f)).read() for f in ("epnn_api_coulomb.hip.h", "epnn_api_coulomb_cell.hip.h"))
    assert 'extern "C" int epnn_coulomb_xyz_excl(' in open_drv and 'extern "C" int epnn_coulomb_xyz_cell_excl(' in cell_drv
    assert "static int excl_build(" in open_drv and cell_drv.count("excl_build(") == 1          # one validator, shared
    kernels = open(os.path.join(csrc, "epnn_coulomb.hip.h")).read()
    assert "void k_cl_excl(" in kernels and "void k_cl_atom(" in kernels and "void k_cl_atom_x(" in kernels
    assert "void k_ew_atom_x(" in open(os.path.join(csrc, "epnn_ewald.hip.h")).read()
    assert os.path.exists(os.path.join(ROOT, "tools", "excl_host_check.hip"))
