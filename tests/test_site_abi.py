"""epnn_coulomb_xyz_site and epnn_coulomb_xyz_cell_site through the layers that need no GPU: declared in include/epnn.h, exported,
bound in epnn_amd/_lib.py with the argument types the header declares, reachable from Engine and EPNNModel, their kernels part of the
translation unit; engine.per_element; the _excl entries keep their declarations.  CPU only."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_coulomb_excl_abi import LIST, ROOT, _ctype, _declared

SITE = ["const float *sigma", "const float *chi", "const float *hard", "int self_term"]


def test_declared_exported_and_bound_with_matching_types():
    from epnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "epnn.h")).read()
    lib = _lib.load()
    for name, excl, at, phi_at in (("epnn_coulomb_xyz_site", "epnn_coulomb_xyz_excl", 9, 14), ("epnn_coulomb_xyz_cell_site", "epnn_coulomb_xyz_cell_excl", 11, 16)):
        decl, base = _declared(header, name), _declared(header, excl)
        # the _excl entry's arguments with the site arrays between alpha and the list, and mu_out behind phi_out
        assert base[at - 1] == "double alpha" and base[phi_at] == "float *phi_out"
        assert decl == base[:at] + SITE + base[at:phi_at + 1] + ["float *mu_out"] + base[phi_at + 1:], name
        assert decl[at + 4:at + 8] == LIST
        assert hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(decl)
        for k, (a, d) in enumerate(zip(args, decl)):
            assert a is _ctype(d), (name, k, d)
    doc = header[header.index("per-atom Gaussian widths, self-energy and on-site terms: the energy"):header.index("int epnn_coulomb_xyz_site")]
    for word in ("INTEGRATION.md", "gamma_ij = 1 / sqrt(2 (sigma_i^2 + sigma_j^2))", "NOT multiplied by", "phi_bg_i", "1 / (2 beta)", "mu_out == phi_out",
                 "rsqrtf(w_i + w_j)", "16 A + 4 A + 8 B", "npairs == 0"):
        assert word in doc, word
    assert "Still missing: one periodic axis (wires); the strain derivative of the slab sum; PME" in header


def test_wrapped_and_part_of_the_translation_unit():
    from epnn_amd import charge_gn, engine
    for cls in (engine.Engine, charge_gn.EPNNModel):
        for plain in ("coulomb_xyz", "coulomb_xyz_cell"):
            p, base = inspect.signature(getattr(cls, plain + "_site")).parameters, inspect.signature(getattr(cls, plain + "_excl")).parameters
            assert set(p) == set(base) | {"sigma", "chi", "hardness", "self_energy"}
            assert all(p[k].default == base[k].default for k in base)
            assert p["sigma"].default is None and p["chi"].default is None and p["hardness"].default is None and p["self_energy"].default is True
    csrc = os.path.join(ROOT, "epnn_amd", "csrc")
    open_drv, cell_drv, run, ent = (open(os.path.join(csrc, f)).read() for f in ("epnn_api_coulomb.hip.h", "epnn_api_coulomb_cell.hip.h",
                                                                                "epnn_api_coulomb_run.hip.h", "epnn_api_site.hip.h"))
    assert 'extern "C" int epnn_coulomb_xyz_site(' in ent and 'extern "C" int epnn_coulomb_xyz_cell_site(' in ent
    assert '#include "epnn_api_site.hip.h"' in open(os.path.join(csrc, "epnn_api.hip")).read()
    assert "coulomb_enter(" in ent and "coulomb_cell_enter(" in ent and "hipLaunchKernelGGL" not in ent       # through the _excl entries' path
    assert "static int site_build(" in open_drv and cell_drv.count("site_build(") == 1         # one validator and builder, shared
    assert len(re.findall(r"^static int coulomb_run\(", run, flags=re.M)) == 1                # still the one driver
    kernels, ewald = (open(os.path.join(csrc, f)).read() for f in ("epnn_coulomb.hip.h", "epnn_ewald.hip.h"))
    for k in ("void k_cl_sweep_site(", "void k_cl_atom_site(", "enum ClMode", "template <int MODE, bool CELL>"):
        assert k in kernels, k
    for k in ("void k_ew_sweep_site(", "void k_ew_atom_site(", "void k_ew_wsum(", "void k_ew_energy_site("):
        assert k in ewald, k
    for k in ("k_cl_sweep_site", "k_ew_sweep_site", "k_cl_atom_site", "k_ew_atom_site", "k_ew_energy_site"):
        assert k in run, k


def test_per_element():
    from epnn_amd.engine import per_element
    Z = np.float32([8, 1, 1, 6, 8])
    out = per_element(Z, {1: 0.5, 6: 1.25, 8: 2.0, 17: 9.0})
    assert out.dtype == np.float32 and out.tolist() == [2.0, 0.5, 0.5, 1.25, 2.0]
    assert per_element(Z, {1: 0.5}, default=3.0).tolist() == [3.0, 0.5, 0.5, 3.0, 3.0]
    assert per_element(np.int64([1, 1]), {1: 0.25}).tolist() == [0.25, 0.25]
    assert per_element(np.zeros(0), {}).shape == (0,)
    with pytest.raises(KeyError, match="Z = 6"):
        per_element(Z, {1: 0.5, 8: 2.0})
    with pytest.raises(ValueError, match="whole atomic numbers"):
        per_element(np.float32([1.5]), {1: 0.5})
    with pytest.raises(ValueError, match=r"shape \(A,\)"):
        per_element(np.zeros((2, 9)), {0: 1.0})


def test_python_refusals_need_no_device():
    """The argument checks Engine._coulomb makes before it reaches the library, on an Engine that was never given a handle."""
    from epnn_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.nx, eng.h = 9, None
    off, xyz, x, Q = np.int32([0, 3]), np.zeros((3, 3), np.float32), np.zeros((3, 9), np.float32), np.zeros(1, np.float32)
    sg = np.full(3, 0.5, np.float32)
    for method, kw in ((eng.coulomb_xyz_site, {}), (eng.coulomb_xyz_cell_site, {"box": np.float32([8, 8, 8]), "ewald": np.ones(6)})):
        with pytest.raises(ValueError, match="both sigma and alpha"):
            method(off, xyz, x, Q, 8, alpha=0.5, sigma=sg, **kw)
        with pytest.raises(ValueError, match="neither sigma nor alpha > 0"):
            method(off, xyz, x, Q, 8, chi=sg, **kw)
        for bad in ({"sigma": sg[:2]}, {"sigma": sg, "chi": np.zeros(4)}, {"sigma": sg, "hardness": np.zeros((3, 1))}):
            with pytest.raises(ValueError, match=r"must have shape \(3,\)"):
                method(off, xyz, x, Q, 8, **bad, **kw)
        with pytest.raises(ValueError, match=r"shape \(P, 2\)"):
            method(off, xyz, x, Q, 8, sigma=sg, exclusions=(np.zeros((2, 3), np.int32), 0.0), **kw)
    with pytest.raises(ValueError, match="give cell= or box="):
        eng.coulomb_xyz_cell_site(off, xyz, x, Q, 8, sigma=sg)
