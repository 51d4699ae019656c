"""epnn_coulomb_xyz_slab_site and epnn_coulomb_xyz_slab_strain_site through the layers that need no GPU: declared in include/epnn.h,
exported, bound in epnn_amd/_lib.py with the argument types the header declares, reachable from Engine and EPNNModel, their kernels
part of the translation unit and launched by the one driver; the refusals that are made before a handle is needed.  The library's own
refusals of arguments (site_build, the width check) sit behind the handle's checks: they run on the device's tests
(tests/test_gpu_coulomb_slab_site.py) and, on the host alone, in tools/ewald_host_check.hip; here the slab entry is held to call the
one validator and the one width check with its row's beta, and the message's wording to be the periodic entry's.  CPU only."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from test_coulomb_excl_abi import LIST, ROOT, _ctype, _declared
from test_site_abi import SITE

ENTRIES = (("epnn_coulomb_xyz_slab_site", "epnn_coulomb_xyz_slab", 16), ("epnn_coulomb_xyz_slab_strain_site", "epnn_coulomb_xyz_slab_strain", 16))


def test_declared_exported_and_bound_with_matching_types():
    from epnn_amd import _lib
    header = open(os.path.join(ROOT, "include", "epnn.h")).read()
    lib = _lib.load()
    for name, base_name, phi_at in ENTRIES:
        decl, base = _declared(header, name), _declared(header, base_name)
        # the slab entry's arguments with the site arrays behind alpha and mu_out behind phi_out: the order of epnn_coulomb_xyz_cell_site
        assert base[10] == "double alpha" and base[11:15] == LIST and base[phi_at] == "float *phi_out"
        assert decl == base[:11] + SITE + base[11:phi_at + 1] + ["float *mu_out"] + base[phi_at + 1:], name
        assert hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(decl)
        for k, (a, d) in enumerate(zip(args, decl)):
            assert a is _ctype(d), (name, k, d)
    assert _declared(header, "epnn_coulomb_xyz_slab_strain_site") == _declared(header, "epnn_coulomb_xyz_cell_site")
    doc = header[header.index("per-atom Gaussian widths, self-energy and on-site terms in slab cells"):header.index("int epnn_coulomb_xyz_slab_site")]
    for word in ("no background term and no per-pair k = 0 correction", "gamma_ii = 1 / (2 sigma_i)", "1 / (2 beta)", "mu_out == phi_out",
                 "epnn_ewald_slab_params(cell, 0, tol)", "16 A + 4 A", "no per-cell sum", "bitwise symmetric", "k_ew_sweep_site"):
        assert word in doc, word


def test_wrapped_and_part_of_the_translation_unit():
    from epnn_amd import charge_gn, engine
    for cls in (engine.Engine, charge_gn.EPNNModel):
        p, base = inspect.signature(cls.coulomb_xyz_slab_site).parameters, inspect.signature(cls.coulomb_xyz_cell_site).parameters
        assert list(p) == list(base)                             # shaped like coulomb_xyz_cell_site
        assert all(p[k].default == base[k].default for k in base)
        assert p["strain"].default is False and p["self_energy"].default is True
    csrc = os.path.join(ROOT, "epnn_amd", "csrc")
    slab_drv, run, ent, kernels = (open(os.path.join(csrc, f)).read() for f in ("epnn_api_coulomb_slab.hip.h", "epnn_api_coulomb_run.hip.h",
                                                                               "epnn_api_site.hip.h", "epnn_ewald_slab.hip.h"))
    assert 'extern "C" int epnn_coulomb_xyz_slab_site(' in ent and 'extern "C" int epnn_coulomb_xyz_slab_strain_site(' in ent
    assert ent.count("coulomb_slab_enter(") == 2 and "hipLaunchKernelGGL" not in ent                   # through the slab entries' path
    # one validator and one width check, shared with the other site entries; the check sees the row's beta
    assert slab_drv.count("site_build(") == 1 and "static int site_build(" not in slab_drv
    assert re.search(r"site_width_check\(name, b, site\.sigma_max\[b\], ewald\[6 \* \(size_t\)b\]\)", slab_drv)
    assert "static int site_width_check(" not in slab_drv
    assert len(re.findall(r"^static int coulomb_run\(", run, flags=re.M)) == 1                       # still the one driver
    for k in ("template <bool X, bool STRAIN, bool SITE = false>", "void k_sl_atom_site(", "void k_sl_atom_strain_site("):
        assert k in kernels, k
    for k in ("k_sl_atom_site<true>", "k_sl_atom_site<false>", "k_sl_atom_strain_site", "k_ew_sweep_site"):
        assert k in run, k
    # the width check's wording is the periodic entry's: one function, one message
    cell_drv = open(os.path.join(csrc, "epnn_api_coulomb_cell.hip.h")).read()
    assert cell_drv.count("sigma_max = %g is above the largest width 1 / (2 beta) = %g") == 1
    host = open(os.path.join(ROOT, "tools", "ewald_host_check.hip")).read()
    assert "CL_SLAB" in host and "epnn_coulomb_xyz_slab_site" in host


def test_null_arguments_are_refused_without_a_device():
    """The entries' first check needs neither a handle nor a device: a NULL handle or a NULL required output is refused by name."""
    from epnn_amd import _lib
    lib = _lib.load()
    lib.epnn_last_error.restype = C.c_char_p
    for name, _, _ in ENTRIES:
        res, args = _lib.SIGNATURES[name]
        zero = [0 if a in (C.c_int, C.c_int64) else 0.0 if a is C.c_double else None for a in args]
        assert getattr(lib, name)(*zero) == 1
        assert lib.epnn_last_error().decode() == name + ": null argument"


def test_python_refusals_need_no_device():
    """The argument checks Engine._coulomb makes before it reaches the library, on an Engine that was never given a handle."""
    from epnn_amd.engine import Engine
    eng = Engine.__new__(Engine)
    eng.nx, eng.h = 9, None
    off, xyz, x, Q = np.int32([0, 3]), np.zeros((3, 3), np.float32), np.zeros((3, 9), np.float32), np.zeros(1, np.float32)
    sg = np.full(3, 0.5, np.float32)
    for strain in (False, True):
        where = "coulomb_xyz_slab_strain_site" if strain else "coulomb_xyz_slab_site"
        kw = {"box": np.float32([8, 8, 0]), "ewald": np.ones(6), "strain": strain}
        with pytest.raises(ValueError, match=where + ": both sigma and alpha"):
            eng.coulomb_xyz_slab_site(off, xyz, x, Q, 8, alpha=0.5, sigma=sg, **kw)
        with pytest.raises(ValueError, match=where + ": self_energy=True with neither sigma nor alpha > 0"):
            eng.coulomb_xyz_slab_site(off, xyz, x, Q, 8, chi=sg, **kw)
        for bad in ({"sigma": sg[:2]}, {"sigma": sg, "chi": np.zeros(4)}, {"sigma": sg, "hardness": np.zeros((3, 1))}):
            with pytest.raises(ValueError, match=r"must have shape \(3,\)"):
                eng.coulomb_xyz_slab_site(off, xyz, x, Q, 8, **bad, **kw)
        with pytest.raises(ValueError, match=r"shape \(P, 2\)"):
            eng.coulomb_xyz_slab_site(off, xyz, x, Q, 8, sigma=sg, exclusions=(np.zeros((2, 3), np.int32), 0.0), **kw)
        with pytest.raises(ValueError, match=r"ewald must have shape \(6,\) or \(1, 6\)"):
            eng.coulomb_xyz_slab_site(off, xyz, x, Q, 8, sigma=sg, box=np.float32([8, 8, 0]), ewald=np.ones(5), strain=strain)
        for box in (np.float32([8, 8, 8]), np.float32([8, 0, 0])):                       # cubes and wires
            with pytest.raises(ValueError, match=where + ": box must have exactly one zero"):
                eng.coulomb_xyz_slab_site(off, xyz, x, Q, 8, sigma=sg, box=box, strain=strain)
        with pytest.raises(ValueError, match="give cell= or box="):
            eng.coulomb_xyz_slab_site(off, xyz, x, Q, 8, sigma=sg, strain=strain)
