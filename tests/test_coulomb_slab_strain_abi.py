"""epnn_coulomb_xyz_slab_strain through the layers that need no GPU: declared in include/epnn.h behind epnn_coulomb_xyz_slab, bound in
epnn_amd/_lib.py with as many arguments as the header declares, reachable as Engine.coulomb_xyz_slab_strain and
EPNNModel.coulomb_xyz_slab_strain; its kernels in the slab's kernel file, the plain slab kernels still there under their names."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "epnn_coulomb_xyz_slab_strain"
PLAIN = "epnn_coulomb_xyz_slab"
ARGS = ["offsets", "xyz", "x", "Q", "N", "cell", "box", "ke", "alpha", "tol", "ewald", "parts", "exclusions"]
# the plain slab entry's first fifteen arguments, then the nine outputs of epnn_coulomb_xyz_cell_excl
OUTPUTS = ["float*q_out", "float*phi_out", "double*e_out", "float*f_out", "float*gstrain_out", "float*ffix_out", "float*fq_out",
           "float*gstrain_fix_out", "float*gstrain_q_out"]
DECLARED = 15 + len(OUTPUTS)


def _declared(header, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", header)
    assert m, "include/epnn.h does not declare " + name
    return m, [a.strip().replace(" ", "") for a in m.group(1).split(",")]


def test_declared_behind_the_plain_entry_with_the_periodic_outputs():
    header = open(os.path.join(ROOT, "include", "epnn.h")).read()
    m, declared = _declared(header, NAME)
    mp, plain = _declared(header, PLAIN)
    _, cell_excl = _declared(header, "epnn_coulomb_xyz_cell_excl")
    assert mp.end() < m.start(), "the new entry is declared behind epnn_coulomb_xyz_slab"
    assert len(declared) == DECLARED and declared[:15] == plain[:15] and declared[15:] == OUTPUTS
    assert declared == cell_excl                                                  # the same list, argument for argument
    doc = header[mp.end():m.start()]
    for text in ("gstrain_out [B][3][3] is required", "2 z_ij (n eps k)", "43 * 2^-24", "16 * 2^-24", "48 A cpieces + 48 A + 36 B", "INTEGRATION.md"):
        assert text in doc, text
    assert "Still missing: one periodic axis (wires); the strain derivative of the slab sum; PME" in header
    assert "No strain derivative" not in header


def test_bound_and_wrapped():
    from epnn_amd import _lib, charge_gn, engine
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == DECLARED
    assert _lib.SIGNATURES[NAME][1] == _lib.SIGNATURES["epnn_coulomb_xyz_cell_excl"][1]
    assert hasattr(_lib.load(), NAME)
    for cls in (engine.Engine, charge_gn.EPNNModel):
        fn = getattr(cls, "coulomb_xyz_slab_strain", None)
        assert fn is not None, f"{cls.__name__}.coulomb_xyz_slab_strain is missing"
        p = inspect.signature(fn).parameters
        assert list(p)[1:] == ARGS
        assert p["cell"].default is None and p["box"].default is None and p["ewald"].default is None and p["exclusions"].default is None
        assert p["ke"].default == engine.KE_EV_ANGSTROM and p["alpha"].default == 0.0 and p["tol"].default == 1e-6
        assert p["parts"].default is False
        assert list(inspect.signature(cls.coulomb_xyz_slab).parameters) == list(p)
    assert inspect.signature(charge_gn.EPNNModel.coulomb_xyz_slab_strain).parameters["N"].default is None
    assert "_coulomb(" in inspect.getsource(engine.Engine.coulomb_xyz_slab_strain)


def test_the_kernels_are_in_the_slab_file():
    csrc = os.path.join(ROOT, "epnn_amd", "csrc")
    kernels = open(os.path.join(csrc, "epnn_ewald_slab.hip.h")).read()
    for k in ("k_sl_sweep", "k_sl_atom", "k_sl_atom_x", "k_sl_sweep_strain", "k_sl_atom_strain", "k_sl_energy_strain"):
        assert re.search(r"__global__ __launch_bounds__\(\d+\) void " + k + r"\(", kernels), k
    assert "__launch_bounds__(64) void k_sl_sweep_strain" in kernels and "template <bool STRAIN>" in kernels
    assert "sl_sweep_body<false>" in kernels and "sl_sweep_body<true>" in kernels and "atomicAdd" not in kernels
    # the slab has no driver of its own: its two entries reach coulomb_run, which launches the strain kernels and runs the one backward
    for f in os.listdir(csrc):
        assert "coulomb_slab_run" not in open(os.path.join(csrc, f)).read(), f
    ent = open(os.path.join(csrc, "epnn_api_coulomb_slab.hip.h")).read()
    assert 'extern "C" int ' + NAME + "(" in ent and 'extern "C" int ' + PLAIN + "(" in ent
    assert "return coulomb_run(" in ent and ent.count("coulomb_slab_enter(h, ") == 2
    drv = open(os.path.join(csrc, "epnn_api_coulomb_run.hip.h")).read()
    assert drv.count("gl_grad_backward(") == 1 and "gl_grad_backward(h, gl, r, B, strain)" in drv
    for k in ("k_sl_sweep_strain", "k_sl_atom_strain", "k_sl_energy_strain"):
        assert k in drv, k
    for other in ("epnn_coulomb.hip.h", "epnn_ewald.hip.h"):
        assert "k_sl_" not in open(os.path.join(csrc, other)).read()
