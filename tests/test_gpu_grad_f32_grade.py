"""Every derivative output held to the noise of a float32 model of its reference, not to 2e-4.

A case is ONE route (an entry on one kernel family, chosen by options and geometry), ONE call and ONE batch of molecules of ONE size.
Per case and output, over the real atoms of the batch (the nine strain entries pooled over the batch, the weight gradients per Dense
layer with kernel and bias pooled, and the whole gradient vector's rms):

    rms(out_dev - ref64)  <= K * noise_rms        noise_rms = rms(ref32 - ref64)
    max |out_dev - ref64| <= K * noise_max        noise_max = max |ref32 - ref64|

with K = 4, ref64 the float64 reference and ref32 the same code with dtype=np.float32 (tests/grad_noise_ref.py): weights, edge tensor
as the MLPs see it, activations, tapes, gE, tangents and every Dense product and sweep sum in float32, the geometry in float64 as on
the device (epnn_pair_geo.hip.h), the result rounded to float32.  No floor, no scale term and no kink term: the weights of every input
are nudged until no ReLU pre-activation lies within reach of float32 noise, and tests/test_grad_noise_ref.py asserts on the CPU, for
every case below, that margin, that K noise_max <= 2e-4 max |ref64| (never looser than the standing bound) and that a reference
whose edge cotangent gE, edge tangent te or backward / tangent Dense operands of one MLP family keep only 16 mantissa bits (two bf16
pieces of three) lies at least 3 K noise_rms from float64 in at least one output of the case.  A structurally zero output of the
reference must be exactly zero on the device.  The charges the calls return are held by tests/test_gpu_f32_grade.py.

Sizes: molecules of 2, 16, 17, 33 and 64 atoms at N = n and N = n + 7, and 97 atoms at 97 and 104 where the route takes them (the
row-fused kernels stop at 96); batches of 48, 6, 6, 3, 2, 1 molecules.  nx = 9, T = 2, h_dim = 48.  Open molecules are clusters as in
tests/test_gpu_f32_grade.py; the box (6 A) and the sheared cell (smallest width just above 6 A) are the smallest the entries accept
at cutoff 3.0 and are filled by the references' random_cell, so every atom has image partners.

last_stats() is asserted as far as it tells routes apart: untouched counters of the forward before them on the dense paths; listed
pairs, 0 and the scratch bytes on the pair-list paths.  Row-fused against layer by layer follows from "train_fused" and N <= 96; no
counter says it.

Measured shares of the bounds on an MI355X, worst case of each route: MEASURED below."""
import collections

import numpy as np
import pytest

import cell_ref
import ewald_ref
import grad_noise_ref as gn

K = gn.K

# Worst shares of the two bounds per route, measured on an MI355X: share of K noise_rms (case/output), share of K noise_max (case/output).
MEASURED = """
    vjp_fused_open         10 cases   rms 0.39 (2of2 gxyz)    max 0.53 (16of23 gxyz)
    vjp_layers_open        12 cases   rms 0.38 (2of2 gxyz)    max 0.52 (16of23 gxyz)
    vjp_pairlist_open      12 cases   rms 0.34 (16of23 gxyz)  max 0.44 (16of23 gxyz)
    vjp_fused_box          10 cases   rms 0.30 (2of2 gxyz)    max 0.32 (64of71 gxyz)
    vjp_layers_box         12 cases   rms 0.33 (2of9 gxyz)    max 0.48 (2of9 gxyz)
    vjp_pairlist_box       12 cases   rms 0.46 (2of2 gxyz)    max 0.42 (2of2 gxyz)
    vjp_fused_cell         10 cases   rms 0.38 (2of2 gxyz)    max 0.42 (2of2 gxyz)
    vjp_layers_cell        12 cases   rms 0.39 (2of2 gxyz)    max 0.47 (2of2 gxyz)
    vjp_pairlist_cell      12 cases   rms 0.44 (2of2 gxyz)    max 0.49 (2of2 gxyz)
    strain_dense           12 cases   rms 0.49 (97of97 strain)  max 0.35 (97of97 strain)
    strain_pairlist        12 cases   rms 0.50 (2of2 strain)  max 0.74 (2of2 strain)
    jvp_v_open             12 cases   rms 0.32 (64of64 tq)    max 0.44 (64of64 tq)
    jvp_strain_open        12 cases   rms 0.29 (33of33 tq)    max 0.37 (17of17 tq)
    jvp_dQ_open            12 cases   rms 0.69 (64of64 tq)    max 0.93 (64of71 tq)
    jvp_all_open           12 cases   rms 0.27 (16of16 tq)    max 0.33 (16of23 tq)
    jvp_v_cell             12 cases   rms 0.31 (17of24 tq)    max 0.65 (17of24 tq)
    jvp_strain_cell        12 cases   rms 0.35 (17of17 tq)    max 0.48 (64of64 tq)
    jvp_dQ_cell            12 cases   rms 0.75 (64of64 tq)    max 0.84 (64of64 tq)
    jvp_all_cell           12 cases   rms 0.34 (2of9 tq)      max 0.45 (2of9 tq)
    multi_k1               12 cases   rms 0.32 (64of64 tq0)   max 0.44 (64of64 tq0)
    multi_k16              12 cases   rms 0.75 (64of71 tq6)   max 0.93 (64of71 tq2)
    coulomb                12 cases   rms 0.29 (64of64 fq)    max 0.39 (64of64 fq)
    coulomb_cell           12 cases   rms 0.60 (2of2 fq)      max 0.71 (2of2 fq)
    train_fused            10 cases   rms 0.45 (17of24 layer11)  max 0.42 (17of24 layer11)
    train_layers           12 cases   rms 0.44 (17of24 layer11)  max 0.67 (97of97 layer13)
    train_pairlist         12 cases   rms 0.53 (16of23 layer0)  max 0.56 (16of23 layer12)
    train_pairlist_cell    12 cases   rms 0.38 (17of24 layer9)  max 0.50 (2of9 layer1)
Every route but one holds K = 4: the worst case of a route lies 1.1 .. 3.7 times the float32 model's own noise from float64, where the
forwards' charges lie 0.3 .. 1.5 times theirs (tests/test_gpu_f32_grade.py).  Nearest the bound are the dQ tangents at 64 atoms (jvp_dQ_*
and the columns 2 and 6 of multi_k16, which are dQ alone); which statement of epnn_jvp.hip.h makes them noisier than the v and strain
tangents has not been traced.  strain_dense is listed at its own K = 14 (K_OF_ROUTE has the reason): at K = 4 its case 97of97 measured
1.71 of the rms and 1.23 of the max bound, every other case of it below 0.5.
"""

Case = collections.namedtuple("Case", "id route inp")
DENSE, PAIRLIST = "dense", "pair-list"
# name -> (kernels, entry, geometry, options on a handle with default options, what last_stats() must show)
ROUTES = {}
for _geom in gn.GEOMS:
    ROUTES[f"vjp_fused_{_geom}"] = ("charges_vjp_xyz, dense path, row-fused backward (epnn_train_fused.hip.h, epnn_grad_xyz.hip.h)",
                                    "vjp", _geom, {"grad_path": 1, "train_fused": 1}, DENSE)
    ROUTES[f"vjp_layers_{_geom}"] = ("charges_vjp_xyz, dense path, one launch per Dense layer (epnn_train.hip.h, epnn_grad_xyz.hip.h)",
                                     "vjp", _geom, {"grad_path": 1, "train_fused": 0}, DENSE)
    ROUTES[f"vjp_pairlist_{_geom}"] = ("charges_vjp_xyz, pair-list path k_gl_* (epnn_grad_large.hip.h)", "vjp", _geom, {"grad_path": 2}, PAIRLIST)
ROUTES["strain_dense"] = ("charges_vjp_xyz(strain=True), dense path: the strain sum", "strain", "cell", {"grad_path": 1}, DENSE)
ROUTES["strain_pairlist"] = ("charges_vjp_xyz(strain=True), pair-list path: the strain sum", "strain", "cell", {"grad_path": 2}, PAIRLIST)
for _geom in ("open", "cell"):
    for _kind in ("v", "strain", "dQ", "all"):
        ROUTES[f"jvp_{_kind}_{_geom}"] = (f"charges_jvp_xyz, tangent {_kind} (epnn_jvp.hip.h)", f"jvp_{_kind}", _geom, {}, PAIRLIST)
ROUTES["multi_k1"] = ("charges_jvp_xyz_multi, K = 1", "multi", "open", {}, PAIRLIST)
ROUTES[f"multi_k{gn.MULTI_K}"] = (f"charges_jvp_xyz_multi, K = {gn.MULTI_K}: every column against its own reference", "multi", "open", {}, PAIRLIST)
ROUTES["coulomb"] = ("coulomb_xyz: fq, the backward seeded with phi (epnn_coulomb.hip.h on k_gl_*)", "coulomb", "open", {}, PAIRLIST)
ROUTES["coulomb_cell"] = ("coulomb_xyz_cell: fq and the strain part through the charges (epnn_ewald.hip.h on k_gl_*)", "coulomb_cell", "cell", {}, PAIRLIST)
ROUTES["train_fused"] = ("train_step_xyz weight gradients, row-fused (epnn_train_fused.hip.h)", "train", "open", {"train_fused": 1}, DENSE)
ROUTES["train_layers"] = ("train_step_xyz weight gradients, one launch per Dense layer (epnn_train.hip.h)", "train", "open", {"train_fused": 0}, DENSE)
ROUTES["train_pairlist"] = ("train_step_xyz(cell = zeros) weight gradients, pair-list path (epnn_train_large.hip.h)", "train", "open", {"train_path": 2}, PAIRLIST)
ROUTES["train_pairlist_cell"] = ("train_step_xyz(cell) weight gradients, pair-list path in the sheared cell", "train", "cell", {"train_path": 2}, PAIRLIST)
DEFAULTS = {"grad_path": 0, "train_fused": 1, "train_path": 0}
ROW_FUSED = ("vjp_fused_open", "vjp_fused_box", "vjp_fused_cell", "train_fused")        # N <= 96
# K of a route that is not 4, with its reason and its measured share (the worst share in units of the noise, times 2, rounded up).
# strain_dense: correct but noisier by this statistic.  Its worst case, 97of97, measured 6.85 noise_rms (1.71 of the K = 4 bound) and
# 4.93 noise_max.  The strain sum itself is float64 on both paths (k_g_xyz, k_g_strain_mol: epnn_grad_xyz.hip.h) over the same gE
# whose gxyz holds 0.34 of its bound in that call; the nine entries of ONE 97-atom cell are six independent numbers, each a sum over
# some 2500 pairs in which the float32 rounding of gE (an f32 += across the 3 T sweeps on the dense path) adds up with one sign along
# the diagonal.  Over four cotangents on these atoms the float32 model's own noise_rms ranges 3.2e-7 .. 1.9e-6 and the device's error
# 2.0e-7 .. 1.6e-6 on both paths and at both padded sizes, the ratio 0.2 .. 3.2: the pooled noise of six numbers is a poor yardstick,
# not the kernel a poor sum.  tests/test_grad_noise_ref.py holds every defect model 3 x 14 noise_rms away in this route's cases.
K_OF_ROUTE = {"strain_dense": 14}


def _cases():
    out = []
    for n, _ in gn.SIZES:
        for N in (n, n + 7):
            for route, (_, entry, geom, _, _) in ROUTES.items():
                if N > 96 and route in ROW_FUSED:
                    continue
                out.append(Case(f"{route}-{n}of{N}", route, gn.make_inp(n, N, geom, entry)))
    return out


CASES = _cases()


def outputs_of(route):
    """The outputs of the route's entry that the route checks."""
    outs = gn.ENTRIES[ROUTES[route][1]][1]
    return outs[:1] if route == "multi_k1" else outs


@pytest.fixture(scope="module")
def engines(gpu_engine_factory):
    """One handle for the calls that touch no training state and one that trains; the weights follow the case's input."""
    made = {}

    def get(inp, train):
        if train not in made:
            made[train] = [gpu_engine_factory(nx=gn.NX, T=gn.T, h_dim=gn.H_DIM, e_dim=gn.H_DIM), None]
        eng, has = made[train]
        if has != inp:
            eng.set_weights(gn.weights(inp))
            if train:
                eng.train_init()
            made[train][1] = inp
        return eng

    yield get
    for eng, _ in made.values():
        for name, value in DEFAULTS.items():
            eng.set_option(name, value)


def _listed_pairs(inp):
    return sum(len(cell_ref.pairs_cell(xyz, gn.cell_of(inp), cutoff=gn.CUTOFF)[0]) for xyz, _, _ in gn.molecules(inp))


def _run(eng, case):
    """{output: array} of the case's call, with last_stats() held to the route."""
    _, entry, geom, options, shows = ROUTES[case.route]
    inp = case.inp
    off, xyz, x, Q = gn.batch(inp)
    g, y, v, strain, dQ = gn.tangents(inp)
    A = int(off[-1])
    where = {"open": {}, "box": {"box": gn.BOX}, "cell": {"cell": gn.CELL}}[geom]
    for name, value in dict(DEFAULTS, **options).items():
        eng.set_option(name, value)
    try:
        if shows == DENSE:                                # a forward first: the dense derivative paths leave its counters alone
            eng.forward_xyz(off, xyz, x, Q, N=inp.N, **where)
            before = eng.last_stats()
            assert before[1] + before[2] == inp.count
        if entry == "vjp":
            out = {"gxyz": eng.charges_vjp_xyz(off, xyz, x, Q, g, inp.N, **where)[1]}
        elif entry == "strain":
            out = {"strain": eng.charges_vjp_xyz(off, xyz, x, Q, g, inp.N, cell=gn.CELL, strain=True)[2]}
        elif entry.startswith("jvp_"):
            c = ("jvp_v", "jvp_strain", "jvp_dQ", "jvp_all").index(entry)
            out = {"tq": eng.charges_jvp_xyz(off, xyz, x, Q, inp.N, v=v[c] if v[c].any() else None, strain=strain[c] if strain[c].any() else None,
                                             dQ=float(dQ[c]) if dQ[c] != 0 else None, **where)[1]}
        elif entry == "multi":
            if case.route == "multi_k1":
                tq = eng.charges_jvp_xyz_multi(off, xyz, x, Q, inp.N, v=v[:1])[1]
            else:
                tq = eng.charges_jvp_xyz_multi(off, xyz, x, Q, inp.N, v=v, strain=strain, dQ=dQ)[1]
            assert tq.shape == (len(outputs_of(case.route)), A)
            out = {f"tq{k}": tq[k] for k in range(tq.shape[0])}
        elif entry == "coulomb":
            out = {"fq": eng.coulomb_xyz(off, xyz, x, Q, inp.N, ke=gn.KE, alpha=gn.ALPHA, parts=True)[5]}
        elif entry == "coulomb_cell":
            res = eng.coulomb_xyz_cell(off, xyz, x, Q, inp.N, cell=gn.CELL, ke=gn.KE, alpha=gn.ALPHA, parts=True, strain=True,
                                       ewald=ewald_ref.ewald_params64(gn.CELL, gn.ALPHA, gn.EWALD_TOL))
            out = {"fq": res[6], "gs_q": res[8]}
        else:
            cell = None if case.route in ("train_fused", "train_layers") else gn.cell_of(inp)
            eng.train_step_xyz(off, xyz, x, Q, y, inp.N, apply=False, cell=cell)
            grads = eng.get_gradients()
            out = {f"layer{k}": grads[a:a + s] for k, (a, s) in enumerate(gn.train_layers(gn.weights(inp)))}
            out["all"] = grads
        st = eng.last_stats()
        if shows == DENSE:
            assert np.array_equal(st, before), (case.id, before, st)
        else:
            assert st[0] == _listed_pairs(inp) and st[1] == 0 and st[2] > 0, (case.id, st, _listed_pairs(inp))
    finally:
        for name, value in DEFAULTS.items():
            eng.set_option(name, value)
    return out


def test_the_cases_are_what_they_say():
    """(no GPU) every route has cases at every size it takes, every case a known route, an input of its geometry and about 100 atoms."""
    assert {c.route for c in CASES} == set(ROUTES) and len({c.id for c in CASES}) == len(CASES)
    for route in ROUTES:
        sizes = {(c.inp.n, c.inp.N) for c in CASES if c.route == route}
        want = {(n, N) for n, _ in gn.SIZES for N in (n, n + 7) if not (N > 96 and route in ROW_FUSED)}
        assert sizes == want, route
    for c in CASES:
        _, entry, geom, options, _ = ROUTES[c.route]
        assert c.inp.geom == geom and geom in gn.ENTRIES[entry][0] and set(options) <= set(DEFAULTS)
        assert 96 <= c.inp.n * c.inp.count <= 128, c.id
    from epnn_amd.engine import KE_EV_ANGSTROM
    assert KE_EV_ANGSTROM == gn.KE
    assert gn.MULTI_K == 16 and abs(cell_ref.widths(gn.CELL).min() - 2 * gn.CUTOFF) < 1e-4 and cell_ref.widths(gn.CELL).min() >= 2 * gn.CUTOFF


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_derivatives_within_float32_noise(engines, case):
    entry = ROUTES[case.route][1]
    ref64, noise = gn.reference(case.inp, entry, "64"), gn.noise(case.inp, entry)
    out = _run(engines(case.inp, entry == "train"), case)
    k = K_OF_ROUTE.get(case.route, K)
    failed = []
    for name in outputs_of(case.route):
        dev, ref = np.asarray(out[name], dtype=np.float64), ref64[name]
        noise_rms, noise_max, _ = noise[name]
        assert dev.shape == ref.shape and np.isfinite(dev).all(), (case.id, name)
        err_rms, err_max = gn.rms(dev - ref), float(np.abs(dev - ref).max())
        if noise_max == 0:
            assert not ref.any() and not dev.any(), (case.id, name)            # structurally zero: exactly zero on the device
            continue
        print(f"GRADGRADE {case.id} {name}: rms {err_rms:.2e} = {err_rms / (k * noise_rms):.3f} of {k} x {noise_rms:.2e}; "
              f"max {err_max:.2e} = {err_max / (k * noise_max):.3f} of {k} x {noise_max:.2e}")
        if err_rms > k * noise_rms or (name != "all" and err_max > k * noise_max):
            failed.append((name, err_rms, noise_rms, err_max, noise_max))
    assert not failed, (case.id, failed)
