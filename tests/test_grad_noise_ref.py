"""The derivative bound of tests/test_gpu_grad_f32_grade.py is meaningful: decided here, on the CPU, for every case of that file.

Per (input, entry) of its cases (tests/grad_noise_ref.py has the inputs, the references and the defect models):

  * no ReLU decision within reach of float32 noise: min |z64| >= 8 max |z32 - z64| over every ReLU pre-activation of the input's
    float64 forward (rows of padded partners and both row orders of the pass network included), and the reference with its ReLU
    decisions shifted by +tau and by -tau returns the bits of the unshifted one.  tau is 0.99 of that min |z64|, not the minimum
    itself: relu'(z) = [z > tau] differs from [z > 0] at z == tau, and the training oracle rounds the edge tensor to float32 before its
    first Dense, which moves its z by 1e-7 against the z measured here;
  * the noise of every output, noise_rms = rms(ref32 - ref64) and noise_max = max |ref32 - ref64|; an output with no noise is
    structurally zero in both;
  * never looser than today: K noise_max <= 2e-4 max |ref64| for every output;
  * defect separation: the reference with (a) gE, (b) te, (c) the backward or tangent Dense operands of one MLP family cut to 16
    mantissa bits lies at least 3 k noise_rms from float64 in at least one output the case asserts (k the largest factor of the
    routes that use the entry: a defect fails a case as soon as one output leaves its bound; a message defect cannot show in the pass
    network's weight gradients).  The float32 model itself lies 1 noise_rms from float64 by definition, the float64 reference 0.

The table of shares is printed (run with -s); with EPNN_TEST_VERBOSE the per-layer variants of (c) as well, which are not asserted."""
import os

import numpy as np
import pytest

import grad_noise_ref as gn
import test_gpu_grad_f32_grade as gpu

PAIRS = sorted({(c.inp, gpu.ROUTES[c.route][1]) for c in gpu.CASES}, key=lambda p: (p[0].n, p[0].N, p[0].geom, p[1]))
INPUTS = sorted({p[0] for p in PAIRS})


def _factor(inp, entry):
    return max(gpu.K_OF_ROUTE.get(c.route, gpu.K) for c in gpu.CASES if c.inp == inp and gpu.ROUTES[c.route][1] == entry)


def _outputs(inp, entry):
    outs = set()
    for c in gpu.CASES:
        if c.inp == inp and gpu.ROUTES[c.route][1] == entry:
            outs |= set(gpu.outputs_of(c.route))
    return [o for o in gn.ENTRIES[entry][1] if o in outs]


def _margin(inp):
    key = ("margin",) + tuple(inp)
    if key not in gn._CACHE:
        gn._CACHE[key] = gn.kink_margin(inp, gn.weights(inp))
    return gn._CACHE[key]


@pytest.mark.parametrize("inp", INPUTS, ids=["-".join(str(v) for v in i) for i in INPUTS])
def test_no_relu_decision_within_reach_of_float32_noise(inp):
    zmin, dz = _margin(inp)
    print(f"KINK {tuple(inp)}: min |z64| {zmin:.2e}, max |z32 - z64| {dz:.2e}, ratio {zmin / dz:.1f}")
    assert zmin >= 8 * dz, (inp, zmin, dz)
    base = gn.random_weights(gn.NX, gn.T, seed=inp.seed, scale=inp.scale)
    w = gn.weights(inp)
    # kernels as they were, only biases moved -- by 1e-5 .. 1e-3 up to 33 atoms and by up to 0.29 beyond (biases are drawn from +-0.1): a
    # column of a pair MLP holds 10^4 rows there, and a window of three margins free of all of them lies far from where the bias was.  The
    # bound is the reach of nudged_weights' own search for a window, far inside the spread of the pre-activations themselves (order 1)
    moved = 0.0
    for m0, m1 in zip([base["upd"]] + base["msg"] + base["pas"], [w["upd"]] + w["msg"] + w["pas"]):
        for (W0, b0), (W1, b1) in zip(m0, m1):
            assert np.array_equal(W0, W1)
            moved = max(moved, float(np.abs(b0 - b1).max()))
    print(f"    largest bias nudge {moved:.1e}")
    assert moved <= 0.5


@pytest.mark.parametrize("inp,entry", PAIRS, ids=[f"{e}-{i.n}of{i.N}-{i.geom}" for i, e in PAIRS])
def test_bound_is_tight_and_separates_the_defects(inp, entry):
    tau = 0.99 * _margin(inp)[0]
    outs = _outputs(inp, entry)
    ref64, noise = gn.reference(inp, entry, "64"), gn.noise(inp, entry)
    for model in ("+tau", "-tau"):
        shifted = gn.reference(inp, entry, model, tau)
        for o in outs:
            assert np.array_equal(shifted[o], ref64[o]), (inp, entry, model, o)
    k = _factor(inp, entry)
    defects = gn.ENTRIES[entry][2]
    shares = {d: {} for d in defects}
    lines = []
    for o in outs:
        noise_rms, noise_max, top = noise[o]
        if noise_max == 0:
            assert not ref64[o].any(), (inp, entry, o)                       # no noise: structurally zero, and the GPU test wants exact zeros
            continue
        assert top > 0 and k * noise_max <= 2e-4 * top, (inp, entry, o, noise_max, top)
        assert gn.rms(gn.reference(inp, entry, "32")[o] - ref64[o]) <= noise_rms
        for d in defects:
            shares[d][o] = gn.rms(gn.reference(inp, entry, d)[o] - ref64[o]) / (k * noise_rms)
        lines.append(f"    {o:8s} noise_rms {noise_rms:.2e} noise_max {noise_max:.2e} = {k * noise_max / top:.1e} max|ref64|;  shares of {k} noise_rms: float64 0, "
                     f"float32 model {1 / k:.2f}, " + ", ".join(f"{d} {shares[d][o]:.1f}" for d in defects))
        if os.environ.get("EPNN_TEST_VERBOSE") and defects:
            per = [f"{f}.{l} {gn.rms(gn.reference(inp, entry, f'{f}.{l}')[o] - ref64[o]) / (k * noise_rms):.1f}" for f in gn.FAMILIES for l in range(3)]
            lines.append("             one layer's operands cut: " + ", ".join(per))
    print(f"NOISE {entry} {tuple(inp)}: kink margin {_margin(inp)[0]:.2e}\n" + "\n".join(lines))
    for d in defects:
        best = max(shares[d].values())
        assert best >= 3, (inp, entry, d, best, shares[d])
