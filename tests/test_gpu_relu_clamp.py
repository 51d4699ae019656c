"""The two forms of the pair MLPs' first ReLU in the fused kernel of the compact entry (k_wave_forward<true, true, true, 2, CLAMP>,
epnn_wave.hip.h; option "relu_clamp", include/epnn_dev.h): the add's output clamp on scaled packs against v_max_f32 on the unscaled ones.

One molecule of each size at which the kernel takes another path, each a batch of its own on one wavefront ("wave2" 0):
    n = 3    smallest                      n = 19   5 copies in block 1, not a power of two
    n = 16   block 0 full                  n = 25   G rows through HBM
    n = 17   16 copies in block 1          n = 32   both blocks full
with decay_model_weights on the element rows they were trained on (tests/test_gpu_rem4x4.py says why).
(a) the two forms give the same bits; (b) both within the float32-grade bound of tests/test_gpu_f32_grade.py against the float64
oracle (its K times the float32 oracle's noise, rms and max, and the standing 1e-5); (c) feature rows scaled up until the scaled
projections leave the clamp's range: the call still returns the max form's bits (finite ones), and epnn_last_stats out[3] says that
a wavefront left the clamp form.  The pack scaling itself, without a GPU: tests/test_relu_clamp_ref.py."""
import os

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_f32_grade import CHARGES, K, TOL, _batch, _cluster, rms

SIZES = (3, 16, 17, 19, 25, 32)
NX, T, N = 9, 5, 34
_CACHE = {}


def _weights():
    if "w" not in _CACHE:
        from epnn_amd import checkpoint
        _CACHE["w"] = checkpoint.load_epnn_weights(os.path.join(ROOT, "models", "decay_model_weights"))
    return _CACHE["w"]


def _molecules():
    """[(xyz, x, Q)]: clusters of test_gpu_f32_grade's density, element rows (atomic number, one-hot of H C N O) as the reference builds them."""
    if "mols" not in _CACHE:
        mols = []
        for k, n in enumerate(SIZES):
            rng = np.random.default_rng(2300 + n)
            xyz = _cluster(rng, n)
            z = rng.choice(4, size=n, p=[0.5, 0.3, 0.1, 0.1])
            x = np.zeros((n, NX), dtype=np.float32)
            x[:, 0] = np.array([1.0, 6.0, 7.0, 8.0], dtype=np.float32)[z]
            x[np.arange(n), 1 + z] = 1.0
            mols.append((xyz, x, float(np.float32(CHARGES[k % 3] * (1.0 if n >= 5 else n / 6.0)))))
        _CACHE["mols"] = mols
    return _CACHE["mols"]


def _references():
    """(q64, q32) per molecule: the float64 and the float32 oracle, once and read-only."""
    if "ref" not in _CACHE:
        from oracle import epnn_oracle as orc
        mols = _molecules()
        dense = [orc.dense_inputs(xyz, x, np.float32(Q), N) for xyz, x, Q in mols]
        stacked = [np.stack([d[k] for d in dense]) for k in range(5)]
        refs = []
        for dtype in (np.float64, np.float32):
            out = orc.model_forward(*stacked, _weights(), dtype)
            qs = [out[b, :len(m[0]), 0].astype(np.float64) for b, m in enumerate(mols)]
            for q in qs:
                assert np.isfinite(q).all()
                q.setflags(write=False)
            refs.append(qs)
        _CACHE["ref"] = tuple(refs)
    return _CACHE["ref"]


def _engine():
    from epnn_amd.engine import Engine
    eng = Engine(nx=NX, T=T)
    eng.set_weights(_weights())
    eng.set_option("wave2", 0)              # one wavefront per molecule: k_wave_forward
    return eng


def _both_forms(eng, mol):
    """q of the clamp form, q of the max form, wavefront-left-the-clamp-form reports of the clamp call."""
    off, xyz, x, Q = _batch([mol])
    out = []
    for form in (1, 0):
        eng.set_option("relu_clamp", form)
        before = int(eng.last_stats()[3])
        q = eng.forward_xyz(off, xyz, x, Q, N=N)
        st = eng.last_stats()
        assert (st[1], st[2]) == (1, 0), st
        out.append((q, int(st[3]) - before))
    (qc, left), (qm, left_max) = out
    assert left_max == 0                     # the max form has nothing to report
    return qc, qm, left


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(SIZES)), ids=[f"n{n}" for n in SIZES])
def test_clamp_form_gives_the_max_form_s_bits_within_float32_noise(k):
    mol = _molecules()[k]
    q64, q32 = _references()[0][k], _references()[1][k]
    noise_rms, noise_max = rms(q32 - q64), float(np.abs(q32 - q64).max())
    assert 0.0 < noise_rms and 0.0 < noise_max
    eng = _engine()
    try:
        qc, qm, left = _both_forms(eng, mol)
    finally:
        eng.close()
    assert left == 0, "sane inputs stay in the clamp's range"
    assert qc.shape == q64.shape and np.isfinite(qc).all() and np.isfinite(qm).all()
    for form, q in (("clamp", qc), ("max", qm)):
        err_rms, err_max = rms(q - q64), float(np.abs(q - q64).max())
        print(f"RELU_CLAMP n = {SIZES[k]} [{form}]: rms {err_rms:.2e} = {err_rms / (K * noise_rms):.3f} of {K} x {noise_rms:.2e}; "
              f"max {err_max:.2e} = {err_max / (K * noise_max):.3f} of {K} x {noise_max:.2e}")
        assert err_rms <= K * noise_rms, (SIZES[k], form, err_rms, noise_rms)
        assert err_max <= min(K * noise_max, TOL), (SIZES[k], form, err_max, noise_max)
    assert np.array_equal(qc.view(np.uint32), qm.view(np.uint32)), (SIZES[k], float(np.abs(qc - qm).max()))


@pytest.mark.gpu
def test_rows_beyond_the_clamp_s_range_run_the_max_form_and_say_so():
    """Feature rows times 2^20, 2^24, ... until a wavefront reports that it left the clamp form (the scaled projections beyond
    relu_lim): from there on, too, the call's bits are the max form's, and they are finite.  No oracle is asked at these magnitudes."""
    xyz, x, Q = _molecules()[SIZES.index(19)]
    eng = _engine()
    try:
        tripped = None
        for e in range(20, 44, 4):
            big = (xyz, (x * np.float32(2.0 ** e)).astype(np.float32), Q)
            qc, qm, left = _both_forms(eng, big)
            print(f"RELU_CLAMP features x 2^{e}: reports {left}, largest |q| {np.abs(qm).max():.3e}, finite {np.isfinite(qm).all()}")
            assert np.isfinite(qc).all() and np.isfinite(qm).all(), e
            assert np.array_equal(qc.view(np.uint32), qm.view(np.uint32)), (e, left)
            if left:
                tripped = e
                break
        assert tripped is not None, "no scale up to 2^40 left the clamp's range"
    finally:
        eng.close()
