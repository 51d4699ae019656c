"""The three-piece split by itself, and what the bound of tests/test_gpu_f32_grade.py can see (CPU, NumPy only).

(a) the split is exact for |x| >= 2^-100 and every piece is a bf16 number; (b) the six-product sum of one Dense is within
2.01 * 2^-24 * sum_k |x_k| |w_k| of the exact product; (c) for the inputs of EVERY case of test_gpu_f32_grade.py, on the references
alone: the six-product model is at most 0.5 noise_rms from the float64 oracle, every defect model (two pieces; each of the six partial
products left out) at least 3 * K * noise_rms, and K * noise_max <= 1e-5 -- noise being the float32 oracle against the float64 one.
A case whose inputs do not give that separation gets other inputs, never a wider bound."""
import numpy as np
import pytest

import split_ref
import test_gpu_f32_grade as grade


def _operands(rng, shape, lo=0.05, hi=1.0):
    a = (rng.uniform(lo, hi, size=shape) * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32)
    a.view(np.uint32)[...] |= 0x101                       # bits in the second and in the third piece of every value
    return a


def test_three_pieces_add_up_exactly_and_each_is_a_bf16():
    rng = np.random.default_rng(0)
    x = np.concatenate([_operands(rng, 20000), (rng.normal(size=20000) * 10.0 ** rng.uniform(-25, 25, 20000)).astype(np.float32),
                        np.float32([2.0 ** -100, -2.0 ** -100, 2.0 ** -100 * (1 + 2.0 ** -23), 3.4e38, 1.0, 0.0, -0.0, 1 + 2.0 ** -23])])
    x = x[(np.abs(x) >= np.float32(2.0 ** -100)) | (x == 0)]
    p = split_ref.pieces(x)
    assert len(p) == 3
    for piece in p:
        assert piece.dtype == np.float32 and np.all(piece.view(np.uint32) & np.uint32(0xFFFF) == 0)       # 16 low bits clear: a bf16
    assert np.array_equal(p[0].astype(np.float64) + p[1].astype(np.float64) + p[2].astype(np.float64), x.astype(np.float64))
    nz = x != 0
    # truncation: a piece keeps 8 significant bits, so what it leaves is below 2^-7 of it (2^-8 on average over random mantissas)
    assert np.all(np.abs(p[1][nz]) < 2.0 ** -7 * np.abs(x[nz])) and np.all(np.abs(p[2][nz]) < 2.0 ** -15 * np.abs(x[nz]))
    # below the range: the third piece of 2^-126 (1 + 2^-23) is a denormal bit that float32 holds but the 16-bit cut of it is zero
    tiny = np.float32([2.0 ** -126 * (1 + 2.0 ** -23)])
    assert sum(q.astype(np.float64) for q in split_ref.pieces(tiny))[0] != float(tiny[0])
    # the test inputs' trick really gives three non-zero pieces
    assert grade.three_pieces(_operands(rng, 1000)) and not grade.three_pieces(np.float32([0.5, 0.7123]))


def test_models_are_what_their_names_say():
    assert len(split_ref.SIX) == 6 and set(split_ref.SIX) == {(1, 1), (1, 2), (2, 1), (1, 3), (2, 2), (3, 1)}
    assert set(split_ref.TWO_PIECES) < set(split_ref.SIX) and len(split_ref.DEFECTS) == 7
    assert sorted(len(k) for k in split_ref.DROP_ONE.values()) == [5] * 6
    assert len({frozenset(k) for k in split_ref.DROP_ONE.values()}) == 6 and all(set(k) < set(split_ref.SIX) for k in split_ref.DROP_ONE.values())
    # all nine products: the exact product of the float32 operands
    rng = np.random.default_rng(1)
    x, w, b = _operands(rng, (7, 32)), _operands(rng, (32, 5)), _operands(rng, 5)
    nine = [(a, c) for a in (1, 2, 3) for c in (1, 2, 3)]
    exact = x.astype(np.float64) @ w.astype(np.float64) + b.astype(np.float64)
    assert np.abs(split_ref.split_dense(x, w, b, nine) - exact).max() <= 1e-15 * np.abs(exact).max()


@pytest.mark.parametrize("k_dim", [16, 32, 80])
def test_six_products_within_the_bound_of_one_product(k_dim):
    """|SIX - exact| <= 2.01 * 2^-24 * sum_k |x_k| |w_k| on random operands: with |x2| ~ 2^-8 |x| and |x3| ~ 2^-16 |x| (and the same
    for w) the omitted x2 w3 + x3 w2 + x3 w3 is about (2 + 2^-8) 2^-24 |x| |w| per term.  (A single term can reach four times that:
    truncation leaves up to 2^-7 and 2^-15, which the test above pins; over the K terms of a product the bound holds with room, and
    it is asserted for every output.)  Every defect model breaks the bound on the same data."""
    rng = np.random.default_rng(10 + k_dim)
    x, w = _operands(rng, (64, k_dim)), _operands(rng, (k_dim, 32), 0.01, 0.5)
    assert grade.three_pieces(x) and grade.three_pieces(w)
    exact = x.astype(np.float64) @ w.astype(np.float64)
    scale = np.abs(x).astype(np.float64) @ np.abs(w).astype(np.float64)
    err = np.abs(split_ref.split_dense(x, w, np.zeros(32), split_ref.SIX) - exact)
    assert np.all(err <= 2.01 * 2.0 ** -24 * scale) and err.max() > 0
    for name, keep in split_ref.DEFECTS.items():
        bad = np.abs(split_ref.split_dense(x, w, np.zeros(32), keep) - exact)
        assert bad.max() > 2.01 * 2.0 ** -24 * scale.flat[np.argmax(bad)], name


def test_swap_is_undone_and_can_be_held_to_one_layer():
    from oracle import epnn_oracle as orc
    saved = orc.mlp
    rng = np.random.default_rng(2)
    rows = _operands(rng, (9, 12)).astype(np.float64)
    layers = [(_operands(rng, (12, 32)), _operands(rng, 32)), (_operands(rng, (32, 32)), _operands(rng, 32)), (_operands(rng, (32, 3)), _operands(rng, 3))]
    layers = orc._cast_layers(layers, np.float64)
    plain = orc.mlp(rows, layers)
    with split_ref.swapped_mlp(split_ref.TWO_PIECES):
        every = orc.mlp(rows, layers)
    with split_ref.swapped_mlp(split_ref.TWO_PIECES, layer=1):
        second = orc.mlp(rows, layers)
    with split_ref.swapped_mlp([(a, c) for a in (1, 2, 3) for c in (1, 2, 3)]):
        nine = orc.mlp(rows, layers)
    assert orc.mlp is saved
    assert np.abs(nine - plain).max() <= 2e-7 * np.abs(plain).max()            # (the hidden activations rounded to float32, no more)
    assert 0 < np.abs(second - plain).max() < np.abs(every - plain).max() < 1e-2
    with pytest.raises(RuntimeError):
        with split_ref.swapped_mlp():
            raise RuntimeError("inside")
    assert orc.mlp is saved


# ---------------------------------------------------------------------------------------------------- (c) what the GPU bound can see
def _model_inputs():
    """(inputs, layer): the distinct inputs of the GPU cases, with the Dense layers their kernels split -- every layer for the fused
    kernels (and for the f32 forwards of the derivative entries, which are held to the same bound), the second alone for the tiled ones."""
    seen = {}
    for c in grade.CASES:
        layer = 1 if grade.ROUTES[c.route][2] == grade.TILED else None
        seen.setdefault((c.inputs, layer), []).append(c.id)
    return list(seen.items())


_MODEL_INPUTS = _model_inputs()


def test_every_gpu_case_is_covered():
    assert {i for (_, _), ids in _MODEL_INPUTS for i in ids} == {c.id for c in grade.CASES}
    assert all(grade.K_OF_ROUTE.get(r, grade.K) >= grade.K for r in grade.ROUTES)


@pytest.mark.parametrize("inp,layer,ids", [(i, l, ids) for (i, l), ids in _MODEL_INPUTS],
                         ids=[ids[0].split("-", 1)[1] + ("-second" if l == 1 else "") for (i, l), ids in _MODEL_INPUTS])
def test_bound_separates_the_design_from_its_defects(inp, layer, ids):
    q64, q32 = grade.references(inp)
    noise_rms, noise_max = grade.rms(q32 - q64), float(np.abs(q32 - q64).max())
    k = max(grade.K_OF_ROUTE.get(c.route, grade.K) for c in grade.CASES if c.id in ids)
    bound = k * noise_rms
    with split_ref.swapped_mlp(split_ref.SIX, layer):
        six = grade.rms(grade.oracle(inp, np.float64) - q64)
    defects = {}
    for name, keep in split_ref.DEFECTS.items():
        with split_ref.swapped_mlp(keep, layer):
            defects[name] = grade.rms(grade.oracle(inp, np.float64) - q64)
    print(f"SEPARATION {ids[0]} (+{len(ids) - 1}): noise rms {noise_rms:.2e} max {noise_max:.2e}; six {six:.2e} = {six / noise_rms:.2f} noise; "
          f"defects {min(defects.values()):.2e} .. {max(defects.values()):.2e} = {min(defects.values()) / bound:.1f} .. {max(defects.values()) / bound:.1f} bounds")
    assert k * noise_max <= grade.TOL, (noise_max, ids)
    assert six <= 0.5 * noise_rms, (six, noise_rms, ids)
    for name, err in defects.items():
        assert err >= 3 * bound, (name, err, bound, ids)
