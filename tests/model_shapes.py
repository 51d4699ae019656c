"""Model shapes other than nx = 9 / 10 and T = 2 / 3 / 5: the (nx, T) pairs the tests use, inputs that exist for every nx, the chosen
seeds, and the conditions that make an input a usable case.  Test helper; NumPy and the float64 references only.

SHAPES holds every nx that epnn_create takes (1..10) once, with T in {1, 4, 6, 7, 8} (2, 3 and 5 run elsewhere), both parities of T
and of nx, and nx = 1..3, 4..7 and 8..10 with their 13, 14 and 15 K-steps of the fused training kernel.  No pair had to be swapped:
every shape has a usable case of every kind.

Features.  nx = 1: the one column is the atomic number.  nx >= 2: the element number in column 0 and a one-hot in columns 1..nx-1,
drawn as tests/test_gpu_grad_large._features draws them, after which atom k < min(n, nx - 1) takes the one-hot column nx - 1 - k:
column 0 and column nx - 1 are non-zero in every molecule, and every column is in every molecule of at least nx - 1 atoms (a
two-atom molecule cannot fill ten columns).  At nx = 2 the one-hot has a single column and today's rule would make every atom the
same hydrogen (the EPN's antisymmetric transfer then cancels every x term exactly): there column 0 draws its own element numbers.

A case is usable when (asserted on the references alone, before the device is consulted)
  forward     the float32 oracle stays within NOISE = 2.5e-6 of the float64 one (the comparison keeps TOL = 1e-5, nothing added);
              the last step matters: the reference at T differs by more than 100 TOL from the same weights cut to T - 1 steps (T = 1:
              from the initial charges Q / n); column 0 and column nx - 1 of x matter: zeroing either moves the reference by more
              than 100 TOL;
  derivative  at least 70 % of the components (gxyz, gstrain) or atoms (tq) have a ReLU-kink bracket (TAU = 2e-5) of at most
              2e-4 max |ref|; the same three sensitivities, measured over the components inside the bracket against their largest
              bound 4e-4 max |ref| (edge_constants.assert_derivative_case's "tight" figure), each above 100.  At T = 1 the model cut
              to no step has q = Q / n: gxyz = 0, gstrain = 0, tq = dQ / n;
  training    the rows of x in every first-layer weight gradient are non-zero in the oracle, and the last step's tensors too.

The seeds below come from an offline scan of the references on the CPU (weight seeds 5..11, scale 0.35 or 0.6, molecule seeds
40..45); the figures they measure are listed in tests/test_gpu_model_shapes.py.  The Coulomb call's cases (COULOMB) take the open case's
seeds where those are usable for fq as well, which they are for every shape but nx = 4, T = 7 (69 % of the components inside the
bracket, 70 % asked); that one takes the scan's first usable entry.
"""
from __future__ import annotations

import functools

import numpy as np

import cell_ref
import edge_constants as ec
import jvp_ref
from conftest import random_weights
from coulomb_ref import coulomb_forces64
from oracle import epnn_oracle as orc
from xyz_grad_ref import vjp64

SHAPES = [(1, 8), (2, 1), (3, 6), (4, 7), (5, 4), (6, 8), (7, 1), (8, 6), (9, 7), (10, 8)]           # (nx, T)
IDS = [f"nx{nx}-T{T}" for nx, T in SHAPES]

TOL = 1e-5           # forward: tests/test_gpu_parity.py
NOISE = 2.5e-6       # float32 oracle against the float64 one
TAU = 2e-5           # ReLU-kink bracket of the derivative references
ZERO = np.zeros((3, 3), np.float32)
BOX = np.float32([7.5, 7.0, 7.2])
SHEARED = np.float32([[8, 0, 0], [2.5, 7.8, 0], [-2, 1.5, 7.6]])                                   # widths 7.27, 7.65, 7.60
CUBIC = np.diag(np.float32([6.5, 6.5, 6.5]))
ELEMENTS = np.array([1, 6, 7, 8, 9, 15, 16, 17, 35])

# ---- the chosen seeds (offline scan; what they measure: the docstring of tests/test_gpu_model_shapes.py)
# forward: (weight seed, scale) for the batches at N = 32 and N = 64 and the 150-atom molecule
FORWARD = {(1, 8): (17, 0.25), (2, 1): (18, 0.35), (3, 6): (17, 0.35), (4, 7): (17, 0.35), (5, 4): (17, 0.35),
           (6, 8): (17, 0.35), (7, 1): (17, 0.35), (8, 6): (17, 0.35), (9, 7): (17, 0.35), (10, 8): (18, 0.3)}
# derivatives, open molecule of 17 atoms at N = 24: (weight seed, scale, molecule seed); also the forward-mode case
OPEN = {(1, 8): (8, 0.6, 43), (2, 1): (5, 0.6, 44), (3, 6): (9, 0.35, 42), (4, 7): (5, 0.6, 40), (5, 4): (7, 0.6, 40),
        (6, 8): (6, 0.6, 43), (7, 1): (5, 0.6, 42), (8, 6): (7, 0.6, 42), (9, 7): (5, 0.6, 43), (10, 8): (6, 0.6, 43)}
# forward mode, the same sizes with v, strain and dQ together: (weight seed, scale, molecule seed)
JVP = {(1, 8): (5, 0.6, 40), (2, 1): (5, 0.6, 45), (3, 6): (9, 0.35, 42), (4, 7): (8, 0.35, 45), (5, 4): (7, 0.6, 40),
       (6, 8): (6, 0.6, 43), (7, 1): (5, 0.6, 42), (8, 6): (8, 0.6, 45), (9, 7): (5, 0.6, 43), (10, 8): (6, 0.6, 43)}
# derivatives, a second open molecule of 33 atoms at N = 40 (more than one 16-row tile) for an even and two odd nx, nx = 1 among them
OPEN_LARGE = {(1, 8): (6, 0.6, 44), (5, 4): (7, 0.6, 40), (8, 6): (6, 0.6, 44)}
JVP_LARGE = {(1, 8): (9, 0.6, 43), (5, 4): (9, 0.6, 42), (8, 6): (6, 0.6, 44)}
# derivatives with strain=True, 20 atoms at N = 24: ("box": np.diag(BOX), or "cell": SHEARED; weight seed, scale, molecule seed)
PERIODIC = {(1, 8): ("box", 7, 0.6, 41), (2, 1): ("cell", 5, 0.6, 42), (3, 6): ("box", 8, 0.6, 43), (4, 7): ("cell", 6, 0.6, 43),
            (5, 4): ("box", 5, 0.6, 40), (6, 8): ("cell", 5, 0.6, 42), (7, 1): ("box", 5, 0.6, 40), (8, 6): ("cell", 5, 0.6, 41),
            (9, 7): ("box", 7, 0.6, 42), (10, 8): ("cell", 5, 0.6, 41)}
# the Coulomb call, the charges' part fq of the forces of the 17-atom open molecule at N = 24 and alpha = 0.3: (weight seed, scale, molecule seed)
COULOMB = {(1, 8): (8, 0.6, 43), (2, 1): (5, 0.6, 44), (3, 6): (9, 0.35, 42), (4, 7): (5, 0.6, 41), (5, 4): (7, 0.6, 40),
           (6, 8): (6, 0.6, 43), (7, 1): (5, 0.6, 42), (8, 6): (7, 0.6, 42), (9, 7): (5, 0.6, 43), (10, 8): (6, 0.6, 43)}
KE = 14.3996454784255
COULOMB_ALPHA = 0.3
# training, 13 atoms open and 24 atoms in CUBIC at N = 24: (weight seed, scale)
TRAIN = {s: (13, 0.4) for s in SHAPES}


# ---------------------------------------------------------------------------------------------------- inputs
def features(rng, n, nx):
    """(x (n, nx) float32, Q) for any nx >= 1 (module docstring)."""
    x = np.zeros((n, nx), dtype=np.float32)
    if nx == 1:
        x[:, 0] = ELEMENTS[rng.integers(0, 9, n)]
        return x, np.float32(rng.integers(-1, 2))
    el = rng.integers(0, nx - 1, n)
    k = np.arange(min(n, nx - 1))
    el[k] = nx - 2 - k
    x[np.arange(n), 1 + el] = 1.0
    x[:, 0] = ELEMENTS[el % 9]
    Q = np.float32(rng.integers(-1, 2))
    if nx == 2:                                        # one one-hot column, one element: column 0 draws its own
        x[:, 0] = ELEMENTS[rng.integers(0, 9, n)]
    return x, Q


def lattice_molecule(n, nx, seed):
    """n atoms on a jittered 1.15 A lattice (no two closer than ~0.9 A), as tests/test_gpu_grad_large._lattice_molecule."""
    rng = np.random.default_rng(seed)
    k = int(np.ceil(n ** (1 / 3)))
    grid = np.array([(a, b, c) for a in range(k) for b in range(k) for c in range(k)], dtype=np.float64)[:n] * 1.15
    xyz = (grid + rng.uniform(-0.1, 0.1, grid.shape)).astype(np.float32)
    return (xyz,) + features(rng, n, nx)


def cell_molecule(n, nx, cell, seed):
    rng = np.random.default_rng(seed)
    return (cell_ref.random_cell(rng, n, cell),) + features(rng, n, nx)


def train_system(n, nx, cell, seed):
    """(xyz, x, Q, y) as tests/test_gpu_train_cell._system: random positions in the cell, or (all-zero cell) a jittered 1.2 A lattice."""
    rng = np.random.default_rng(seed)
    if np.any(cell):
        xyz = cell_ref.random_cell(rng, n, cell)
    else:
        k = int(np.ceil(n ** (1 / 3)))
        grid = np.array([(a, b, c) for a in range(k) for b in range(k) for c in range(k)], dtype=np.float64)[:n] * 1.2
        xyz = (grid + rng.uniform(-0.15, 0.15, grid.shape)).astype(np.float32)
    x, Q = features(rng, n, nx)
    return xyz, x, Q, rng.normal(scale=0.3, size=n).astype(np.float32)


def assert_columns(x, what=""):
    """Column 0 and column nx - 1 are non-zero, and every column where the molecule has the atoms for it."""
    n, nx = x.shape
    used = (x != 0).any(0)
    assert used[0] and used[nx - 1], (what, used)
    assert n < nx - 1 or used.all(), (what, used)


def cut(w):
    """The same weights with the last GNN step and the last EPN step taken away."""
    return {"msg": w["msg"][:-1], "upd": w["upd"], "pas": w["pas"][:-1]}


def without_column(x, k):
    x = x.copy()
    x[:, k] = 0
    return x


# ---------------------------------------------------------------------------------------------------- forward
FORWARD_GROUPS = {"N32": (32, (2, 15, 16, 17, 32)), "N64": (64, (33, 48, 64)), "n150": (150, (150,))}


def forward_conditions(shape, w, mols, N, what):
    """Asserts the forward conditions on the batch; returns (float64 references per molecule, the measured figures)."""
    nx, T = shape
    kw = dict(N=N, dtype=np.float64)
    ref = [orc.forward_xyz(m[0], m[1], m[2], w, **kw) for m in mols]
    cat = np.concatenate([r[:len(m[0])] for r, m in zip(ref, mols)])
    r32 = np.concatenate([orc.forward_xyz(m[0], m[1], m[2], w, N=N, dtype=np.float32)[:len(m[0])] for m in mols])
    if T > 1:
        prev = np.concatenate([orc.forward_xyz(m[0], m[1], m[2], cut(w), **kw)[:len(m[0])] for m in mols])
    else:
        prev = np.concatenate([np.full(len(m[0]), np.float64(np.float32(m[2]) / np.float32(len(m[0])))) for m in mols])
    fig = {"noise": float(np.abs(r32 - cat).max()), "T": float(np.abs(cat - prev).max())}
    for name, k in (("col0", 0), ("col_last", nx - 1)):
        other = np.concatenate([orc.forward_xyz(m[0], without_column(m[1], k), m[2], w, **kw)[:len(m[0])] for m in mols])
        fig[name] = float(np.abs(cat - other).max())
    print(f"{what}: float32 noise {fig['noise']:.1e}; the last step moves q by {fig['T']:.1e}, column 0 by {fig['col0']:.1e}, "
          f"column {nx - 1} by {fig['col_last']:.1e}")
    for m in mols:
        assert_columns(m[1], what)
    assert fig["noise"] <= NOISE, (what, fig)
    assert min(fig["T"], fig["col0"], fig["col_last"]) > 100 * TOL, (what, fig)
    return ref, fig


@functools.lru_cache(maxsize=None)
def forward_case(shape, group):
    """(w, molecules, N, float64 references, figures) of a shape's forward batch: "N32", "N64" or "n150"."""
    nx, T = shape
    seed, scale = FORWARD[shape]
    N, ns = FORWARD_GROUPS[group]
    w = random_weights(nx, T, seed=seed, scale=scale)
    mols = [lattice_molecule(n, nx, seed=n) for n in ns]
    ref, fig = forward_conditions(shape, w, mols, N, f"nx = {nx}, T = {T}, forward {group}")
    return w, mols, N, ref, fig


# ---------------------------------------------------------------------------------------------------- derivatives
def derivative_conditions(shape, fn, zero, what):
    """fn(w, x, kink_shift) -> tuple of arrays (each a derivative with one bracket per component); zero: the same tuple for the
    model cut to no step (T = 1).  Asserts the kink rule and the three sensitivities per array; returns (at, (lo, hi), kink, figures)."""
    nx, T = shape
    w, x = fn.w, fn.x
    at, lo, hi = fn(w, x, 0.0), fn(w, x, +TAU), fn(w, x, -TAU)
    prev = fn(cut(w), x, 0.0) if T > 1 else zero
    others = {"T": prev, "col0": fn(w, without_column(x, 0), 0.0), "col_last": fn(w, without_column(x, nx - 1), 0.0)}
    kink = [np.abs(a - b) for a, b in zip(lo, hi)]
    figs = []
    for k in range(len(at)):
        fig = {}
        for name, other in others.items():
            fig[name] = ec.assert_derivative_case(at[k], kink[k], other[k], f"{what} [{k}] against {name}")[1]
        fig["share"], fig["worst"] = ec.kink_share(at[k], kink[k])
        assert min(fig["T"], fig["col0"], fig["col_last"]) > 100, (what, k, fig)
        figs.append(fig)
    return at, (lo, hi), kink, figs


class _Fn:
    def __init__(self, w, x, call):
        self.w, self.x, self.call = w, x, call

    def __call__(self, w, x, shift):
        return self.call(w, x, shift)


def cotangent(n):
    """test_gpu_grad_large._check's g (seed 0), float32."""
    return np.random.default_rng(0).normal(size=n).astype(np.float32)


def _open_tables(size, jvp=False):
    return ((JVP if jvp else OPEN), 17, 24) if size == "small" else ((JVP_LARGE if jvp else OPEN_LARGE), 33, 40)


@functools.lru_cache(maxsize=None)
def open_case(shape, size="small"):
    """(w, molecule, N, g, q, gxyz, kink per component, (gxyz at +TAU, at -TAU), figures) of a shape's open gradient case, against vjp64."""
    nx, T = shape
    table, n, N = _open_tables(size)
    wseed, scale, mseed = table[shape]
    w = random_weights(nx, T, seed=wseed, scale=scale)
    mol = lattice_molecule(n, nx, seed=mseed)
    assert_columns(mol[1])
    g = cotangent(n)
    g64 = g.astype(np.float64)
    q = vjp64(mol[0], mol[1], mol[2], g64, w, N=N)[0]
    fn = _Fn(w, mol[1], lambda w_, x_, s: (vjp64(mol[0], x_, mol[2], g64, w_, N=N, kink_shift=s)[1],))
    at, (lo, hi), kink, figs = derivative_conditions(shape, fn, (np.zeros((n, 3)),), f"nx = {nx}, T = {T}, open ({n}, {N}) gxyz")
    return w, mol, N, g, q, at[0], kink[0], (lo[0], hi[0]), figs[0]


@functools.lru_cache(maxsize=None)
def coulomb_case(shape):
    """(w, molecule, N, q, phi, fq, kink per component, (fq at +TAU, at -TAU), figures) of a shape's case of the Coulomb call against
    coulomb_forces64 at alpha = COULOMB_ALPHA: fq = -vjp64(g = phi of the reference's own charges), the part of the forces that goes
    through dq/dxyz.  The model cut by a step, or without a column of x, has other charges and another phi as well."""
    nx, T = shape
    wseed, scale, mseed = COULOMB[shape]
    n, N = 17, 24
    w = random_weights(nx, T, seed=wseed, scale=scale)
    mol = lattice_molecule(n, nx, seed=mseed)
    assert_columns(mol[1])
    q, phi = coulomb_forces64(mol[0], mol[1], mol[2], w, N, KE, COULOMB_ALPHA)[:2]
    fn = _Fn(w, mol[1], lambda w_, x_, s: (coulomb_forces64(mol[0], x_, mol[2], w_, N, KE, COULOMB_ALPHA, kink_shift=s)[5],))
    at, (lo, hi), kink, figs = derivative_conditions(shape, fn, (np.zeros((n, 3)),), f"nx = {nx}, T = {T}, coulomb ({n}, {N}) fq")
    return w, mol, N, q, phi, at[0], kink[0], (lo[0], hi[0]), figs[0]


@functools.lru_cache(maxsize=None)
def periodic_case(shape):
    """(w, molecule, N, cell, g, q, gxyz, gstrain, kink of gxyz, kink of gstrain, ((gxyz, gstrain) at +TAU, at -TAU), figures of
    both) against strain64."""
    nx, T = shape
    kind, wseed, scale, mseed = PERIODIC[shape]
    cell = np.diag(BOX).astype(np.float32) if kind == "box" else SHEARED
    n, N = 20, 24
    w = random_weights(nx, T, seed=wseed, scale=scale)
    mol = cell_molecule(n, nx, cell, mseed)
    assert_columns(mol[1])
    g = cotangent(n)
    g64 = g.astype(np.float64)
    q = cell_ref.strain64(mol[0], mol[1], mol[2], g64, cell, w, N=N)[0]
    fn = _Fn(w, mol[1], lambda w_, x_, s: cell_ref.strain64(mol[0], x_, mol[2], g64, cell, w_, N=N, kink_shift=s)[1:])
    at, shifted, kink, figs = derivative_conditions(shape, fn, (np.zeros((n, 3)), np.zeros((3, 3))), f"nx = {nx}, T = {T}, {kind} gxyz / gstrain")
    return w, mol, N, cell, g, q, at[0], at[1], kink[0], kink[1], shifted, figs


def tangents(n, seed):
    """v (n, 3) ~ N(0, 1), strain (3, 3) ~ 0.3 N(0, 1), dQ ~ N(0, 1), float32: the three kinds together."""
    rng = np.random.default_rng(seed)
    return {"v": rng.normal(size=(n, 3)).astype(np.float32), "strain": (0.3 * rng.normal(size=(3, 3))).astype(np.float32),
            "dQ": np.float32(rng.normal())}


@functools.lru_cache(maxsize=None)
def jvp_case(shape, size="small"):
    """(w, molecule, N, tangents, q, tq, kink per atom, figures) of a lattice molecule with v, strain and dQ together, against jvp64."""
    nx, T = shape
    table, n, N = _open_tables(size, jvp=True)
    wseed, scale, mseed = table[shape]
    w = random_weights(nx, T, seed=wseed, scale=scale)
    mol = lattice_molecule(n, nx, seed=mseed)
    assert_columns(mol[1])
    tan = tangents(n, 100 + n)
    kw = dict(N=N, v=tan["v"], strain=tan["strain"], dQ=float(tan["dQ"]))
    q = jvp_ref.jvp64(mol[0], mol[1], mol[2], w, **kw)[0]
    fn = _Fn(w, mol[1], lambda w_, x_, s: (jvp_ref.jvp64(mol[0], x_, mol[2], w_, kink_shift=s, **kw)[1],))
    at, _, kink, figs = derivative_conditions(shape, fn, (np.full(n, float(tan["dQ"]) / n),), f"nx = {nx}, T = {T}, open ({n}, {N}) tq")
    return w, mol, N, tan, q, at[0], kink[0], figs[0]


# ---------------------------------------------------------------------------------------------------- training
def x_rows(nx, h_dim=48):
    """Rows of a first-layer kernel [x_i | h_i | q_i, x_j | h_j | q_j, e] that multiply x: 0..nx-1 and F..F+nx-1."""
    F = nx + h_dim + 1
    return np.concatenate([np.arange(nx), F + np.arange(nx)])


@functools.lru_cache(maxsize=None)
def train_case(shape):
    """(w, systems, cells, N) of a shape's training batch: 13 atoms open and 24 atoms in CUBIC, N = 24."""
    nx, T = shape
    wseed, scale = TRAIN[shape]
    w = random_weights(nx, T, seed=wseed, scale=scale)
    cells = [ZERO, CUBIC]
    mols = [train_system(13, nx, ZERO, seed=28), train_system(24, nx, CUBIC, seed=170)]
    for m in mols:
        assert_columns(m[1])
    return w, mols, cells, 24


def train_conditions(shape, grads, what=""):
    """On the oracle's gradient dict: the rows of x in msg[t][0] and pas[t][0] are non-zero for every t (each half, each column where
    the batch has it), and so are all tensors of the last step.  Returns the smallest x-row maximum over the largest entry."""
    nx, T = shape
    least = np.inf
    for t in range(T):
        for part in ("msg", "pas"):
            W = np.asarray(grads[part][t][0][0])
            rows = np.abs(W[x_rows(nx)]).max(1)
            assert (rows > 0).all(), (what, part, t, rows)
            least = min(least, float(rows.min() / np.abs(W).max()))
    for part in ("msg", "pas"):
        for W, b in grads[part][T - 1]:
            assert np.abs(W).max() > 0, (what, part)
    print(f"{what}: the smallest x row of a first-layer gradient is {least:.1e} of its tensor's largest entry")
    return least
