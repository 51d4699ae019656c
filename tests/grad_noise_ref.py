"""The inputs, references and defect models behind the derivative bound (tests/test_grad_noise_ref.py on the CPU,
tests/test_gpu_grad_f32_grade.py on the GPU). Test helper.

An input (`Inp`) is a batch of `count` molecules of exactly n atoms padded to N, open, in the smallest orthorhombic box or in the
smallest sheared cell the entries accept at cutoff 3.0.  An entry (`ENTRIES`) is one derivative of the charges on that input; its
reference is evaluated under a `model`:

    "64"      the float64 reference (xyz_grad_ref / cell_ref / periodic_ref / jvp_ref / coulomb_ref / ewald_ref / the training oracle)
    "32"      the same code with dtype=np.float32: the float32 model of the device's kernels, whose distance from "64" is the noise
    "+tau", "-tau"   the float64 reference with its ReLU decisions shifted (kink_shift)
    "gE"      float64 with the edge cotangent gE cut to 16 mantissa bits (two bf16 pieces), defect (a)
    "te"      float64 with the edge tangent te cut to 16 mantissa bits, defect (b)
    "msg", "upd", "pas"   float64 with every operand of the backward (or tangent) Dense products of that MLP family cut to 16
              mantissa bits, the dW products included, defect (c); "msg.0" .. "pas.2": one layer of the family only

Every reference is kept once per (input, entry, model) and read-only.  The weights of an input are random_weights(9, 2, seed, scale)
of WEIGHTS_OF with biases nudged (`nudged_weights`) until no ReLU pre-activation of the input's float64 forward lies within 16 times the
float32 model's own error in these pre-activations: the derivative of a ReLU network jumps where one crosses zero, and the bound of
the GPU test has no room for a kink term.
"""
from __future__ import annotations

import collections
import contextlib

import numpy as np

import cell_ref
import coulomb_ref
import ewald_ref
import jvp_ref
import periodic_ref
import xyz_grad_ref as xgr
from conftest import random_weights
from oracle import epnn_oracle as orc
from oracle import epnn_oracle_train as otr

K = 4                       # times the float32 model's noise
NX, T, H_DIM = 9, 2, 48
CUTOFF = 3.0
ALPHA = 0.5                 # of the Coulomb calls
KE = 14.3996454784255       # eV Angstrom / e^2 (engine.KE_EV_ANGSTROM)
EWALD_TOL = 1e-6
MULTI_K = 16                # the largest K of epnn_charges_jvp_multi_xyz_cell (include/epnn.h)
SIZES = ((2, 48), (16, 6), (17, 6), (33, 3), (64, 2), (97, 1))           # (atoms, molecules): about 100 atoms a batch
CHARGES = (0.7123, -1.3371, 0.3001)
# random_weights' (seed, scale) by entry group and molecule size, chosen on the CPU so that every defect model of every case lies
# 3 K noise_rms from float64 (tests/test_grad_noise_ref.py): in small molecules the GNN's share of a derivative grows with the scale,
# in large ones the sums over a hundred partners do, until the activations and with them the float32 noise run away.  The Coulomb
# entries have weights of their own: the noise of fq is mostly that of the charges behind its seed phi, several times the backward's.
WEIGHTS_OF = {("main", 2): (5, 1.0), ("main", 16): (5, 0.8), ("main", 17): (5, 0.8), ("main", 33): (5, 0.7), ("main", 64): (5, 0.6),
              ("main", 97): (5, 0.7),
              ("coulomb", 2): (5, 0.9), ("coulomb", 16): (5, 0.8), ("coulomb", 17): (1, 0.7), ("coulomb", 33): (5, 0.7),
              ("coulomb", 64): (5, 0.6), ("coulomb", 97): (5, 0.6),
              ("coulomb", 2, 2, "open"): (8, 0.9), ("coulomb", 2, 9, "open"): (2, 0.9), ("coulomb", 2, 2, "cell"): (4, 0.9),
              ("coulomb", 64, 64, "open"): (2, 0.7), ("coulomb", 64, 71, "open"): (3, 0.6), ("coulomb", 64, 64, "cell"): (1, 0.6),
              ("coulomb", 97, 97, "cell"): (8, 0.6), ("coulomb", 97, 104, "cell"): (2, 0.6),
              ("coulomb", 97, 97, "open"): (17, 0.6), ("coulomb", 97, 104, "open"): (12, 0.6),
              # the strain entry runs on the main weights but for two inputs whose gE defect lay 2.0 and 2.3 bounds off at that route's K
              ("strain", 33, 33, "cell"): (4, 0.7), ("strain", 97, 104, "cell"): (8, 0.6)}
MARGIN_FACTOR = 16          # nudged_weights clears |z| < 16 max |z32 - z64|; the test asserts 8

BOX = np.float32([6.0, 6.0, 6.0])                                        # width 2 * cutoff: the smallest box


def _smallest_sheared():
    shape = np.array([[1.0, 0.0, 0.0], [0.35, 1.0, 0.0], [-0.3, 0.25, 1.0]])
    w = cell_ref.widths(shape.astype(np.float32)).min()
    return np.float32(shape * (2 * CUTOFF / w) * (1 + 1e-6))


CELL = _smallest_sheared()                                               # smallest perpendicular width just above 2 * cutoff
GEOMS = ("open", "box", "cell")

Inp = collections.namedtuple("Inp", "n count N geom seed scale")


def make_inp(n, N, geom, entry):
    """The input of an entry: the Coulomb entries have weights of their own (WEIGHTS_OF), some of them per padded size and geometry."""
    group = "coulomb" if entry.startswith("coulomb") else ("strain" if entry == "strain" else "main")
    return Inp(n, dict(SIZES)[n], N, geom, *WEIGHTS_OF.get((group, n, N, geom), WEIGHTS_OF[("coulomb" if group == "coulomb" else "main", n)]))


# entry -> (geometries, outputs, defect models that apply)
FAMILIES = ("msg", "upd", "pas")
ENTRIES = {
    "vjp":        (("open", "box", "cell"), ("gxyz",), ("gE",) + FAMILIES),
    "strain":     (("cell",), ("strain",), ("gE",) + FAMILIES),
    "jvp_v":      (("open", "cell"), ("tq",), ("te",) + FAMILIES),
    "jvp_strain": (("open", "cell"), ("tq",), ("te",) + FAMILIES),
    "jvp_dQ":     (("open", "cell"), ("tq",), FAMILIES),
    "jvp_all":    (("open", "cell"), ("tq",), ("te",) + FAMILIES),
    "multi":      (("open",), tuple(f"tq{k}" for k in range(MULTI_K)), ()),        # (its columns' defects: the jvp entries')
    "coulomb":    (("open",), ("fq",), ("gE",) + FAMILIES),
    "coulomb_cell": (("cell",), ("fq", "gs_q"), ("gE",) + FAMILIES),
    "train":      (("open", "cell"), tuple(f"layer{k}" for k in range(3 * (1 + 2 * T))) + ("all",), FAMILIES),
}
_CACHE = {}


def cell_of(inp):
    return {"open": np.zeros((3, 3), np.float32), "box": np.diag(BOX).astype(np.float32), "cell": CELL}[inp.geom]


def rms(a):
    return float(np.sqrt(np.mean(np.square(np.asarray(a, dtype=np.float64)))))


def cut16(a):
    """a with every value cut to 16 mantissa bits: what two truncated bf16 pieces keep of a float32."""
    f = np.ascontiguousarray(a, dtype=np.float32)
    return (f.view(np.uint32) & np.uint32(0xFFFFFF00)).view(np.float32).astype(np.asarray(a).dtype)


def _dense_rows(rng, n, nx):
    x = rng.uniform(0.05, 1.0, size=(n, nx)).astype(np.float32)
    x.view(np.uint32)[...] |= 0x101
    return x


def _cluster(rng, n):
    """n points in a cube that holds 0.2 atoms per cubic Angstrom, at least 1.0 apart (as tests/test_gpu_f32_grade.py)."""
    span = (n / 0.2) ** (1.0 / 3.0)
    pts = []
    while len(pts) < n:
        p = rng.uniform(0, span, size=3)
        if all(np.linalg.norm(p - o) > 1.0 for o in pts):
            pts.append(p)
    return np.asarray(pts, dtype=np.float32)


def molecules(inp):
    """[(xyz, x, Q)]: molecule k of a batch has its own seed; the same atoms at N = n and N = n + 7."""
    key = ("mols", inp.n, inp.count, inp.geom)
    if key not in _CACHE:
        mols = []
        for k in range(inp.count):
            rng = np.random.default_rng(9000 + 131 * k + inp.n)
            if inp.geom == "open":
                xyz = _cluster(rng, inp.n)
            elif inp.geom == "box":
                xyz = periodic_ref.random_cell(rng, inp.n, BOX)
            else:
                xyz = cell_ref.random_cell(rng, inp.n, CELL)
            Q = CHARGES[k % 3] * (1.0 if inp.n >= 5 else inp.n / 6.0)
            mols.append((xyz, _dense_rows(rng, inp.n, NX), float(np.float32(Q))))
        _CACHE[key] = mols
    return _CACHE[key]


def batch(inp):
    mols = molecules(inp)
    off = np.arange(inp.count + 1, dtype=np.int32) * inp.n
    return (off, np.concatenate([m[0] for m in mols]), np.concatenate([m[1] for m in mols]), np.array([m[2] for m in mols], dtype=np.float32))


def tangents(inp):
    """g (A,), y (A,), and MULTI_K directions: v (K, A, 3), strain (K, 3, 3), dQ (K,).  Direction 0 is v alone, 1 strain alone, 2 dQ
    alone, 3 all three (the four jvp entries); the others mix them."""
    key = ("tan", inp.n, inp.count)
    if key not in _CACHE:
        rng = np.random.default_rng(77 + inp.n)
        A = inp.n * inp.count
        g = rng.normal(size=A).astype(np.float32)
        y = rng.uniform(-0.5, 0.5, size=A).astype(np.float32)
        v = rng.normal(size=(MULTI_K, A, 3)).astype(np.float32)
        strain = (0.3 * rng.normal(size=(MULTI_K, 3, 3))).astype(np.float32)
        dQ = rng.uniform(-1.0, 1.0, size=MULTI_K).astype(np.float32)
        v[1], v[2] = 0, 0
        strain[0], strain[2] = 0, 0
        dQ[0], dQ[1] = 0, 0
        for k in range(4, MULTI_K):                                      # the further columns: each kind alone and in pairs, in turn
            if k % 3 == 0:
                strain[k] = 0
            if k % 3 == 1:
                dQ[k] = 0
            if k % 4 == 2:
                v[k] = 0
        _CACHE[key] = (g, y, v, strain, dQ)
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------- recording and defects
class _Stop(Exception):
    pass


def _family(layers, where=None):
    if where in ("listed", "swapped") or layers[-1][0].shape[1] == 1:
        return "pas"
    return "upd" if layers[0][0].shape[0] == H_DIM + 32 else "msg"


def _parse(defect):
    """(family, layer or None) of a defect (c) model name."""
    fam, _, layer = defect.partition(".")
    return fam, (int(layer) if layer else None)


@contextlib.contextmanager
def instrumented(defect=None, record=None, stop_after=None):
    """The references' MLP functions replaced by ones that (record) append the ReLU pre-activations of every forward MLP call to
    `record`, as (family, [z of layer 1, z of layer 2]), and (defect) run a defect model.  Without a defect the replaced functions
    compute what the originals compute, statement by statement."""
    saved = otr._mlp_fwd, otr._mlp_bwd, jvp_ref._mlp, xgr._CUT_GE, jvp_ref._CUT_TE
    fam_cut, layer_cut = _parse(defect) if defect in _DENSE_DEFECTS else (None, None)
    ident = lambda a: a

    def cutter(layers, where, l):
        return cut16 if _family(layers, where) == fam_cut and layer_cut in (None, l) else ident

    def fwd(rows, layers):
        out, tape = saved[0](rows, layers)
        if record is not None:
            record.append((_family(layers), tape[1][1:]))
            if stop_after is not None and len(record) == stop_after:
                raise _Stop()
        return out, tape

    def bwd(dout, tape, layers, where="gnn"):
        acts, pres = tape
        shift = otr._KINK_SHIFT if otr._KINK_WHERE in ("all", where) else 0.0
        grads = [None] * len(layers)
        last = len(layers) - 1
        c = cutter(layers, where, last)
        W, b = layers[-1]
        grads[-1] = (c(acts[-1]).T @ c(dout), dout.sum(0))
        d = c(dout) @ c(W).T
        for l in range(len(layers) - 2, -1, -1):
            c = cutter(layers, where, l)
            d = d * (pres[l + 1] > shift)
            W, b = layers[l]
            grads[l] = (c(acts[l]).T @ c(d), d.sum(0))
            d = c(d) @ c(W).T
        return d, grads

    def jmlp(X, tX, layers, s):
        pres = []
        for l, (W, b) in enumerate(layers[:-1]):
            c = cutter(layers, None, l)
            pre = X @ W + b
            tX = (c(tX) @ c(W)) * (pre > s)
            X = np.maximum(pre, 0)
            pres.append(pre)
        if record is not None:
            record.append((_family(layers), pres))
        W, b = layers[-1]
        c = cutter(layers, None, len(layers) - 1)
        return X @ W + b, c(tX) @ c(W)

    otr._mlp_fwd = fwd
    if fam_cut is not None:
        otr._mlp_bwd = bwd
    if fam_cut is not None or record is not None:
        jvp_ref._mlp = jmlp
    xgr._CUT_GE = cut16 if defect == "gE" else None
    jvp_ref._CUT_TE = cut16 if defect == "te" else None
    try:
        yield
    finally:
        otr._mlp_fwd, otr._mlp_bwd, jvp_ref._mlp, xgr._CUT_GE, jvp_ref._CUT_TE = saved


_DENSE_DEFECTS = FAMILIES + tuple(f"{f}.{l}" for f in FAMILIES for l in range(3))


# ---------------------------------------------------------------------------------------------------- pre-activations and the nudge
def _vjp(inp, mol, g, w, **kw):
    """(q, gxyz, strain or None) of one molecule in the input's geometry."""
    xyz, x, Q = mol
    if inp.geom == "open":
        return xgr.vjp64(xyz, x, Q, g, w, N=inp.N, **kw) + (None,)
    if inp.geom == "box":
        return periodic_ref.vjp64_pbc(xyz, x, Q, g, BOX, w, N=inp.N, **kw) + (None,)
    return cell_ref.strain64(xyz, x, Q, g, CELL, w, N=inp.N, **kw)


_STAGES = [("msg", 0, 0), ("msg", 0, 1), ("upd", None, 0), ("upd", None, 1), ("msg", 1, 0), ("msg", 1, 1),
           ("pas", 0, 0), ("pas", 0, 1), ("pas", 1, 0), ("pas", 1, 1)]


def preacts(inp, w, dtype=np.float64):
    """{(family, step or None for the shared update MLP, layer): z (rows, units)} of the batch's forward: every row the reference
    evaluates, padded partners and both row orders of the pass network included."""
    out = collections.defaultdict(list)
    for mol in molecules(inp):
        rec = []
        with instrumented(record=rec, stop_after=4 * T):
            try:
                _vjp(inp, mol, np.zeros(inp.n), w, dtype=dtype)
            except _Stop:
                pass
        fams = [f for f, _ in rec]
        assert fams == ["msg", "upd"] * T + ["pas"] * (2 * T), fams
        for k, (fam, zs) in enumerate(rec):
            t = None if fam == "upd" else (k // 2 if fam == "msg" else (k - 2 * T) // 2)
            for l, z in enumerate(zs):
                out[(fam, t, l)].append(np.asarray(z, dtype=np.float64))
    return {key: np.concatenate(v) for key, v in out.items()}


def kink_margin(inp, w):
    """(min |z64|, max |z32 - z64|) over every ReLU pre-activation of the batch."""
    z64, z32 = preacts(inp, w, np.float64), preacts(inp, w, np.float32)
    return min(float(np.abs(z).min()) for z in z64.values()), max(float(np.abs(z32[k] - z64[k]).max()) for k in z64)


def _copy(w):
    c = lambda m: [(np.array(W, dtype=np.float32), np.array(b, dtype=np.float32)) for W, b in m]
    return {"msg": [c(m) for m in w["msg"]], "upd": c(w["upd"]), "pas": [c(m) for m in w["pas"]]}


def nudged_weights(inp, base, margin, rounds=60):
    """`base` with biases moved until every ReLU pre-activation of the input's float64 forward has |z| >= margin: the first stage (in
    the order the forward runs them) with a unit inside the margin gets that unit's bias moved by the smallest multiple of the margin
    that leaves the unit's whole column 1.5 margins clear; then the forward runs again, to a fixed point."""
    w = _copy(base)
    for _ in range(rounds):
        zs = preacts(inp, w)
        for fam, t, l in _STAGES:
            z = zs[(fam, t, l)]
            bad = np.nonzero(np.abs(z).min(0) < margin)[0]
            if not bad.size:
                continue
            bias = (w["upd"] if fam == "upd" else w[fam][t])[l][1]
            for u in bad:
                col = z[:, u]
                for k in range(1, 4000):
                    steps = [np.float32(bias[u] + s * k * margin) for s in (1.0, -1.0)]
                    ok = [b for b in steps if np.abs(col + (float(b) - float(bias[u]))).min() >= 1.5 * margin]
                    if ok:
                        bias[u] = ok[0]
                        break
                else:
                    raise AssertionError(f"no clear bias for {fam} {t} layer {l} unit {u} of {inp}")
            break
        else:
            return w
    raise AssertionError(f"the nudge of {inp} did not settle in {rounds} rounds")


def weights(inp):
    """The input's weights: the base weights nudged clear of its ReLU kinks."""
    key = ("w",) + tuple(inp)
    if key not in _CACHE:
        base = random_weights(NX, T, seed=inp.seed, scale=inp.scale)
        _CACHE[key] = nudged_weights(inp, base, MARGIN_FACTOR * kink_margin(inp, base)[1])
    return _CACHE[key]


# ---------------------------------------------------------------------------------------------------- the references
def _dense_batch(inp):
    mols = molecules(inp)
    dense = []
    for xyz, x, Q in mols:
        d = list(orc.dense_inputs(xyz, x, np.float32(Q), inp.N, h_dim=H_DIM, e_dim=H_DIM))
        if inp.geom != "open":
            d[1][:inp.n, :inp.n] = cell_ref.get_init_edges_cell(xyz, cell_of(inp), num=H_DIM)[0]
        dense.append(d)
    return [np.stack([d[k] for d in dense]) for k in range(5)]


def train_layers(w):
    """[(offset, size)] of every Dense layer (kernel and bias) in the flat gradient vector (otr.flatten's order)."""
    out, pos = [], 0
    for m in [w["upd"]] + list(w["msg"]) + list(w["pas"]):
        for W, b in m:
            out.append((pos, W.size + b.size))
            pos += W.size + b.size
    return out


def _evaluate(inp, entry, dtype, kink_shift):
    w = weights(inp)
    mols = molecules(inp)
    g, y, v, strain, dQ = tangents(inp)
    kw = dict(dtype=dtype, kink_shift=kink_shift)
    sl = lambda k: slice(k * inp.n, (k + 1) * inp.n)
    if entry in ("vjp", "strain"):
        res = [_vjp(inp, m, g[sl(k)].astype(np.float64), w, **kw) for k, m in enumerate(mols)]
        return {"gxyz": np.concatenate([r[1][:, :3] for r in res])} if entry == "vjp" else {"strain": np.stack([r[2] for r in res])}
    if entry.startswith("jvp_") or entry == "multi":
        cols = {"jvp_v": [0], "jvp_strain": [1], "jvp_dQ": [2], "jvp_all": [3], "multi": range(MULTI_K)}[entry]
        out = {}
        for c in cols:
            tq = [jvp_ref.jvp64(xyz, x, Q, w, N=inp.N, v=v[c][sl(k)] if v[c].any() else None, strain=strain[c] if strain[c].any() else None,
                                dQ=float(dQ[c]) if dQ[c] != 0 else None, cell=None if inp.geom == "open" else cell_of(inp), **kw)[1]
                  for k, (xyz, x, Q) in enumerate(mols)]
            out["tq" if entry != "multi" else f"tq{c}"] = np.concatenate(tq)
        return out
    if entry == "coulomb":
        return {"fq": np.concatenate([coulomb_ref.coulomb_forces64(xyz, x, Q, w, inp.N, KE, ALPHA, **kw)[5] for xyz, x, Q in mols])}
    if entry == "coulomb_cell":
        params = ewald_ref.ewald_params64(CELL, ALPHA, EWALD_TOL)
        res = [ewald_ref.ewald_forces64(xyz, x, Q, CELL, w, inp.N, KE, ALPHA, params, **kw) for xyz, x, Q in mols]
        return {"fq": np.concatenate([r[6] for r in res]), "gs_q": np.stack([r[8] for r in res])}
    assert entry == "train"
    yd = np.zeros((inp.count, inp.N, 1), dtype=np.float32)
    yd[:, :inp.n, 0] = y.reshape(inp.count, inp.n)
    grads = otr.flatten(otr.loss_and_grads(*_dense_batch(inp), yd, w, **kw)[2])
    if np.dtype(dtype) != np.float64:
        grads = grads.astype(np.float32).astype(np.float64)
    out = {f"layer{k}": grads[a:a + s] for k, (a, s) in enumerate(train_layers(w))}
    out["all"] = grads
    return out


def reference(inp, entry, model="64", tau=None):
    """{output: array} of the entry on the input under the model (module docstring); kept and read-only."""
    assert inp.geom in ENTRIES[entry][0], (inp, entry)
    key = ("ref", tuple(inp), entry, model, tau)
    if key not in _CACHE:
        if model in ("64", "32"):
            out = _evaluate(inp, entry, np.float64 if model == "64" else np.float32, 0.0)
        elif model in ("+tau", "-tau"):
            out = _evaluate(inp, entry, np.float64, tau if model == "+tau" else -tau)
        else:
            with instrumented(defect=model):
                out = _evaluate(inp, entry, np.float64, 0.0)
        for a in out.values():
            assert np.isfinite(a).all(), (inp, entry, model)
            a.setflags(write=False)
        _CACHE[key] = out
    return _CACHE[key]


def noise(inp, entry):
    """{output: (noise_rms, noise_max, max |ref64|)}."""
    r64, r32 = reference(inp, entry, "64"), reference(inp, entry, "32")
    return {k: (rms(r32[k] - r64[k]), float(np.abs(r32[k] - r64[k]).max()), float(np.abs(r64[k]).max())) for k in r64}
