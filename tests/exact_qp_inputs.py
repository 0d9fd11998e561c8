"""Exact cases for the quasiparticle family of the C ABI: mpsk_qp_half, mpsk_qp_apply, mpsk_qp_heff_site,
mpsk_transfer_left_pair and mpsk_transfer_right_pair (the sums of include/mpsk.h).  Same rules as tests/exact_inputs.py
and tests/exact_proj_inputs.py, which this module reuses: integer-valued operands whose every partial sum stays below
2^50 (asserted per case and per sub-case), so fp64 never rounds, every correct route returns the same bits and the
comparison is np.array_equal; and Gaussian cases inside a derived componentwise bound.  All entries are MPSK_F64 only.

Operations and sub-cases (`keys`).  A case record holds the operands once and one reference per key:

    qp_half   half[a,t,m,u] = sum G[a,w,c] AL[c,s,m] O[w,t,s,u]                                     key "half"
    qp_apply  y = proj(G, B, O, R) + proj(lB, AR, O, R) + proj(G, AL, O, rB)                        keys COMBOS
    qp_heff   Xout = VL^T (y with B = VL X, Dlo = Dl, Dro = Dr) - E X                               keys (combo, E)
    tl_pair   out[q,v,b] = sum_i Vi[p,w,a] Ai[a,s,b] O[w,t,s,v] Ab[p,t,q]                           key "pair"
    tr_pair   out[a,w,p] = sum_i Ai[a,s,b] Vi[b,v,q] O[w,t,s,v] Ab[p,t,q]                           key "pair"

    proj(G, x, O, R)[p,t,q] = sum G[p,w,a] x[a,s,b] O[w,t,s,v] R[b,v,q]

COMBOS: "all" both pairs, "no_left" without (lB, AR), "no_right" without (half, rB), "plain" neither.  E is 0 or the
dyadic E_DYADIC.  Environments are stacked [Dbra, W, Dket] (uploaded as W slabs), O is the dense [Wl, d, d, Wr] form of
the slice with index order [w, t(out), s(in), v]; VL is [Dl d, n] with rows (p, t), p fastest.  mpsk_qp_heff_site is
multilinear, so VL, AL and X are integer arrays like everything else: nothing is orthogonal, and n, Dr2 are free.

Every term is evaluated pairwise with np.tensordot: order 1 is the bracket order of the library (left environment first;
the right pair transfer contracts the ket first), order 2 starts from the other end.  conv = _hp gives the longdouble
reference (exact cases: while the work stays under ei.LD_MAX_WORK), conv = _abs_hp the right-hand side of the bound.

The 2^50 guard.  The worst-case magnitude of a key is the sum over its terms of prod(max|operand|) prod(contracted
extents) (plus |E| max|X|).  The centre term of qp_heff has six operands (VL, G, VL, X, O, R) and five contracted
extents (Dl d, Dl, n, Wl d, Dr Wr); at (512, 2, 512, 64) entries in [-4, 4] would reach 2^51.6, so that case draws VL and
X from {-1, 0, 1} and the environments and site tensors from [-2, 2].  `t["ranges"]` records the range of every operand
and `t["magnitude"][key]` the worst case of every key.

The componentwise bound of the Gaussian cases, by the rules at the top of tests/exact_inputs.py.  The stages of one
term nest, (1 + gamma_a)(1 + gamma_b)(1 + gamma_c) - 1 <= gamma_{a+b+c}, so a term of bracket order (a)(w s)(b v) errs
by at most (Ka + Wl d + Kb Wr + 8) u |term|, |term| the same contraction of the absolute values and 8 the two roundings
of slack per stage boundary; started from the other end the extents are (Kb + d Wr + Wl Ka), and the larger of the two is
taken, so the bound holds for either order (tests/test_exact_qp_inputs_cpu.py evaluates numpy fp64 in order 2 against
it).  (Ka, Kb) = (Dl, Dr) for the centre term, (Dl2, Dr) for the (lB, AR) term, (Dl, Dr2) for the (half, rB) term.  The
library adds the (lB, AR) product into the stage-1 buffer of the centre term and the (half, rB) product onto y: each is
one more rounding on what is already there, the same count as adding finished terms, and a sum of t terms is bounded by
the sum of the terms' bounds plus t roundings on the sum of the absolute values:

    |got - ref| <= sum_i (depth_i + 8) u |term_i| + t u sum_i |term_i|        (t = 0 for a single term)

qp_heff: the centre term passes through B = VL X first (extent n) and every term through the pull-back (extent Dl d);
gamma Z is one rounding for the product and one for the addition, which every term of the accumulator shares: depth_i
grows by Dl d + 2 (+ n for the centre term), and -E X is a term of its own with depth 2 - 8 (two roundings in all).
Pair transfers, per term i: left (Dl_i + Wl d + Dlb d) or (Dlb + d Wl + Dl_i d), right (Dr_i + Wr d + d Drb) or
(Drb + Wr d + d Dr_i).  qp_half: (Dl + Wl d) or (d + Wl Dl).  No margin is added anywhere.

`wrong(op, t, key, how)` evaluates plausible WRONG contractions on the same operands; the CPU self-check requires every
one of them to change the reference of every exact case it applies to."""
from __future__ import annotations

import functools

import numpy as np

import exact_inputs as ei
import exact_proj_inputs as epi
from exact_inputs import LD, U, _abs_hp, _hp, _rng, assert_exact_range, gauss_array, int_array

OPS = ("qp_half", "qp_apply", "qp_heff", "tl_pair", "tr_pair")
COMBOS = ("all", "no_left", "no_right", "plain")
E_DYADIC = -2.5
DENSE_W, DENSE_D = ei.DENSE_W, ei.DENSE_D
MAXSEG = epi.MAXSEG
RAGGED_CHIS, ALIGNED_CHIS = epi.RAGGED["chis"], epi.ALIGNED["chis"]

# bonds: (Dlo, Dl, Dl2, Dr, Dr2, Dro) of qp_half / qp_apply; the pair transfers read the same six numbers as
# (Dlb, Dl1, Dl2, Dr, Dr2, Drb) -- left: kets [Dl1, d, Dr], [Dl2, d, Dr]; right: kets [Dl1, d, Dr], [Dl1, d, Dr2].
# heff: (Dl, Dl2, Dr, Dr2, n) of qp_heff (Dlo = Dl, Dro = Dr, VL [Dl d, n]).
SHAPES = {
    # every bond different and odd or prime-ish, one 65 and one 33 (PROJ = (20, 33, 65, 48)): unaligned loaders, odd offsets
    "ragged": dict(bonds=(20, 33, 17, 65, 29, 48), heff=(33, 17, 65, 29, 37), chis=RAGGED_CHIS, d=2),
    # all 128 but Dl2 = Dr2 = 64: ALIGNED = true on 64- and 128-wide tiles, even table offsets, K % 16 == 0, 2 x 2 tiles of 64
    "aligned": dict(bonds=(128, 128, 64, 128, 64, 128), heff=(128, 64, 128, 64, 128), chis=ALIGNED_CHIS, d=2),
    # aligned main bonds, odd Dl2 = Dr2 = 33: the accumulating launch takes the unaligned kernel (dense route: tabs_even
    # true, then false, on two dense_tab keys); n = 223 = 2 * 128 - 33 gives the ZADD store a ragged edge and an odd ldz
    "mixed_parity": dict(bonds=(128, 128, 33, 128, 33, 128), heff=(128, 33, 128, 33, 223), chis=ALIGNED_CHIS, d=2),
    # sparse d = 3; Dl2 = Dl and Dr2 = Dr so that the mutants that exchange operands of equal shape apply
    "d3": dict(bonds=(20, 17, 17, 23, 23, 19), heff=(17, 17, 23, 23, 28), chis=RAGGED_CHIS, d=3),
    # qp_apply: Dr = Dr2 = 256 on five used levels: both stage-3 launches have KT = 5 * 16 = 80 >= 64 k-tiles on 2 tiles
    "longk": dict(bonds=(64, 64, 64, 256, 256, 64), levels=5, d=2),
    # tl_pair: stage 3 contracts (p, t), K = Dlb d = 1024 = 64 k-tiles on 5 tiles of 64 x 64
    "longk_tl": dict(bonds=(512, 64, 64, 64, 64, 64), levels=5, d=2),
    # the shape of test_split_k_pullback: pull-back M = n = 512, N = 64, K = 1024 (8 tiles, 64 k-tiles); Dl2 = 64
    "splitk_pullback": dict(heff=(512, 64, 64, 512, 512), chis=ALIGNED_CHIS, d=2,
                            ranges=dict(VL=1, X=1, G=2, R=2, lB=2, AR=2, AL=2, rB=2)),
    # 33 used levels of chi 1 on tiny bonds: both segment lists of qp_apply are chunked (32 + 1)
    "maxseg": dict(bonds=(6, 10, 7, 12, 12, 9), levels=33, d=2),
}
EXACT_SHAPES = ("ragged", "aligned", "mixed_parity")       # run on every tile, on the three slice kinds
VARIANTS = ("sparse", "dense")                             # dense: the [4, 2, 2, 4] tensor (GEMM route and mix route)
DEGENERATE = ("zeros", "empty", "b")
DEGENERATE_BONDS = dict(bonds=(20, 33, 17, 65, 29, 48), heff=(33, 17, 65, 29, 37))

_td = np.tensordot


def _id(a):
    return np.asarray(a)


# ------------------------------------------------------------------------------------------------------------------
# contractions
# ------------------------------------------------------------------------------------------------------------------
def proj(G, x, O, R, order=1):
    """y[p,t,q] = sum G[p,w,a] x[a,s,b] O[w,t,s,v] R[b,v,q]; order 1: (a)(w s)(b v), order 2: (b)(s v)(w a)"""
    if order == 1:
        t2 = _td(_td(G, x, (2, 0)), O, ([1, 2], [0, 2]))                    # [p,w,s,b] -> [p,b,t,v]
        return _td(t2, R, ([1, 3], [0, 1]))
    r2 = _td(_td(x, R, (2, 0)), O, ([1, 2], [2, 3]))                        # [a,s,v,q] -> [a,q,w,t]
    return _td(G, r2, ([1, 2], [2, 0])).transpose(0, 2, 1)


def half(G, AL, O, order=1):
    """half[a,t,m,u] = sum G[a,w,c] AL[c,s,m] O[w,t,s,u]; order 1: (c)(w s), order 2: (s)(w c)"""
    if order == 1:
        return _td(_td(G, AL, (2, 0)), O, ([1, 2], [0, 2])).transpose(0, 2, 1, 3)      # [a,w,s,m] -> [a,m,t,u]
    c = _td(AL, O, (1, 2))                                                  # [c,m,w,t,u]
    return _td(G, c, ([1, 2], [2, 0])).transpose(0, 2, 1, 3)


def tl(V, A, O, Ab, order=1):
    """out[q,v,b] = sum V[p,w,a] A[a,s,b] O[w,t,s,v] Ab[p,t,q]; order 1: (a)(w s)(p t), order 2: (p)(t w)(a s)"""
    if order == 1:
        t2 = _td(_td(V, A, (2, 0)), O, ([1, 2], [0, 2]))                    # [p,b,t,v]
        return _td(Ab, t2, ([0, 1], [0, 2])).transpose(0, 2, 1)
    c2 = _td(_td(Ab, V, (0, 0)), O, ([0, 2], [1, 0]))                       # [t,q,w,a] -> [q,a,s,v]
    return _td(c2, A, ([1, 2], [0, 1]))


def tr(V, A, O, Ab, order=1):
    """out[a,w,p] = sum A[a,s,b] V[b,v,q] O[w,t,s,v] Ab[p,t,q]; order 1: (b)(s v)(t q), order 2: (q)(t v)(s b)"""
    if order == 1:
        r2 = _td(_td(A, V, (2, 0)), O, ([1, 2], [2, 3]))                    # [a,s,v,q] -> [a,q,w,t]
        return _td(r2, Ab, ([1, 3], [2, 1]))
    c2 = _td(O, _td(V, Ab, (2, 2)), ([1, 3], [3, 1]))                       # [b,v,p,t] -> [w,s,b,p]
    return _td(A, c2, ([1, 2], [1, 2]))


def _proj_depth(Ka, Kb, O):
    Wl, d, _, Wr = O.shape
    return max(Ka + Wl * d + Kb * Wr, Kb + d * Wr + Wl * Ka)


def has_pairs(combo):
    """(the (lB, AR) pair is given, the (half, rB) pair is given)"""
    return combo in ("all", "no_right"), combo in ("all", "no_left")


def pull(VL, y):
    """VL^T y with the rows (p, t) of VL column-major, p fastest"""
    return _td(VL, y.reshape((VL.shape[0], y.shape[2]), order="F"), (0, 0))


def site_of(VL, X, d):
    return _td(VL, X, (1, 0)).reshape((VL.shape[0] // d, d, X.shape[1]), order="F")


TERM_MUTANTS = ("ts_swapped", "half_with_GR", "half_from_B", "ket2_first_env", "levels_reversed", "rB_levels_reversed")
_CACHE = {}


def _site_terms(op, t, conv, order, mut):
    """{label: (term, depth)} of every term the operation can have, before the keys select and combine them"""
    g = lambda k: conv(t[k])
    O = g("O")
    if mut == "ts_swapped":
        O = np.swapaxes(O, 1, 2)
    Wl, d, _, Wr = O.shape
    if op == "qp_half":
        G = g("G")[:, ::-1, :] if mut == "levels_reversed" else g("G")
        Dl = t["AL"].shape[0]
        return {"half": (half(G, g("AL"), O, order), max(Dl + Wl * d, d + Wl * Dl))}
    if op in ("tl_pair", "tr_pair"):
        f = tl if op == "tl_pair" else tr
        Ab = g("Ab")
        Db = (t["Ab"].shape[0] if op == "tl_pair" else t["Ab"].shape[2]) * d
        out = {}
        for i in ("1", "2"):
            V = g("V1") if (mut == "ket2_first_env" and i == "2") else g("V" + i)
            K = t["A" + i].shape[0 if op == "tl_pair" else 2]
            W = Wl if op == "tl_pair" else Wr
            out[i] = (f(V, g("A" + i), O, Ab, order), max(K + W * d + Db, Db // d + W * d + K * d))
        return out
    G, R = g("G"), g("R")
    B = site_of(g("VL"), g("X"), d) if op == "qp_heff" else g("B")
    Dl, Dr, Dl2, Dr2 = t["G"].shape[2], t["R"].shape[0], t["lB"].shape[2], t["rB"].shape[0]
    rB = g("rB")[:, ::-1, :] if mut == "rB_levels_reversed" else g("rB")
    third = (G, g("AL"), O, rB)
    if mut == "half_with_GR":
        third = (G, g("AL"), O, R)
    elif mut == "half_from_B":
        third = (G, B, O, rB)
    out = {"B": (proj(G, B, O, R, order), _proj_depth(Dl, Dr, O)),
           "L": (proj(g("lB"), g("AR"), O, R, order), _proj_depth(Dl2, Dr, O)),
           "R": (proj(*third, order), _proj_depth(Dl, Dr2, O))}
    if op == "qp_heff":
        rows, n = t["VL"].shape
        VL = g("VL")
        if mut == "pullback_untransposed":               # the buffer of VL read as an [n, rows] matrix, not transposed
            VL = np.ravel(VL, order="F").reshape((n, rows), order="F").T
        out = {k: (pull(VL, y), dep + rows + 2 + (n if k == "B" else 0)) for k, (y, dep) in out.items()}
    return out


def site_terms(op, t, conv=_id, order=1, mut=None):
    if mut not in TERM_MUTANTS and mut != "pullback_untransposed":
        mut = None
    k = (t["name"], conv.__name__, order, mut)
    if k not in _CACHE:
        _CACHE[k] = _site_terms(op, t, conv, order, mut)
    return _CACHE[k]


def terms(op, t, key, conv=_id, order=1, mut=None):
    """[(term, depth)] of sub-case `key`, in the order the library adds them"""
    st = site_terms(op, t, conv, order, mut)
    if op == "qp_half":
        return [st["half"]]
    if op in ("tl_pair", "tr_pair"):
        return [st["1"], st["2"]]
    combo, E = key if op == "qp_heff" else (key, 0.0)
    left, right = has_pairs(combo)
    out = [st["B"]] + ([st["L"]] if left else []) + ([st["R"]] if right else [])
    if op == "qp_heff" and E != 0.0:
        X = conv(t["X"])
        out.append((abs(E) * X if conv is _abs_hp else -E * X, 2 - 8))
    return out


def evaluate(op, t, key, conv=_id, order=1):
    ts = terms(op, t, key, conv, order)
    out = ts[0][0]
    for x, _ in ts[1:]:
        out = out + x
    return out


def bound(op, t, key):
    """the componentwise bound of the module docstring, in longdouble"""
    ts = terms(op, t, key, _abs_hp, 1)
    total = sum(x for x, _ in ts)
    b = sum((dep + 8) * LD(U) * x for x, dep in ts)
    return b + (len(ts) * LD(U) * total if len(ts) > 1 else 0)


def keys(op, shape="ragged"):
    if op == "qp_half":
        return ["half"]
    if op in ("tl_pair", "tr_pair"):
        return ["pair"]
    if op == "qp_apply":
        return list(COMBOS)
    if shape == "splitk_pullback":                   # the sub-cases of test_split_k_pullback
        return [(c, E) for c in ("all", "plain") for E in (0.0, E_DYADIC)]
    return [(c, E) for c in COMBOS for E in (0.0, E_DYADIC)]


def key_id(key):
    return key if isinstance(key, str) else f"{key[0]}-E{key[1]:g}"


# ------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------
def int_range(rng, r, *shape):
    """integers uniform in [-r, r] as fp64; r = 4 is ei.int_array"""
    if r == 4:
        return int_array(rng, *shape)
    return rng.integers(-r, r + 1, size=shape).astype(np.float64)


def _magnitude(op, t, key):
    """sum over the terms of prod(max|operand|) prod(contracted extents), asserted below 2^50"""
    O = t["O"]
    Wl, d, _, Wr = O.shape
    if op == "qp_half":
        return assert_exact_range([t["G"], t["AL"], O], [t["AL"].shape[0], Wl, d], t["name"])
    if op in ("tl_pair", "tr_pair"):
        Dlb, _, Drb = t["Ab"].shape
        m = 0.0
        for i in ("1", "2"):
            K = t["A" + i].shape[0 if op == "tl_pair" else 2]
            ext = [K, Wl, d, Dlb, d] if op == "tl_pair" else [K, Wr, d, Drb, d]
            m += ei.magnitude([t["V" + i], t["A" + i], O, t["Ab"]], ext)
        assert m < ei.LIMIT, f"{t['name']}: worst-case magnitude {m:.3e} is not below 2^50"
        return m
    combo, E = key if op == "qp_heff" else (key, 0.0)
    left, right = has_pairs(combo)
    Dl, Dr, Dl2, Dr2 = t["G"].shape[2], t["R"].shape[0], t["lB"].shape[2], t["rB"].shape[0]
    pre, ext = [], []
    if op == "qp_heff":
        rows, n = t["VL"].shape
        pre, ext = [t["VL"]], [rows]
        centre = ei.magnitude(pre + [t["G"], t["VL"], t["X"], O, t["R"]], ext + [Dl, n, Wl, d, Dr, Wr])
    else:
        centre = ei.magnitude([t["G"], t["B"], O, t["R"]], [Dl, Wl, d, Dr, Wr])
    m = centre
    if left:
        m += ei.magnitude(pre + [t["lB"], t["AR"], O, t["R"]], ext + [Dl2, Wl, d, Dr, Wr])
    if right:
        m += ei.magnitude(pre + [t["G"], t["AL"], O, t["rB"]], ext + [Dl, Wl, d, Dr2, Wr])
    if E != 0.0:
        m += ei.magnitude([t["X"], [abs(E)]], [])
    assert m < ei.LIMIT, f"{t['name']}-{key_id(key)}: worst-case magnitude {m:.3e} is not below 2^50"
    return m


def _work(op, t):
    """multiply-adds of all terms of the operation (the largest key), as the LD_MAX_WORK budget counts them"""
    O = t["O"]
    Wl, d, _, Wr = O.shape
    stage = lambda R_, Ka, Kb, Ro: R_ * Wl * Ka * d * Kb + R_ * Kb * Wl * Wr * d * d + R_ * d * Kb * Wr * Ro
    if op == "qp_half":
        Dlo, _, Dl = t["G"].shape
        return Dlo * Wl * Dl * d * t["AL"].shape[2] * (1 + Wr)
    if op in ("tl_pair", "tr_pair"):
        Dlb, _, Drb = t["Ab"].shape
        return sum(stage(Dlb, t["A" + i].shape[0], t["A" + i].shape[2], Drb) for i in ("1", "2"))
    Dlo, _, Dl = t["G"].shape
    Dr, _, Dro = t["R"].shape
    w = stage(Dlo, Dl, Dr, Dro) + stage(Dlo, t["lB"].shape[2], Dr, Dro) + stage(Dlo, Dl, t["rB"].shape[0], Dro)
    if op == "qp_heff":
        rows, n = t["VL"].shape
        w += 4 * rows * n * Dr
    return w


def _finish(op, t, kind, shape):
    t["op"], t["kind"], t["shape"] = op, kind, shape
    t["keys"] = keys(op, shape)
    t["work"] = _work(op, t)
    if kind == "int":
        t["magnitude"] = {k: _magnitude(op, t, k) for k in t["keys"]}
        t["refs"] = {k: evaluate(op, t, k) for k in t["keys"]}
        t["bounds"] = {k: None for k in t["keys"]}
    else:
        t["refs"] = {k: evaluate(op, t, k, _hp) for k in t["keys"]}
        t["bounds"] = {k: bound(op, t, k) for k in t["keys"]}
    for v in list(t.values()) + list(t["refs"].values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


def _operands(op, t, rng, draw, bonds, heff, d, W):
    """draw the operands of `op` into t; draw(name, *shape)"""
    if op == "qp_heff":
        Dl, Dl2, Dr, Dr2, n = heff
        t.update(G=draw("G", Dl, W, Dl), R=draw("R", Dr, W, Dr), VL=draw("VL", Dl * d, n), X=draw("X", n, Dr),
                 lB=draw("lB", Dl, W, Dl2), AR=draw("AR", Dl2, d, Dr), AL=draw("AL", Dl, d, Dr2), rB=draw("rB", Dr2, W, Dr))
        return
    Dlo, Dl, Dl2, Dr, Dr2, Dro = bonds
    if op == "qp_half":
        t.update(G=draw("G", Dlo, W, Dl), AL=draw("AL", Dl, d, Dr2))
    elif op == "qp_apply":
        t.update(G=draw("G", Dlo, W, Dl), R=draw("R", Dr, W, Dro), B=draw("B", Dl, d, Dr), lB=draw("lB", Dlo, W, Dl2),
                 AR=draw("AR", Dl2, d, Dr), AL=draw("AL", Dl, d, Dr2), rB=draw("rB", Dr2, W, Dro))
    elif op == "tl_pair":                            # (Dlb, Dl1, Dl2, Dr, -, Drb)
        t.update(V1=draw("V1", Dlo, W, Dl), A1=draw("A1", Dl, d, Dr), V2=draw("V2", Dlo, W, Dl2), A2=draw("A2", Dl2, d, Dr),
                 Ab=draw("Ab", Dlo, d, Dro))
    elif op == "tr_pair":                            # (Dlb, Dl, -, Dr1, Dr2, Drb)
        t.update(V1=draw("V1", Dr, W, Dro), A1=draw("A1", Dl, d, Dr), V2=draw("V2", Dr2, W, Dro), A2=draw("A2", Dl, d, Dr2),
                 Ab=draw("Ab", Dlo, d, Dro))
    else:
        raise KeyError(op)


@functools.lru_cache(maxsize=None)
def case(op, shape="ragged", kind="int", variant="sparse"):
    """Operands, references and bounds (None: exact) of one case; built once, shared, never modified.  variant "dense":
    the dense tensor [4, 2, 2, 4]; shapes with `levels`: epi.long_slice on that many levels of chi 1, all of them used."""
    import mpskit_oracle as mo
    S = SHAPES[shape]
    name = f"{op}-{shape}-{variant}-{kind}"
    rng = _rng(name)
    ranges = dict(S.get("ranges", {})) if op == "qp_heff" else {}
    if kind == "int":
        draw = lambda k, *shp: int_range(rng, ranges.get(k, 4), *shp)
    else:
        draw = lambda k, *shp: gauss_array(rng, *shp)
    d = S["d"]
    if variant == "dense":
        d = DENSE_D
        s = mo.SparseMPOSlice(1, d, [DENSE_W], [DENSE_W], {(0, 0): draw("O", DENSE_W, d, d, DENSE_W)})
    elif "levels" in S:
        s = epi.long_slice(rng, S["levels"], d)
    else:
        while True:                                  # a slice symmetric in (t, s) could not show the two swapped: draw again
            s = ei.rand_slice(rng, len(S["chis"]), d, S["chis"], int_array if kind == "int" else gauss_array)
            if not np.array_equal(s.full(), np.swapaxes(s.full(), 1, 2)):
                break
    t = {"name": name, "dense": variant == "dense", "s": s, "O": np.asarray(s.full(), dtype=np.float64), "chis": list(s.chil),
         "slice_args": (s.odim, s.d, list(s.chil), list(s.chir), dict(s.Os)),
         "ranges": {k: ranges.get(k, 4) for k in ("G", "R", "B", "VL", "X", "lB", "AR", "AL", "rB", "V1", "A1", "V2", "A2", "Ab", "O")}}
    if "levels" in S:
        col, row = epi.used_levels(t["O"])
        assert col.all() and row.all(), name                 # every level is used: the segment lists have `levels` entries
    _operands(op, t, rng, draw, S.get("bonds"), S.get("heff"), d, sum(s.chil))
    return _finish(op, t, kind, shape)


def cases_exact():
    """(op, shape, variant) of the integer cases that run on every tile (the dense ones on both routes)"""
    return [(op, shp, v) for op in OPS for shp in EXACT_SHAPES for v in VARIANTS]


def cases_auto():
    """(op, shape, variant) of the integer cases that run on the automatic tile only"""
    return [("qp_apply", "longk", "sparse"), ("tl_pair", "longk_tl", "sparse"), ("qp_heff", "splitk_pullback", "sparse"),
            ("qp_apply", "maxseg", "sparse"), ("tr_pair", "maxseg", "sparse")] + [(op, "d3", "sparse") for op in OPS]


def cases_gauss():
    return [(op, "ragged", v) for op in OPS for v in VARIANTS]


def case_id(c):
    return "-".join(c)


# ------------------------------------------------------------------------------------------------------------------
# degenerate slices
# ------------------------------------------------------------------------------------------------------------------
def degenerate_slice_args(which):
    """(odim, d, chil, chir, blocks) of mpsk_mposlice_create.  "zeros": dense blocks whose entries are all zero -- the
    library derives the used levels from the values, so no level is used on the way out; "empty": no blocks at all; "b":
    epi.degenerate_slice("b"), an interior level nothing enters and one nothing leaves."""
    chis, d = epi.DEGENERATE_CHIS, epi.DEGENERATE_D
    if which == "zeros":
        blocks = {(0, 1): np.zeros((chis[0], d, d, chis[1])), (1, 3): np.zeros((chis[1], d, d, chis[3])),
                  (3, 4): np.zeros((chis[3], d, d, chis[4]))}
    elif which == "empty":
        blocks = {}
    else:
        blocks = dict(epi.degenerate_slice(which).Os)
    return len(chis), d, list(chis), list(chis), blocks


@functools.lru_cache(maxsize=None)
def degenerate_case(op, which):
    """qp_apply / qp_heff on ragged bonds over a degenerate slice; every environment slab is non-zero"""
    odim, d, chil, chir, blocks = degenerate_slice_args(which)
    name = f"degenerate-{op}-{which}"
    rng = _rng(name)
    W = sum(chil)
    O = np.zeros((W, d, d, W))
    off = np.concatenate([[0], np.cumsum(chil)])
    for (i, j), v in blocks.items():
        blk = v * np.einsum("wv,ts->wtsv", np.eye(chil[i]), np.eye(d)) if np.isscalar(v) else np.asarray(v)
        O[off[i]:off[i + 1], :, :, off[j]:off[j + 1]] = blk
    t = {"name": name, "dense": False, "O": O, "chis": list(chil), "slice_args": (odim, d, chil, chir, blocks), "ranges": {}}
    _operands(op, t, rng, lambda k, *shp: int_array(rng, *shp), DEGENERATE_BONDS["bonds"], DEGENERATE_BONDS["heff"], d, W)
    for k in ("G", "R", "lB", "rB"):
        assert np.abs(t[k]).max(axis=(0, 2)).min() > 0, name
    return _finish(op, t, "int", "degenerate")


# ------------------------------------------------------------------------------------------------------------------
# plausible wrong contractions (tests/test_exact_qp_inputs_cpu.py: each must differ from the reference)
# ------------------------------------------------------------------------------------------------------------------
WRONG = ("lB_dropped", "lB_twice", "half_with_GR", "half_from_B", "rB_dropped", "rB_levels_reversed", "ket2_dropped",
         "ket2_twice", "ket2_first_env", "ts_swapped", "levels_reversed", "E_sign", "Z_transposed", "Z_wrong_ld",
         "pullback_untransposed", "E_before_pullback")


def wrong(op, t, key, how):
    """sub-case `key` of `op` with one plausible mistake; None when the mistake does not apply to it"""
    sel = lambda lab: site_terms(op, t, mut=how)[lab][0]
    if op == "qp_half":
        return sel("half") if how in ("ts_swapped", "levels_reversed") else None
    if op in ("tl_pair", "tr_pair"):
        if how == "ket2_dropped":
            return sel("1")
        if how == "ket2_twice":
            return sel("1") + 2 * sel("2")
        if how == "ket2_first_env":                  # the second ket contracted with the first environment
            return sel("1") + sel("2") if t["V1"].shape == t["V2"].shape else None
        return sel("1") + sel("2") if how == "ts_swapped" else None
    if op not in ("qp_apply", "qp_heff"):
        raise KeyError(op)
    combo, E = key if op == "qp_heff" else (key, 0.0)
    left, right = has_pairs(combo)
    cB, cL, cR = 1, int(left), int(right)
    same_r = t["R"].shape == t["rB"].shape
    if how in ("lB_dropped", "lB_twice"):
        if not left:
            return None
        cL = 0 if how == "lB_dropped" else 2
    elif how in ("half_with_GR", "half_from_B", "rB_dropped", "rB_levels_reversed"):
        if not right or (how in ("half_with_GR", "half_from_B") and not same_r):
            return None
        cR = 0 if how == "rB_dropped" else 1
    elif how in ("E_sign", "Z_transposed", "Z_wrong_ld", "E_before_pullback"):
        if op != "qp_heff" or E == 0.0 or (how == "Z_transposed" and t["X"].shape[0] != t["X"].shape[1]):
            return None
    elif how == "pullback_untransposed":
        if op != "qp_heff":
            return None
    elif how != "ts_swapped":
        return None
    out = cB * sel("B")
    if cL:
        out = out + cL * sel("L")
    if cR:
        out = out + cR * sel("R")
    if op == "qp_heff" and E != 0.0:
        X, VL = t["X"], t["VL"]
        n, Dr = X.shape
        Z = X
        if how == "E_sign":
            Z = -X
        elif how == "Z_transposed":
            Z = X.T
        elif how == "Z_wrong_ld":                    # Z read at a leading dimension of Dl d (wrapped into the buffer of X)
            i, j = np.meshgrid(np.arange(n), np.arange(Dr), indexing="ij")
            Z = np.ravel(X, order="F")[(i + j * VL.shape[0]) % X.size]
        elif how == "E_before_pullback":             # VL^T (y - E B), B = VL X: VL is not orthogonal here
            Z = _td(VL, _td(VL, X, (1, 0)), (0, 0))
        out = out - E * Z
    return out


# what the cases of each operation must be able to detect (at least one exact case where the mistake applies)
REQUIRED = {
    "qp_half": {"ts_swapped", "levels_reversed"},
    "qp_apply": {"lB_dropped", "lB_twice", "half_with_GR", "half_from_B", "rB_dropped", "rB_levels_reversed", "ts_swapped"},
    "qp_heff": {"lB_dropped", "lB_twice", "half_with_GR", "half_from_B", "rB_dropped", "rB_levels_reversed", "ts_swapped", "E_sign",
                "Z_transposed", "Z_wrong_ld", "pullback_untransposed", "E_before_pullback"},
    "tl_pair": {"ket2_dropped", "ket2_twice", "ket2_first_env", "ts_swapped"},
    "tr_pair": {"ket2_dropped", "ket2_twice", "ket2_first_env", "ts_swapped"},
}
