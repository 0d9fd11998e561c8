"""Exact cases for the dense-MPO GEMM route of the C ABI (slices of mpsk_mposlice_create_dense, mpsk_hac_info mode 4) at
every slice shape the route serves.  Same rules as tests/exact_inputs.py, which this module reuses as it stands
(int_array, magnitude / LIMIT, U, TILES, the nested componentwise bound, the longdouble conventions): integer-valued
operands whose every partial sum stays below 2^50 (asserted per sub-case), so fp64 never rounds, every correct route
returns the same bits and the comparison is np.array_equal; and Gaussian cases inside the derived bound.  MPSK_F64 only.

One `site(slc, bonds, kind, zeros)` record holds the dense tensor O[Wl, d, d, Wr] (index order [w, t(out), s(in), v]) and
the operands of every operation; `ref(op, t)` is the reference of one operation, evaluated once and shared.

    dAC        y[p,t,q] = sum G[p,w,a] x[a,s,b] O[w,t,s,v] R[b,v,q]             G [Dlo, Wl, Dl], R [Dr, Wr, Dr]
    dAC_proj   the same with Rp [Dr, Wr, Dro]
    hac        mpsk_hac_create + mpsk_hac_apply on (G, R): the reference of dAC
    hac_axpby  a0 x + a1 (H x) on the square Gs [Dl, Wl, Dl] (a shift needs Dlo == Dl), A1 = 0.5, A0 = -2
    hac_blk    H x on (Gs, R) with x in nblk = 2 / 3 row blocks (the nblk that divide Dl)
    tl, tl_ex  out[q,v,b] = sum Gt[p,w,a] x[a,s,b] O[w,t,s,v] Ab[p,t,q]        Gt [Dlb, Wl, Dl], Ab [Dlb, d, Drb]
    tr, tr_ex  out[a,w,p] = sum x[a,s,b] Rt[b,v,q] O[w,t,s,v] Ab[p,t,q]        Rt [Dr, Wr, Drb]
    tl_pair    tl(Gt, x) + tl(V2l [Dlb, Wl, Dl2], A2l [Dl2, d, Dr])
    tr_pair    tr(Rt, x) + tr(V2r [Dr2, Wr, Drb], A2r [Dl, d, Dr2])

mpsk_hac_apply_axpby has no accumulated y0: its contract (include/mpsk.h) is y = a0 x + a1 (H x) with y overwritten, so
the integer vector that a0 scales is x itself, and on O == 0 the result is exactly a0 x.

Environments are stacked [Dbra, W, Dket].  Every contraction is pairwise np.tensordot in two bracket orders: order 1 is
left-first, (a)(w s)(b v) -- the order of dAC_dense / transfer_left_dense; the right transfer contracts the bra first, as
mpsk_transfer_right does -- and order 2 is MPO-first, (s) then (w a) then the rest.  conv = _hp gives the longdouble
reference (exact cases: while the work stays under ei.LD_MAX_WORK), conv = _abs_hp the right-hand side of the bound.

Bonds.  BONDS lists (Dl, Dr); AUX gives the other six (Dlo, Dro, Dlb, Drb, Dl2, Dr2).  (7, 13) and (65, 33) are ragged:
every bond different, Dlo != Dl, Dro != Dr, Dlb != Dl, Drb != Dr, and R Dk or Dk odd, so dense_stage1 runs with
tabs_even false (the scalar-table loader of the batched GEMM); (64, 64) is square and even; (1, 1) is the smallest.  (13, 7)
serves the cache revisits.  nblk = 2, 3 must divide Dl, which no ragged bond of the list does: hac_blk has (66, 33) of its
own, and (64, 64) with nblk = 2.

The componentwise bound of the Gaussian cases (rules at the top of tests/exact_inputs.py): the three stages nest, so one
term errs by at most (depth + 8) u |term|, depth the sum of the contracted extents of the stages in the one bracket order
the library has for the operation on this route (`_depth`: the Gaussian cases run in mode 4, where nothing is folded into
an environment, so no second order is possible), 8 the two roundings of slack per stage boundary, |term| the same
contraction of the absolute values.  A pair transfer adds the second stage-1 product into the buffer of the first:
the sum of the two terms' bounds plus 2 u (|term 1| + |term 2|), as in tests/exact_qp_inputs.py.  hac_axpby passes H x
through one fused pass a0 x + a1 y: two more roundings on either term, (depth + 10) u (|a1| |H x| + |a0| |x|).

`wrong(op, t, how)` evaluates the plausible faults of this route listed in WRONG on the same operands; the CPU
self-check requires every one of them to change the reference of every exact sub-case it applies to."""
from __future__ import annotations

import functools

import numpy as np

import exact_inputs as ei
from exact_inputs import LD, U, _abs_hp, _hp, _rng, gauss_array, int_array

OPS = ("dAC", "dAC_proj", "hac", "hac_axpby", "hac_blk", "tl", "tr", "tl_ex", "tr_ex", "tl_pair", "tr_pair")
A1, A0 = 0.5, -2.0                                         # dyadic scalars of hac_axpby
NBLK = (2, 3)
GEMM_BK = 16                                               # mpsk_gemm.hip: depth of one k-tile

SLICES = [(2, 2, 2), (3, 5, 2), (5, 3, 3), (9, 7, 3), (16, 16, 16), (1, 4, 2), (4, 1, 2)]        # (Wl, Wr, d)
WORKLOAD = (16, 16, 16)
RECT = [(3, 5, 2), (5, 3, 3)]                              # ragged in every sense: rectangular both ways, odd W, odd d
BONDS = [(1, 1), (7, 13), (64, 64), (65, 33)]              # (Dl, Dr)
BONDS_WORKLOAD = [(7, 13), (64, 64)]
BLK_BONDS = (66, 33)
# (Dlo, Dro, Dlb, Drb, Dl2, Dr2)
AUX = {(1, 1): (1, 1, 1, 1, 1, 1), (7, 13): (5, 11, 9, 6, 3, 10), (13, 7): (11, 5, 6, 9, 10, 3), (64, 64): (64,) * 6,
       (65, 33): (20, 48, 34, 17, 29, 40), (66, 33): (66, 33, 66, 33, 66, 33)}
ZEROS = ("v0", "w0", "both", "all")
ZERO_SLICES = {(5, 3, 3): dict(w=1, v=1, bonds=[(7, 13), (65, 33)]), WORKLOAD: dict(w=9, v=5, bonds=[(7, 13)])}
GAUSS = [((5, 3, 3), (65, 33)), (WORKLOAD, (64, 64))]

_td = np.tensordot


def _id(a):
    return np.asarray(a)


def square_aux(bonds):
    Dl, Dr = bonds
    return (Dl, Dr, Dl, Dr, Dl, Dr)


# ------------------------------------------------------------------------------------------------------------------
# contractions
# ------------------------------------------------------------------------------------------------------------------
def proj(G, x, O, R, order=1):
    """y[p,t,q] = sum G[p,w,a] x[a,s,b] O[w,t,s,v] R[b,v,q]; order 1: (a)(w s)(b v), order 2: (s)(w a)(b v)"""
    if order == 1:
        t2 = _td(_td(G, x, (2, 0)), O, ([1, 2], [0, 2]))                    # [p,w,s,b] -> [p,b,t,v]
    else:
        t2 = _td(G, _td(x, O, (1, 2)), ([1, 2], [2, 0]))                    # [a,b,w,t,v] -> [p,b,t,v]
    return _td(t2, R, ([1, 3], [0, 1]))


def tl(V, A, O, Ab, order=1):
    """out[q,v,b] = sum V[p,w,a] A[a,s,b] O[w,t,s,v] Ab[p,t,q]; order 1: (a)(w s)(p t), order 2: (s)(w a)(p t)"""
    if order == 1:
        t2 = _td(_td(V, A, (2, 0)), O, ([1, 2], [0, 2]))                    # [p,b,t,v]
    else:
        t2 = _td(V, _td(A, O, (1, 2)), ([1, 2], [2, 0]))
    return _td(Ab, t2, ([0, 1], [0, 2])).transpose(0, 2, 1)


def tr(V, A, O, Ab, order=1):
    """out[a,w,p] = sum A[a,s,b] V[b,v,q] O[w,t,s,v] Ab[p,t,q]; order 1: (q)(t v)(s b), order 2: (s)(b v)(t q),
    order 3 (ket first, the order of the pair transfer): (b)(v s)(t q)"""
    if order == 3:
        r2 = _td(_td(A, V, (2, 0)), O, ([1, 2], [2, 3]))                    # [a,s,v,q] -> [a,q,w,t]
        return _td(r2, Ab, ([1, 3], [2, 1]))
    if order == 1:
        c2 = _td(_td(V, Ab, (2, 2)), O, ([3, 1], [1, 3]))                   # [b,v,p,t] -> [b,p,w,s]
        return _td(A, c2, ([1, 2], [3, 0])).transpose(0, 2, 1)
    t = _td(_td(A, O, (1, 2)), V, ([1, 4], [0, 1]))                         # [a,b,w,t,v] -> [a,w,t,q]
    return _td(t, Ab, ([2, 3], [1, 2]))


def _terms(op, t):
    """[(function, operand names)] of the terms of `op`, in the order the library adds them"""
    if op in ("dAC", "hac"):
        return [(proj, ("G", "x", "O", "R"))]
    if op == "dAC_proj":
        return [(proj, ("G", "x", "O", "Rp"))]
    if op in ("hac_axpby", "hac_blk"):
        return [(proj, ("Gs", "x", "O", "R"))]
    if op in ("tl", "tl_ex"):
        return [(tl, ("Gt", "x", "O", "Ab"))]
    if op in ("tr", "tr_ex"):
        return [(tr, ("Rt", "x", "O", "Ab"))]
    if op == "tl_pair":
        return [(tl, ("Gt", "x", "O", "Ab")), (tl, ("V2l", "A2l", "O", "Ab"))]
    if op == "tr_pair":
        return [(tr, ("Rt", "x", "O", "Ab")), (tr, ("V2r", "A2r", "O", "Ab"))]
    if op == "tl2":                      # the second terms of the pair transfers on their own (the bound takes them apart)
        return [(tl, ("V2l", "A2l", "O", "Ab"))]
    if op == "tr2":
        return [(tr, ("V2r", "A2r", "O", "Ab"))]
    raise KeyError(op)


def _depth(f, a, b, O, c, pair=False):
    """sum of the contracted extents of the three stages of one term, in the one bracket order the library has for it on
    this route (the Gaussian cases run on mode 4: nothing is folded into the right environment)"""
    Wl, d, _, Wr = O.shape
    if f is proj:                        # dAC_dense, and dAC_impl under nblk != 1: (a)(w s)(b v)
        return b.shape[0] + Wl * d + b.shape[2] * Wr
    if f is tl:                          # transfer_left_dense: (a)(w s)(p t)
        return b.shape[0] + Wl * d + c.shape[0] * d
    Dr, Drb = b.shape[2], c.shape[2]
    if pair:                             # mpsk_transfer_right_pair, ket first: (b)(v s)(t q)
        return Dr + Wr * d + d * Drb
    return Drb + Wr * d + d * Dr         # mpsk_transfer_right, bra first: (q)(v t)(s b)


def _extents(f, a, b, O, c):
    """every contracted extent of one term (the 2^50 guard)"""
    Wl, d, _, Wr = O.shape
    if f is proj:
        return [b.shape[0], Wl, d, b.shape[2], Wr]
    if f is tl:
        return [b.shape[0], Wl, d, c.shape[0], d]
    return [b.shape[2], Wr, d, c.shape[2], d]


_TERMS = {}


def evaluate(op, t, conv=_id, order=1, over=None):
    """`op` on conv(operand); over: operands that replace those of t (the wrong contractions)"""
    g = lambda k: conv(over[k] if over and k in over else t[k])
    out = None
    for f, names in _terms(op, t):
        # the longdouble terms are shared between the operations that have them (and between aliased operands)
        key = None if over or conv is _id else (f.__name__, conv.__name__, order) + tuple(id(t[k]) for k in names)
        if key is None or key not in _TERMS:
            y = f(*(g(k) for k in names), order)
            if key is not None:
                y.setflags(write=False)
                _TERMS[key] = y
        else:
            y = _TERMS[key]
        out = y if out is None else out + y
    if op == "hac_axpby":
        a0, a1 = (abs(A0), abs(A1)) if conv is _abs_hp else (A0, A1)
        out = a0 * g("x") + a1 * out
    return out


def _single(op):
    """the single-term operations whose terms make up `op`"""
    return {"tl_pair": ("tl", "tl2"), "tr_pair": ("tr", "tr2"), "hac_axpby": ("hac_blk",)}.get(op, (op,))


def bound(op, t):
    """the componentwise bound of the module docstring, in longdouble"""
    ts = [(evaluate(o, t, _abs_hp), _depth(f, *(t[k] for k in names), pair=op == "tr_pair")) for o, (f, names) in zip(_single(op), _terms(op, t))]
    if op == "hac_axpby":
        (y, dep), = ts
        return (dep + 10) * LD(U) * (abs(A1) * y + abs(A0) * _abs_hp(t["x"]))
    b = sum((dep + 8) * LD(U) * y for y, dep in ts)
    return b + (len(ts) * LD(U) * sum(y for y, _ in ts) if len(ts) > 1 else 0)


def magnitude(op, t):
    """sum over the terms of prod(max|operand|) prod(contracted extents) (hac_axpby: |a1| times it plus |a0| max|x|)"""
    m = sum(ei.magnitude([t[k] for k in names], _extents(f, *(t[k] for k in names))) for f, names in _terms(op, t))
    if op == "hac_axpby":
        m = abs(A1) * m + abs(A0) * ei.magnitude([t["x"]], [])
    assert m < ei.LIMIT, f"{t['name']}-{op}: worst-case magnitude {m:.3e} is not below 2^50"
    return m


def work(op, t):
    """multiply-adds of the left-first order of all terms, as the LD_MAX_WORK budget counts them"""
    Wl, d, _, Wr = t["O"].shape
    w = 0
    for f, names in _terms(op, t):
        a, b, _, c = (t[k] for k in names)
        if f is tr:                      # (q): Dr Wr Drb (Dlb d); the MPO; (s b): Dl (d Dr) (Wl Dlb)
            Dl, Dr, Dlb, Drb = b.shape[0], b.shape[2], c.shape[0], c.shape[2]
            w += Dr * Wr * Drb * Dlb * d + Dr * Dlb * Wl * Wr * d * d + Dl * d * Dr * Wl * Dlb
        else:                            # (a): rows Wl Dk (d Nb); the MPO; (b v) or (p t): rows d Nb Wr out
            rows, Dk, Nb, out = a.shape[0], b.shape[0], b.shape[2], c.shape[2]
            w += rows * Wl * Dk * d * Nb + rows * Nb * Wl * Wr * d * d + rows * d * Nb * Wr * out
    return w


def nblks(t):
    return [n for n in NBLK if t["x"].shape[0] % n == 0]


def applies(op, t):
    """whether the site has the operation: hac_blk needs an nblk that divides Dl"""
    return bool(nblks(t)) if op == "hac_blk" else True


_REFS = {}


def ref(op, t):
    """the reference of `op` on site t (exact: fp64, left-first; Gaussian: longdouble), evaluated once"""
    k = (t["name"], _terms(op, t)[0][1], len(_terms(op, t)), op == "hac_axpby")
    if k not in _REFS:
        r = evaluate(op, t, _hp if t["kind"] == "gauss" else _id)
        r.setflags(write=False)
        if t["kind"] == "int":
            magnitude(op, t)
        _REFS[k] = r
    return _REFS[k]


@functools.lru_cache(maxsize=None)
def _bound(op, name):
    return bound(op, _SITES[name])


def bound_of(op, t):
    """None for an exact case, else the bound (evaluated once per operation that shares it)"""
    if t["kind"] == "int":
        return None
    return _bound({"hac": "dAC", "hac_blk": "hac_blk", "tl_ex": "tl", "tr_ex": "tr"}.get(op, op), t["name"])


# ------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------
def is_generic(O):
    """not symmetric under s <-> t, under w <-> v (where Wl == Wr), or under reversal of any index of extent > 1"""
    if np.array_equal(O, np.swapaxes(O, 1, 2)) and O.shape[1] > 1:
        return False
    if O.shape[0] == O.shape[3] > 1 and np.array_equal(O, O.transpose(3, 1, 2, 0)):
        return False
    return not any(O.shape[ax] > 1 and np.array_equal(O, np.flip(O, ax)) for ax in range(4))


def zero_levels(slc, zeros):
    """(input levels w, output levels v) that the structured-zero kind plants"""
    if zeros in ("", "all"):
        return [], []
    z = ZERO_SLICES[slc]
    return ([z["w"]] if zeros in ("w0", "both") else []), ([z["v"]] if zeros in ("v0", "both") else [])


@functools.lru_cache(maxsize=None)
def dense_O(slc, kind="int", zeros=""):
    """the dense tensor of a slice shape: drawn once per (shape, kind, zeros), whatever the bonds.  Every (w, v) pair of
    levels that is not planted zero holds a non-zero, and the tensor is generic (is_generic) apart from the planted levels."""
    Wl, Wr, d = slc
    rng = _rng(f"dense-O-{slc}-{kind}-{zeros}")
    if zeros == "all":
        O = np.zeros((Wl, d, d, Wr))
        O.setflags(write=False)
        return O
    zw, zv = zero_levels(slc, zeros)
    while True:
        O = (int_array if kind == "int" else gauss_array)(rng, Wl, d, d, Wr)
        O[zw] = 0.0
        O[..., zv] = 0.0
        pairs = np.abs(O).max(axis=(1, 2)) > 0
        pairs[zw] = True
        pairs[:, zv] = True
        if is_generic(O) and pairs.all():
            break
    O.setflags(write=False)
    return O


_SITES = {}


@functools.lru_cache(maxsize=None)
def site(slc, bonds, kind="int", zeros="", aux=None):
    """O and the operands of every operation at slice shape slc = (Wl, Wr, d) and bonds = (Dl, Dr); aux: the other six
    bonds (default AUX[bonds]).  Built once, shared, never modified."""
    Wl, Wr, d = slc
    Dl, Dr = bonds
    Dlo, Dro, Dlb, Drb, Dl2, Dr2 = aux or AUX[bonds]
    name = f"dense-{Wl}x{Wr}x{d}-{Dl}x{Dr}-{kind}{'-' + zeros if zeros else ''}{'-aux' + 'x'.join(map(str, aux)) if aux else ''}"
    rng = _rng(name)
    base = functools.partial(int_array if kind == "int" else gauss_array, rng)
    if bonds == (1, 1) and kind == "int":                   # single-element slabs: none may be zero
        draw = lambda *shp: (lambda a: np.where(a == 0, 1.0, a))(base(*shp))
    else:
        draw = base
    t = {"name": name, "kind": kind, "slc": slc, "bonds": bonds, "zeros": zeros, "O": dense_O(slc, kind, zeros), "chil": [Wl],
         "chir": [Wr], "dims": dict(Dl=Dl, Dr=Dr, Dlo=Dlo, Dro=Dro, Dlb=Dlb, Drb=Drb, Dl2=Dl2, Dr2=Dr2)}
    t.update(G=draw(Dlo, Wl, Dl), Gs=draw(Dl, Wl, Dl), R=draw(Dr, Wr, Dr), Rp=draw(Dr, Wr, Dro), x=draw(Dl, d, Dr),
             Gt=draw(Dlb, Wl, Dl), Rt=draw(Dr, Wr, Drb), Ab=draw(Dlb, d, Drb), V2l=draw(Dlb, Wl, Dl2), A2l=draw(Dl2, d, Dr),
             V2r=draw(Dr2, Wr, Drb), A2r=draw(Dl, d, Dr2))
    if Dlo == Dl:
        t["Gs"] = t["G"]                                     # square bonds: the square left environment is G itself,
    if Dro == Dr:
        t["Rp"] = t["R"]                                     # and the projection's right environment is R
    for k in ("G", "Gs", "R", "Rp", "Gt", "Rt", "V2l", "V2r"):
        assert np.abs(t[k]).max(axis=(0, 2)).min() > 0 or Dl * Dr == 1, name       # every slab, read or not, is non-zero
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _SITES[name] = t
    return t


OPERANDS = ("G", "Gs", "R", "Rp", "x", "Gt", "Rt", "Ab", "V2l", "A2l", "V2r", "A2r")
ENVS = ("G", "Gs", "R", "Rp", "Gt", "Rt", "V2l", "V2r")


def oracle_slice(t):
    import mpskit_oracle as mo
    Wl, d, _, Wr = t["O"].shape
    return mo.SparseMPOSlice(1, d, [Wl], [Wr], {(0, 0): np.array(t["O"])} if t["O"].any() else {})


# ------------------------------------------------------------------------------------------------------------------
# case lists: (slc, bonds, zeros)
# ------------------------------------------------------------------------------------------------------------------
def sites_exact():
    """every generic integer site: each slice shape at each of its bonds"""
    return [(s, b, "") for s in SLICES for b in (BONDS_WORKLOAD if s == WORKLOAD else BONDS)]


def sites_zero():
    return [(s, b, z) for s, v in ZERO_SLICES.items() for b in v["bonds"] for z in ZEROS]


def sites_blk():
    """hac_blk alone: (66, 33) takes nblk = 2 and 3"""
    return [(s, BLK_BONDS, "") for s in RECT]


def sites_tiles():
    """the sites that run on each of the four forced tiles and on the automatic one"""
    return [(s, b, "") for s in RECT for b in ((7, 13), (65, 33))] + [(WORKLOAD, (64, 64), "")]


def sites_ragged():
    """the ragged sites that also run on the mix route of the same slice (MPSK_DENSE_ROUTE=0)"""
    return [(s, b, "") for s in RECT for b in ((7, 13), (65, 33))] + [c for c in sites_zero() if c[0] == (5, 3, 3)]


def sites_pair():
    """the sites of the pair transfers: both rectangular slices on the ragged bonds, the workload on (7, 13)"""
    return [(s, b, "") for s in RECT for b in ((7, 13), (65, 33))] + [(WORKLOAD, (7, 13), "")]


def ops_of(c):
    """the operations that run on site c"""
    t = site(c[0], c[1], "int", c[2])
    if c[1] == BLK_BONDS:
        return ["hac_blk"]
    pair = (c[0], c[1], "") in sites_pair() and not c[2]
    return [op for op in OPS if applies(op, t) and (pair or op not in ("tl_pair", "tr_pair"))]


def subcases_exact():
    """(op, slc, bonds, zeros) of every exact sub-case"""
    return [(op,) + c for c in sites_exact() + sites_zero() + sites_blk() for op in ops_of(c)]


def site_id(c):
    s, b, z = c
    return f"{s[0]}x{s[1]}x{s[2]}-{b[0]}x{b[1]}{'-' + z if z else ''}"


def sub_id(c):
    return f"{c[0]}-{site_id(c[1:])}"


def gauss_site(slc, bonds, op):
    """the Gaussian site of `op`: hac_blk on the (5, 3, 3) slice moves to (66, 33), where nblk = 2 and 3 divide Dl"""
    if op == "hac_blk" and bonds == (65, 33):
        bonds = BLK_BONDS
    return site(slc, bonds, "gauss")


# ------------------------------------------------------------------------------------------------------------------
# plausible wrong contractions of the dense route
# ------------------------------------------------------------------------------------------------------------------
# name -> (what it models, the exact sub-cases it applies to)
WRONG = {
    "sw_as_ws": ("(s, w) read as (w, s) in the T1 column index z = s + d w", "every op; Wl > 1 and d > 1, O != 0"),
    "left_tab_right": ("dense_tab: the left table (z / d, z % d) used on the right side", "tr_pair; Wr == d, O != 0"),
    "O_st_swapped": ("O with s and t exchanged", "every op; O != 0"),
    "O_wv_swapped": ("O with w and v exchanged", "every op; Wl == Wr > 1, O != 0"),
    "last_v_dropped": ("last level v dropped", "every op; O[..., Wr - 1] != 0"),
    "last_sw_dropped": ("last (s, w) column of T1 dropped: a K-tail of stage 2", "every op; O[Wl - 1, :, d - 1, :] != 0"),
    "last_ktile_dropped": ("last k-tile of stage 2 dropped (K = d Wl, depth 16)", "every op; d Wl > 16, those rows of Od != 0"),
    "first_level_twice": ("first level v counted twice", "every op; O[..., 0] != 0"),
    "GR_transposed": ("the slabs of the right environment transposed", "ops with a square right environment; D > 1, O != 0"),
    "Ab_untransposed": ("Ab not transposed in stage 3 of the left transfer", "tl, tl_ex; Dlb == Drb > 1, O != 0 (no pair site is square)"),
    "zero_from_neighbour": ("a zero level not skipped but read from the neighbouring level", "every op; zeros v0, w0, both"),
    "beta_on_product": ("beta (a0) applied to the product term", "hac_axpby; O != 0"),
}


def wrong(op, t, how):
    """`op` on site t with one plausible mistake; None when the mistake does not apply"""
    O = t["O"]
    Wl, d, _, Wr = O.shape
    if not O.any():
        return None                                          # O == 0: every contraction is zero, nothing to tell apart
    over = {}
    if how == "sw_as_ws":                                    # column z holds (w', s') with z = w' + Wl s'
        z = np.arange(Wl)[:, None] + Wl * np.arange(d)[None, :]
        over["O"] = O[z // d, :, z % d, :].transpose(0, 2, 1, 3)
    elif how == "left_tab_right":                            # column z = s + d v read as (s', v') = (z / d, z % d)
        if op != "tr_pair" or Wr != d:
            return None
        over["O"] = O.transpose(0, 1, 3, 2)
    elif how == "O_st_swapped":
        over["O"] = np.swapaxes(O, 1, 2)
    elif how == "O_wv_swapped":
        if Wl != Wr:
            return None
        over["O"] = O.transpose(3, 1, 2, 0)
    elif how in ("last_v_dropped", "last_sw_dropped", "last_ktile_dropped", "first_level_twice"):
        Ow = O.copy()
        if how == "last_v_dropped":
            Ow[..., -1] = 0
        elif how == "last_sw_dropped":
            Ow[-1, :, -1, :] = 0
        elif how == "first_level_twice":
            Ow[..., 0] *= 2
        else:
            K = d * Wl
            if K <= GEMM_BK:
                return None
            z = np.arange((K - 1) // GEMM_BK * GEMM_BK, K)
            Ow[z // d, :, z % d, :] = 0
        over["O"] = Ow
    elif how == "GR_transposed":
        k = {proj: 3, tr: 0}.get(_terms(op, t)[0][0])
        if k is None or len(_terms(op, t)) > 1:
            return None
        k = _terms(op, t)[0][1][k]
        if t[k].shape[0] != t[k].shape[2] or t[k].shape[0] == 1:
            return None
        over[k] = np.swapaxes(t[k], 0, 2)
    elif how == "Ab_untransposed":
        if _terms(op, t)[0][0] is not tl or t["Ab"].shape[0] != t["Ab"].shape[2] or t["Ab"].shape[0] == 1:
            return None
        over["Ab"] = np.swapaxes(t["Ab"], 0, 2)
    elif how == "zero_from_neighbour":
        zw, zv = zero_levels(t["slc"], t["zeros"])
        if not zw and not zv:
            return None
        Ow = O.copy()
        for w in zw:
            Ow[w] = O[w + 1]
        for v in zv:
            Ow[..., v] = O[..., v + 1]
        over["O"] = Ow
    elif how == "beta_on_product":
        if op != "hac_axpby":
            return None
        return A0 * t["x"] + A0 * evaluate("hac_blk", t)
    else:
        raise KeyError(how)
    if "O" in over and np.array_equal(over["O"], O):
        return None
    return evaluate(op, t, over=over)
