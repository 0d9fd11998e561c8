"""Exact cases for the entry points behind approximate / VOMPS / changebonds / multiline / the multi-GPU path: the
rectangular projections (dC_proj, dAC_proj, dAC2_proj), the factorised two-site product (dAC2_product), the complex dAC2
and dC, the blocked vector layout (dAC_blocked, hac_apply(nblk)), the transfers whose bra tensor has other bonds than the
ket tensor (with a slice and as W pass-through slabs) and regularize.  Same rules as tests/exact_inputs.py, which this
module reuses as it stands: integer-valued operands whose every partial sum stays below 2^50 (asserted per case), so fp64
never rounds and the comparison is np.array_equal; one Gaussian case per operation inside the componentwise bound

    |got - ref| <= (4 if complex else 1) * (depth + 2 n_stages + 2) * u * contract(|operands|)

in longdouble, where depth is the sum of the contracted extents of the stages (the maximum over the bracket orders the
library has for the entry point, `depth()` names each) and every stage boundary gets two roundings of slack.

Every operation is ONE plain pairwise np.einsum(optimize=False) contraction, `contract(op, t, conv)`: conv = _hp gives
the longdouble reference, conv = _abs_hp the right-hand side of the bound, and without conv it is the fp64 reference of
the integer cases.  `wrong(op, t, how)` evaluates a list of plausible WRONG contractions on the same operands;
tests/test_exact_proj_inputs_cpu.py checks that each differs from the reference, i.e. that the inputs can tell a subtly
wrong kernel from a right one.

Shapes.  Ragged: (Dlo, Dl, Dm, Dr, Dro) = (20, 33, 17, 65, 48), pairwise distinct and mostly odd, chis (1, 3, 2, 1),
d1 = 2 != d2 = 3, so no swapped stride or extent passes.  Aligned: (64, 128, 64, 128, 64), five levels of chi 1, d = 2:
every extent a multiple of 64 and every leading dimension even (aligned loaders, the VEC2 branch of the slab mix)."""
from __future__ import annotations

import functools

import numpy as np

import exact_inputs as ei
from exact_inputs import LD, U, _abs_hp, _hp, _rng, assert_exact_range, gauss_array, int_array, rand_slice

RAGGED = dict(Dlo=20, Dl=33, Dm=17, Dr=65, Dro=48, chis=(1, 3, 2, 1), d1=2, d2=3, tag="ragged")
ALIGNED = dict(Dlo=64, Dl=128, Dm=64, Dr=128, Dro=64, chis=(1, 1, 1, 1, 1), d1=2, d2=2, tag="aligned")
# the transfers: (Dl, Dr) of A, (Dlb, Drb) of Ab, Dlb != Dl and Drb != Dr
MIXED = {"ragged": dict(Dl=33, Dr=65, Dlb=20, Drb=48), "aligned": dict(Dl=128, Dr=64, Dlb=64, Drb=128)}
# the blocked vector layout: (nblk, Dl, Dr, chis, d)
BLOCKED = {"nblk2": dict(nblk=2, Dl=128, Dr=64, chis=(1, 1, 1, 1, 1), d=2), "nblk3": dict(nblk=3, Dl=33, Dr=65, chis=(1, 3, 2, 1), d=2)}
REG = {"ragged": (33, 65), "aligned": (128, 64)}        # regularize: slabs [D1, D2]
PASS_W = 3                                              # pass-through transfers: W independent slabs
DENSE_W, DENSE_D = ei.DENSE_W, ei.DENSE_D
DEGENERATE_CHIS, DEGENERATE_D = (1, 2, 1, 2, 1), 2
MAXSEG = 32                                             # mpsk_internal.h: K-segments of one GEMM launch
TINY = (6, 10)                                          # (Dl, Dr) of the cases that only probe the segment count

_e = functools.partial(np.einsum, optimize=False)


def _id(a):
    return np.asarray(a)


def _stack(env):
    return np.concatenate([np.asarray(x) for x in env], axis=1)         # list of [Db, chi, Dk] -> [Db, W, Dk]


def _unstack(G, chis):
    out, o = [], 0
    for c in chis:
        out.append(G[:, o:o + c, :])
        o += c
    return out


# ------------------------------------------------------------------------------------------------------------------
# the blocked vector layout of mpsk_dAC_blocked / mpsk_hac_apply(nblk)
# ------------------------------------------------------------------------------------------------------------------
def to_blocks(x, nblk):
    """x[Dl, d, Dr] -> the flat vector of its nblk row blocks, block q = x[q n:(q + 1) n] stored as a contiguous
    column-major [n, d, Dr] tensor at offset q n d Dr (include/mpsk.h, mpsk_dAC_blocked)"""
    Dl = x.shape[0]
    assert Dl % nblk == 0
    n = Dl // nblk
    return np.concatenate([np.ravel(x[q * n:(q + 1) * n], order="F") for q in range(nblk)])


def from_blocks(flat, nblk, shape):
    Dl = shape[0]
    n = Dl // nblk
    size = n * int(np.prod(shape[1:]))
    return np.concatenate([flat[q * size:(q + 1) * size].reshape((n,) + tuple(shape[1:]), order="F") for q in range(nblk)], axis=0)


# ------------------------------------------------------------------------------------------------------------------
# contractions
# ------------------------------------------------------------------------------------------------------------------
def contract(op, t, conv=_id):
    """Operation `op` on conv(operand), as plain pairwise einsums.  G / R: stacked environments [Db, W, Dk]; O / O2: the
    dense [Wl, d, d, Wr] form of the slices, index order [w, t(out), s(in), v].  The transfers come back stacked over
    levels, [Drb, Wr, Dr] and [Dl, Wl, Dlb]."""
    g = lambda k: conv(t[k])
    cj = _id if conv is _abs_hp else np.conj                    # |conj(z)| = |z|: the bound needs no conjugate
    if op in ("dC", "dC_proj"):                                  # y[p,q] = sum_w GL[w][p,a] c[a,b] GR[w][b,q]
        return _e("pwb,bwq->pq", _e("pwa,ab->pwb", g("G"), g("x")), g("R"))
    if op in ("dAC", "dAC_proj", "dAC_blocked", "hac_blocked"):  # y[p,t,q] = sum GL[w][p,a] x[a,s,b] O[w,t,s,v] GR[v][b,q]
        t1 = _e("pwa,asb->pwsb", g("G"), g("x"))
        return _e("pbtv,bvq->ptq", _e("pwsb,wtsv->pbtv", t1, g("O")), g("R"))
    if op == "dAC2":                                             # x2[a,s1,b,s2] -> y2[p,t1,q,t2]
        t1 = _e("pwsbr,wtsu->ptubr", _e("pwa,asbr->pwsbr", g("G"), g("x")), g("O"))
        return _e("ptbzv,bvq->ptqz", _e("ptubr,uzrv->ptbzv", t1, g("O2")), g("R"))
    if op in ("dAC2_proj", "dAC2_product"):                      # the two factors AC[a,s1,m], AR[m,s2,b]; Y[p,t1,q,t2]
        lh = _e("pwsm,wtsu->ptum", _e("pwa,asm->pwsm", g("G"), g("AC")), g("O"))
        rh = _e("uzrv,mrvq->umzq", g("O2"), _e("mrb,bvq->mrvq", g("AR"), g("R")))
        return _e("ptum,umzq->ptqz", lh, rh)
    if op == "tl":                                               # GLout[v][q,b] = sum GLin[w][p,a] A[a,s,b] O[w,t,s,v] conj(Ab[p,t,q])
        t2 = _e("pwsb,wtsv->pbtv", _e("pwa,asb->pwsb", g("G"), g("A")), g("O"))
        return _e("ptq,pbtv->qvb", cj(g("Ab")), t2)
    if op == "tr":                                               # GRout[w][a,p] = sum A[a,s,b] O[w,t,s,v] conj(Ab[p,t,q]) GRin[v][b,q]
        t1 = _e("bvq,ptq->bvpt", g("R"), cj(g("Ab")))
        return _e("asb,wsbp->awp", g("A"), _e("wtsv,bvpt->wsbp", g("O"), t1))
    if op == "tl0":                                              # H == NULL: W pass-through slabs
        return _e("psq,pwsb->qwb", cj(g("Ab")), _e("pwa,asb->pwsb", g("G"), g("A")))
    if op == "tr0":
        return _e("asb,bwps->awp", g("A"), _e("bwq,psq->bwps", g("R"), cj(g("Ab"))))
    if op == "reg":                                              # v[w] -= <lvec^T, v[w]> rvec; v stacked [D1, W, D2]
        coef = _e("xy,ywx->w", g("lvec"), g("v"))
        upd = _e("w,pq->pwq", coef, g("rvec"))
        return g("v") + upd if conv is _abs_hp else g("v") - upd
    raise KeyError(op)


def depth(op, t):
    """(sum of the contracted extents of the stages, number of stages): the larger over the bracket orders that
    mpsk_api.hip has for the entry point; complex extents count complex elements (the factor 4 covers the rest)."""
    if op in ("dC", "dC_proj"):          # dC_f64 / dC_c128: stage1 (a), then one segmented GEMM over (w b)
        Dl, Dr = t["x"].shape
        return Dl + t["G"].shape[1] * Dr, 2
    if op in ("dAC", "dAC_proj", "dAC_blocked", "hac_blocked"):
        # dAC_impl / dAC_dense / dAC_c128, left first: (a)(w s)(b v).  mpsk_hac_apply in mode 1 folds the slice into the
        # right environment when the operator is created: (v)(a)(w s b)
        Wl, d, _, Wr = t["O"].shape
        Dl, _, Dr = t["x"].shape
        if op == "hac_blocked":
            return max(Dl + Wl * d + Dr * Wr, Wr + Dl + Wl * d * Dr), 3
        return Dl + Wl * d + Dr * Wr, 3
    if op in ("dAC2", "dAC2_proj", "dAC2_product"):
        Wl, d1, _, Wm = t["O"].shape
        _, d2, _, Wr = t["O2"].shape
        if op == "dAC2" or t["cplx"]:
            # dAC2_c128: (a), the pair plan folds O1 O2 over u on the host (pair_plan) and mixes (w s1 s2) in one pass,
            # then (b v).  The complex mpsk_dAC2_proj builds theta = AC AR first: one more stage over m.
            Dl, Dr = (t["x"].shape[0], t["x"].shape[2]) if op == "dAC2" else (t["AC"].shape[0], t["AR"].shape[2])
            dd, n = Dl + (Wm + Wl * d1 * d2) + Dr * Wr, 4
            return (dd + t["AC"].shape[2], n + 1) if op != "dAC2" else (dd, n)
        # dAC2_factorised: the halves (a)(w s1) and (b v)(s2) round independently and meet in one GEMM over (u m)
        Dl, _, Dm = t["AC"].shape
        Dr = t["AR"].shape[2]
        return (Dl + Wl * d1) + (Dr + Wr * d2) + Wm * Dm, 5
    Dl, d, Dr = t["A"].shape
    Dlb, _, Drb = t["Ab"].shape
    if op == "tl":                       # transfer_left_f64 / _dense / _c128: (a)(w s)(p t)
        return Dl + t["O"].shape[0] * d + Dlb * d, 3
    if op == "tr":                       # mpsk_transfer_right: (q)(v t)(s b)   |   transfer_right_c128: (b)(v s)(t q)
        Wr = t["O"].shape[3]
        return max(Drb + Wr * d + d * Dr, Dr + Wr * d + d * Drb), 3
    if op == "tl0":                      # the same without the mix
        return Dl + Dlb * d, 2
    if op == "tr0":
        return max(Drb + d * Dr, Dr + d * Drb), 2
    raise KeyError(op)


CONTRACTED = {           # every contracted index of the operation, by the names used in `_extents`
    "dC": "Dl W Dr", "dC_proj": "Dl W Dr", "dAC": "Dl Wl d1 Dr Wr", "dAC_proj": "Dl Wl d1 Dr Wr", "dAC_blocked": "Dl Wl d1 Dr Wr",
    "hac_blocked": "Dl Wl d1 Dr Wr", "dAC2": "Dl Wl d1 Wm d2 Dr Wr", "dAC2_proj": "Dl Wl d1 Dm Wm d2 Dr Wr",
    "dAC2_product": "Dl Wl d1 Dm Wm d2 Dr Wr", "tl": "Dl Wl d1 Dlb d1", "tr": "Dr Wr d1 Drb d1", "tl0": "Dl Dlb d1", "tr0": "Dr Drb d1",
    "reg": "D1 D2"}
OPERANDS = ("G", "R", "x", "AC", "AR", "A", "Ab", "O", "O2", "v", "lvec", "rvec")


def _finish(op, t, kind, cplx, ext):
    """reference, bound and the 2^50 guard of a case whose operands are in place"""
    t["op"], t["kind"], t["cplx"] = op, kind, cplx
    operands = [t[k] for k in OPERANDS if k in t]
    if kind == "int":
        # every contracted index; a product of n complex factors is 2^(n-1) real terms: a factor 2 per complex operand
        t["magnitude"] = assert_exact_range(operands, [ext[k] for k in CONTRACTED[op].split()] + [2 if cplx else 1] * len(operands),
                                            t["name"])
        t["ref"], t["bound"] = contract(op, t), None
    else:
        dd, n = (ext["D1"] * ext["D2"], 2) if op == "reg" else depth(op, t)     # reg: the dot over (D1 D2), then the update
        t["ref"] = contract(op, t, _hp)
        t["bound"] = (4 if cplx else 1) * (dd + 2 * n + 2) * LD(U) * contract(op, t, _abs_hp)
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


def _slice(rng, chis, d, kind, cplx, dense=False):
    import mpskit_oracle as mo
    draw = int_array if kind == "int" else gauss_array
    if dense:
        return mo.SparseMPOSlice(1, DENSE_D, [DENSE_W], [DENSE_W], {(0, 0): draw(rng, DENSE_W, DENSE_D, DENSE_D, DENSE_W, cplx=cplx)})
    return rand_slice(rng, len(chis), d, chis, draw, cplx=cplx)


@functools.lru_cache(maxsize=None)
def case(op, shape="ragged", kind="int", cplx=False, variant="", W=3):
    """Operands, reference and bound (None: exact) of one case; built once, shared, never modified.
    shape: "ragged" / "aligned" (blocked: "nblk2" / "nblk3").  variant: "" sparse slice, "dense" one dense MPO tensor
    [4, 2, 2, 4].  W: slabs of the slice-less operations (dC_proj, dC, tl0, tr0, reg)."""
    name = f"{op}-{shape}-{variant or 'sparse'}-{kind}-{'c128' if cplx else 'f64'}-W{W}"
    rng = _rng(name)
    draw = functools.partial(int_array if kind == "int" else gauss_array, cplx=cplx)
    dense = variant == "dense"
    t = {"name": name, "dense": dense}
    if op == "reg":
        D1, D2 = REG[shape]
        t.update(v=draw(rng, D1, W, D2), lvec=draw(rng, D2, D1), rvec=draw(rng, D1, D2), chis=[1] * W)
        return _finish(op, t, kind, cplx, dict(D1=D1, D2=D2))
    if op in ("dAC_blocked", "hac_blocked"):
        b = BLOCKED[shape]
        chis, d, Dl, Dr, nblk = b["chis"], b["d"], b["Dl"], b["Dr"], b["nblk"]
        s = _slice(rng, chis, d, kind, cplx)
        W_ = sum(chis)
        t.update(s=s, O=s.full(), chis=list(chis), nblk=nblk, G=draw(rng, Dl, W_, Dl), R=draw(rng, Dr, W_, Dr), x=draw(rng, Dl, d, Dr))
        return _finish(op, t, kind, cplx, dict(Dl=Dl, Dr=Dr, Wl=W_, Wr=W_, d1=d))
    if op in ("tl", "tr", "tl0", "tr0"):
        m = MIXED[shape]
        Dl, Dr, Dlb, Drb = m["Dl"], m["Dr"], m["Dlb"], m["Drb"]
        chis, d = ((RAGGED if shape == "ragged" else ALIGNED)["chis"], 2) if not dense else ((DENSE_W,), DENSE_D)
        if op in ("tl0", "tr0"):
            chis = (1,) * W
        else:
            s = _slice(rng, chis, d, kind, cplx, dense)
            t.update(s=s, O=s.full())
        W_ = sum(chis)
        t.update(chis=list(chis), A=draw(rng, Dl, d, Dr), Ab=draw(rng, Dlb, d, Drb))
        if op in ("tl", "tl0"):
            t["G"] = draw(rng, Dlb, W_, Dl)
        else:
            t["R"] = draw(rng, Dr, W_, Drb)
        return _finish(op, t, kind, cplx, dict(Dl=Dl, Dr=Dr, Dlb=Dlb, Drb=Drb, Wl=W_, Wr=W_, d1=d))
    g = RAGGED if shape == "ragged" else ALIGNED
    Dlo, Dl, Dm, Dr, Dro, chis, d1, d2 = (g[k] for k in ("Dlo", "Dl", "Dm", "Dr", "Dro", "chis", "d1", "d2"))
    if op in ("dC", "dC_proj"):
        if op == "dC":
            Dro = Dr                                             # mpsk_dC: GR slabs are square
        t.update(G=draw(rng, Dlo, W, Dl), R=draw(rng, Dr, W, Dro), x=draw(rng, Dl, Dr), chis=[1] * W)
        return _finish(op, t, kind, cplx, dict(Dl=Dl, Dr=Dr, W=W))
    if dense:
        chis, d1, d2 = (DENSE_W,), DENSE_D, DENSE_D
    W_ = sum(chis)
    s = _slice(rng, chis, d1, kind, cplx, dense)
    t.update(s=s, O=s.full(), chis=list(chis))
    ext = dict(Dl=Dl, Dm=Dm, Dr=Dr, Wl=W_, Wm=W_, Wr=W_, d1=d1, d2=d2)
    if op == "dAC_proj":
        t.update(G=draw(rng, Dlo, W_, Dl), R=draw(rng, Dr, W_, Dro), x=draw(rng, Dl, d1, Dr))
        return _finish(op, t, kind, cplx, ext)
    s2 = _slice(rng, chis, d2, kind, cplx, dense)
    t.update(s2=s2, O2=s2.full())
    if op == "dAC2":                                             # mpsk_dAC2: Dlo rows of GL, square GR
        t.update(G=draw(rng, Dlo, W_, Dl), R=draw(rng, Dr, W_, Dr), x=draw(rng, Dl, d1, Dr, d2))
    elif op == "dAC2_proj":
        t.update(G=draw(rng, Dlo, W_, Dl), R=draw(rng, Dr, W_, Dro), AC=draw(rng, Dl, d1, Dm), AR=draw(rng, Dm, d2, Dr))
    elif op == "dAC2_product":                                   # square environments
        t.update(G=draw(rng, Dl, W_, Dl), R=draw(rng, Dr, W_, Dr), AC=draw(rng, Dl, d1, Dm), AR=draw(rng, Dm, d2, Dr))
    else:
        raise KeyError(op)
    return _finish(op, t, kind, cplx, ext)


def cases_exact():
    """(op, shape, cplx, variant, W) of every integer case of section 1; each runs on the four forced tiles and on the
    automatic one (regularize has no GEMM and no tile: it runs once)"""
    out = []
    for shp in ("ragged", "aligned"):
        out += [("dC_proj", shp, False, "", W) for W in (1, 3)]
        out += [("dAC_proj", shp, True, "", 0), ("dAC_proj", shp, False, "dense", 0)]
        out += [("dAC2_proj", shp, False, "", 0), ("dAC2_proj", shp, True, "", 0), ("dAC2_proj", shp, False, "dense", 0)]
        out += [("dAC2_product", shp, False, "", 0), ("dAC2_product", shp, False, "dense", 0)]
        out += [("dAC2", shp, True, "", 0), ("dC", shp, True, "", 3)]
        for op in ("tl", "tr"):
            out += [(op, shp, False, "", 0), (op, shp, True, "", 0), (op, shp, False, "dense", 0)]
            out += [(op + "0", shp, False, "", PASS_W), (op + "0", shp, True, "", PASS_W)]
    out += [(op, shp, False, "", 0) for op in ("dAC_blocked", "hac_blocked") for shp in ("nblk2", "nblk3")]
    return out


def reg_cases():
    return [("reg", shp, False, "", W) for shp in ("ragged", "aligned") for W in (1, 3)]


def cases_gauss():
    """one Gaussian case per operation (and dtype / slice kind of the table), all on the ragged shape"""
    out = [("dC_proj", "ragged", False, "", 3), ("dAC_proj", "ragged", True, "", 0), ("dAC_proj", "ragged", False, "dense", 0),
           ("dAC2_proj", "ragged", False, "", 0), ("dAC2_proj", "ragged", True, "", 0), ("dAC2_proj", "ragged", False, "dense", 0),
           ("dAC2_product", "ragged", False, "", 0), ("dAC2_product", "ragged", False, "dense", 0),
           ("dAC2", "ragged", True, "", 0), ("dC", "ragged", True, "", 3),
           ("dAC_blocked", "nblk3", False, "", 0), ("hac_blocked", "nblk3", False, "", 0)]
    for op in ("tl", "tr"):
        out += [(op, "ragged", False, "", 0), (op, "ragged", True, "", 0), (op, "ragged", False, "dense", 0),
                (op + "0", "ragged", False, "", PASS_W), (op + "0", "ragged", True, "", PASS_W)]
    return out + [("reg", "ragged", False, "", 3)]


def case_id(c):
    op, shape, cplx, variant, W = c
    return f"{op}-{shape}{'-' + variant if variant else ''}-{'c128' if cplx else 'f64'}{f'-W{W}' if W else ''}"


# ------------------------------------------------------------------------------------------------------------------
# degenerate slices: hand-written block tables on chis (1, 2, 1, 2, 1), d = 2
# ------------------------------------------------------------------------------------------------------------------
DEGENERATE = ("a", "b", "c", "d")
# levels (of the 7) that no block enters / that no block leaves
DEGENERATE_UNUSED = {"a": ([6], [6]), "b": ([3], [4, 5]), "c": ([], []), "d": (list(range(7)), list(range(7)))}
DEGENERATE_OPS = ("dAC", "dAC_proj", "dAC2", "dAC2_proj", "dAC2_product", "tl", "tr")


def degenerate_slice(which, cplx=False, salt=""):
    """(a) nothing enters the last level; (b) nothing enters block level 2 and nothing leaves block level 3; (c) scalar
    blocks only; (d) no blocks at all"""
    import mpskit_oracle as mo
    chis, d = DEGENERATE_CHIS, DEGENERATE_D
    rng = _rng(f"degenerate-{which}-{cplx}-{salt}")

    def D(i, j):
        while True:                                              # every (w, v) pair of a dense block holds a non-zero
            b = int_array(rng, chis[i], d, d, chis[j], cplx=cplx)
            if np.abs(b).reshape(chis[i], d * d, chis[j]).max(axis=1).min() > 0:
                return b

    if which == "a":
        blocks = {(0, 0): 1.0, (0, 1): D(0, 1), (0, 2): D(0, 2), (1, 1): 2.0, (1, 3): D(1, 3), (2, 3): D(2, 3), (0, 3): D(0, 3),
                  (2, 2): -1.0, (3, 3): 2.0}
    elif which == "b":
        blocks = {(0, 0): 1.0, (0, 1): D(0, 1), (1, 1): 3.0, (1, 3): D(1, 3), (2, 3): D(2, 3), (2, 4): D(2, 4), (0, 3): D(0, 3),
                  (1, 4): D(1, 4), (0, 4): D(0, 4), (4, 4): 1.0}
    elif which == "c":
        blocks = {(0, 0): 1.0, (0, 2): 2.0, (2, 2): -3.0, (1, 1): 2.0, (1, 3): -1.0, (3, 3): 4.0, (2, 4): 3.0, (0, 4): -2.0,
                  (4, 4): 1.0}
        if cplx:
            blocks[(1, 3)] = -1.0 + 2.0j
    elif which == "d":
        blocks = {}
    else:
        raise KeyError(which)
    return mo.SparseMPOSlice(len(chis), d, list(chis), list(chis), blocks)


def used_levels(O):
    """(col_used[Wr], row_used[Wl]) as mposlice_build derives them from the dense form"""
    nz = np.abs(O) != 0
    return nz.any(axis=(0, 1, 2)), nz.any(axis=(1, 2, 3))


@functools.lru_cache(maxsize=None)
def degenerate_case(op, which, cplx=False):
    """integer case of `op` on degenerate slice `which` (two-site operations: the same kind of slice on both sites), ragged
    bonds; the environment slabs of the unused levels are non-zero like all the others"""
    g = RAGGED
    Dlo, Dl, Dm, Dr, Dro = (g[k] for k in ("Dlo", "Dl", "Dm", "Dr", "Dro"))
    chis, d = DEGENERATE_CHIS, DEGENERATE_D
    W_ = sum(chis)
    name = f"degenerate-{which}-{op}-{'c128' if cplx else 'f64'}"
    rng = _rng(name)
    draw = functools.partial(int_array, cplx=cplx)
    s = degenerate_slice(which, cplx)
    t = {"name": name, "s": s, "O": np.asarray(s.full(), dtype=np.complex128 if cplx else np.float64), "chis": list(chis)}
    ext = dict(Dl=Dl, Dm=Dm, Dr=Dr, Wl=W_, Wm=W_, Wr=W_, d1=d, d2=d)
    if op in ("dAC2", "dAC2_proj", "dAC2_product"):
        s2 = degenerate_slice(which, cplx, salt="site2")
        t.update(s2=s2, O2=np.asarray(s2.full(), dtype=t["O"].dtype))
    if op == "dAC":
        t.update(G=draw(rng, Dlo, W_, Dl), R=draw(rng, Dr, W_, Dr), x=draw(rng, Dl, d, Dr))
    elif op == "dAC_proj":
        t.update(G=draw(rng, Dlo, W_, Dl), R=draw(rng, Dr, W_, Dro), x=draw(rng, Dl, d, Dr))
    elif op == "dAC2":
        t.update(G=draw(rng, Dlo, W_, Dl), R=draw(rng, Dr, W_, Dr), x=draw(rng, Dl, d, Dr, d))
    elif op == "dAC2_proj":
        t.update(G=draw(rng, Dlo, W_, Dl), R=draw(rng, Dr, W_, Dro), AC=draw(rng, Dl, d, Dm), AR=draw(rng, Dm, d, Dr))
    elif op == "dAC2_product":
        t.update(G=draw(rng, Dl, W_, Dl), R=draw(rng, Dr, W_, Dr), AC=draw(rng, Dl, d, Dm), AR=draw(rng, Dm, d, Dr))
    elif op in ("tl", "tr"):
        m = MIXED["ragged"]
        ext.update(Dl=m["Dl"], Dr=m["Dr"], Dlb=m["Dlb"], Drb=m["Drb"])
        t.update(A=draw(rng, m["Dl"], d, m["Dr"]), Ab=draw(rng, m["Dlb"], d, m["Drb"]))
        if op == "tl":
            t["G"] = draw(rng, m["Dlb"], W_, m["Dl"])
        else:
            t["R"] = draw(rng, m["Dr"], W_, m["Drb"])
    else:
        raise KeyError(op)
    for k in ("G", "R"):
        if k in t:
            assert np.abs(t[k]).max(axis=(0, 2)).min() > 0, name                # every slab, used or not, is non-zero
    return _finish(op, t, "int", cplx, ext)


def degenerate_cases():
    """(op, which, cplx): (a)-(d) through every operation in f64; (a) and (d) in c128 where the entry point has it
    (mpsk_dAC2_product is MPSK_F64 only)"""
    out = [(op, w, False) for op in DEGENERATE_OPS for w in DEGENERATE]
    out += [(op, w, True) for op in DEGENERATE_OPS if op != "dAC2_product" for w in ("a", "d")]
    return out


# ------------------------------------------------------------------------------------------------------------------
# more K-segments than MAXSEG
# ------------------------------------------------------------------------------------------------------------------
def long_slice(rng, W, d, cplx=False, density=0.5):
    """W levels of chi 1, upper triangular, integer fill of density ~0.5; the corners are 1 and every (i, i + 1) block is
    present, so every level has a block coming in and one going out"""
    import mpskit_oracle as mo

    def D():
        while True:
            b = int_array(rng, 1, d, d, 1, cplx=cplx)
            if np.abs(b).max() > 0 and not np.allclose(b[0, :, :, 0], b[0, 0, 0, 0] * np.eye(d)):
                return b

    blocks = {(0, 0): 1.0, (W - 1, W - 1): 1.0}
    for i in range(W):
        for j in range(i, W):
            if (i, j) not in blocks and (j == i + 1 or rng.random() < density):
                blocks[(i, j)] = D()
    return mo.SparseMPOSlice(W, d, [1] * W, [1] * W, blocks)


def rc_nseg(O):
    """K-segments per batch of the right-combined operator (mpsk_hac mode 1), as mposlice_build counts them: the largest
    number, over t, of (w, s) pairs with a non-zero O[w, t, s, :]"""
    return int((np.abs(O) != 0).any(axis=3).sum(axis=(0, 2)).max())


@functools.lru_cache(maxsize=None)
def long_case(op, W, cplx=False):
    """tiny bonds (Dlo = Dl = 6, Dr = 10), d = 2, W levels of chi 1: only the segment count is probed.
    op: dAC / tl / tr on long_slice(W); dC on W slabs."""
    Dl, Dr = TINY
    d = 2
    name = f"long-{op}-W{W}-{'c128' if cplx else 'f64'}"
    rng = _rng(name)
    draw = functools.partial(int_array, cplx=cplx)
    t = {"name": name, "chis": [1] * W}
    ext = dict(Dl=Dl, Dr=Dr, Wl=W, Wr=W, W=W, d1=d, Dlb=Dl, Drb=Dr)
    if op != "dC":
        s = long_slice(rng, W, d, cplx)
        t.update(s=s, O=s.full())
        col, row = used_levels(t["O"])
        assert col.all() and row.all(), name                     # every level is used: the segment list has W entries
    if op in ("dAC", "dC"):
        t.update(G=draw(rng, Dl, W, Dl), R=draw(rng, Dr, W, Dr), x=draw(rng, *((Dl, Dr) if op == "dC" else (Dl, d, Dr))))
    elif op == "tl":
        t.update(G=draw(rng, Dl, W, Dl), A=draw(rng, Dl, d, Dr), Ab=draw(rng, Dl, d, Dr))
    elif op == "tr":
        t.update(R=draw(rng, Dr, W, Dr), A=draw(rng, Dl, d, Dr), Ab=draw(rng, Dl, d, Dr))
    else:
        raise KeyError(op)
    return _finish(op, t, "int", cplx, ext)


def long_cases():
    """(op, W, cplx): 33 real levels = 33 segments; 17 complex levels = 34 plane segments"""
    return [("dAC", 33, False), ("tl", 33, False), ("tr", 33, False), ("dC", 33, False), ("dAC", 17, True), ("tr", 17, True)]


HAC_LONG_W = 20          # mode 1 of the prepared operator: up to Wl d = 40 segments per t from the device table


# ------------------------------------------------------------------------------------------------------------------
# plausible wrong contractions (tests/test_exact_proj_inputs_cpu.py: each must differ from the reference)
# ------------------------------------------------------------------------------------------------------------------
def _swap_ts(O):
    return np.swapaxes(O, 1, 2)


def wrong(op, t, how):
    """the contraction of `op` with one plausible mistake; None when the mistake does not apply to the case"""
    u = dict(t)
    has = lambda k: k in t
    if how == "ts_swapped":                                      # t and s swapped in O
        if not has("O"):
            return None
        u["O"] = _swap_ts(t["O"])
    elif how == "ts_swapped_site2":
        if not has("O2"):
            return None
        u["O2"] = _swap_ts(t["O2"])
    elif how == "conj_dropped":                                  # conj dropped on Ab
        if not (has("Ab") and t["cplx"]):
            return None
        u["Ab"] = np.conj(t["Ab"])
    elif how == "GR_transposed":                                 # slabs of the (square) right environment transposed
        if not has("R") or t["R"].shape[0] != t["R"].shape[2]:
            return None
        u["R"] = np.swapaxes(t["R"], 0, 2)
    elif how == "GL_transposed":
        if not has("G") or t["G"].shape[0] != t["G"].shape[2]:
            return None
        u["G"] = np.swapaxes(t["G"], 0, 2)
    elif how in ("levels_reversed", "last_level_skipped", "level_counted_twice") and not (has("R") or has("G")):
        return None
    elif how == "levels_reversed":                               # environment levels in reversed order
        k = "R" if has("R") else "G"
        if t[k].shape[1] == 1:
            return None
        u[k] = t[k][:, ::-1, :]
    elif how == "d1_d2_swapped":                                 # the two physical legs of a two-site tensor swapped
        if has("x") and t["x"].ndim == 4 and t["x"].shape[1] == t["x"].shape[3]:
            u["x"] = np.swapaxes(t["x"], 1, 3)
        elif has("AC") and t["O"].shape[1] == t["O2"].shape[1]:
            return np.swapaxes(contract(op, t), 1, 3)            # result planes (t1, t2) swapped
        else:
            return None
    elif how == "blocks_permuted":                               # row blocks of a blocked x read in another order
        if not has("nblk"):
            return None
        n = t["x"].shape[0] // t["nblk"]
        u["x"] = np.concatenate([t["x"][n:], t["x"][:n]], axis=0)
    elif how == "last_level_skipped":
        k = "R" if has("R") else "G"
        a = t[k].copy()
        a[:, -1, :] = 0
        u[k] = a
    elif how == "level_counted_twice":
        k = "R" if has("R") else "G"
        a = t[k].copy()
        a[:, 0, :] *= 2
        u[k] = a
    elif how == "unused_level_contributes":                      # an identity block INTO the first level nothing enters
        if not has("O"):
            return None
        last = "O2" if has("O2") else "O"                        # the slice next to the right environment
        col = used_levels(t[last])[0]
        if col.all():
            return None
        d = t[last].shape[1]
        O = t[last].copy()
        O[0, :, :, int(np.argmin(col))] += np.eye(d)
        u[last] = O
        if last == "O2" and not np.abs(t["O"][0, :, :, 0]).any():      # two sites: level 0 of the middle bond must be fed
            O1 = t["O"].copy()
            O1[0, :, :, 0] += np.eye(O1.shape[1])
            u["O"] = O1
    elif how == "unused_row_contributes":                        # an identity block OUT OF the first level nothing leaves
        if not has("O"):
            return None
        k = "O2" if has("O2") else "O"                           # two sites: the row_used of the second slice
        row = used_levels(t[k])[1]
        if row.all():
            return None
        r = int(np.argmin(row))
        O = t[k].copy()
        O[r, :, :, -1] += np.eye(O.shape[1])
        u[k] = O
        if k == "O2" and not np.abs(t["O"][0, :, :, r]).any():   # ... and level r of the middle bond must be fed
            O1 = t["O"].copy()
            O1[0, :, :, r] += np.eye(O1.shape[1])
            u["O"] = O1
    elif how == "reg_sign":                                      # regularize: the update added
        if not has("lvec"):
            return None
        return 2 * t["v"] - contract(op, t)
    elif how == "reg_shared_coef":                               # regularize: the dot of slab 0 used for every slab
        if not has("lvec") or t["v"].shape[1] == 1:
            return None
        u["v"] = np.repeat(t["v"][:, :1, :], t["v"].shape[1], axis=1)
        return t["v"] - (u["v"] - contract(op, u))
    else:
        raise KeyError(how)
    return contract(op, u)


WRONG = ("ts_swapped", "ts_swapped_site2", "conj_dropped", "GR_transposed", "GL_transposed", "levels_reversed", "d1_d2_swapped",
         "blocks_permuted", "last_level_skipped", "level_counted_twice", "unused_level_contributes", "unused_row_contributes",
         "reg_sign", "reg_shared_coef")
