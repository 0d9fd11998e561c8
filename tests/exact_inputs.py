"""Inputs whose result is exact, and the componentwise bound for the ones whose result is not.

Exact inputs.  Operands hold small integers stored as fp64 (uniform in [-4, 4]; Gaussian integers for complex128), the
scalars are dyadic (alpha = 0.5, beta = -2) and scalar MPO blocks are integers.  Every product and every partial sum of
every bracket order is then an integer (or half of one) far below 2^53, so fp64 arithmetic never rounds: ANY correct
route -- whatever the tile, the split, the order of the shares, the MFMA order or a folded form of the operator -- returns
the same bits, numpy's own fp64 product is the exact reference at any size, and the comparison is np.array_equal.  The
condition is checked, not assumed: `magnitude()` is prod(max|operand|) * prod(contracted extents), the largest value any
partial sum can reach, and every case asserts it below 2^50.

Integers this small would also survive an accidental fp32 path, so every family gets one Gaussian case as well, held to
the standard componentwise bound (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., section 3.1 / 3.5):
a length-K inner product evaluated in ANY order, with or without FMA, satisfies |fl(x.y) - x.y| <= gamma_K |x|.|y| with
gamma_K = K u / (1 - K u), u = 2^-53.  alpha * acc + beta * c adds at most two more roundings on the product term and two
on the beta term, so

    |got - ref| <= gamma_{K+2} (|alpha| |op A| |op B| + |beta| |C0|) <= (K + 4) u (|alpha| |op A| |op B| + |beta| |C0|)

elementwise for every K < 2^40; it needs no margin.  The reference is numpy in np.longdouble (64-bit significand here:
its own error, K 2^-64 |A||B|, is 2^-11 of the 2 u |A||B| the last inequality gives away for K <= 2^11).

complex128: a complex product is four real ones.  Re(sum a b) = sum (ar br - ai bi) is a real inner product of length
2 K, Im likewise, so each component errs by at most gamma_{2K+2} sum (|ar||br| + |ai||bi|) <= gamma_{2K+2} sum |a||b|
(Cauchy-Schwarz on the two-vectors (|ar|, |ai|), (|br|, |bi|)).  The modulus of the error is at most sqrt(2) times that:
2 sqrt(2) (K + 2) u sum |a||b| up to second order -- below the 4 (K + 4) u sum |a||b| used here (the factor 4 for the four
real products behind each complex one).

Three-factor operator contractions (dAC, dC, dAC2, the transfers): the stages nest, (1 + gamma_a)(1 + gamma_b)(1 + gamma_c) - 1
<= gamma_{a+b+c}, so K + 4 becomes the sum of the contracted extents of the stages plus 8 (two roundings of slack per
stage boundary), and the right-hand side is the same contraction of the absolute values.  Where the library may bracket
the stages in more than one order (the MPO folded into an environment first) the larger sum is taken.

tests/test_exact_inputs_cpu.py checks all of this without a GPU: the 2^50 guard of every exact case, numpy fp64 == the
longdouble reference on the exact cases, and numpy fp64 inside the bound on every Gaussian case.
"""
from __future__ import annotations

import functools
import zlib
from dataclasses import dataclass, replace

import numpy as np

U = 2.0 ** -53
LIMIT = 2.0 ** 50
ALPHA, BETA = 0.5, -2.0
TILES = [(64, 64), (128, 64), (64, 128), (128, 128)]
LD = np.longdouble
CLD = np.clongdouble
LD_MAX_WORK = 15 * 10 ** 7      # M N K up to which an exact case is also multiplied out in longdouble


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def int_array(rng, *shape, cplx=False):
    """integers uniform in [-4, 4] as fp64; Gaussian integers (both parts in [-4, 4]) for complex128"""
    a = rng.integers(-4, 5, size=shape).astype(np.float64)
    if cplx:
        a = a + 1j * rng.integers(-4, 5, size=shape).astype(np.float64)
    return a


def gauss_array(rng, *shape, cplx=False):
    a = rng.standard_normal(shape)
    if cplx:
        a = a + 1j * rng.standard_normal(shape)
    return a


def magnitude(operands, contracted):
    """prod(max|operand|) * prod(contracted extents): no partial sum of any bracket order exceeds it"""
    m = 1.0
    for a in operands:
        m *= float(np.abs(a).max(initial=0.0))
    for k in contracted:
        m *= float(k)
    return m


def assert_exact_range(operands, contracted, what=""):
    m = magnitude(operands, contracted)
    assert m < LIMIT, f"{what}: worst-case magnitude {m:.3e} is not below 2^50"
    return m


# ------------------------------------------------------------------------------------------------------------------
# GEMM cases
# ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GemmCase:
    """C = alpha op(A) op(B) + beta C through mpsk_gemm; op = (conjugate) transpose.  pa / pb / pc: rows of padding in the
    leading dimensions (complex: in complex elements).  kind "int": exact comparison; "gauss": componentwise bound.
    beta0: beta == 0 with C pre-filled with NaN (the result must not read C).  tile (0, 0): the automatic choice."""
    group: str
    M: int
    N: int
    K: int
    tA: int = 0
    tB: int = 0
    pa: int = 0
    pb: int = 0
    pc: int = 0
    kind: str = "int"
    cplx: bool = False
    beta0: bool = False
    tile: tuple = (0, 0)

    @property
    def data_key(self):
        return replace(self, tile=(0, 0), group="")

    @property
    def name(self):
        t = "NT"[self.tA] + "NT"[self.tB]
        return (f"{self.group}-{'c128' if self.cplx else 'f64'}-{self.kind}-{self.M}x{self.N}x{self.K}-{t}"
                f"-ld+{self.pa}+{self.pb}+{self.pc}{'-beta0' if self.beta0 else ''}-tile{self.tile[0]}x{self.tile[1]}")


def _sentinel(rows, cols):
    """integer pattern for the padding rows of C: distinct from any result a wrong store would plausibly leave"""
    i, j = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    return (1000.0 + (7 * i + 13 * j) % 97).astype(np.float64)


@functools.lru_cache(maxsize=None)
def _gemm_data(key: GemmCase):
    """(A_store, B_store, C_store, alpha, beta, ref[M, N], bound[M, N] or None); built once per data_key and never modified
    (the stores are read-only arrays)"""
    c = key
    rng = _rng(c.name)
    draw = int_array if c.kind == "int" else gauss_array
    ar, ac = (c.K, c.M) if c.tA else (c.M, c.K)
    br, bc = (c.N, c.K) if c.tB else (c.K, c.N)
    A, B, C0 = draw(rng, ar, ac, cplx=c.cplx), draw(rng, br, bc, cplx=c.cplx), draw(rng, c.M, c.N, cplx=c.cplx)
    alpha, beta = ALPHA, (0.0 if c.beta0 else BETA)
    dt = np.complex128 if c.cplx else np.float64
    nan = complex(np.nan, np.nan) if c.cplx else np.nan
    # padding rows of A and B hold NaN: a loader that strays into them poisons the result
    As = np.full((ar + c.pa, ac), nan, dtype=dt); As[:ar] = A
    Bs = np.full((br + c.pb, bc), nan, dtype=dt); Bs[:br] = B
    Cs = _sentinel(c.M + c.pc, c.N).astype(dt)
    Cs[:c.M] = nan if c.beta0 else C0
    opA = A.conj().T if c.tA else A
    opB = B.conj().T if c.tB else B
    hp = CLD if c.cplx else LD
    if c.kind == "int" and c.M * c.N * c.K > LD_MAX_WORK:
        hp = dt                  # the longdouble product of a case this size takes seconds: the 2^50 guard alone vouches
    ref_hp = alpha * (opA.astype(hp) @ opB.astype(hp))
    if not c.beta0:
        ref_hp = ref_hp + beta * C0.astype(hp)
    bound = None
    if c.kind == "int":
        assert_exact_range([A, B, [abs(alpha)]], [c.K * (2 if c.cplx else 1)], c.name)
        assert_exact_range([C0, [abs(beta)]], [], c.name)
        ref = ref_hp.astype(dt)
        assert np.array_equal(ref.astype(hp), ref_hp), c.name            # the reference itself is exact
    else:
        ref = ref_hp
        s = abs(alpha) * (np.abs(opA).astype(LD) @ np.abs(opB).astype(LD)) + abs(beta) * np.abs(C0).astype(LD)
        bound = (4 if c.cplx else 1) * (c.K + 4) * LD(U) * s
    for a in (As, Bs, Cs):
        a.setflags(write=False)
    return As, Bs, Cs, alpha, beta, ref, bound


def gemm_data(case: GemmCase):
    return _gemm_data(case.data_key)


def numpy_fp64_gemm(case: GemmCase):
    """what numpy's own fp64 product gives for the case (the CPU self-check compares it with the reference)"""
    As, Bs, Cs, alpha, beta, _, _ = gemm_data(case)
    ar = case.K if case.tA else case.M
    br = case.N if case.tB else case.K
    A, B = As[:ar], Bs[:br]
    out = alpha * ((A.conj().T if case.tA else A) @ (B.conj().T if case.tB else B))
    return out if case.beta0 else out + beta * Cs[:case.M]


def compare(got, ref, bound, name):
    """None if `got` passes (exact when bound is None, else |got - ref| <= bound elementwise); otherwise a JSON-able record"""
    if bound is None:
        if np.array_equal(got, ref):
            return None
        bad = ~(got == ref)
        err = np.abs(np.where(np.isfinite(got), got, np.inf) - ref)
    else:
        err = np.abs(got.astype(ref.dtype) - ref)
        bad = ~(err <= bound)
        if not bad.any():
            return None
    idx = np.argwhere(bad)
    fin = np.isfinite(err)
    return {"case": name, "n_bad": int(bad.sum()), "first_bad": [int(i) for i in idx[0]],
            "max_finite_err": float(err[fin].max()) if fin.any() else None, "nonfinite": int((~np.isfinite(got)).sum())}


def _aligned_ragged(group, M, N, K, pads, kind="int", cplx=False):
    return [GemmCase(group, M, N, K, tA, tB, pa=p, pb=p, kind=kind, cplx=cplx) for tA in (0, 1) for tB in (0, 1) for p in pads]


def gemm_case_groups():
    """{group: [GemmCase without a tile]} -- the case list of tests/test_gpu_gemm_tiles.py, every group run on every tile"""
    g = {}
    # aligned kernels: every extent a multiple of 128 / 16; ld == rows and ld == rows + 2 (even: still the aligned loader)
    g["aligned"] = _aligned_ragged("aligned", 256, 256, 96, (0, 2))
    # unaligned kernels: partial tiles in M and N for both tile widths, a K tail; ld odd (== rows) and rows + 3
    g["ragged"] = _aligned_ragged("ragged", 193, 131, 77, (0, 3))
    g["shortk"] = [GemmCase("shortk", 70, 130, K, t, t) for K in (1, 5, 15, 16, 17) for t in (0, 1)]
    edges = (63, 64, 65, 127, 128, 129)
    g["edges"] = [GemmCase("edges", M, N, 33) for M in edges for N in edges]
    # C with padding rows that must survive (sentinel pattern, ldc = M + 5), and beta == 0 over a NaN-filled C
    g["cbuf"] = [GemmCase("cbuf", 193, 131, 77, pc=5), GemmCase("cbuf", 256, 256, 96, pc=5),
                 GemmCase("cbuf", 193, 131, 77, beta0=True), GemmCase("cbuf", 256, 256, 96, beta0=True)]
    g["complex"] = (_aligned_ragged("complex", 256, 256, 96, (0,), cplx=True)
                    + _aligned_ragged("complex", 193, 131, 77, (0,), cplx=True))
    g["gauss"] = (_aligned_ragged("gauss", 193, 131, 77, (0,), kind="gauss")
                  + _aligned_ragged("gauss", 193, 131, 77, (0,), kind="gauss", cplx=True))
    return g


SPLITK_SHAPES = [(128, 128, 2048), (192, 192, 1600), (256, 128, 4096)]
SPLITK_RAGGED = (193, 131, 1109)        # KT = 70: partial tiles and a K tail through the unaligned split-K body


def splitk_cases():
    """long-K shapes on the automatic (64x64) tile: the split-K heuristic, or MPSK_SPLITK_F in a child process, decides
    the number of shares (KT = 128, 100, 256 k-tiles: f = 3 gives uneven shares on all three, 34 + 34 + 32 at K = 1600)"""
    return ([GemmCase("splitk", M, N, K, tA, 0) for (M, N, K) in SPLITK_SHAPES for tA in (0, 1)]
            + [GemmCase("splitk", *SPLITK_RAGGED, tA, 1) for tA in (0, 1)])


def gemm_cases(tiles=TILES):
    """the whole in-process list: every group on every forced tile, then the split-K shapes on the automatic tile"""
    out = []
    for cases in gemm_case_groups().values():
        for t in tiles:
            out += [replace(c, tile=tuple(t)) for c in cases]
    return out + splitk_cases()


def streamk_cases():
    """MPSK_STREAMK=1: Tb = 144 tiles of 128x128 and Ub / 512 = 18 >= 16 take the stream-K branch of gemm_f64"""
    return [GemmCase("streamk", 1536, 1536, 1024)]


def run_gemm_case(be, case: GemmCase):
    """Run one case through mpsk_gemm on backend `be`; returns None or a mismatch record.  The tile is forced for the call
    and the automatic choice restored (the knob is process-wide)."""
    As, Bs, Cs, alpha, beta, ref, bound = gemm_data(case)
    up, down = (be.upload_c, be.download_c) if case.cplx else (be.upload, be.download)
    dA, dB, dC = up(As), up(Bs), up(Cs)
    be.lib.mpsk_ctx_force_tile(be.ctx, *case.tile)
    try:
        if case.cplx:
            be._set_dtype(True)
        try:
            be.gemm_raw(case.tA, case.tB, case.M, case.N, case.K, alpha, dA.ptr, As.shape[0], dB.ptr, Bs.shape[0], beta,
                        dC.ptr, Cs.shape[0])
        finally:
            if case.cplx:
                be._set_dtype(False)
    finally:
        be.lib.mpsk_ctx_force_tile(be.ctx, 0, 0)
    got = down(dC)                                   # the whole allocation the test owns, padding rows included
    rec = compare(got[:case.M], ref, bound, case.name)
    if rec is None and case.pc and not np.array_equal(got[case.M:], Cs[case.M:]):
        rec = {"case": case.name, "padding_rows_of_C_changed": int((got[case.M:] != Cs[case.M:]).sum())}
    return rec


def run_gemm_cases(be, cases):
    return [r for r in (run_gemm_case(be, c) for c in cases) if r is not None]


# ------------------------------------------------------------------------------------------------------------------
# operator cases: dAC / dC / dAC2 / transfers / projection / dense-MPO slice
# ------------------------------------------------------------------------------------------------------------------
RAGGED = (33, 65, 2, (1, 3, 2, 1))
ALIGNED = (128, 128, 2, (1, 1, 1, 1, 1))
LONGK = (256, 256, 2, (1, 1, 1, 1, 1))  # stage 3 of dAC: 5 segments of 16 k-tiles = 80 >= 64 on 32 tiles: split-K territory
PROJ = (20, 33, 65, 48)                 # Dlo, Dl, Dr, Dro
DENSE_W, DENSE_D = 4, 2


def rand_slice(rng, odim, d, chis, draw, cplx=False, density=0.6, scal_prob=0.3):
    """block-sparse slice with the MPOHamiltonian structure (upper triangular, 1 on the corners), as tests/test_gpu_ops.py
    builds it, with the entries of the blocks and the scalar blocks taken from `draw`"""
    import mpskit_oracle as mo
    blocks = {(0, 0): 1.0, (odim - 1, odim - 1): 1.0}
    for i in range(odim):
        for j in range(i, odim):
            if (i, j) in blocks:
                continue
            if rng.random() < density:
                if chis[i] == chis[j] and rng.random() < scal_prob:
                    v = draw(rng, 1, cplx=cplx)[0]
                    blocks[(i, j)] = complex(v) if cplx else float(v)
                else:
                    blocks[(i, j)] = draw(rng, chis[i], d, d, chis[j], cplx=cplx)
    return mo.SparseMPOSlice(odim, d, list(chis), list(chis), blocks)


def _stack(env):
    return np.concatenate([np.asarray(e) for e in env], axis=1)         # list of [Db, chi, Dk] -> [Db, W, Dk]


def contract(op, t, conv=lambda a: a):
    """The operator as plain pairwise einsums on conv(operand) -- conv = longdouble cast for the reference, |.| in
    longdouble for the bound.  O: the dense [Wl, d, d, Wr] form of the slice; G / R: stacked environments [Db, W, Dk].
    Results in the layout the oracle returns (stacked over levels for the transfers)."""
    e = functools.partial(np.einsum, optimize=False)
    g = lambda k: conv(t[k])
    if op == "dAC":
        t1 = e("pwa,asb->pwsb", g("G"), g("x"))
        return e("pbtv,bvq->ptq", e("pwsb,wtsv->pbtv", t1, g("O")), g("R"))
    if op == "dC":
        return e("pwb,bwq->pq", e("pwa,ab->pwb", g("G"), g("x")), g("R"))
    if op == "dAC2":
        t1 = e("pwa,asbr->pwsbr", g("G"), g("x"))
        t2 = e("pwsbr,wtsu->ptubr", t1, g("O"))
        return e("ptbzv,bvq->ptqz", e("ptubr,uzrv->ptbzv", t2, g("O2")), g("R"))
    cj = (lambda a: a) if conv is not _hp else np.conj
    if op == "tl":
        t2 = e("pwsb,wtsv->pbtv", e("pwa,asb->pwsb", g("G"), g("A")), g("O"))
        return e("ptq,pbtv->qvb", cj(g("Ab")), t2)
    if op == "tr":
        t1 = e("bvq,ptq->bvpt", g("R"), cj(g("Ab")))
        return e("asb,wsbp->awp", g("A"), e("wtsv,bvpt->wsbp", g("O"), t1))
    raise KeyError(op)


def _hp(a):
    a = np.asarray(a)
    return a.astype(CLD if np.iscomplexobj(a) else LD)


def _abs_hp(a):
    return np.abs(np.asarray(a)).astype(LD)


def op_depth(op, t):
    """sum of the contracted extents of the stages, the larger over the bracket orders the library has"""
    O = t["O"]
    Wl, d, _, Wr = O.shape
    if op == "dAC":                      # (a)(w s)(b v)   |   MPO folded into the right environment: (v)(a)(w s b)
        Dl, Dr = t["x"].shape[0], t["x"].shape[2]
        return max(Dl + Wl * d + Dr * Wr, Wr + Dl + Wl * d * Dr)
    if op == "dC":
        Dl, Dr = t["x"].shape
        return Dl + Dr * Wl
    if op == "dAC2":                     # (a)(w s)(u r)(b v)   |   the two slices mixed as one pass: (a)(w s r)(b v)
        Dl, _, Dr, d2 = t["x"].shape
        Wm = O.shape[3]
        return Dl + max(Wl * d + Wm * d2, Wl * d * d2) + Dr * t["O2"].shape[3]
    Dl, _, Dr = t["A"].shape
    Dlb, _, Drb = t["Ab"].shape
    if op == "tl":                       # (a)(w s)(p t)
        return Dl + Wl * d + Dlb * d
    if op == "tr":                       # (b)(v s)(t q)   |   (q)(v t)(s b)
        return max(Dr + Wr * d + d * Drb, Drb + Wr * d + d * Dr)
    raise KeyError(op)


@functools.lru_cache(maxsize=None)
def op_case(op, shape, kind="int", cplx=False, variant=""):
    """Operands, oracle-layout reference and bound (None: exact) of one operator case.  shape: RAGGED / ALIGNED;
    variant "proj": rectangular environments (PROJ); "dense": one dense MPO tensor [4, 2, 2, 4] instead of a sparse slice.
    The dict is built once and shared; nothing in it is modified afterwards."""
    import mpskit_oracle as mo
    Dl, Dr, d, chis = shape
    name = f"{op}-{variant}-{kind}-{'c128' if cplx else 'f64'}-{Dl}x{Dr}"
    rng = _rng(name)
    draw = functools.partial(int_array if kind == "int" else gauss_array, cplx=cplx)
    if variant == "dense":
        O = draw(rng, DENSE_W, DENSE_D, DENSE_D, DENSE_W)
        chis, d = (DENSE_W,), DENSE_D
        s = mo.SparseMPOSlice(1, d, [DENSE_W], [DENSE_W], {(0, 0): O})
    else:
        s = rand_slice(rng, len(chis), d, chis, functools.partial(int_array if kind == "int" else gauss_array), cplx=cplx)
    Dlo, Dro = (PROJ[0], PROJ[3]) if variant == "proj" else (Dl, Dr)
    t = {"name": name, "s": s, "O": s.full(), "chis": list(chis), "d": d}
    if op in ("dAC", "dC", "dAC2"):
        t["GL"] = [draw(rng, Dlo, c, Dl) for c in chis]
        t["GR"] = [draw(rng, Dr, c, Dro) for c in chis]
        t["G"], t["R"] = _stack(t["GL"]), _stack(t["GR"])
        t["x"] = draw(rng, *{"dAC": (Dl, d, Dr), "dC": (Dl, Dr), "dAC2": (Dl, d, Dr, d)}[op])
        if op == "dAC2":
            t["s2"] = rand_slice(rng, len(chis), d, chis, functools.partial(int_array if kind == "int" else gauss_array), cplx=cplx)
            t["O2"] = t["s2"].full()
            oracle = lambda: mo.dAC2(t["x"], s, t["s2"], t["GL"], t["GR"])
        elif op == "dC":
            oracle = lambda: mo.dC(t["x"], t["GL"], t["GR"])
        else:
            oracle = lambda: mo.dAC(t["x"], s, t["GL"], t["GR"])
    else:
        t["A"], t["Ab"] = draw(rng, Dl, d, Dr), draw(rng, Dl, d, Dr)
        if op == "tl":
            t["GL"] = [draw(rng, Dl, c, Dl) for c in chis]
            t["G"] = _stack(t["GL"])
            oracle = lambda: _stack(mo.transfer_left(t["GL"], s, t["A"], t["Ab"]))
        else:
            t["GR"] = [draw(rng, Dr, c, Dr) for c in chis]
            t["R"] = _stack(t["GR"])
            oracle = lambda: _stack(mo.transfer_right(t["GR"], s, t["A"], t["Ab"]))
    operands = [t[k] for k in ("G", "R", "x", "A", "Ab", "O2") if k in t] + ([] if op == "dC" else [t["O"]])
    if kind == "int":
        # every contracted index of the operator; a product of n complex factors is 2^(n-1) real terms
        Wl, Wr = t["O"].shape[0], t["O"].shape[3]
        ext = {"dAC": [Dl, Wl, d, Dr, Wr], "dC": [Dl, Dr, Wl], "dAC2": [Dl, Wl, d, d, Dr, Wr, t["O2"].shape[3] if "O2" in t else 1],
               "tl": [Dl, Wl, d, Dl, d], "tr": [Dr, Wr, d, Dr, d]}[op]
        t["magnitude"] = assert_exact_range(operands, ext + [2 if cplx else 1] * len(operands), name)
        t["ref"], t["bound"] = oracle(), None
    else:
        t["ref"] = contract(op, t, _hp)
        t["bound"] = (4 if cplx else 1) * (op_depth(op, t) + 8) * LD(U) * contract(op, t, _abs_hp)
        t["oracle"] = oracle
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


def op_cases_exact():
    """(op, shape, cplx, variant) of every exact operator case of tests/test_gpu_ops_tiles.py"""
    out = [(op, shp, False, "") for op in ("dAC", "dC", "tl", "tr") for shp in (RAGGED, ALIGNED)]
    out += [("dAC2", RAGGED, False, ""), ("dAC", RAGGED, False, "proj")]
    out += [(op, shp, False, "dense") for op in ("dAC", "tl", "tr") for shp in (RAGGED, ALIGNED)]
    out += [(op, shp, True, "") for op in ("dAC", "tl", "tr") for shp in (RAGGED, ALIGNED)]
    return out


def op_cases_gauss():
    """one Gaussian case per operator, all on the small ragged shape"""
    out = [(op, RAGGED, False, "") for op in ("dAC", "dC", "dAC2", "tl", "tr")]
    out += [("dAC", RAGGED, False, "proj")] + [(op, RAGGED, False, "dense") for op in ("dAC", "tl", "tr")]
    out += [(op, RAGGED, True, "") for op in ("dAC", "tl", "tr")]
    return out
