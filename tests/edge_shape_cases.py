"""Exact cases at the shapes both ends of a finite chain pass: bonds 1 to 9, through every route a sweep takes there.

With physical dimension d the bonds of a finite chain run 1, d, d^2, ... up to the bulk D and back, so every DMRG, TDVP,
approximate, propagator, WindowMPS and finite-linalg call sees AC [1, 2, 2], [2, 2, 4], ..., [2, 2, 1], bond matrices 1 x 1
and 2 x 2 and two-site tensors [1, 2, 4, 2].  There one 64 x 64 tile holds a single partial MFMA fragment in M and in N,
K is shorter than one k-step, odd Dl gives column starts that are only 8-byte aligned, a planar complex copy has one
element, and a segment table has more levels than the bond has rows.  The other exact modules stop at bond 17.

Rules of tests/exact_inputs.py, reused as they stand: integer operands in [-4, 4] (Gaussian integers for complex128) whose
every partial sum stays below 2^50 (asserted per case), so any correct route returns the same bits and the comparison is
np.array_equal; one Gaussian case per entry at (Dl, Dr) = (3, 7), d = 3 inside the componentwise bound of the module that
already derives it (exact_proj_inputs._finish, exact_canonical_inputs.hac_case / transfer_case, exact_inputs.GemmCase).
Every case has two independent references: mpskit_oracle (block by block, BLAS tensordot) and the pairwise einsum
`contract`; tests/test_edge_shape_cases_cpu.py holds them to each other.

The bond ladder: (Dl, Dr, d) of every site a chain of d = 2 or d = 3 visits, the odd pair (3, 7) / (7, 3), and for the
two-site entries also theta [1, 2, 4, 2], its mirror and [2, 2, 2, 2].  Slices: chis (1, 3, 2, 1), (1, 1, 1, 1, 1), the
smallest legal slice (odim 2, chis (1, 1): the identity corners and one block), and for complex128 a slice with complex
scalar blocks.  A case whose reference would be identically zero is redrawn (salt), so none is vacuous.
"""
from __future__ import annotations

import functools
import itertools
from dataclasses import dataclass

import numpy as np

import exact_canonical_inputs as eci
import exact_inputs as ei
import exact_proj_inputs as epi
from exact_inputs import ALPHA, LD, U, _abs_hp, _hp, _rng, assert_exact_range, gauss_array, int_array, rand_slice

LADDER_D2 = [(1, 1), (1, 2), (2, 4), (4, 8), (8, 4), (4, 2), (2, 1)]
LADDER_D3 = [(1, 3), (3, 9), (9, 3), (3, 1)]
LADDER_ODD = [(3, 7), (7, 3)]
LADDER = [(a, b, 2) for a, b in LADDER_D2] + [(a, b, 3) for a, b in LADDER_D3 + LADDER_ODD]       # (Dl, Dr, d)
TWO_SITE = [(1, 4, 2), (4, 1, 2), (2, 2, 2)]
BONDS = (1, 2, 3, 4, 7, 8, 9)
GAUSS_SHAPE = (3, 7, 3)
SLICES = ("chi", "five", "min")
SLICES_C128 = SLICES + ("cscal",)
CHIS = {"chi": (1, 3, 2, 1), "five": (1, 1, 1, 1, 1), "min": (1, 1), "cscal": (1, 1, 1)}
MAX_BOND = 9

# entry -> (operation of exact_proj_inputs.contract, dtypes it has, shapes): include/mpsk.h says which entries are complex
ENTRIES = {
    "dAC": ("dAC", (False, True), LADDER), "dC": ("dC", (False, True), LADDER),
    "dAC2": ("dAC2", (False, True), LADDER + TWO_SITE), "dAC_proj": ("dAC_proj", (False, True), LADDER),
    "dC_proj": ("dC_proj", (False,), LADDER), "dC_proj_c": ("dC_proj", (True,), LADDER),
    "dAC2_proj": ("dAC2_proj", (False, True), LADDER + TWO_SITE), "dAC2_product": ("dAC2_product", (False,), LADDER + TWO_SITE),
    "tl": ("tl", (False, True), LADDER), "tr": ("tr", (False, True), LADDER)}

# Refusals by contract: (entry, condition) -> (error code, text of mpsk_last_error, the line of include/mpsk.h behind it)
REFUSALS = {
    ("hac_apply", "nblk does not divide Dl"): (
        1, "nblk must divide Dl (and be <= 32)", "x is given as nblk row blocks, block q = x[q Dl/nblk : (q+1) Dl/nblk, :, :]"),
    ("hac_apply", "nblk > 1 on a complex operator"): (
        3, "the blocked layout is implemented for MPSK_F64 only",
        "The blocked layout (nblk > 1) is taken by MPSK_F64 operators in modes 0, 1 and 4"),
    ("hac_apply", "nblk > 1 in mode 3"): (
        3, "the Jordan-form operator takes the plain vector layout only",
        "The blocked layout (nblk > 1) is taken by MPSK_F64 operators in modes 0, 1 and 4"),
    ("regularize_axpby", "complex operand at an 8-byte offset"): (
        1, "complex operands must be 16-byte aligned", "Complex tensors are INTERLEAVED complex128"),
    ("dC_proj", "ctx set to MPSK_C128"): (3, "mpsk_dC_proj: implemented for MPSK_F64 only", "MPSK_F64 only: a ctx set to MPSK_C128 (mpsk_ctx_set_dtype) gets MPSK_ERR_UNSUPPORTED"),
}


def other_bonds(Dl, Dr):
    """(Dlo, Dm, Dro) of the projection and two-factor entries: bonds of the ladder, pairwise different from their neighbour
    where the ladder allows it"""
    i, j = BONDS.index(Dl), BONDS.index(Dr)
    return BONDS[(i + 2) % len(BONDS)], BONDS[(i + j + 1) % len(BONDS)], BONDS[(j + 3) % len(BONDS)]


# ------------------------------------------------------------------------------------------------------------------
# slices
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_slice(which, d, kind="int", cplx=False, salt=""):
    """"chi" / "five": exact_inputs.rand_slice on chis (1, 3, 2, 1) / (1, 1, 1, 1, 1), redrawn until it holds a dense block
    and (chi) a scalar block off the corners; "min": odim 2, the corners and one dense block; "cscal": three levels of
    chi 1 with two complex scalar blocks (the complex128 mix plan) and two dense ones"""
    import mpskit_oracle as mo
    chis = CHIS[which]
    draw = int_array if kind == "int" else gauss_array
    rng = _rng(f"edge-slice-{which}-{d}-{kind}-{cplx}-{salt}")

    def dense(cl, cr):
        while True:
            b = draw(rng, cl, d, d, cr, cplx=cplx)
            if np.abs(b).reshape(cl, d * d, cr).max(axis=1).min() > 0:
                return b

    if which == "min":
        return mo.SparseMPOSlice(2, d, [1, 1], [1, 1], {(0, 0): 1.0, (1, 1): 1.0, (0, 1): dense(1, 1)})
    if which == "cscal":
        assert cplx
        sc = (2.0 + 3.0j, -1.0 + 2.0j) if kind == "int" else tuple(complex(v) for v in gauss_array(rng, 2, cplx=True))
        return mo.SparseMPOSlice(3, d, [1, 1, 1], [1, 1, 1], {(0, 0): 1.0, (2, 2): 1.0, (1, 1): sc[0], (0, 2): sc[1],
                                                              (0, 1): dense(1, 1), (1, 2): dense(1, 1)})
    for _ in range(200):
        s = rand_slice(rng, len(chis), d, chis, draw, cplx=cplx)
        off = [k for k in s.Os if k not in ((0, 0), (len(chis) - 1, len(chis) - 1))]
        if any(not s.isscal(*k) for k in off) and (which == "five" or any(s.isscal(*k) for k in off)):
            return s
    raise AssertionError(which)


# ------------------------------------------------------------------------------------------------------------------
# section 2 / 4: operators on sparse slices and the plain transfers
# ------------------------------------------------------------------------------------------------------------------
def oracle_ref(t):
    """the second reference: mpskit_oracle on the same operands, in the layout of epi.contract"""
    import mpskit_oracle as mo
    op, chis = t["op"], t["chis"]
    G = epi._unstack(t["G"], chis) if "G" in t else None
    R = epi._unstack(t["R"], chis) if "R" in t else None
    if op in ("dAC", "dAC_proj"):
        return mo.dAC(t["x"], t["s"], G, R)
    if op in ("dC", "dC_proj"):
        return mo.dC(t["x"], G, R)
    if op == "dAC2":
        return mo.dAC2(t["x"], t["s"], t["s2"], G, R)
    if op in ("dAC2_proj", "dAC2_product"):
        theta = np.einsum("asm,mrb->asbr", t["AC"], t["AR"], optimize=False)
        return mo.dAC2(theta, t["s"], t["s2"], G, R)
    if op == "tl":
        return epi._stack(mo.transfer_left(G, t["s"], t["A"], t["Ab"]))
    if op == "tr":
        return epi._stack(mo.transfer_right(R, t["s"], t["A"], t["Ab"]))
    if op == "reg":
        return mo.regularize_env(t["v"], t["lvec"], t["rvec"])
    raise KeyError(op)


def _operands(t, op, rng, draw, Dl, Dr, d, W):
    Dlo, Dm, Dro = other_bonds(Dl, Dr)
    if op in ("dC", "dC_proj"):
        t.update(G=draw(rng, Dlo if op == "dC_proj" else Dl, W, Dl), R=draw(rng, Dr, W, Dro if op == "dC_proj" else Dr), x=draw(rng, Dl, Dr))
    elif op == "dAC":
        t.update(G=draw(rng, Dl, W, Dl), R=draw(rng, Dr, W, Dr), x=draw(rng, Dl, d, Dr))
    elif op == "dAC_proj":
        t.update(G=draw(rng, Dlo, W, Dl), R=draw(rng, Dr, W, Dro), x=draw(rng, Dl, d, Dr))
    elif op == "dAC2":
        t.update(G=draw(rng, Dl, W, Dl), R=draw(rng, Dr, W, Dr), x=draw(rng, Dl, d, Dr, d))
    elif op == "dAC2_proj":
        t.update(G=draw(rng, Dlo, W, Dl), R=draw(rng, Dr, W, Dro), AC=draw(rng, Dl, d, Dm), AR=draw(rng, Dm, d, Dr))
    elif op == "dAC2_product":
        t.update(G=draw(rng, Dl, W, Dl), R=draw(rng, Dr, W, Dr), AC=draw(rng, Dl, d, Dm), AR=draw(rng, Dm, d, Dr))
    elif op == "tl":                                    # the bra of a finite chain has the bonds of the ket
        t.update(G=draw(rng, Dl, W, Dl), A=draw(rng, Dl, d, Dr), Ab=draw(rng, Dl, d, Dr))
    elif op == "tr":
        t.update(R=draw(rng, Dr, W, Dr), A=draw(rng, Dl, d, Dr), Ab=draw(rng, Dl, d, Dr))
    else:
        raise KeyError(op)
    return dict(Dl=Dl, Dm=Dm, Dr=Dr, Dlb=Dl, Drb=Dr, Wl=W, Wm=W, Wr=W, W=W, d1=d, d2=d)


@functools.lru_cache(maxsize=None)
def op_case(entry, Dl, Dr, d, which, kind="int", cplx=False):
    """operands, reference and bound (None: exact) of one operator case, through exact_proj_inputs._finish; built once,
    shared, never modified"""
    op = ENTRIES[entry][0]
    chis = CHIS[which]
    W = sum(chis)
    draw = functools.partial(int_array if kind == "int" else gauss_array, cplx=cplx)
    for salt in range(50):
        name = f"edge-{entry}-{which}-{kind}-{'c128' if cplx else 'f64'}-{Dl}x{d}x{Dr}" + (f"-salt{salt}" if salt else "")
        rng = _rng(name)
        t = {"name": name, "entry": entry, "chis": list(chis), "dense": False, "shape": (Dl, Dr, d), "slice": which}
        if op not in ("dC", "dC_proj"):
            s = edge_slice(which, d, kind, cplx, salt=str(salt) if salt else "")
            t.update(s=s, O=np.asarray(s.full(), dtype=np.complex128 if cplx else np.float64))
            if op.startswith("dAC2"):
                s2 = edge_slice(which, d, kind, cplx, salt=f"site2-{salt}")
                t.update(s2=s2, O2=np.asarray(s2.full(), dtype=t["O"].dtype))
        ext = _operands(t, op, rng, draw, Dl, Dr, d, W)
        t = epi._finish(op, t, kind, cplx, ext)
        if kind != "int" or np.any(t["ref"] != 0):
            return t
    raise AssertionError(f"{name}: every draw is vacuous")


def op_keys():
    """(entry, Dl, Dr, d, slice, cplx) of every integer operator case"""
    out = []
    for entry, (_, dtypes, shapes) in ENTRIES.items():
        for cplx in dtypes:
            for which in (SLICES_C128 if cplx else SLICES):
                out += [(entry, Dl, Dr, d, which, cplx) for (Dl, Dr, d) in shapes]
    return out


def op_gauss_keys():
    Dl, Dr, d = GAUSS_SHAPE
    return [(entry, Dl, Dr, d, "chi", cplx) for entry, (_, dtypes, _) in ENTRIES.items() for cplx in dtypes]


def key_id(k):
    entry, Dl, Dr, d, which, cplx = k
    return f"{entry}-{which}-{'c128' if cplx else 'f64'}-{Dl}x{d}x{Dr}"


def hac_bound(t):
    """componentwise bound of one Gaussian prepared-operator application in any mode: the depth of exact_proj_inputs for
    "hac_blocked" (the larger of the mix bracket and the right-combined one) or the case's own mode-3 depth"""
    if "depth" in t:                                     # exact_canonical_inputs.hac_case
        return t["bound"]
    dd, n = epi.depth("hac_blocked", t)
    return (4 if t["cplx"] else 1) * (dd + 2 * n + 2) * LD(U) * epi.contract("dAC", t, _abs_hp)


def axpby_bound(t, a0, a1):
    """y = a0 x + a1 H x in one fused pass behind the application: two products and one sum more"""
    c = 4 if t["cplx"] else 1
    return abs(a1) * hac_bound(t) + c * 3 * LD(U) * (abs(a0) * _abs_hp(t["x"]) + abs(a1) * epi.contract("dAC", t, _abs_hp))


def expected_hac_mode(t):
    """the mode mpsk_hac_create picks for a real sparse slice without flags: mode 1 when the slice has a right-combined
    form and the cost model of mpsk_hac_create_ex (mirrored here) does not price it above the mix form"""
    O = t["O"]
    Dl, _, Dr = t["x"].shape
    d = O.shape[1]
    Wl = O.shape[0]
    wr_used = int(epi.used_levels(O)[0].sum())
    ns = epi.rc_nseg(O)
    u3 = 2.0 * Dl * Dr * Dr
    t_mix = wr_used * d * u3 / 50e12 + (Wl + wr_used) * 8.0 * Dl * d * Dr / 3e12 + 6e-6
    return 1 if ns > 0 and ns * d * u3 / 50e12 <= t_mix else 0


# ------------------------------------------------------------------------------------------------------------------
# section 1: the GEMM core, packed -- one upload and one download per group
# ------------------------------------------------------------------------------------------------------------------
GEMM_EXTENTS = (1, 2, 3, 4, 8, 9)
PAIR_EXTENTS = (1, 2, 5)
GEMM_BETA = 1.0


@dataclass(frozen=True)
class GemmGroup:
    """all 216 shapes (M, N, K) of GEMM_EXTENTS^3 for one dtype, transpose pair, beta and leading-dimension padding.
    beta0: beta = 0 over a NaN-filled C, else beta = 1 over an integer C.  pad: rows of padding in every leading dimension
    (1: every column start of an fp64 operand is only 8-byte aligned); the padding rows of A and B hold NaN, those of C a
    sentinel pattern that must survive."""
    cplx: bool
    tA: int
    tB: int
    beta0: bool
    pad: int

    @property
    def name(self):
        return (f"edge-gemm-{'c128' if self.cplx else 'f64'}-{'NT'[self.tA]}{'NT'[self.tB]}-{'beta0' if self.beta0 else 'beta1'}"
                f"-ld+{self.pad}")


def gemm_groups():
    return [GemmGroup(c, tA, tB, b0, p) for c in (False, True) for tA in (0, 1) for tB in (0, 1) for b0 in (True, False) for p in (0, 1)]


def _pack(parts, dt, fill):
    """flat buffer of the column-major stores, each starting on an even element (16 bytes for fp64); the gaps hold `fill`"""
    offs, n = [], 0
    for p in parts:
        offs.append(n)
        n += p.size + (p.size & 1)
    flat = np.full(max(n, 1), fill, dtype=dt)
    for o, p in zip(offs, parts):
        flat[o:o + p.size] = np.ravel(p, order="F")
    return flat, offs


@functools.lru_cache(maxsize=None)
def gemm_group_data(g: GemmGroup):
    """{"A", "B", "C": packed stores, "expect": what the C buffer must hold afterwards (results, sentinels and gaps),
    "calls": [(M, N, K, offA, lda, offB, ldb, offC, ldc)] in elements, "alpha", "beta", "items": per-call operands}"""
    rng = _rng(g.name)
    dt = np.complex128 if g.cplx else np.float64
    nan = complex(np.nan, np.nan) if g.cplx else np.nan
    beta = 0.0 if g.beta0 else GEMM_BETA
    As, Bs, Cs, Es, shapes, items = [], [], [], [], [], []
    for M, N, K in itertools.product(GEMM_EXTENTS, repeat=3):
        ar, ac = (K, M) if g.tA else (M, K)
        br, bc = (N, K) if g.tB else (K, N)
        while True:
            A, B, C0 = int_array(rng, ar, ac, cplx=g.cplx), int_array(rng, br, bc, cplx=g.cplx), int_array(rng, M, N, cplx=g.cplx)
            opA, opB = (A.conj().T if g.tA else A), (B.conj().T if g.tB else B)
            prod = opA @ opB
            ref = ALPHA * prod + (0 if g.beta0 else beta * C0)
            if np.any(prod != 0) and np.any(ref != 0):   # a single zero operand would make a 1 x 1 x 1 case vacuous
                break
        assert_exact_range([A, B, [ALPHA]], [K * (2 if g.cplx else 1)], g.name)
        hp = ei.CLD if g.cplx else LD
        ref_hp = ALPHA * (opA.astype(hp) @ opB.astype(hp)) + (0 if g.beta0 else beta * C0.astype(hp))
        assert np.array_equal(ref.astype(hp), ref_hp), (g.name, M, N, K)
        a = np.full((ar + g.pad, ac), nan, dtype=dt); a[:ar] = A
        b = np.full((br + g.pad, bc), nan, dtype=dt); b[:br] = B
        c = ei._sentinel(M + g.pad, N).astype(dt); c[:M] = nan if g.beta0 else C0
        e = c.copy(); e[:M] = ref
        As.append(a); Bs.append(b); Cs.append(c); Es.append(e); shapes.append((M, N, K))
        items.append((A, B, C0, ref))
    fa, oa = _pack(As, dt, nan)
    fb, ob = _pack(Bs, dt, nan)
    fc, oc = _pack(Cs, dt, 4000.0)
    fe, _ = _pack(Es, dt, 4000.0)
    calls = [(M, N, K, oa[i], As[i].shape[0], ob[i], Bs[i].shape[0], oc[i], Cs[i].shape[0]) for i, (M, N, K) in enumerate(shapes)]
    for x in (fa, fb, fc, fe):
        x.setflags(write=False)
    return {"A": fa, "B": fb, "C": fc, "expect": fe, "calls": calls, "alpha": ALPHA, "beta": beta, "items": items}


def gemm_mismatch(g, got):
    """None, or the first call of the group whose part of the C buffer (padding row and gap included) is not as expected"""
    data = gemm_group_data(g)
    if np.array_equal(got, data["expect"]):
        return None
    bad = np.flatnonzero(~(got == data["expect"]))
    offs = [c[7] for c in data["calls"]]
    i = int(np.searchsorted(offs, bad[0], side="right") - 1)
    M, N, K = data["calls"][i][:3]
    return {"group": g.name, "first_bad_shape": (M, N, K), "n_bad": int(bad.size), "offset_in_call": int(bad[0] - offs[i])}


GEMM_GAUSS = [ei.GemmCase("edge", 3, 7, 9, tA, tB, pa=1, pb=1, pc=1, kind="gauss", cplx=c) for c in (False, True)
              for (tA, tB) in ((0, 0), (1, 1))]


@functools.lru_cache(maxsize=None)
def gemm_pair_case(M, N, K, with_q=True):
    """mpsk_gemm_pair on integers: out_r = beta_r out_r + (P diag(a_r) + Q diag(b_r)) B, r = 1, 2; beta1 = 0 over NaN,
    beta2 = 1 over integers; every leading dimension has one padding row (NaN in the operands, sentinels in the outputs)"""
    name = f"edge-gemm_pair-{M}x{N}x{K}-{'pq' if with_q else 'p'}"
    rng = _rng(name)
    while True:
        P, Q, B = int_array(rng, M, K), int_array(rng, M, K), int_array(rng, K, N)
        coef = int_array(rng, K, 4)                      # column r = row r of the ABI: a1, b1, a2, b2
        C2 = int_array(rng, M, N)
        q = Q if with_q else np.zeros_like(Q)
        r1 = (P * coef[:, 0] + q * coef[:, 1]) @ B
        r2 = (P * coef[:, 2] + q * coef[:, 3]) @ B + C2
        if np.any(r1 != 0) and np.any(r2 != 0):
            break
    assert_exact_range([P, B, coef, [2.0]], [K], name)
    t = {"name": name, "P": P, "Q": Q if with_q else None, "B": B, "coef": coef, "C2": C2, "ref1": r1, "ref2": r2}
    hp = lambda a: a.astype(LD)
    t["ref1_hp"] = (hp(P) * hp(coef[:, 0]) + hp(q) * hp(coef[:, 1])) @ hp(B)
    return t


@functools.lru_cache(maxsize=None)
def gemm_pair_gauss():
    """the Gaussian case of mpsk_gemm_pair at M, N, K = 3, 7, 9 with both outputs; out2 accumulates (beta2 = 1).  Bound in the
    style of exact_inputs.GemmCase: the staged operand P a + Q b is two products and one sum (three roundings) in front of
    a length-K inner product, beta out adds two: (K + 3 + 2) u (|P| |a| + |Q| |b|) |B| + 2 u |beta| |out|."""
    M, N, K = 3, 7, 9
    name = "edge-gemm_pair-gauss"
    rng = _rng(name)
    P, Q, B, coef, C2 = (gauss_array(rng, *shp) for shp in ((M, K), (M, K), (K, N), (K, 4), (M, N)))
    hp = lambda a: a.astype(LD)
    mix = lambda f, a, b: (f(P) * f(coef[:, a]) + f(Q) * f(coef[:, b])) @ f(B)
    t = {"name": name, "P": P, "Q": Q, "B": B, "coef": coef, "C2": C2, "ref1": mix(hp, 0, 1), "ref2": mix(hp, 2, 3) + hp(C2)}
    t["bound1"] = (K + 5) * LD(U) * mix(_abs_hp, 0, 1)
    t["bound2"] = (K + 5) * LD(U) * mix(_abs_hp, 2, 3) + 2 * LD(U) * _abs_hp(C2)
    t["fp64_1"], t["fp64_2"] = mix(lambda a: a, 0, 1), mix(lambda a: a, 2, 3) + C2
    return t


def gemm_pair_keys():
    return [(M, N, K, True) for M, N, K in itertools.product(PAIR_EXTENTS, repeat=3)] + [(1, 1, 1, False), (5, 2, 1, False)]


# ------------------------------------------------------------------------------------------------------------------
# section 3: prepared operators -- modes 0 / 1 / 2 on the sparse slices above, mode 3 on the Jordan-form families
# ------------------------------------------------------------------------------------------------------------------
def jordan_families(d):
    return [f for f in eci.FAMILIES if eci.DPHYS[f] == d]


def hac3_keys():
    """(family, Dl, Dr, cplx) of the mode-3 cases: exact_canonical_inputs.hac_case on the whole ladder"""
    return [(f, Dl, Dr, cplx) for cplx in (False, True) for (Dl, Dr, d) in LADDER for f in jordan_families(d)]


AXPBY_REAL = (-2.0, 0.5)                     # (a0, a1): y = a0 x + a1 H x, dyadic
AXPBY_CPLX = (1.0 - 2.0j, 0.5j)
HSUM_COEFS = (2.0, -3.0)


@functools.lru_cache(maxsize=None)
def hsum_case(route, Dl, Dr, d, cplx=False, kind="int"):
    """two terms on one site.  route 1: two Jordan-form families on canonical environments (folded); route 2: two sparse
    slices of different W (accumulated).  ref = sum_k HSUM_COEFS[k] H_k x, the oracle term by term."""
    import mpskit_oracle as mo
    name = f"edge-hsum{route}-{kind}-{'c128' if cplx else 'f64'}-{Dl}x{d}x{Dr}"
    if route == 1:
        fams = jordan_families(d)
        fams = [fams[0], fams[-1]]
        terms = [eci.hac_case(f, Dl, Dr, kind, cplx) for f in fams]
        x = terms[0]["x"]
    else:
        terms = [op_case("dAC", Dl, Dr, d, w, kind, cplx) for w in ("chi", "min")]
        x = terms[0]["x"]
    parts = []
    for t in terms:
        GL = t["GL"] if "GL" in t else epi._unstack(t["G"], t["chis"])
        GR = t["GR"] if "GR" in t else epi._unstack(t["R"], t["chis"])
        parts.append((t["s"], GL, GR, t["O"], t["G"], t["R"], t["chis"]))
    each = lambda conv: [ei.contract("dAC", {"G": G, "R": R, "O": O, "x": x}, conv) for (_s, _gl, _gr, O, G, R, _c) in parts]
    orc = sum(c * mo.dAC(x, s, GL, GR) for c, (s, GL, GR, *_rest) in zip(HSUM_COEFS, parts))
    t = {"name": name, "route": route, "cplx": cplx, "x": x, "parts": parts, "d": d, "oracle": orc}
    if kind == "int":
        t["ref"], t["bound"] = orc, None
        t["ref2"] = sum(c * y for c, y in zip(HSUM_COEFS, each(lambda a: a)))
        assert sum(abs(c) * u["magnitude"] for c, u in zip(HSUM_COEFS, terms)) < ei.LIMIT, name
    else:
        # every term inside its own bound; the coefficient and the accumulation (route 1: in the folds, route 2: alpha and
        # beta = 1 of the last stage) add two roundings per term on the sum of the absolute values
        t["ref"] = sum(c * y for c, y in zip(HSUM_COEFS, each(_hp)))
        absval = sum(abs(c) * y for c, y in zip(HSUM_COEFS, each(_abs_hp)))
        slack = [u["depth"] + 8 if "depth" in u else sum(epi.depth("hac_blocked", u)[i] * k for i, k in ((0, 1), (1, 2))) + 2 for u in terms]
        t["bound"] = (4 if cplx else 1) * LD(U) * (sum(abs(c) * k * y for c, k, y in zip(HSUM_COEFS, slack, each(_abs_hp)))
                                                   + 2 * len(terms) * absval)
    return t


def hsum_keys():
    Dl, Dr, d = 2, 4, 2
    return [(1, Dl, Dr, d, False), (2, Dl, Dr, d, False), (1, Dl, Dr, d, True), (2, Dl, Dr, d, True), (1, 1, 1, 2, False),
            (2, 1, 1, 2, False), (1, 3, 9, 3, False), (2, 3, 9, 3, False)]


# ------------------------------------------------------------------------------------------------------------------
# section 4: canonical transfers, pair transfers, Gram entries
# ------------------------------------------------------------------------------------------------------------------
def canonical_keys():
    """(side, family, Dl, d, Dr): exact_canonical_inputs.transfer_case on the whole ladder (dyadic isometries)"""
    return [(side, f, Dl, d, Dr) for side in ("l", "r") for (Dl, Dr, d) in LADDER for f in jordan_families(d)]


def pair_model(O, Dl, Dr):
    """mpsk_transfer_pair_model (host only, no device): {"pairs", "route"} as (left, right) -- the pairs the slice records
    per side (the D block adds one on the left only) and the route the model chooses at (Dl, Dr): 1 pair-Gram, 0 level by
    level"""
    import ctypes as C
    from mpskit_jl_amd import _lib
    lib = _lib.load()
    Of = np.asfortranarray(O, dtype=np.float64)
    out = [(C.c_int * 2)() for _ in range(4)]
    _lib.check(lib.mpsk_transfer_pair_model(O.shape[0], O.shape[3], O.shape[1], Of.ctypes.data_as(C.c_void_p), Dl, Dr, *out),
               "mpsk_transfer_pair_model")
    return {"pairs": tuple(out[0]), "route": tuple(out[3])}


@functools.lru_cache(maxsize=None)
def pair_case(side, Dl, Dr, d, which):
    """mpsk_transfer_left_pair / _right_pair: two transfers through one slice and one bra whose kets and environments differ
    (the second ket has another bond on the environment side)"""
    import mpskit_oracle as mo
    left = side == "l"
    chis = CHIS[which]
    W = sum(chis)
    D2 = other_bonds(Dl, Dr)[1]
    for salt in range(50):
        name = f"edge-t{side}_pair-{which}-{Dl}x{d}x{Dr}-{salt}"
        rng = _rng(name)
        s = edge_slice(which, d, "int", False, salt=str(salt) if salt else "")
        O = np.asarray(s.full(), dtype=np.float64)
        Ab = int_array(rng, Dl, d, Dr)
        if left:
            V1, A1, V2, A2 = int_array(rng, Dl, W, Dl), int_array(rng, Dl, d, Dr), int_array(rng, Dl, W, D2), int_array(rng, D2, d, Dr)
            t1, t2 = {"G": V1, "A": A1, "Ab": Ab, "O": O}, {"G": V2, "A": A2, "Ab": Ab, "O": O}
            ref = epi.contract("tl", t1) + epi.contract("tl", t2)
            orc = (epi._stack(mo.transfer_left(epi._unstack(V1, chis), s, A1, Ab))
                   + epi._stack(mo.transfer_left(epi._unstack(V2, chis), s, A2, Ab)))
            ext = [max(Dl, D2), W, d, Dl, d]
        else:
            V1, A1, V2, A2 = int_array(rng, Dr, W, Dr), int_array(rng, Dl, d, Dr), int_array(rng, D2, W, Dr), int_array(rng, Dl, d, D2)
            t1, t2 = {"R": V1, "A": A1, "Ab": Ab, "O": O}, {"R": V2, "A": A2, "Ab": Ab, "O": O}
            ref = epi.contract("tr", t1) + epi.contract("tr", t2)
            orc = (epi._stack(mo.transfer_right(epi._unstack(V1, chis), s, A1, Ab))
                   + epi._stack(mo.transfer_right(epi._unstack(V2, chis), s, A2, Ab)))
            ext = [max(Dr, D2), W, d, Dr, d]
        if np.any(ref != 0):
            break
    m = 2 * assert_exact_range([V1, A1, Ab, O], ext, name)
    t = {"name": name, "side": side, "s": s, "chis": list(chis), "V1": V1, "A1": A1, "V2": V2, "A2": A2, "Ab": Ab, "ref": ref,
         "oracle": orc, "magnitude": m}
    return t


def pair_keys():
    return [(side, Dl, Dr, d, w) for side in ("l", "r") for (Dl, Dr, d) in LADDER for w in ("chi", "min")]


@functools.lru_cache(maxsize=None)
def gram_case(Dl, Dr, d, cplx):
    """site_gram[w][t,s] = sum conj(Ab[p,t,b]) X[w][p,s,b]; transfer_left_gram: the pass-through transfer of W slabs and the
    Gram of its stage-1 product; transfer_left_gram_env: one slab closed on the right with R [Dr, Dr]"""
    W = 2
    for salt in range(50):
        name = f"edge-gram-{'c128' if cplx else 'f64'}-{Dl}x{d}x{Dr}-{salt}"
        rng = _rng(name)
        draw = functools.partial(int_array, cplx=cplx)
        X, Ab, A, V, R = draw(rng, W, Dl, d, Dr), draw(rng, Dl, d, Dr), draw(rng, Dl, d, Dr), draw(rng, Dl, W, Dl), draw(rng, Dr, Dr)
        e = functools.partial(np.einsum, optimize=False)
        site = e("ptb,wpsb->wts", np.conj(Ab), X)
        T1 = e("pwa,asb->wpsb", V, A)
        tgram = e("ptb,wpsb->wts", np.conj(Ab), T1)
        vout = epi.contract("tl0", {"G": V, "A": A, "Ab": Ab})
        egram = e("ptq,psq->ts", np.conj(Ab), e("psb,bq->psq", T1[0], R))
        if all(np.any(a != 0) for a in (site, tgram, vout, egram)):
            break
    n = 2 if cplx else 1
    assert_exact_range([V, A, Ab, R], [Dl, Dl, Dr, Dr, n, n, n, n], name)
    return {"name": name, "cplx": cplx, "W": W, "X": X, "Ab": Ab, "A": A, "V": V, "R": R, "site": site, "tgram": tgram, "vout": vout,
            "egram": egram}


def gram_keys():
    return [(Dl, Dr, d, cplx) for cplx in (False, True) for (Dl, Dr, d) in LADDER]


# ------------------------------------------------------------------------------------------------------------------
# section 5: small memory-bound entries
# ------------------------------------------------------------------------------------------------------------------
REG_SCALARS = (0.5, -2.0)                    # (a0, a1) of mpsk_regularize_axpby


@functools.lru_cache(maxsize=None)
def reg_case(W, D1, D2, cplx=False, kind="int"):
    """mpsk_regularize (fp64) and mpsk_regularize_axpby (both dtypes) at (W, D1, D2) on the ladder"""
    draw = functools.partial(int_array if kind == "int" else gauss_array, cplx=cplx)
    for salt in range(50):
        name = f"edge-reg-{kind}-{'c128' if cplx else 'f64'}-W{W}-{D1}x{D2}-{salt}"
        rng = _rng(name)
        t = {"name": name, "v": draw(rng, D1, W, D2), "lvec": draw(rng, D2, D1), "rvec": draw(rng, D1, D2), "chis": [1] * W}
        xs = draw(rng, D1, W, D2)
        t = epi._finish("reg", t, kind, cplx, dict(D1=D1, D2=D2))
        a0, a1 = REG_SCALARS
        t["xs"] = xs
        t["ref_axpby"] = a0 * (xs if kind == "int" else _hp(xs)) + a1 * t["ref"]
        if kind != "int":
            t["bound_axpby"] = abs(a1) * t["bound"] + 3 * LD(U) * (abs(a0) * _abs_hp(xs) + abs(a1) * np.abs(t["ref"]))
        if kind != "int" or (np.any(t["ref"] != 0) and np.any(t["ref"] != t["v"])):
            return t
    raise AssertionError(name)


def reg_keys():
    return [(W, Dl, Dr, cplx) for cplx in (False, True) for (Dl, Dr, _d) in LADDER for W in (1, 3)]


@functools.lru_cache(maxsize=None)
def dsum_case(side, Dl, Dr, d):
    """mpsk_dsum_site on two chain-edge tensors of bonds (Dl, Dr): what FiniteMPS + FiniteMPS does at this site.  Left:
    G [Dn, 2 Dl] (Dn = 1 at site 1: G = [1 1] when Dl = 1); right: G [2 Dr, Dn]."""
    left = side == "left"
    Dn = (1 if Dl == 1 else min(2 * Dl, MAX_BOND)) if left else (1 if Dr == 1 else min(2 * Dr, MAX_BOND))
    for salt in range(50):
        name = f"edge-dsum-{side}-{Dl}x{d}x{Dr}-{salt}"
        rng = _rng(name)
        A1, A2 = int_array(rng, Dl, d, Dr), int_array(rng, Dl, d, Dr)
        if left:
            G = np.ones((1, 2)) if Dl == 1 else int_array(rng, Dn, 2 * Dl)
            ref = np.concatenate([np.einsum("na,asb->nsb", G[:, :Dl], A1), np.einsum("na,asb->nsb", G[:, Dl:], A2)], axis=2)
        else:
            G = np.ones((2, 1)) if Dr == 1 else int_array(rng, 2 * Dr, Dn)
            ref = np.concatenate([np.einsum("asb,bn->asn", A1, G[:Dr]), np.einsum("asb,bn->asn", A2, G[Dr:])], axis=0)
        if np.any(ref[..., :1] != 0) and np.any(ref != 0):
            break
    assert_exact_range([G, A1], [max(Dl, Dr)], name)
    ref_hp = (np.concatenate([np.einsum("na,asb->nsb", _hp(G[:, :Dl]), _hp(A1)), np.einsum("na,asb->nsb", _hp(G[:, Dl:]), _hp(A2))], axis=2)
              if left else np.concatenate([np.einsum("asb,bn->asn", _hp(A1), _hp(G[:Dr])), np.einsum("asb,bn->asn", _hp(A2), _hp(G[Dr:]))], axis=0))
    return {"name": name, "side": side, "G": G, "A1": A1, "A2": A2, "ref": ref, "ref_hp": ref_hp}


def dsum_keys():
    return [(side, Dl, Dr, d) for side in ("left", "right") for (Dl, Dr, d) in LADDER]


COPY_SHAPES = [(1, 1), (1, 3), (3, 1)]


@functools.lru_cache(maxsize=None)
def copy_case(rows, cols):
    """mpsk_copy2d / mpsk_cx_embed / mpsk_cx_half with padded leading dimensions: source padding NaN, destination pre-filled
    with a sentinel pattern.  cx: H is rows x cols complex (2 rows x cols doubles), E its real 2 rows x 2 cols embedding."""
    name = f"edge-copy-{rows}x{cols}"
    rng = _rng(name)
    src = int_array(rng, rows, cols) + 5.0                              # never zero
    H = int_array(rng, rows, cols, cplx=True) + (5.0 + 5.0j)
    Hd = np.empty((2 * rows, cols)); Hd[0::2], Hd[1::2] = H.real, H.imag
    E = np.empty((2 * rows, 2 * cols))
    E[:, 0::2] = Hd
    E[0::2, 1::2], E[1::2, 1::2] = -H.imag, H.real                      # J h: (re, im) -> (-im, re)
    Ez = np.empty((rows, 2, cols, 2), dtype=np.float64)                 # the same from the 2 x 2 block of a complex number
    Ez[:, 0, :, 0], Ez[:, 1, :, 0], Ez[:, 0, :, 1], Ez[:, 1, :, 1] = H.real, H.imag, -H.imag, H.real
    assert np.array_equal(E, Ez.reshape(2 * rows, 2 * cols))
    # a nearly embedded matrix: structured part + an integer perturbation that the structured part averages to halves
    Ep = E + int_array(rng, 2 * rows, 2 * cols)
    half = np.empty((2 * rows, cols))
    half[0::2] = (Ep[0::2, 0::2] + Ep[1::2, 1::2]) / 2
    half[1::2] = (Ep[1::2, 0::2] - Ep[0::2, 1::2]) / 2
    return {"name": name, "rows": rows, "cols": cols, "src": src, "Hd": Hd, "E": E, "Ep": Ep, "half": half}


# ------------------------------------------------------------------------------------------------------------------
# the whole-edge composite: one walk over the seven sites of the d = 2 ladder
# ------------------------------------------------------------------------------------------------------------------
COMPOSITE_RANGE = 1


def _walk_int(rng, r, *shape):
    while True:
        a = rng.integers(-r, r + 1, size=shape).astype(np.float64)
        if np.any(a != 0):
            return a


@functools.lru_cache(maxsize=None)
def composite(which="chi"):
    """Seven sites in chain order with bonds LADDER_D2, one slice per site (all of family `which`), integer tensors in
    [-COMPOSITE_RANGE, COMPOSITE_RANGE].  GL[0] / GR[7] are the chain-edge environments [1, W, 1]; left environments are
    carried site by site with transfer_left, right ones with transfer_right; at each site dAC of the site tensor, at
    each bond dC of a bond matrix.  Every carried environment re-enters the next step, so the magnitude grows by the
    contracted extents per site: assert_exact_range is applied to every step with the environment's actual maximum."""
    for salt in range(200):
        out = _composite(which, salt)
        if all(np.any(a != 0) for k in ("GL", "GR", "dAC", "dC") for a in out[k]):      # no step of the walk is vacuous
            return out
    raise AssertionError(which)


def _composite(which, salt):
    import mpskit_oracle as mo
    d = 2
    chis = CHIS[which]
    W = sum(chis)
    name = f"edge-composite-{which}-{salt}"
    rng = _rng(name)
    r = COMPOSITE_RANGE
    L = len(LADDER_D2)
    sites = []
    for i, (Dl, Dr) in enumerate(LADDER_D2):
        s = edge_slice(which, d, "int", False, salt=f"walk{i}-{salt}")
        sites.append({"s": s, "O": np.asarray(s.full(), dtype=np.float64), "A": _walk_int(rng, r, Dl, d, Dr), "x": _walk_int(rng, r, Dl, d, Dr),
                      "c": _walk_int(rng, r, Dr, Dr), "Dl": Dl, "Dr": Dr})
    GL = [_walk_int(rng, r, 1, W, 1)]
    GR = [None] * L + [_walk_int(rng, r, 1, W, 1)]
    GLo, GRo = [GL[0]], list(GR)
    for i, st in enumerate(sites):
        t = {"G": GL[i], "A": st["A"], "Ab": st["A"], "O": st["O"]}
        assert_exact_range([GL[i], st["A"], st["A"], st["O"]], [st["Dl"], W, d, st["Dl"], d], f"{name} GL[{i + 1}]")
        GL.append(epi.contract("tl", t))
        GLo.append(epi._stack(mo.transfer_left(epi._unstack(GLo[i], chis), st["s"], st["A"], st["A"])))
    for i in range(L - 1, -1, -1):
        st = sites[i]
        t = {"R": GR[i + 1], "A": st["A"], "Ab": st["A"], "O": st["O"]}
        assert_exact_range([GR[i + 1], st["A"], st["A"], st["O"]], [st["Dr"], W, d, st["Dr"], d], f"{name} GR[{i}]")
        GR[i] = epi.contract("tr", t)
        GRo[i] = epi._stack(mo.transfer_right(epi._unstack(GRo[i + 1], chis), st["s"], st["A"], st["A"]))
    dAC, dC, dACo, dCo = [], [], [], []
    for i, st in enumerate(sites):
        t = {"G": GL[i], "R": GR[i + 1], "x": st["x"], "O": st["O"]}
        assert_exact_range([GL[i], GR[i + 1], st["x"], st["O"]], [st["Dl"], W, d, st["Dr"], W], f"{name} dAC[{i}]")
        dAC.append(epi.contract("dAC", t))
        dACo.append(mo.dAC(st["x"], st["s"], epi._unstack(GL[i], chis), epi._unstack(GR[i + 1], chis)))
        t = {"G": GL[i + 1], "R": GR[i + 1], "x": st["c"]}
        assert_exact_range([GL[i + 1], GR[i + 1], st["c"]], [st["Dr"], st["Dr"], W], f"{name} dC[{i}]")
        dC.append(epi.contract("dC", t))
        dCo.append(mo.dC(st["c"], epi._unstack(GL[i + 1], chis), epi._unstack(GR[i + 1], chis)))
    out = {"name": name, "chis": list(chis), "sites": sites, "GL": GL, "GR": GR, "dAC": dAC, "dC": dC,
           "oracle": {"GL": GLo, "GR": GRo, "dAC": dACo, "dC": dCo}}
    for v in GL + GR + dAC + dC:
        v.setflags(write=False)
    return out


COMPOSITE_SLICES = ("chi", "five", "min")


# ------------------------------------------------------------------------------------------------------------------
# quasiparticle entries: mpsk_qp_half, mpsk_qp_apply, mpsk_qp_heff_site through tests/exact_qp_inputs.py
# ------------------------------------------------------------------------------------------------------------------
QP_OPS = ("qp_half", "qp_apply", "qp_heff")


def qp_bonds(Dl, Dr, d):
    """((Dlo, Dl, Dl2, Dr, Dr2, Dro), (Dl, Dl2, Dr, Dr2, n)) in the order of exact_qp_inputs.SHAPES: the second kets' bonds
    from the ladder; n = Dl d - Dr columns of VL (the complement of an AL [Dl, d, Dr]), at least one and at most 9"""
    Dlo, Dm, Dro = other_bonds(Dl, Dr)
    Dr2 = BONDS[(BONDS.index(Dm) + 2) % len(BONDS)]
    n = min(MAX_BOND, max(1, Dl * d - Dr))
    return (Dlo, Dl, Dm, Dr, Dr2, Dro), (Dl, Dm, Dr, Dr2, n)


@functools.lru_cache(maxsize=None)
def qp_case(op, Dl, Dr, d, which, kind="int"):
    """one case record of exact_qp_inputs (operands once, one reference and bound per sub-case key: with and without
    the optional pairs, E = 0 and dyadic) on an edge slice at ladder bonds; MPSK_F64 only.  op: QP_OPS, tl_pair, tr_pair."""
    import exact_qp_inputs as eq
    bonds, heff = qp_bonds(Dl, Dr, d)
    for salt in range(50):
        name = f"edge-{op}-{which}-{kind}-{Dl}x{d}x{Dr}" + (f"-salt{salt}" if salt else "")
        rng = _rng(name)
        s = edge_slice(which, d, kind, False, salt=f"qp{salt}")
        draw = (lambda k, *shp: int_array(rng, *shp)) if kind == "int" else (lambda k, *shp: gauss_array(rng, *shp))
        t = {"name": name, "dense": False, "s": s, "O": np.asarray(s.full(), dtype=np.float64), "chis": list(s.chil),
             "slice_args": (s.odim, s.d, list(s.chil), list(s.chir), dict(s.Os)), "ranges": {}}
        eq._operands(op, t, rng, draw, bonds, heff, d, sum(s.chil))
        t = eq._finish(op, t, kind, "edge")
        if kind != "int" or all(np.any(r != 0) for r in t["refs"].values()):
            return t
    raise AssertionError(name)


def qp_oracle(t, key):
    """the second reference of a sub-case: every term through mpskit_oracle.dAC / transfer_left / transfer_right (block
    by block) instead of the dense O"""
    import exact_qp_inputs as eq
    import mpskit_oracle as mo
    op, s, chis = t["op"], t["s"], t["chis"]
    un = lambda k: epi._unstack(t[k], chis)
    if op == "tl_pair":
        return sum(epi._stack(mo.transfer_left(un("V" + i), s, t["A" + i], t["Ab"])) for i in "12")
    if op == "tr_pair":
        return sum(epi._stack(mo.transfer_right(un("V" + i), s, t["A" + i], t["Ab"])) for i in "12")
    if op == "qp_half":
        return None
    combo, E = key if op == "qp_heff" else (key, 0.0)
    left, right = eq.has_pairs(combo)
    B = eq.site_of(t["VL"], t["X"], s.d) if op == "qp_heff" else t["B"]
    y = mo.dAC(B, s, un("G"), un("R"))
    if left:
        y = y + mo.dAC(t["AR"], s, un("lB"), un("R"))
    if right:
        y = y + mo.dAC(t["AL"], s, un("G"), un("rB"))
    return eq.pull(t["VL"], y) - E * t["X"] if op == "qp_heff" else y


def qp_keys():
    return [(op, Dl, Dr, d, w) for op in QP_OPS for (Dl, Dr, d) in LADDER for w in SLICES]


def qp_gauss_keys():
    Dl, Dr, d = GAUSS_SHAPE
    return [(op, Dl, Dr, d, "chi") for op in QP_OPS + ("tl_pair", "tr_pair")]


# ------------------------------------------------------------------------------------------------------------------
# Gaussian cases of the Gram entries and of mpsk_dsum_site at (3, 7), d = 3
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def gram_gauss(cplx):
    """Bounds, (4 if complex else 1) * depth * u * the same contraction of the absolute values.  site_gram: one inner
    product over (p, b), depth Dl Dr (tests/test_gpu_site_gram.py; its separate complex bounds on the two components,
    2 Dl Dr u each, give a modulus below 4 Dl Dr u).  transfer_left_gram: the stage-1 product (a: Dl) under the Gram,
    two roundings of slack at the stage boundary.  transfer_left_gram_env: stage 1 (Dl), the closing product (Dr), the
    epilogue contraction over (p, q), four roundings of slack.  Vout / Lout: exact_proj_inputs.depth("tl0")."""
    Dl, Dr, d = GAUSS_SHAPE
    W = 2
    name = f"edge-gram-gauss-{'c128' if cplx else 'f64'}"
    rng = _rng(name)
    draw = functools.partial(gauss_array, cplx=cplx)
    t = {"name": name, "cplx": cplx, "W": W, "X": draw(rng, W, Dl, d, Dr), "Ab": draw(rng, Dl, d, Dr), "A": draw(rng, Dl, d, Dr),
         "V": draw(rng, Dl, W, Dl), "R": draw(rng, Dr, Dr)}
    e = functools.partial(np.einsum, optimize=False)

    def all_of(f, cj):
        X, Ab, A, V, R = (f(t[k]) for k in ("X", "Ab", "A", "V", "R"))
        T1 = e("pwa,asb->wpsb", V, A)
        return {"site": e("ptb,wpsb->wts", cj(Ab), X), "tgram": e("ptb,wpsb->wts", cj(Ab), T1),
                "egram": e("ptq,psq->ts", cj(Ab), e("psb,bq->psq", T1[0], R)),
                "vout": e("psq,pwsb->qwb", cj(Ab), e("pwa,asb->pwsb", V, A))}

    ref, av, f64 = all_of(_hp, np.conj), all_of(_abs_hp, lambda a: a), all_of(lambda a: a, np.conj)
    c = (4 if cplx else 1) * LD(U)
    dd, n = epi.depth("tl0", {"A": t["A"], "Ab": t["Ab"]})
    depths = {"site": Dl * Dr, "tgram": Dl + Dl * Dr + 2, "egram": Dl + Dr + Dl * Dr + 4, "vout": dd + 2 * n + 2}
    for k in ref:
        t[k], t["bound_" + k], t["fp64_" + k] = ref[k], c * depths[k] * av[k], f64[k]
    return t


@functools.lru_cache(maxsize=None)
def dsum_gauss(side):
    """mpsk_dsum_site on Gaussian tensors of bonds (3, 7), d = 3; the bound of tests/test_gpu_dsum_site.py: K u sum |G| |A|
    per entry, K the contracted extent of the block the entry belongs to (both blocks have the same one here)"""
    Dl, Dr, d = GAUSS_SHAPE
    left = side == "left"
    Dn = 5
    name = f"edge-dsum-gauss-{side}"
    rng = _rng(name)
    A1, A2 = gauss_array(rng, Dl, d, Dr), gauss_array(rng, Dl, d, Dr)
    G = gauss_array(rng, Dn, 2 * Dl) if left else gauss_array(rng, 2 * Dr, Dn)

    def ref(f):
        g, a1, a2 = f(G), f(A1), f(A2)
        if left:
            return np.concatenate([np.einsum("na,asb->nsb", g[:, :Dl], a1), np.einsum("na,asb->nsb", g[:, Dl:], a2)], axis=2)
        return np.concatenate([np.einsum("asb,bn->asn", a1, g[:Dr]), np.einsum("asb,bn->asn", a2, g[Dr:])], axis=0)

    K = Dl if left else Dr
    return {"name": name, "side": side, "G": G, "A1": A1, "A2": A2, "ref": ref(_hp), "bound": K * LD(U) * ref(_abs_hp),
            "fp64": ref(lambda a: a)}


def hac_gauss_keys():
    """(cplx, MPSK_HAC_MODE or None): the Gaussian prepared-operator cases of modes 0, 1 (real, forced) and 2 (complex)"""
    return [(False, "0"), (False, "1"), (True, None)]


def hsum_gauss_keys():
    Dl, Dr, d = GAUSS_SHAPE
    return [(route, Dl, Dr, d, cplx) for cplx in (False, True) for route in (1, 2)]


# ------------------------------------------------------------------------------------------------------------------
# the case list
# ------------------------------------------------------------------------------------------------------------------
def case_ids():
    """one id per case of the module (a GEMM group of 216 shapes counts once); tests/test_edge_shape_cases_cpu.py holds the
    count to a literal"""
    ids = [g.name for g in gemm_groups()] + [c.name for c in GEMM_GAUSS]
    ids += [f"gemm_pair-{M}x{N}x{K}-{q}" for (M, N, K, q) in gemm_pair_keys()]
    ids += [key_id(k) for k in op_keys()] + ["gauss-" + key_id(k) for k in op_gauss_keys()]
    ids += [f"hac3-{f}-{'c128' if c else 'f64'}-{Dl}x{Dr}" for (f, Dl, Dr, c) in hac3_keys()]
    ids += [f"hsum{r}-{'c128' if c else 'f64'}-{Dl}x{d}x{Dr}" for (r, Dl, Dr, d, c) in hsum_keys()]
    ids += [f"canonical-t{s}-{f}-{Dl}x{d}x{Dr}" for (s, f, Dl, d, Dr) in canonical_keys()]
    ids += [f"t{s}_pair-{w}-{Dl}x{d}x{Dr}" for (s, Dl, Dr, d, w) in pair_keys()]
    ids += [f"gram-{'c128' if c else 'f64'}-{Dl}x{d}x{Dr}" for (Dl, Dr, d, c) in gram_keys()]
    ids += [f"reg-{'c128' if c else 'f64'}-W{W}-{D1}x{D2}" for (W, D1, D2, c) in reg_keys()]
    ids += [f"dsum-{s}-{Dl}x{d}x{Dr}" for (s, Dl, Dr, d) in dsum_keys()]
    ids += [f"copy-{r}x{c}" for (r, c) in COPY_SHAPES] + [f"composite-{w}" for w in COMPOSITE_SLICES]
    ids += ["gauss-hac3-f64", "gauss-hac3-c128", "gauss-canonical-tl", "gauss-canonical-tr", "gauss-reg-f64", "gauss-reg-c128"]
    ids += [f"{op}-{w}-{Dl}x{d}x{Dr}" for (op, Dl, Dr, d, w) in qp_keys()] + [f"gauss-{k[0]}" for k in qp_gauss_keys()]
    ids += ["gauss-gemm_pair", "gauss-gram-f64", "gauss-gram-c128", "gauss-dsum-left", "gauss-dsum-right"]
    ids += [f"gauss-hac-{'c128' if c else 'f64'}-mode{m or 2}" for (c, m) in hac_gauss_keys()]
    ids += [f"gauss-hsum{r}-{'c128' if c else 'f64'}" for (r, _a, _b, _d, c) in hsum_gauss_keys()]
    return ids
