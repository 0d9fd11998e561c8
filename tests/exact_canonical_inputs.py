"""Exact inputs for the Jordan-form H_AC (mpsk_hac mode 3, real and complex) and the canonical environment transfers.

Both routes rest on promises: level 0 of GL / level W-1 of GR is the identity, and for the transfers A is an isometry.
All of them can be kept with numbers fp64 never rounds, so the whole computation -- the folds GRc0 / GLc, the per-batch-
table GEMMs, the elementwise plans tl / tr and the final contraction with A -- is exact and ANY correct route returns the
bits of the general oracle (mo.dAC / mo.transfer_left / mo.transfer_right on the same operands):

  * an identity level is integer data, and mode 3 asks for nothing else: every other level of the environments, the
    vector and every block of the slice hold integers in [-4, 4] (Gaussian integers for the complex twin, the corners of
    the slice exactly real);
  * H_k / sqrt(k) is orthogonal with entries +-2^-j for k = 4^j.  A block-diagonal sum of such matrices, k in
    {1, 4, 16, 64, 256}, shuffled by fixed signed row and column permutations, is an n x n orthogonal matrix for every n,
    and its first columns are an isometry whose entries are integer multiples of a power of two.

Guard.  Every operand is an integer multiple of a unit 2^-e; the result and every partial sum of every bracket order is a
multiple of the product of the units and no larger than exact_inputs.magnitude(operands, contracted extents).  Each case
asserts magnitude / unit < 2^50, so nothing is ever rounded.  tests/test_exact_canonical_inputs_cpu.py also multiplies the
small shapes out in longdouble and finds the bits of the fp64 oracle.

The slices (levels 0 and W-1 have chi = 1, O[0,0] = O[W-1,W-1] = 1, no block with w > 0 and v < W-1):
  full    d = 2, chis (1,1,1,1,1): every C, B and D block a dense 2 x 2 block without a zero: both folds use all d^2 slabs
  sparse  d = 3, chis (1,1,1,1), no D block; C blocks strictly upper, B blocks strictly lower triangular in (t, s): the
          per-t slab lists have lengths 3, 2, 1 (1, 2, 3) and are padded with the empty slab, the two families use
          different slab sets, and the T slab of transfer_left is overwritten (beta = 0)
  chi     d = 2, chis (1,3,2,1): C / B blocks [1,d,d,chi] / [chi,d,d,1], the D block the scalar block 3.0
  onsite  W = 2, chis (1,1), only a D block: the plan tr is empty and T == T2 in transfer_left
jordan_mirror() repeats the few host lines of mposlice_build that decide the Jordan form and the segment counts; NSEG
holds what each family must give.

One Gaussian case per route (mode 3 real, mode 3 complex, left and right transfer), because integers would survive a
stray fp32 path: identity levels exact, every other entry Gaussian, A the Q factor of a Gaussian matrix.  The check is the
componentwise bound of exact_inputs, (depth + 8) u times the same contraction of the absolute values in longdouble (x 4
for complex), with depth the sum of the contracted extents of every stage of the route:

  mode 3            fold GRc0 (v: Wr), fold GLc (w: Wl), one K loop over both families (d Dr + d Dl):
                        depth = Wr + Wl + d (Dl + Dr)
  transfer_left     level W-1: fold GLc (w: Wl), T = GLc A (+ the plan tl over s: d) (K = d Dl, + d), A^T T (K = Dl d);
                    the levels 0 < v < W-1 see only the plan (d) and A^T T2 (Dl d):
                        depth = Wl + d + 2 d Dl
  transfer_right    level 0: fold GRc0 (v: Wr), X = A GRc0 (K = d Dr), X A^T (K = d Dr); the levels between: plan tr (d)
                    and X A^T (d Dr):
                        depth = Wr + d + 2 d Dr

(the three-stage bracket of the oracle has Dl + Wl d + Dl d resp. Dr + Wr d + d Dr, never more).  Identity terms are
multiplications by exact ones and zeros in the reference too, so route and reference sum the same products.  The identity
level of a canonical transfer's output is written, not computed: it is compared with np.eye by array_equal and left out
of the bound.  numpy_folded() evaluates the folded forms in plain fp64; the CPU test holds it (and the oracle) to every
bound, and to the oracle's bits on the integer cases.
"""
from __future__ import annotations

import functools

import numpy as np

import exact_inputs as ei
from exact_factor_inputs import hadamard

FAMILIES = ("full", "sparse", "chi", "onsite")
CHIS = {"full": (1, 1, 1, 1, 1), "sparse": (1, 1, 1, 1), "chi": (1, 3, 2, 1), "onsite": (1, 1)}
DPHYS = {"full": 2, "sparse": 3, "chi": 2, "onsite": 2}
NSEG = {"full": (2, 2), "sparse": (3, 3), "chi": (2, 2), "onsite": (2, 1)}      # (jr_nseg, jl_nseg)
PADDED = {"full": (False, False), "sparse": (True, True), "chi": (False, False), "onsite": (False, False)}
HADAMARD_ORDERS = (256, 64, 16, 4, 1)
LD_MAX_WORK = 3 * 10 ** 7               # multiply-adds of the first stage up to which a case is also run in longdouble

# (Dl, Dr) of mode 3: one launch aligned / one launch with odd tables / two launches even / two launches odd
HAC_SHAPES = [(128, 128), (65, 65), (34, 66), (33, 65)]
HAC_LAUNCH2_SHAPES = [(128, 128), (65, 65)]
HAC_C128_FAMILIES = ("full", "sparse")
HAC_C128_SHAPES = [(33, 65), (128, 128)]
LONGK = 256
# (Dl, d, Dr) of transfer_left; transfer_right takes the mirror image (Dr, d, Dl).  (16, 2, 32) and (1, 2, 2): square
# isometries (growing bond, chain edge); (43, 3, 129): an odd square one with more than one block of every tile
TRANSFER_SHAPES_D2 = [(128, 2, 128), (33, 2, 65), (16, 2, 32), (1, 2, 2)]
TRANSFER_SHAPES_D3 = [(5, 3, 9), (4, 3, 12), (43, 3, 129)]
GAUSS_CASES = [("hac", "chi", False), ("hac", "full", True), ("tl", "chi", False), ("tr", "chi", False)]
GAUSS_HAC_SHAPE = (33, 65)
GAUSS_TRANSFER_SHAPE = (33, 2, 65)


def transfer_shapes(family, side):
    """the shapes one slice handle is applied at, in order; the first one comes again at the end (table caches)"""
    shapes = TRANSFER_SHAPES_D3 if DPHYS[family] == 3 else TRANSFER_SHAPES_D2
    if side == "r":
        shapes = [(Dr, d, Dl) for (Dl, d, Dr) in shapes]
    return list(shapes) + [shapes[0]]


# ------------------------------------------------------------------------------------------------------------------
# slices
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def jordan_slice(family, kind="int", cplx=False):
    """(oracle slice, dense O[Wl, d, d, Wr]) of one family; kind "gauss": the same pattern with Gaussian entries"""
    import mpskit_oracle as mo
    chis, d = CHIS[family], DPHYS[family]
    W = len(chis)
    rng = ei._rng(f"jordan-{family}-{kind}-{cplx}")
    draw = ei.int_array if kind == "int" else ei.gauss_array
    upper, lower = np.triu(np.ones((d, d)), 1), np.tril(np.ones((d, d)), -1)        # in (t, s)

    def block(cl, cr, mask=None):
        b = draw(rng, cl, d, d, cr, cplx=cplx)
        if kind == "int":
            b = np.where(b == 0, 1.0, b)                    # a dense block: no entry is zero
        return b if mask is None else b * mask[None, :, :, None]

    blocks = {(0, 0): 1.0, (W - 1, W - 1): 1.0}
    for w in range(1, W - 1):
        blocks[(0, w)] = block(1, chis[w], upper if family == "sparse" else None)               # C
        blocks[(w, W - 1)] = block(chis[w], 1, lower if family == "sparse" else None)           # B
    if family in ("full", "onsite"):
        blocks[(0, W - 1)] = block(1, 1)                                                         # D
    if family == "chi":
        blocks[(0, W - 1)] = 3.0
    s = mo.SparseMPOSlice(W, d, list(chis), list(chis), blocks)
    assert set(s.Os) == set(blocks), (family, sorted(s.Os))
    O = s.full()
    O.setflags(write=False)
    return s, O


def jordan_mirror(O):
    """The host lines of mposlice_build that decide the Jordan form: corners exactly the identity, nothing enters level 0
    or leaves level W-1 otherwise; slab p = s + d t of the right (left) fold is used when some O[0,t,s,v] (O[w>0,t,s,W-1])
    is non-zero; per t the used slabs are listed and the lists padded to the longest."""
    Wl, d, _, Wr = O.shape
    eye = np.eye(d)
    ok = (Wl >= 2 and Wr >= 2 and np.array_equal(O[0, :, :, 0], eye) and np.array_equal(O[Wl - 1, :, :, Wr - 1], eye)
          and not np.any(O[1:, :, :, :Wr - 1]))
    r_used = np.any(O[0] != 0, axis=2)                                  # [t, s]
    l_used = np.any(O[1:, :, :, Wr - 1] != 0, axis=0)                   # [t, s]
    nr, nl = r_used.sum(axis=1), l_used.sum(axis=1)
    return {"jordan": bool(ok and nr.max() > 0 and nl.max() > 0), "jr_nseg": int(nr.max()), "jl_nseg": int(nl.max()),
            "jr_padded": bool(nr.min() < nr.max()), "jl_padded": bool(nl.min() < nl.max()),
            "r_used": r_used, "l_used": l_used, "nslabs": 2 * d * d,    # mpsk_hac_info: both folds have d^2 output slabs
            "tl_dblock": bool(np.any(O[0, :, :, Wr - 1] != 0)) if Wr > 1 else False}


# ------------------------------------------------------------------------------------------------------------------
# environments and isometries
# ------------------------------------------------------------------------------------------------------------------
def env(rng, draw, D, chis, ident, cplx=False):
    """[D, chi, D] per level from `draw`; level `ident` (chi = 1) the identity"""
    out = [draw(rng, D, c, D, cplx=cplx) for c in chis]
    out[ident] = np.eye(D, dtype=out[0].dtype)[:, None, :].copy()
    return out


def dyadic_orthogonal(n, name):
    """n x n orthogonal, entries 0 or +-2^-j: blocks H_k / sqrt(k), k = 4^j, under fixed signed permutations"""
    Q = np.zeros((n, n))
    o = 0
    for k in HADAMARD_ORDERS:
        while n - o >= k:
            Q[o:o + k, o:o + k] = hadamard(k) * (1.0 / (1 << (k.bit_length() // 2)))        # 1 / sqrt(4^j) = 2^-j
            o += k
    rng = ei._rng(f"perm-{name}-{n}")
    pr, pc = rng.permutation(n), rng.permutation(n)
    sr, sc = rng.choice([-1.0, 1.0], n), rng.choice([-1.0, 1.0], n)
    Q = (sr[:, None] * Q[pr])[:, pc] * sc[None, :]
    assert np.array_equal(Q.T @ Q, np.eye(n)) and np.array_equal(Q @ Q.T, np.eye(n)), n
    return Q


def dyadic_unit(a):
    """the power of two every entry of `a` is an integer multiple of"""
    nz = np.abs(a[a != 0])
    u = float(nz.min())
    assert u == 2.0 ** np.round(np.log2(u)) and np.array_equal(a / u, np.round(a / u)), u
    return u


def left_isometry(Dl, d, Dr, kind="int"):
    """A[Dl, d, Dr] with sum_{p,t} A[p,t,q] A[p,t,b] = delta_qb, exactly for kind "int" """
    assert Dr <= Dl * d
    if kind == "int":
        A = dyadic_orthogonal(Dl * d, "left")[:, :Dr].reshape(Dl, d, Dr).copy()
        assert np.array_equal(np.einsum("ptq,ptb->qb", A, A), np.eye(Dr))
    else:
        A = np.linalg.qr(ei.gauss_array(ei._rng(f"isoL-{Dl}-{d}-{Dr}"), Dl * d, Dr))[0].reshape(Dl, d, Dr).copy()
    return A


def right_isometry(Dl, d, Dr, kind="int"):
    """A[Dl, d, Dr] with sum_{t,b} A[a,t,b] A[p,t,b] = delta_ap: the transpose of the construction above"""
    assert Dl <= d * Dr
    if kind == "int":
        A = dyadic_orthogonal(d * Dr, "right")[:, :Dl].T.reshape(Dl, d, Dr).copy()
        assert np.array_equal(np.einsum("atb,ptb->ap", A, A), np.eye(Dl))
    else:
        A = np.linalg.qr(ei.gauss_array(ei._rng(f"isoR-{Dl}-{d}-{Dr}"), d * Dr, Dl))[0].T.reshape(Dl, d, Dr).copy()
    return A


# ------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------
def _freeze(t):
    for v in t.values():
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return t


def _guard(t, operands, contracted, unit=1.0):
    m = ei.magnitude(operands, contracted)
    assert m / unit < ei.LIMIT, f"{t['name']}: magnitude {m:.3e} / unit {unit:.3e} is not below 2^50"
    t["magnitude"], t["unit"] = m, unit


@functools.lru_cache(maxsize=None)
def hac_case(family, Dl, Dr, kind="int", cplx=False):
    """operands of one mode-3 matvec: integer (Gaussian) environments [D, W, D] with GL[0] = GR[W-1] = 1, the oracle's
    result and the bound (None: exact).  Built once, shared, never modified."""
    import mpskit_oracle as mo
    s, O = jordan_slice(family, kind, cplx)
    chis, d = CHIS[family], DPHYS[family]
    W = sum(chis)
    name = f"hac3-{family}-{kind}-{'c128' if cplx else 'f64'}-{Dl}x{Dr}"
    rng = ei._rng(name)
    draw = ei.int_array if kind == "int" else ei.gauss_array
    t = {"name": name, "op": "dAC", "family": family, "s": s, "O": O, "chis": list(chis), "d": d, "cplx": cplx,
         "mirror": jordan_mirror(O)}
    t["GL"] = env(rng, draw, Dl, chis, 0, cplx)
    t["GR"] = env(rng, draw, Dr, chis, len(chis) - 1, cplx)
    t["G"], t["R"] = ei._stack(t["GL"]), ei._stack(t["GR"])
    t["x"] = draw(rng, Dl, d, Dr, cplx=cplx)
    t["work"] = Dl * W * Dl * d * Dr
    if kind == "int":
        ops = [t["G"], t["R"], t["x"], O]
        _guard(t, ops, [Dl, W, d, Dr, W] + [2 if cplx else 1] * len(ops))
        t["ref"], t["bound"] = mo.dAC(t["x"], s, t["GL"], t["GR"]), None
    else:
        t["depth"] = 2 * W + d * (Dl + Dr)
        t["ref"] = ei.contract("dAC", t, ei._hp)
        t["bound"] = (4 if cplx else 1) * (t["depth"] + 8) * ei.LD(ei.U) * ei.contract("dAC", t, ei._abs_hp)
        t["oracle"] = lambda: mo.dAC(t["x"], s, t["GL"], t["GR"])
    return _freeze(t)


@functools.lru_cache(maxsize=None)
def transfer_case(side, family, Dl, d, Dr, kind="int"):
    """operands of one canonical transfer (side "l" / "r"): the isometry A (== Ab), the input environment with its
    identity level, the oracle's result stacked over the levels, the bound (None: exact) and the index of the level
    the route writes"""
    import mpskit_oracle as mo
    assert d == DPHYS[family]
    s, O = jordan_slice(family, kind, False)
    chis = CHIS[family]
    W = sum(chis)
    left = side == "l"
    op = "tl" if left else "tr"
    name = f"{op}-{family}-{kind}-{Dl}x{d}x{Dr}"
    rng = ei._rng(name)
    draw = ei.int_array if kind == "int" else ei.gauss_array
    t = {"name": name, "op": op, "family": family, "s": s, "O": O, "chis": list(chis), "d": d, "cplx": False,
         "mirror": jordan_mirror(O), "ident": 0 if left else W - 1, "n_out": Dr if left else Dl}
    t["A"] = (left_isometry if left else right_isometry)(Dl, d, Dr, kind)
    t["Ab"] = t["A"]
    Dk = Dl if left else Dr                                 # the side the input environment lives on
    if left:
        t["GL"] = env(rng, draw, Dl, chis, 0)
        t["G"] = ei._stack(t["GL"])
        oracle = lambda: ei._stack(mo.transfer_left(t["GL"], s, t["A"], t["A"]))
    else:
        t["GR"] = env(rng, draw, Dr, chis, len(chis) - 1)
        t["R"] = ei._stack(t["GR"])
        oracle = lambda: ei._stack(mo.transfer_right(t["GR"], s, t["A"], t["A"]))
    t["work"] = Dk * W * Dk * d * (Dr if left else Dl)
    if kind == "int":
        u = dyadic_unit(t["A"])
        _guard(t, [t["G" if left else "R"], t["A"], t["A"], O], [Dk, W, d, Dk, d], unit=u * u)
        t["ref"], t["bound"] = oracle(), None
    else:
        t["depth"] = W + d + 2 * d * Dk
        t["ref"] = ei.contract(op, t, ei._hp)
        t["bound"] = (t["depth"] + 8) * ei.LD(ei.U) * ei.contract(op, t, ei._abs_hp)
        t["oracle"] = oracle
    return _freeze(t)


def gauss_case(route, family, cplx):
    if route == "hac":
        return hac_case(family, *GAUSS_HAC_SHAPE, "gauss", cplx)
    Dl, d, Dr = GAUSS_TRANSFER_SHAPE
    return transfer_case("l", family, Dl, d, Dr, "gauss") if route == "tl" else transfer_case("r", family, Dr, d, Dl, "gauss")


def hp_reference(t):
    """the contraction in longdouble (operands converted exactly)"""
    return ei.contract(t["op"], t, ei._hp)


def numpy_folded(t):
    """The folded forms the routes evaluate, in plain numpy at the operands' own precision:
         mode 3          y[:,t,:] = sum_s x[:,s,:] GRc0[s,t] + sum_s GLc[s,t] x[:,s,:]
         transfer_left   level 0 = 1;  0 < v < W-1: A^T (O[0,:,:,v] A);  W-1: A^T (GLc A + O[0,:,:,W-1] A)
         transfer_right  level W-1 = 1;  0 < w < W-1: (O[w,:,:,W-1] A) A^T;  0: (A GRc0) A^T
       with GRc0[s,t] = sum_v O[0,t,s,v] GR[v] and GLc[s,t] = sum_{w>0} O[w,t,s,W-1] GL[w]."""
    O = t["O"]
    W = O.shape[0]
    e = np.einsum
    if t["op"] == "dAC":
        GRc0 = e("tsv,bvq->stbq", O[0], t["R"])
        GLc = e("wts,pwa->stpa", O[1:, :, :, W - 1], t["G"][:, 1:, :])
        return e("asb,stbq->atq", t["x"], GRc0) + e("stpa,asq->ptq", GLc, t["x"])
    A = t["A"]
    if t["op"] == "tl":
        GLc = e("wts,pwa->stpa", O[1:, :, :, W - 1], t["G"][:, 1:, :])
        T2 = e("tsv,psb->vptb", O[0, :, :, 1:], A)                                 # levels 1 .. W-1
        T2[W - 2] += e("stpa,asb->ptb", GLc, A)
        out = np.empty((A.shape[2], W, A.shape[2]), dtype=A.dtype)
        out[:, 0, :] = np.eye(A.shape[2])
        out[:, 1:, :] = e("ptq,vptb->qvb", A, T2)
        return out
    GRc0 = e("tsv,bvq->stbq", O[0], t["R"])
    X = np.empty((W - 1,) + A.shape, dtype=A.dtype)                                # levels 0 .. W-2
    X[0] = e("asb,stbq->atq", A, GRc0)
    X[1:] = e("wts,asb->watb", O[1:W - 1, :, :, W - 1], A)
    out = np.empty((A.shape[0], W, A.shape[0]), dtype=A.dtype)
    out[:, W - 1, :] = np.eye(A.shape[0])
    out[:, :W - 1, :] = e("watb,ptb->awp", X, A)
    return out


def check(got, t, what=""):
    """None if `got` (oracle layout) passes the case's criterion, else a JSON-able record.  Exact cases: every entry the
    oracle's bits.  Gaussian transfers: the written level exactly the identity, every other level inside the bound."""
    name = f"{t['name']}{' ' + what if what else ''}"
    if t["bound"] is None or t["op"] == "dAC":
        return ei.compare(got, t["ref"], t["bound"], name)
    i = t["ident"]
    if not np.array_equal(got[:, i, :], np.eye(t["n_out"])):
        return {"case": name, "identity_level_not_exact": float(np.abs(got[:, i, :] - np.eye(t["n_out"])).max())}
    keep = [k for k in range(got.shape[1]) if k != i]
    return ei.compare(got[:, keep, :], t["ref"][:, keep, :], t["bound"][:, keep, :], name)


def bound_ratio(got, t):
    """max |got - ref| / bound over the entries the bound covers (Gaussian cases)"""
    keep = slice(None) if t["op"] == "dAC" else [k for k in range(got.shape[1]) if k != t["ident"]]
    g, r, b = (got, t["ref"], t["bound"]) if t["op"] == "dAC" else (got[:, keep, :], t["ref"][:, keep, :], t["bound"][:, keep, :])
    err = np.abs(g.astype(r.dtype) - r)
    return float((err[b > 0] / b[b > 0]).max())


# ------------------------------------------------------------------------------------------------------------------
# the runner: the same code on the device backend and on the host stand-in (tests/cpu_backend.py)
# ------------------------------------------------------------------------------------------------------------------
def make_slice(be, t):
    s = t["s"]
    return be.mposlice(s.odim, s.d, s.chil, s.chir, dict(s.Os), cplx=t["cplx"])


def run_hac(be, t, H=None, flag=True, axpby=None):
    """Prepare H_AC on the case's environments -- flag: MPSK_HAC_CANONICAL (real) / MPSK_HAC_CANONICAL_C128 (complex) --
    and apply it once; axpby = (a1, a0): through mpsk_hac_apply_axpby.  Returns (y, info)."""
    cplx = t["cplx"]
    up, down = (be.upload_c, be.download_c) if cplx else (be.upload, be.download)
    up_env = be.upload_env_c if cplx else be.upload_env
    H = make_slice(be, t) if H is None else H
    x = up(t["x"])
    hac = be.hac_create_ex(H, up_env(t["GL"]), up_env(t["GR"]), canonical=flag and not cplx, canonical_c128=flag and cplx)
    try:
        info = hac.info()
        y = down(hac.apply(x) if axpby is None else hac.apply_axpby(axpby[0], x, axpby[1]))
    finally:
        hac.close()
    return y, info


def run_transfer(be, H, t, canonical=True):
    """one transfer of the case through slice handle H, A and Ab the same tensor; result stacked over the levels"""
    A = be.upload(t["A"])
    if t["op"] == "tl":
        out = be.transfer_left(H, be.upload_env(t["GL"]), A, A, canonical=canonical)
    else:
        out = be.transfer_right(H, be.upload_env(t["GR"]), A, A, canonical=canonical)
    return np.concatenate(be.download_env(out, t["chis"]), axis=1)


def run_transfer_sequence(be, side, family, kind="int"):
    """every shape of transfer_shapes() on ONE slice handle (the per-shape segment tables are cached on it; the first
    shape comes back at the end): list of (case, result)"""
    shapes = transfer_shapes(family, side)
    cases = [transfer_case(side, family, *shp, kind) for shp in shapes]
    H = make_slice(be, cases[0])
    return [(t, run_transfer(be, H, t)) for t in cases]

