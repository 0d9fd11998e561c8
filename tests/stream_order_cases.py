"""The cases of tests/test_gpu_stream_order.py: per ABI family the smallest shape that reaches the route named, with a
TRUE and a DECOY operand set (same shapes, another seed of the same exact family) so that a read ahead of the producer gives
a different, exactly representable result (tests/stream_order.py).

A case is host data only, so tests/test_stream_order_cases_cpu.py can check without a GPU that both operand sets pass the
exactness guard of the input module they come from and that replacing ANY single operand by its decoy changes the
reference result.  Operands and outputs are flat fp64 arrays in the device layout (column-major; environments as slabs;
complex tensors interleaved).  `run(be, dev, obj)` issues the entry point(s) on backend `be` with the buffers `dev[name]`
and whatever `setup(be)` made (slice handles, prepared operators: built from host data or from operands that are NOT
staged); `reference(ops)` is plain numpy on the same flat arrays -- exact for the integer / dyadic families, so the GPU
comparison is np.array_equal; the factorization cases carry a `check` built from the bounds of tests/exact_factor_inputs.py
(and, for mpsk_complement_tsvd, from the contract of include/mpsk.h) instead."""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np

import exact_canonical_inputs as ci
import exact_factor_inputs as fi
import exact_inputs as ei
import exact_vector_inputs as vi


@dataclass
class Case:
    name: str
    family: str
    operands: dict                    # name -> (true, decoy), flat fp64
    outputs: dict                     # name -> doubles; a name that is also an operand is updated in place
    run: object                       # run(be, dev, obj) -> {host result name: value} or None
    reference: object                 # reference({name: flat}) -> {output name | "ret:" + host name: array}
    guard: object                     # guard({name: flat}): the exactness guard of the input module, asserting
    sync: object = False              # the entry synchronises (host scalars, tsvd, tsplit, complement_tsvd, qr_commit, a
                                      # CholeskyQR3 that is not deferred); None: the header does not say
    setup: object = None              # setup(be) -> obj
    check: object = None              # check(got) -> [failures]; None: np.array_equal with reference(true operands)
    private: str = ""                 # the private stream(s) of the ctx the entry reaches
    extra: dict = field(default_factory=dict)

    def true(self):
        return {k: v[0] for k, v in self.operands.items()}

    def decoy(self):
        return {k: v[1] for k, v in self.operands.items()}


def F(a):
    """logical-order ndarray -> flat device layout (column-major; complex: interleaved)"""
    a = np.asarray(a)
    if np.iscomplexobj(a):
        return np.ravel(a.astype(np.complex128), order="F").view(np.float64).copy()
    return np.ravel(a.astype(np.float64), order="F").copy()


def Uf(flat, shape, cplx=False):
    flat = np.asarray(flat, dtype=np.float64)
    return (flat.view(np.complex128) if cplx else flat).reshape(shape, order="F")


def ENV(G):
    """stacked environment [Db, W, Dk] -> W column-major slabs"""
    return F(np.transpose(np.asarray(G), (0, 2, 1)))


def UENV(flat, Db, W, Dk, cplx=False):
    return np.transpose(Uf(flat, (Db, Dk, W), cplx), (0, 2, 1))


@contextlib.contextmanager
def env_setting(**kv):
    """environment settings the library reads per call, for the duration of one call"""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _ints(name, *shape, cplx=False):
    return ei.int_array(ei._rng("stream-order-" + name), *shape, cplx=cplx)


def _pair(name, *shape, cplx=False):
    return _ints(name + "-true", *shape, cplx=cplx), _ints(name + "-decoy", *shape, cplx=cplx)


def _lib_ok(be, rc, what):
    from mpskit_jl_amd._lib import check
    check(rc, what)


CASES = []


def _add(case):
    assert case.name not in [c.name for c in CASES], case.name
    CASES.append(case)
    return case


# ----------------------------------------------------------------------------------------------------------------------
# GEMM core
# ----------------------------------------------------------------------------------------------------------------------
def _gemm_case(name, M, N, K, tA, tB):
    ar, ac = (K, M) if tA else (M, K)
    br, bc = (N, K) if tB else (K, N)
    A, B, Cm = _pair(name + "A", ar, ac), _pair(name + "B", br, bc), _pair(name + "C", M, N)

    def run(be, dev, obj):
        be.gemm_raw(tA, tB, M, N, K, ei.ALPHA, dev["A"].ptr, ar, dev["B"].ptr, br, ei.BETA, dev["C"].ptr, M)

    def reference(o):
        a, b = Uf(o["A"], (ar, ac)), Uf(o["B"], (br, bc))
        return {"C": F(ei.ALPHA * ((a.T if tA else a) @ (b.T if tB else b)) + ei.BETA * Uf(o["C"], (M, N)))}

    def guard(o):
        ei.assert_exact_range([o["A"], o["B"], [ei.ALPHA]], [K], name)
        ei.assert_exact_range([o["C"], [ei.BETA]], [], name)

    return _add(Case(name, "gemm", {"A": (F(A[0]), F(A[1])), "B": (F(B[0]), F(B[1])), "C": (F(Cm[0]), F(Cm[1]))},
                     {"C": M * N}, run, reference, guard))


_gemm_case("gemm-NN-128x128x64", 128, 128, 64, 0, 0)                       # one aligned tile
_gemm_case("gemm-TN-splitk-193x131x1109", *ei.SPLITK_RAGGED, 1, 0)         # partials + fixup, workspace keyed by stream


def _gemm_pair_case():
    M, N, K = 65, 33, 40
    P, Q, B, cf = _pair("gpP", M, K), _pair("gpQ", M, K), _pair("gpB", K, N), _pair("gpcoef", K, 4)

    def run(be, dev, obj):
        be.gemm_pair_raw(M, N, K, dev["P"].ptr, M, dev["Q"].ptr, M, dev["B"].ptr, K, dev["coef"].ptr, K, 0.0, dev["out1"].ptr, M,
                         0.0, dev["out2"].ptr, M)

    def reference(o):
        p, q, b, c = Uf(o["P"], (M, K)), Uf(o["Q"], (M, K)), Uf(o["B"], (K, N)), Uf(o["coef"], (K, 4))
        return {"out1": F((p * c[:, 0] + q * c[:, 1]) @ b), "out2": F((p * c[:, 2] + q * c[:, 3]) @ b)}

    def guard(o):
        ei.assert_exact_range([o["P"], o["coef"], o["B"], [2.0]], [K], "gemm_pair")
        ei.assert_exact_range([o["Q"], o["coef"], o["B"], [2.0]], [K], "gemm_pair")

    _add(Case("gemm_pair-65x33x40", "gemm", {"P": (F(P[0]), F(P[1])), "Q": (F(Q[0]), F(Q[1])), "B": (F(B[0]), F(B[1])),
                                           "coef": (F(cf[0]), F(cf[1]))}, {"out1": M * N, "out2": M * N}, run, reference, guard))


_gemm_pair_case()


def _copy_embed_case():
    rows, cols, ldd = 70, 33, 75
    m, n = 35, 9                                                       # complex m x n: 2m x n doubles, embedding 2m x 2n
    src, h = _pair("copy2d", rows, cols), _pair("cxh", 2 * m, n)

    def run(be, dev, obj):
        be.copy2d(rows, cols, dev["src"].ptr, rows, dev["dst"].ptr, ldd)
        be.cx_embed_raw(m, n, dev["h"].ptr, 2 * m, dev["E"].ptr, 2 * m)
        be.cx_half_raw(m, n, dev["E"].ptr, 2 * m, dev["h2"].ptr, 2 * m)

    def reference(o):
        from stream_order import SENTINEL
        dst = np.full((ldd, cols), SENTINEL)
        dst[:rows] = Uf(o["src"], (rows, cols))
        hh = Uf(o["h"], (2 * m, n))
        E = np.empty((2 * m, 2 * n))
        E[:, 0::2] = hh
        E[0::2, 1::2], E[1::2, 1::2] = -hh[1::2], hh[0::2]             # J h: (re, im) -> (-im, re)
        return {"dst": F(dst), "E": F(E), "h2": F(hh)}

    def guard(o):
        ei.assert_exact_range([o["src"]], [], "copy2d")
        ei.assert_exact_range([o["h"]], [], "cx_embed")

    _add(Case("copy2d+cx_embed+cx_half", "gemm", {"src": (F(src[0]), F(src[1])), "h": (F(h[0]), F(h[1]))},
              {"dst": ldd * cols, "E": 4 * m * n, "h2": 2 * m * n}, run, reference, guard))


_copy_embed_case()


# ----------------------------------------------------------------------------------------------------------------------
# operators (tests/exact_inputs.py: RAGGED = the smallest multi-tile shape; tests/exact_canonical_inputs.py for mode 3)
# ----------------------------------------------------------------------------------------------------------------------
def _decoy_like(name, a):
    a = np.asarray(a)
    return ei.int_array(ei._rng("stream-order-decoy-" + name), *a.shape, cplx=np.iscomplexobj(a))


def _slice(be, s, cplx=False):
    return be.mposlice(s.odim, s.d, s.chil, s.chir, dict(s.Os), cplx=cplx)


def _op_case(op, cplx=False, staged=("GL", "GR", "x"), via="abi", variant="", mode=None, axpby=None):
    """mpsk_dAC / mpsk_dC / mpsk_dAC2 (via "abi") or the prepared operator (via "hac": only x is staged, the environments
    belong to the prepared object) on op_case(op, RAGGED).  mode: MPSK_HAC_MODE while the operator is created -- 0 the
    three-stage slab mix, 1 the MPO folded into the right environment -- asserted through mpsk_hac_info; axpby = (a1, a0):
    through mpsk_hac_apply_axpby with dyadic scalars."""
    t = ei.op_case(op, ei.RAGGED, "int", cplx, variant)
    Dl, Dr, d, chis = ei.RAGGED
    W = sum(chis)
    xs = t["x"].shape
    name = (f"{op}{'-hac' if via == 'hac' else ''}{'-mode%d' % mode if mode is not None else ''}{'-axpby' if axpby else ''}"
            f"-{'c128' if cplx else 'f64'}-{Dl}x{Dr}")
    true = {"GL": ENV(t["G"]), "GR": ENV(t["R"]), "x": F(t["x"])}
    dec = {"GL": ENV(_decoy_like(name + "G", t["G"])), "GR": ENV(_decoy_like(name + "R", t["R"])),
           "x": F(_decoy_like(name + "x", t["x"]))}
    m = 2 if cplx else 1
    ysize = m * t["x"].size

    def setup(be):
        obj = {}
        if op != "dC":
            obj["H"] = _slice(be, t["s"], cplx)
        if op == "dAC2":
            obj["H2"] = _slice(be, t["s2"], cplx)
        if via == "hac":
            obj["GL"], obj["GR"] = be.upload(true["GL"]).reshape(W, m * Dl, Dl), be.upload(true["GR"]).reshape(W, m * Dr, Dr)
            assert mode is not None, "a prepared-operator case names its mode"
            with env_setting(MPSK_HAC_MODE=mode):
                obj["hac"] = be.hac_create(obj["H"], obj["GL"], obj["GR"])
            assert obj["hac"].info()["mode"] == mode, (mode, obj["hac"].info())
        return obj

    def run(be, dev, obj):
        x = dev["x"].reshape(*((m * xs[0],) + xs[1:]))
        y = dev["y"].reshape(*x.shape)
        if via == "hac":
            if axpby:
                obj["hac"].apply_axpby(axpby[0], x, axpby[1], out=y)
            else:
                obj["hac"].apply(x, out=y)
            return
        GL, GR = dev["GL"].reshape(W, m * Dl, Dl), dev["GR"].reshape(W, m * Dr, Dr)
        if op == "dAC":
            be.dAC(obj["H"], GL, GR, x, out=y)
        elif op == "dC":
            be.dC(GL, GR, x, out=y, cplx=cplx)
        else:
            be.dAC2(obj["H"], obj["H2"], GL, GR, x, out=y)

    def reference(o):
        u = {"O": t["O"], "G": UENV(o.get("GL", true["GL"]), Dl, W, Dl, cplx), "R": UENV(o.get("GR", true["GR"]), Dr, W, Dr, cplx),
             "x": Uf(o["x"], xs, cplx)}
        if op == "dAC2":
            u["O2"] = t["O2"]
        y = ei.contract(op, u)
        return {"y": F(axpby[1] * u["x"] + axpby[0] * y if axpby else y)}

    def guard(o):
        ops = [o.get("GL", true["GL"]), o.get("GR", true["GR"]), o["x"], t["O"]] + ([t["O2"]] if op == "dAC2" else [])
        ops += [[2.0 * max(abs(a) for a in axpby)]] if axpby else []
        ext = {"dAC": [Dl, W, d, Dr, W], "dC": [Dl, Dr, W], "dAC2": [Dl, W, d, d, Dr, W, W]}[op]
        ei.assert_exact_range(ops, ext + [2 if cplx else 1] * len(ops), name)

    keep = staged if via == "abi" else ("x",)
    return _add(Case(name, "operators", {k: (true[k], dec[k]) for k in keep}, {"y": ysize}, run, reference, guard, setup=setup))


_op_case("dAC")
_op_case("dAC", via="hac", mode=0)                                          # the three-stage operator
_op_case("dAC", via="hac", mode=1)                                          # the MPO folded into the right environment
_op_case("dAC", via="hac", mode=0, axpby=(0.5, -2.0))
_op_case("dC")
_op_case("dAC2")
_op_case("dAC", cplx=True)


def _hac3_case():
    """mpsk_hac_apply_axpby on the Jordan-form operator of canonical environments (mode 3), dyadic a1 / a0"""
    t = ci.hac_case("full", 65, 65)
    a1, a0 = 0.5, -2.0
    xd = _decoy_like("hac3x", t["x"])

    def setup(be):
        H = ci.make_slice(be, t)
        GL, GR = be.upload_env(t["GL"]), be.upload_env(t["GR"])
        hac = be.hac_create_ex(H, GL, GR, canonical=True)
        assert hac.info()["mode"] == 3, hac.info()
        return {"H": H, "GL": GL, "GR": GR, "hac": hac}

    def run(be, dev, obj):
        obj["hac"].apply_axpby(a1, dev["x"].reshape(*t["x"].shape), a0, out=dev["y"].reshape(*t["x"].shape))

    def reference(o):
        x = Uf(o["x"], t["x"].shape)
        return {"y": F(a0 * x + a1 * ei.contract("dAC", {"O": t["O"], "G": t["G"], "R": t["R"], "x": x}))}

    def guard(o):
        ei.assert_exact_range([t["G"], t["R"], o["x"], t["O"], [2.0]], [65, 5, 2, 65, 5], "hac3")

    _add(Case("hac_apply_axpby-mode3-65x65", "operators", {"x": (F(t["x"]), F(xd))}, {"y": t["x"].size}, run, reference, guard,
              setup=setup))


_hac3_case()


def _hsum_case(route):
    """mpsk_hsum_apply: route 1 = two canonical terms folded into one mode-3 operator, route 2 = two general terms accumulated"""
    coefs = (0.5, -2.0)
    if route == 1:
        ts = [ci.hac_case("full", 65, 65), ci.hac_case("chi", 65, 65)]
    else:
        ts = [ei.op_case("dAC", ei.RAGGED, "int", False, ""), ei.op_case("dAC", ei.RAGGED, "int", False, "second-term")]
    xs = ts[0]["x"].shape
    xd = _decoy_like(f"hsum{route}x", ts[0]["x"])

    def setup(be):
        Hs = [_slice(be, t["s"]) for t in ts]
        GLs, GRs = [be.upload_env(t["GL"]) for t in ts], [be.upload_env(t["GR"]) for t in ts]
        h = be.hsum_create(Hs, GLs, GRs, canonical=route == 1)
        assert h.info()["route"] == route, h.info()
        h.set_coefs(coefs)
        return {"keep": (Hs, GLs, GRs), "h": h}

    def run(be, dev, obj):
        obj["h"].apply(dev["x"].reshape(*xs), out=dev["y"].reshape(*xs))

    def reference(o):
        x = Uf(o["x"], xs)
        return {"y": F(sum(c * ei.contract("dAC", {"O": t["O"], "G": t["G"], "R": t["R"], "x": x}) for c, t in zip(coefs, ts)))}

    def guard(o):
        for t in ts:
            W = t["O"].shape[0]
            ei.assert_exact_range([t["G"], t["R"], o["x"], t["O"], [4.0]], [xs[0], W, xs[1], xs[2], W], f"hsum{route}")

    _add(Case(f"hsum_apply-route{route}", "operators", {"x": (F(ts[0]["x"]), F(xd))}, {"y": ts[0]["x"].size}, run, reference,
              guard, setup=setup))


_hsum_case(1)
_hsum_case(2)


# ----------------------------------------------------------------------------------------------------------------------
# transfers and the site kernels
# ----------------------------------------------------------------------------------------------------------------------
def _transfer_case(side):
    """mpsk_transfer_left / mpsk_transfer_right through a sparse slice on op_case(RAGGED)"""
    op = "tl" if side == "l" else "tr"
    t = ei.op_case(op, ei.RAGGED, "int", False, "")
    Dl, Dr, d, chis = ei.RAGGED
    W = sum(chis)
    Dk = Dl if side == "l" else Dr
    ek = "G" if side == "l" else "R"
    name = f"transfer_{'left' if side == 'l' else 'right'}-mpo-{Dl}x{Dr}"
    ops = {"V": (ENV(t[ek]), ENV(_decoy_like(name + "V", t[ek]))), "A": (F(t["A"]), F(_decoy_like(name + "A", t["A"]))),
           "Ab": (F(t["Ab"]), F(_decoy_like(name + "Ab", t["Ab"])))}
    Do = Dr if side == "l" else Dl

    def run(be, dev, obj):
        A, Ab, V = dev["A"].reshape(Dl, d, Dr), dev["Ab"].reshape(Dl, d, Dr), dev["V"].reshape(W, Dk, Dk)
        (be.transfer_left if side == "l" else be.transfer_right)(obj, V, A, Ab, out=dev["out"].reshape(W, Do, Do))

    def reference(o):
        u = {"O": t["O"], ek: UENV(o["V"], Dk, W, Dk), "A": Uf(o["A"], (Dl, d, Dr)), "Ab": Uf(o["Ab"], (Dl, d, Dr))}
        return {"out": ENV(ei.contract(op, u))}

    def guard(o):
        ei.assert_exact_range([o["V"], o["A"], o["Ab"], t["O"]], [Dk, W, d, Dk, d], name)

    _add(Case(name, "transfers", ops, {"out": W * Do * Do}, run, reference, guard, setup=lambda be: _slice(be, t["s"])))


_transfer_case("l")
_transfer_case("r")


def _passthrough_case():
    """mpsk_transfer_left and mpsk_transfer_right with H == NULL: W independent slabs"""
    W, d, Dl, Dr, Dlb, Drb = 3, 2, 33, 65, 20, 48
    V, A, Ab = _pair("ptV", Dr, W, Drb), _pair("ptA", Dl, d, Dr), _pair("ptAb", Dlb, d, Drb)
    Vl = _pair("ptVl", Dlb, W, Dl)

    def run_l(be, dev, obj):
        be.transfer_left(None, dev["V"].reshape(W, Dlb, Dl), dev["A"].reshape(Dl, d, Dr), dev["Ab"].reshape(Dlb, d, Drb),
                         out=dev["out"].reshape(W, Drb, Dr))

    def ref_l(o):
        v, a, ab = UENV(o["V"], Dlb, W, Dl), Uf(o["A"], (Dl, d, Dr)), Uf(o["Ab"], (Dlb, d, Drb))
        return {"out": ENV(np.einsum("pwa,asb,psq->qwb", v, a, ab, optimize=False))}

    _add(Case("transfer_left-passthrough-33x65", "transfers", {"V": (ENV(Vl[0]), ENV(Vl[1])), "A": (F(A[0]), F(A[1])),
                                                              "Ab": (F(Ab[0]), F(Ab[1]))}, {"out": W * Drb * Dr}, run_l, ref_l,
              lambda o: ei.assert_exact_range([o["V"], o["A"], o["Ab"]], [Dl, Dlb, d], "passthrough left")))

    def run(be, dev, obj):
        be.transfer_right(None, dev["V"].reshape(W, Dr, Drb), dev["A"].reshape(Dl, d, Dr), dev["Ab"].reshape(Dlb, d, Drb),
                          out=dev["out"].reshape(W, Dl, Dlb))

    def reference(o):
        v, a, ab = UENV(o["V"], Dr, W, Drb), Uf(o["A"], (Dl, d, Dr)), Uf(o["Ab"], (Dlb, d, Drb))
        return {"out": ENV(np.einsum("asb,bwq,psq->awp", a, v, ab, optimize=False))}

    _add(Case("transfer_right-passthrough-33x65", "transfers", {"V": (ENV(V[0]), ENV(V[1])), "A": (F(A[0]), F(A[1])),
                                                               "Ab": (F(Ab[0]), F(Ab[1]))}, {"out": W * Dl * Dlb}, run, reference,
              lambda o: ei.assert_exact_range([o["V"], o["A"], o["Ab"]], [Dr, Drb, d], "passthrough")))


_passthrough_case()


def _canonical_transfer_case(mode, side="l"):
    """mpsk_transfer_left_ex / mpsk_transfer_right_ex under MPSK_TRANSFER_CANONICAL: mode 1 the level-by-level route, mode 2
    the pair-Gram route (64 x 2 x 64).  A and Ab are ONE buffer; the decoy isometry is A with the indices of its contracted
    side reversed (still an isometry, another Gram pattern)."""
    D, d = 64, 2
    left = side == "l"
    t = ci.transfer_case(side, "full", D, d, D)
    W = sum(t["chis"])
    Gd = ci.env(ei._rng("stream-order-decoy-canon-G" + side), ei.int_array, D, t["chis"], t["ident"])
    Ad = np.ascontiguousarray(t["A"][::-1, ::-1, :] if left else t["A"][:, ::-1, ::-1])
    name = f"transfer_{'left' if left else 'right'}_ex-canonical-mode{mode}-64x2x64"
    op, ek = ("tl", "G") if left else ("tr", "R")

    def run(be, dev, obj):
        A = dev["A"].reshape(D, d, D)
        n0 = be.transfer_stats()["pair"]
        with env_setting(MPSK_TRANSFER_MODE=mode):
            (be.transfer_left if left else be.transfer_right)(obj, dev["V"].reshape(W, D, D), A, A, out=dev["out"].reshape(W, D, D),
                                                              canonical=True)
        assert be.transfer_stats()["pair"] - n0 == (1 if mode == 2 else 0), "route"

    def reference(o):
        a = Uf(o["A"], (D, d, D))
        return {"out": ENV(ei.contract(op, {"O": t["O"], ek: UENV(o["V"], D, W, D), "A": a, "Ab": a}))}

    def guard(o):
        a = Uf(o["A"], (D, d, D))
        u = ci.dyadic_unit(a)
        assert np.array_equal(np.einsum("ptq,ptb->qb" if left else "atb,ptb->ap", a, a), np.eye(D)), "not an isometry on that side"
        assert ei.magnitude([o["V"], a, a, t["O"]], [D, W, d, D, d]) / (u * u) < ei.LIMIT, name

    _add(Case(name, "transfers", {"V": (ENV(t[ek]), ENV(ei._stack(Gd))), "A": (F(t["A"]), F(Ad))}, {"out": W * D * D}, run,
              reference, guard, setup=lambda be: ci.make_slice(be, t)))


_canonical_transfer_case(1)
_canonical_transfer_case(2)
_canonical_transfer_case(1, "r")
_canonical_transfer_case(2, "r")


def _pair_transfer_case():
    """mpsk_transfer_left_pair: two kets and environments through one slice and one bra"""
    t = ei.op_case("tl", ei.RAGGED, "int", False, "")
    d, chis = ei.RAGGED[2], ei.RAGGED[3]
    W = sum(chis)
    Dl1, Dl2, Dr, Dlb, Drb = 33, 20, 65, 17, 48
    shp = {"V1": (Dlb, W, Dl1), "A1": (Dl1, d, Dr), "V2": (Dlb, W, Dl2), "A2": (Dl2, d, Dr), "Ab": (Dlb, d, Drb)}
    lay = lambda k, a: ENV(a) if k[0] == "V" else F(a)
    ops = {k: tuple(lay(k, a) for a in _pair("tlp" + k, *s)) for k, s in shp.items()}

    def run(be, dev, obj):
        r = lambda k: dev[k].reshape(*((W, shp[k][0], shp[k][2]) if k[0] == "V" else shp[k]))
        be.transfer_left_pair(obj, r("V1"), r("A1"), r("V2"), r("A2"), r("Ab"), out=dev["out"].reshape(W, Drb, Dr))

    def reference(o):
        u = {k: (UENV(o[k], s[0], W, s[2]) if k[0] == "V" else Uf(o[k], s)) for k, s in shp.items()}
        c = lambda V, A: ei.contract("tl", {"O": t["O"], "G": V, "A": A, "Ab": u["Ab"]})
        return {"out": ENV(c(u["V1"], u["A1"]) + c(u["V2"], u["A2"]))}

    def guard(o):
        ei.assert_exact_range([o["V1"], o["A1"], o["Ab"], t["O"], [2.0]], [Dl1, W, d, Dlb, d], "tl_pair")
        ei.assert_exact_range([o["V2"], o["A2"], o["Ab"], t["O"], [2.0]], [Dl2, W, d, Dlb, d], "tl_pair")

    _add(Case("transfer_left_pair-33+20x65", "transfers", ops, {"out": W * Drb * Dr}, run, reference, guard,
              setup=lambda be: _slice(be, t["s"])))


_pair_transfer_case()


def _gram_cases():
    d, Dl, Dr, Dlb, Drb = 2, 33, 65, 20, 65
    shp = {"Lin": (Dlb, Dl), "A": (Dl, d, Dr), "Ab": (Dlb, d, Drb), "R": (Dr, Drb)}
    ops = {k: tuple(F(a) for a in _pair("tlge" + k, *s)) for k, s in shp.items()}

    def run(be, dev, obj):
        r = lambda k: dev[k].reshape(*shp[k])
        be.transfer_left_gram_env(r("Lin"), r("A"), r("Ab"), r("R"), dev["gram"].reshape(d, d), out=dev["Lout"].reshape(1, Drb, Dr))

    def reference(o):
        u = {k: Uf(o[k], s) for k, s in shp.items()}
        T1 = np.einsum("pa,asb->psb", u["Lin"], u["A"], optimize=False)
        return {"Lout": F(np.einsum("psq,psb->qb", u["Ab"], T1, optimize=False)),
                "gram": F(np.einsum("ptq,psq->ts", u["Ab"], np.einsum("psb,bq->psq", T1, u["R"], optimize=False), optimize=False))}

    _add(Case("transfer_left_gram_env-33x65", "transfers", ops, {"Lout": Drb * Dr, "gram": d * d}, run, reference,
              lambda o: ei.assert_exact_range([o["Lin"], o["A"], o["Ab"], o["R"]], [Dl, Dr, Dlb, Drb], "gram_env")))
    W = 3
    X, Ab = _pair("sgX", Dl, d, Dr, W), _pair("sgAb", Dl, d, Dr)

    def run_sg(be, dev, obj):
        be.site_gram(dev["X"].reshape(W, Dl, d, Dr), dev["Ab"].reshape(Dl, d, Dr), out=dev["g"].reshape(W, d, d))

    def ref_sg(o):
        return {"g": F(np.einsum("ptb,psbw->tsw", Uf(o["Ab"], (Dl, d, Dr)), Uf(o["X"], (Dl, d, Dr, W)), optimize=False))}

    _add(Case("site_gram-3x33x2x65", "transfers", {"X": (F(X[0]), F(X[1])), "Ab": (F(Ab[0]), F(Ab[1]))}, {"g": W * d * d}, run_sg,
              ref_sg, lambda o: ei.assert_exact_range([o["X"], o["Ab"]], [Dl, Dr], "site_gram")))


_gram_cases()


def _regularize_dsum_cases():
    W, D1, D2 = 3, 33, 65
    v, lv, rv = _pair("regv", D1, W, D2), _pair("regl", D2, D1), _pair("regr", D1, D2)

    def run(be, dev, obj):
        be.regularize(dev["v"].reshape(W, D1, D2), dev["lvec"].reshape(D2, D1), dev["rvec"].reshape(D1, D2))

    def reference(o):
        vv, l, r = UENV(o["v"], D1, W, D2), Uf(o["lvec"], (D2, D1)), Uf(o["rvec"], (D1, D2))
        return {"v": ENV(vv - np.einsum("w,pq->pwq", np.einsum("xy,ywx->w", l, vv), r))}

    _add(Case("regularize-3x33x65", "transfers", {"v": (ENV(v[0]), ENV(v[1])), "lvec": (F(lv[0]), F(lv[1])), "rvec": (F(rv[0]), F(rv[1]))},
              {"v": W * D1 * D2}, run, reference,
              lambda o: ei.assert_exact_range([o["lvec"], o["v"], o["rvec"]], [D1, D2], "regularize")))
    d, Dn, E1, E2 = 2, 33, 20, 17
    Da, Db = 13, 24
    G, A1, A2 = _pair("dsG", Dn, Da + Db), _pair("dsA1", Da, d, E1), _pair("dsA2", Db, d, E2)

    def run_ds(be, dev, obj):
        be.dsum_site("left", dev["G"].reshape(Dn, Da + Db), dev["A1"].reshape(Da, d, E1), dev["A2"].reshape(Db, d, E2),
                     out=dev["out"].reshape(Dn, d, E1 + E2))

    def ref_ds(o):
        g, a1, a2 = Uf(o["G"], (Dn, Da + Db)), Uf(o["A1"], (Da, d, E1)), Uf(o["A2"], (Db, d, E2))
        out = np.empty((Dn, d, E1 + E2))
        out[:, :, :E1] = np.einsum("na,ase->nse", g[:, :Da], a1)
        out[:, :, E1:] = np.einsum("na,ase->nse", g[:, Da:], a2)
        return {"out": F(out)}

    def guard_ds(o):
        ei.assert_exact_range([o["G"], o["A1"]], [Da], "dsum left")
        ei.assert_exact_range([o["G"], o["A2"]], [Db], "dsum left")

    _add(Case("dsum_site-left-33x(13+24)", "transfers", {"G": (F(G[0]), F(G[1])), "A1": (F(A1[0]), F(A1[1])), "A2": (F(A2[0]), F(A2[1]))},
              {"out": Dn * d * (E1 + E2)}, run_ds, ref_ds, guard_ds))
    Gr = _pair("dsGr", E1 + E2, Dn)

    def run_dsr(be, dev, obj):
        be.dsum_site("right", dev["G"].reshape(E1 + E2, Dn), dev["A1"].reshape(Da, d, E1), dev["A2"].reshape(Db, d, E2),
                     out=dev["out"].reshape(Da + Db, d, Dn))

    def ref_dsr(o):
        g, a1, a2 = Uf(o["G"], (E1 + E2, Dn)), Uf(o["A1"], (Da, d, E1)), Uf(o["A2"], (Db, d, E2))
        out = np.empty((Da + Db, d, Dn))
        out[:Da] = np.einsum("ase,en->asn", a1, g[:E1])
        out[Da:] = np.einsum("ase,en->asn", a2, g[E1:])
        return {"out": F(out)}

    def guard_dsr(o):
        ei.assert_exact_range([o["G"], o["A1"]], [E1], "dsum right")
        ei.assert_exact_range([o["G"], o["A2"]], [E2], "dsum right")

    _add(Case("dsum_site-right-(13+24)x33", "transfers", {"G": (F(Gr[0]), F(Gr[1])), "A1": (F(A1[0]), F(A1[1])), "A2": (F(A2[0]), F(A2[1]))},
              {"out": (Da + Db) * d * Dn}, run_dsr, ref_dsr, guard_dsr))


_regularize_dsum_cases()


# ----------------------------------------------------------------------------------------------------------------------
# factorizations: the entries that fork to the ctx's private streams
# ----------------------------------------------------------------------------------------------------------------------
def _factor_guard(*built):
    """The matrices of tests/exact_factor_inputs.py pass their exactness guard inside the builders (magnitude below 2^50,
    fp64 product == longdouble product).  An operand here is such a matrix, or one with its rows and columns shuffled --
    the family's own last construction step, which moves no entry off the grid: the guard checks finiteness, the 2^50
    limit and that the operand holds exactly the entries of a matrix a builder returned."""
    keys = [np.sort(np.abs(F(a))) for a in built]

    def guard(o):
        for name, a in o.items():
            assert np.all(np.isfinite(a)) and np.abs(a).max() < fi.LIMIT, name
            k = np.sort(np.abs(a))
            assert any(k.shape == b.shape and np.array_equal(k, b) for b in keys), f"{name}: not a matrix of the builders"
    return guard


def _shuffled(A, name):
    """another member of A's family: the same exact matrix behind other row and column permutations"""
    rng = fi._rng("stream-order-decoy-" + name)
    return np.ascontiguousarray(A[rng.permutation(A.shape[0])][:, rng.permutation(A.shape[1])])


def _svd_reference(m, n, cplx=False):
    """what a full SVD determines: the singular values and the product U diag(S) Vh (the matrix itself)"""
    def reference(o):
        A = Uf(o["A"], (m, n), cplx)
        return {"S": np.linalg.svd(A, compute_uv=False), "USVh": F(A)}
    return reference


def _qr_mats(m, n):
    """four members of one QR family at one shape: (matrix, check(Q, R, what)) -- 8 x 4 from the tall (Householder) family,
    larger shapes from qr_matrix (CholeskyQR3)"""
    out = []
    for g in (3, 4, 5, 6):
        if n <= 64:
            hc = fi.HouseCase(m, n, g)
            out.append((hc.matrix()[0], lambda Q, R, what, hc=hc: fi.check_house_factors(hc, Q, R, what)))
        else:
            qc = fi.QrCase(m, n, g)
            out.append((fi.qr_matrix(m, n, g)[0], lambda Q, R, what, qc=qc: fi.check_qr_factors(qc, Q, R, what)))
    return out


def _qr_sync(n):
    """CholeskyQR3 (n > 64) reads the device's success flag before a call that is not deferred returns: it synchronises.
    The header leaves the Householder route (n <= 64) open: None accepts either, and run_delayed then demands that a call
    which outlasted the producer really waited for it."""
    return True if n > 64 else None


def _qr_ref(a):
    Q, R = fi.lapack_qrpos(a)
    return Q, R


def _qr_single_cases(m, n):
    (A, chk), _, (Ad, _), _ = _qr_mats(m, n)
    _no_guard = _factor_guard(A, Ad, A.T, Ad.T)

    def run(be, dev, obj):
        _lib_ok(be, be.lib.mpsk_qrpos(be.ctx, m, n, dev["A"].ptr, m, dev["Q"].ptr, m, dev["R"].ptr, n), "mpsk_qrpos")

    def reference(o):
        Q, R = _qr_ref(Uf(o["A"], (m, n)))
        return {"Q": F(Q), "R": F(R)}

    _add(Case(f"qrpos-{m}x{n}", "factorizations", {"A": (F(A), F(Ad))}, {"Q": m * n, "R": n * n}, run, reference, _no_guard,
              sync=_qr_sync(n), check=lambda got: chk(Uf(got["Q"], (m, n)), Uf(got["R"], (n, n)), "qrpos")))
    At, Adt = np.ascontiguousarray(A.T), np.ascontiguousarray(Ad.T)

    def run_lq(be, dev, obj):
        _lib_ok(be, be.lib.mpsk_lqpos(be.ctx, n, m, dev["A"].ptr, n, dev["L"].ptr, n, dev["Q"].ptr, n), "mpsk_lqpos")

    def ref_lq(o):
        Q, R = _qr_ref(Uf(o["A"], (n, m)).T)
        return {"L": F(R.T), "Q": F(Q.T)}

    _add(Case(f"lqpos-{n}x{m}", "factorizations", {"A": (F(At), F(Adt))}, {"L": n * n, "Q": n * m}, run_lq, ref_lq, _no_guard,
              sync=_qr_sync(n), check=lambda got: chk(Uf(got["Q"], (n, m)).T.copy(), Uf(got["L"], (n, n)).T.copy(), "lqpos")))


_qr_single_cases(768, 256)


def _qr_pair_cases(m, n, kinds):
    (A1, c1), (A2, c2), (D1, _), (D2, _) = _qr_mats(m, n)
    A2t, D2t = np.ascontiguousarray(A2.T), np.ascontiguousarray(D2.T)
    _no_guard = _factor_guard(A1, A2, D1, D2)
    big = n > 64
    outs2 = {"Q1": m * n, "R1": n * n, "Q2": m * n, "R2": n * n}

    def qrpos2(be, dev):
        _lib_ok(be, be.lib.mpsk_qrpos2(be.ctx, m, n, dev["A1"].ptr, m, dev["Q1"].ptr, m, dev["R1"].ptr, n, dev["A2"].ptr, m,
                                      dev["Q2"].ptr, m, dev["R2"].ptr, n), "mpsk_qrpos2")

    def ref2(o):
        (Q1, R1), (Q2, R2) = _qr_ref(Uf(o["A1"], (m, n))), _qr_ref(Uf(o["A2"], (m, n)))
        return {"Q1": F(Q1), "R1": F(R1), "Q2": F(Q2), "R2": F(R2)}

    def chk2(got):
        return (c1(Uf(got["Q1"], (m, n)), Uf(got["R1"], (n, n)), "qrpos2 first")
                + c2(Uf(got["Q2"], (m, n)), Uf(got["R2"], (n, n)), "qrpos2 second"))

    ops2 = {"A1": (F(A1), F(D1)), "A2": (F(A2), F(D2))}
    if "qrpos2" in kinds:
        _add(Case(f"qrpos2-{m}x{n}", "factorizations", ops2, outs2, lambda be, dev, obj: qrpos2(be, dev), ref2, _no_guard, sync=_qr_sync(n),
                  check=chk2,
                  private="stream2 (fork / join)" if big else "none: the sequential branch"))
    if "defer" in kinds:
        def run_defer(be, dev, obj):
            be.qr_defer()
            qrpos2(be, dev)
            return {"redone": be.qr_commit()}

        def chk_defer(got):
            return chk2(got) + ([] if int(got["ret:redone"]) == 0 else [f"qr_commit redone = {got['ret:redone']} on a well-conditioned pair"])

        _add(Case(f"qr_defer+qrpos2+qr_commit-{m}x{n}", "factorizations", ops2, outs2, run_defer,
                  lambda o: dict(ref2(o), **{"ret:redone": np.asarray(0)}), _no_guard, sync=True, check=chk_defer,
                  private="stream2; the commit reads the device flag"))
    if "qrlq" in kinds:
        def run_qrlq(be, dev, obj):
            _lib_ok(be, be.lib.mpsk_qrlq_pair(be.ctx, m, n, dev["A1"].ptr, m, dev["Q1"].ptr, m, dev["R1"].ptr, n, dev["A2"].ptr, n,
                                             dev["L2"].ptr, n, dev["Q2"].ptr, n), "mpsk_qrlq_pair")

        def ref_qrlq(o):
            (Q1, R1), (Q2, R2) = _qr_ref(Uf(o["A1"], (m, n))), _qr_ref(Uf(o["A2"], (n, m)).T)
            return {"Q1": F(Q1), "R1": F(R1), "L2": F(R2.T), "Q2": F(Q2.T)}

        def chk_qrlq(got):
            return (c1(Uf(got["Q1"], (m, n)), Uf(got["R1"], (n, n)), "qrlq_pair qr")
                    + c2(Uf(got["Q2"], (n, m)).T.copy(), Uf(got["L2"], (n, n)).T.copy(), "qrlq_pair lq"))

        _add(Case(f"qrlq_pair-{m}x{n}", "factorizations", {"A1": (F(A1), F(D1)), "A2": (F(A2t), F(D2t))},
                  {"Q1": m * n, "R1": n * n, "L2": n * n, "Q2": n * m}, run_qrlq, ref_qrlq, _no_guard, sync=_qr_sync(n), check=chk_qrlq,
                  private="stream2 (fork / join)" if big else "none: the sequential branch"))


_qr_pair_cases(8, 4, ("qrpos2", "qrlq"))
_qr_pair_cases(768, 256, ("qrpos2", "qrlq", "defer"))


def _side_case():
    """mpsk_ctx_side_mark / _begin / _end around one mpsk_gemm: the product runs on the ctx's second stream, ordered after the
    mark (which follows the producer) and joined by side_end"""
    M, N, K = 128, 128, 64
    A, B = _pair("sideA", M, K), _pair("sideB", K, N)

    def run(be, dev, obj):
        be.side_mark()
        be.side_begin()
        try:
            be.gemm_raw(0, 0, M, N, K, 1.0, dev["A"].ptr, M, dev["B"].ptr, K, 0.0, dev["C"].ptr, M)
        finally:
            be.side_end()

    _add(Case("side_section+gemm-128x128x64", "factorizations", {"A": (F(A[0]), F(A[1])), "B": (F(B[0]), F(B[1]))}, {"C": M * N}, run,
              lambda o: {"C": F(Uf(o["A"], (M, K)) @ Uf(o["B"], (K, N)))},
              lambda o: ei.assert_exact_range([o["A"], o["B"]], [K], "side"), private="stream2 (side section)"))


_side_case()


def _svd_case(sc, private):
    """mpsk_tsvd of one chained schedule of fi.chain_cases()"""
    m, n = sc.m, sc.n
    k = min(m, n)
    A = fi.svd_matrix(m, n, sc.family)[0]
    Ad = _shuffled(A, sc.name)

    def run(be, dev, obj):
        kept, disc = C.c_int(0), C.c_double(0.0)
        be.set_svd_mode(sc.mode)
        try:
            with env_setting(**sc.envd):
                _lib_ok(be, be.lib.mpsk_tsvd(be.ctx, m, n, dev["A"].ptr, m, dev["U"].ptr, m, dev["S"].ptr, dev["Vh"].ptr, k, 0, 0.0,
                                            C.byref(kept), C.byref(disc)), "mpsk_tsvd")
        finally:
            be.set_svd_mode(3)
        return {"kept": kept.value, "disc": disc.value}

    def check(got):
        bad = fi.check_svd_factors(sc, Uf(got["U"], (m, k)), got["S"], Uf(got["Vh"], (k, n)))
        if int(got["ret:kept"]) != k or float(got["ret:disc"]) != 0.0:
            bad.append(f"kept {got['ret:kept']}, disc {got['ret:disc']} without truncation")
        return bad

    _add(Case(f"tsvd-{sc.name}", "factorizations", {"A": (F(A), F(Ad))}, {"U": m * k, "S": k, "Vh": k * n}, run,
              _svd_reference(m, n), _factor_guard(A), sync=True, check=check, private=private))


def _chain(m, n, family, call, mode, chains):
    return next(c for c in fi.chain_cases() if (c.m, c.n, c.family, c.call, c.mode, c.envd[fi.CH]) == (m, n, family, call, mode, chains))


_svd_case(_chain(256, 256, "int", "tsvd", 3, "2"), "xstreams[0] = stream2 (2 chains)")
_svd_case(_chain(1024, 512, "int", "tsvd", 0, "4"), "stream2 and xstreams[1..2] (4 chains)")


def _split_case(mode):
    """mpsk_tsplit at 200 x 200: svd mode 2 (V-free iteration, 2 chains) and mode 3 with max_keep = 32 (the checked subspace
    stage in front of it)"""
    sc = _chain(200, 200, "int", "tsplit", 2, "2")
    m = n = kf = 200
    keep = 0 if mode == 2 else 32
    A, Sx, _ = fi.svd_matrix(m, n, "int")
    Ad = _shuffled(A, f"tsplit{mode}")
    bound = fi.svd_bound(sc)

    def run(be, dev, obj):
        kept, disc = C.c_int(0), C.c_double(0.0)
        be.set_svd_mode(mode)
        try:
            with env_setting(**sc.envd):
                _lib_ok(be, be.lib.mpsk_tsplit(be.ctx, m, n, dev["A"].ptr, m, keep, 0.0, dev["AL"].ptr, m, dev["C"].ptr, kf,
                                              dev["AR"].ptr, kf, dev["S"].ptr, C.byref(kept), C.byref(disc)), "mpsk_tsplit")
        finally:
            be.set_svd_mode(3)
        return {"kept": kept.value, "disc": disc.value}

    def check(got):
        k = int(got["ret:kept"])
        if k != (kf if mode == 2 else keep):
            return [f"kept {k}"]
        al, c, ar = Uf(got["AL"], (m, kf))[:, :k], Uf(got["C"], (kf, kf))[:k, :k], Uf(got["AR"], (kf, n))[:k]
        if mode == 2:
            return fi.check_split_factors(sc, al, c, ar, got["S"][:k])
        bad = []                                    # truncated: the kept values, the isometries, and the residual, which is the
        S = got["S"][:k]                            # discarded tail whatever basis a tie at the cut picks
        if not np.abs(S.astype(fi.LD) - Sx[:k]).max() <= bound:
            bad.append(f"|S - S_exact| = {float(np.abs(S - Sx[:k]).max()):.3e} > {bound:.3e}")
        eu, ev = np.abs(al.T @ al - np.eye(k)).max(), np.abs(ar @ ar.T - np.eye(k)).max()
        if not (eu < 1e-12 and ev < 1e-12):
            bad.append(f"isometry al {eu:.3e} ar {ev:.3e} >= 1e-12")
        tail = float(np.sqrt(np.sum(Sx[k:] ** 2)))
        res = float(np.linalg.norm(al @ c @ ar - A))
        if not abs(res - tail) <= np.sqrt(m * n) * bound:          # every entry within `bound`: the Frobenius norm within sqrt(m n) of it
            bad.append(f"| |al c ar - A|_F - tail | = {abs(res - tail):.3e} > {np.sqrt(m * n) * bound:.3e}")
        if not abs(float(got["ret:disc"]) - tail) <= np.sqrt(n) * bound:
            bad.append(f"disc {got['ret:disc']} against the exact tail {tail}")
        return bad

    _add(Case(f"tsplit-mode{mode}-200x200", "factorizations", {"A": (F(A), F(Ad))},
              {"AL": m * kf, "C": kf * kf, "AR": kf * n, "S": kf}, run,
              _svd_reference(m, n), _factor_guard(A), sync=True, check=check, private="stream2 (= xstreams[0])"))


_split_case(2)
_split_case(3)


def _csplit_case():
    """complex128 mpsk_tsplit (trunc_err > 0: the native complex SVD picks k) at 120 x 100"""
    m, n = 120, 100
    kf = n
    sc = fi.SvdCase(m, n, "int", "tsvd_c", 3)
    A, Sx, _ = fi.svd_matrix(m, n, "int", True)
    Ad = _shuffled(A, "tsplit-c128")
    bound = fi.svd_bound(sc)
    terr = 0.25 * float(Sx[-1])                                       # below the smallest value: nothing is discarded

    def run(be, dev, obj):
        kept, disc = C.c_int(0), C.c_double(0.0)
        be._set_dtype(True)
        try:
            _lib_ok(be, be.lib.mpsk_tsplit(be.ctx, m, n, dev["A"].ptr, m, 0, terr, dev["AL"].ptr, m, dev["C"].ptr, kf, dev["AR"].ptr,
                                          kf, dev["S"].ptr, C.byref(kept), C.byref(disc)), "mpsk_tsplit (C128)")
        finally:
            be._set_dtype(False)
        return {"kept": kept.value, "disc": disc.value}

    def check(got):
        if int(got["ret:kept"]) != kf:
            return [f"kept {got['ret:kept']}"]
        al, c, ar = Uf(got["AL"], (m, kf), True), Uf(got["C"], (kf, kf), True), Uf(got["AR"], (kf, n), True)
        bad = []
        if not np.abs(got["S"].astype(fi.LD) - Sx).max() <= bound:
            bad.append("|S - S_exact| above the bound")
        eu, ev = np.abs(al.conj().T @ al - np.eye(kf)).max(), np.abs(ar @ ar.conj().T - np.eye(kf)).max()
        if not (eu < 1e-12 and ev < 1e-12):
            bad.append(f"isometry al {eu:.3e} ar {ev:.3e} >= 1e-12")
        if np.abs(np.triu(c, 1)).max() != 0.0 or np.abs(np.diag(c).imag).max() != 0.0 or not np.all(np.diag(c).real > 0):
            bad.append("C is not lower triangular with a real positive diagonal")
        er = float(np.abs(al @ c @ ar - A).max())
        if not er <= bound:
            bad.append(f"|al c ar - A| = {er:.3e} > {bound:.3e}")
        return bad

    _add(Case("tsplit-c128-120x100", "factorizations", {"A": (F(A), F(Ad))},
              {"AL": 2 * m * kf, "C": 2 * kf * kf, "AR": 2 * kf * n, "S": kf}, run,
              _svd_reference(m, n, True), _factor_guard(A), sync=True, check=check, private="stream2"))


_csplit_case()


def _planted(m, n, pl, pr, sig, rng):
    """Y whose complement part is NL diag(sig) NR^T plus components inside span(QL) / span(QR) (tests/test_gpu_changebonds_inf.py)"""
    Qm, _ = np.linalg.qr(rng.standard_normal((m, m)))
    Qn, _ = np.linalg.qr(rng.standard_normal((n, n)))
    QL, NL = Qm[:, :pl], Qm[:, pl:]
    QR, NR = Qn[:, :pr].T, Qn[:, pr:].T
    r = min(m - pl, n - pr, len(sig))
    Y = (NL[:, :r] * sig[:r]) @ NR[:r] + QL @ rng.standard_normal((pl, n)) + rng.standard_normal((m, pr)) @ QR
    return Y, QL, np.ascontiguousarray(QR)


def _complement_case(m, n, p, k):
    """mpsk_complement_tsvd on a planted spectrum; min(m, n) > 64: the split route, else mpsk_tsvd of the complement part.
    The checks are the contract of include/mpsk.h, as tests/test_gpu_changebonds_inf.py applies it."""
    sig = 2.0 ** (-np.arange(min(m, n) - p) / 4.0)
    T = _planted(m, n, p, p, sig, np.random.default_rng(m + k))
    D = _planted(m, n, p, p, 3.0 * sig, np.random.default_rng(m + k + 1))

    def run(be, dev, obj):
        kept = C.c_int(-1)
        _lib_ok(be, be.lib.mpsk_complement_tsvd(be.ctx, m, n, dev["Y"].ptr, m, dev["QL"].ptr, m, p, dev["QR"].ptr, p, p, k, dev["U"].ptr,
                                               m, dev["S"].ptr, dev["Vt"].ptr, k, C.byref(kept)), "mpsk_complement_tsvd")
        return {"kept": kept.value}

    def reference(o):
        Y, QL, QR = Uf(o["Y"], (m, n)), Uf(o["QL"], (m, p)), Uf(o["QR"], (p, n))
        X = (np.eye(m) - QL @ QL.T) @ Y @ (np.eye(n) - QR.T @ QR)
        return {"S": np.linalg.svd(X, compute_uv=False)[:k]}

    def check(got):
        if int(got["ret:kept"]) != k:
            return [f"kept {got['ret:kept']}"]
        u, s, vt = Uf(got["U"], (m, k)), got["S"], Uf(got["Vt"], (k, n))
        QL, QR = T[1], T[2]
        bad = []
        if not np.all(np.diff(s) <= 0):
            bad.append("S is not descending")
        if not np.abs(s - sig[:k]).max() <= 1e-10 * max(sig[0], s[0]):
            bad.append(f"|S - sigma| = {np.abs(s - sig[:k]).max():.3e}")
        for what, e in (("U^T U", u.T @ u - np.eye(k)), ("Vt Vt^T", vt @ vt.T - np.eye(k)), ("QL^T U", QL.T @ u), ("Vt QR^T", vt @ QR.T)):
            if not np.abs(e).max() <= 1e-12:
                bad.append(f"{what}: {np.abs(e).max():.3e} > 1e-12")
        return bad

    def guard(o):
        QL, QR = Uf(o["QL"], (m, p)), Uf(o["QR"], (p, n))
        assert np.abs(QL.T @ QL - np.eye(p)).max() < 1e-13 and np.abs(QR @ QR.T - np.eye(p)).max() < 1e-13

    _add(Case(f"complement_tsvd-{m}x{n}-p{p}-k{k}", "factorizations", {"Y": (F(T[0]), F(D[0])), "QL": (F(T[1]), F(D[1])),
                                                                     "QR": (F(T[2]), F(D[2]))}, {"U": m * k, "S": k, "Vt": k * n},
              run, reference, guard, sync=True, check=check, private="stream2 / xstreams through mpsk_tsplit" if min(m, n) > 64 else ""))


_complement_case(96, 96, 48, 16)
_complement_case(40, 56, 20, 8)


# ----------------------------------------------------------------------------------------------------------------------
# Krylov vectors (tests/exact_vector_inputs.py): n = 4099 and the two-trip length D2_TRIP + 1
# ----------------------------------------------------------------------------------------------------------------------
VEC_K = 3                     # fused kernels (k <= 8)
VEC_K_LONG = 12               # the long CGS2 kernels (9 <= k <= 32)


def _families(n, cplx=False, kmax=VEC_K_LONG):
    return vi.Family(n, cplx, kmax), vi.Family(n, cplx, kmax + 1)        # the seed depends on kmax: another member, same n


def _vec_ops(ft, fd, k, extra=()):
    ops = {f"x{j}": (F(ft.x(j)), F(fd.x(j))) for j in range(k)}
    ops["y"] = (F(ft.y()), F(fd.y()))
    if "z" in extra:
        ops["z"] = (F(ft.z()), F(fd.z()))
    return ops


def _vec_guard(n, k, cplx=False):
    """the guard of tests/exact_vector_inputs.py (cgs2_sweep: the largest abs-sum any partial sum of two CGS rounds can
    reach, from the data) on the numerators read back from the flat operands"""
    from types import SimpleNamespace
    a = vi.exponent(n)

    def guard(o):
        X = np.stack([o[f"x{j}"] for j in range(k)]) * 2.0 ** a
        y = o["y"] if "y" in o else np.zeros_like(o["x0"])
        assert np.array_equal(np.round(X), X) and np.abs(X).max() <= 1, "basis off the dyadic grid"
        assert np.array_equal(np.round(y), y) and np.abs(y).max() <= 4, "y is not a small integer vector"
        X, y = X.astype(np.int64), y.astype(np.int64)
        fam = SimpleNamespace(a=a, n=n, cplx=cplx, Xr=X, yr=y)
        if cplx:
            fam = SimpleNamespace(a=a, n=n, cplx=True, Xr=X[:, 0::2], Xi=X[:, 1::2], yr=y[0::2], yi=y[1::2])
        assert next(vi.cgs2_sweep(fam, [k]))["guard"] < vi.LIMIT, "guard of the exact vector family"
    return guard


def _X(o, k, cplx=False):
    return np.stack([Uf(o[f"x{j}"], (-1,), cplx) for j in range(k)])


def _host_scalar_cases(n):
    ft, fd = _families(n)
    k = VEC_K
    xs = lambda dev, kk=k: [dev[f"x{j}"] for j in range(kk)]

    def run(be, dev, obj):
        d2 = be.vdiff_nrm2(dev["y"], dev["z"])
        return {"dot": be.dot(dev["x0"], dev["y"]), "nrm2": be.norm(dev["y"]), "diff": d2[0], "nx": d2[1],
                "multidot": be.multidot(xs(dev), dev["y"])}

    def reference(o):
        X, y, z = _X(o, k), o["y"], o["z"]
        return {"ret:dot": np.asarray(X[0] @ y), "ret:nrm2": np.asarray(np.sqrt(float(y @ y))), "ret:diff": np.asarray((y - z) @ (y - z)),
                "ret:nx": np.asarray(y @ y), "ret:multidot": X @ y}

    _add(Case(f"vdot+vnrm2+vdiff_nrm2+vmultidot-n{n}", "vectors", _vec_ops(ft, fd, k, ("z",)), {}, run, reference, _vec_guard(n, k),
              sync=True))

    def run_gs(be, dev, obj):
        return {"h": be.gs_step(xs(dev), dev["y"])}

    def ref_gs(o):
        X, y = _X(o, k), o["y"]
        h = X @ y
        return {"ret:h": h, "y": y - h @ X}

    _add(Case(f"vgs_step-n{n}", "vectors", _vec_ops(ft, fd, k), {"y": n}, run_gs, ref_gs, _vec_guard(n, k), sync=True))


def _orth_check(fam, k, dev_form, slot_off=3):
    """the checks of vi.run_orth on one record: coefficients bit for bit, |remainder|^2, beta and y inside the derived bounds"""
    rec = next(vi.cgs2_sweep(fam, [k]))
    assert rec["guard"] < vi.LIMIT
    nd = 2 * fam.n if fam.cplx else fam.n
    long = (not fam.cplx) and vi.MD < k <= vi.ML
    fn2, fb = vi.n2_factor(nd, long), vi.beta_factor(nd, long)
    b_ref = vi.beta_ld(rec)
    yn_ref = rec["y2"].astype(vi.CLD if fam.cplx else vi.LD) / b_ref

    def check(got):
        out = []
        y = got["y"].view(np.complex128) if fam.cplx else got["y"]
        vi.within(y, yn_ref, fb * np.abs(yn_ref), "y", out)
        if dev_form:
            s = got["slot"]
            vi.same(s[:slot_off], np.full(slot_off, -7.0), "slot head", out)
            vi.same(s[slot_off + 2 * k + 1:], np.full(2, -7.0), "slot tail", out)
            vi.same(s[slot_off:slot_off + k], rec["h1"], "h1", out)
            vi.same(s[slot_off + k:slot_off + 2 * k], rec["h2"], "h2", out)
            vi.close_exact(s[slot_off + 2 * k], vi.n2_fraction(rec), fn2, "n2", out)
        else:
            h = got["ret:h"].view(np.complex128) if fam.cplx else got["ret:h"]
            vi.same(h, rec["h"], "h", out)
            vi.within(got["ret:beta"], b_ref, fb * b_ref, "beta", out)
        return out
    return check


def _orth_ref(k, cplx=False):
    def reference(o):
        r = vi.numpy_cgs2(_X(o, k, cplx), Uf(o["y"], (-1,), cplx))
        return {"y": F(r["yn"]), "ret:h": F(r["h"])}
    return reference


def _orth_cases(n, k):
    ft, fd = _families(n)
    xs = lambda dev: [dev[f"x{j}"] for j in range(k)]

    def run(be, dev, obj):
        h, beta = be.orth_step(xs(dev), dev["y"])
        return {"h": h, "beta": beta}

    _add(Case(f"vorth_step-n{n}-k{k}", "vectors", _vec_ops(ft, fd, k), {"y": n}, run, _orth_ref(k), _vec_guard(n, k), sync=True,
              check=_orth_check(ft, k, False)))
    slot = np.full(3 + 2 * k + 1 + 2, -7.0)
    ops = _vec_ops(ft, fd, k)
    ops["slot"] = (slot, slot - 1.0)

    def run_dev(be, dev, obj):
        be.orth_step_dev(xs(dev), dev["y"], dev["slot"], 3)

    _add(Case(f"vorth_step_dev-n{n}-k{k}", "vectors", ops, {"y": n, "slot": slot.size}, run_dev, _orth_ref(k), _vec_guard(n, k),
              check=_orth_check(ft, k, True), extra={"scratch": ("slot",)}))


def _complex_vec_case(n):
    ft, fd = vi.Family(n, True, VEC_K), vi.Family(n, True, VEC_K + 1)
    k = VEC_K
    xs = lambda dev: [dev[f"x{j}"] for j in range(k)]

    def run(be, dev, obj):
        z = be.dotc(dev["x0"], dev["z"])
        h, beta = be.orth_step_c(xs(dev), dev["y"])
        return {"dotc": np.array([z.real, z.imag]), "h": h.view(np.float64), "beta": beta}

    def reference(o):
        r = _orth_ref(k, True)(o)
        z = np.vdot(Uf(o["x0"], (-1,), True), Uf(o["z"], (-1,), True))
        return dict(r, **{"ret:dotc": np.array([z.real, z.imag])})

    inner = _orth_check(ft, k, False)

    def check(got):
        out = inner(got)
        z = np.vdot(ft.x(0), ft.z())
        vi.same(got["ret:dotc"], np.array([z.real, z.imag]), "dotc", out)
        return out

    _add(Case(f"vdotc+vorth_step_c-n{n}", "vectors", _vec_ops(ft, fd, k, ("z",)), {"y": 2 * n}, run, reference,
              _vec_guard(n, k, True), sync=True, check=check))


def _device_slot_cases(n):
    ft, fd = _families(n)
    k = VEC_K
    N2 = float(int((ft.yr * ft.yr).sum()))
    fb = vi.beta_factor(n)
    yn_ref = ft.y().astype(vi.LD) / vi.beta_ld({"N2": int(N2), "e2": 0})
    cf, cfd = vi.lincomb_coefs(k), vi.lincomb_coefs(k + 1)[:k]
    ops = _vec_ops(ft, fd, k)
    ops["coef"] = (cf, cfd)

    def run(be, dev, obj):
        be.nrm2_dev(dev["y"], dev["slot"], 1)
        be.normalize_dev(dev["y"], out=dev["yn"], slot=dev["slot"], offset=2)
        be.lincomb_dev([dev[f"x{j}"] for j in range(k)], dev["coef"], out=dev["lc"])

    def reference(o):
        from stream_order import SENTINEL
        y = o["y"]
        return {"slot": np.array([SENTINEL, y @ y, y @ y, SENTINEL]), "yn": y / np.sqrt(y @ y), "lc": o["coef"] @ _X(o, k)}

    def check(got):
        out = []
        ref = reference({kk: v[0] for kk, v in ops.items()})
        vi.same(got["slot"], ref["slot"], "nrm2_dev / normalize_dev slot", out)
        vi.same(got["lc"], vi.exact_lincomb(ft, cf)[0], "lincomb_dev", out)
        vi.within(got["yn"], yn_ref, fb * np.abs(yn_ref), "normalize_dev", out)
        return out

    _add(Case(f"vnrm2_dev+vnormalize_dev+vlincomb_dev-n{n}", "vectors", ops, {"slot": 4, "yn": n, "lc": n}, run, reference,
              _vec_guard(n, k), check=check))
    m = 3
    S = vi.multilincomb_coefs(k, m)

    def run_ml(be, dev, obj):
        be.multilincomb([dev[f"x{j}"] for j in range(k)], S, [dev[f"o{j}"] for j in range(m)])

    _add(Case(f"vmultilincomb-n{n}", "vectors", {kk: v for kk, v in _vec_ops(ft, fd, k).items() if kk != "y"}, {f"o{j}": n for j in range(m)},
              run_ml, lambda o: {f"o{j}": S[:, j] @ _X(o, k) for j in range(m)}, _vec_guard(n, k)))


def _ritz_case():
    m, stride = 4, 9
    slot, slotd = vi.arnoldi_slots(m, stride), vi.arnoldi_slots(m, stride, seed="stream-order-decoy")
    ref = vi.ritz_reference(slot, m, stride)

    def run(be, dev, obj):
        be.ritz_dev(m, stride, dev["slot"], dev["buf"])

    def reference(o):
        c, info = vi.numpy_ritz(vi.ritz_reference(o["slot"], m, stride))
        return {"coef": c, "info": info}

    def check(got):
        coef, info = got["buf"][:m], got["buf"][32:35]
        out = [f"{kk} error {v:.2f} u-units > {vi.RITZ_BOUND:.2f}" for kk, v in vi.ritz_ratios(coef, info, ref).items()
               if not v <= vi.RITZ_BOUND]
        if info[2] != ref["me"]:
            out.append(f"effective m {info[2]}")
        return out

    def guard(o):                                   # synthesised Arnoldi slots: finite, and no invariant-subspace cut
        assert np.all(np.isfinite(o["slot"])) and vi.ritz_reference(o["slot"], m, stride)["me"] == m

    _add(Case("vritz_dev-m4", "vectors", {"slot": (slot, slotd)}, {"buf": 40}, run, reference, guard, check=check))


for _n in (4099, vi.D2_TRIP + 1):
    _host_scalar_cases(_n)
_orth_cases(4099, VEC_K)
_orth_cases(4099, VEC_K_LONG)
_orth_cases(vi.D2_TRIP + 1, VEC_K)
_complex_vec_case(4097)
_device_slot_cases(4099)
_device_slot_cases(vi.D2_TRIP + 1)
_ritz_case()

# ----------------------------------------------------------------------------------------------------------------------
# the dense-MPO GEMM route (tests/exact_dense_inputs.py), the quasiparticle site operator, the fixed-budget eigensolve
# ----------------------------------------------------------------------------------------------------------------------
def _dense_case(which):
    """the dense slice (3, 5, 2) at bonds (65, 33) with MPSK_DENSE_ROUTE=1 (the middle contraction as one GEMM):
    "dAC" = mpsk_dAC, "hac_axpby" = mpsk_hac_apply_axpby on the mode-4 operator (only x staged)"""
    import exact_dense_inputs as ed
    t = ed.site((3, 5, 2), (65, 33))
    Wl, Wr, d = t["slc"]
    Dl, Dr = t["bonds"]
    xd = _decoy_like("dense-x", t["x"])
    true = {"GL": ENV(t["Gs"]), "GR": ENV(t["R"]), "x": F(t["x"])}
    dec = {"GL": ENV(_decoy_like("dense-G", t["Gs"])), "GR": ENV(_decoy_like("dense-R", t["R"])), "x": F(xd)}

    def setup(be):
        obj = {"H": be.mposlice_dense(t["O"])}
        if which == "hac_axpby":
            obj["GL"], obj["GR"] = be.upload(true["GL"]).reshape(Wl, Dl, Dl), be.upload(true["GR"]).reshape(Wr, Dr, Dr)
            with env_setting(MPSK_DENSE_ROUTE=1):
                obj["hac"] = be.hac_create(obj["H"], obj["GL"], obj["GR"])
            assert obj["hac"].info()["mode"] == 4, obj["hac"].info()
        return obj

    def run(be, dev, obj):
        x, y = dev["x"].reshape(Dl, d, Dr), dev["y"].reshape(Dl, d, Dr)
        with env_setting(MPSK_DENSE_ROUTE=1):
            if which == "hac_axpby":
                obj["hac"].apply_axpby(ed.A1, x, ed.A0, out=y)
            else:
                be.dAC(obj["H"], dev["GL"].reshape(Wl, Dl, Dl), dev["GR"].reshape(Wr, Dr, Dr), x, out=y)

    def _over(o):
        return {"Gs": UENV(o.get("GL", true["GL"]), Dl, Wl, Dl), "G": UENV(o.get("GL", true["GL"]), Dl, Wl, Dl),
                "R": UENV(o.get("GR", true["GR"]), Dr, Wr, Dr), "x": Uf(o["x"], (Dl, d, Dr))}

    def reference(o):
        return {"y": F(ed.evaluate("hac_axpby" if which == "hac_axpby" else "hac_blk", t, over=_over(o)))}

    def guard(o):
        u = _over(o)
        ei.assert_exact_range([u["Gs"], u["x"], t["O"], u["R"], [abs(ed.A1) + abs(ed.A0)]], [Dl, Wl, d, Dr, Wr], "dense " + which)

    keep = ("x",) if which == "hac_axpby" else ("GL", "GR", "x")
    _add(Case(f"{'hac_apply_axpby-mode4' if which == 'hac_axpby' else 'dAC'}-dense-3x5x2-65x33", "operators",
              {k: (true[k], dec[k]) for k in keep}, {"y": Dl * d * Dr}, run, reference, guard, setup=setup))


_dense_case("dAC")
_dense_case("hac_axpby")


def _qp_heff_case():
    """mpsk_qp_half then mpsk_qp_heff_site with both pairs and a dyadic E on the ragged case of tests/exact_qp_inputs.py"""
    import exact_qp_inputs as eq
    t = eq.case("qp_heff", "ragged", "int", "sparse")
    key = ("all", eq.E_DYADIC)
    Dl, Dl2, Dr, Dr2, n = eq.SHAPES["ragged"]["heff"]
    d, O = t["s"].d, t["O"]
    W = O.shape[0]
    envs = {"G": (Dl, W, Dl), "R": (Dr, W, Dr), "lB": (Dl, W, Dl2), "rB": (Dr2, W, Dr)}
    mats = {"VL": (Dl * d, n), "X": (n, Dr), "AR": (Dl2, d, Dr), "AL": (Dl, d, Dr2)}
    lay = lambda k, a: ENV(a) if k in envs else F(a)
    ops = {k: (lay(k, t[k]), lay(k, _decoy_like("qp-" + k, t[k]))) for k in list(envs) + list(mats)}
    nhalf = W * d * Dl * Dr2

    def run(be, dev, obj):
        e = lambda k: dev[k].reshape(W, envs[k][0], envs[k][2])
        m = lambda k: dev[k].reshape(*mats[k])
        _lib_ok(be, be.lib.mpsk_qp_half(be.ctx, obj.handle, Dl, Dl, Dr2, dev["G"].ptr, dev["AL"].ptr, dev["half"].ptr), "mpsk_qp_half")
        be.qp_heff_site(obj, e("G"), e("R"), m("VL"), m("X"), eq.E_DYADIC, lB=e("lB"), AR=m("AR"), half=dev["half"], rB=e("rB"),
                        out=dev["out"].reshape(n, Dr))

    def _un(o):
        u = {k: UENV(o[k], *shp) for k, shp in envs.items()}
        u.update({k: Uf(o[k], shp) for k, shp in mats.items()})
        return u

    def reference(o):
        u = _un(o)
        B = eq.site_of(u["VL"], u["X"], d)
        y = eq.proj(u["G"], B, O, u["R"]) + eq.proj(u["lB"], u["AR"], O, u["R"]) + eq.proj(u["G"], u["AL"], O, u["rB"])
        return {"out": F(eq.pull(u["VL"], y) - eq.E_DYADIC * u["X"])}

    def guard(o):
        eq._magnitude("qp_heff", dict(_un(o), O=O, name=t["name"]), key)

    _add(Case("qp_half+qp_heff_site-ragged", "transfers", ops, {"half": nhalf, "out": n * Dr}, run, reference, guard,
              setup=lambda be: be.mposlice(*t["slice_args"])))


_qp_heff_case()


def _eigsolve_case():
    """mpsk_hac_eigsolve_fixed at m = 4 on the Jordan-form operator (mode 3) of tests/eigsolve_cases.py: the whole Arnoldi /
    Ritz loop is enqueued without a host synchronisation.  The Ritz vector within the module's bound B of its longdouble
    Lanczos, first_image within its componentwise bound."""
    import eigsolve_cases as ec
    c = ("ragged", 3, 4, "gauss")
    t = ec.case_operands(c)
    m, shape, n = c[2], t["x0"].shape, t["n"]
    xd = ei.gauss_array(ei._rng("stream-order-decoy-eigsolve"), *shape)
    nscal = m * (2 * m + 1) + 40
    c_order = lambda flat: Uf(flat, shape).ravel()                      # the module's vectors are the C-order ravel

    def setup(be):
        s = t["s"]
        H = be.mposlice(s.odim, s.d, s.chil, s.chir, dict(s.Os))
        GL, GR = be.upload_env(t["GL"]), be.upload_env(t["GR"])
        with env_setting(MPSK_HAC_MODE=3):
            hac = be.hac_create_ex(H, GL, GR, canonical=True)
        assert hac.info()["mode"] == 3, hac.info()
        return {"keep": (H, GL, GR), "hac": hac}

    def run(be, dev, obj):
        vecs = [dev[f"v{j}"].reshape(*shape) for j in range(m + 2)]
        obj["hac"].eigsolve_fixed(dev["x0"].reshape(*shape), m, vecs, dev["scal"], dev["y"].reshape(*shape), dev["first"].reshape(*shape))

    def reference(o):
        tt = dict(t, x0=Uf(o["x0"], shape))
        V, slot = ec._device_recurrence(tt, m)
        coef, lam, _ = ec._device_ritz(slot, m, 2 * m + 1)
        return {"y": ec._assemble(V, coef, m), "lambda": np.asarray(lam)}

    def check(got):
        r = ec.reference(c)
        B, _ = ec.bound(c)
        bad = []
        err = float(np.abs(c_order(got["y"]).astype(ec.LD) - r["y"]).max())
        if not err <= B:
            bad.append(f"|y - y_ref| = {err:.3e} > B = {B:.3e}")
        fb = ec.first_image_bound(t)
        if not np.all(np.abs(c_order(got["first"]).astype(ec.LD) - r["first"]) <= fb):
            bad.append("first_image outside its componentwise bound")
        if not np.array_equal(got["x0"], F(t["x0"])):
            bad.append("x0 was modified")
        lam = got["scal"][m * (2 * m + 1) + 32]
        if not abs(lam - r["theta"]) <= B * r["normH"]:
            bad.append(f"lambda {lam} against {r['theta']}")
        return bad

    def guard(o):                                                       # Gaussian family: finite operands, symmetric H_eff (asserted
        assert np.all(np.isfinite(o["x0"])) and float(o["x0"] @ o["x0"]) > 0     # by the module when it builds the operator)

    outs = {f"v{j}": n for j in range(m + 2)}
    outs.update(scal=nscal, y=n, first=n, x0=n)
    _add(Case("hac_eigsolve_fixed-m4-mode3-9x2x14", "vectors", {"x0": (F(t["x0"]), F(xd))}, outs, run, reference, guard, setup=setup,
              check=check))


_eigsolve_case()


def by_family():
    out = {}
    for c in CASES:
        out.setdefault(c.family, []).append(c)
    return out
