"""Cases for changebonds on interleaved complex storage: mpsk_complement_tsvd under MPSK_C128 (entry level, planted spectra)
and mpskit_jl_amd.native_cplx.changebonds on a NativeInfiniteMPS (state level).  The bodies take a backend:
tests/test_native_changebonds_cases_cpu.py runs them on the NumPy stand-ins below and records what it measured in
profiles/native_changebonds_bounds.log; tests/test_gpu_native_changebonds.py runs them on the device and reads its bounds
from that file.  Every bar comes from the contract of the entry (include/mpsk.h), from the planted data or from the host
run -- never from the code under test.

Entry level.  Y = NL diag(s) NR + QL G1 + G2 QR with complex unitaries from numpy.linalg.qr and Gaussian G1, G2: the part
inside the ranges of QL and QR^H is junk the projector must remove.  The contract: |S_j - s_j| <= 1e-10 s_0 and the four
orthogonality residuals <= 1e-12.  Where the planted gap allows, the projectors on the leading vectors match the planted
ones: a perturbation E of X turns a singular subspace separated by `gap` from the rest by sin(theta) <= |E| / gap (Wedin),
|E| is what the contract allows the values to move by, 1e-10 s_0, and left and right subspaces move together, hence
PROJECTOR_BAR = 2 * 1e-10 s_0 / gap.

"Flat" spectrum of the fallback case: with every non-zero singular value EQUAL, X is a multiple of a partial isometry, every
subspace of its range is a singular subspace and the check of the range finder passes rightly.  What cannot pass is a
spectrum that decays too slowly for the fixed number of iterations: s_j = 1 - j / 256 on a complement of 88 x 76, wider than
the r = 72 rows of the range finder: (s_73 / s_8)^9 = 0.13, eleven digits short of the 1e-12 of the check.

State level: d = 2, D = 4 and 6, unit cells of 1 and 2 sites, the Y-field Hamiltonian of tests/native_ham_inf_cases.py."""
import ctypes as C
import os

import numpy as np

import mpskit_jl_amd as mk
import mpskit_oracle as mo
import native_ham_inf_cases as hc
from cpu_backend_ham_inf import CpuHamInfBackend
from mpskit_jl_amd import native_cplx as nc
from mpskit_jl_amd.native_cplx import changebonds, expansion_directions  # noqa: F401  (the entries under test)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LOG = os.path.join(ROOT, "profiles", "native_changebonds_bounds.log")
F64_GOLDEN = os.path.join(ROOT, "tests", "golden", "complement_tsvd_f64.npz")
MARGIN = 100.0
S_BAR = 1e-10                         # |S_j - s_j| <= S_BAR s_0            (include/mpsk.h)
ORTH_BAR = 1e-12                      # U^H U, Vt Vt^H, QL^H U, Vt QR^H     (include/mpsk.h)
EPS = 2.220446049250313e-16
STATE_SIZES = [(1, 4), (2, 4), (1, 6)]      # (unit cell, D)
SENTINEL = -7.25 + 3.5j


def gauss_c(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ---- entry level: the cases ---------------------------------------------------------------------------------------------

def graded(n):
    return 2.0 ** (-np.arange(n, dtype=np.float64))


def planted(m, n, pl, pr, sig, rng, real=False):
    """(Y, QL or None, QR or None, NL, NR): the complement part of Y is NL[:, :r] diag(sig) NR[:r]"""
    g = (lambda *s: rng.standard_normal(s)) if real else (lambda *s: gauss_c(rng, *s))
    Qm, _ = np.linalg.qr(g(m, m))
    Qn, _ = np.linalg.qr(g(n, n))
    QL, NL = Qm[:, :pl], Qm[:, pl:]
    QR, NR = Qn[:, :pr].conj().T, Qn[:, pr:].conj().T
    r = min(m - pl, n - pr, len(sig))
    Y = (NL[:, :r] * sig[:r]) @ NR[:r]
    if pl:
        Y = Y + QL @ g(pl, n)
    if pr:
        Y = Y + g(m, pr) @ QR
    return Y, (QL if pl else None), (QR if pr else None), NL, NR


def entry_case(name):
    """{"Y", "QL", "QR", "k", "sig" (planted values, zero-padded to kept), "NL", "NR", "ld" (ldy, ldu, ldvt) or None, "route"}"""
    rng = np.random.default_rng(sum(map(ord, name)))
    ld, route, real = None, "subspace", False
    if name == "small_8":
        dims, sig, route = (8, 8, 4, 4, 2), graded(4), "full"
    elif name == "small_12x9":
        dims, sig, route = (12, 9, 4, 3, 3), graded(6), "full"
    elif name == "range_96x80":
        dims, sig = (96, 80, 48, 40, 8), graded(40)
    elif name == "range_80x120":
        dims, sig = (80, 120, 40, 60, 5), graded(40)
    elif name == "range_200x180":                  # the complement (160 x 150) is wider than the r = 72 rows of the range finder
        dims, sig = (200, 180, 40, 30, 8), graded(150)
    elif name == "range_ld":
        dims, sig, ld = (96, 80, 48, 40, 8), graded(40), (97, 99, 10)
    elif name == "left_none":
        dims, sig = (96, 80, 0, 40, 8), graded(40)
    elif name == "right_none":
        dims, sig = (96, 80, 48, 0, 8), graded(48)
    elif name == "flat":
        dims, sig, route = (96, 80, 8, 4, 8), 1.0 - np.arange(76) / 256.0, "full"
    elif name == "rank3":
        dims, sig = (96, 80, 48, 40, 8), np.array([3.0, 2.0, 1.0])
    elif name == "zero":
        dims, sig, route = (96, 80, 48, 40, 8), np.zeros(0), "full"
    elif name == "inside_QL":
        dims, sig, route = (96, 80, 48, 40, 8), np.zeros(0), "full"
    elif name == "real_operands":
        dims, sig, real = (96, 80, 48, 40, 8), graded(40), True
    else:
        raise KeyError(name)
    m, n, pl, pr, k = dims
    Y, QL, QR, NL, NR = planted(m, n, pl, pr, sig, rng, real)
    if name == "zero":
        Y = np.zeros_like(Y)
    if name == "inside_QL":
        Y = QL @ gauss_c(rng, pl, n)
    kept = min(k, m - pl, n - pr)
    ref = np.zeros(kept)
    ref[:min(kept, len(sig))] = sig[:kept]
    return dict(name=name, Y=Y.astype(np.complex128), QL=QL, QR=QR, k=k, kept=kept, sig=ref, rank=min(kept, len(sig)), NL=NL, NR=NR,
                ld=ld, route=route)


ENTRY_CASES = ["small_8", "small_12x9", "range_96x80", "range_80x120", "range_200x180", "range_ld", "left_none", "right_none",
               "flat", "rank3", "zero", "inside_QL", "real_operands"]


def zero_threshold(Y):
    """singular values at or below the rounding level of the projection are returned as exactly 0 (include/mpsk.h)"""
    m, n = Y.shape
    return 32.0 * EPS * np.sqrt(m + n) * max(np.abs(Y.real).max(initial=0.0), np.abs(Y.imag).max(initial=0.0))


def complement_tsvd_host(Y, QL, QR, k, rng=None):
    """NumPy reference of the entry: (U, S, Vt, kept) with the completion inside the complement"""
    rng = np.random.default_rng(7) if rng is None else rng
    m, n = Y.shape
    pl = 0 if QL is None else QL.shape[1]
    pr = 0 if QR is None else QR.shape[0]
    kept = max(0, min(k, m - pl, n - pr))
    if kept == 0:
        return None, None, None, 0
    PL = np.eye(m) - (QL @ QL.conj().T if pl else 0.0)
    PR = np.eye(n) - (QR.conj().T @ QR if pr else 0.0)
    u, s, vt = np.linalg.svd(PL @ Y @ PR)
    have = int(np.sum(s[:kept] > zero_threshold(Y)))
    U, Vt, S = gauss_c(rng, m, kept), gauss_c(rng, kept, n), np.zeros(kept)
    U[:, :have], Vt[:have], S[:have] = u[:, :have], vt[:have], s[:have]
    for _ in range(2):
        U, _ = mo.qrpos(PL @ U)
        _, Vt = mo.lqpos(Vt @ PR)
    return U, S, Vt, kept


def entry_residuals(case, u, s, vt):
    """what the contract bounds, measured: {"S", "UU", "VV", "QLU", "VQR", "PU", "PV" (projector differences, nan without a gap)}"""
    QL, QR, sig, kept = case["QL"], case["QR"], case["sig"], case["kept"]
    assert u.shape == (case["Y"].shape[0], kept) and vt.shape == (kept, case["Y"].shape[1]) and s.shape == (kept,)
    assert np.all(np.diff(s) <= 0), "S is not descending"
    out = {"S": np.abs(s - sig).max() / max(sig[0], s[0], 1e-300) if max(sig[0], s[0]) > 0 else 0.0,
           "UU": np.abs(u.conj().T @ u - np.eye(kept)).max(), "VV": np.abs(vt @ vt.conj().T - np.eye(kept)).max(),
           "QLU": 0.0 if QL is None else np.abs(QL.conj().T @ u).max(), "VQR": 0.0 if QR is None else np.abs(vt @ QR.conj().T).max(),
           "PU": float("nan"), "PV": float("nan")}
    bar = projector_bar(case)
    if bar is not None:
        g = case["rank"]
        NL, NR = case["NL"][:, :g], case["NR"][:g]
        out["PU"] = np.abs(u[:, :g] @ u[:, :g].conj().T - NL @ NL.conj().T).max()
        out["PV"] = np.abs(vt[:g].conj().T @ vt[:g] - NR.conj().T @ NR).max()
    return out


def projector_bar(case):
    """2 S_BAR s_0 / gap for the leading `rank` planted vectors, None when the planted gap is too small to say anything (the
    bar above 1e-6) or nothing is planted"""
    g, sig = case["rank"], case["sig"]
    if g == 0 or case["name"] == "flat":
        return None
    full = entry_planted_values(case)
    nxt = full[g] if len(full) > g else 0.0
    gap = sig[g - 1] - nxt
    bar = 2.0 * S_BAR * sig[0] / gap if gap > 0 else np.inf
    return bar if bar <= 1e-6 else None


def entry_planted_values(case):
    return {"small_8": graded(4), "small_12x9": graded(6), "range_96x80": graded(40), "range_80x120": graded(40),
            "range_200x180": graded(150), "range_ld": graded(40), "left_none": graded(40), "right_none": graded(48),
            "rank3": np.array([3.0, 2.0, 1.0]), "real_operands": graded(40)}.get(case["name"], np.zeros(0))


def check_entry(case, u, s, vt):
    """the contract's own bars, the exact zeros beyond the rank and the projector bar; returns the residuals"""
    res = entry_residuals(case, u, s, vt)
    assert res["S"] <= S_BAR, res
    for key in ("UU", "VV", "QLU", "VQR"):
        assert res[key] <= ORTH_BAR, (key, res)
    assert np.all(s[case["rank"]:] == 0.0), s
    bar = projector_bar(case)
    if bar is not None:
        assert res["PU"] <= bar and res["PV"] <= bar, (res, bar)
    return res


def host_entry(case):
    U, S, Vt, kept = complement_tsvd_host(case["Y"], case["QL"], case["QR"], case["k"])
    assert kept == case["kept"]
    return U, S, Vt


def _padded(a, ld):
    out = np.full((ld, a.shape[1]), SENTINEL, dtype=np.complex128)
    out[:a.shape[0]] = a
    return out


def device_entry(be, case, cplx=True):
    """the entry through its C signature (leading dimensions, NULL pointers); returns host (u, s, vt).  With case["ld"] the
    operands sit in padded buffers whose padding rows must come back untouched.  cplx=False: the fp64 entry on real operands."""
    Y, QL, QR, k, kept = case["Y"], case["QL"], case["QR"], case["k"], case["kept"]
    m, n = Y.shape
    ldy, ldu, ldvt = case["ld"] if case["ld"] else (m, m, max(kept, 1))
    up = be.upload_c if cplx else (lambda a: be.upload(np.ascontiguousarray(a.real)))
    down = be.download_c if cplx else be.download
    dY = up(_padded(Y, ldy))
    dQL = None if QL is None else up(QL)
    dQR = None if QR is None else up(QR)
    dU, dVt = up(np.full((ldu, kept), SENTINEL)), up(np.full((ldvt, n), SENTINEL))
    dS = be.upload(np.full(kept, -1.0))
    got = C.c_int(-1)
    from mpskit_jl_amd._lib import check
    be._set_dtype(cplx)
    try:
        check(be.lib.mpsk_complement_tsvd(be.ctx, m, n, dY.ptr, ldy, None if dQL is None else dQL.ptr, m,
                                          0 if QL is None else QL.shape[1], None if dQR is None else dQR.ptr,
                                          1 if QR is None else QR.shape[0], 0 if QR is None else QR.shape[0], k, dU.ptr, ldu,
                                          dS.ptr, dVt.ptr, ldvt, C.byref(got)), "mpsk_complement_tsvd")
    finally:
        be._set_dtype(False)
    assert got.value == kept, (got.value, kept)
    u, vt, s = down(dU), down(dVt), be.download(dS)
    sent = SENTINEL if cplx else SENTINEL.real
    assert np.all(u[m:] == sent) and np.all(vt[kept:] == sent), "padding rows were written"
    assert np.all(down(dY)[m:] == sent)
    return u[:m], s, vt[:kept]


def f64_golden_case():
    """the fp64 case whose device output is pinned bit for bit (tests/golden/complement_tsvd_f64.npz): real planted operands of
    the kind tests/test_gpu_changebonds_inf.py uses, range-finder route of the fp64 split"""
    rng = np.random.default_rng(260)
    m, n, p, k = 260, 390, 130, 16
    sig = 2.0 ** (-np.arange(130) / 4.0)
    Qm, _ = np.linalg.qr(rng.standard_normal((m, m)))
    Qn, _ = np.linalg.qr(rng.standard_normal((n, n)))
    QL, NL, QR, NR = Qm[:, :p], Qm[:, p:], Qn[:, :p].T, Qn[:, p:].T
    Y = (NL * sig) @ NR[:p] + QL @ rng.standard_normal((p, n)) + rng.standard_normal((m, p)) @ QR
    return Y, QL, QR, k, sig


def f64_golden_run():
    """on a context of its own: the iteration count of the fp64 split starts from what the context's last call needed"""
    Y, QL, QR, k, _ = f64_golden_case()
    be = mk.Backend(0)
    try:
        U, S, Vt, kept = be.complement_tsvd(be.upload(Y), be.upload(QL), be.upload(QR), k)
        return be.download(U), be.download(S), be.download(Vt)
    finally:
        be.close()


# ---- the NumPy stand-ins ----------------------------------------------------------------------------------------------------

class CpuChangebondsBackend(CpuHamInfBackend):
    """CpuHamInfBackend + what the composed route of native_cplx.changebonds calls: tsvd_c and the complex dAC2_proj.  It has no
    complement_tsvd_c: the dispatch takes the composed route."""

    def tsvd_c(self, theta, max_keep=0, trunc_err=0.0):
        self._count("tsvd_c")
        U, S, Vh = np.linalg.svd(self.download_c(theta), full_matrices=False)
        k = len(S) if not max_keep else min(len(S), int(max_keep))
        if trunc_err > 0:
            while k > 1 and np.sqrt(np.sum(S[k - 1:] ** 2)) <= trunc_err:
                k -= 1
        return self.upload_c(U), self.upload(S), self.upload_c(Vh), k, float(np.sqrt(np.sum(S[k:] ** 2)))

    def dAC2_proj(self, H1, H2, GL, GR, AC, AR, out=None):
        assert getattr(H1, "cplx", False) and getattr(H2, "cplx", False), "the stand-in contracts complex slices only"
        self._count("dAC2_proj_c")
        theta = np.einsum("asm,mtb->asbt", self.download_c(AC), self.download_c(AR))
        y = mo.dAC2(theta, H1.oracle, H2.oracle, self._env_c(GL, H1.chil), self._env_c(GR, H2.chir))
        o = self.empty(GL.shape[1], y.shape[1], y.shape[2], y.shape[3]) if out is None else out
        return self._set_c(o, y)


class CpuChangebondsDeviceBackend(CpuChangebondsBackend):
    """and the NumPy reference of mpsk_complement_tsvd under MPSK_C128, so that the "device" route of the host code runs here"""

    def complement_tsvd_c(self, Y, QL, QR, k):
        self._count("complement_tsvd_c")
        U, S, Vt, kept = complement_tsvd_host(self.download_c(Y), None if QL is None else self.download_c(QL),
                                              None if QR is None else self.download_c(QR), k)
        if kept == 0:
            return None, None, None, 0
        return self.upload_c(U), self.upload(S), self.upload_c(Vt), kept


# ---- state level ----------------------------------------------------------------------------------------------------------

def random_state(be, n, D, seed=11):
    return nc.NativeInfiniteMPS.random(2, D, np.random.default_rng(seed + 10 * n + D), n=n, be=be)


def gauge_residual(psi):
    """largest of |AL^H AL - 1|, |AR AR^H - 1|, |AL CR - AC|, |CR AR - AC| over the unit cell (max-abs)"""
    h, n, worst = psi.to_host(), len(psi), 0.0
    for i in range(n):
        al, ar, ac, c, cl = h["AL"][i], h["AR"][i], h["AC"][i], h["CR"][i], h["CR"][(i - 1) % n]
        Dl, d, Dr = al.shape
        worst = max(worst, np.abs(np.einsum("asb,asc->bc", al.conj(), al) - np.eye(Dr)).max(),
                    np.abs(np.einsum("asb,csb->ac", ar, ar.conj()) - np.eye(Dl)).max(),
                    np.abs(np.einsum("asb,bc->asc", al, c) - ac).max(), np.abs(np.einsum("ab,bsc->asc", cl, ar) - ac).max())
    return worst


def case_gauge(be, n, D, kind, route):
    """OptimalExpand(2) / RandExpand(2) on a random state: (gauge residual, | |dot(new, old)| - 1 |); sizes are asserted"""
    psi = random_state(be, n, D)
    if kind == "optimal":
        new, envs = nc.changebonds(psi, hc.tfi_y(be, hc.G0), mk.OptimalExpand(trunc_dim=2), route=route)
        assert isinstance(envs, nc.NativeMPOHamInfEnv)
    else:
        new = nc.changebonds(psi, mk.RandExpand(trunc_dim=2), rng=np.random.default_rng(3), route=route)
    assert isinstance(new, nc.NativeInfiniteMPS) and len(new) == n
    for i in range(n):
        assert new.dims(i) == (D + 2, 2, D + 2) and new.CR[i].shape == (2 * (D + 2), D + 2)
        assert psi.dims(i) == (D, 2, D)                                  # a copying version
    return gauge_residual(new), abs(abs(nc.dot(new, psi)) - 1.0)


def literal_singular_values(Y, al, ar, k):
    """optimalexpand.jl:25-32 by NumPy: null spaces from the complete QR, full SVD"""
    Dl, d, Dm = al.shape
    m = Dl * d
    A = al.reshape(m, Dm, order="F")
    B = np.transpose(ar, (0, 2, 1)).reshape(Dm, -1, order="F")           # [m, (b, s)]
    NL = np.linalg.qr(A, mode="complete")[0][:, Dm:]
    NR = np.linalg.qr(B.conj().T, mode="complete")[0][:, Dm:].conj().T
    return np.linalg.svd(NL.conj().T @ Y @ NR.conj().T, compute_uv=False)[:k]


def case_singular_values(be, n, D, routes):
    """per bond and route: S of native_cplx.expansion_directions against the literal algorithm on the downloaded tensors.
    Returns the largest |S - S_literal| / S_literal[0] and the largest difference between the routes, same scale."""
    psi = random_state(be, n, D)
    H = hc.tfi_y(be, hc.G0)
    envs = nc.environments(psi, H)
    worst, between, k = 0.0, 0.0, 2
    for i in range(n):
        Y = be.dAC2_proj(envs.O(i), envs.O(i + 1), envs.leftenv(i, psi), envs.rightenv(i + 1, psi), psi.AC[i], psi.AR[(i + 1) % n])
        Yh = be.download_c(Y).reshape(D * 2, D * 2, order="F")
        ref = literal_singular_values(Yh, be.download_c(psi.AL[i]), be.download_c(psi.AR[(i + 1) % n]), k)
        got = {}
        for route in routes:
            U, Vt, S, kept = nc.expansion_directions(psi, H, envs, i, k, route=route)
            assert kept == k and U.shape == (4 * D, k) and Vt.shape == (2 * k, 2 * D)
            got[route] = S
            worst = max(worst, np.abs(S - ref).max() / ref[0])
        if len(routes) == 2:
            between = max(between, np.abs(got[routes[0]] - got[routes[1]]).max() / ref[0])
    return worst, between


def case_real_groundstate(be, n, D, route):
    """S of the expansion of a real ground state on interleaved storage against mk.changebonds.expansion_directions on the real
    InfiniteMPS.  Returns (largest |S_c - S_r|, S_r[0], |Y|_F): the two environments are solved to ENV_TOL independently, so
    the operands Y differ by ~ENV_TOL |Y| and the values with them."""
    from mpskit_jl_amd.changebonds import expansion_directions
    psi, H, _, _ = hc.real_groundstate(be, n, D)
    envs = mk.environments(psi, H)
    nat = nc.NativeInfiniteMPS.from_real(psi)
    nenv = nc.environments(nat, H)
    worst, s0, ynorm = 0.0, 0.0, 0.0
    for i in range(n):
        _, _, Sr, kr = expansion_directions(psi, H, envs, i, 2, route="composed")
        _, _, Sc, kc = nc.expansion_directions(nat, H, nenv, i, 2, route=route)
        assert kr == kc == 2
        Y = be.dAC2_proj(nenv.O(i), nenv.O(i + 1), nenv.leftenv(i, nat), nenv.rightenv(i + 1, nat), nat.AC[i], nat.AR[(i + 1) % n])
        worst, s0, ynorm = max(worst, np.abs(Sc - Sr).max()), max(s0, Sr[0]), max(ynorm, be.norm(Y))
    return worst, s0, ynorm


def real_groundstate_bar(s0, ynorm):
    return S_BAR * s0 + MARGIN * hc.ENV_TOL * ynorm


def schmidt(be, psi, i=0):
    return np.linalg.svd(be.download_c(psi.CR[i]), compute_uv=False)


def case_svdcut(be, n, D, route):
    """expand by 2, cut back: SvdCut(trunc_dim = D) and SvdCut(trunc_err) both return bond D and the state.  The expanded state
    has D Schmidt values of a random state and 2 zeros: the cut 1e-8 falls in that gap (asserted).  Returns the largest
    | |dot| - 1 | and the largest |Schmidt value kept - Schmidt value before|."""
    psi = random_state(be, n, D)
    big = nc.changebonds(psi, mk.RandExpand(trunc_dim=2), rng=np.random.default_rng(5), route=route)
    worst_dot, worst_s = 0.0, 0.0
    for alg in (mk.SvdCut(trunc_dim=D), mk.SvdCut(trunc_err=1e-8)):
        cut = nc.changebonds(big, alg)
        for i in range(n):
            s_old, s_big = schmidt(be, psi, i), schmidt(be, big, i)
            assert s_old[-1] > 1e-4 and np.all(s_big[D:] < 1e-12), (s_old, s_big)
            assert cut.dims(i) == (D, 2, D)
            worst_s = max(worst_s, np.abs(schmidt(be, cut, i) - s_old).max())
        worst_dot = max(worst_dot, abs(abs(nc.dot(cut, psi)) - 1.0))
    return worst_dot, worst_s


def case_growing(be, route=None):
    """VUMPS at D = 4, OptimalExpand to 8, VUMPS again on the Y-field model, one-site unit cell.  Returns (E4, E8, eps8, E_ref)."""
    n = 1
    _, _, E_ref, _ = hc.real_groundstate(be, n, 8)
    H = hc.tfi_y(be, hc.G0)
    psi = nc.NativeInfiniteMPS.random(2, 4, np.random.default_rng(6), n=n, be=be)
    alg = mk.VUMPS(tol=hc.VUMPS_TOL, maxiter=200)
    psi, envs, _ = mk.find_groundstate(psi, H, alg)
    E4 = complex(np.sum(mk.expectation_value(psi, H, envs))) / n
    psi, envs = nc.changebonds(psi, H, mk.OptimalExpand(trunc_dim=4), envs, route=route)
    assert psi.dims(0) == (8, 2, 8)
    psi, envs, eps = mk.find_groundstate(psi, H, alg, envs)
    E8 = complex(np.sum(mk.expectation_value(psi, H, envs))) / n
    return E4, E8, eps, E_ref


def case_real_time(be, route=None, steps=5, dt=0.05):
    """g = 0.7 ground state at D = 4 under the g = 1.2 Hamiltonian: 5 TDVP steps, OptimalExpand(2), 5 more.  Returns (|E after the
    expansion - E before|, energy drift over the whole run), energies per site from fresh environments."""
    psi0, _, _, _ = hc.real_groundstate(be, 1, 4)
    H = hc.tfi(be, hc.G1)
    psi = nc.NativeInfiniteMPS.from_real(psi0)
    envs = nc.environments(psi, H)
    energy = lambda p: float(np.sum(mk.expectation_value(p, H, nc.environments(p, H))).real)
    e0 = energy(psi)
    for k in range(steps):
        psi, envs = mk.timestep(psi, H, k * dt, dt, mk.TDVP(), envs)
    before = energy(psi)
    psi, envs = nc.changebonds(psi, H, mk.OptimalExpand(trunc_dim=2), envs, route=route)
    assert psi.dims(0) == (6, 2, 6)
    after = energy(psi)
    for k in range(steps, 2 * steps):
        psi, envs = mk.timestep(psi, H, k * dt, dt, mk.TDVP(), envs)
    assert psi.dims(0) == (6, 2, 6)
    return abs(after - before), abs(energy(psi) - e0)


def case_refusals(be):
    import pytest
    psi = random_state(be, 1, 4)
    psi3 = random_state(be, 3, 4)
    H = hc.tfi(be, hc.G0)
    alg = mk.OptimalExpand(trunc_dim=2)
    with pytest.raises(NotImplementedError, match="LazySum"):
        nc.changebonds(psi, mk.LazySum([H, H]), alg)
    with pytest.raises(NotImplementedError, match="MultipliedOperator"):
        nc.changebonds(psi, mk.MultipliedOperator(H, lambda t: 1.0 + t), alg)
    with pytest.raises(NotImplementedError, match="DenseMPO"):
        nc.changebonds(psi, mk.classical_ising(), alg)
    with pytest.raises(NotImplementedError, match="MPOMultiline"):
        nc.changebonds(psi, mk.MPOMultiline.__new__(mk.MPOMultiline), alg)
    two = nc.ComplexMPOHamiltonian([{(0, 0): 1, (0, 1): -hc.Z, (1, 2): hc.Z, (0, 2): -hc.G0 * hc.Y, (2, 2): 1}] * 2, be)
    with pytest.raises(ValueError, match="multiple"):
        nc.changebonds(psi3, two, alg)
    with pytest.raises(TypeError, match="unknown changebonds algorithm"):
        nc.changebonds(psi, H, mk.VUMPS())
    with pytest.raises(TypeError, match="needs the operator"):
        nc.changebonds(psi, alg)
    with pytest.raises(TypeError, match="NativeInfiniteMPS"):
        nc.changebonds(mk.InfiniteMPS.random(2, 4, np.random.default_rng(1), be=be), H, alg)
    with pytest.raises(ValueError, match="route"):
        nc.changebonds(psi, H, alg, route="fastest")
    with pytest.raises(NotImplementedError, match="changebonds"):
        mk.changebonds(psi, H, alg)


# ---- the bounds file ------------------------------------------------------------------------------------------------------

def write_bounds(records, lines):
    """records: {name: (measured value, floor)}; the bound of each is MARGIN x max(value, floor)"""
    with open(BOUNDS_LOG, "w") as f:
        f.write("# written by tests/test_native_changebonds_cases_cpu.py (NumPy stand-ins); read by "
                "tests/test_gpu_native_changebonds.py\n")
        f.write(f"# BOUND <name> <bound> = {MARGIN:g} x max(what the host run measured, the floor of that quantity: one rounding "
                "error of the data for residuals, the tolerance of the solver behind it for overlaps and energies)\n")
        for text in lines:
            f.write("NATIVE-CHANGEBONDS host " + text + "\n")
        for name in sorted(records):
            v, floor = records[name]
            f.write(f"BOUND {name} {MARGIN * max(v, floor):.6e}\n")


def read_bounds():
    out = {}
    with open(BOUNDS_LOG) as f:
        for line in f:
            if line.startswith("BOUND "):
                _, name, val = line.split()
                out[name] = float(val)
    return out
