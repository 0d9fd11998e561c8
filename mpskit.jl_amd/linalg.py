"""Linear algebra of finite MPS (src/states/finitemps.jl:365-469): psi1 + psi2, psi1 - psi2, a * psi, dot(psi1, psi2),
normalize -- for FiniteMPS (real and bond-embedded complex tensors, cplx.py) and for NativeFiniteMPS (interleaved complex).

The sum is the reference's algorithm: a QRpos sweep from the left over sites 0 .. L//2 - 1, an LQpos sweep from the right over
sites L - 1 .. L//2, and the centre bond R (C1 (+) C2) L.  The isometries F1 / F2 that embed the addends' bonds into the
direct sum are never formed: they are block offsets.  The site step -- the carried gauge factor times the direct sum of the
two site tensors -- is one launch of mpsk_dsum_site (Backend.dsum_site) on the fused route, and two GEMMs (plus two strided
copies on the right half, whose blocks interleave along the fastest index) on the composed route.  A backend without
dsum_site takes the composed route; FUSED_BY_DEFAULT picks the route where both exist.

Near the edges the matrix to factor is wider than tall (rows < cols): the bond dimension is min(rows, cols) = rows, so the
isometry is square and ANY orthogonal matrix does; the identity (on the right half: the permutation that is the identity on
the (s, b) pair) is the exact choice, costs nothing, and is an embedding when the tensors are.
"""
from __future__ import annotations

import numpy as np

from ._lib import MpskError
from .backend import DTensor
from .states import FiniteMPS, leftorth, rightorth
from .native_cplx import NativeFiniteMPS

# Route of the site step where the backend has both (fused=None), by the measured table profiles/dsum_timings.json
# (tools/bench_dsum.py; L = 32, d = 2, site step at the bulk shape, fused vs composed in ms):
#   D1 = D2 = 64: left 0.021 / 0.027, right 0.021 / 0.035;   256: 0.030 / 0.046, 0.030 / 0.052;
#   1024: left 0.333 / 0.320, right 0.295 / 0.320.
# The right-hand step (whose composed route needs two strided copies) is fused at every size; the left-hand step, whose
# composed route is two plain GEMMs, is fused below FUSED_LEFT_BELOW (between 256 and 1024 nothing was measured).
FUSED_BY_DEFAULT = True
FUSED_LEFT_BELOW = 1024


def _use_fused(be, fused, large=False):
    has = hasattr(be, "dsum_site")
    if fused and not has:
        raise MpskError("fused=True: this backend has no dsum_site")
    return (has and FUSED_BY_DEFAULT and not large) if fused is None else bool(fused)


# ---- site steps on real / embedded tensors ---------------------------------------------------------------------------------

def dsum_left(be, G: DTensor, A1: DTensor, A2: DTensor, fused=None):
    """out[Dn, d, E1 + E2]: out[:, :, :E1] = G[:, :D1] A1, out[:, :, E1:] = G[:, D1:] A2   (finitemps.jl:397-406)"""
    if _use_fused(be, fused, large=max(A1.shape[0], A2.shape[0]) >= FUSED_LEFT_BELOW):
        return be.dsum_site("left", G, A1, A2)
    Dn = G.shape[0]
    (D1, d, E1), (D2, _, E2) = A1.shape, A2.shape
    out = be.empty(Dn, d, E1 + E2)
    be.gemm_raw(False, False, Dn, d * E1, D1, 1.0, G.ptr, Dn, A1.ptr, D1, 0.0, out.ptr, Dn)
    be.gemm_raw(False, False, Dn, d * E2, D2, 1.0, G.ptr + 8 * Dn * D1, Dn, A2.ptr, D2, 0.0, out.ptr + 8 * Dn * d * E1, Dn)
    return out


def dsum_right(be, G: DTensor, A1: DTensor, A2: DTensor, fused=None):
    """out[D1 + D2, d, Dn]: out[:D1, s, :] = A1[:, s, :] G[:E1, :], out[D1:, s, :] = A2[:, s, :] G[E1:, :]   (:423-432)"""
    if _use_fused(be, fused):
        return be.dsum_site("right", G, A1, A2)
    Et, Dn = G.shape
    (D1, d, E1), (D2, _, E2) = A1.shape, A2.shape
    out = be.empty(D1 + D2, d, Dn)
    for A, D, E, g_off, o_off in ((A1, D1, E1, 0, 0), (A2, D2, E2, E1, D1)):
        T = be.empty(D * d, Dn)
        be.gemm_raw(False, False, D * d, Dn, E, 1.0, A.ptr, D * d, G.ptr + 8 * g_off, Et, 0.0, T.ptr, D * d)
        be.copy2d(D, d * Dn, T.ptr, D, out.ptr + 8 * o_off, D1 + D2)        # rows (a, s) -> a + s (D1 + D2)
    return out


def _factor_left(be, M: DTensor, cplx):
    """M[Dn, d, E] -> (AL[Dn, d, k], R[k, E]), k = min(Dn d, E)"""
    Dn, d, E = M.shape
    if Dn * d >= E:
        return leftorth(be, M, cplx)
    return be.upload(np.eye(Dn * d)).reshape(Dn, d, Dn * d), M.reshape(Dn * d, E)


def _factor_right(be, M: DTensor, cplx):
    """M[Dt, d, Dn] -> (L[Dt, k], AR[k, d, Dn]), k = min(Dt, d Dn)"""
    Dt, d, Dn = M.shape
    if Dt <= d * Dn:
        return rightorth(be, M, cplx)
    c = 2 if cplx else 1
    K, Dr = d * Dn // c, Dn // c
    P = np.eye(K).reshape((K, d, Dr), order="F")                 # P[k, s, b] = delta(k, s + d b)
    if cplx:
        from .cplx import embed
        P = embed(P)
    AR = be.upload(P)
    return be.gemm(M.reshape(Dt, d * Dn), AR.reshape(d * Dn, d * Dn), transB=True), AR


def _check_pair(what, psi1, psi2, dims1, dims2):
    if len(psi1) != len(psi2):
        raise ValueError(f"Cannot {what} states of length {len(psi1)} and {len(psi2)}")
    if psi1.be is not psi2.be:
        raise ValueError(f"Cannot {what} states that live on two backends")
    for i, (a, b) in enumerate(zip(dims1, dims2)):
        if a != b:
            raise ValueError(f"Cannot {what} states whose physical dimensions differ at site {i} ({a} and {b})")


def _phys(psi):
    if isinstance(psi, NativeFiniteMPS):
        return [psi.dims(i)[1] for i in range(len(psi))]
    return [(psi.ALs[i] or psi.ARs[i] or psi.ACs[i]).shape[1] for i in range(len(psi))]


def add(psi1, psi2, fused=None):
    """psi1 + psi2 (finitemps.jl:375-443) in canonical form: AL on sites < L//2, AR on sites >= L//2, one bond matrix.
    Untruncated: the bonds are min(rows, cols) of each factored matrix (D1 + D2 in the bulk).  fused: None = the default
    route, True / False = insist on mpsk_dsum_site / on the composed route."""
    if isinstance(psi1, NativeFiniteMPS) and isinstance(psi2, NativeFiniteMPS):
        return _add_native(psi1, psi2)
    if not (isinstance(psi1, FiniteMPS) and isinstance(psi2, FiniteMPS)):
        raise TypeError(f"add takes two FiniteMPS or two NativeFiniteMPS, not {type(psi1).__name__} and {type(psi2).__name__}")
    _check_pair("add", psi1, psi2, _phys(psi1), _phys(psi2))
    if psi1.cplx != psi2.cplx:
        raise ValueError("Cannot add a real and a complex state: build both from complex tensors")
    N, be, cx = len(psi1), psi1.be, psi1.cplx
    if N < 2:
        raise ValueError("add is not implemented for length < 2")
    half = N // 2
    b = 2 if cx else 1                                             # boundary bond (embedded: the 2x2 block of the number 1)
    ALs, ARs = [None] * N, [None] * N
    G = be.upload(np.hstack([np.eye(b), np.eye(b)]))               # F1' + F2' at the left edge: [1 1]
    for i in range(half):
        ALs[i], G = _factor_left(be, dsum_left(be, G, psi1.AL(i), psi2.AL(i), fused), cx)
    R = G
    G = be.upload(np.vstack([np.eye(b), np.eye(b)]))
    for i in range(N - 1, half - 1, -1):
        G, ARs[i] = _factor_right(be, dsum_right(be, G, psi1.AR(i), psi2.AR(i), fused), cx)
    C1, C2 = psi1.CR(half - 1), psi2.CR(half - 1)
    RC = dsum_left(be, R, C1.reshape(C1.shape[0], 1, C1.shape[1]), C2.reshape(C2.shape[0], 1, C2.shape[1]), fused)
    CLs = [None] * (N + 1)
    CLs[half] = be.gemm(RC.reshape(R.shape[0], G.shape[0]), G)     # R (C1 (+) C2) L
    return FiniteMPS.from_canonical(ALs, ARs, [None] * N, CLs, be, cplx=cx)


def sub(psi1, psi2, fused=None):
    """psi1 - psi2 = psi1 + (-1 * psi2)   (finitemps.jl:445)"""
    return add(psi1, scale(psi2, -1.0), fused)


# ---- scalars ---------------------------------------------------------------------------------------------------------------

def _scaled(be, t: DTensor, a: complex):
    """a new tensor a * t; a complex a acts on an embedded / interleaved tensor through the (re, im) pairs of its first index"""
    if a.imag == 0.0:
        return be.scal(a.real, be.copy(t))
    return be.axpby(a.real, t, a.imag, be.times_i(t))


def scale_(psi, a):
    """lmul! / rmul! (finitemps.jl:447-457): every cached AC and CL is replaced by its multiple (the tensors themselves are
    shared with copies of the state and stay as they are)."""
    a = complex(a)
    if isinstance(psi, NativeFiniteMPS):
        psi.A[psi.center] = _scaled(psi.be, psi.A[psi.center], a)
        return psi
    if a.imag != 0.0 and not psi.cplx:
        raise TypeError("a real state times a complex number: build the state from complex tensors")
    if all(t is None for t in psi.ACs) and all(t is None for t in psi.CLs):
        psi.AC(0)
    psi.ACs = [None if t is None else _scaled(psi.be, t, a) for t in psi.ACs]
    psi.CLs = [None if t is None else _scaled(psi.be, t, a) for t in psi.CLs]
    return psi


def scale(psi, a):
    """a * psi = psi * a (finitemps.jl:372-373)"""
    return scale_(psi.copy(), a)


def normalize_(psi):
    """normalize! (finitemps.jl:468)"""
    return scale_(psi, 1.0 / psi.norm())


def normalize(psi):
    """normalize (finitemps.jl:469): a normalised copy"""
    return normalize_(psi.copy())


# ---- overlap ---------------------------------------------------------------------------------------------------------------

def _widened(psi):
    """(AC(0), [AR(1) ..]) of a real state as embedded tensors: a real state next to a complex one (cold path)"""
    from .cplx import embed
    be = psi.be
    up = lambda t: be.upload(embed(be.download(t)))
    return up(psi.AC(0)), [up(psi.AR(i)) for i in range(1, len(psi))]


def dot(psi1, psi2):
    """dot(psi1, psi2) = <psi1|psi2> (finitemps.jl:459-464), conjugate-linear in psi1: the pass-through right transfers of
    (psi2.AR, psi1.AR) over sites 1 .. L - 1, closed with the two AC(0).  float for two real states, complex otherwise."""
    if isinstance(psi1, NativeFiniteMPS) and isinstance(psi2, NativeFiniteMPS):
        return _dot_native(psi1, psi2)
    if not (isinstance(psi1, FiniteMPS) and isinstance(psi2, FiniteMPS)):
        raise TypeError(f"dot takes two FiniteMPS or two NativeFiniteMPS, not {type(psi1).__name__} and {type(psi2).__name__}")
    if len(psi1) != len(psi2):
        raise ValueError(f"MPS with different length ({len(psi1)} and {len(psi2)})")
    _check_pair("take the overlap of", psi1, psi2, _phys(psi1), _phys(psi2))
    N, be = len(psi1), psi1.be
    cx = psi1.cplx or psi2.cplx
    (bra0, bra), (ket0, ket) = [_widened(p) if cx and not p.cplx else (p.AC(0), [p.AR(i) for i in range(1, N)])
                                for p in (psi1, psi2)]
    b = 2 if cx else 1
    rho = be.upload(np.eye(b)).reshape(1, b, b)                    # r_RR(psi2)
    for i in range(N - 2, -1, -1):
        rho = be.transfer_right(None, rho, ket[i], bra[i])         # [Dl ket, Dl bra]
    Dl, d, Dk = ket0.shape
    x = be.gemm(ket0.reshape(Dl * d, Dk), rho.reshape(rho.shape[1], rho.shape[2])).reshape(bra0.shape)
    if not cx:
        return float(be.dot(bra0, x))
    # the overlap of two embeddings: <v, x> = zr + i zi with 2 zr = v_E . x_E, 2 zi = (i v)_E . x_E (excitations.Proj_ddAC)
    return complex(0.5 * be.dot(bra0, x), 0.5 * be.dot(be.times_i(bra0), x))


# ---- interleaved complex states (composed route on the MPSK_C128 entry points) -----------------------------------------------

def _centred(psi, pos):
    """psi with its centre at pos, as a new state on shared tensors (a gauge step replaces list entries, never a tensor)"""
    out = object.__new__(NativeFiniteMPS)
    out.be, out.N, out.center, out.A = psi.be, psi.N, psi.center, list(psi.A)
    out.move_center(pos)
    return out


def _dot_native(psi1, psi2):
    if len(psi1) != len(psi2):
        raise ValueError(f"MPS with different length ({len(psi1)} and {len(psi2)})")
    _check_pair("take the overlap of", psi1, psi2, _phys(psi1), _phys(psi2))
    from .window import _right_step, _eye
    be, N = psi1.be, len(psi1)
    bra, ket = _centred(psi1, 0), _centred(psi2, 0)
    rho = _eye(be, 1, True)
    for i in range(N - 1, 0, -1):
        rho = _right_step(be, True, rho, ket.A[i], bra.A[i])
    Dl, d, Dk = ket.dims(0)
    x = be.gemm_c(ket.A[0].reshape(2 * Dl * d, Dk), rho.reshape(rho.shape[1], rho.shape[2]))
    # conj(a) . x on the interleaved doubles: Re = a . x, Im = (i a) . x
    return complex(be.dot(bra.A[0], x), be.dot(be.times_i(bra.A[0]), x))


def _view(t: DTensor, offset, shape):
    n = int(np.prod(shape))
    return DTensor(t.buf[offset:offset + n], shape)


def _add_native(psi1, psi2):
    """the two half sweeps on gemm_c / qrpos_c / lqpos_c; the result is centred at L//2"""
    _check_pair("add", psi1, psi2, _phys(psi1), _phys(psi2))
    N, be = len(psi1), psi1.be
    if N < 2:
        raise ValueError("add is not implemented for length < 2")
    half = N // 2
    p1, p2 = _centred(psi1, half), _centred(psi2, half)
    cs, ars = [], []
    for p in (p1, p2):                                             # AC(half) = C AR(half)
        Dl, d, Dr = p.dims(half)
        c, q = be.lqpos_c(p.A[half].reshape(2 * Dl, d * Dr))
        cs.append(c)
        ars.append(q.reshape(q.shape[0], d, Dr))
    A = [None] * N
    G = be.upload_c(np.ones((1, 2)))
    for i in range(half):
        (D1, d, E1), (D2, _, E2) = p1.dims(i), p2.dims(i)
        Dn = G.shape[0] // 2
        M = be.empty(2 * Dn, d, E1 + E2)
        be.gemm_c(_view(G, 0, (2 * Dn, D1)), p1.A[i].reshape(2 * D1, d * E1), out=_view(M, 0, (2 * Dn, d * E1)))
        be.gemm_c(_view(G, 2 * Dn * D1, (2 * Dn, D2)), p2.A[i].reshape(2 * D2, d * E2),
                  out=_view(M, 2 * Dn * d * E1, (2 * Dn, d * E2)))
        if Dn * d >= E1 + E2:
            Q, G = be.qrpos_c(M.reshape(2 * Dn * d, E1 + E2))
            A[i] = Q.reshape(2 * Dn, d, Q.shape[1])
        else:
            A[i] = be.upload_c(np.eye(Dn * d).reshape((Dn, d, Dn * d), order="F"))
            G = M.reshape(2 * Dn * d, E1 + E2)
    R = G
    G = be.upload_c(np.ones((2, 1)))
    for i in range(N - 1, half - 1, -1):
        A1, A2 = (ars[0], ars[1]) if i == half else (p1.A[i], p2.A[i])
        (D1, d, E1), (D2, _, E2) = (A1.shape[0] // 2, A1.shape[1], A1.shape[2]), (A2.shape[0] // 2, A2.shape[1], A2.shape[2])
        Et, Dn = G.shape[0] // 2, G.shape[1]
        M = be.empty(2 * (D1 + D2), d, Dn)
        for Ak, D, E, g_off, o_off in ((A1, D1, E1, 0, 0), (A2, D2, E2, E1, D1)):
            Gk = be.empty(2 * E, Dn)
            be.copy2d(2 * E, Dn, G.ptr + 16 * g_off, 2 * Et, Gk.ptr, 2 * E)
            T = be.gemm_c(Ak.reshape(2 * D * d, E), Gk)
            be.copy2d(2 * D, d * Dn, T.ptr, 2 * D, M.ptr + 16 * o_off, 2 * (D1 + D2))
        Dt = D1 + D2
        if Dt <= d * Dn:
            G, Q = be.lqpos_c(M.reshape(2 * Dt, d * Dn))
            A[i] = Q.reshape(Q.shape[0], d, Dn)
        else:
            A[i] = be.upload_c(np.eye(d * Dn).reshape((d * Dn, d, Dn), order="F"))
            G = M.reshape(2 * Dt, d * Dn)
    # centre: R (C1 (+) C2) L, then AC(half) = C AR(half)
    kL, (D1, E1), (D2, E2) = R.shape[0] // 2, (cs[0].shape[0] // 2, cs[0].shape[1]), (cs[1].shape[0] // 2, cs[1].shape[1])
    RC = be.empty(2 * kL, E1 + E2)
    be.gemm_c(_view(R, 0, (2 * kL, D1)), cs[0], out=_view(RC, 0, (2 * kL, E1)))
    be.gemm_c(_view(R, 2 * kL * D1, (2 * kL, D2)), cs[1], out=_view(RC, 2 * kL * E1, (2 * kL, E2)))
    C = be.gemm_c(RC, G)
    _, d, Dr = A[half].shape
    A[half] = be.gemm_c(C, A[half].reshape(A[half].shape[0], d * Dr)).reshape(2 * kL, d, Dr)
    out = object.__new__(NativeFiniteMPS)
    out.be, out.N, out.center, out.A = be, N, half, A
    return out
