"""Local measurements: one-site and multi-site expectation values (src/algorithms/expval.jl:23-61) and two-point
correlators (src/algorithms/correlators.jl:10-43) of FiniteMPS, InfiniteMPS and native_cplx.NativeFiniteMPS.

Operators are NumPy arrays with the bra index first, O[t,s] = <t|O|s>; an N-site operator is O[t1..tN, s1..sN]; an MPO
tensor is [Wl, t, s, Wr].  Results are floats / float64 arrays when the state and the operators are real, complex otherwise.

Two routes.  The device route (backends with `site_gram` and `transfer_left_gram`, include/mpsk.h) takes everything a site
can say about one-site operators from ONE d x d Gram matrix over the physical index:
    rho_i[t,s]      = sum_{p,b} conj(AC_i[p,t,b]) AC_i[p,s,b]                   <O_i> = sum O[t,s] rho_i[t,s]
    gram_j[w][t,s]  = sum V[w][p,a] AR_j[a,s,b] conj(AR_j[p,t,b])               G_j   = sum O2[w,t,s] gram_j[w][t,s]
with V the left vector of the correlator carried by pass-through transfers; gram_j is a by-product of the transfer's own
intermediate.  All Gram matrices of a call go into one device buffer and come back in one download: no host round trip
inside a loop.  Sites of a correlator range that are not asked for take the plain transfer_left.
The composed route (`device=False`, and every backend without the two methods) uses entry points every backend has: the
correlator is closed per site with a transfer through a slice of O2 and a dot with the identity, rho comes from dots of the
d physical planes of AC.
"""
from __future__ import annotations

import numpy as np

from ._lib import MpskError
from .backend import DTensor
from .states import FiniteMPS, InfiniteMPS

__all__ = ["expectation_value", "correlator", "decompose_localmpo"]


# ---- operators -----------------------------------------------------------------------------------------------------

def decompose_localmpo(O, tol=1e-12):
    """N-site operator O[t1..tN, s1..sN] -> list of N MPO tensors [Wl, t, s, Wr] with trivial outer legs, by successive
    SVDs that drop singular values <= tol (utility.jl:42-54, Defaults.tol)."""
    O = np.asarray(O)
    if O.ndim < 2 or O.ndim % 2:
        raise ValueError(f"a local operator has as many bra as ket indices, not shape {O.shape}")
    N = O.ndim // 2
    rest = O.reshape((1,) + O.shape)                         # [Wl, t_1..t_k, s_1..s_k]
    out = []
    for k in range(N, 1, -1):
        Wl, dt, ds = rest.shape[0], rest.shape[1], rest.shape[k + 1]
        perm = (0, 1, k + 1) + tuple(range(2, k + 1)) + tuple(range(k + 2, 2 * k + 1))
        tail = tuple(rest.shape[i] for i in perm[3:])
        U, S, Vh = np.linalg.svd(rest.transpose(perm).reshape(Wl * dt * ds, -1), full_matrices=False)
        r = max(int(np.count_nonzero(S > tol)), 1)
        out.append((U[:, :r] * S[:r]).reshape(Wl, dt, ds, r))
        rest = Vh[:r].reshape((r,) + tail)
    out.append(rest.reshape(rest.shape + (1,)))
    return out


def _is_array_list(O):
    return isinstance(O, (list, tuple)) and len(O) > 0 and all(isinstance(o, np.ndarray) for o in O)


def is_local_operator(O, at):
    """the dispatch rule of algorithms.expectation_value: an ndarray or a list of ndarrays, with an int or no position"""
    return (isinstance(O, np.ndarray) or _is_array_list(O)) and (at is None or isinstance(at, (int, np.integer)))


def _mpo_tensors(O):
    """operator argument of the `at` form -> list of MPO tensors with trivial outer legs"""
    if isinstance(O, np.ndarray):
        return decompose_localmpo(O)
    ts = [np.asarray(o) for o in O]
    if any(t.ndim != 4 or t.shape[1] != t.shape[2] for t in ts):
        raise ValueError("a local MPO is a list of tensors [Wl, d, d, Wr]")
    if ts[0].shape[0] != 1 or ts[-1].shape[3] != 1:
        raise ValueError(f"a local MPO starts and ends in a trivial leg, not {ts[0].shape[0]} and {ts[-1].shape[3]}")
    if any(a.shape[3] != b.shape[0] for a, b in zip(ts, ts[1:])):
        raise ValueError("the bond legs of the local MPO do not match")
    return ts


def _real_chain(ts):
    """complex MPO tensors -> real ones on doubled bonds: a complex number travels as the row (re, im), a tensor w acts as
    [[Re w, Im w], [-Im w, Re w]]; the chain starts from (1, 0) and ends in the two levels (re, im)."""
    out = []
    for k, t in enumerate(ts):
        re, im = t.real, t.imag
        top = np.concatenate([re, im], axis=3)
        out.append(top if k == 0 else np.concatenate([top, np.concatenate([-im, re], axis=3)], axis=0))
    return out


def _as_left_tensor(O1):
    O1 = np.asarray(O1)
    if O1.ndim == 2:
        O1 = O1[None, :, :, None]
    if O1.ndim != 4 or O1.shape[0] != 1 or O1.shape[1] != O1.shape[2]:
        raise ValueError(f"O1 is a [d,d] array or an MPO tensor [1,d,d,W], not {O1.shape}")
    return O1


def _as_right_tensor(O2):
    O2 = np.asarray(O2)
    if O2.ndim == 2:
        O2 = O2[None, :, :, None]
    if O2.ndim != 4 or O2.shape[3] != 1 or O2.shape[1] != O2.shape[2]:
        raise ValueError(f"O2 is a [d,d] array or an MPO tensor [W,d,d,1], not {O2.shape}")
    return O2[:, :, :, 0]


def _js(i, js):
    if isinstance(js, (int, np.integer)):
        js, scalar = [int(js)], True
    else:
        js, scalar = [int(j) for j in js], False
    if not js:
        raise ValueError("correlator: empty js")
    if js[0] <= i or any(b <= a for a, b in zip(js, js[1:])):
        raise ValueError(f"correlator: js must be increasing and start after i = {i}, got {js[:4]}{'...' if len(js) > 4 else ''}")
    return js, scalar


# ---- states ----------------------------------------------------------------------------------------------------------

class _RealView:
    """AC / AR / AL / CR of a real FiniteMPS or InfiniteMPS by site (periodic for the infinite state)"""
    cplx = False

    def __init__(self, psi):
        if getattr(psi, "cplx", False):
            raise NotImplementedError("local measurements on a complex (embedded) state: use a native_cplx.NativeFiniteMPS "
                                      "with native_cplx.expectation_value / native_cplx.correlator")
        self.psi, self.be, self.n = psi, psi.be, len(psi)
        self.finite = isinstance(psi, FiniteMPS)
        if not self.finite and not isinstance(psi, InfiniteMPS):
            raise TypeError(f"local measurements need a FiniteMPS or an InfiniteMPS, not {type(psi).__name__}")

    def _site(self, i, what):
        if self.finite:
            if not 0 <= i < self.n:
                raise ValueError(f"{what}: site {i} outside the chain of {self.n} sites")
            return i
        return i % self.n

    def prepare(self, i):
        self._site(i, "measurement")

    def AC(self, i):
        i = self._site(i, "AC")
        return self.psi.AC(i) if self.finite else self.psi.AC[i]

    def AR(self, i):
        i = self._site(i, "AR")
        return self.psi.AR(i) if self.finite else self.psi.AR[i]

    def AL(self, i):
        i = self._site(i, "AL")
        return self.psi.AL(i) if self.finite else self.psi.AL[i]

    def CR(self, i):
        i = self._site(i, "CR")
        return self.psi.CR(i) if self.finite else self.psi.CR[i]

    def dims(self, A):
        return A.shape

    def identity(self, D):
        return self.be.upload(np.eye(D)).reshape(1, D, D)

    def slice(self, O):
        return self.be.mposlice(1, O.shape[1], [O.shape[0]], [O.shape[3]], {(0, 0): np.ascontiguousarray(O)})

    def transfer(self, H, V, A):
        return self.be.transfer_left(H, V, A, A)

    def host(self, buf):
        return self.be.download(buf)

    def trace(self, G, eye):
        """traces of the slabs of G"""
        n = eye.size
        return np.array([self.be.dot(DTensor(G.buf[w * n:(w + 1) * n], eye.shape), eye) for w in range(G.shape[0])])

    def planes_gram(self, ac):
        """rho[t,s] = sum_{p,b} ac[p,t,b] ac[p,s,b] from dots of the d physical planes (copied out of ac)"""
        be = self.be
        Dl, d, Dr = ac.shape
        planes = []
        for t in range(d):
            pl = be.empty(Dl, Dr)
            be.copy2d(Dl, Dr, ac.ptr + 8 * t * Dl, Dl * d, pl.ptr, Dl)
            planes.append(pl)
        rho = np.zeros((d, d))
        for t in range(d):
            for s in range(t, d):
                rho[t, s] = rho[s, t] = be.dot(planes[t], planes[s])
        return rho


class _NativeView:
    """the same for a native_cplx.NativeFiniteMPS: interleaved complex128 tensors, mixed-canonical around the centre"""
    cplx = True
    finite = True

    def __init__(self, psi):
        self.psi, self.be, self.n = psi, psi.be, len(psi)

    def prepare(self, i):
        if not 0 <= i < self.n:
            raise ValueError(f"site {i} outside the chain of {self.n} sites")
        self.psi.move_center(i)

    def AC(self, i):
        self.prepare(i)
        return self.psi.A[i]

    def AR(self, i):
        if not self.psi.center < i < self.n:
            raise ValueError(f"AR: site {i} is not right of the centre {self.psi.center}")
        return self.psi.A[i]

    def dims(self, A):
        return A.shape[0] // 2, A.shape[1], A.shape[2]

    def identity(self, D):
        return self.be.upload_env_c([np.eye(D, dtype=np.complex128)[:, None, :]])

    def slice(self, O):
        return self.be.mposlice(1, O.shape[1], [O.shape[0]], [O.shape[3]],
                                {(0, 0): np.ascontiguousarray(O, dtype=np.complex128)}, cplx=True)

    def transfer(self, H, V, A):
        return self.be.transfer_left(H, V, A, A, cplx=True)

    def host(self, buf):
        return self.be.download(buf).view(np.complex128)

    def _dotc(self, x, y):
        """conj(x) . y from real inner products of the interleaved vectors: Re = x . y, Im = -(x . (i y))"""
        be = self.be
        return complex(be.dot(x, y), -be.dot(x, be.times_i(y)))

    def trace(self, G, eye):
        n = eye.size
        return np.array([self._dotc(eye, DTensor(G.buf[w * n:(w + 1) * n], eye.shape)) for w in range(G.shape[0])])

    def planes_gram(self, ac):
        be = self.be
        Dl, d, Dr = self.dims(ac)
        planes = []
        for t in range(d):
            pl = be.empty(2 * Dl, Dr)
            be.copy2d(2 * Dl, Dr, ac.ptr + 16 * t * Dl, 2 * Dl * d, pl.ptr, 2 * Dl)
            planes.append(pl)
        rho = np.zeros((d, d), dtype=np.complex128)
        for t in range(d):
            for s in range(t, d):
                rho[t, s] = self._dotc(planes[t], planes[s])
                rho[s, t] = np.conj(rho[t, s])
        return rho


def _view(psi):
    from .native_cplx import NativeFiniteMPS
    return _NativeView(psi) if isinstance(psi, NativeFiniteMPS) else _RealView(psi)


def _device_route(be, device):
    has = hasattr(be, "site_gram") and hasattr(be, "transfer_left_gram")
    if device and not has:
        raise MpskError("device=True: this backend has no site_gram / transfer_left_gram")
    return has if device is None else bool(device)


# ---- expectation values ------------------------------------------------------------------------------------------------

def _expval_onesite(v, O, device):
    n = v.n
    ops = [np.asarray(O)] * n if isinstance(O, np.ndarray) else [np.asarray(o) for o in O]
    if len(ops) != n:
        raise ValueError(f"one operator per site: {len(ops)} operators for {n} sites")
    be, c = v.be, 2 if v.cplx else 1
    acs, rhos = [], []
    if not v.cplx:                                         # (a native state holds one AC at a time: taken inside the loops)
        acs = [v.AC(i) for i in range(n)]
    ds = [v.dims(a)[1] for a in acs] if acs else [v.dims(a)[1] for a in v.psi.A]
    for i, (o, d) in enumerate(zip(ops, ds)):
        if o.shape != (d, d):
            raise ValueError(f"site {i}: operator of shape {o.shape} on a physical dimension {d}")
    if _device_route(be, device):
        offs = np.concatenate([[0], np.cumsum([c * d * d for d in ds])]).astype(int)
        buf = be.empty(int(offs[-1]))
        for i in range(n):
            ac = acs[i] if acs else v.AC(i)
            be.site_gram(ac, ac, out=DTensor(buf.buf[offs[i]:offs[i + 1]], (1, c * ds[i], ds[i])), cplx=v.cplx)
        flat = v.host(buf)                                 # the one download
        rhos = [flat[offs[i] // c:offs[i + 1] // c].reshape((ds[i], ds[i]), order="F") for i in range(n)]
    else:
        rhos = [v.planes_gram(acs[i] if acs else v.AC(i)) for i in range(n)]
    vals = np.array([np.sum(o * r) for o, r in zip(ops, rhos)])
    if not v.cplx and not any(np.iscomplexobj(o) for o in ops):
        return vals.real.astype(np.float64)
    return vals.astype(np.complex128)


def _expval_at(v, O, at):
    if v.cplx:
        raise NotImplementedError("multi-site expectation values of a NativeFiniteMPS: use correlator for two sites")
    ts = _mpo_tensors(O)
    cx = any(np.iscomplexobj(t) for t in ts)
    if cx:
        ts = _real_chain(ts)
    be, at = v.be, int(at)
    if v.finite and not (0 <= at and at + len(ts) <= v.n):
        raise ValueError(f"a {len(ts)}-site operator at {at} does not fit a chain of {v.n} sites")
    V = v.identity(v.AL(at).shape[0])
    for k, t in enumerate(ts):
        A = v.AL(at + k)
        if t.shape[1] != A.shape[1]:
            raise ValueError(f"site {at + k}: operator of physical dimension {t.shape[1]} on {A.shape[1]}")
        V = v.transfer(v.slice(t), V, A)
    C = v.CR(at + len(ts) - 1)
    r = be.gemm(C, C, transB=True)                          # closed with r = C C^dag (symmetric): sum V[q,b] r[b,q]
    n = r.size
    vals = [be.dot(DTensor(V.buf[w * n:(w + 1) * n], r.shape), r) for w in range(V.shape[0])]
    return complex(vals[0], vals[1]) if cx else float(vals[0])


def expectation_value(psi, O, at=None, device=None):
    """expectation_value(psi, O): <O_i> for every site, O one [d,d] array or a list of one per site (expval.jl:23-37).
    expectation_value(psi, O, at): an N-site operator O[t1..tN, s1..sN], or a list of MPO tensors with trivial outer legs,
    with its first site at `at` (expval.jl:42-61): transfers through the AL tensors, closed with CR.
    device: None = the fused route when the backend has it, False = the composed route, True = insist on the fused one."""
    v = _view(psi)
    if at is None:
        return _expval_onesite(v, O, device)
    return _expval_at(v, O, at)


# ---- correlators -------------------------------------------------------------------------------------------------------

def correlator(psi, O1, O2, i=None, js=None, device=None):
    """correlator(psi, O1, O2, i, js) = [<O1_i O2_j> for j in js]  (correlators.jl:14-38); correlator(psi, O12, i, js) with a
    two-site operator O12[t1,t2,s1,s2] splits it first (:40-43).  O1 / O2 are [d,d] arrays or MPO tensors [1,d,d,W] /
    [W,d,d,1].  js: an int (a scalar comes back) or an increasing iterable with js[0] > i; an InfiniteMPS takes any j."""
    from . import window
    if isinstance(psi, window.WindowMPS):
        return window.correlator(psi, O1, O2, i, js, device=device)
    if js is None:                                         # correlator(psi, O12, i, js)
        O12, i, js = np.asarray(O1), O2, i
        if O12.ndim != 4 or i is None or js is None:
            raise TypeError("correlator(psi, O1, O2, i, js) or correlator(psi, O12, i, js) with O12[t1,t2,s1,s2]")
        O1, O2 = decompose_localmpo(O12)
    if not isinstance(i, (int, np.integer)):
        raise TypeError(f"correlator: i must be an int, not {type(i).__name__}")
    i = int(i)
    js, scalar = _js(i, js)
    v = _view(psi)
    be = v.be
    O1, O2 = _as_left_tensor(O1), _as_right_tensor(O2)
    W = O1.shape[3]
    if O2.shape[0] != W or O2.shape[1] != O1.shape[1]:
        raise ValueError(f"O1 {O1.shape} and O2 {O2.shape + (1,)} do not match")
    if v.finite and js[-1] >= v.n:
        raise ValueError(f"correlator: site {js[-1]} outside the chain of {v.n} sites")
    v.prepare(i)
    ac = v.AC(i)
    d = v.dims(ac)[1]
    if d != O1.shape[1]:
        raise ValueError(f"operators of physical dimension {O1.shape[1]} on a site of dimension {d}")
    # a complex O1 on a real state: Re and Im as 2W real slabs, combined on the host; the state stays real
    split = not v.cplx and np.iscomplexobj(O1)
    O1d = np.concatenate([O1.real, O1.imag], axis=3) if split else (O1 if v.cplx else O1.real)
    Wt = O1d.shape[3]
    V = v.transfer(v.slice(O1d), v.identity(v.dims(ac)[0]), ac)      # V[w][q,b] = sum AC[a,s,b] O1[t,s,w] conj(AC[a,t,q])
    want = set(js)
    c = 2 if v.cplx else 1
    real_out = not v.cplx and not split and not np.iscomplexobj(O2)
    if _device_route(be, device):
        g = Wt * c * d * d
        buf = be.empty(len(js) * g)
        k = 0
        for j in range(i + 1, js[-1] + 1):
            A = v.AR(j)
            if v.dims(A)[1] != d:
                raise ValueError(f"site {j} has physical dimension {v.dims(A)[1]}, the operators {d}")
            if j in want:
                V = be.transfer_left_gram(V, A, A, DTensor(buf.buf[k * g:(k + 1) * g], (Wt, c * d, d)), last=j == js[-1],
                                          cplx=v.cplx)
                k += 1
            else:
                V = v.transfer(None, V, A)
        gram = v.host(buf).reshape(len(js), Wt, d, d).transpose(0, 1, 3, 2)     # the one download; [k, w, t, s]
        if split:
            gram = gram[:, :W] + 1j * gram[:, W:]
        G = np.einsum("wts,kwts->k", O2, gram)
    else:
        # the closing slice: levels (re, im) of sum_w O2[w] (V[w] + i V[W + w])
        if v.cplx:
            close = O2[:, :, :, None]
        elif real_out:
            close = O2.real[:, :, :, None]
        else:
            re, im = O2.real[:, :, :, None], O2.imag[:, :, :, None]
            close = np.concatenate([re, im], axis=3)
            if split:
                close = np.concatenate([close, np.concatenate([-im, re], axis=3)], axis=0)
        H2 = v.slice(close)
        G = np.zeros(len(js), dtype=np.complex128)
        k = 0
        eye = None
        for j in range(i + 1, js[-1] + 1):
            A = v.AR(j)
            if v.dims(A)[1] != d:
                raise ValueError(f"site {j} has physical dimension {v.dims(A)[1]}, the operators {d}")
            if j in want:
                Dr = v.dims(A)[2]
                if eye is None or eye.shape[-1] != Dr:
                    eye = v.identity(Dr)
                    eye = eye.reshape(eye.shape[1], eye.shape[2])
                tr = v.trace(v.transfer(H2, V, A), eye)
                G[k] = tr[0] if len(tr) == 1 else complex(tr[0].real, tr[1].real)
                k += 1
            if j < js[-1]:
                V = v.transfer(None, V, A)
    G = G.real.astype(np.float64) if real_out else G.astype(np.complex128)
    return (float(G[0]) if real_out else complex(G[0])) if scalar else G
