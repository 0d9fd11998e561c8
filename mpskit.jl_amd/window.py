"""WindowMPS (src/states/windowmps.jl): a finite window of L tensors between the fixed infinite environments of one or two
uniform states -- the state type of local quenches and dynamical correlation functions in the thermodynamic limit.

The window is a FiniteMPS (real tensors) or a native_cplx.NativeFiniteMPS (interleaved complex128 tensors) whose outer
bonds carry the bond dimension of the uniform states; the uniform parts are never modified.  The environments of a window
(`environments(window, H)`, FinEnv.jl:84-89) are finite environments that START from copies of the infinite fixed points:
level 0 of the left one and level W-1 of the right one are identities and AL / AR of the window are isometries, so a real
window keeps the canonical promise behind the Jordan-form routes (mpsk_hac mode 3, MPSK_TRANSFER_CANONICAL) -- WindowEnv
checks the two identities once, on the host, and keeps the dense route when they do not hold.

The finite drivers take a WindowMPS by delegation to its window: find_groundstate (DMRG / DMRG2), timestep / time_evolve
(TDVP / TDVP2), changebonds, approximate, entropy, entanglement_spectrum, calc_galerkin, local expectation_value /
correlator.  Two-site updates and bond changes only ever split the L - 1 inner bonds: the outer bonds stay those of the
environments.  propagator on a window is not built.  On a complex window the drivers are find_groundstate, timestep /
time_evolve, expectation_value, variance, correlator, dot and transition; the AL / AR / AC / CR views, calc_galerkin,
changebonds, approximate, entropy and entanglement_spectrum are for real windows and raise NotImplementedError otherwise.

Overlaps of two windows on the same environments: dot(w1, w2) and transition(bra, ket, O) = [<bra| O_j |ket>]_j.  With
both states left-canonical up to their last bond matrices C, Cb, the site matrices are
    M_j[t,s] = sum conj(ALb_j[p,t,q]) L_j[p,a] AL_j[a,s,b] R_j[b,q],      R_{L-1} = C Cb^dag,
    R_{j-1}[a,p] = sum AL_j[a,s,b] R_j[b,q] conj(ALb_j[p,s,q])            (one right-to-left sweep, stored),
    L_{j+1}[q,b] = sum conj(ALb_j[p,t,q]) L_j[p,a] AL_j[a,t,b]            (carried left to right),
which is  sum conj(ACb_j) L_j AC_j R'_j  with the right-canonical R' of the AR tensors, by AC_j = AL_j C_j = C_{j-1} AR_j.
Written this way the transfer that mpsk_transfer_left_gram_env returns IS the next L: one call per site gives M_j and
L_{j+1} from one shared stage-1 product, and the product with R_j never reaches memory.
"""
from __future__ import annotations

import numpy as np

from ._lib import MpskError
from .backend import DTensor
from .environments import FinEnv, MultipleEnvironments, MPOHamInfEnv, environments as _environments
from .states import FiniteMPS, InfiniteMPS
from . import native_cplx
from .native_cplx import NativeFiniteMPS, NativeFinEnv

__all__ = ["WindowMPS", "WindowEnv", "NativeWindowEnv", "environments", "dot", "transition", "FUSED_BY_DEFAULT"]

# transition() with device=None picks the route per dtype from the measured table (tools/bench_window.py,
# profiles/window_timings.json, README): the fused closing product is 4 to 9 % faster than the composed route for real
# tensors at D = 256 and D = 1024, and slower for complex ones at both sizes (0.55x / 0.92x), so complex windows take the
# composed route unless device=True asks for the fused one.  The real-tensor margin at D = 1024 (4 %, one run of 9-window
# medians) is of the size of run-to-run spread: the real default is "not slower", not a measured gain.  Only these two
# sizes were measured, so the switch is per dtype, not per size.
FUSED_BY_DEFAULT = {"f64": True, "c128": False}


def _native(psi):
    return isinstance(psi, NativeFiniteMPS)


def _edges(window):
    """(left, right) outer bond dimensions of a window state"""
    if _native(window):
        return window.dims(0)[0], window.dims(len(window) - 1)[2]
    L = len(window)
    t = window.ARs[L - 1] if window.ARs[L - 1] is not None else window.AL(L - 1)
    return window.AL(0).shape[0], t.shape[2]


class WindowMPS:
    """WindowMPS(left_gs, window[, right_gs]) / WindowMPS(psi_inf, L)  (windowmps.jl:39-111)."""

    def __init__(self, left_gs, window, right_gs=None):
        if not isinstance(left_gs, InfiniteMPS):
            raise TypeError(f"the environment of a window is an InfiniteMPS, not {type(left_gs).__name__}")
        right_gs = left_gs if right_gs is None else right_gs          # the same object, not a copy (windowmps.jl:57-60)
        if not isinstance(right_gs, InfiniteMPS):
            raise TypeError(f"the environment of a window is an InfiniteMPS, not {type(right_gs).__name__}")
        if getattr(left_gs, "cplx", False) or getattr(right_gs, "cplx", False):
            raise NotImplementedError("windows in complex (embedded) uniform states are not implemented")
        be = left_gs.be
        if isinstance(window, (int, np.integer)):                     # WindowMPS(psi, L): promote L sites (windowmps.jl:99-111)
            window = self._promote(left_gs, int(window))
        elif isinstance(window, (list, tuple)):
            arrs = [np.asarray(a) for a in window]
            if any(np.iscomplexobj(a) for a in arrs):
                window = NativeFiniteMPS(arrs, be, normalize=False)
            else:
                window = FiniteMPS(arrs, be=be)
        if isinstance(window, FiniteMPS) and window.cplx:
            raise NotImplementedError("an embedded-complex (cplx.py) window: use a native_cplx.NativeFiniteMPS")
        if not isinstance(window, (FiniteMPS, NativeFiniteMPS)):
            raise TypeError(f"a window is a FiniteMPS, a NativeFiniteMPS or a list of arrays, not {type(window).__name__}")
        Dl, Dr = _edges(window)
        nl, nr, L = len(left_gs), len(right_gs), len(window)
        if Dl != left_gs.AL[0].shape[0] or Dr != right_gs.AR[(L - 1) % nr].shape[2]:
            raise ValueError(f"the outer bonds of the window ({Dl}, {Dr}) do not match those of the environments "
                             f"({left_gs.AL[0].shape[0]}, {right_gs.AR[(L - 1) % nr].shape[2]})")
        self.left_gs, self.window, self.right_gs, self.be = left_gs, window, right_gs, be

    @staticmethod
    def _promote(psi, L):
        n = len(psi)
        return FiniteMPS.from_canonical([psi.AL[i % n] for i in range(L)], [psi.AR[i % n] for i in range(L)],
                                        [psi.AC[i % n] for i in range(L)], [psi.CR[(i - 1) % n] for i in range(L + 1)], psi.be)

    @classmethod
    def random(cls, L, d, D, left_gs, right_gs=None, rng=None, dtype=None):
        """FiniteMPS.random with the outer bonds fixed by the environments: bond dimensions min(Dl d^i, D, d^(L-i) Dr)."""
        rng = np.random.default_rng(0) if rng is None else rng
        rgs = left_gs if right_gs is None else right_gs
        dims = [left_gs.AL[0].shape[0]]
        for _ in range(1, L):
            dims.append(min(dims[-1] * d, D))
        dims.append(rgs.AR[(L - 1) % len(rgs)].shape[2])
        for k in range(L - 1, 0, -1):
            dims[k] = min(dims[k], dims[k + 1] * d)
        cx = dtype is not None and np.issubdtype(dtype, np.complexfloating)
        As = [rng.random((dims[i], d, dims[i + 1])) + (1j * rng.random((dims[i], d, dims[i + 1])) if cx else 0.0)
              for i in range(L)]
        out = cls(left_gs, As, right_gs)
        return out.normalize()

    # ---- the window's views (orthoview.jl:11,33,81,145-149) ----
    @property
    def cplx(self):
        return _native(self.window)

    def __len__(self):
        return len(self.window)

    def _real(self, what):
        if _native(self.window):
            raise NotImplementedError(f"{what} of a complex window: its NativeFiniteMPS keeps one centre (window.window)")
        return self.window

    def AL(self, i):
        return self._real("AL").AL(i)

    def AR(self, i):
        return self._real("AR").AR(i)

    def AC(self, i):
        return self._real("AC").AC(i)

    def CR(self, i):
        return self._real("CR").CR(i)

    def set_AC(self, i, vec):
        self._real("set_AC").set_AC(i, vec)

    def set_CR(self, i, vec):
        self._real("set_CR").set_CR(i, vec)

    def copy(self):
        return WindowMPS(self.left_gs, self.window.copy(), self.right_gs)

    def with_window(self, window):
        return WindowMPS(self.left_gs, window, self.right_gs)

    def norm(self):
        return self.window.norm()

    def normalize(self):
        self.__imul__(1.0 / self.norm())
        return self

    def __imul__(self, a):
        w, be = self.window, self.be
        a = complex(a)
        if _native(w):
            t = w.A[w.center]
            if a.imag != 0.0:                        # (re + i im) t on the interleaved tensor
                be.axpby(a.imag, be.times_i(t), a.real, t)
            else:
                be.scal(a.real, t)
        else:
            if a.imag != 0.0:
                raise TypeError("a real window times a complex number: build the window from complex tensors")
            ac = be.copy(w.AC(len(w) - 1))
            be.scal(a.real, ac)
            w.set_AC(len(w) - 1, ac)
        return self

    def __mul__(self, a):
        out = self.copy()                            # (a scaled FiniteMPS gets a new AC: the shared tensors stay as they are)
        out *= a
        return out

    __rmul__ = __mul__

    def max_Ds(self):
        w = self.window
        return max([w.dims(i)[2] for i in range(len(w))] + [w.dims(0)[0]]) if _native(w) else max(w.bond_dims() + [_edges(w)[0]])

    def l_LL(self):
        """left fixed point of the transfer matrix of left_gs.AL at the window's left edge: the identity"""
        return self.be.upload(np.eye(_edges(self.window)[0]))

    def r_RR(self):
        return self.be.upload(np.eye(_edges(self.window)[1]))

    def to_host(self):
        return self.window.to_host()


# ---- environments ----------------------------------------------------------------------------------------------------------

def _is_identity(be, env, level, tol=1e-10):
    W, D1, D2 = env.shape
    n = D1 * D2
    h = be.download(DTensor(env.buf[level * n:(level + 1) * n], (D1, D2)))
    return D1 == D2 and float(np.abs(h - np.eye(D1)).max()) <= tol


class WindowEnv(FinEnv):
    """FinEnv of a real window: the start environments are copies of the infinite fixed points (FinEnv.jl:84-89).  The
    canonical routes are taken when the two start identities were found to hold (once, at construction)."""

    def __init__(self, window, H, GL0, GRL):
        be, L = window.be, len(window)
        super().__init__(window, H, leftstart=be.copy(GL0), rightstart=be.copy(GRL))
        self.window_canonical = _is_identity(be, self.leftenvs[0], 0) and _is_identity(be, self.rightenvs[L], GRL.shape[0] - 1)

    def _canonical(self, psi):
        return (self.canonical and self.window_canonical and not getattr(psi, "cplx", False)
                and hasattr(self.be, "transfer_left_ex"))


class NativeWindowEnv(NativeFinEnv):
    """NativeFinEnv of an interleaved complex window on real infinite environments: the edge slabs are widened to complex
    once, here."""

    def __init__(self, window, H, GL0, GRL):
        from .cplx import HalfEmbeddedOp
        be = self.be = window.be
        L = self.L = len(window)
        if window.center != 0:
            raise ValueError("the environments of a complex window are built with its centre at site 0")
        self.H = H
        self.opp = [HalfEmbeddedOp._cslice(be, H[i]) for i in range(L)]
        to_host = be.download_env if hasattr(be, "download_env") else be._env
        widen = lambda t, chis: be.upload_env_c(to_host(t, chis))
        self.GL = [widen(GL0, H[0].chil)] + [None] * L
        self.GR = [None] * L + [widen(GRL, H[L - 1].chir)]
        self.n_transfers = 0
        for j in range(L - 1, 0, -1):
            self.extend_right(window, j)


class _OverlapEnv:
    """environments(below_window, above_window) (FinEnv.jl:91-99): the l_LL / r_RR starts of a plain overlap"""

    def __init__(self, below, above):
        _same_environments(below, above)
        self.below, self.above = below, above
        self.leftstart, self.rightstart = below.l_LL(), below.r_RR()


def environments(state, H, lenvs=None, renvs=None):
    """environments(window, H[, lenvs, renvs]) (FinEnv.jl:84-89); environments(below_window, above_window) (:91-99)."""
    from .operators import LazySum, MultipliedOperator, MPOHamiltonian
    if isinstance(H, WindowMPS):
        return _OverlapEnv(state, H)
    if isinstance(H, MultipliedOperator):
        return environments(state, H.op, lenvs, renvs)
    if isinstance(H, LazySum):
        les = lenvs.envs if isinstance(lenvs, MultipleEnvironments) else [lenvs] * len(list(H))
        res = renvs.envs if isinstance(renvs, MultipleEnvironments) else [renvs] * len(list(H))
        if _native(state.window):
            raise NotImplementedError("a LazySum on a complex window")
        return MultipleEnvironments(H, [environments(state, h, le, re) for h, le, re in zip(H, les, res)])
    if not isinstance(H, MPOHamiltonian):
        raise TypeError(f"the environments of a window take an MPOHamiltonian, not {type(H).__name__}")
    L = len(state)
    lenvs = _environments(state.left_gs, H) if lenvs is None else lenvs
    if renvs is None:
        renvs = lenvs if state.right_gs is state.left_gs else _environments(state.right_gs, H)
    if type(lenvs) is not MPOHamInfEnv or type(renvs) is not MPOHamInfEnv:      # not its interleaved subclass either
        raise TypeError("lenvs / renvs are the MPOHamInfEnv of the uniform states")
    GL0 = lenvs.leftenv(0, state.left_gs)
    GRL = renvs.rightenv(L - 1, state.right_gs)
    cls = NativeWindowEnv if _native(state.window) else WindowEnv
    return cls(state.window, H, GL0, GRL)


# ---- drivers: delegation to the window --------------------------------------------------------------------------------------

def find_groundstate(state, H, alg=None, envs=None, **kw):
    from . import algorithms
    envs = environments(state, H) if envs is None else envs
    if _native(state.window):
        alg = algorithms.DMRG() if alg is None else alg
        psi, envs, eps = native_cplx.find_groundstate(state.window.copy(), H, alg, envs)
    else:
        psi, envs, eps = algorithms.find_groundstate(state.window, H, alg, envs, **kw)
    return state.with_window(psi), envs, eps


def timestep(state, H, t, dt, alg=None, envs=None):
    from . import algorithms
    envs = environments(state, H) if envs is None else envs
    alg = algorithms.TDVP() if alg is None else alg
    if _native(state.window):
        psi, envs = native_cplx.timestep(state.window.copy(), H, t, dt, alg, envs)
    else:
        psi, envs = algorithms.timestep(state.window, H, t, dt, alg, envs)
    return state.with_window(psi), envs


def changebonds(state, H=None, alg=None, envs=None, rng=None):
    from .changebonds import OptimalExpand, SvdCut, RandExpand, changebonds as _changebonds
    w = state._real("changebonds")
    if isinstance(H, (OptimalExpand, SvdCut, RandExpand)) and alg is None:
        H, alg = None, H
    if isinstance(alg, OptimalExpand) and envs is None:
        envs = environments(state, H)
    edges = _edges(w)
    out = _changebonds(w, H, alg, envs, rng)
    psi = out[0] if isinstance(out, tuple) else out
    if _edges(psi) != edges:
        raise MpskError("changebonds changed an outer bond of the window")
    new = state.with_window(psi)
    return (new, out[1]) if isinstance(out, tuple) else new


def approximate(state, toapprox, alg, envs=None):
    """approximate(window, (O, above_window) | above_window, alg): on the windows, with the trivial edge of equal outer bonds"""
    from .approximate import approximate as _approx
    w = state._real("approximate")

    def unwrap(sq):
        if isinstance(sq, tuple):
            _same_environments(state, sq[1])
            return (sq[0], sq[1]._real("approximate"))
        _same_environments(state, sq)
        return sq._real("approximate")
    ta = [unwrap(s) for s in toapprox] if isinstance(toapprox, list) else unwrap(toapprox)
    psi, envs, eps = _approx(w, ta, alg, envs)
    return state.with_window(psi), envs, eps


def calc_galerkin(state, pos, envs):
    from . import algorithms
    return algorithms.calc_galerkin(state._real("calc_galerkin"), pos, envs)


def _native_site_energies(psi, H, envs):
    """per-site energies of expval.jl:92-109 for an interleaved window: the centre walks a copy from 0 to L - 1"""
    from .cplx import HalfEmbeddedOp
    be, L = psi.be, len(psi)
    psi = psi.copy()
    psi.move_center(0)
    GL = envs.GL[0]
    ens = np.zeros(L)
    for i in range(L):
        ac = psi.A[i]
        y = be.hac_create(HalfEmbeddedOp._cslice(be, H.energy_slice(i)), GL, envs.GR[i + 1]).apply(ac)
        ens[i] = be.dot(ac, y) / be.dot(ac, ac)
        if i < L - 1:
            psi._shift_right(i)
            GL = be.transfer_left(envs.opp[i], GL, psi.A[i], psi.A[i])
    return ens


def expectation_value(state, H, envs=None, *, device=None):
    """local operators: expectation_value(window, O[, at]) as for a finite chain.  A Hamiltonian: (vals, tot) as
    expval.jl:76-87 -- vals the per-site energies, tot = <AC| H_AC |AC> / |AC|^2 over all MPO blocks."""
    from . import algorithms, measure
    from .derivatives import ddAC
    w = state.window
    if measure.is_local_operator(H, envs):
        return native_cplx.expectation_value(w, H, device=device) if _native(w) else \
            measure.expectation_value(w, H, envs, device=device)
    envs = environments(state, H) if envs is None else envs
    if _native(w):
        if w.center != 0:
            raise ValueError("a complex window is kept with its centre at site 0")
        return _native_site_energies(w, H, envs), float(native_cplx.energy(w, envs))
    vals = algorithms.expectation_value(w, H, envs)
    be, L = w.be, len(w)
    ac = w.AC(L - 1)
    tot = be.dot(ac, ddAC(L - 1, w, H, envs)(ac)) / be.dot(ac, ac)
    return vals, float(tot)


def variance(state, H, envs=None):
    """variance(window, H[, envs]) (toolbox.jl:147-152): tot of H^2 on the squared environments minus tot of H squared.
    The squared edge environments of corvector.jl:156-192 are the products GL[i]^dag GL[j] and GR[i] GR[j]^dag of the window
    environments of H, so <AC| (H^2)_AC |AC> on them is |H_AC AC|^2: the squared operator is not built, and
        variance = |H_AC AC|^2 / |AC|^2 - (<AC| H_AC |AC> / |AC|^2)^2
    at the site where expectation_value takes tot.  It vanishes when AC is an eigenvector of H_AC."""
    from .derivatives import ddAC
    envs = environments(state, H) if envs is None else envs
    w = state.window
    be = w.be
    if _native(w):
        if w.center != 0:
            raise ValueError("a complex window is kept with its centre at site 0")
        L = len(w)                                   # the centre walks a copy to the last site, as tot of the reference
        psi, GL = w.copy(), envs.GL[0]
        for i in range(L - 1):
            psi._shift_right(i)
            GL = be.transfer_left(envs.opp[i], GL, psi.A[i], psi.A[i])
        ac = psi.A[L - 1]
        y = be.hac_create(envs.opp[L - 1], GL, envs.GR[L]).apply(ac)
    else:
        ac = w.AC(len(w) - 1)
        y = ddAC(len(w) - 1, w, H, envs)(ac)
    n2 = be.dot(ac, ac)
    return float(be.dot(y, y) / n2 - (be.dot(ac, y) / n2) ** 2)


def correlator(state, *a, **kw):
    from . import measure
    w = state.window
    return native_cplx.correlator(w, *a, **kw) if _native(w) else measure.correlator(w, *a, **kw)


# ---- overlaps ---------------------------------------------------------------------------------------------------------------

def _same_environments(a, b):
    """windowmps.jl:165-176: the same objects, or uniform states whose overlap is 1 to 1e-8"""
    from .statmech import dot as _dot_inf
    if not isinstance(a, WindowMPS) or not isinstance(b, WindowMPS):
        raise TypeError("two WindowMPS are needed")
    if len(a) != len(b):
        raise ValueError(f"the windows have different lengths ({len(a)} != {len(b)})")
    for x, y, side in ((a.left_gs, b.left_gs, "left"), (a.right_gs, b.right_gs, "right")):
        if x is y:
            continue
        if len(x) != len(y) or x.AL[0].shape != y.AL[0].shape or abs(_dot_inf(x, y) - 1.0) > 1e-8:
            raise ValueError(f"the {side} environments of the two windows differ")


class _Left:
    """left-canonical form of a window as device tensors of one dtype: AL_0 .. AL_{L-1} and the last bond matrix C"""

    def __init__(self, state, cx):
        be = self.be = state.be
        w = state.window
        L = len(w)
        if _native(w):
            psi = w.copy()
            psi.move_center(L - 1)
            Dl, d, Dr = psi.dims(L - 1)
            Q, R = be.qrpos_c(psi.A[L - 1].reshape(2 * Dl * d, Dr))
            self.AL = psi.A[:L - 1] + [Q.reshape(2 * Dl, d, R.shape[1])]
            self.C = R
        else:
            AL, C = [w.AL(i) for i in range(L)], w.CR(L - 1)
            if cx:                                          # a real state next to a complex one: widened once
                AL = [be.upload_c(be.download(t)) for t in AL]
                C = be.upload_c(be.download(C))
            self.AL, self.C = AL, C
        c = 2 if cx else 1
        self.dims = [(t.shape[0] // c, t.shape[1], t.shape[2]) for t in self.AL]


def _overlap_sweeps(bra, ket):
    """(cx, b, k, R list) with R[j] [Dr_j, Drb_j] (shape (1, c Dr, Drb)) the closing matrix of site j"""
    _same_environments(bra, ket)
    be = ket.be
    cx = _native(bra.window) or _native(ket.window)
    if cx and not hasattr(be, "upload_c"):
        raise MpskError("complex windows need a backend with the MPSK_C128 entry points")
    b, k = _Left(bra, cx), _Left(ket, cx)
    L = len(ket)
    mm = be.gemm_c if cx else be.gemm
    R = [None] * L
    r = mm(k.C, b.C, transB=True)                            # C Cb^dag
    R[L - 1] = r.reshape(1, *r.shape)
    for j in range(L - 1, 0, -1):
        R[j - 1] = _right_step(be, cx, R[j], k.AL[j], b.AL[j])
    return cx, b, k, R


def _right_step(be, cx, R, A, Ab):
    """sum A[a,s,b] R[b,q] conj(Ab[p,s,q]) as (A R) Ab^dag: the two products of a pass-through right transfer"""
    c = 2 if cx else 1
    mm = be.gemm_c if cx else be.gemm
    Dl, d, Dr = A.shape[0] // c, A.shape[1], A.shape[2]
    Dlb, Drb = Ab.shape[0] // c, Ab.shape[2]
    X = mm(A.reshape(c * Dl * d, Dr), R.reshape(c * Dr, Drb))
    out = mm(X.reshape(c * Dl, d * Drb), Ab.reshape(c * Dlb, d * Drb), transB=True)
    return out.reshape(1, c * Dl, Dlb)


def _eye(be, D, cx):
    e = np.eye(D)
    return be.upload_env_c([e[:, None, :]]) if cx else be.upload(e).reshape(1, D, D)


def _use_fused(be, device, d, cx):
    has = hasattr(be, "transfer_left_gram_env") and hasattr(be, "site_gram")
    if device and not has:
        raise MpskError("device=True: this backend has no transfer_left_gram_env")
    if device is None:
        return has and d <= 64 and FUSED_BY_DEFAULT["c128" if cx else "f64"]
    return bool(device)


def _site_matrices(bra, ket, device=None):
    """the L matrices M_j[t,s] (host, complex when either state is)"""
    cx, b, k, R = _overlap_sweeps(bra, ket)
    be, L = ket.be, len(ket)
    c = 2 if cx else 1
    kw = {"cplx": True} if cx else {}
    mm = be.gemm_c if cx else be.gemm
    ds = [dm[1] for dm in k.dims]
    if any(db[1] != dk for db, dk in zip(b.dims, ds)):
        raise ValueError("the physical dimensions of the two windows differ")
    Lm = _eye(be, k.dims[0][0], cx)
    Ms = []
    has_gram = hasattr(be, "site_gram")
    offs = np.concatenate([[0], np.cumsum([c * d * d for d in ds])]).astype(int)
    buf = be.empty(int(offs[-1])) if has_gram else None
    for j in range(L):
        A, Ab = k.AL[j], b.AL[j]
        (Dl, d, Dr), (Dlb, _, Drb) = k.dims[j], b.dims[j]
        last = j == L - 1
        gram = None if buf is None else DTensor(buf.buf[offs[j]:offs[j + 1]], (c * d, d))
        if has_gram and _use_fused(be, device, d, cx):
            Lm = be.transfer_left_gram_env(Lm.reshape(c * Dlb, Dl), A, Ab, R[j].reshape(c * Dr, Drb), gram, last=last, **kw)
            continue
        # composed route: X = (L A) R materialised, then the site Gram (or, without it, d^2 dots on the host side)
        T1 = mm(Lm.reshape(c * Dlb, Dl), A.reshape(c * Dl, d * Dr))                     # [Dlb, (s, b)]
        X = mm(T1.reshape(c * Dlb * d, Dr), R[j].reshape(c * Dr, Drb)).reshape(c * Dlb, d, Drb)
        if has_gram:
            be.site_gram(X, Ab, out=DTensor(gram.buf, (1, c * d, d)), **kw)
        else:
            xh = be.download_c(X) if cx else be.download(X)
            ah = be.download_c(Ab) if cx else be.download(Ab)
            Ms.append(np.einsum("ptq,psq->ts", np.conj(ah), xh))
        if not last:                                        # L_{j+1} = Ab^dag T1, the second product of the pass-through transfer
            Lm = mm(Ab.reshape(c * Dlb * d, Drb), T1.reshape(c * Dlb * d, Dr), transA=True).reshape(1, c * Drb, Dr)
    if has_gram:
        flat = be.download(buf)
        flat = flat.view(np.complex128) if cx else flat
        Ms = [flat[offs[j] // c:offs[j + 1] // c].reshape((ds[j], ds[j]), order="F") for j in range(L)]
    return Ms


def transition(bra, ket, O=None, device=None):
    """[<bra| O_j |ket>]_j for a one-site operator O[t,s] or a list of one per site; O=None: the L matrices M_j[t,s]
    themselves (<bra| O_j |ket> = sum O[t,s] M_j[t,s]).  bra and ket: windows on the same environments, of any bond
    dimensions; a real one is widened when the other is complex.  device: None = the faster route by the
    measured table (FUSED_BY_DEFAULT: fused for real tensors, composed for complex ones), False = the composed route (gemm +
    site Gram), True = insist on the fused closing product."""
    Ms = _site_matrices(bra, ket, device)
    if O is None:
        return Ms
    ops = [np.asarray(O)] * len(Ms) if isinstance(O, np.ndarray) else [np.asarray(o) for o in O]
    if len(ops) != len(Ms):
        raise ValueError(f"one operator per site: {len(ops)} operators for {len(Ms)} sites")
    for j, (o, m) in enumerate(zip(ops, Ms)):
        if o.shape != m.shape:
            raise ValueError(f"site {j}: operator of shape {o.shape} on a physical dimension {m.shape[0]}")
    vals = np.array([np.sum(o * m) for o, m in zip(ops, Ms)])
    if not np.iscomplexobj(Ms[0]) and not any(np.iscomplexobj(o) for o in ops):
        return vals.real.astype(np.float64)
    return vals.astype(np.complex128)


def dot(bra, ket):
    """dot(w1, w2) = <w1|w2> (windowmps.jl:165-176); raises when the environments differ."""
    cx, b, k, R = _overlap_sweeps(bra, ket)
    be = ket.be
    # <bra|ket> = tr(R_{-1}) with one more step of the stored sweep: sum AL_0 R_0 conj(ALb_0), closed with the identity
    r = _right_step(be, cx, R[0], k.AL[0], b.AL[0])
    h = be.download_c(r.reshape(r.shape[1], r.shape[2])) if cx else be.download(r.reshape(r.shape[1], r.shape[2]))
    v = np.trace(h)
    return complex(v) if cx else float(v)
