"""Effective-Hamiltonian ("derivative") operators, src/algorithms/derivatives.jl:6-71.
Same names and call convention as the reference: `h = ddAC(pos, psi, H, envs); y = h(x)` /
`h * x`; every application is ONE call into libmpsk (mpsk_dAC / mpsk_dC / mpsk_dAC2)."""
from __future__ import annotations

import os

from .backend import DTensor


class MPO_ddC:  # MPO_∂∂C  derivatives.jl:6-9
    def __init__(self, be, leftenv, rightenv):
        self.be, self.leftenv, self.rightenv = be, leftenv, rightenv

    def __call__(self, x: DTensor, out: DTensor = None):
        return self.be.dC(self.leftenv, self.rightenv, x, out=out)

    __mul__ = __call__


class MPO_ddAC:  # MPO_∂∂AC  derivatives.jl:11-15
    """Built once per site visit, applied by every Krylov step: the first application prepares the device-side
    operator (mpsk_hac_create: MPO tensor folded into the right environment where that saves the slab mix), every
    application is then mpsk_hac_apply."""

    def __init__(self, be, o, leftenv, rightenv, canonical=False):
        self.be, self.o, self.leftenv, self.rightenv = be, o, leftenv, rightenv
        # canonical: level 0 of leftenv and level W-1 of rightenv are identities (environments of a finite chain in
        # canonical form), which lets a Jordan-form slice skip the identity products (mpsk_hac_create_ex, mode 3)
        self.canonical = bool(canonical)
        self._hac = None

    def _prepare(self):
        if self._hac is None:
            if self.canonical and hasattr(self.be, "hac_create_ex"):
                self._hac = self.be.hac_create_ex(self.o, self.leftenv, self.rightenv, canonical=True)
            else:
                self._hac = self.be.hac_create(self.o, self.leftenv, self.rightenv)
        return self._hac

    def __call__(self, x: DTensor, out: DTensor = None):
        if not hasattr(self.be, "hac_create"):                   # host stand-in backend of the CPU tests
            return self.be.dAC(self.o, self.leftenv, self.rightenv, x, out=out)
        return self._prepare().apply(x, out=out)

    __mul__ = __call__

    def apply_axpby(self, a1, x: DTensor, a0, out: DTensor = None):
        """out = a0 x + a1 (H_AC x) in one library call (mpsk_hac_apply_axpby): what a shifted linear solve applies."""
        if not hasattr(self.be, "hac_create"):                   # host stand-in backend of the CPU tests
            if complex(a0).imag != 0.0 or complex(a1).imag != 0.0:
                raise TypeError("MPO_ddAC.apply_axpby on a real backend takes real a0 and a1")
            y = self.be.dAC(self.o, self.leftenv, self.rightenv, x, out=out)
            return self.be.axpby(complex(a0).real, x, complex(a1).real, y)
        return self._prepare().apply_axpby(a1, x, a0, out=out)

    def eigsolve_fixed(self, x0: DTensor, m: int, vecs, scal: DTensor, out: DTensor, first_image: DTensor = None):
        """Fixed-budget :SR solve in one library call (mpsk_hac_eigsolve_fixed); None if this operator cannot take it
        (host stand-in backend, complex operator)."""
        if not hasattr(self.be, "hac_create"):
            return None
        self._prepare()
        if self._hac.cplx or self._hac.Dlo != self._hac.Dl:
            return None
        return self._hac.eigsolve_fixed(x0, m, vecs, scal, out, first_image)


class MPO_ddAC2:  # MPO_∂∂AC2  derivatives.jl:17-22
    def __init__(self, be, o1, o2, leftenv, rightenv):
        self.be, self.o1, self.o2, self.leftenv, self.rightenv = be, o1, o2, leftenv, rightenv

    def __call__(self, x: DTensor, out: DTensor = None):
        return self.be.dAC2(self.o1, self.o2, self.leftenv, self.rightenv, x, out=out)

    __mul__ = __call__


class LazyDerivativeSum:  # derivatives.jl:310-323 : (h::LazySum{<:DerivativeOperator})(x) = sum(f_k * h_k(x))
    def __init__(self, be, terms, fs):
        self.be, self.terms, self.fs = be, list(terms), list(fs)

    def __call__(self, x: DTensor, out: DTensor = None):
        y = self.terms[0](x, out=out)
        if self.fs[0] != 1.0:
            self.be.scal(self.fs[0], y)
        for f, h in zip(self.fs[1:], self.terms[1:]):
            self.be.axpby(f, h(x), 1.0, y)
        return y

    __mul__ = __call__


class _ComposedAt:
    """sum_k c_k h_k(x) at fixed numbers c_k, term by term (the composed route of a timed sum): every term writes into a
    buffer that is kept, the first one straight into `out`."""

    def __init__(self, be, terms, coefs, owner):
        self.be, self.terms, self.coefs, self.owner = be, terms, coefs, owner

    def __call__(self, x: DTensor, out: DTensor = None):
        be = self.be
        y = self.terms[0](x, out=out)
        if self.coefs[0] != 1.0:
            be.scal(self.coefs[0], y)
        for c, h in zip(self.coefs[1:], self.terms[1:]):
            tmp = self.owner._tmp
            if tmp is None or tmp.shape != y.shape:
                tmp = self.owner._tmp = be.empty(*y.shape)
            be.axpby(c, h(x, out=tmp), 1.0, y)
        return y

    __mul__ = __call__


class _HSumAt:
    """the prepared sum (mpsk_hsum) with the coefficients it was last given: one library call per application."""

    def __init__(self, hsum):
        self.hsum = hsum

    def __call__(self, x: DTensor, out: DTensor = None):
        return self.hsum.apply(x, out=out)

    __mul__ = __call__

    def apply_axpby(self, a1, x: DTensor, a0, out: DTensor = None):
        return self.hsum.apply_axpby(a1, x, a0, out=out)


class TimedDerivativeSum:  # derivatives.jl:283-323
    """Effective Hamiltonian of a MultipliedOperator / of a LazySum with prefactors f_k that may depend on time: callable
    as h(x, t) (and as h(x) when no f_k is a function); h.at(t) is the operator at the fixed time t, which is what an
    integrator applies many times.  With `hsum` (a zero-argument factory of a backend PreparedHSum over the same terms) and
    real f_k(t) the fixed-time operator is the device-side sum: built once per site visit, set_coefs once per time."""

    def __init__(self, be, terms, fs, hsum=None, wrap=None):
        self.be, self.terms, self.fs = be, list(terms), list(fs)
        self.timed = any(callable(f) for f in self.fs)
        self._make, self._hsum, self._tmp = hsum, None, None
        self._wrap = wrap                # embedded complex states: the device sum iterates on half-embedded vectors

    def coefs(self, t=None):
        if self.timed and t is None:
            raise ValueError("a time-dependent effective Hamiltonian needs its time: h(x, t).  Only the time-evolution "
                             "drivers pass one; every other driver takes the evaluated operator H(t)")
        return [f(t) if callable(f) else f for f in self.fs]

    def at(self, t=None):
        cs = self.coefs(t)
        if self._make is not None and all(complex(c).imag == 0.0 for c in cs):
            if self._hsum is None:
                self._hsum = self._make()
            self._hsum.set_coefs([complex(c).real for c in cs])
            op = _HSumAt(self._hsum)
            return op if self._wrap is None else self._wrap(op)
        cs = [complex(c).real if complex(c).imag == 0.0 else complex(c) for c in cs]
        if any(isinstance(c, complex) for c in cs):
            raise NotImplementedError("complex-valued prefactors f(t) are not implemented, on any kind of state: with an "
                                      "imaginary step the midpoint t + dt/2 is complex, so f must return a real number there")
        return _ComposedAt(self.be, self.terms, cs, self)

    def __call__(self, x: DTensor, t=None, out: DTensor = None):
        if isinstance(t, DTensor):                           # h(x, out) of the untimed case
            t, out = None, t
        return self.at(t)(x, out=out)

    __mul__ = __call__

    def info(self):
        """route of the device-side sum (mpsk_hsum_info), None while / where the composed route is used."""
        return None if self._hsum is None else self._hsum.info()


def _timed_lazy(fn, pos, psi, H, envs):
    """derivative of a timed LazySum: the terms as a sum builds them, the prefactors kept as functions.  ddAC on plain
    finite / infinite Hamiltonian environments of a real state goes through mpsk_hsum (folded on canonical finite
    environments, accumulated otherwise); everything else is composed."""
    from .environments import FinEnv, MPOHamInfEnv
    be = psi.be
    cx = getattr(psi, "cplx", False)
    es = envs.envs
    make = wrap = None
    on = os.environ.get("MPSK_HSUM", "1") != "0"              # "0": always the composed route (A/B switch)
    # `type(e) is`, not isinstance: native_cplx.NativeMPOHamInfEnv subclasses MPOHamInfEnv and must stay excluded here
    if (fn is ddAC and on and hasattr(be, "hsum_create") and len(es) <= 8
            and (all(type(e) is FinEnv for e in es) or all(type(e) is MPOHamInfEnv for e in es))):
        opps = [e.opp[pos] if hasattr(e, "opp") else h[pos] for h, e in zip(H, es)]
        GLs = [e.leftenv(pos, psi) for e in es]
        GRs = [e.rightenv(pos, psi) for e in es]
        if not cx:
            canonical = all(type(e) is FinEnv and e._canonical(psi) for e in es)
            make = lambda: be.hsum_create(opps, GLs, GRs, canonical=canonical)
        elif not any(_native_cplx(psi, gl, gr) for gl, gr in zip(GLs, GRs)):
            # embedded complex state: the real slices on the embedded (doubled) environments, accumulated route
            make = lambda: be.hsum_create(opps, GLs, GRs)
            wrap = lambda op: _half_space(psi, op, "AC", GRs[0])
    kw = {"canonical": False} if fn is ddAC else {}
    terms = [fn(pos, psi, h, e, **kw) for h, e in zip(H, es)]
    if cx and any(hasattr(e, "vector") for e in es):
        raise NotImplementedError("a timed sum with a projector term on an embedded complex state")
    return TimedDerivativeSum(be, terms, H._fs, hsum=make, wrap=wrap)


def _multiplied(fn, pos, psi, H, envs):
    """derivative of a MultipliedOperator f * op (derivatives.jl:283-308): f times the derivative of op."""
    return TimedDerivativeSum(psi.be, [fn(pos, psi, H.op, envs)], [H.f])


def _lazy(fn, pos, psi, H, envs):
    if getattr(H, "timed", False):
        return _timed_lazy(fn, pos, psi, H, envs)
    kw = {"canonical": False} if fn is ddAC else {}          # the terms of a sum keep the dense operator
    op = LazyDerivativeSum(psi.be, [fn(pos, psi, h, e, **kw) for h, e in zip(H, envs.envs)], H.fs)
    if getattr(psi, "cplx", False) and any(hasattr(e, "vector") for e in envs.envs):
        # a projector term exists in the embedded sector only: iterate on half-embedded vectors (cplx.HalfSpaceOp)
        from .cplx import HalfSpaceOp
        kind = {"ddAC": "AC", "ddC": "C", "ddAC2": "AC2"}[fn.__name__]
        t = psi.AC(pos) if kind != "C" else psi.CR(pos)
        Dr2 = psi.AR(pos + 1).shape[2] if kind == "AC2" else t.shape[-1]
        return HalfSpaceOp(psi.be, op, kind, Dr2 // 2)
    return op


def _is_lazy(H, envs):
    return hasattr(envs, "envs") and (hasattr(H, "_fs") or hasattr(H, "fs"))


def _is_multiplied(H):
    from .operators import MultipliedOperator
    return isinstance(H, MultipliedOperator)


NATIVE_CPLX_MIN_D = 384     # embedded bond dimension 2 D below which the embedded matvec wins (launch-bound regime:
                            # profiles/r02_bench_cplx.log -- native 1.81x at D = 1024, 1.57x at 512, 0.76x at 256)


def _native_cplx(psi, *envs_):
    """complex (embedded) state on a backend with the MPSK_C128 kernels: apply through cplx.HalfEmbeddedOp when the
    tensors are large enough for the halved flop count to matter."""
    if not (getattr(psi, "cplx", False) and hasattr(psi.be, "hac_create")):
        return False
    mode = os.environ.get("MPSK_NATIVE_CPLX", "auto")          # "0": always embedded, "1": always native (A/B switch)
    if mode in ("0", "1"):
        return mode == "1"
    return all(e.shape[1] // 2 >= NATIVE_CPLX_MIN_D for e in envs_)


def _half_space(psi, op, kind, GR):
    """Embedded complex state below the native-kernel threshold: the operator still runs on embedded tensors, but the Krylov
    solvers iterate on HALF-embedded (= interleaved complex) vectors (cplx.HalfSpaceOp: encode . op . decode).  On embedded
    vectors the real space is twice the complex one -- besides the embeddings it holds the anti-structured tensors X_E sigma_z,
    on which an embedded operator acts as its partial complex conjugate, with eigenvalues that can lie BELOW the ground state.
    A solve that restarts from a converged tensor (fixed-budget sweeps: the first residual is rounding noise, normalised to
    O(1)) drifts into that sector: measured on a converged L = 16, D = 64 Heisenberg chain, sweep energies of -7.13 against a
    ground-state energy of -6.9117 (tools/native_vs_embedded.py).  On half vectors the sector does not exist."""
    if not getattr(psi, "cplx", False):
        return op
    from .cplx import HalfSpaceOp
    return HalfSpaceOp(psi.be, op, kind, GR.shape[1] // 2)


def ddC(pos, psi, H, envs):  # ∂∂C  derivatives.jl:34-36
    if _is_multiplied(H):
        return _multiplied(ddC, pos, psi, H, envs)
    if _is_lazy(H, envs):
        return _lazy(ddC, pos, psi, H, envs)
    if _native_cplx(psi, envs.leftenv(pos + 1, psi), envs.rightenv(pos, psi)):
        from .cplx import HalfEmbeddedOp
        return HalfEmbeddedOp(psi.be, "C", [], envs.leftenv(pos + 1, psi), envs.rightenv(pos, psi))
    GR = envs.rightenv(pos, psi)
    return _half_space(psi, MPO_ddC(psi.be, envs.leftenv(pos + 1, psi), GR), "C", GR)


def ddAC(pos, psi, H, envs, canonical=None):  # ∂∂AC  derivatives.jl:44-46
    """canonical: None = decide here -- only the environments of a plain FinEnv on a real state are canonical (level 0 of
    GL and level W-1 of GR identities); every other kind (sums, projectors, infinite / sharded environments) and every
    complex state keeps the dense operator."""
    if _is_multiplied(H):
        return _multiplied(ddAC, pos, psi, H, envs)
    if _is_lazy(H, envs):
        return _lazy(ddAC, pos, psi, H, envs)
    if hasattr(envs, "vector"):          # ProjectionOperator term (excitations.py): rank-one |v><v|
        from .excitations import Proj_ddAC
        return Proj_ddAC(psi.be, envs.vector(pos, psi), bool(getattr(psi, "cplx", False)))
    opp = envs.opp[pos] if hasattr(envs, "opp") else H[pos]
    if _native_cplx(psi, envs.leftenv(pos, psi), envs.rightenv(pos, psi)):
        from .cplx import HalfEmbeddedOp
        return HalfEmbeddedOp(psi.be, "AC", [opp], envs.leftenv(pos, psi), envs.rightenv(pos, psi))
    GR = envs.rightenv(pos, psi)
    if canonical is None:
        from .environments import FinEnv
        # (a window's environments, window.WindowEnv, keep the promise when their two start identities were verified)
        canonical = ((type(envs) is FinEnv or (getattr(envs, "window_canonical", False) and getattr(envs, "canonical", False)))
                     and not getattr(psi, "cplx", False))
    return _half_space(psi, MPO_ddAC(psi.be, opp, envs.leftenv(pos, psi), GR, canonical=canonical), "AC", GR)


def ddAC2(pos, psi, H, envs):  # ∂∂AC2  derivatives.jl:55-58
    if _is_multiplied(H):
        return _multiplied(ddAC2, pos, psi, H, envs)
    if _is_lazy(H, envs):
        return _lazy(ddAC2, pos, psi, H, envs)
    o1 = envs.opp[pos] if hasattr(envs, "opp") else H[pos]
    o2 = envs.opp[pos + 1] if hasattr(envs, "opp") else H[pos + 1]
    if _native_cplx(psi, envs.leftenv(pos, psi), envs.rightenv(pos + 1, psi)):
        from .cplx import HalfEmbeddedOp
        return HalfEmbeddedOp(psi.be, "AC2", [o1, o2], envs.leftenv(pos, psi), envs.rightenv(pos + 1, psi))
    GR = envs.rightenv(pos + 1, psi)
    return _half_space(psi, MPO_ddAC2(psi.be, o1, o2, envs.leftenv(pos, psi), GR), "AC2", GR)
