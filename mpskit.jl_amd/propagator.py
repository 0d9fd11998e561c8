"""propagator / DynamicalDMRG (src/algorithms/propagator/corvector.jl:23-204): the dynamical correlation function
G(z) = <psi0| (z - H)^-1 |psi0> of a finite chain by the correction-vector method (cond-mat/0203500).

A site visit is a LINEAR SOLVE with the prepared one-site operator, GMRES(tol = 1e-12, krylovdim = 30, maxiter = 100): tens
of H_AC applications per visit, each one call of mpsk_hac_apply_axpby (the shifted operator a0 + a1 H_AC), and Krylov vector
arithmetic on the device.  Two flavours:
    NaiveInvert  (H_AC - z) AC' = -tos, value = <psi0|init>.  Complex whenever z is: runs on interleaved complex storage
                 (native_cplx.NativeFiniteMPS / NativeFinEnv) with a Krylov space over the complex numbers (mpsk_v*_c).
    Jeckelmann   (H2_AC - 2 omega H1_AC + |z|^2) AC' = -eta tos with H2 = H * H.  Real H and psi0 keep everything fp64
                 (FiniteMPS / FinEnv / FinEnvPair).
`tos` is psi0 projected on the tangent space of the correction vector `init` (ac_proj with the environments of
<init|psi0>).  `init` is never normalised: its norm carries the value."""
from __future__ import annotations

import math
import warnings
from dataclasses import dataclass, field

import numpy as np

from . import krylov
from .algorithms import _no_cplx
from .approximate import ac_proj
from .backend import DTensor
from .derivatives import ddAC
from .environments import environments
from .native_cplx import ComplexMPOHamiltonian, NativeFinEnv, NativeFiniteMPS
from .operators import MPOHamiltonian
from .states import FiniteMPS


class NaiveInvert:  # corvector.jl:48
    pass


class Jeckelmann:  # corvector.jl:99
    pass


@dataclass
class GMRES:  # Defaults.linearsolver  (defaults.jl:34)
    tol: float = 1e-12
    maxiter: int = 100
    krylovdim: int = 30


@dataclass
class DynamicalDMRG:  # corvector.jl:23-29
    flavour: object = field(default_factory=NaiveInvert)
    solver: GMRES = field(default_factory=GMRES)
    tol: float = 1e-11            # Defaults.tol * 10
    maxiter: int = 100
    verbosity: int = 0


class LinearCombination:  # utility/linearcombination.jl
    """sum_i coeffs[i] * opps[i] as a site operator: `lc(x, out)` applies every term to x.  `apply_axpby(a1, x, a0, out)`
    is a0 x + a1 lc(x) with the shift folded into the first term's own call where that term has one (MPO_ddAC).  cplx: the
    vectors are interleaved complex tensors and the coefficients may be complex."""

    def __init__(self, be, opps, coeffs, cplx=False):
        if len(opps) != len(coeffs) or not opps:
            raise ValueError("LinearCombination: one coefficient per operator")
        self.be, self.opps, self.coeffs = be, tuple(opps), tuple(coeffs)
        self.vs = krylov.ComplexVec(be) if cplx else krylov._RealVec(be)
        self._tmp = None                  # image of the later terms: one scratch tensor for the whole solve

    def apply_axpby(self, a1, x: DTensor, a0, out: DTensor = None):
        be, vs = self.be, self.vs
        out = be.empty(*x.shape) if out is None else out
        first = self.opps[0]
        if hasattr(first, "apply_axpby"):
            first.apply_axpby(a1 * self.coeffs[0], x, a0, out)
        else:
            first(x, out)
            vs.axpby(a0, x, a1 * self.coeffs[0], out)
        for c, h in zip(self.coeffs[1:], self.opps[1:]):
            if self._tmp is None or self._tmp.shape != out.shape:
                self._tmp = be.empty(*out.shape)
            vs.axpby(a1 * c, h(x, self._tmp), 1.0, out)
        return out

    def __call__(self, x: DTensor, out: DTensor = None):
        return self.apply_axpby(1.0, x, 0.0, out)

    __mul__ = __call__


def _warn(pos, info):
    if not info.converged:
        warnings.warn(f"propagator ({pos}) failed to converge: normres = {info.normres:.3e}", RuntimeWarning, stacklevel=3)


def _abs_change(be, new: DTensor, old: DTensor):
    """norm(AC' - AC)  (corvector.jl:70)"""
    if hasattr(be, "vdiff_nrm2"):
        return math.sqrt(max(be.vdiff_nrm2(new, old)[0], 0.0))
    return be.norm(be.axpby(-1.0, old, 1.0, be.copy(new)))


def _sweep_log(alg, it, eps):
    if alg.verbosity >= 3:
        print(f"[ Info: DDMRG {it:3d}:\terr = {eps:.10e}", flush=True)


def _order(L):
    return list(range(0, L - 1)) + list(range(L - 1, 0, -1))      # [1:L-1; L:-1:2]


def propagator(psi0, z, H, alg: DynamicalDMRG = None, init=None, canonical=True):
    """propagator(psi0, z, H, alg; init = copy(psi0)) -> (value, init)  (corvector.jl:50-90, :101-154):
    value = <psi0| (z - H)^-1 |psi0> as a Python complex (what the reference's code computes: no E0 term), init = the
    correction vector, un-normalised.  A site solve that does not converge warns and never raises.
    NaiveInvert accepts a real FiniteMPS or a native_cplx.NativeFiniteMPS start and returns a NativeFiniteMPS; Jeckelmann
    takes a real FiniteMPS and a real MPOHamiltonian and stays in fp64.  canonical=False keeps NaiveInvert on the general
    complex operator (mode 2) instead of the Jordan-form one (A/B switch; the result is the same)."""
    alg = DynamicalDMRG() if alg is None else alg
    if isinstance(alg.flavour, Jeckelmann):
        return _jeckelmann(psi0, complex(z), H, alg, init)
    if isinstance(alg.flavour, NaiveInvert):
        return _naive_invert(psi0, complex(z), H, alg, init, canonical)
    raise TypeError(f"DynamicalDMRG flavour must be NaiveInvert or Jeckelmann, not {type(alg.flavour).__name__}")


# ---- Jeckelmann: fp64 on the lazy-gauge FiniteMPS -------------------------------------------------------------------------

def _jeckelmann(psi0, z, H, alg, init):  # corvector.jl:101-154
    if not isinstance(psi0, FiniteMPS) or getattr(psi0, "cplx", False) or (init is not None and getattr(init, "cplx", True)):
        raise NotImplementedError("propagator with the Jeckelmann flavour takes a real FiniteMPS: a complex state is not "
                                  "implemented (use NaiveInvert, which runs on interleaved complex storage)")
    if not isinstance(H, MPOHamiltonian) or getattr(H[0], "cplx", False):
        raise NotImplementedError("propagator with the Jeckelmann flavour takes a real MPOHamiltonian (H2 = conj(H) * H of "
                                  "a complex operator is not implemented)")
    omega, eta = z.real, z.imag
    if eta == 0.0:
        raise ValueError("propagator (Jeckelmann): z needs a non-zero imaginary part")
    be, L = psi0.be, len(psi0)
    A = psi0.copy()                       # the views of the copy fill their own caches: psi0 itself is left as it was
    init = A.copy() if init is None else init
    envs1 = environments(init, H)
    H2 = H * H                            # squaredenvs (corvector.jl:156-192): on a finite chain the boundary vectors of
    envs2 = environments(init, H2)        # environments(init, H2) are already the squared ones
    mixed = environments(init, A)         # <init|psi0>
    ws = krylov.KrylovWorkspace(be)
    sv = alg.solver
    eps = 2 * alg.tol
    for it in range(1, alg.maxiter + 1):
        eps = 0.0
        for pos in _order(L):
            tos = ac_proj(pos, init, mixed)
            op = LinearCombination(be, (ddAC(pos, init, H, envs1), ddAC(pos, init, H2, envs2)), (-2.0 * omega, 1.0))
            ac = init.AC(pos)
            rhs = be.axpby(-eta, tos, 0.0, be.empty(*tos.shape))
            new, info = krylov.linsolve(be, op, rhs, ac, a0=abs(z) ** 2, a1=1.0, tol=sv.tol, krylovdim=sv.krylovdim,
                                        maxiter=sv.maxiter, ws=ws)
            eps = max(eps, _abs_change(be, new, ac))
            init.set_AC(pos, new)
            _warn(pos, info)
        _sweep_log(alg, it, eps)
        if eps <= alg.tol:
            break
    else:
        if alg.verbosity >= 1 and alg.maxiter >= 1:
            warnings.warn(f"propagator: not converged after {alg.maxiter} sweeps, err = {eps:.3e}", RuntimeWarning, stacklevel=3)
    a = be.dot(ac_proj(0, init, mixed), init.AC(0))                        # <psi0|init>
    hmixed = environments(A, (H, init))                                     # <psi0|H|init>
    b = be.dot(A.AC(0), ac_proj(0, A, hmixed))
    init.eps = eps
    return complex(b / eta - omega / eta * a, a), init


# ---- NaiveInvert: interleaved complex storage -------------------------------------------------------------------------------

class _OverlapEnv:
    """environments(init, psi0) on interleaved storage (FinEnv.jl:91-99): GL[j] (2 D_init, D_psi0) left of site j, GR[j]
    (2 D_psi0, D_init) right of site j - 1, no operator leg.  An update is two complex products (mpsk_gemm under MPSK_C128).
    The tensors of psi0 are fixed; only `below` moves."""

    def __init__(self, below: NativeFiniteMPS, above: NativeFiniteMPS):
        be = self.be = below.be
        L = self.L = len(below)
        if len(above) != L:
            raise ValueError(f"the two states have different lengths ({L} != {len(above)})")
        self.above = above
        self.GL = [be.upload_c(np.eye(below.dims(0)[0], above.dims(0)[0]))] + [None] * L
        self.GR = [None] * L + [be.upload_c(np.eye(above.dims(L - 1)[2], below.dims(L - 1)[2]))]
        for j in range(L - 1, below.center, -1):
            self.extend_right(below, j)
        for j in range(0, below.center):
            self.extend_left(below, j)

    def extend_left(self, psi, j):
        be, a, b = self.be, self.above.A[j], psi.A[j]
        Da2, d, Dra = a.shape
        Db2, _, Drb = b.shape
        t = be.gemm_c(self.GL[j], a.reshape(Da2, d * Dra))                            # [D_b, (d, Dr_a)]
        self.GL[j + 1] = be.gemm_c(b.reshape(Db2 * d, Drb), t.reshape(Db2 * d, Dra), transA=True)

    def extend_right(self, psi, j):
        be, a, b = self.be, self.above.A[j], psi.A[j]
        Da2, d, Dra = a.shape
        Db2, _, Drb = b.shape
        t = be.gemm_c(a.reshape(Da2 * d, Dra), self.GR[j + 1])                        # [(Dl_a, d), Dr_b]
        self.GR[j] = be.gemm_c(t.reshape(Da2, d * Drb), b.reshape(Db2, d * Drb), transB=True)

    def ac_proj(self, pos):
        """ac_proj(pos, init, mixedenvs)  (derivatives.jl:210-215): GL psi0.A[pos] GR, [D_init, d, D_init]"""
        be, a = self.be, self.above.A[pos]
        Da2, d, Dra = a.shape
        t = be.gemm_c(self.GL[pos], a.reshape(Da2, d * Dra))
        Db2 = t.shape[0]
        y = be.gemm_c(t.reshape(Db2 * d, Dra), self.GR[pos + 1])
        return y.reshape(Db2, d, y.shape[1])


class _ShiftedHAC:
    """H_AC of the centre site on interleaved vectors with its shifted form a0 x + a1 H_AC x (mpsk_hac_apply_axpby)."""

    def __init__(self, be, envs: NativeFinEnv, pos, canonical=True):
        self.vs = krylov.ComplexVec(be)
        if canonical and hasattr(be, "hac_create_ex"):
            # the environments of the correction vector are canonical: the Jordan-form operator (MPSK_HAC_CANONICAL_C128)
            self.h = be.hac_create_ex(envs.opp[pos], envs.GL[pos], envs.GR[pos + 1], canonical_c128=True)
        else:
            self.h = be.hac_create(envs.opp[pos], envs.GL[pos], envs.GR[pos + 1])

    def __call__(self, x, out=None):
        return self.h.apply(x, out=out)

    def apply_axpby(self, a1, x, a0, out=None):
        if hasattr(self.h, "apply_axpby"):
            return self.h.apply_axpby(a1, x, a0, out=out)
        return self.vs.axpby(a0, x, a1, self.h.apply(x, out=out))


def to_native(psi0) -> NativeFiniteMPS:
    """a real FiniteMPS as a NativeFiniteMPS (interleaved complex128, zero imaginary parts, same norm); a NativeFiniteMPS is
    copied."""
    if isinstance(psi0, NativeFiniteMPS):
        return psi0.copy()
    if not isinstance(psi0, FiniteMPS):
        raise TypeError(f"propagator takes a FiniteMPS or a NativeFiniteMPS, not {type(psi0).__name__}")
    _no_cplx(psi0, "propagator (convert the state to a native_cplx.NativeFiniteMPS)")
    return NativeFiniteMPS(psi0.copy().to_host(), psi0.be, normalize=False)


def _naive_invert(psi0, z, H, alg, init, canonical=True):  # corvector.jl:50-90
    if not isinstance(H, (MPOHamiltonian, ComplexMPOHamiltonian)):
        raise TypeError(f"propagator takes an MPOHamiltonian, not {type(H).__name__}")
    A = to_native(psi0)
    be, L = A.be, len(A)
    init = A.copy() if init is None else to_native(init)
    init.move_center(0)
    h_envs = NativeFinEnv(init, H)
    mixed = _OverlapEnv(init, A)
    vs = krylov.ComplexVec(be)
    ws = krylov.KrylovWorkspace(be)
    sv = alg.solver
    eps = 2 * alg.tol
    stats = {"matvecs": 0, "solves": 0}

    def visit(pos):
        tos = mixed.ac_proj(pos)
        ac = init.A[pos]
        rhs = vs.axpby(-1.0, tos, 0.0, be.empty(*tos.shape))
        new, info = krylov.linsolve(be, _ShiftedHAC(be, h_envs, pos, canonical), rhs, ac, a0=-z, a1=1.0, tol=sv.tol,
                                    krylovdim=sv.krylovdim, maxiter=sv.maxiter, ws=ws, cplx=True)
        stats["matvecs"] += info.numops
        stats["solves"] += 1
        change = _abs_change(be, new, ac)
        init.A[pos] = new
        _warn(pos, info)
        return change

    sweeps = 0
    for it in range(1, alg.maxiter + 1):
        eps, sweeps = 0.0, it
        for pos in range(0, L - 1):
            eps = max(eps, visit(pos))
            init._shift_right(pos)
            h_envs.extend_left(init, pos)
            mixed.extend_left(init, pos)
        for pos in range(L - 1, 0, -1):
            eps = max(eps, visit(pos))
            init._shift_left(pos)
            h_envs.extend_right(init, pos)
            mixed.extend_right(init, pos)
        _sweep_log(alg, it, eps)
        if eps <= alg.tol:
            break
    else:
        if alg.verbosity >= 1 and alg.maxiter >= 1:
            warnings.warn(f"propagator: not converged after {alg.maxiter} sweeps, err = {eps:.3e}", RuntimeWarning, stacklevel=3)
    value = vs.dot(mixed.ac_proj(0), init.A[0])                             # dot(psi0, init)
    init.eps, init.sweeps, init.solver_stats = eps, sweeps, stats
    return complex(value), init
