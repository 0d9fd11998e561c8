"""fidelity_susceptibility (src/algorithms/fidelity_susceptibility.jl) and effective_excitation_hamiltonian
(src/algorithms/excitation/quasiparticleexcitation.jl:254-328) on the quasiparticle tangent space of a real ground state.

    chi[a, b] = <x_a, x_b>,     H_eff x_a = T_a,     T_a[i] = VL_i^T (H_AC^{V_a}(i) AC_i)

with H_eff the effective excitation Hamiltonian of H0 (energy subtracted) at momentum 0 and one real part.  H_eff is applied
once per GMRES step: on the fused route every site is one mpsk_qp_heff_site (quasiparticle.py, _QPContext(device=True)).

The right-hand side.  Line 13 of the reference contracts the local tensor of H0 between the environments of V, which drops
V's own term at site i and is only well formed when H0 and V have the same MPO shape.  Here the right-hand side is built
from V's own slice, ddAC(i, state, V, venvs): the tangent-space projection of V |psi>, which is what the exact expression
chi_ab = <psi| V_a Q (H0 - E0)^-2 Q V_b |psi> (Q = 1 - |psi><psi|) needs, and what the exact test compares against."""
from __future__ import annotations

import warnings

import numpy as np

from . import krylov
from .derivatives import ddAC
from .environments import environments as _environments
from .operators import LazySum, MPOHamiltonian, MultipliedOperator
from .quasiparticle import LeftGaugedQP, QuasiparticleAnsatz, _QPContext, _has_heff_entries, _view
from .states import FiniteMPS, InfiniteMPS

# device=None of fidelity_susceptibility / effective_excitation_hamiltonian: the fused route only where mpsk_qp_heff_site
# measured faster than the composed sequence at BOTH sizes of tools/bench_qp_heff.py (profiles/qp_heff_timings.json, README:
# composed with B reused / fused = 1.25 at D = 256 and 1.42 at D = 1024)
FUSED_BY_DEFAULT = True


def _use_device(be, device):
    if device is None:
        return FUSED_BY_DEFAULT and _has_heff_entries(be)
    return bool(device)          # device=True on a backend without the entries: _QPContext raises


def _check_operator(H, name):
    if isinstance(H, LazySum):
        raise TypeError(f"{name}: a LazySum is not supported, pass one MPOHamiltonian")
    if isinstance(H, MultipliedOperator):
        raise TypeError(f"{name}: a MultipliedOperator (timed or untimed) is not supported, pass one MPOHamiltonian")
    if not isinstance(H, MPOHamiltonian):
        raise TypeError(f"{name}: expected an MPOHamiltonian, got {type(H).__name__}")


def _check_state(state, name="state"):
    if not isinstance(state, (FiniteMPS, InfiniteMPS)):
        raise TypeError(f"{name}: expected a FiniteMPS or an InfiniteMPS, got {type(state).__name__}")
    if getattr(state, "cplx", False):
        raise NotImplementedError(f"{name}: complex ground states are not built (real fp64 states only)")


def qp_dot(a: LeftGaugedQP, b: LeftGaugedQP):
    """dot(a, b) of two LeftGaugedQP on the same ground state: sum_i <X_a[i], X_b[i]> (the B tensors B = VL X have the same
    inner product, VL^T VL = 1).  A float for one real part, complex when either side carries two."""
    if a.left_gs is not b.left_gs or a.right_gs is not b.right_gs or a.N != b.N:
        raise ValueError("qp_dot: the two quasiparticle states live on different ground states")
    be, N = a.be, a.N
    part = lambda q, k: _view(q.vec, k * N, (N,))
    rr = be.dot(part(a, 0), part(b, 0))
    if a.nparts == 1 and b.nparts == 1:
        return float(rr)
    ai = part(a, 1) if a.nparts == 2 else None
    bi = part(b, 1) if b.nparts == 2 else None
    re, im = rr, 0.0
    if ai is not None and bi is not None:
        re += be.dot(ai, bi)
    if bi is not None:
        im += be.dot(part(a, 0), bi)
    if ai is not None:
        im -= be.dot(ai, part(b, 0))
    return complex(re, im)                      # <a, b> = conj(a) . b


def effective_excitation_hamiltonian(H, phi: LeftGaugedQP, envs=None, device=None) -> LeftGaugedQP:
    """effective_excitation_hamiltonian(H, phi, environments(phi, H, envs))  (quasiparticleexcitation.jl:254-328): the
    effective Hamiltonian of the quasiparticle tangent space applied to phi, the ground-state energy subtracted.  envs: the
    environments of phi.left_gs under H.  device: None = FUSED_BY_DEFAULT, True = mpsk_qp_heff_site and the pair transfers,
    False = the composed route (also what a backend without the entries runs)."""
    _check_operator(H, "H")
    if not isinstance(phi, LeftGaugedQP):
        raise TypeError(f"phi: expected a LeftGaugedQP, got {type(phi).__name__}")
    be = phi.be
    envs = _environments(phi.left_gs, H) if envs is None else envs
    ctx = _QPContext(H, phi, envs, QuasiparticleAnsatz(), None, _use_device(be, device))
    out = be.empty(phi.vec.shape)
    ctx.heff(phi, phi.vec, out)
    return phi.with_vec(out)


def _rhs(state, V, phi: LeftGaugedQP):
    """T[i] = VL_i^T (H_AC^V(i) AC_i) as the flat X vector of phi."""
    be = state.be
    venvs = _environments(state, V)
    out = be.zeros(phi.vec.shape)
    for i in range(len(phi)):
        if phi.xshapes[i][0] == 0:
            continue
        ac = state.AC(i) if phi.finite else state.AC[i]
        t = ddAC(i, state, V, venvs)(ac)
        Dl, d, Dr = t.shape
        be.gemm(phi.VLs[i], t.reshape(Dl * d, Dr), transA=True, out=phi.X(0, i, out))
    return out


def tangent_vectors(state, H0, Vs, henvs=None, *, maxiter=100, tol=1e-12, device=None):
    """The `tangent_vecs` of fidelity_susceptibility.jl:9-25 -> (xs, Ts): for every V the solution x of H_eff x = T and the
    right-hand side T, both as LeftGaugedQP on one shared set of VL (momentum 0, one real part)."""
    _check_state(state, "state")
    _check_operator(H0, "H0")
    if isinstance(Vs, (MPOHamiltonian, LazySum, MultipliedOperator)) or not hasattr(Vs, "__len__"):
        raise TypeError("Vs: expected a list of MPOHamiltonian")
    for a, V in enumerate(Vs):
        _check_operator(V, f"Vs[{a}]")
    be = state.be
    henvs = _environments(state, H0) if henvs is None else henvs
    phi = LeftGaugedQP.random(state, 0.0)
    ctx = _QPContext(H0, phi, henvs, QuasiparticleAnsatz(), None, _use_device(be, device))
    ws = krylov.KrylovWorkspace(be)             # not ctx.ws: the environment solves run inside this solver's matvec

    def op(x, out):
        return ctx.heff(phi, x, out)

    xs, Ts = [], []
    for V in Vs:
        T = _rhs(state, V, phi)
        info = {}
        x = krylov.gmres(be, op, T, T, tol=tol, maxiter=maxiter, ws=ws, info=info)
        if not info["converged"]:
            warnings.warn(f"failed to converge: normres = {info['normres']}")        # fidelity_susceptibility.jl:21
        xs.append(phi.with_vec(x))
        Ts.append(phi.with_vec(T))
    return xs, Ts


def fidelity_susceptibility(state, H0, Vs, henvs=None, *, maxiter=100, tol=1e-12, device=None):
    """fidelity_susceptibility(state, H0, Vs, henvs; maxiter, tol)  (fidelity_susceptibility.jl) -> chi[len(Vs), len(Vs)]:
    the Gram matrix of the tangent vectors x_a that solve H_eff x_a = T_a (GMRES from x = T_a), H_eff the effective
    excitation Hamiltonian of H0 on the left-gauged tangent space of `state` at momentum 0.

    state: a real FiniteMPS or InfiniteMPS; H0 and every V: MPOHamiltonian (V may have another MPO bond dimension and
    another period than H0).  The right-hand side is T_a[i] = VL_i^T (H_AC^{V_a}(i) AC_i) with V_a's OWN slice and
    environments -- not the reference's line 13, which puts H0's local tensor between V's environments (see the module
    docstring).  For a finite chain at full bond dimension chi_ab = <psi| V_a Q (H0 - E0)^-2 Q V_b |psi>.  Not rescaled by
    the system size or the unit cell (as the reference).

    device: None = FUSED_BY_DEFAULT, True / False = the fused / the composed route of the operator."""
    xs, _ = tangent_vectors(state, H0, Vs, henvs, maxiter=maxiter, tol=tol, device=device)
    vecs = [x.vec for x in xs]
    chi = np.zeros((len(vecs), len(vecs)))
    for a, v in enumerate(vecs):
        chi[:, a] = state.be.multidot(vecs, v)
    return chi
