"""approximate (src/algorithms/approximate/approximate.jl:1-27, fvomps.jl:1-87) for FiniteMPS and make_time_mpo
(src/algorithms/timestep/timeevmpo.jl): apply an MPO to a finite MPS / compress a state variationally, and the W^I / W^II
evolution MPOs that are usually applied that way.

A site visit has no Krylov loop: it is ONE projection of the tensors of the state `above` on the tangent space of the state
`below` (ac_proj / ac2_proj, derivatives.jl:210-226), one gauge step and one mixed transfer.  The projection runs on
mpsk_dAC_proj / mpsk_dAC2_proj (rectangular environments; the two-site form never builds the two-site tensor of `above`) and
the convergence measure on mpsk_vdiff_nrm2.  Backends without these entry points take the composed route (dAC / dAC2 on a
formed two-site tensor, two norms) -- the pattern changebonds uses for dAC2_product.

approximate for InfiniteMPS (src/algorithms/approximate/vomps.jl): the VOMPS power method on the mixed environments of
statmech.PerMPOInfEnv -- per site one ac_proj (mpsk_dAC_proj) and one c_proj (mpsk_dC_proj), then a regauge.  The IDMRG1 / IDMRG2
forms (approximate/idmrg.jl) and complex tensors are not implemented.  An MPSMultiline with (MPOMultiline, MPSMultiline):
multiline.approximate, the same loop over all rows of a column at once."""
from __future__ import annotations

import math
import time
from dataclasses import dataclass

import numpy as np

from .algorithms import DMRG, DMRG2, VOMPS, VUMPS, _log, _no_cplx, _two_site_tensor, regauge, updatetol
from .backend import DTensor
from .environments import FinEnvPair, environments
from .operators import MPOHamiltonian, SparseMPO
from .states import InfiniteMPS
from .statmech import DenseMPO, PerMPOInfEnv, calc_galerkin as _calc_galerkin_mpo


# ---- projections --------------------------------------------------------------------------------------------------

def _sandwich(be, GL: DTensor, x: DTensor, GR: DTensor):
    """GL[0] x GR[0] for pass-through environments (no operator, one slab each): two plain products."""
    Wl, Dlo, Dl = GL.shape
    Wr, Dr, Dro = GR.shape
    t = be.gemm(DTensor(GL.buf, (Dlo, Dl)), x.reshape(Dl, x.size // Dl))
    return be.gemm(t.reshape(t.size // Dr, Dr), DTensor(GR.buf, (Dr, Dro)))


def ac_proj(pos, below, envs, *rest):
    """ac_proj(pos, below, envs)  (derivatives.jl:210-219): dAC of above.AC[pos] with the environments of `below`
    (FinEnvPair, or statmech.PerMPOInfEnv on uniform states).  ac_proj(row, col, below, envs): the two-index form on the
    environments of an MPSMultiline (derivatives.jl:216-219)."""
    if rest:
        row, col, below, envs = pos, below, envs, rest[0]
        return envs.ac_proj(row, col, below)
    if isinstance(envs, PerMPOInfEnv):
        return envs.ac_proj(pos, below)
    be = below.be
    GL, GR = envs.leftenv(pos, below), envs.rightenv(pos, below)
    x, H = envs.above.AC(pos), envs.opp[pos]
    Dlo, d, Dro = GL.shape[1], x.shape[1], GR.shape[2]
    if H is None:
        return _sandwich(be, GL, x, GR).reshape(Dlo, d, Dro)
    if hasattr(be, "dAC_proj"):
        return be.dAC_proj(H, GL, GR, x)
    return be.dAC(H, GL, GR, x, out=be.empty(Dlo, d, Dro))


def c_proj(pos, below, envs, *rest):
    """c_proj(pos, below, envs)  (derivatives.jl:204-207): dC of above.CR[pos] with the environments of `below` (uniform
    states; mpsk_dC_proj).  c_proj(row, col, below, envs): the two-index form on the environments of an MPSMultiline."""
    if rest:
        return rest[0].c_proj(pos, below, envs)
    return envs.c_proj(pos, below)


def ac2_proj(pos, below, envs: FinEnvPair):
    """ac2_proj(pos, below, envs)  (derivatives.jl:220-226): dAC2 of above.AC[pos] * above.AR[pos + 1]; Y[Dlo, d1, Dro, d2]."""
    be = below.be
    GL, GR = envs.leftenv(pos, below), envs.rightenv(pos + 1, below)
    ac, ar = envs.above.AC(pos), envs.above.AR(pos + 1)
    H1, H2 = envs.opp[pos], envs.opp[pos + 1]
    Dlo, Dro = GL.shape[1], GR.shape[2]
    if H1 is None:
        theta = _two_site_tensor(be, ac, ar)                        # [Dl, d1, Dr, d2]: GR acts on the third index
        Dl, d1, Dr, d2 = theta.shape
        t = be.gemm(DTensor(GL.buf, (Dlo, Dl)), theta.reshape(Dl, d1 * Dr * d2))
        out = be.empty(Dlo, d1, Dro, d2)
        for s2 in range(d2):
            be.gemm_raw(False, False, Dlo * d1, Dro, Dr, 1.0, t.ptr + 8 * s2 * Dlo * d1 * Dr, Dlo * d1, GR.ptr, Dr, 0.0,
                        out.ptr + 8 * s2 * Dlo * d1 * Dro, Dlo * d1)
        return out
    if hasattr(be, "dAC2_proj"):
        return be.dAC2_proj(H1, H2, GL, GR, ac, ar)
    theta = _two_site_tensor(be, ac, ar)
    return be.dAC2(H1, H2, GL, GR, theta, out=be.empty(Dlo, theta.shape[1], Dro, theta.shape[3]))


def _rel_change(be, new: DTensor, old: DTensor):
    """norm(new - old) / norm(new)  (fvomps.jl:27, :66)."""
    if hasattr(be, "vdiff_nrm2"):
        d2, n2 = be.vdiff_nrm2(new, old)
        return math.sqrt(max(d2, 0.0) / n2)
    n = be.norm(new)
    diff = be.axpby(-1.0, old, 1.0, be.copy(new))
    return be.norm(diff) / n


def _sum(be, terms):
    acc = terms[0]
    for t in terms[1:]:
        be.axpby(1.0, t, 1.0, acc)
    return acc


# ---- approximate ----------------------------------------------------------------------------------------------------

def approximate(psi0, toapprox, alg, envs=None):
    """approximate(psi0, toapprox, alg[, envs]) -> (psi, envs, eps)  (approximate.jl:1-27, fvomps.jl:1-87).
    toapprox: an (O, above) pair, a bare FiniteMPS, or a list of those (summed); alg: DMRG() (one-site, fixed bond dimension)
    or DMRG2() (two-site, alg's truncation).  envs: what a previous call returned.  eps is the largest relative change of a
    site tensor during the last sweep; the (iteration, eps) pairs of all sweeps are kept as `.history` on every returned
    environment.  Complex states / operators: native_cplx.approximate.
    psi0 an InfiniteMPS: toapprox = (O, above) with O a DenseMPO or a real SparseMPO (make_time_mpo of an infinite
    Hamiltonian), alg = VOMPS() (approximate/vomps.jl; a VUMPS is converted, as the reference's deprecation does); eps is the
    Galerkin error.  psi0 an MPSMultiline: toapprox = (MPOMultiline, MPSMultiline), alg = VOMPS() (multiline.approximate).
    Not implemented for uniform states: IDMRG1 / IDMRG2 (approximate/idmrg.jl), complex tensors."""
    from . import multiline, native_cplx, window
    if isinstance(psi0, window.WindowMPS):
        return window.approximate(psi0, toapprox, alg, envs)
    if isinstance(psi0, native_cplx.NativeInfiniteMPS):
        return native_cplx.approximate(psi0, toapprox, alg, envs)
    if isinstance(psi0, multiline.MPSMultiline):
        return multiline.approximate(psi0, toapprox, alg, envs)
    if isinstance(psi0, InfiniteMPS):
        return _approximate_inf(psi0, toapprox, alg, envs)
    _no_cplx(psi0, "approximate")
    single = not isinstance(toapprox, list)
    squash = [toapprox] if single else list(toapprox)
    for sq in squash:
        _no_cplx(sq[1] if isinstance(sq, tuple) else sq, "approximate")
        if isinstance(sq, tuple) and getattr(sq[0], "cplx", False):
            raise NotImplementedError("approximate with a complex operator: use native_cplx.approximate (interleaved storage)")
    psi = psi0.copy()
    if envs is None:
        envs = [environments(psi, sq) for sq in squash]
    elif single:
        envs = [envs]
    if isinstance(alg, DMRG2):
        psi, envs, eps = _approximate2(psi, squash, alg, envs)
    elif isinstance(alg, DMRG):
        psi, envs, eps = _approximate1(psi, squash, alg, envs)
    else:
        raise TypeError(f"approximate takes DMRG or DMRG2, not {type(alg).__name__}")
    return psi, (envs[0] if single else envs), eps


def _approximate_inf(psi, toapprox, alg, envs=None):  # approximate/vomps.jl:1-80 (one row)
    if isinstance(alg, VUMPS):           # vomps.jl:12-17
        alg = VOMPS(tol=alg.tol, maxiter=alg.maxiter, finalize=alg.finalize, verbosity=alg.verbosity,
                    gauge_tol_min=alg.gauge_tol_min, gauge_tol_max=alg.gauge_tol_max, gauge_tol_factor=alg.gauge_tol_factor,
                    env_tol_min=alg.env_tol_min, env_tol_max=alg.env_tol_max, env_tol_factor=alg.env_tol_factor)
    if not isinstance(alg, VOMPS):
        raise TypeError(f"approximate on an InfiniteMPS takes VOMPS (or VUMPS), not {type(alg).__name__}")
    if not (isinstance(toapprox, tuple) and len(toapprox) == 2 and isinstance(toapprox[0], (DenseMPO, SparseMPO))
            and isinstance(toapprox[1], InfiniteMPS)):
        raise TypeError("approximate on an InfiniteMPS takes (O, above): a DenseMPO or SparseMPO and an InfiniteMPS")
    O, above = toapprox
    if getattr(psi, "cplx", False) or getattr(above, "cplx", False) or getattr(O, "cplx", False):
        raise NotImplementedError("approximate on an InfiniteMPS: complex states / operators are not supported (real fp64 only); "
                                  "native_cplx.NativeInfiniteMPS runs them on interleaved storage (native_cplx.approximate)")
    if len(above) != len(psi):
        raise ValueError(f"unit cells of the states above ({len(above)}) and below ({len(psi)}) differ")
    be, n = psi.be, len(psi)
    envs = environments(psi, toapprox) if envs is None else envs
    eps = _calc_galerkin_mpo(psi, envs)
    t0, history = time.time(), []
    for it in range(1, alg.maxiter + 1):
        newAL = [regauge(be, ac_proj(loc, psi, envs), c_proj(loc, psi, envs)) for loc in range(n)]
        gtol = updatetol(alg.gauge_tol_min, alg.gauge_tol_max, alg.gauge_tol_factor, it, eps)
        psi = InfiniteMPS.from_AL(newAL, psi.CR[n - 1], tol=gtol, be=be)
        envs.recalculate(psi, updatetol(alg.env_tol_min, alg.env_tol_max, alg.env_tol_factor, it, eps))
        if alg.finalize is not None:
            psi, envs = alg.finalize(it, psi, toapprox, envs)
        eps = _calc_galerkin_mpo(psi, envs)
        _finish(alg, "VOMPS", it, eps, t0, history)
        if eps <= alg.tol:
            break
    envs.history = history
    return psi, envs, eps


def _finish(alg, name, it, eps, t0, history):
    history.append((it, eps))
    _log(alg, name, it, float("nan"), eps, t0)


def _approximate1(psi, squash, alg: DMRG, envs):  # fvomps.jl:51-87
    be, L = psi.be, len(psi)
    eps = 2 * alg.tol                    # what is returned when maxiter < 1 (fvomps.jl:13,53)
    t0, history = time.time(), []
    for it in range(1, alg.maxiter + 1):
        eps = 0.0
        for pos in list(range(0, L - 1)) + list(range(L - 1, 0, -1)):
            new = _sum(be, [ac_proj(pos, psi, e) for e in envs])
            eps = max(eps, _rel_change(be, new, psi.AC(pos)))
            psi.set_AC(pos, new)
        if alg.finalize is not None:
            psi, envs = alg.finalize(it, psi, squash, envs)
        _finish(alg, "DMRG", it, eps, t0, history)
        if eps < alg.tol:
            break
    for e in envs:                       # the eps of every sweep, on each environment that is returned (as _dmrg2 keeps its own)
        e.history = history
    return psi, envs, eps


def _approximate2(psi, squash, alg: DMRG2, envs):  # fvomps.jl:11-49
    be, L = psi.be, len(psi)
    eps = 2 * alg.tol                    # what is returned when maxiter < 1 (fvomps.jl:13,53)
    t0, history = time.time(), []
    trunc_err = alg.trunc_err if alg.trunc_dim <= 0 else 0.0
    for it in range(1, alg.maxiter + 1):
        eps = 0.0
        for pos in list(range(0, L - 1)) + list(range(L - 3, -1, -1)):
            new = _sum(be, [ac2_proj(pos, psi, e) for e in envs])
            Dl, d1, Dr, d2 = new.shape
            alm, c, arm, _, _ = be.tsplit(new.reshape(Dl * d1, Dr * d2), max_keep=alg.trunc_dim, trunc_err=trunc_err)
            k = c.shape[0]
            old = _two_site_tensor(be, psi.AC(pos), psi.AR(pos + 1))
            rec = be.gemm(be.gemm(alm, c), arm)                     # al * c * ar
            eps = max(eps, _rel_change_to(be, DTensor(rec.buf, old.shape), old))
            ar = be.empty(k, d2, Dr)                                # ar[k, s2, b] = arm[k, (b, s2)]
            for s2 in range(d2):
                be.copy2d(k, Dr, arm.ptr + 8 * s2 * k * Dr, k, ar.ptr + 8 * s2 * k, k * d2)
            psi.set_AC(pos, (alm.reshape(Dl, d1, k), c))
            psi.set_AC(pos + 1, (c, ar))
        if alg.finalize is not None:
            psi, envs = alg.finalize(it, psi, squash, envs)
        _finish(alg, "DMRG2", it, eps, t0, history)
        if eps < alg.tol:
            break
    for e in envs:                       # the eps of every sweep, on each environment that is returned (as _dmrg2 keeps its own)
        e.history = history
    return psi, envs, eps


def _rel_change_to(be, rec: DTensor, old: DTensor):
    """norm(rec - old) / norm(old)  (fvomps.jl:27: the denominator is the CURRENT two-site tensor)."""
    if hasattr(be, "vdiff_nrm2"):
        d2, n2 = be.vdiff_nrm2(old, rec)
        return math.sqrt(max(d2, 0.0) / n2)
    n = be.norm(old)
    diff = be.axpby(-1.0, old, 1.0, be.copy(rec))
    return be.norm(diff) / n


# ---- make_time_mpo ---------------------------------------------------------------------------------------------------

@dataclass
class WII:  # timeevmpo.jl:3-6
    tol: float = 1e-12
    maxiter: int = 100


@dataclass
class TaylorCluster:  # timeevmpo.jl:8
    N: int = 1


def WI():  # timeevmpo.jl:10
    return TaylorCluster(1)


def _site_matrices(sl, odim, d):
    """the blocks of one slice as d x d matrices (levels of dimension 1), None where there is no block"""
    M = [[None] * odim for _ in range(odim)]
    for (i, j), v in sl.blocks.items():
        if np.isscalar(v):
            M[i][j] = v * np.eye(d)
        else:
            a = np.asarray(v)
            if a.shape[0] != 1 or a.shape[3] != 1:
                raise NotImplementedError("make_time_mpo: MPO levels of dimension 1 only")
            M[i][j] = a[0, :, :, 0]
    return M


def make_time_mpo(H: MPOHamiltonian, dt, alg=None):
    """make_time_mpo(H, dt, alg)  (timeevmpo.jl:12-207): the MPO of exp(tau H), tau = -i dt, to second order in tau per
    application: alg = WII() (arXiv:1407.1832 / 1901.05824, odim - 1 levels) or TaylorCluster(1) == WI().  The result is a
    SparseMPO (both boundary vectors on level 0), stored real when tau is real (dt purely imaginary).  A dt with a real part
    gives a complex SparseMPO, for a finite chain and for an infinite Hamiltonian alike: native_cplx.approximate applies it
    (NativeFiniteMPS; NativeInfiniteMPS with VOMPS)."""
    from scipy.linalg import expm
    alg = WII() if alg is None else alg
    tau = -1j * complex(dt)
    tau = tau.real if tau.imag == 0 else tau
    n, d = H.odim, H.d
    data = []
    for site in range(H.period):
        M = _site_matrices(H[site], n, d)
        Z = np.zeros((d, d))
        g = lambda i, j: Z if M[i][j] is None else M[i][j]
        blk = {}
        if isinstance(alg, WII):  # timeevmpo.jl:150-207
            # the reference multiplies both the C and the B blocks by sqrt(tau); a = sqrt|tau| on C and b = tau / a on B is
            # the same operator in another gauge of the MPO bond (levels >= 1 rescaled by sqrt(tau) / a) and stays real for
            # real tau of either sign
            a = math.sqrt(abs(tau))
            b = tau / a
            D = g(0, n - 1)
            for j in range(1, n - 1):
                for k in range(1, n - 1):
                    G = np.zeros((4 * d, 4 * d), dtype=np.result_type(type(tau), float))
                    for q in range(4):
                        G[q * d:(q + 1) * d, q * d:(q + 1) * d] = tau * D
                    G[d:2 * d, 0:d] = a * g(0, k)
                    G[2 * d:3 * d, 0:d] = b * g(j, n - 1)
                    G[3 * d:, 0:d] = g(j, k)
                    G[3 * d:, d:2 * d] = b * g(j, n - 1)
                    G[3 * d:, 2 * d:3 * d] = a * g(0, k)
                    y = expm(G)[:, 0:d]
                    blk[(0, 0)], blk[(0, k)], blk[(j, 0)], blk[(j, k)] = y[0:d], y[d:2 * d], y[2 * d:3 * d], y[3 * d:]
            if n == 2:
                blk[(0, 0)] = expm(tau * D)
        elif isinstance(alg, TaylorCluster):  # timeevmpo.jl:12-108 for N = 1
            if alg.N != 1:
                raise NotImplementedError("make_time_mpo: TaylorCluster(N) is implemented for N = 1 (WI)")
            S = [[None if M[i][j] is None else M[i][j].astype(np.result_type(type(tau), float)) for j in range(n)]
                 for i in range(n)]
            top = n - 1
            for ia in range(n):           # embed the next order (:27-43)
                for ib in range(1, n):
                    if ia == top:
                        continue
                    n3, n1 = (ib == top) + 1, (ia == 0) + 1
                    for e_b in ((ib, top), (top, ib)):
                        for e_a in ((ia, 0), (0, ia)):
                            if S[e_a[0]][e_b[0]] is None or S[e_a[1]][e_b[1]] is None:
                                continue
                            add = S[e_a[1]][e_b[1]] @ S[e_a[0]][e_b[0]] * (tau / (2 * n1 * n3))
                            S[ia][ib] = add if S[ia][ib] is None else S[ia][ib] + add
            for i in range(top):          # loopback (:46-55): the finished level feeds the start level, then is dropped
                if S[i][top] is not None:
                    S[i][0] = tau * S[i][top] if S[i][0] is None else S[i][0] + tau * S[i][top]
            for i in range(top):
                for j in range(top):
                    if S[i][j] is not None:
                        blk[(i, j)] = S[i][j]
        else:
            raise TypeError(f"make_time_mpo takes WII or TaylorCluster, not {type(alg).__name__}")
        data.append(blk)
    return SparseMPO(data, d, be=H.be)
