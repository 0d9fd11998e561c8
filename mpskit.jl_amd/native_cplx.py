"""complex128 finite MPS on INTERLEAVED storage: states, environments and the one-site drivers entirely on the MPSK_C128 entry
points of the C ABI (include/mpsk.h) -- mpsk_hac_* / mpsk_dC / mpsk_transfer_* (native complex kernels) and, since round 3,
mpsk_qrpos / mpsk_lqpos / mpsk_gemm under mpsk_ctx_set_dtype(MPSK_C128).  A site tensor A[Dl, d, Dr] of complex numbers is ONE
device buffer of 2 Dl d Dr doubles in Julia's Array{ComplexF64} layout (shape (2 Dl, d, Dr) as a real tensor): 2x the memory of
a real state, where the bond-embedded states of cplx.py take 4x and run their transfers at 8x the real flops.

This module is the proof that a complex host needs nothing but the C ABI (it is what a Julia `ROCTensor{ComplexF64}` backend
would do): the state is kept in explicit mixed-canonical form (sites left of the centre left-orthonormal,
right of it right-orthonormal), which is all the one-site algorithms need --
    find_groundstate (DMRG, dmrg.jl:22-55)   ->  NativeFiniteMPS + dmrg_sweep / dmrg
    find_groundstate (DMRG2, dmrg.jl:80-137) ->  dmrg2_sweep   (mpsk_dAC2 complex, mpsk_tsplit under MPSK_C128)
    timestep (TDVP, tdvp.jl:61-94)           ->  tdvp_step
    timestep (TDVP2, tdvp.jl:113-146)        ->  tdvp2_step
    approximate (fvomps.jl:11-87)            ->  approximate   (mpsk_dAC_proj / mpsk_dAC2_proj complex, NativeFinEnvPair)
    approximate (approximate/vomps.jl)       ->  approximate on a NativeInfiniteMPS (uniform state, second half of this file:
                                                 mpsk_dAC_proj / mpsk_dC_proj_c, NativePerMPOInfEnv, VOMPS)
The lazy-gauge FiniteMPS of states.py (all drivers, two-site algorithms, infinite systems, excitations) stays on the embedded
representation; the Krylov solvers are shared (real inner products on the 2n doubles of an interleaved vector are all a
Hermitian Lanczos / Arnoldi iteration needs, and multiplication by i is mpsk_vtimes_i)."""
from __future__ import annotations

import os

import numpy as np

from .backend import Backend, DTensor
from . import krylov
from .cplx import HalfEmbeddedOp
from .environments import MPOHamInfEnv


def _mat(t: DTensor, rows2, cols):
    return t.reshape(rows2, cols)


class NativeFiniteMPS:
    """finite MPS with interleaved complex128 site tensors in mixed-canonical form around `center` (which holds AC)."""

    def __init__(self, tensors, be: Backend, normalize=True):
        self.be = be
        self.A = [be.upload_c(np.asarray(t, dtype=np.complex128)) for t in tensors]     # (2 Dl, d, Dr) each
        self.N = len(self.A)
        self.center = self.N - 1
        for i in range(self.N - 1, 0, -1):                     # right-canonicalise: A_i = L Q, A_{i-1} <- A_{i-1} L
            self._shift_left(i)
        if normalize:
            be.scal(1.0 / be.norm(self.A[0]), self.A[0])

    def __len__(self):
        return self.N

    def dims(self, i):
        Dl2, d, Dr = self.A[i].shape
        return Dl2 // 2, d, Dr

    def _shift_right(self, i):
        """centre i -> i + 1:  AC_i = AL C (QRpos),  AC_{i+1} = C AR_{i+1}   (orthoview.jl:49-60, :99)"""
        be = self.be
        Dl, d, Dr = self.dims(i)
        Q, R = be.qrpos_c(_mat(self.A[i], 2 * Dl * d, Dr))
        k = R.shape[1]
        self.A[i] = Q.reshape(2 * Dl, d, k)
        Dn, dn, Drn = self.dims(i + 1)
        nxt = be.gemm_c(R, _mat(self.A[i + 1], 2 * Dn, dn * Drn))
        self.A[i + 1] = nxt.reshape(2 * k, dn, Drn)
        self.center = i + 1
        return R

    def _shift_left(self, i):
        """centre i -> i - 1:  AC_i = C AR (LQpos),  AC_{i-1} = AL_{i-1} C   (orthoview.jl:61-72, :103)"""
        be = self.be
        Dl, d, Dr = self.dims(i)
        Lm, Q = be.lqpos_c(_mat(self.A[i], 2 * Dl, d * Dr))
        k = Lm.shape[1]
        self.A[i] = Q.reshape(2 * k, d, Dr)
        Dp, dp, Drp = self.dims(i - 1)
        prv = be.gemm_c(_mat(self.A[i - 1], 2 * Dp * dp, Drp), Lm)
        self.A[i - 1] = prv.reshape(2 * Dp, dp, k)
        self.center = i - 1
        return Lm

    def move_center(self, pos):
        while self.center < pos:
            self._shift_right(self.center)
        while self.center > pos:
            self._shift_left(self.center)

    def norm(self):
        return self.be.norm(self.A[self.center])

    def to_host(self):
        """complex host tensors (mixed-canonical around the current centre)."""
        return [self.be.download_c(t) for t in self.A]

    def bytes(self):
        return 8 * sum(t.size for t in self.A)

    def copy(self):
        out = object.__new__(NativeFiniteMPS)
        out.be, out.N, out.center = self.be, self.N, self.center
        out.A = [self.be.copy(t) for t in self.A]
        return out

    # ---- linear algebra (finitemps.jl:365-469; linalg.py: the composed route on gemm_c / qrpos_c / lqpos_c) ----
    __array_ufunc__ = None

    def __add__(self, other):
        from . import linalg
        return linalg.add(self, other) if isinstance(other, NativeFiniteMPS) else NotImplemented

    def __sub__(self, other):
        from . import linalg
        return linalg.sub(self, other) if isinstance(other, NativeFiniteMPS) else NotImplemented

    def __mul__(self, a):
        from . import linalg
        return linalg.scale(self, a) if isinstance(a, (int, float, complex, np.number)) else NotImplemented

    __rmul__ = __mul__

    def __neg__(self):
        return self * -1.0

    def normalize(self):
        from . import linalg
        return linalg.normalize_(self)

    def dot(self, other):
        from . import linalg
        return linalg.dot(self, other)


class ComplexMPOHamiltonian:
    """MPOHamiltonian with ComplexF64 entries (mpohamiltonian.jl:8-31): a periodic list of MPSK_C128 slices.  `data[site]` =
    {(i, j): scalar | d x d | [chi_i, d, d, chi_j]} with complex values, levels 0 .. odim - 1, H[0, 0] = H[odim-1, odim-1] = 1.
    (The real MPOHamiltonian of operators.py is accepted by the drivers as well: its slices get complex twins.)"""

    def __init__(self, data, be: Backend, d=None):
        if isinstance(data, dict):
            data = [data]
        self.be, self.period = be, len(data)
        self.odim = 1 + max(max(i, j) for blk in data for (i, j) in blk)
        for blk in data:
            for v in blk.values():
                if d is None and not np.isscalar(v):
                    a = np.asarray(v)
                    d = a.shape[0] if a.ndim == 2 else a.shape[1]
        self.d = int(d)
        chis = [[1] * self.odim for _ in range(self.period + 1)]
        for s_, blk in enumerate(data):
            for (i, j), v in blk.items():
                if not np.isscalar(v) and np.asarray(v).ndim == 4:
                    chis[s_][i], chis[s_ + 1][j] = np.asarray(v).shape[0], np.asarray(v).shape[3]
        for i in range(self.odim):
            chis[0][i] = chis[self.period][i] = max(chis[0][i], chis[self.period][i])
        self.chis, self.slices = chis, []
        for s_, blk in enumerate(data):
            blocks = {}
            for (i, j), v in blk.items():
                if np.isscalar(v):
                    if v != 0:
                        blocks[(i, j)] = complex(v)
                    continue
                a = np.asarray(v, dtype=np.complex128)
                blocks[(i, j)] = a[None, :, :, None] if a.ndim == 2 else a
            self.slices.append(be.mposlice(self.odim, self.d, chis[s_], chis[s_ + 1], blocks, cplx=True))

    def __getitem__(self, i):
        return self.slices[i % self.period]

    def __len__(self):
        return self.period

    def isid(self, i):  # mpohamiltonian.jl:53-58
        return all(s.isscal(i, i) and abs(s.blocks[(i, i)] - 1) < 1e-14 for s in self.slices)

    def contains(self, site, i, j):
        """whether block (i, j) of the slice of `site` is present; the block itself is self[site].blocks[(i, j)]"""
        return self[site].contains(i, j)


def _boundary(be, chis, D, active):
    """FinEnv.jl:49-67: identity on the active level, zeros elsewhere -- complex interleaved slabs (W, 2 D, D)."""
    blocks = []
    for i, chi in enumerate(chis):
        b = np.zeros((D, chi, D), dtype=np.complex128)
        if i == active:
            for k in range(chi):
                b[:, k, :] = np.eye(D)
        blocks.append(b)
    return be.upload_env_c(blocks)


class NativeFinEnv:
    """left / right environments of a NativeFiniteMPS (FinEnv.jl:9-145), interleaved complex slabs (W, 2 Dbra, Dket); valid
    for sites strictly left / right of the centre and refreshed as the centre moves (the drivers below move it one site at
    a time and call `extend_left` / `extend_right`)."""

    def __init__(self, psi: NativeFiniteMPS, H):
        be = self.be = psi.be
        L = self.L = len(psi)
        if isinstance(H, ComplexMPOHamiltonian):
            self.opp = [H[i] for i in range(L)]
            chil, chir = H.chis[0], H.chis[(L - 1) % H.period + 1]
        else:                                                   # real MPOHamiltonian: complex twins of its slices
            self.opp = [HalfEmbeddedOp._cslice(be, H[i]) for i in range(L)]
            chil, chir = H[0].chil, H[L - 1].chir
        odim = H.odim
        self.GL = [_boundary(be, chil, psi.dims(0)[0], 0)] + [None] * L
        self.GR = [None] * L + [_boundary(be, chir, psi.dims(L - 1)[2], odim - 1)]
        self.n_transfers = 0
        c = psi.center
        for j in range(L - 1, c, -1):
            self.extend_right(psi, j)
        for j in range(0, c):
            self.extend_left(psi, j)

    def extend_left(self, psi, j):
        """GL[j + 1] from GL[j] and the left-orthonormal A[j]  (FinEnv.jl:131-145, transfer.jl:105-110)"""
        self.GL[j + 1] = self.be.transfer_left(self.opp[j], self.GL[j], psi.A[j], psi.A[j])
        self.n_transfers += 1

    def extend_right(self, psi, j):
        """GR[j] from GR[j + 1] and the right-orthonormal A[j]  (FinEnv.jl:114-129)"""
        self.GR[j] = self.be.transfer_right(self.opp[j], self.GR[j + 1], psi.A[j], psi.A[j])
        self.n_transfers += 1

    def bytes(self):
        return 8 * sum(t.size for t in self.GL + self.GR if t is not None)


def _sum_terms(H):
    """(operators, prefactors) of a LazySum / MultipliedOperator, None for a plain operator."""
    from .operators import LazySum, MultipliedOperator
    if isinstance(H, LazySum):
        return list(H), list(H._fs)
    if isinstance(H, MultipliedOperator):
        return [H.op], [H.f]
    return None


class NativeMultipleEnv:
    """MultipleEnvironments (multipleenv.jl) for interleaved states: one NativeFinEnv per term of a LazySum (or the one of a
    MultipliedOperator), moved together; `fs` are the prefactors, numbers or functions of time.  The environments of a
    NativeFiniteMPS are canonical, so the one-site generator of the sum is the folded mpsk_hsum (MPSK_HAC_CANONICAL_C128)."""

    def __init__(self, psi: NativeFiniteMPS, H):
        ops, self.fs = _sum_terms(H)
        self.be, self.H = psi.be, H
        self.envs = [NativeFinEnv(psi, o) for o in ops]
        self.timed = any(callable(f) for f in self.fs)
        self.routes = set()              # routes the device-side sums took so far (mpsk_hsum_info), for inspection

    def extend_left(self, psi, j):
        for e in self.envs:
            e.extend_left(psi, j)

    def extend_right(self, psi, j):
        for e in self.envs:
            e.extend_right(psi, j)

    @property
    def n_transfers(self):
        return sum(e.n_transfers for e in self.envs)

    def coefs(self, t):
        if self.timed and t is None:
            raise ValueError("a time-dependent sum needs its time")
        cs = [f(t) if callable(f) else f for f in self.fs]
        if any(complex(c).imag != 0.0 for c in cs):
            raise NotImplementedError("complex-valued prefactors f(t) on interleaved states are not implemented")
        return [complex(c).real for c in cs]


class _SumOp:
    """sum_k c_k op_k(x) at fixed real numbers c_k, term by term, on interleaved vectors."""

    def __init__(self, be, ops, coefs):
        self.be, self.ops, self.coefs, self._tmp = be, ops, coefs, None

    def __call__(self, x, out=None):
        be = self.be
        y = self.ops[0](x, out=out)
        if self.coefs[0] != 1.0:
            be.scal(self.coefs[0], y)
        for c, op in zip(self.coefs[1:], self.ops[1:]):
            if self._tmp is None or self._tmp.shape != y.shape:
                self._tmp = be.empty(*y.shape)
            be.axpby(c, op(x, out=self._tmp), 1.0, y)
        return y


def _eval_time(t, dt, frac):
    """t + frac dt, a float when it is real (integrators.jl:20-25: the midpoint of the sub-step)"""
    te = complex(t) + frac * complex(dt)
    return te.real if te.imag == 0.0 else te


def _gen_ac(be, envs, pos, te):
    """H_AC of site pos at the evaluation time te"""
    if not isinstance(envs, NativeMultipleEnv):
        return _HAC(be, envs, pos)
    cs = envs.coefs(te)
    es = envs.envs
    if hasattr(be, "hsum_create") and len(es) <= 8 and os.environ.get("MPSK_HSUM", "1") != "0":
        h = be.hsum_create([e.opp[pos] for e in es], [e.GL[pos] for e in es], [e.GR[pos + 1] for e in es],
                           canonical_c128=True)
        h.set_coefs(cs)
        envs.routes.add(h.info()["route"])
        return lambda x, out=None: h.apply(x, out=out)
    return _SumOp(be, [_HAC(be, e, pos) for e in es], cs)


def _gen_c(be, envs, GLi, GRi, te):
    """H_C on the bond whose environments are GL[GLi] and GR[GRi]"""
    def one(e):
        hc = _HC.__new__(_HC)
        hc.be, hc.GL, hc.GR = be, e.GL[GLi], e.GR[GRi]
        return hc
    if not isinstance(envs, NativeMultipleEnv):
        return one(envs)
    return _SumOp(be, [one(e) for e in envs.envs], envs.coefs(te))


def _gen_ac2(be, envs, pos, te):
    def one(e):
        h1, h2, GL, GR = e.opp[pos], e.opp[pos + 1], e.GL[pos], e.GR[pos + 2]
        return lambda x, out=None: be.dAC2(h1, h2, GL, GR, x, out=out)
    if not isinstance(envs, NativeMultipleEnv):
        return one(envs)
    return _SumOp(be, [one(e) for e in envs.envs], envs.coefs(te))


class _HAC:
    """H_AC of the centre site on interleaved vectors (derivatives.jl:77-93): prepared operator, one call per application."""

    def __init__(self, be, envs, pos):
        self.h = be.hac_create(envs.opp[pos], envs.GL[pos], envs.GR[pos + 1])

    def __call__(self, x, out=None):
        return self.h.apply(x, out=out)


class _HC:
    """H_C of the bond right of site pos (derivatives.jl:3-31)."""

    def __init__(self, be, envs, pos):
        self.be, self.GL, self.GR = be, envs.GL[pos + 1], envs.GR[pos + 1]

    def __call__(self, x, out=None):
        return self.be.dC(self.GL, self.GR, x, out=out, cplx=True)


def energy(psi: NativeFiniteMPS, envs: NativeFinEnv, t=None):
    """<psi|H|psi> / <psi|psi> at the current centre (Re <AC, H_AC AC>; the imaginary part vanishes for Hermitian H).
    t: the time of a time-dependent sum (NativeMultipleEnv)."""
    be = psi.be
    ac = psi.A[psi.center]
    return be.dot(ac, _gen_ac(be, envs, psi.center, t)(ac)) / be.dot(ac, ac)


def dmrg_sweep(psi: NativeFiniteMPS, H, envs: NativeFinEnv, eigalg, ws=None):
    """One DMRG sweep, pos in [1:L-1; L:-1:2] (dmrg.jl:33-38): eigsolve with H_AC at the centre, QRpos / LQpos to the next
    site, one environment transfer.  Starts and ends with the centre at site 0.  Returns the energy after the sweep."""
    be, L = psi.be, len(psi)
    ws = krylov.KrylovWorkspace(be) if ws is None else ws
    psi.move_center(0)

    def solve(pos):
        h = _HAC(be, envs, pos)
        _, vec, _, _ = krylov.eigsolve_sr(be, h, psi.A[pos], tol=eigalg.tol, krylovdim=eigalg.krylovdim,
                                          maxiter=eigalg.maxiter, fixed_matvecs=eigalg.fixed_matvecs, ws=ws)
        psi.A[pos] = vec

    for pos in range(0, L - 1):
        solve(pos)
        psi._shift_right(pos)
        envs.extend_left(psi, pos)
    for pos in range(L - 1, 0, -1):
        solve(pos)
        psi._shift_left(pos)
        envs.extend_right(psi, pos)
    return energy(psi, envs)


def dmrg(psi: NativeFiniteMPS, H, eigalg, maxiter=10, tol=1e-10, envs=None, verbose=False):
    """find_groundstate(psi, H, DMRG(...)) on interleaved complex storage: sweeps until the energy change is below tol."""
    envs = NativeFinEnv(psi, H) if envs is None else envs
    ws = krylov.KrylovWorkspace(psi.be)
    E_old, log = np.inf, []
    for it in range(1, maxiter + 1):
        E = dmrg_sweep(psi, H, envs, eigalg, ws)
        log.append((it, E))
        if verbose:
            print(f"DMRG (native complex) {it:3d}: obj = {E:+.12e}")
        if abs(E - E_old) <= tol * max(1.0, abs(E)):
            break
        E_old = E
    return psi, envs, log


def tdvp_step(psi: NativeFiniteMPS, H, envs: NativeFinEnv, t, dt, alg, ws=None):
    """timestep!(psi, H, t, dt, TDVP())  (tdvp.jl:61-94): forward integration of AC by dt / 2, backward integration of the bond
    matrix, left to right and back; any complex dt (real time: exp(-i dt H))."""
    from .algorithms import _integrate_embedded
    be, L = psi.be, len(psi)
    ws = krylov.KrylovWorkspace(be) if ws is None else ws
    psi.move_center(0)
    fwd, bwd = -1j * complex(dt) / 2, 1j * complex(dt) / 2
    # evaluation times of a time-dependent generator (tdvp.jl:61-91 through integrators.jl:20-25)
    t_ac1, t_c1, t_ac2, t_c2 = (_eval_time(t, dt, f) for f in (0.25, -0.25, 0.75, 0.25))
    for i in range(L - 1):
        psi.A[i] = _integrate_embedded(be, _gen_ac(be, envs, i, t_ac1), psi.A[i], fwd, alg, ws)
        Dl, d, Dr = psi.dims(i)
        Q, R = be.qrpos_c(_mat(psi.A[i], 2 * Dl * d, Dr))
        psi.A[i] = Q.reshape(2 * Dl, d, R.shape[1])
        envs.extend_left(psi, i)
        C = _integrate_embedded(be, _gen_c(be, envs, i + 1, i + 1, t_c1), R, bwd, alg, ws)
        Dn, dn, Drn = psi.dims(i + 1)
        psi.A[i + 1] = be.gemm_c(C, _mat(psi.A[i + 1], 2 * Dn, dn * Drn)).reshape(2 * C.shape[0] // 2, dn, Drn)
        psi.center = i + 1
    psi.A[L - 1] = _integrate_embedded(be, _gen_ac(be, envs, L - 1, t_ac1), psi.A[L - 1], fwd, alg, ws)
    for i in range(L - 1, 0, -1):
        psi.A[i] = _integrate_embedded(be, _gen_ac(be, envs, i, t_ac2), psi.A[i], fwd, alg, ws)
        Dl, d, Dr = psi.dims(i)
        Lm, Q = be.lqpos_c(_mat(psi.A[i], 2 * Dl, d * Dr))
        psi.A[i] = Q.reshape(2 * Lm.shape[1], d, Dr)
        envs.extend_right(psi, i)
        # the bond matrix between i - 1 and i: H_C with GL[i] and GR[i]
        C = _integrate_embedded(be, _gen_c(be, envs, i, i, t_c2), Lm, bwd, alg, ws)
        Dp, dp, Drp = psi.dims(i - 1)
        psi.A[i - 1] = be.gemm_c(_mat(psi.A[i - 1], 2 * Dp * dp, Drp), C).reshape(2 * Dp, dp, C.shape[1])
        psi.center = i - 1
    psi.A[0] = _integrate_embedded(be, _gen_ac(be, envs, 0, t_ac2), psi.A[0], fwd, alg, ws)
    return psi, envs


def _two_site(be, left: DTensor, right: DTensor):
    """theta[a, s1, b, s2] = sum_m left[a, s1, m] right[m, s2, b] on interleaved tensors (dmrg.jl:92 / :108): d2 complex GEMMs
    on strided views of `right` (mpsk_gemm under MPSK_C128; leading dimensions and offsets in complex elements)."""
    Dl, d1, Dm = left.shape[0] // 2, left.shape[1], left.shape[2]
    _, d2, Dr = right.shape
    theta = be.empty(2 * Dl, d1, Dr, d2)
    be._set_dtype(True)
    try:
        for s2 in range(d2):
            be.gemm_raw(False, False, Dl * d1, Dr, Dm, 1.0, left.ptr, Dl * d1, right.ptr + 16 * s2 * Dm, Dm * d2, 0.0,
                        theta.ptr + 16 * s2 * Dl * d1 * Dr, Dl * d1)
    finally:
        be._set_dtype(False)
    return theta


def _split(be, theta, trunc_dim, trunc_err):
    # trunc_err is passed only when set: the truncdim call stays exactly what it was
    if trunc_err:
        return be.tsplit_c(theta, max_keep=trunc_dim, trunc_err=trunc_err)
    return be.tsplit_c(theta, max_keep=trunc_dim)


def dmrg2_sweep(psi: NativeFiniteMPS, H, envs: NativeFinEnv, eigalg, trunc_dim, ws=None, trunc_err=0.0):
    """One two-site DMRG sweep (dmrg.jl:86-120) on interleaved storage: theta = AC AR, eigsolve with H_AC2 (mpsk_dAC2 complex),
    al, c, ar = tsvd!(theta; trunc) through mpsk_tsplit under MPSK_C128 (truncdim(trunc_dim); truncerr(trunc_err) when that is
    nonzero, through the native complex SVD), normalize!(c).  Centre at site 0 before and after.  Returns the energy after the
    sweep."""
    be, L = psi.be, len(psi)
    ws = krylov.KrylovWorkspace(be) if ws is None else ws
    psi.move_center(0)

    def update(pos, theta):
        h1, h2, GL, GR = envs.opp[pos], envs.opp[pos + 1], envs.GL[pos], envs.GR[pos + 2]
        op = lambda x, out=None: be.dAC2(h1, h2, GL, GR, x, out=out)
        _, new, _, _ = krylov.eigsolve_sr(be, op, theta, tol=eigalg.tol, krylovdim=eigalg.krylovdim, maxiter=eigalg.maxiter,
                                          fixed_matvecs=eigalg.fixed_matvecs, ws=ws)
        Dl2, d1, Dr, d2 = new.shape
        al, c, arm, _, _ = _split(be, new.reshape(Dl2 * d1, Dr * d2), trunc_dim, trunc_err)
        k = c.shape[1]
        be.scal(1.0 / be.norm(c), c)                                     # normalize!(c)
        ar = be.empty(2 * k, d2, Dr)                                     # ar[k, s2, b] = arm[k, (b, s2)]
        for s2 in range(d2):
            be.copy2d(2 * k, Dr, arm.ptr + 8 * s2 * 2 * k * Dr, 2 * k, ar.ptr + 8 * s2 * 2 * k, 2 * k * d2)
        return al.reshape(Dl2, d1, k), c, ar

    for pos in range(0, L - 1):
        al, c, ar = update(pos, _two_site(be, psi.A[pos], psi.A[pos + 1]))
        k, d2, Dr = c.shape[1], ar.shape[1], ar.shape[2]
        psi.A[pos] = al
        psi.A[pos + 1] = be.gemm_c(c, ar.reshape(2 * k, d2 * Dr)).reshape(2 * k, d2, Dr)      # AC_{pos+1} = c ar
        psi.center = pos + 1
        envs.extend_left(psi, pos)
    for pos in range(L - 2, -1, -1):
        al, c, ar = update(pos, _two_site(be, psi.A[pos], psi.A[pos + 1]))
        Dl2, d1, k = al.shape
        psi.A[pos + 1] = ar
        psi.A[pos] = be.gemm_c(al.reshape(Dl2 * d1, k), c).reshape(Dl2, d1, k)                # AC_pos = al c
        psi.center = pos
        envs.extend_right(psi, pos + 1)
    return energy(psi, envs)


def tdvp2_step(psi: NativeFiniteMPS, H, envs: NativeFinEnv, t, dt, alg, trunc_dim, ws=None, trunc_err=0.0):
    """timestep!(psi, H, t, dt, TDVP2(truncdim(D)))  (tdvp.jl:113-146) on interleaved storage: two-site tensors integrated
    forward by dt / 2 and split (mpsk_tsplit under MPSK_C128; NO normalisation of c: the evolution is unitary), the new
    centre integrated backward, left to right and back."""
    from .algorithms import _integrate_embedded
    be, L = psi.be, len(psi)
    ws = krylov.KrylovWorkspace(be) if ws is None else ws
    psi.move_center(0)
    fwd, bwd = -1j * complex(dt) / 2, 1j * complex(dt) / 2
    # evaluation times of a time-dependent generator (tdvp.jl:113-146 through integrators.jl:20-25)
    t_f2, t_f1, t_b2, t_b1 = (_eval_time(t, dt, f) for f in (0.25, -0.25, 0.75, 0.25))

    def evolve_and_split(pos, theta, te):
        new = _integrate_embedded(be, _gen_ac2(be, envs, pos, te), theta, fwd, alg, ws)
        Dl2, d1, Dr, d2 = new.shape
        al, c, arm, _, _ = _split(be, new.reshape(Dl2 * d1, Dr * d2), trunc_dim, trunc_err)
        k = c.shape[1]
        ar = be.empty(2 * k, d2, Dr)
        for s2 in range(d2):
            be.copy2d(2 * k, Dr, arm.ptr + 8 * s2 * 2 * k * Dr, 2 * k, ar.ptr + 8 * s2 * 2 * k, 2 * k * d2)
        return al.reshape(Dl2, d1, k), c, ar

    for i in range(L - 1):
        al, c, ar = evolve_and_split(i, _two_site(be, psi.A[i], psi.A[i + 1]), t_f2)
        k, d2, Dr = c.shape[1], ar.shape[1], ar.shape[2]
        psi.A[i] = al
        psi.A[i + 1] = be.gemm_c(c, ar.reshape(2 * k, d2 * Dr)).reshape(2 * k, d2, Dr)
        psi.center = i + 1
        envs.extend_left(psi, i)
        if i != L - 2:
            psi.A[i + 1] = _integrate_embedded(be, _gen_ac(be, envs, i + 1, t_f1), psi.A[i + 1], bwd, alg, ws)
    for i in range(L - 1, 0, -1):
        al, c, ar = evolve_and_split(i - 1, _two_site(be, psi.A[i - 1], psi.A[i]), t_b2)
        Dl2, d1, k = al.shape
        psi.A[i] = ar
        psi.A[i - 1] = be.gemm_c(al.reshape(Dl2 * d1, k), c).reshape(Dl2, d1, k)
        psi.center = i - 1
        envs.extend_right(psi, i)
        if i != 1:
            psi.A[i - 1] = _integrate_embedded(be, _gen_ac(be, envs, i - 1, t_b1), psi.A[i - 1], bwd, alg, ws)
    return psi, envs


# ---- approximate on interleaved storage (approximate.jl:1-27, fvomps.jl:1-87) -----------------------------------------------

def _boundary_pair(be, chis, D1, D2, active):
    """_boundary for two states: slabs [D1, D2], the (rectangular) identity on the active level."""
    blocks = []
    for i, chi in enumerate(chis):
        b = np.zeros((D1, chi, D2), dtype=np.complex128)
        if i == active:
            b[:, :, :] = np.eye(D1, D2)[:, None, :]
        blocks.append(b)
    return be.upload_env_c(blocks)


class NativeFinEnvPair:
    """Pair form of NativeFinEnv (FinEnv.jl:21-70 with `above`): environments of <below| O |above> as interleaved complex
    slabs, GL[j] (W, 2 D_below, D_above) left of site j and GR[j] (W, 2 D_above, D_below) right of site j - 1.  It keeps its
    own copy of `above` and moves that copy's centre together with the centre of `below`, so that at centre c the copy
    holds AL (sites < c), AC (site c) and AR (sites > c) of the state above.  O: a SparseMPO (real or complex; right
    boundary on level 0, FinEnv.jl:61), a ComplexMPOHamiltonian or a real MPOHamiltonian (level odim - 1); real slices get
    complex twins."""

    def __init__(self, below: NativeFiniteMPS, O, above: NativeFiniteMPS):
        from .operators import SparseMPO
        be = self.be = below.be
        L = self.L = len(below)
        if len(above) != L:
            raise ValueError(f"the two states have different lengths ({L} != {len(above)})")
        native = isinstance(O, ComplexMPOHamiltonian) or (isinstance(O, SparseMPO) and O.cplx)
        self.opp = [O[i] if native else HalfEmbeddedOp._cslice(be, O[i]) for i in range(L)]
        ract = 0 if isinstance(O, SparseMPO) else O.odim - 1
        self.above = above.copy()
        self.above.move_center(below.center)
        self.GL = [_boundary_pair(be, self.opp[0].chil, below.dims(0)[0], above.dims(0)[0], 0)] + [None] * L
        self.GR = [None] * L + [_boundary_pair(be, self.opp[L - 1].chir, above.dims(L - 1)[2], below.dims(L - 1)[2], ract)]
        self.n_transfers = 0
        c = below.center
        for j in range(L - 1, c, -1):
            self.extend_right(below, j)
        for j in range(0, c):
            self.extend_left(below, j)

    def extend_left(self, psi, j):
        self.GL[j + 1] = self.be.transfer_left(self.opp[j], self.GL[j], self.above.A[j], psi.A[j])
        self.n_transfers += 1

    def extend_right(self, psi, j):
        self.GR[j] = self.be.transfer_right(self.opp[j], self.GR[j + 1], self.above.A[j], psi.A[j])
        self.n_transfers += 1

    def move_center(self, psi, pos):
        """move the centre of `psi` and of the copy of `above` to pos, one site at a time, with one mixed transfer each"""
        while psi.center < pos:
            j = psi.center
            psi._shift_right(j)
            self.above._shift_right(j)
            self.extend_left(psi, j)
        while psi.center > pos:
            j = psi.center
            psi._shift_left(j)
            self.above._shift_left(j)
            self.extend_right(psi, j)


def _rel_diff(be, x: DTensor, y: DTensor):
    """norm(x - y) / norm(x) of two interleaved tensors (mpsk_vdiff_nrm2 on their doubles)"""
    d2, n2 = be.vdiff_nrm2(x, y)
    return float(np.sqrt(max(d2, 0.0) / n2))


def approximate(psi0, toapprox, alg, envs=None, device=None):
    """approximate(psi0, (O, above), DMRG(...) | DMRG2(...)) on interleaved complex states (fvomps.jl:11-87): every site visit
    is one mpsk_dAC_proj / mpsk_dAC2_proj under MPSK_C128, one complex gauge step and one mixed transfer.  O may be the
    complex SparseMPO of a real-time make_time_mpo.  Returns (psi, envs, eps) with eps of the last sweep as in the
    reference; the eps of every sweep is kept in envs.history.
    psi0 a NativeInfiniteMPS: approximate(psi0, (O, above), VOMPS(...)) (approximate/vomps.jl), per site one mpsk_dAC_proj, one
    mpsk_dC_proj_c (device: the route of c_proj, see NativePerMPOInfEnv), a regauge; eps is the Galerkin error."""
    from .algorithms import DMRG, DMRG2
    if isinstance(psi0, NativeInfiniteMPS):
        return _approximate_inf(psi0, toapprox, alg, envs, device=device)
    O, above = toapprox
    be, L = psi0.be, len(psi0)
    psi = psi0.copy()
    psi.move_center(0)
    if envs is None:
        envs = NativeFinEnvPair(psi, O, above)
    else:
        envs.move_center(psi, 0)
    ab, opp = envs.above, envs.opp
    if isinstance(alg, DMRG2):
        trunc_err = alg.trunc_err if alg.trunc_dim <= 0 else 0.0

        def visit(pos, forward):
            envs.move_center(psi, pos)
            y = be.dAC2_proj(opp[pos], opp[pos + 1], envs.GL[pos], envs.GR[pos + 2], ab.A[pos], ab.A[pos + 1])
            Dl2, d1, Dr, d2 = y.shape
            al, c, arm, _, _ = _split(be, y.reshape(Dl2 * d1, Dr * d2), alg.trunc_dim, trunc_err)
            k = c.shape[1]
            old = _two_site(be, psi.A[pos], psi.A[pos + 1])
            rec = be.gemm_c(be.gemm_c(al, c), arm)                                       # al * c * ar
            e = _rel_diff(be, old, DTensor(rec.buf, old.shape))
            ar = be.empty(2 * k, d2, Dr)                                                 # ar[k, s2, b] = arm[k, (b, s2)]
            for s2 in range(d2):
                be.copy2d(2 * k, Dr, arm.ptr + 8 * s2 * 2 * k * Dr, 2 * k, ar.ptr + 8 * s2 * 2 * k, 2 * k * d2)
            if forward:                                                                  # centre moves to pos + 1
                psi.A[pos] = al.reshape(Dl2, d1, k)
                psi.A[pos + 1] = be.gemm_c(c, ar.reshape(2 * k, d2 * Dr)).reshape(2 * k, d2, Dr)
                psi.center = pos + 1
                ab._shift_right(pos)
                envs.extend_left(psi, pos)
            else:                                                                        # centre stays at pos
                psi.A[pos] = be.gemm_c(al, c).reshape(Dl2, d1, k)
                psi.A[pos + 1] = ar
                envs.extend_right(psi, pos + 1)
            return e
        order = [(p, True) for p in range(0, L - 1)] + [(p, False) for p in range(L - 3, -1, -1)]
    elif isinstance(alg, DMRG):
        def visit(pos, forward):
            envs.move_center(psi, pos)
            new = be.dAC_proj(opp[pos], envs.GL[pos], envs.GR[pos + 1], ab.A[pos])
            e = _rel_diff(be, new, psi.A[pos])
            psi.A[pos] = new
            return e
        order = [(p, True) for p in range(0, L - 1)] + [(p, False) for p in range(L - 1, 0, -1)]
    else:
        raise TypeError(f"approximate on interleaved states takes DMRG or DMRG2, not {type(alg).__name__}")
    eps, history = 2 * alg.tol, []
    for it in range(1, alg.maxiter + 1):
        eps = 0.0
        for pos, forward in order:
            eps = max(eps, visit(pos, forward))
        history.append((it, eps))
        if alg.verbosity >= 3:
            print(f"[ Info: approximate {type(alg).__name__} (interleaved complex) {it:3d}:\terr = {eps:.10e}", flush=True)
        if eps < alg.tol:
            break
    envs.move_center(psi, 0)
    envs.history = history
    return psi, envs, eps


# ---- the reference's entry points on interleaved states (same algorithm objects as algorithms.py) ---------------------------

def find_groundstate(psi: NativeFiniteMPS, H, alg, envs: NativeFinEnv = None):
    """find_groundstate(psi, H, DMRG(...) | DMRG2(...))  (dmrg.jl:22-55, :80-137): sweeps until the energy moves by less than
    alg.tol (relative) or alg.maxiter is reached.  Returns (psi, envs, |dE| of the last sweep)."""
    from .algorithms import DMRG, DMRG2, VUMPS
    if isinstance(psi, NativeInfiniteMPS):       # find_groundstate(psi, H, VUMPS(...)) (vumps.jl:29-92): (psi, envs, galerkin)
        _refuse_inf_alg(alg, "find_groundstate")
        if not isinstance(alg, VUMPS):
            raise TypeError(f"find_groundstate on a NativeInfiniteMPS takes VUMPS, not {type(alg).__name__}")
        _refuse_ham(H)
        return _vumps_inf(psi, H, alg, envs)
    envs = NativeFinEnv(psi, H) if envs is None else envs
    ws = krylov.KrylovWorkspace(psi.be)
    E_old, delta = np.inf, np.inf
    for it in range(1, alg.maxiter + 1):
        if isinstance(alg, DMRG2):   # the scheme of the real host (algorithms.py: _dmrg2)
            trunc_err = alg.trunc_err if alg.trunc_dim <= 0 else 0.0
            E = dmrg2_sweep(psi, H, envs, alg.eigalg, alg.trunc_dim, ws, trunc_err=trunc_err)
        elif isinstance(alg, DMRG):
            E = dmrg_sweep(psi, H, envs, alg.eigalg, ws)
        else:
            raise TypeError(f"find_groundstate on interleaved states takes DMRG or DMRG2, not {type(alg).__name__}")
        delta = abs(E - E_old)
        if alg.verbosity >= 3:
            print(f"[ Info: {type(alg).__name__} (interleaved complex) {it:3d}:\tobj = {E:+.12e}\tdE = {delta:.3e}")
        if delta <= alg.tol * max(1.0, abs(E)):
            break
        E_old = E
    return psi, envs, delta


def propagator(psi0: NativeFiniteMPS, z, H, alg=None, init: NativeFiniteMPS = None, canonical=True):
    """propagator(psi0, z, H, DynamicalDMRG(flavour = NaiveInvert()))  (corvector.jl:50-90) on interleaved states: the
    sweep of mpskit.jl_amd/propagator.py, which runs this flavour on NativeFiniteMPS / NativeFinEnv.  The site operator is
    asked for in Jordan form (MPSK_HAC_CANONICAL_C128); canonical=False keeps the general complex one.  Returns (value, init)."""
    from .propagator import DynamicalDMRG, NaiveInvert, propagator as _propagator
    alg = DynamicalDMRG() if alg is None else alg
    if not isinstance(alg.flavour, NaiveInvert):
        raise NotImplementedError("propagator on interleaved complex states: the NaiveInvert flavour only (Jeckelmann with a "
                                  "complex state is not implemented)")
    return _propagator(psi0, z, H, alg, init=init, canonical=canonical)


def timestep(psi: NativeFiniteMPS, H, t, dt, alg, envs: NativeFinEnv = None):
    """timestep(psi, H, t, dt, TDVP() | TDVP2(...))  (tdvp.jl:61-94, :113-146).  H: an MPOHamiltonian, or a LazySum /
    MultipliedOperator of them, timed or not (environments: NativeMultipleEnv).  Returns (psi, envs)."""
    from .algorithms import TDVP, TDVP2
    if isinstance(psi, NativeInfiniteMPS):       # tdvp.jl:21-59; the reference has no two-site scheme for a uniform state
        if isinstance(alg, TDVP2):
            raise NotImplementedError("timestep on a NativeInfiniteMPS: TDVP2 is not defined for a uniform state (TDVP only)")
        if not isinstance(alg, TDVP):
            raise TypeError(f"timestep on a NativeInfiniteMPS takes TDVP, not {type(alg).__name__}")
        _refuse_ham(H)
        return _timestep_inf(psi, H, t, dt, alg, envs)
    if envs is None:
        envs = NativeFinEnv(psi, H) if _sum_terms(H) is None else NativeMultipleEnv(psi, H)
    if isinstance(alg, TDVP2):
        trunc_err = alg.trunc_err if alg.trunc_dim <= 0 else 0.0
        return tdvp2_step(psi, H, envs, t, dt, alg, alg.trunc_dim, trunc_err=trunc_err)
    if isinstance(alg, TDVP):
        return tdvp_step(psi, H, envs, t, dt, alg)
    raise TypeError(f"timestep on interleaved states takes TDVP or TDVP2, not {type(alg).__name__}")


def expectation_value(psi: NativeFiniteMPS, O, envs=None, device=None):
    """expectation_value(psi, O): <O_i> of every site for a [d,d] operator or a list of one per site (expval.jl:23-37), complex.
    One mpsk_site_gram(AC_i, AC_i) under MPSK_C128 per site, one download (measure.py).  The centre is moved on a copy: psi
    and the environments that follow its gauge stay as they are."""
    from . import measure
    if isinstance(psi, NativeInfiniteMPS):
        from .operators import MPOHamiltonian
        if isinstance(O, (MPOHamiltonian, ComplexMPOHamiltonian)) or isinstance(envs, NativeMPOHamInfEnv):
            return _energy_inf(psi, O, envs)       # the energy per site of the unit cell (expval.jl:111-124), complex
        if not isinstance(O, (np.ndarray, list, tuple)):
            _refuse_ham(O)
        return _expval_inf(psi, O)
    return measure.expectation_value(psi.copy(), O, None, device=device)


def correlator(psi: NativeFiniteMPS, O1, O2, i=None, js=None, device=None):
    """correlator(psi, O1, O2, i, js) / correlator(psi, O12, i, js)  (correlators.jl:10-43), complex: move_center(i) on a
    copy, then one mpsk_transfer_left_gram under MPSK_C128 per site asked for through the right-canonical tensors."""
    from . import measure
    return measure.correlator(psi.copy(), O1, O2, i, js, device=device)


# ---- uniform states on interleaved storage (infinitemps.jl, ortho.jl, permpoinfenv.jl, approximate/vomps.jl) ---------------
# The same storage as above: every tensor is ONE buffer of interleaved complex128, first dimension doubled.  The gauge runs
# on qrpos_c / lqpos_c / gemm_c, the transfers on the complex mpsk_transfer_left / _right (the kernel conjugates the bra), and
# the non-Hermitian fixed points on krylov.eigsolve_lm_planar, whose planar [Re | Im] vectors are one mpsk_vsplit_c /
# mpsk_vjoin_c away from the interleaved tensors the operators take.

def _mul_CA(be, C: DTensor, A: DTensor):
    Dl2, d, Dr = A.shape
    return be.gemm_c(C, A.reshape(Dl2, d * Dr)).reshape(C.shape[0], d, Dr)


def _mul_AC(be, A: DTensor, C: DTensor):
    Dl2, d, Dr = A.shape
    return be.gemm_c(A.reshape(Dl2 * d, Dr), C).reshape(Dl2, d, C.shape[1])


def _dotc(be, x: DTensor, y: DTensor):
    """conj(x) . y from real inner products of the interleaved doubles: Re = x . y, Im = -(x . (i y))"""
    return complex(be.dot(x, y), -be.dot(x, be.times_i(y)))


def _eig_lm_c(be, op, x0: DTensor, tol, krylovdim=30, maxiter=100):
    """Leading (:LM) eigenpair of a complex-linear `op` on interleaved tensors of the shape of x0: the complex Arnoldi of
    krylov.eigsolve_lm_planar, one split / join per application.  tol is relative to the operator's scale |op x0| / |x0|, as
    statmech._eig_lm takes it.  Returns (complex eigenvalue, interleaved eigenvector of unit norm)."""
    import warnings
    shape = x0.shape
    z = be.empty(*shape)

    def mv(p, out):
        be.join_c(p, shape, out=z)
        return be.split_c(op(z), out=out)

    scale = be.norm(op(x0)) / be.norm(x0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # an unconverged restart only costs the caller another outer iteration
        vals, vecs, _, _ = krylov.eigsolve_lm_planar(be, mv, be.split_c(x0), num=1, tol=tol * max(scale, 1e-300),
                                                     krylovdim=krylovdim, maxiter=maxiter)
    return complex(vals[0]), be.join_c(vecs[0], shape)


def _bond_tl(be, v: DTensor, A: DTensor, Ab: DTensor):
    """v'[q, b] = sum conj(Ab[p, s, q]) v[p, a] A[a, s, b] on one interleaved slab (transfer.jl:18-25)"""
    r = be.transfer_left(None, v.reshape(1, *v.shape), A, Ab, cplx=True)
    return r.reshape(r.shape[1], r.shape[2])


def _bond_tr(be, v: DTensor, A: DTensor, Ab: DTensor):
    """v'[a, p] = sum A[a, s, b] v[b, q] conj(Ab[p, s, q])"""
    r = be.transfer_right(None, v.reshape(1, *v.shape), A, Ab, cplx=True)
    return r.reshape(r.shape[1], r.shape[2])


def _gauge_change(be, new: DTensor, old: DTensor):
    """|new - old| of two bond matrices"""
    if hasattr(be, "vdiff_nrm2"):
        return float(np.sqrt(max(be.vdiff_nrm2(new, old)[0], 0.0)))
    return be.norm(be.axpby(-1.0, old, 1.0, be.copy(new)))


def uniform_leftorth(be, A, C0: DTensor, tol=1e-14, maxiter=100, eig_miniter=10):
    """ortho.jl uniform_leftorth! on interleaved tensors: per site C A -> QRpos until |C0 - C1| < tol; from iteration
    eig_miniter on the sweep starts from the leading eigenvector of flip(TransferMatrix(A, AL)).  Returns (AL, CR)."""
    n = len(A)
    c = be.copy(C0)
    be.scal(1.0 / be.norm(c), c)
    CR, AL = [None] * n, [None] * n
    CR[n - 1] = c
    eps, it = np.inf, 0
    while True:
        if it >= eig_miniter:
            def tm(v):
                for i in range(n):
                    v = _bond_tl(be, v, A[i], AL[i])
                return v
            _, vec = _eig_lm_c(be, tm, CR[n - 1], max(eps * eps, tol / 10, 1e-15), maxiter=10)
            _, CR[n - 1] = be.qrpos_c(vec)
        C_old = CR[n - 1]
        for i in range(n):
            x = _mul_CA(be, CR[(i - 1) % n], A[i])
            Dl2, d, Dr = x.shape
            Q, R = be.qrpos_c(x.reshape(Dl2 * d, Dr))
            AL[i], CR[i] = Q.reshape(Dl2, d, Dr), R
        be.scal(1.0 / be.norm(CR[n - 1]), CR[n - 1])
        eps = _gauge_change(be, CR[n - 1], C_old)
        it += 1
        if eps < tol or it > maxiter:
            return AL, CR


def uniform_rightorth(be, A, C0: DTensor, tol=1e-14, maxiter=100, eig_miniter=10):
    """ortho.jl uniform_rightorth! on interleaved tensors: per site A C -> LQpos, right to left.  Returns (AR, CR)."""
    n = len(A)
    c = be.copy(C0)
    be.scal(1.0 / be.norm(c), c)
    CR, AR = [None] * n, [None] * n
    CR[n - 1] = c
    eps, it = np.inf, 0
    while True:
        if it >= eig_miniter:
            def tm(v):
                for i in range(n - 1, -1, -1):
                    v = _bond_tr(be, v, A[i], AR[i])
                return v
            _, vec = _eig_lm_c(be, tm, CR[n - 1], max(eps * eps, tol / 10, 1e-15), maxiter=10)
            CR[n - 1], _ = be.lqpos_c(vec)
        C_old = CR[n - 1]
        for i in range(n - 1, -1, -1):
            x = _mul_AC(be, A[i], CR[i])
            Dl2, d, Dr = x.shape
            Lm, Q = be.lqpos_c(x.reshape(Dl2, d * Dr))
            CR[(i - 1) % n], AR[i] = Lm, Q.reshape(Dl2, d, Dr)
        be.scal(1.0 / be.norm(CR[n - 1]), CR[n - 1])
        eps = _gauge_change(be, CR[n - 1], C_old)
        it += 1
        if eps < tol or it > maxiter:
            return AR, CR


class NativeInfiniteMPS:
    """InfiniteMPS (infinitemps.jl:46-104) with interleaved complex128 tensors: AL, AR, AC [Dl, d, Dr] as (2 Dl, d, Dr) and CR
    (bond right of site i) as (2 D, D), per site of a unit cell of any length.  |CR| = 1, AL CR = CR AR = AC."""

    def __init__(self, tensors, be: Backend = None, tol=1e-14, maxiter=100):
        from .backend import default_backend
        be = self.be = default_backend() if be is None else be
        A = [be.upload_c(np.asarray(t, dtype=np.complex128)) for t in tensors]
        D = A[0].shape[0] // 2
        if A[-1].shape[2] != D or any(A[i].shape[2] != A[i + 1].shape[0] // 2 for i in range(len(A) - 1)):
            raise ValueError("the bond dimensions of the unit cell do not chain")
        AL, CR = uniform_leftorth(be, A, be.upload_c(np.eye(D, dtype=np.complex128)), tol, maxiter)      # gaugefix! order :LR
        self.AL = AL
        self.AR, self.CR = uniform_rightorth(be, AL, CR[-1], tol, maxiter)
        self.AC = [_mul_AC(be, self.AL[i], self.CR[i]) for i in range(len(A))]

    @classmethod
    def _of(cls, AL, AR, CR, AC, be):
        out = object.__new__(cls)
        out.AL, out.AR, out.CR, out.AC, out.be = list(AL), list(AR), list(CR), list(AC), be
        return out

    @classmethod
    def random(cls, d, D, rng, n=1, be=None):
        return cls([rng.standard_normal((D, d, D)) + 1j * rng.standard_normal((D, d, D)) for _ in range(n)], be=be)

    @classmethod
    def from_AL(cls, AL, C0: DTensor, tol=1e-14, maxiter=100, be=None):
        """infinitemps.jl:172-186 (gaugefix! order = :R): AL are kept, AR / CR / AC follow from them."""
        from .backend import default_backend
        be = default_backend() if be is None else be
        AR, CR = uniform_rightorth(be, AL, C0, tol, maxiter)
        return cls._of(AL, AR, CR, [_mul_AC(be, AL[i], CR[i]) for i in range(len(AL))], be)

    @classmethod
    def from_real(cls, psi):
        """an InfiniteMPS (real, or complex on the bond embedding of cplx.py) on interleaved storage, in the gauge it has"""
        from .states import InfiniteMPS
        if not isinstance(psi, InfiniteMPS):
            raise TypeError(f"from_real takes an InfiniteMPS, not {type(psi).__name__}")
        be = psi.be

        def cv(t):
            h = be.download(t)
            if getattr(psi, "cplx", False):
                from .cplx import extract
                h = extract(h)
            return be.upload_c(h)
        return cls._of(*([cv(t) for t in ts] for ts in (psi.AL, psi.AR, psi.CR, psi.AC)), be)

    def __len__(self):
        return len(self.AL)

    def dims(self, i):
        Dl2, d, Dr = self.AL[i % len(self)].shape
        return Dl2 // 2, d, Dr

    def copy(self):
        cp = lambda ts: [self.be.copy(t) for t in ts]
        return NativeInfiniteMPS._of(cp(self.AL), cp(self.AR), cp(self.CR), cp(self.AC), self.be)

    def to_host(self):
        """{"AL", "AR", "AC", "CR"}: lists of complex arrays, one per site"""
        return {k: [self.be.download_c(t) for t in getattr(self, k)] for k in ("AL", "AR", "AC", "CR")}

    def bytes(self):
        return 8 * sum(t.size for k in ("AL", "AR", "AC", "CR") for t in getattr(self, k))


def as_complex_mpo(O):
    """a SparseMPO in complex storage (the same operator; every slice an MPSK_C128 slice), a complex one as it is"""
    from .operators import SparseMPO
    if not isinstance(O, SparseMPO):
        raise TypeError(f"as_complex_mpo takes a SparseMPO, not {type(O).__name__}")
    if O.cplx:
        return O
    out = SparseMPO(O.data, O.d, be=O.be, chis=O.chis)
    out.cplx = True                  # the slices are built on first use, as MPSK_C128 slices of the same blocks
    return out


def dC_proj_c_composed(be, GL: DTensor, GR: DTensor, c: DTensor):
    """sum_w GL[w] c GR[w] on interleaved operands from plain complex products, one pair per slab, summed with axpby: the
    route of backends without dC_proj_c (the pattern of statmech.dC_proj_composed)."""
    W, Dlo2, Dl = GL.shape
    _, Dr2, Dro = GR.shape
    acc = None
    for w in range(W):
        gl = DTensor(GL.buf[w * Dlo2 * Dl:(w + 1) * Dlo2 * Dl], (Dlo2, Dl))
        gr = DTensor(GR.buf[w * Dr2 * Dro:(w + 1) * Dr2 * Dro], (Dr2, Dro))
        y = be.gemm_c(be.gemm_c(gl, c), gr)
        acc = y if acc is None else be.axpby(1.0, y, 1.0, acc)
    return acc


# route of c_proj when the caller does not force one: the fused mpsk_dC_proj_c wherever the backend has it
C_PROJ_FUSED_DEFAULT = True


def _c_proj_route(be, device):
    has = hasattr(be, "dC_proj_c")
    if device and not has:
        from ._lib import MpskError
        raise MpskError("device=True: this backend has no dC_proj_c")
    return (has and C_PROJ_FUSED_DEFAULT) if device is None else bool(device)


class NativePerMPOInfEnv:
    """environments(below, (O, above)) of permpoinfenv.jl:29-42 on interleaved storage: lw[i] (W, 2 D_below, D_above) and
    rw[i] (W, 2 D_above, D_below), the left / right fixed points of the mixed transfer operators of <below| O |above> across
    the unit cell.  O: a SparseMPO, complex (a real-time make_time_mpo) or real (its slices get complex twins); `above` is
    fixed for the life of the object.  device: the route of c_proj (None: the default, True: mpsk_dC_proj_c, False: composed)."""

    def __init__(self, below: NativeInfiniteMPS, toapprox, tol=1e-12, krylovdim=30, maxiter=100, rng=None, device=None):
        from .operators import SparseMPO
        if not (isinstance(toapprox, tuple) and len(toapprox) == 2):
            raise TypeError("NativePerMPOInfEnv takes (below, (O, above))")
        O, above = toapprox
        _refuse_out_of_scope(O, above)
        if not isinstance(O, SparseMPO):
            raise TypeError(f"NativePerMPOInfEnv takes a SparseMPO, not {type(O).__name__}")
        if not isinstance(above, NativeInfiniteMPS) or not isinstance(below, NativeInfiniteMPS):
            raise TypeError("NativePerMPOInfEnv takes NativeInfiniteMPS states (NativeInfiniteMPS.from_real converts one)")
        if len(above) != len(below):
            raise ValueError(f"unit cells of the states above ({len(above)}) and below ({len(below)}) differ")
        if len(below) % len(O) != 0:
            raise ValueError(f"unit cell of the state ({len(below)}) is not a multiple of the MPO's ({len(O)})")
        be = self.be = below.be
        if O.be is None:
            O.be = be
        if O.be is not be:
            raise ValueError("the SparseMPO and the state live on different backends")
        self.opp, self.above, self.device = O, above, device
        self.slices = list(O.slices) if O.cplx else [HalfEmbeddedOp._cslice(be, s) for s in O.slices]
        self.tol, self.krylovdim, self.maxiter = tol, krylovdim, maxiter
        self.rng = np.random.default_rng(0) if rng is None else rng
        self.lw = self.rw = self.dependency = None
        self.recalculate(below, tol)

    def O(self, pos):
        return self.slices[pos % len(self.slices)]

    def _random(self, W, D1, D2):
        z = self.rng.standard_normal((D1, W, D2)) + 1j * self.rng.standard_normal((D1, W, D2))
        return self.be.upload_env_c([z])

    def recalculate(self, psi: NativeInfiniteMPS, tol=None):
        """permpoinfenv.jl recalculate!: restart from the previous fixed points when the bonds of the state below are
        unchanged, from random start vectors otherwise."""
        tol = self.tol if tol is None else tol
        n, old, ab = len(psi), self.dependency, self.above
        if len(ab) != n:
            raise ValueError(f"unit cells of the states above ({len(ab)}) and below ({n}) differ")
        if old is not None and len(old) == n and all(a.shape == b.shape for a, b in zip(old.CR, psi.CR)):
            L0, R0 = self.be.copy(self.lw[0]), self.be.copy(self.rw[n - 1])
        else:
            L0 = self._random(self.O(0).Wl, psi.dims(0)[0], ab.dims(0)[0])
            R0 = self._random(self.O(n - 1).Wr, ab.dims(n - 1)[2], psi.dims(n - 1)[2])
        self.lw, self.rw = self._mixed_fixpoints(psi, L0, R0, tol)
        self.dependency, self.tol = psi, tol
        return self

    def leftenv(self, pos, psi):
        if self.dependency is not psi:
            self.recalculate(psi)
        return self.lw[pos % len(psi)]

    def rightenv(self, pos, psi):
        if self.dependency is not psi:
            self.recalculate(psi)
        return self.rw[pos % len(psi)]

    def ac_proj(self, pos, below):
        """ac_proj (derivatives.jl:216-219): mpsk_dAC_proj of above.AC[pos] on the environments of `below`"""
        return self.be.dAC_proj(self.O(pos), self.leftenv(pos, below), self.rightenv(pos, below), self.above.AC[pos % len(below)])

    def c_proj(self, pos, below):
        """c_proj (derivatives.jl:204-207): mpsk_dC_proj_c of above.CR[pos] on the environments of `below`"""
        return self._dC(self.leftenv(pos + 1, below), self.rightenv(pos, below), self.above.CR[pos % len(below)])

    def _dC(self, GL, GR, c):
        if _c_proj_route(self.be, self.device):
            return self.be.dC_proj_c(GL, GR, c)
        return dC_proj_c_composed(self.be, GL, GR, c)

    def _mixed_fixpoints(self, psi, L0, R0, tol):  # permpoinfenv.jl:138-189 (one row)
        be, n, top = self.be, len(psi), self.above

        def tl(v):
            for i in range(n):
                v = be.transfer_left(self.O(i), v, top.AL[i], psi.AL[i])
            return v

        def tr(v):
            for i in range(n - 1, -1, -1):
                v = be.transfer_right(self.O(i), v, top.AR[i], psi.AR[i])
            return v

        _, gl = _eig_lm_c(be, tl, L0, tol, self.krylovdim, self.maxiter)
        _, gr = _eig_lm_c(be, tr, R0, tol, self.krylovdim, self.maxiter)
        GL, GR = [None] * n, [None] * n
        GL[0], GR[n - 1] = gl, gr
        for i in range(1, n):
            GL[i] = be.transfer_left(self.O(i - 1), GL[i - 1], top.AL[i - 1], psi.AL[i - 1])
        for i in range(n - 2, -1, -1):
            GR[i] = be.transfer_right(self.O(i + 1), GR[i + 1], top.AR[i + 1], psi.AR[i + 1])
        # |dot(CR_below, c_proj)| = 1 for every column (permpoinfenv.jl:178-185): both factors by 1 / sqrt|lambda|
        for col in range(n):
            lam = _dotc(be, psi.CR[col], self._dC(GL[(col + 1) % n], GR[col], top.CR[col]))
            f = 1.0 / np.sqrt(abs(lam))
            be.scal(f, GL[(col + 1) % n])
            be.scal(f, GR[col])
        return GL, GR


def _refuse_out_of_scope(O, *states):
    from .statmech import DenseMPO
    from .multiline import MPSMultiline, MPOMultiline
    if isinstance(O, DenseMPO):
        raise NotImplementedError("DenseMPO targets are not implemented on NativeInfiniteMPS (SparseMPO only)")
    if isinstance(O, MPOMultiline) or any(isinstance(s, MPSMultiline) for s in states):
        raise NotImplementedError("MPSMultiline / MPOMultiline are not implemented on interleaved complex storage")


def regauge(be, AC: DTensor, C: DTensor):
    """regauge!(AC, C; alg = QRpos()) -> AL = Q_AC Q_C^dag   (ortho.jl:127-131) on interleaved tensors"""
    Dl2, d, Dr = AC.shape
    Qac, _ = be.qrpos_c(AC.reshape(Dl2 * d, Dr))
    Qc, _ = be.qrpos_c(C)
    return be.gemm_c(Qac, Qc, transB=True).reshape(Dl2, d, Dr)


def calc_galerkin(psi: NativeInfiniteMPS, envs: NativePerMPOInfEnv):
    """max over the unit cell of || (1 - AL AL^dag) normalize(ac_proj) ||  (toolbox.jl:26-38, environments with a state above)"""
    if isinstance(envs, NativeMPOHamInfEnv):     # toolbox.jl:17-22 with the Hamiltonian's H_AC
        return _calc_galerkin_inf(psi, envs)
    return max(_galerkin_norm(psi.be, psi.AL[loc], envs.ac_proj(loc, psi)) for loc in range(len(psi)))


def _galerkin_norm(be, AL: DTensor, g: DTensor):
    """|| (1 - AL AL^dag) normalize(g) || on interleaved tensors; g is overwritten"""
    be.scal(1.0 / be.norm(g), g)
    Dl2, d, Dr = AL.shape
    alm, gm = AL.reshape(Dl2 * d, Dr), g.reshape(Dl2 * d, g.shape[2])
    be.gemm_c(alm, be.gemm_c(alm, gm, transA=True), alpha=-1.0, beta=1.0, out=gm)
    return be.norm(gm)


def _approximate_inf(psi: NativeInfiniteMPS, toapprox, alg, envs=None, device=None):  # approximate/vomps.jl:1-80 (one row)
    import time
    from .algorithms import IDMRG1, IDMRG2, VOMPS, VUMPS, updatetol, _log
    if isinstance(alg, (IDMRG1, IDMRG2)):
        raise NotImplementedError(f"approximate on a NativeInfiniteMPS: {type(alg).__name__} is not implemented (VOMPS only)")
    if isinstance(alg, VUMPS):           # vomps.jl:12-17
        alg = VOMPS(tol=alg.tol, maxiter=alg.maxiter, finalize=alg.finalize, verbosity=alg.verbosity,
                    gauge_tol_min=alg.gauge_tol_min, gauge_tol_max=alg.gauge_tol_max, gauge_tol_factor=alg.gauge_tol_factor,
                    env_tol_min=alg.env_tol_min, env_tol_max=alg.env_tol_max, env_tol_factor=alg.env_tol_factor)
    if not isinstance(alg, VOMPS):
        raise TypeError(f"approximate on a NativeInfiniteMPS takes VOMPS (or VUMPS), not {type(alg).__name__}")
    be, n = psi.be, len(psi)
    envs = NativePerMPOInfEnv(psi, toapprox, device=device) if envs is None else envs
    eps = calc_galerkin(psi, envs)
    t0, history = time.time(), []
    for it in range(1, alg.maxiter + 1):
        newAL = [regauge(be, envs.ac_proj(loc, psi), envs.c_proj(loc, psi)) for loc in range(n)]
        gtol = updatetol(alg.gauge_tol_min, alg.gauge_tol_max, alg.gauge_tol_factor, it, eps)
        psi = NativeInfiniteMPS.from_AL(newAL, psi.CR[n - 1], tol=gtol, be=be)
        envs.recalculate(psi, updatetol(alg.env_tol_min, alg.env_tol_max, alg.env_tol_factor, it, eps))
        if alg.finalize is not None:
            psi, envs = alg.finalize(it, psi, toapprox, envs)
        eps = calc_galerkin(psi, envs)
        history.append((it, eps))
        _log(alg, "VOMPS (interleaved complex)", it, float("nan"), eps, t0)
        if eps <= alg.tol:
            break
    envs.history = history
    return psi, envs, eps


def dot(psi1, psi2, krylovdim=30, tol=1e-12, rng=None):
    """dot(psi1, psi2) of two NativeInfiniteMPS (infinitemps.jl:258-264): the leading (:LM) eigenvalue of the mixed pass-through
    transfer TransferMatrix(psi2.AL, psi1.AL) of one unit cell, complex.  Two NativeFiniteMPS: linalg.dot."""
    if isinstance(psi1, NativeFiniteMPS) and isinstance(psi2, NativeFiniteMPS):
        from . import linalg
        return linalg.dot(psi1, psi2)
    if not (isinstance(psi1, NativeInfiniteMPS) and isinstance(psi2, NativeInfiniteMPS)):
        raise TypeError("native_cplx.dot takes two NativeInfiniteMPS or two NativeFiniteMPS")
    if len(psi1) != len(psi2):
        raise ValueError("dot: the unit cells do not match")
    be, n = psi1.be, len(psi1)
    rng = np.random.default_rng(0) if rng is None else rng
    Db, Dk = psi1.dims(0)[0], psi2.dims(0)[0]
    v0 = be.upload_c(rng.standard_normal((Db, Dk)) + 1j * rng.standard_normal((Db, Dk)))

    def tl(v):
        for i in range(n):
            v = _bond_tl(be, v, psi2.AL[i], psi1.AL[i])
        return v

    val, _ = _eig_lm_c(be, tl, v0, tol, krylovdim, 100)
    return val


def _expval_inf(psi: NativeInfiniteMPS, O):
    """<O_i> of every site of the unit cell for a [d, d] operator or a list of one per site: one mpsk_site_gram(AC_i, AC_i)
    under MPSK_C128 per site (expval.jl:23-37)"""
    be, n = psi.be, len(psi)
    ops = [np.asarray(O)] * n if np.asarray(O[0]).ndim == 1 else [np.asarray(o) for o in O]
    if len(ops) != n:
        raise ValueError(f"{len(ops)} operators for a unit cell of {n} sites")
    out = np.zeros(n, dtype=np.complex128)
    for i in range(n):
        d = psi.AC[i].shape[1]
        rho = be.download_c(be.site_gram(psi.AC[i], psi.AC[i], cplx=True).reshape(2 * d, d))     # rho[t, s]
        out[i] = np.sum(ops[i] * rho)
    return out


# ---- Hamiltonian environments and the uniform drivers on interleaved storage (mpohaminfenv.jl, vumps.jl, tdvp.jl:21-59) ----

# route of the regularised transfer matrix when the caller does not force one: mpsk_regularize_axpby wherever the backend has
# it (profiles/native_ham_inf_timings.json, section "reg_op": the fused route is the faster one at D = 256 and D = 1024)
REG_FUSED_DEFAULT = True


def _reg_route(be, device):
    has = hasattr(be, "regularize_axpby")
    if device and not has:
        from ._lib import MpskError
        raise MpskError("device=True: this backend has no regularize_axpby")
    return (has and REG_FUSED_DEFAULT) if device is None else bool(device)


def _refuse_ham(H):
    from .operators import LazySum, MultipliedOperator, MPOHamiltonian
    from .statmech import DenseMPO
    from .multiline import MPOMultiline
    if isinstance(H, LazySum):
        raise NotImplementedError("LazySum Hamiltonians are not implemented on NativeInfiniteMPS (NativeMPOHamInfEnv)")
    if isinstance(H, MultipliedOperator):
        raise NotImplementedError("MultipliedOperator / TimedOperator Hamiltonians are not implemented on NativeInfiniteMPS")
    if isinstance(H, DenseMPO):
        raise NotImplementedError("DenseMPO is not implemented on NativeInfiniteMPS (NativeMPOHamInfEnv takes an MPOHamiltonian)")
    if isinstance(H, MPOMultiline):
        raise NotImplementedError("MPOMultiline is not implemented on NativeInfiniteMPS")
    if not isinstance(H, (MPOHamiltonian, ComplexMPOHamiltonian)):
        raise TypeError(f"NativeMPOHamInfEnv takes an MPOHamiltonian or a ComplexMPOHamiltonian, not {type(H).__name__}")


def _slab(t: DTensor, w):
    """slab w of an environment (W, 2 D1, D2) as a (1, 2 D1, D2) view"""
    n = t.shape[1] * t.shape[2]
    return DTensor(t.buf[w * n:(w + 1) * n], (1, t.shape[1], t.shape[2]))


class _RegOp:
    """x -> x - regularize(T x) on interleaved slabs (transfermatrix.jl:29-33, :70-76), the operator of the GMRES solve of an
    identity level: `cell` applies the n pass-through transfers, lvec / rvec are the two fixed points as mpsk_regularize_axpby
    takes them.  fused: one regularize_axpby(y, lvec, rvec, a1=-1, x=x, a0=1, out=out); composed: conj(lvec^T) is uploaded
    once, the coefficient of a slab is one dotc, the rank-one update and the sum are axpby_c."""

    def __init__(self, be, cell, lvec, rvec, fused):
        self.be, self.cell, self.lvec, self.rvec, self.fused = be, cell, lvec, rvec, fused
        if not fused:
            self.vs = krylov.ComplexVec(be)
            self.u = be.upload_c(np.conj(be.download_c(lvec).T))

    def project(self, v):
        """regularize!(v, lvec, rvec) in place"""
        be = self.be
        if self.fused:
            return be.regularize_axpby(v, self.lvec, self.rvec, out=v, cplx=True)
        rv = self.rvec.reshape(1, *self.rvec.shape)
        for w in range(v.shape[0]):
            vw = _slab(v, w)
            self.vs.axpby(-self.vs.dot(self.u.reshape(vw.shape), vw), rv, 1.0, vw)
        return v

    def __call__(self, x, out):
        be = self.be
        y = self.cell(x)
        if self.fused:
            return be.regularize_axpby(y, self.lvec, self.rvec, a1=-1.0, x=x, a0=1.0, out=out, cplx=True)
        self.project(y)
        self.vs.axpby(1.0, x, 0.0, out)
        return self.vs.axpby(-1.0, y, 1.0, out)

    def apply_axpby(self, a1, x, a0, out):          # krylov.linsolve: the operator itself is the shifted one (a0 = 0, a1 = 1)
        assert a0 == 0 and a1 == 1
        return self(x, out)


class _PlainOp:
    """x -> x - T x for a diagonal level that is not the identity (mpohaminfenv.jl:109-115)"""

    def __init__(self, be, cell):
        self.be, self.cell, self.vs = be, cell, krylov.ComplexVec(be)

    def __call__(self, x, out):
        y = self.cell(x)
        self.vs.axpby(1.0, x, 0.0, out)
        return self.vs.axpby(-1.0, y, 1.0, out)

    def apply_axpby(self, a1, x, a0, out):
        assert a0 == 0 and a1 == 1
        return self(x, out)


class NativeMPOHamInfEnv(MPOHamInfEnv):
    """environments(psi::NativeInfiniteMPS, H) of mpohaminfenv.jl:40-215 on interleaved storage: environments.MPOHamInfEnv
    with its leaves overridden, and nothing else -- the level solver, the cycles, recalculate and the assembled, cached site
    environments are the base class's.  Level i of site s is its own (chi, 2 D, D) tensor of interleaved slabs.  Identity
    levels are solved by GMRES over the complex numbers (krylov.linsolve, cplx=True) on the regularised transfer matrix, whose
    application is the n pass-through complex transfers and one mpsk_regularize_axpby.
    H: a real MPOHamiltonian (its slices get complex twins) or a ComplexMPOHamiltonian whose period divides the unit cell.
    device: the route of the regulariser (None: REG_FUSED_DEFAULT, True: mpsk_regularize_axpby, False: composed from
    dotc / axpby_c)."""

    def __init__(self, psi: NativeInfiniteMPS, H, tol=1e-12, maxiter=100, rng=None, device=None):
        _refuse_ham(H)
        if not isinstance(psi, NativeInfiniteMPS):
            raise TypeError("NativeMPOHamInfEnv takes a NativeInfiniteMPS (NativeInfiniteMPS.from_real converts one)")
        if len(psi) % H.period != 0:
            raise ValueError(f"unit cell of the state ({len(psi)}) is not a multiple of the Hamiltonian's period ({H.period})")
        be, self.device = psi.be, device
        native = isinstance(H, ComplexMPOHamiltonian)
        self.opp = [H[s] if native else HalfEmbeddedOp._cslice(be, H[s]) for s in range(H.period)]
        self._blk, self._col, self._eyes = {}, {}, {}
        self.n_reg = 0                        # applications of the regularised operator (both routes), for inspection
        super().__init__(psi, H, tol, maxiter, rng)

    # ---- the leaves of MPOHamInfEnv on interleaved storage ----
    def O(self, pos):
        """the MPSK_C128 slice of site pos"""
        return self.opp[pos % len(self.opp)]

    def isid(self, i):
        return all(s.isscal(i, i) and abs(s.blocks[(i, i)] - 1) < 1e-14 for s in self.opp)

    def _bonds(self, psi, s):
        Dl, _, Dr = psi.dims(s)
        return Dl, Dr

    def _solve_tol(self, psi, tol):
        """None is the tolerance of the last recalculation that named one; the route of the regulariser is settled here, so
        that device=True on a backend without the entry is refused before anything is computed"""
        if len(psi) % len(self.opp) != 0:
            raise ValueError(f"unit cell of the state ({len(psi)}) is not a multiple of the Hamiltonian's period "
                             f"({len(self.opp)})")
        self._fused = _reg_route(self.be, self.device)
        self.tol = self.tol if tol is None else tol
        return self.tol

    def _random_level(self, chi, D):
        return self.be.upload_env_c([np.transpose(self.rng.random((chi, D, D)), (1, 0, 2)).astype(np.complex128)])

    def _identity_level(self, chi, D):
        return self.be.upload_env_c([np.stack([np.eye(D, dtype=np.complex128)] * chi, axis=1)])

    def _eye(self, D):
        if D not in self._eyes:
            self._eyes[D] = self.be.upload_c(np.eye(D, dtype=np.complex128))
        return self._eyes[D]

    def _CCd(self, psi, s):
        """r_LL of the bond right of site s as mpsk_regularize_axpby reads it: lvec[ket, bra] = C C^dag"""
        c = psi.CR[s % len(psi)]
        return self.be.gemm_c(c, c, transB=True)

    def _CdC(self, psi, s):
        """l_RR of the bond left of site s: lvec[bra, ket] = C^dag C"""
        c = psi.CR[(s - 1) % len(psi)]
        return self.be.gemm_c(c, c, transA=True)

    def _scaled(self, z, t):
        """z t for a complex number z (mpsk_vaxpby_c into a new tensor; never the real scal)"""
        return krylov.ComplexVec(self.be).axpby(z, t, 0.0, self.be.empty(*t.shape))

    def _level_slice(self, s, i, j):
        key = (s % len(self.opp), i, j)
        if key not in self._blk:
            O = self.O(s).blocks[(i, j)]
            self._blk[key] = self.be.mposlice(1, self.H.d, [O.shape[0]], [O.shape[3]], {(0, 0): O}, cplx=True)
        return self._blk[key]

    def _tl(self, v, s, i, j, A):
        """the (i -> j) block of the left transfer through site s: a scalar block is the pass-through transfer times it"""
        be, O = self.be, self.O(s).blocks[(i, j)]
        if np.isscalar(O):
            out = be.transfer_left(None, v, A, A, cplx=True)
            return out if O == 1 else self._scaled(O, out)
        return be.transfer_left(self._level_slice(s, i, j), v, A, A)

    def _tr(self, v, s, i, j, A):
        be, O = self.be, self.O(s).blocks[(i, j)]
        if np.isscalar(O):
            out = be.transfer_right(None, v, A, A, cplx=True)
            return out if O == 1 else self._scaled(O, out)
        return be.transfer_right(self._level_slice(s, i, j), v, A, A)

    def _solve(self, op, b, x0, tol):
        if self.be.norm(b) == 0:
            return self.be.zeros(*b.shape)
        x, info = krylov.linsolve(self.be, op, b, x0, a0=0.0, a1=1.0, tol=tol, maxiter=self.maxiter, ws=self.ws, cplx=True)
        self.n_reg += info.numops
        return x

    def _solve_identity(self, cell, lvec, rvec, b, x0, tol):
        return self._solve(_RegOp(self.be, cell, lvec, rvec, self._fused), b, x0, tol)

    def _solve_plain(self, cell, b, x0, tol):
        return self._solve(_PlainOp(self.be, cell), b, x0, tol)

    def project(self, v, lvec, rvec):
        return _RegOp(self.be, None, lvec, rvec, self._fused).project(v)

    # ---- the site operators (derivatives.jl:3-31, :77-93) ----
    def hac(self, pos, psi):
        """the prepared H_AC of site pos (mpsk_hac_create on the assembled environments, mode 2)"""
        return self.be.hac_create(self.O(pos), self.leftenv(pos, psi), self.rightenv(pos, psi))

    def hc(self, pos, psi):
        """H_C of the bond right of site pos"""
        be, GL, GR = self.be, self.leftenv(pos + 1, psi), self.rightenv(pos, psi)
        return lambda x, out=None: be.dC(GL, GR, x, out=out, cplx=True)


def environments(psi: NativeInfiniteMPS, H, **kw):
    """environments(psi, H): NativeMPOHamInfEnv for a Hamiltonian, NativePerMPOInfEnv for H = (O, above)"""
    if isinstance(H, tuple):
        return NativePerMPOInfEnv(psi, H, **kw)
    return NativeMPOHamInfEnv(psi, H, **kw)


def _galerkin_ham(psi: NativeInfiniteMPS, envs: NativeMPOHamInfEnv, loc):
    """|| (1 - AL AL^dag) normalize(H_AC AC) || of one site (toolbox.jl:17-22)"""
    return _galerkin_norm(psi.be, psi.AL[loc], envs.hac(loc, psi).apply(psi.AC[loc]))


def _energy_inf(psi: NativeInfiniteMPS, H, envs: NativeMPOHamInfEnv = None):
    """energy per site of the unit cell (expval.jl:111-124), complex: the last column of the site slice applied to the assembled
    left environment through AC, traced over the bond -- one transfer and one dotc per site, on the device."""
    envs = NativeMPOHamInfEnv(psi, H) if envs is None else envs
    be, n, odim = psi.be, len(psi), envs.H.odim
    vs = krylov.ComplexVec(be)
    ens = np.zeros(n, dtype=np.complex128)
    for i in range(n):
        O, key = envs.O(i), i % len(envs.opp)
        if key not in envs._col:
            col = {(j, 0): O.blocks[(j, odim - 1)] for j in range(odim) if O.contains(j, odim - 1)}
            envs._col[key] = be.mposlice(odim, envs.H.d, O.chil, [O.chir[odim - 1]] + [1] * (odim - 1), col, cplx=True)
        apl = be.transfer_left(envs._col[key], envs.leftenv(i, psi), psi.AC[i], psi.AC[i])
        first = DTensor(apl.buf[:apl.shape[1] * apl.shape[2]], (apl.shape[1], apl.shape[2]))      # slab 0: [bra, ket]
        ens[i] = vs.dot(envs._eye(first.shape[1]), first)
    return ens


# ---- what the uniform drivers ask of the state's storage: algorithms._vumps / algorithms._timestep_inf are the loops, and look
# these names up here for a NativeInfiniteMPS and in algorithms.py for an InfiniteMPS (algorithms._storage) ----

VUMPS_LABEL = "VUMPS (interleaved complex)"


def _groundstate_AL(psi, H, envs, loc, tol, krylovdim, ws):
    """AL of site loc from the lowest eigenvectors of H_AC and H_C, solved to `tol` (vumps.jl:46-60)"""
    be = psi.be
    _, AC, _, _ = krylov.eigsolve_sr(be, envs.hac(loc, psi).apply, psi.AC[loc], tol=tol, krylovdim=krylovdim, ws=ws)
    _, C, _, _ = krylov.eigsolve_sr(be, envs.hc(loc, psi), psi.CR[loc], tol=tol, krylovdim=krylovdim, ws=ws)
    return regauge(be, AC, C)


def _evolved_AL(psi, H, envs, loc, t, dt, alg, ws):
    """AL of site loc from AC and C evolved over dt (tdvp.jl:27-45)"""
    from .algorithms import _integrate_embedded
    be, z, h = psi.be, -1j * complex(dt), envs.hac(loc, psi)
    ac = _integrate_embedded(be, lambda x, out=None: h.apply(x, out=out), psi.AC[loc], z, alg, ws)
    c = _integrate_embedded(be, envs.hc(loc, psi), psi.CR[loc], z, alg, ws)
    return regauge(be, ac, c)


def _from_AL(psi, AL, **kw):
    return NativeInfiniteMPS.from_AL(AL, psi.CR[len(psi) - 1], be=psi.be, **kw)


def _calc_galerkin_inf(psi, envs):
    return max(_galerkin_ham(psi, envs, loc) for loc in range(len(psi)))


def _energy_sum(psi, H, envs):
    return float(np.sum(_energy_inf(psi, H, envs)).real)


def _vumps_inf(psi: NativeInfiniteMPS, H, alg, envs=None, device=None):  # vumps.jl:29-92
    from .algorithms import _vumps
    return _vumps(psi, H, alg, NativeMPOHamInfEnv(psi, H, device=device) if envs is None else envs)


def _timestep_inf(psi: NativeInfiniteMPS, H, t, dt, alg, envs=None, device=None):  # tdvp.jl:21-59 (leftorthflag = true)
    from . import algorithms
    return algorithms._timestep_inf(psi, H, t, dt, alg, NativeMPOHamInfEnv(psi, H, device=device) if envs is None else envs)


def time_evolve(psi, H, t_span, alg=None, envs=None):
    """time_evolve(psi, H, t_span, TDVP())  (time_evolve.jl:20-40) on interleaved states: consecutive timesteps"""
    from . import algorithms
    if isinstance(psi, NativeInfiniteMPS):       # algorithms.timestep hands a uniform state back to timestep above
        return algorithms.time_evolve(psi, H, t_span, alg, envs)
    # a NativeFiniteMPS keeps its own loop: algorithms.timestep would copy it and build the environments of a real chain
    alg = algorithms.TDVP() if alg is None else alg
    for t0, t1 in zip(t_span[:-1], t_span[1:]):
        psi, envs = timestep(psi, H, t0, t1 - t0, alg, envs)
        if alg.finalize is not None:
            psi, envs = alg.finalize(t0, psi, H, envs)
    return psi, envs


def _refuse_inf_alg(alg, what):
    from .algorithms import GradientGrassmann, IDMRG1, IDMRG2, UnionAlg
    if isinstance(alg, UnionAlg):
        _refuse_inf_alg(alg.alg1, what)
        _refuse_inf_alg(alg.alg2, what)
    if isinstance(alg, (GradientGrassmann, IDMRG1, IDMRG2)):
        raise NotImplementedError(f"{what} on a NativeInfiniteMPS: {type(alg).__name__} is not implemented (VUMPS only)")


# ---- changebonds on interleaved storage (changebonds/optimalexpand.jl:16-67, randexpand.jl:15-34, svdcut.jl:35-46,
# changebonds.jl:13-38): changebonds._changebonds_infinite with complex operands.  An interleaved tensor (2 Dl, d, Dr) is a real
# tensor whose first dimension is doubled, so the layout helpers of changebonds.py (_tail_matrix, _from_tail_matrix, _pad_site)
# serve on doubled row counts as they are ----

# route of the expansion directions when the caller does not force one, above changebonds.DEVICE_ROUTE_MIN: mpsk_complement_tsvd
# under MPSK_C128 wherever the backend has it (profiles/expand_native_timings.json)
EXPAND_DEVICE_DEFAULT = True


def _expand_route(be, m, n, route):
    from .changebonds import DEVICE_ROUTE_MIN
    has = hasattr(be, "complement_tsvd_c")
    if route is None:
        return has and EXPAND_DEVICE_DEFAULT and min(m, n) > DEVICE_ROUTE_MIN
    if route not in ("device", "composed"):
        raise ValueError(f"route must be None, 'device' or 'composed', not {route!r}")
    if route == "device" and not has:
        from ._lib import MpskError
        raise MpskError("route='device': this backend has no complement_tsvd_c")
    return route == "device"


def _gauss_c(be, rng, r, c):
    return be.upload_c(rng.standard_normal((r, c)) + 1j * rng.standard_normal((r, c)))


def _complement_cols_c(be, Q: DTensor, rng):
    """orthonormal basis N (m x (m - p)) of the complement of the orthonormal columns of Q (m x p): QRpos of a projected
    Gaussian block, projected twice (changebonds._complement_cols on complex tensors)"""
    m, p = Q.shape[0] // 2, Q.shape[1]
    if m == p:
        return None
    Y = _gauss_c(be, rng, m, m - p)
    for _ in range(2):
        be.gemm_c(Q, be.gemm_c(Q, Y, transA=True), alpha=-1.0, beta=1.0, out=Y)
        Y, _ = be.qrpos_c(Y)
    return Y


def _complement_rows_c(be, B: DTensor, rng):
    """orthonormal rows N ((n - p) x n) spanning the complement of the orthonormal rows of B (p x n)"""
    p, n = B.shape[0] // 2, B.shape[1]
    if p == n:
        return None
    Y = _gauss_c(be, rng, n - p, n)
    for _ in range(2):
        be.gemm_c(be.gemm_c(Y, B, transB=True), B, alpha=-1.0, beta=1.0, out=Y)
        _, Y = be.lqpos_c(Y)
    return Y


def _complement_directions_c(be, Y, QL, Bm, k, rng, dev):
    """the k leading singular vectors of NL^dag Y NR^dag lifted back (optimalexpand.jl:25-32): U (m x kept), Vt (kept x n) and
    the singular values on the host.  dev: mpsk_complement_tsvd under MPSK_C128; otherwise the literal algorithm."""
    n = Y.shape[1]
    if dev:
        U, S, Vt, kept = be.complement_tsvd_c(Y, QL, Bm, k)
        if kept == 0:
            return None, None, np.zeros(0), 0
        return U, Vt, be.download(S), kept
    NL, NR = _complement_cols_c(be, QL, rng), _complement_rows_c(be, Bm, rng)
    if NL is None or NR is None:
        return None, None, np.zeros(0), 0
    nl, nr = NL.shape[1], NR.shape[0] // 2
    inter = be.gemm_c(be.gemm_c(NL, Y, transA=True), NR, transB=True)          # nl x nr
    Uk, S, Vh, kept, _ = be.tsvd_c(inter, max_keep=min(k, nl, nr))
    kmax = Vh.shape[0] // 2
    Vk = be.empty(2 * kept, nr)
    be.copy2d(2 * kept, nr, Vh.ptr, 2 * kmax, Vk.ptr, 2 * kept)
    U = be.gemm_c(NL, DTensor(Uk.buf, (2 * nl, kept)))
    Vt = be.gemm_c(Vk, NR)
    return U, Vt, be.download(DTensor(S.buf, (kept,))), kept


def expansion_directions(psi: NativeInfiniteMPS, H, envs, i, k, rng=None, route=None, Y=None):
    """Expansion directions of bond i (between sites i and i + 1): (U (2 Dl d, kept), Vt (2 kept, Dr d) with (b, s) columns, S on
    the host, kept).  Y given: that matrix instead of H_AC2 (AC_i AR_{i+1}) (RandExpand)."""
    from .changebonds import _tail_matrix
    be, n = psi.be, len(psi)
    rng = np.random.default_rng(0) if rng is None else rng
    ac, al, ar = psi.AC[i % n], psi.AL[i % n], psi.AR[(i + 1) % n]
    Dl2, d1, Dm = ac.shape
    _, d2, Dr = ar.shape
    m, nn = (Dl2 // 2) * d1, Dr * d2
    dev = _expand_route(be, m, nn, route)
    if Y is None:
        Y = be.dAC2_proj(envs.O(i), envs.O(i + 1), envs.leftenv(i, psi), envs.rightenv(i + 1, psi), ac, ar)
    return _complement_directions_c(be, Y.reshape(2 * m, nn), al.reshape(2 * m, Dm), _tail_matrix(be, ar), k, rng, dev)


def _expand(psi: NativeInfiniteMPS, Us, Vts, ks):
    """changebonds.jl:13-38 on device tensors: AL -> [AL U; 0 0], AR -> [AR 0; Vt 0], CR -> [CR 0; 0 0], AC = AL CR.  Us[i] /
    Vts[i] / ks[i] belong to the bond right of site i.  The result is in mixed gauge as it stands (changebonds._expand)."""
    from .changebonds import _from_tail_matrix, _pad_site
    be, n = psi.be, len(psi)
    AL, AR, CR, AC = [None] * n, [None] * n, [None] * n, [None] * n
    for i in range(n):
        kl, kr = ks[(i - 1) % n], ks[i]
        Dl2, d, Dr = psi.AL[i].shape
        Dn2 = Dl2 + 2 * kl
        al = _pad_site(be, psi.AL[i], 2 * kl, kr)
        if kr:                                                # U[(a, s), j] -> al[a, s, Dr + j]
            for s in range(d):
                be.copy2d(Dl2, kr, Us[i].ptr + 8 * s * Dl2, Dl2 * d, al.ptr + 8 * (s * Dn2 + Dn2 * d * Dr), Dn2 * d)
        ar = _pad_site(be, psi.AR[i], 2 * kl, kr)
        if kl:                                                # Vt[j, (b, s)] -> ar[Dl + j, s, b]
            _from_tail_matrix(be, Vts[(i - 1) % n], d, Dr, ar, Dl2)
        c = be.zeros(2 * (Dr + kr), Dr + kr)
        be.copy2d(2 * Dr, Dr, psi.CR[i].ptr, 2 * Dr, c.ptr, 2 * (Dr + kr))
        AL[i], AR[i], CR[i] = al, ar, c
    for i in range(n):
        AC[i] = _mul_AC(be, AL[i], CR[i])
    return NativeInfiniteMPS._of(AL, AR, CR, AC, be)


def _expand_inf(psi: NativeInfiniteMPS, H, alg, envs, rng, route):
    from .changebonds import RandExpand
    n = len(psi)
    Us, Vts, ks = [None] * n, [None] * n, [0] * n
    for i in range(n):
        Y = None
        if isinstance(alg, RandExpand):                       # randexpand.jl:20: a Gaussian two-site block
            Dl, d1, _ = psi.dims(i)
            _, d2, Dr = psi.dims(i + 1)
            Y = _gauss_c(psi.be, rng, Dl * d1, Dr * d2)
        Us[i], Vts[i], _, ks[i] = expansion_directions(psi, H, envs, i, alg.trunc_dim, rng, route, Y)
    return _expand(psi, Us, Vts, ks)


def _svd_cut_inf(psi: NativeInfiniteMPS, alg):
    """svdcut.jl:35-46: tsvd of every CR, AL[i] <- AL[i] U_i, AL[i+1] <- U_i^dag AL[i+1], then the gauge from the new ALs"""
    be, n = psi.be, len(psi)
    ALs = list(psi.AL)
    ncr = None
    for i in range(n):
        c = psi.CR[i]
        D = c.shape[1]
        U, S, _, k, _ = be.tsvd_c(c, max_keep=alg.trunc_dim, trunc_err=alg.trunc_err)
        Uk = DTensor(U.buf, (2 * D, k))                       # the leading columns of U (2 D, D)
        Dl2, d, _ = ALs[i].shape
        ALs[i] = be.gemm_c(ALs[i].reshape(Dl2 * d, D), Uk).reshape(Dl2, d, k)
        j = (i + 1) % n
        _, d2, Dr2 = ALs[j].shape
        ALs[j] = be.gemm_c(Uk, ALs[j].reshape(2 * D, d2 * Dr2), transA=True).reshape(2 * k, d2, Dr2)
        ncr = be.upload_c(np.diag(be.download(DTensor(S.buf, (k,)))).astype(np.complex128))
    return NativeInfiniteMPS.from_AL(ALs, ncr, be=be)


def changebonds(psi: NativeInfiniteMPS, H=None, alg=None, envs=None, rng=None, route=None):
    """changebonds(psi, H, alg[, envs]) -> (psi', envs)  /  changebonds(psi, SvdCut(...) | RandExpand(...)) -> psi' for a
    NativeInfiniteMPS (copying versions; changebonds.changebonds keeps refusing the class, this is its entry).  OptimalExpand:
    H a real MPOHamiltonian or a ComplexMPOHamiltonian whose period divides the unit cell; the environments are
    environments(psi, H) when none are passed, and the ones returned are still attached to the old state, as in the
    reference: they recalculate themselves when they are next read with the new one.  route: None = dispatch, "device"
    (mpsk_complement_tsvd under MPSK_C128) / "composed" (null-space bases, full SVD) = forced."""
    from .changebonds import OptimalExpand, RandExpand, SvdCut
    if not isinstance(psi, NativeInfiniteMPS):
        raise TypeError(f"native_cplx.changebonds takes a NativeInfiniteMPS, not {type(psi).__name__}")
    if isinstance(H, (OptimalExpand, SvdCut, RandExpand)) and alg is None:
        H, alg = None, H
    if H is not None:
        _refuse_ham(H)
    if not isinstance(alg, (OptimalExpand, RandExpand, SvdCut)):
        raise TypeError(f"unknown changebonds algorithm {alg!r}")
    rng = np.random.default_rng(0) if rng is None else rng
    if isinstance(alg, SvdCut):
        out = _svd_cut_inf(psi, alg)
        return out if H is None else (out, envs)
    if isinstance(alg, RandExpand):
        out = _expand_inf(psi, None, alg, None, rng, route)
        return out if H is None else (out, envs)
    if H is None:
        raise TypeError("OptimalExpand needs the operator: changebonds(psi, H, OptimalExpand(...)[, envs])")
    if len(psi) % H.period != 0:
        raise ValueError(f"unit cell of the state ({len(psi)}) is not a multiple of the Hamiltonian's period ({H.period})")
    envs = environments(psi, H) if envs is None else envs
    return _expand_inf(psi, H, alg, envs, rng, route), envs
