"""excitations(H, QuasiparticleAnsatz(), ...) : the quasiparticle (tangent-space) ansatz on top of a finite or a
uniform ground state  (src/algorithms/excitation/quasiparticleexcitation.jl:39-143,254-362, src/environments/qpenv.jl:55-170,
src/algorithms/excitation/exci_transfer_system.jl, src/states/quasiparticle_state.jl:8-104).

Trivial charge sector: the utility leg of the excitation tensor has dimension one, B[a, s, b] = VL[a, s, n] X[n, b], so every
"excited-tensor" contraction of the reference (transfer.jl:48-62,113-126, the three terms of
_effective_excitation_local_apply) IS one of the hot-path kernels with another operand in the ket / environment slot:

    B in the centre      mpsk_dAC(H, GL,  GR,  B)
    B to the left        mpsk_dAC(H, lB,  GR,  AR)        lB = sum of the (AR ket, AL bra) transfers of B further left
    B to the right       mpsk_dAC(H, GL,  rB,  AL)
    lB / rB updates      mpsk_transfer_left/right(H, env, ket = B or AR/AL, bra = AL/AR)

Complex arithmetic.  The ground state and H are real, so every map above is REAL-linear in B; the only complex numbers
are the momentum phases.  A quasiparticle object is therefore carried as one (|sin p| = 0: momentum 0 or pi, and every
finite chain) or two (real, imaginary) real device tensors, the kernels run once per part and a phase e^{i a} mixes the two
parts with one mpsk_vlincomb each.  That is 2x the real flops for a general momentum -- the optimum for a complex vector
under a real operator (no bond embedding, no complex GEMM).  The Hermitian eigenproblem on C^N becomes the symmetric one on
R^{2N} = [Re | Im] with every eigenvalue doubled (v and i v); the Lanczos solver sees an ordinary real vector.

Built: LeftGaugedQP over an MPOHamiltonian -- FiniteQP, InfiniteQP at any momentum, topologically trivial
(left_gs is right_gs, regularised environments) and domain-wall excitations between two different ground states (no
regularisation, energies renormalised by the mean of the two); `variance` of a finite QP state (toolbox.py); the
statistical-mechanics method over a DenseMPO / MPOMultiline (excitations_statmech at the end of this file: topologically
trivial, two real parts at every momentum).  Not built: charged sectors, RightGaugedQP conversion, domain walls and
`variance` of a statistical-mechanics quasiparticle."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from . import krylov
from .backend import DTensor
from .environments import environments as _environments
from .states import FiniteMPS


@dataclass
class QuasiparticleAnsatz:  # quasiparticleexcitation.jl:23-34 : Arnoldi(krylovdim = 30, tol = 1e-10, eager = true)
    tol: float = 1e-10
    krylovdim: int = 30
    maxiter: int = 100
    solver_tol: float = 1e-12      # Defaults.linearsolver (GMRES) of the quasiparticle environments
    solver_maxiter: int = 100


def _view(t: DTensor, off, shape):
    n = int(np.prod(shape))
    return DTensor(t.buf[off:off + n], shape)


class LeftGaugedQP:
    """quasiparticle_state.jl:8-17 : B[i] = VL[i] X[i],  AL[i]^dag VL[i] = 0.  `vec` is the flat device vector
    [Re X_0 .. Re X_{n-1} | Im X_0 .. Im X_{n-1}] (the second half only for a complex momentum phase)."""

    def __init__(self, gs, VLs, xshapes, momentum, vec: DTensor, nparts, right_gs=None):
        self.left_gs = gs
        self.right_gs = gs if right_gs is None else right_gs       # !(left_gs === right_gs) => domain-wall excitation  :9-11
        self.be = gs.be
        self.VLs, self.xshapes, self.momentum, self.vec, self.nparts = VLs, xshapes, momentum, vec, nparts
        self.finite = isinstance(gs, FiniteMPS)
        self.offs = np.concatenate([[0], np.cumsum([a * b for a, b in xshapes])]).astype(int)
        self.N = int(self.offs[-1])

    @classmethod
    def random(cls, gs, momentum=0.0, rng=None, right_gs=None):
        """LeftGaugedQP(rand, left_gs, right_gs; momentum)  :33-46 ; VL from a projected random block + QRpos (any
        orthonormal basis of the complement of AL spans the same tangent space)."""
        from .changebonds import _complement_cols
        be = gs.be
        rng = np.random.default_rng(0) if rng is None else rng
        finite = isinstance(gs, FiniteMPS)
        n = len(gs)
        ALs = [gs.AL(i) for i in range(n)] if finite else gs.AL
        rgs = gs if right_gs is None else right_gs
        ARs = [rgs.AR(i) for i in range(n)] if finite else rgs.AR
        VLs, shapes = [], []
        for i in range(n):
            Dl, d, Dr = ALs[i].shape
            VLs.append(_complement_cols(be, ALs[i].reshape(Dl * d, Dr), rng))
            shapes.append((Dl * d - Dr, ARs[i].shape[2]))
        nparts = 1 if (finite or abs(np.sin(momentum)) < 1e-12) else 2
        N = sum(a * b for a, b in shapes)
        vec = be.upload(rng.random(N * nparts))
        return cls(gs, VLs, shapes, 0.0 if finite else float(momentum), vec, nparts, right_gs)

    @property
    def trivial(self):
        return self.left_gs is self.right_gs

    def __len__(self):
        return len(self.VLs)

    def with_vec(self, vec):
        return LeftGaugedQP(self.left_gs, self.VLs, self.xshapes, self.momentum, vec, self.nparts, self.right_gs)

    def X(self, part, i, vec=None):
        vec = self.vec if vec is None else vec
        return _view(vec, part * self.N + int(self.offs[i]), self.xshapes[i])

    def B(self, part, i, vec=None):  # Base.getindex  :95
        be = self.be
        gs = self.left_gs
        al = gs.AL(i) if self.finite else gs.AL[i]
        Dl, d, _ = al.shape
        if self.xshapes[i][0] == 0:
            return be.zeros(Dl, d, self.xshapes[i][1])
        return be.gemm(self.VLs[i], self.X(part, i, vec)).reshape(Dl, d, self.xshapes[i][1])

    def B_host(self, i):
        """the excitation tensor of site i as a (complex) NumPy array -- test / inspection helper."""
        re = self.be.download(self.B(0, i))
        return re if self.nparts == 1 else re + 1j * self.be.download(self.B(1, i))


# ---- complex objects as lists of 1 or 2 real device tensors -------------------------------------------------------
def _lin(f, z):
    return [f(p) for p in z]


def _acc(be, a, b):
    """a += b (None = zero)."""
    if b is None:
        return a
    if a is None:
        return b
    for pa, pb in zip(a, b):
        be.axpby(1.0, pb, 1.0, pa)
    return a


def _phase(be, z, ang):
    """z * e^{i ang}, in place for a real phase."""
    c, s = np.cos(ang), np.sin(ang)
    if len(z) == 1:
        if round(c) != 1:
            be.scal(float(round(c)), z[0])
        return z
    re, im = z
    return [be.lincomb([re, im], [c, -s]), be.lincomb([re, im], [s, c])]


def _has_heff_entries(be):
    return bool(getattr(be, "has_qp_heff", False)) and all(
        hasattr(be, m) for m in ("qp_half", "qp_heff_site", "transfer_left_pair", "transfer_right_pair"))


class _QPContext:
    """Everything that does not depend on X: ground-state tensors, environments, regularisation bonds, energies.

    device=True: the fused route -- mpsk_qp_heff_site per site and part (B = VL X, the three terms, the pull-back and
    -E X in one entry), the B-independent half of the third term once per site and context (mpsk_qp_half), and the pair
    transfers wherever qp_envs adds a transfer of B to a transfer of lB / rB.  device=False: the composed route (three
    mpsk_dAC, three axpby, two GEMMs), which is also what a backend without the entries runs."""

    def __init__(self, H, phi: LeftGaugedQP, lenvs, alg: QuasiparticleAnsatz, renvs=None, device=False):
        self.H, self.alg, self.be = H, alg, phi.be
        be = self.be
        if device and not _has_heff_entries(be):
            from ._lib import MpskError
            raise MpskError("device=True: this backend has no mpsk_qp_heff_site / pair transfers")
        self.device = bool(device)
        self.half = {}                  # site -> mpsk_qp_half(H[site], GL[site], AL[site]), made on first use
        gs, rgs = phi.left_gs, phi.right_gs
        self.trivial = phi.trivial
        renvs = lenvs if (renvs is None and self.trivial) else (_environments(rgs, H) if renvs is None else renvs)
        n = self.n = len(phi)
        self.finite = phi.finite
        self.p = phi.momentum
        self.AL = [gs.AL(i) for i in range(n)] if self.finite else list(gs.AL)
        self.AR = [rgs.AR(i) for i in range(n)] if self.finite else list(rgs.AR)
        self.GL = [lenvs.leftenv(i, gs) for i in range(n)]
        self.GR = [renvs.rightenv(i, rgs) for i in range(n)]

        def energies(st, envs):        # effective_excitation_renormalization_energy  :330-362
            AC = [st.AC(i) for i in range(n)] if self.finite else list(st.AC)
            return [be.dot(AC[i], be.dAC(H[i], envs.leftenv(i, st), envs.rightenv(i, st), AC[i])) for i in range(n)]
        self.E = energies(gs, lenvs)
        if not self.trivial:
            self.E = [(a + b) / 2 for a, b in zip(self.E, energies(rgs, renvs))]
        self.odim = H.odim
        self.ids = [i for i in range(1, self.odim - 1) if H.isid(i)]
        self.ws = krylov.KrylovWorkspace(be)
        if not self.finite and self.trivial:
            self.C = list(gs.CR)                                                    # bond right of site s
            self.Ct = [be.gemm(c, be.upload(np.eye(c.shape[0])), transA=True) for c in self.C]   # C^T on the device

    # ---- level views of an assembled (W, D, D) environment ----
    def _levels(self, t: DTensor, chis):
        _, Db, Dk = t.shape
        out, off = [], 0
        for c in chis:
            out.append(_view(t, off, (c, Db, Dk)))
            off += c * Db * Dk
        return out

    def _reg(self, v: DTensor, bond):
        """v[:, w, :] -= <C, v[:, w, :]> C   (qpenv.jl:69-76 / transfermatrix.jl:87-90 with a one-dimensional MPO leg)."""
        return self.be.regularize(v, self.Ct[bond % self.n], self.C[bond % self.n])

    def _reg_ids(self, z, chis, bond):
        if not self.trivial:                # qpenv.jl:68,85 `if exci.trivial`
            return z
        for part in z:
            lv = self._levels(part, chis)
            for i in self.ids:
                self._reg(lv[i], bond)
        return z

    def _tblock(self, left, v: DTensor, O, A, Ab):
        be = self.be
        f = be.transfer_left if left else be.transfer_right
        if np.isscalar(O):
            out = f(None, v, A, Ab)
            if O != 1:
                be.scal(O, out)
            return out
        blk = be.mposlice(1, A.shape[1], [O.shape[0]], [O.shape[3]], {(0, 0): O})
        return f(blk, v, A, Ab)

    # ---- exci_transfer_system.jl ----
    def _transfer_system(self, left, start_levels):
        """x = b + e^{-+ i p n} (x T_cell), level by level (triangular H); identity levels by GMRES on the
        regularised mixed transfer matrix.  start_levels[i]: list of parts (level views)."""
        be, H, n, odim = self.be, self.H, self.n, self.odim
        ket, bra = (self.AR, self.AL) if left else (self.AL, self.AR)
        ang = (-self.p if left else self.p) * n
        c, s = np.cos(ang), np.sin(ang)
        nparts = len(start_levels[0])
        if nparts == 1:
            c, s = float(round(c)), 0.0
        found = [None] * odim
        order = range(odim) if left else range(odim - 1, -1, -1)
        sites = range(n) if left else range(n - 1, -1, -1)
        for i in order:
            # found[<i] (left) / found[>i] (right) pushed once through the unit cell, level i of the result
            v = list(found)
            last = n - 1 if left else 0
            for st in sites:
                out = [None] * odim
                rng_k = [i] if st == last else (range(0, i + 1) if left else range(i, odim))
                for k in rng_k:
                    rng_j = range(0, k + 1) if left else range(k, odim)
                    for j in rng_j:
                        blk = (j, k) if left else (k, j)
                        if v[j] is None or not H[st].contains(*blk):
                            continue
                        O = H[st].blocks[blk]
                        out[k] = _acc(be, out[k], _lin(lambda x: self._tblock(left, x, O, ket[st], bra[st]), v[j]))
                v = out
            start = v[i]
            if start is not None:
                start = _phase(be, start, ang)
                if H.isid(i) and self.trivial:
                    for part in start:
                        self._reg(part, n - 1)
            b = _acc(be, [be.copy(x) for x in start_levels[i]], start)
            if all(H[st].contains(i, i) for st in range(n)):
                isid = H.isid(i)
                shape = b[0].shape
                sz = b[0].size
                flat = be.empty(sz * nparts)
                for k, part in enumerate(b):
                    flat.buf[k * sz:(k + 1) * sz].copy_(part.buf[:sz])

                def op(x, out):
                    xs = [_view(x, k * sz, shape) for k in range(nparts)]
                    ys = []
                    for xp in xs:
                        y = xp
                        for st in sites:
                            O = 1.0 if isid else H[st].blocks[(i, i)]
                            y = self._tblock(left, y, O, ket[st], bra[st])
                        if isid and self.trivial:
                            self._reg(y, n - 1)
                        ys.append(y)
                    if nparts == 1:
                        be.lincomb([xs[0], ys[0]], [1.0, -c], out=_view(out, 0, shape))
                    else:
                        be.lincomb([xs[0], ys[0], ys[1]], [1.0, -c, s], out=_view(out, 0, shape))
                        be.lincomb([xs[1], ys[0], ys[1]], [1.0, -s, -c], out=_view(out, sz, shape))
                    return out
                sol = krylov.gmres(be, op, flat, flat, tol=self.alg.solver_tol, maxiter=self.alg.solver_maxiter, ws=self.ws)
                b = [_view(sol, k * sz, shape) for k in range(nparts)]
            found[i] = b
        return found

    def _assemble(self, levels, nparts):
        be = self.be
        out = []
        for k in range(nparts):
            parts = [lv[k] for lv in levels]
            W = sum(p.shape[0] for p in parts)
            t = be.empty(W, parts[0].shape[1], parts[0].shape[2])
            off = 0
            for p in parts:
                t.buf[off:off + p.size].copy_(p.buf[:p.size])
                off += p.size
            out.append(t)
        return out

    # ---- qpenv.jl ----
    def qp_envs(self, phi: LeftGaugedQP, vec: DTensor):
        be, H, n = self.be, self.H, self.n
        AL, AR = self.AL, self.AR
        nparts = phi.nparts
        Bs = [[phi.B(k, s, vec) for k in range(nparts)] for s in range(n)]
        lBs, rBs = [None] * n, [None] * n

        def left(pos, lB):              # T(GL; B, AL) + T(lB; AR, AL): the B of this site joins what came from further left
            if lB is None:
                return _lin(lambda b: be.transfer_left(H[pos], self.GL[pos], b, AL[pos]), Bs[pos])
            if self.device:
                return [be.transfer_left_pair(H[pos], self.GL[pos], b, v, AR[pos], AL[pos]) for b, v in zip(Bs[pos], lB)]
            nxt = _lin(lambda b: be.transfer_left(H[pos], self.GL[pos], b, AL[pos]), Bs[pos])
            return _acc(be, nxt, _lin(lambda v: be.transfer_left(H[pos], v, AR[pos], AL[pos]), lB))

        def right(pos, rB):
            if rB is None:
                return _lin(lambda b: be.transfer_right(H[pos], self.GR[pos], b, AR[pos]), Bs[pos])
            if self.device:
                return [be.transfer_right_pair(H[pos], self.GR[pos], b, v, AL[pos], AR[pos]) for b, v in zip(Bs[pos], rB)]
            nxt = _lin(lambda b: be.transfer_right(H[pos], self.GR[pos], b, AR[pos]), Bs[pos])
            return _acc(be, nxt, _lin(lambda v: be.transfer_right(H[pos], v, AL[pos], AR[pos]), rB))

        if self.finite:                                                              # :146-170
            for pos in range(n - 1):
                lBs[pos + 1] = left(pos, lBs[pos])
            for pos in range(n - 1, 0, -1):
                rBs[pos - 1] = right(pos, rBs[pos])
            return Bs, lBs, rBs
        p = self.p
        for pos in range(n):                                                         # :66-79
            lBs[(pos + 1) % n] = self._reg_ids(_phase(be, left(pos, lBs[pos]), -p), H[pos].chir, pos)
        for pos in range(n - 1, -1, -1):                                             # :81-97
            nxt = right(pos, rBs[pos] if pos != n - 1 else None)
            rBs[(pos - 1) % n] = self._reg_ids(_phase(be, nxt, p), H[pos].chil, pos - 1)
        # :99-105  geometric sums over all unit cells further away
        lv = [self._levels(part, H[0].chil) for part in lBs[0]]
        found = self._transfer_system(True, [[lv[k][i] for k in range(nparts)] for i in range(self.odim)])
        lBs[0] = self._assemble(found, nparts)
        rv = [self._levels(part, H[n - 1].chir) for part in rBs[n - 1]]
        found = self._transfer_system(False, [[rv[k][i] for k in range(nparts)] for i in range(self.odim)])
        rBs[n - 1] = self._assemble(found, nparts)
        cur = lBs[0]
        for i in range(n - 1):                                                       # :107-123
            cur = _lin(lambda v: be.transfer_left(H[i], v, AR[i], AL[i]), cur)
            cur = self._reg_ids(_phase(be, cur, -p), H[i].chir, i)
            lBs[i + 1] = _acc(be, lBs[i + 1], cur)
        cur = rBs[n - 1]
        for i in range(n - 1, 0, -1):                                                # :124-141
            cur = _lin(lambda v: be.transfer_right(H[i], v, AL[i], AR[i]), cur)
            cur = self._reg_ids(_phase(be, cur, p), H[i].chil, i - 1)
            rBs[i - 1] = _acc(be, rBs[i - 1], cur)
        return Bs, lBs, rBs

    # ---- quasiparticleexcitation.jl:254-328 ----
    def heff(self, phi: LeftGaugedQP, x: DTensor, out: DTensor):
        be, H, n = self.be, self.H, self.n
        Bs, lBs, rBs = self.qp_envs(phi, x)
        for loc in range(n):
            if phi.xshapes[loc][0] == 0:
                continue
            Dl, d, _ = self.AL[loc].shape
            if self.device:
                half = None
                if rBs[loc] is not None:
                    if loc not in self.half:
                        self.half[loc] = be.qp_half(H[loc], self.GL[loc], self.AL[loc])
                    half = self.half[loc]
                for k in range(phi.nparts):
                    lB, rB = (None if z is None else z[k] for z in (lBs[loc], rBs[loc]))
                    be.qp_heff_site(H[loc], self.GL[loc], self.GR[loc], phi.VLs[loc], phi.X(k, loc, x), self.E[loc], lB,
                                    None if lB is None else self.AR[loc], half, rB, out=phi.X(k, loc, out))
                continue
            for k in range(phi.nparts):
                B = Bs[loc][k]
                Bn = be.dAC(H[loc], self.GL[loc], self.GR[loc], B)                     # B in the centre
                be.axpby(-self.E[loc], B, 1.0, Bn)
                if lBs[loc] is not None:                                              # B to the left
                    be.axpby(1.0, be.dAC(H[loc], lBs[loc][k], self.GR[loc], self.AR[loc]), 1.0, Bn)
                if rBs[loc] is not None:                                              # B to the right
                    be.axpby(1.0, be.dAC(H[loc], self.GL[loc], rBs[loc][k], self.AL[loc]), 1.0, Bn)
                be.gemm(phi.VLs[loc], Bn.reshape(Dl * d, Bn.shape[2]), transA=True, out=phi.X(k, loc, out))   # setindex! :101
        return out


def _times_i_vec(be, phi, v):
    """i v on [Re | Im]."""
    out = be.empty(v.shape)
    N = phi.N
    be.lincomb([_view(v, N, (N,))], [-1.0], out=_view(out, 0, (N,)))
    be.lincomb([_view(v, 0, (N,))], [1.0], out=_view(out, N, (N,)))
    return out


def excitations_qp(H, alg: QuasiparticleAnsatz, phi0: LeftGaugedQP, lenvs=None, renvs=None, num=1, device=False):
    """excitations(H, alg, phi0::QP, lenvs, renvs; num)  :39-64,127-143 -> (energies, [LeftGaugedQP]).  device=True: the
    fused route of _QPContext (mpsk_qp_heff_site, pair transfers); the default is the composed one."""
    be = phi0.be
    lenvs = _environments(phi0.left_gs, H) if lenvs is None else lenvs
    ctx = _QPContext(H, phi0, lenvs, alg, renvs, device)
    eig_ws = krylov.KrylovWorkspace(be)      # NOT ctx.ws: the GMRES solves run inside this solver's matvec
    found, Es = [], []
    for _ in range(num):
        def op(x, out):
            ctx.heff(phi0, x, out)
            for f, lf in zip(found, Es):       # states already found are shifted up out of the way
                be.axpby((10.0 + 10.0 * abs(lf)) * be.dot(f, x), f, 1.0, out)
            return out
        lam, v, _, res = krylov.eigsolve_sr(be, op, phi0.vec, tol=alg.tol, krylovdim=alg.krylovdim, maxiter=alg.maxiter,
                                            ws=eig_ws)
        if res > alg.tol:
            import warnings
            warnings.warn(f"excitation failed to converge: normres = {res:.3e}")     # :47-48
        v = be.copy(v)
        Es.append(float(lam))
        found.append(v)
        if phi0.nparts == 2:
            found.append(_times_i_vec(be, phi0, v))
            Es.append(float(lam))
    keep = range(0, len(found), phi0.nparts)
    return [Es[k] for k in keep], [phi0.with_vec(found[k]) for k in keep]


def excitations_momenta(H, alg: QuasiparticleAnsatz, momenta, psi, lenvs=None, rpsi=None, renvs=None, num=1, rng=None,
                        device=False):
    """excitations(H, alg, momentum | momenta, lmps::InfiniteMPS, lenvs, rmps, renvs; num)  :84-125.  A scalar momentum
    returns (energies[num], states[num]); a list returns (E[len(momenta), num], states[len(momenta)][num]).  rmps different
    from lmps: domain-wall (topologically non-trivial) excitations between two ground states."""
    lenvs = _environments(psi, H) if lenvs is None else lenvs
    rpsi = psi if rpsi is None else rpsi
    renvs = (lenvs if rpsi is psi else _environments(rpsi, H)) if renvs is None else renvs
    rng = np.random.default_rng(0) if rng is None else rng
    if np.isscalar(momenta):
        return excitations_qp(H, alg, LeftGaugedQP.random(psi, momenta, rng, rpsi), lenvs, renvs, num, device)
    Ep, Bp = [], []
    for p in momenta:
        e, b = excitations_qp(H, alg, LeftGaugedQP.random(psi, float(p), rng, rpsi), lenvs, renvs, num, device)
        Ep.append(e)
        Bp.append(b)
    return np.array(Ep), Bp


# ======================================================================================================================
# Statistical-mechanics excitations: excitations(H::DenseMPO | MPOMultiline, QuasiparticleAnsatz(), momentum, psi, envs)
# (quasiparticleexcitation.jl:170-228 dispatch, :258-293 effective operator, qpenv.jl:171-303 environments)
# ======================================================================================================================
# device=None picks the route per slice kind from the measured table (tools/bench_qp_statmech.py,
# profiles/qp_statmech_timings.json, README): "mix" = slices whose MPO stage is the slab mix (chi d below the crossover of
# mpsk_mposlice_create_dense), "gemm" = slices whose MPO stage is a GEMM of its own.
FUSED_BY_DEFAULT = {"mix": True, "gemm": True}


def _slice_kind(O):
    import os
    ev = os.environ.get("MPSK_DENSE_ROUTE", "")
    if ev[:1] in ("0", "1"):
        return "gemm" if ev[0] == "1" else "mix"
    return "gemm" if min(O.Wl, O.Wr) * O.d >= 8 else "mix"


def _use_fused(be, device, O):
    has = all(hasattr(be, m) for m in ("qp_half", "qp_apply", "transfer_left_pair", "transfer_right_pair"))
    if device and not has:
        from ._lib import MpskError
        raise MpskError("device=True: this backend has no mpsk_qp_apply / pair transfers")
    if device is None:
        return has and FUSED_BY_DEFAULT[_slice_kind(O)]
    return bool(device)


def _cscale(be, z, s):
    """(re, im) * s for a complex scalar s."""
    re, im = z
    a, b = float(np.real(s)), float(np.imag(s))
    return [be.lincomb([re, im], [a, -b]), be.lincomb([re, im], [b, a])]


class _StatmechContext:
    """Everything of the effective operator that depends neither on the momentum nor on X: per (row, column) the slice, the
    tensors of the row above and the row below, the environments, the site eigenvalue lam = <AC_below, H_AC AC_above> (its
    inverse is the reference's left_renorms = right_renorms of a topologically trivial excitation, qpenv.jl:205-226, and lam
    itself the `en` every site of the result is divided by, quasiparticleexcitation.jl:267-271), the fixed points
    that regularise the two mixed transfer matrices (qpenv.jl:259-271), and on the fused route the B-independent halves.

    Rows of different bond dimensions: the reference writes `en` and the lvec of tm_LR with the legs of the two rows
    exchanged, which is the same number only when the rows are equal; here both are contracted as the network
    dictates (bra legs with the row below), and they agree with the reference whenever its expressions are defined."""

    def __init__(self, psi, rows_env, alg, device):
        self.be = be = psi.be
        self.alg = alg
        self.R, self.n = R, n = psi.shape
        self.psi = psi
        self.O = [[rows_env[r].O(c) for c in range(n)] for r in range(R)]
        self.GL = [[rows_env[r].lw[c] for c in range(n)] for r in range(R)]
        self.GR = [[rows_env[r].rw[c] for c in range(n)] for r in range(R)]
        self.fused = _use_fused(be, device, self.O[0][0])
        self.lam = [[be.dot(psi.AC[r + 1, c], self._proj(self.O[r][c], self.GL[r][c], self.GR[r][c], psi.AC[r, c]))
                     for c in range(n)] for r in range(R)]
        self.ws = krylov.KrylovWorkspace(be)
        self.Ll, self.Rl, self.Rr, self.Lr = [], [], [], []
        for r in range(R):
            Ca, Cb = psi.CR[r, n - 1], psi.CR[r + 1, n - 1]
            gl, gr = self.GL[r][0], self.GR[r][n - 1]
            W = gl.shape[0]
            sl = lambda t, w: _view(t, w * t.shape[1] * t.shape[2], t.shape[1:])
            Ll, Rl, Rr, Lr = be.empty(gl.shape), be.empty(gl.shape), be.empty(gr.shape), be.empty(gr.shape)
            for w in range(W):
                be.gemm(sl(gl, w), Ca, out=sl(Ll, w))                       # left fixed point of T(AR above, AL below)
                be.gemm(Cb, sl(gr, w), transB=True, out=sl(Rl, w))          # its right fixed point, slabs transposed
                be.gemm(Ca, sl(gr, w), out=sl(Rr, w))                       # right fixed point of T(AL above, AR below)
                be.gemm(sl(gl, w), Cb, transA=True, out=sl(Lr, w))          # its left fixed point, slabs transposed
            self.Ll.append(Ll), self.Rl.append(Rl), self.Rr.append(Rr), self.Lr.append(Lr)
        self.half = None
        if self.fused:                                                       # once per site and ground state
            self.half = [[be.qp_half(self.O[r][c], self.GL[r][c], psi.AL[r, c]) for c in range(n)] for r in range(R)]

    # ---- the two routes ----
    def _proj(self, O, GL, GR, x):
        be = self.be
        if hasattr(be, "dAC_proj"):
            return be.dAC_proj(O, GL, GR, x)
        return be.dAC(O, GL, GR, x, out=be.empty(GL.shape[1], x.shape[1], GR.shape[2]))

    def _tl(self, O, V, A, Ab):
        f = getattr(self.be, "transfer_left_ex", None)
        return f(O, V, A, Ab) if f is not None else self.be.transfer_left(O, V, A, Ab)

    def _tr(self, O, V, A, Ab):
        f = getattr(self.be, "transfer_right_ex", None)
        return f(O, V, A, Ab) if f is not None else self.be.transfer_right(O, V, A, Ab)

    def _tl_pair(self, O, V1, A1, V2, A2, Ab):
        be = self.be
        if self.fused:
            return be.transfer_left_pair(O, V1, A1, V2, A2, Ab)
        return be.axpby(1.0, self._tl(O, V2, A2, Ab), 1.0, self._tl(O, V1, A1, Ab))

    def _tr_pair(self, O, V1, A1, V2, A2, Ab):
        be = self.be
        if self.fused:
            return be.transfer_right_pair(O, V1, A1, V2, A2, Ab)
        return be.axpby(1.0, self._tr(O, V2, A2, Ab), 1.0, self._tr(O, V1, A1, Ab))

    def _local(self, r, c, B, lB, rB):
        """T = GL B O GR + lB AR O GR + GL AL O rB   (quasiparticleexcitation.jl:273-286), one real part."""
        be, psi = self.be, self.psi
        O, GL, GR = self.O[r][c], self.GL[r][c], self.GR[r][c]
        if self.fused:
            return be.qp_apply(O, GL, GR, B, lB, psi.AR[r, c], self.half[r][c], rB)
        T = self._proj(O, GL, GR, B)
        be.axpby(1.0, self._proj(O, lB, GR, psi.AR[r, c]), 1.0, T)
        be.axpby(1.0, self._proj(O, GL, rB, psi.AL[r, c]), 1.0, T)
        return T

    # ---- qpenv.jl:171-303 for one row ----
    def _geometric_sum(self, left, r, b, coef):
        """x = b + coef x T_reg (left) / b + coef T_reg x (right): one GMRES solve on the planar pair (qpenv.jl:273-283)."""
        be, psi, n = self.be, self.psi, self.n
        shape, sz = b[0].shape, b[0].size
        flat = be.empty(2 * sz)
        for k in range(2):
            flat.buf[k * sz:(k + 1) * sz].copy_(b[k].buf[:sz])
        lv, rv = (self.Rl[r], self.Ll[r]) if left else (self.Lr[r], self.Rr[r])
        a, bb = float(np.real(coef)), float(np.imag(coef))

        def op(x, out):
            ys = []
            for k in range(2):
                v = _view(x, k * sz, shape)
                if left:
                    for c in range(n):
                        v = self._tl(self.O[r][c], v, psi.AR[r, c], psi.AL[r + 1, c])
                else:
                    for c in range(n - 1, -1, -1):
                        v = self._tr(self.O[r][c], v, psi.AL[r, c], psi.AR[r + 1, c])
                be.axpby(-be.dot(v, lv), rv, 1.0, v)                        # regularize!(v, lvec, rvec), transfermatrix.jl:83-85
                ys.append(v)
            xs = [_view(x, k * sz, shape) for k in range(2)]
            be.lincomb([xs[0], ys[0], ys[1]], [1.0, -a, bb], out=_view(out, 0, shape))
            be.lincomb([xs[1], ys[0], ys[1]], [1.0, -bb, -a], out=_view(out, sz, shape))
            return out

        sol = krylov.gmres(be, op, flat, flat, tol=self.alg.solver_tol, maxiter=self.alg.solver_maxiter, ws=self.ws)
        return [be.copy(_view(sol, k * sz, shape)) for k in range(2)]

    def qp_envs(self, r, Bs, p):
        be, psi, n = self.be, self.psi, self.n
        O, GL, GR = self.O[r], self.GL[r], self.GR[r]
        ARa, ALa = [psi.AR[r, c] for c in range(n)], [psi.AL[r, c] for c in range(n)]
        ALb, ARb = [psi.AL[r + 1, c] for c in range(n)], [psi.AR[r + 1, c] for c in range(n)]
        ren = [1.0 / self.lam[r][c] for c in range(n)]
        el, er = np.exp(-1j * p), np.exp(1j * p)
        lBs, rBs = [None] * n, [None] * n
        cur = None
        for c in range(n):                                                   # :238-244
            if cur is None:
                nxt = [self._tl(O[c], GL[c], Bs[c][k], ALb[c]) for k in range(2)]
            else:
                nxt = [self._tl_pair(O[c], cur[k], ARa[c], GL[c], Bs[c][k], ALb[c]) for k in range(2)]
            cur = lBs[c] = _cscale(be, nxt, ren[c] * el)
        cur = None
        for c in range(n - 1, -1, -1):                                       # :246-252
            if cur is None:
                nxt = [self._tr(O[c], GR[c], Bs[c][k], ARb[c]) for k in range(2)]
            else:
                nxt = [self._tr_pair(O[c], cur[k], ALa[c], GR[c], Bs[c][k], ARb[c]) for k in range(2)]
            cur = rBs[c] = _cscale(be, nxt, ren[c] * er)
        prod = float(np.prod(ren))
        lBs[n - 1] = self._geometric_sum(True, r, lBs[n - 1], el ** n * prod)      # :273-277
        rBs[0] = self._geometric_sum(False, r, rBs[0], er ** n * prod)             # :279-283
        cur = lBs[n - 1]
        for c in range(n - 1):                                               # :285-291
            cur = _cscale(be, [self._tl(O[c], cur[k], ARa[c], ALb[c]) for k in range(2)], ren[c] * el)
            _acc(be, lBs[c], cur)
        cur = rBs[0]
        for c in range(n - 1, 0, -1):                                        # :293-299
            cur = _cscale(be, [self._tr(O[c], cur[k], ALa[c], ARb[c]) for k in range(2)], ren[c] * er)
            _acc(be, rBs[c], cur)
        return lBs, rBs


class MultilineQP:
    """Multiline{<:InfiniteQP}: one LeftGaugedQP per row on one flat device vector [Re rows | Im rows].  qp[r] is the row
    as a LeftGaugedQP of its own (two parts)."""

    def __init__(self, rows, momentum, vec=None):
        self.be = rows[0].be
        self.rows, self.momentum = rows, float(momentum)
        self.Ns = [q.N for q in rows]
        self.roff = np.concatenate([[0], np.cumsum(self.Ns)]).astype(int)
        self.N = int(self.roff[-1])
        if vec is None:
            vec = self.be.empty(2 * self.N)
            for r, q in enumerate(rows):
                for k in range(2):
                    dst = _view(vec, k * self.N + int(self.roff[r]), (q.N,))
                    if k < q.nparts:
                        self.be.axpby(1.0, _view(q.vec, k * q.N, (q.N,)), 0.0, dst)
                    else:
                        self.be.scal(0.0, dst)
        self.vec = vec

    def __len__(self):
        return len(self.rows)

    def X(self, part, r, c, vec=None):
        q = self.rows[r % len(self.rows)]
        vec = self.vec if vec is None else vec
        return _view(vec, part * self.N + int(self.roff[r % len(self.rows)]) + int(q.offs[c]), q.xshapes[c])

    def B(self, part, r, c, vec=None):
        q = self.rows[r % len(self.rows)]
        Dl, d, _ = q.left_gs.AL[c].shape
        return self.be.gemm(q.VLs[c], self.X(part, r, c, vec)).reshape(Dl, d, q.xshapes[c][1])

    def __getitem__(self, r):
        q = self.rows[r % len(self.rows)]
        be = self.be
        v = be.empty(2 * q.N)
        for k in range(2):
            be.axpby(1.0, _view(self.vec, k * self.N + int(self.roff[r % len(self.rows)]), (q.N,)), 0.0, _view(v, k * q.N, (q.N,)))
        return LeftGaugedQP(q.left_gs, q.VLs, q.xshapes, self.momentum, v, 2)

    def with_vec(self, vec):
        return MultilineQP(self.rows, self.momentum, vec)


def _statmech_heff(ctx: _StatmechContext, phi: MultilineQP, x: DTensor, out: DTensor):
    """effective_excitation_hamiltonian(H::MPOMultiline, phi)  :258-293: row r + 1 of the result from row r of the input,
    every site divided by its own en."""
    be, R, n = ctx.be, ctx.R, ctx.n
    for r in range(R):
        Bs = [[phi.B(k, r, c, x) for k in range(2)] for c in range(n)]
        lBs, rBs = ctx.qp_envs(r, Bs, phi.momentum)
        q = phi.rows[(r + 1) % R]
        for c in range(n):
            for k in range(2):
                T = ctx._local(r, c, Bs[c][k], lBs[(c - 1) % n][k], rBs[(c + 1) % n][k])
                Dl, d, Dr = T.shape
                be.gemm(q.VLs[c], T.reshape(Dl * d, Dr), transA=True, alpha=1.0 / ctx.lam[r][c], out=phi.X(k, r + 1, c, out))
    return out


def excitations_statmech(H, alg: QuasiparticleAnsatz, momenta, psi, envs=None, rpsi=None, renvs=None, num=1, rng=None,
                         device=None):
    """excitations(H::DenseMPO | MPOMultiline, QuasiparticleAnsatz(), momentum | momenta | [LeftGaugedQP per row], psi[, envs];
    num)  (quasiparticleexcitation.jl:170-228): the `num` largest-magnitude (:LM) eigenvalues of the effective operator of
    the row-to-row transfer matrix on the quasiparticle tangent space, normalised by the leading eigenvalue per site, so that
    |E| = exp(-eps(p)) with eps the excitation's inverse correlation length at momentum p.

    A DenseMPO with an InfiniteMPS of any unit cell is converted to one row (:202-216) and its states come back as
    LeftGaugedQP; an MPOMultiline with an MPSMultiline gives MultilineQP states (one LeftGaugedQP per row, qp[r]).  A scalar
    momentum returns (E[num] complex, states[num]); a list returns (E[len(momenta), num], states[len(momenta)][num]).

    The operator is not Hermitian and an eigenvector can be complex at any momentum, p = 0 included, so a
    statistical-mechanics quasiparticle always carries two real parts [Re | Im] and every kernel runs once per part: at
    p = 0 and p = pi this costs a factor of two over what a real vector would need (the Hamiltonian method carries one part
    there).  The eigensolver is the complex Arnoldi of krylov.eigsolve_lm_planar.

    device: None = the route FUSED_BY_DEFAULT gives for the slice kind, True = insist on mpsk_qp_apply and the pair
    transfers (mpsk_qp_half once per site per call), False = the composed route (mpsk_dAC_proj, the _ex transfers, axpby),
    which is also what a backend without the new entries runs."""
    from . import multiline, statmech
    if rpsi is not None and rpsi is not psi:
        raise NotImplementedError("excitations of a transfer matrix between two different ground states are not built: "
                                  "\"there is a phase ambiguity in topologically nontrivial statmech excitations\" "
                                  "(qpenv.jl:176-177)")
    one_row = isinstance(H, statmech.DenseMPO) and not isinstance(psi, multiline.MPSMultiline)
    if one_row:                                                              # :202-216
        envs = statmech.environments(psi, H) if envs is None else envs
        envs.leftenv(0, psi)
        rows_env = [envs]
        psi = multiline.MPSMultiline(psi)
    else:
        H = multiline.MPOMultiline(H) if isinstance(H, statmech.DenseMPO) else H
        if not isinstance(H, multiline.MPOMultiline) or not isinstance(psi, multiline.MPSMultiline):
            raise TypeError("excitations of a transfer matrix take (DenseMPO, InfiniteMPS) or (MPOMultiline, MPSMultiline)")
        envs = multiline.environments(psi, H) if envs is None else envs
        envs._fresh(psi)
        rows_env = envs.sub
    be = psi.be
    rng = np.random.default_rng(0) if rng is None else rng
    R = psi.shape[0]
    ctx = _StatmechContext(psi, rows_env, alg, device)

    def solve(phi0: MultilineQP):
        def op(x, out):
            return _statmech_heff(ctx, phi0, x, out)
        vals, vecs, _, conv = krylov.eigsolve_lm_planar(be, op, phi0.vec, num=num, tol=alg.tol, krylovdim=alg.krylovdim,
                                                        maxiter=alg.maxiter)
        if conv < num:
            import warnings
            warnings.warn("excitation failed to converge")                  # :184-185
        states = [phi0.with_vec(v) for v in vecs]
        return vals, [s[0] for s in states] if one_row else states

    def start(p):
        rows = []
        for r in range(R):
            q = LeftGaugedQP.random(psi[r], p, rng)
            rows.append(LeftGaugedQP(psi[r], q.VLs, q.xshapes, float(p), be.upload(rng.random(2 * q.N)), 2))
        return MultilineQP(rows, p)

    if isinstance(momenta, LeftGaugedQP):
        momenta = [momenta]
    if isinstance(momenta, (list, tuple)) and momenta and isinstance(momenta[0], LeftGaugedQP):
        if len(momenta) != R:
            raise ValueError(f"{len(momenta)} quasiparticle rows for a state of {R} rows")
        for r, q in enumerate(momenta):
            if not q.trivial:
                raise NotImplementedError("\"there is a phase ambiguity in topologically nontrivial statmech excitations\" "
                                          "(qpenv.jl:176-177): domain-wall excitations of a transfer matrix are not built")
            if q.left_gs is not psi[r]:
                raise ValueError(f"quasiparticle row {r} was built on another ground state")
        return solve(MultilineQP(list(momenta), momenta[0].momentum))
    if np.isscalar(momenta):
        return solve(start(float(momenta)))
    Ep, Bp = [], []
    for p in momenta:
        e, b = solve(start(float(p)))
        Ep.append(e)
        Bp.append(b)
    return np.array(Ep), Bp
