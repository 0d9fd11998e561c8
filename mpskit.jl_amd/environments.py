"""Environment caches on the device: FinEnv (src/environments/FinEnv.jl:9-145) and MPOHamInfEnv
(src/environments/mpohaminfenv.jl:4-215).  Each environment is ONE device tensor of W slabs
(include/mpsk.h layout); an update is one mpsk_transfer_left / mpsk_transfer_right call."""
from __future__ import annotations

import numpy as np

from .backend import Backend, DTensor
from . import krylov


def _start_env(be: Backend, chis, D, active_level):
    """FinEnv.jl:49-67: identity (x) ones(chi_i) on the active level, zeros elsewhere."""
    W = sum(chis)
    host = np.zeros((W, D, D))
    off = 0
    for i, chi in enumerate(chis):
        if i == active_level:
            for k in range(chi):
                host[off + k] = np.eye(D)
        off += chi
    t = be.upload(np.transpose(host, (1, 2, 0)))       # logical (D, D, W) -> column-major slabs
    return DTensor(t.buf, (W, D, D))


class FinEnv:
    """Cache of L+1 left / right environments with identity(`is`)-based invalidation
    (FinEnv.jl:114-145): an AL/AR that was invalidated and recomputed is a new object, so the
    environments that depend on it are rebuilt exactly when the reference rebuilds them."""

    def __init__(self, psi, H, leftstart=None, rightstart=None):
        """leftstart / rightstart: the environments left of site 0 / right of site L-1 when they are not the trivial ones
        of a finite chain (window.WindowEnv, FinEnv.jl:84-89)"""
        be = self.be = psi.be
        L = len(psi)
        self.H = H
        self.opp = [H[i] for i in range(L)]
        odim = H.odim
        if leftstart is None:
            leftstart = _start_env(be, self.opp[0].chil, psi.AL(0).shape[0], 0)
        if rightstart is None:
            t = psi.ARs[L - 1] if psi.ARs[L - 1] is not None else psi.AL(L - 1)
            rightstart = _start_env(be, self.opp[L - 1].chir, t.shape[2], odim - 1)
        self.leftenvs = [leftstart] + [None] * L
        self.rightenvs = [None] * L + [rightstart]
        self.ldeps = [None] * L
        self.rdeps = [None] * L
        self.n_transfers = 0
        self.canonical = True          # MultipleEnvironments switches it off for the terms of a sum

    def _canonical(self, psi):
        """the condition ddAC uses for mode 3: a plain FinEnv on a real state keeps level 0 of every left environment and
        level W-1 of every right environment the identity, and AL / AR are isometries -- the promise behind the canonical
        route of mpsk_transfer_left_ex / mpsk_transfer_right_ex.  Subclasses and backends without that entry: dense."""
        return (self.canonical and type(self) is FinEnv and not getattr(psi, "cplx", False)
                and hasattr(self.be, "transfer_left_ex"))

    def rightenv(self, ind, psi):  # FinEnv.jl:114-129
        L = len(psi)
        a = None
        for i in range(L - 1, ind, -1):
            if psi.AR(i) is not self.rdeps[i]:
                a = i
                break
        if a is not None:
            kw = {"canonical": True} if self._canonical(psi) else {}
            for j in range(a, ind, -1):
                ar = psi.AR(j)
                self.rightenvs[j] = self.be.transfer_right(self.opp[j], self.rightenvs[j + 1], ar, ar, **kw)
                self.rdeps[j] = ar
                self.n_transfers += 1
        return self.rightenvs[ind + 1]

    def leftenv(self, ind, psi):  # FinEnv.jl:131-145
        a = None
        for i in range(0, ind):
            if psi.AL(i) is not self.ldeps[i]:
                a = i
                break
        if a is not None:
            kw = {"canonical": True} if self._canonical(psi) else {}
            for j in range(a, ind):
                al = psi.AL(j)
                self.leftenvs[j + 1] = self.be.transfer_left(self.opp[j], self.leftenvs[j], al, al, **kw)
                self.ldeps[j] = al
                self.n_transfers += 1
        return self.leftenvs[ind]

    def poison(self, ind):  # FinEnv.jl:108-111
        self.ldeps[ind] = None
        self.rdeps[ind] = None


def _start_env_pair(be: Backend, chis, D1, D2, active_level):
    """_start_env for two states: W slabs [D1, D2], the (rectangular) identity on the active level (FinEnv.jl:48-66 with
    l_LL / r_RR the trivial edge of a finite chain; D1 = D2 = 1 for the chains FiniteMPS.random builds)."""
    W = sum(chis)
    host = np.zeros((W, D1, D2))
    off = 0
    for i, chi in enumerate(chis):
        if i == active_level:
            host[off:off + chi] = np.eye(D1, D2)
        off += chi
    t = be.upload(np.transpose(host, (1, 2, 0)))
    return DTensor(t.buf, (W, D1, D2))


class FinEnvPair(FinEnv):
    """environments(below, (O, above)) / environments(below, above)  (FinEnv.jl:21-99): the environments of <below| O |above>.
    GL[w] is [D_below, D_above], GR[v] is [D_above, D_below]; an update is one mixed transfer with the ket tensor of `above`
    and the bra tensor of `below`.  Only `below` is tracked (FinEnv.jl:115,132): `above` is assumed not to change.
    O: MPOHamiltonian (right boundary on level odim - 1), SparseMPO (level 0, FinEnv.jl:61), a finite dense MPO (DenseMPO
    or a list of L tensors [Wl, d, d, Wr] with edge dimensions 1, FinEnv.jl:72-81) or None (plain overlap, :91-99)."""

    def __init__(self, below, O, above):
        from .operators import SparseMPO
        from .statmech import DenseMPO
        be = self.be = below.be
        L = len(below)
        if len(above) != L:
            raise ValueError(f"the two states have different lengths ({L} != {len(above)})")
        self.H, self.above = O, above
        edge = lambda psi: (psi.ARs[L - 1] if psi.ARs[L - 1] is not None else psi.AL(L - 1)).shape[2]
        Db0, Da0, DbL, DaL = below.AL(0).shape[0], above.AL(0).shape[0], edge(below), edge(above)
        if O is None:
            self.opp, chil, chir, ract = [None] * L, [1], [1], 0
        elif isinstance(O, (DenseMPO, list, tuple)):
            ts = [np.asarray(O[i], dtype=float) for i in range(L)]
            if len(O) != L or ts[0].shape[0] != 1 or ts[-1].shape[3] != 1:
                raise ValueError("a finite dense MPO needs one tensor per site and edge dimensions 1")
            mk = be.mposlice_dense if hasattr(be, "mposlice_dense") else \
                (lambda o: be.mposlice(1, o.shape[1], [o.shape[0]], [o.shape[3]], {(0, 0): o}))
            self.opp, chil, chir, ract = [mk(o) for o in ts], [1], [1], 0
        else:
            self.opp = [O[i] for i in range(L)]
            chil, chir = self.opp[0].chil, self.opp[L - 1].chir
            ract = 0 if isinstance(O, SparseMPO) else O.odim - 1
        self.leftenvs = [_start_env_pair(be, chil, Db0, Da0, 0)] + [None] * L
        self.rightenvs = [None] * L + [_start_env_pair(be, chir, DaL, DbL, ract)]
        self.ldeps = [None] * L
        self.rdeps = [None] * L
        self.n_transfers = 0
        self.canonical = False

    def rightenv(self, ind, psi):  # FinEnv.jl:114-129
        L = len(psi)
        a = None
        for i in range(L - 1, ind, -1):
            if psi.AR(i) is not self.rdeps[i]:
                a = i
                break
        if a is not None:
            for j in range(a, ind, -1):
                ar = psi.AR(j)
                self.rightenvs[j] = self.be.transfer_right(self.opp[j], self.rightenvs[j + 1], self.above.AR(j), ar)
                self.rdeps[j] = ar
                self.n_transfers += 1
        return self.rightenvs[ind + 1]

    def leftenv(self, ind, psi):  # FinEnv.jl:131-145
        a = None
        for i in range(0, ind):
            if psi.AL(i) is not self.ldeps[i]:
                a = i
                break
        if a is not None:
            for j in range(a, ind):
                al = psi.AL(j)
                self.leftenvs[j + 1] = self.be.transfer_left(self.opp[j], self.leftenvs[j], self.above.AL(j), al)
                self.ldeps[j] = al
                self.n_transfers += 1
        return self.leftenvs[ind]


class MultipleEnvironments:
    """MultipleEnvironments (src/environments/multipleenv.jl:1-62): one environment object per LazySum term."""

    def __init__(self, H, envs):
        self.H, self.envs = H, list(envs)
        if getattr(H, "timed", False):       # a timed sum folds its terms on canonical environments (mpsk_hsum, route 1)
            return
        for e in self.envs:                  # the terms of a sum keep the dense transfers (as ddAC keeps their dense operator)
            if isinstance(e, FinEnv):
                e.canonical = False

    def recalculate(self, psi, tol=None):
        for e in self.envs:
            e.recalculate(psi, tol)
        return self


def environments(psi, H, *args, **kw):
    """environments(window, H[, lenvs, renvs]): window.environments.  environments(psi, H)  (FinEnv.jl:41-70 / mpohaminfenv.jl:40-44 / multipleenv.jl:30-34; a DenseMPO:
    permpoinfenv.jl:20-29, an InfiniteMPS with H = (O, above): permpoinfenv.jl:29-42, both statmech.PerMPOInfEnv)."""
    from .states import FiniteMPS
    from .operators import LazySum, MultipliedOperator
    from .statmech import DenseMPO, PerMPOInfEnv
    from . import window
    if isinstance(psi, window.WindowMPS):                                       # FinEnv.jl:84-99
        return window.environments(psi, H, *args, **kw)
    if args:
        raise TypeError("environments(psi, H): start environments are taken for a WindowMPS only")
    from . import native_cplx
    if isinstance(psi, native_cplx.NativeInfiniteMPS):                         # interleaved complex uniform state
        return native_cplx.environments(psi, H, **kw)
    if isinstance(H, MultipliedOperator):                                       # multipliedoperator.jl:50-52
        return environments(psi, H.op, **kw)
    if isinstance(psi, FiniteMPS) and isinstance(H, (tuple, FiniteMPS)):       # FinEnv.jl:21-23, :91-99
        O, above = H if isinstance(H, tuple) else (None, H)
        return FinEnvPair(psi, O, above)
    if isinstance(H, tuple):                                                    # permpoinfenv.jl:29-42
        from .statmech import environments as _mixed
        return _mixed(psi, H, **kw)
    if isinstance(H, DenseMPO):
        return PerMPOInfEnv(psi, H, **kw)
    from .multiline import MPSMultiline
    if isinstance(psi, MPSMultiline):                                           # permpoinfenv.jl:23-27
        return PerMPOInfEnv(psi, H, **kw)
    if isinstance(H, LazySum):
        return MultipleEnvironments(H, [environments(psi, h, **kw) for h in H])
    if isinstance(psi, FiniteMPS):
        return FinEnv(psi, H)
    return MPOHamInfEnv(psi, H, **kw)


class MPOHamInfEnv:
    """Infinite-MPS Hamiltonian environments: level-by-level triangular solve, GMRES on the
    regularised transfer matrix for identity levels (mpohaminfenv.jl:76-215).  Level i of site s is
    stored as its own (chi, D, D) device tensor; a site's full environment for the matvec kernels
    is assembled (device-to-device) on demand.
    This class owns the algorithm: which level is zeroed, when a cycle runs, which bond's fixed point regularises which site.
    The arithmetic sits in the methods under "leaves"; native_cplx.NativeMPOHamInfEnv overrides exactly those for interleaved
    complex storage, level tensors (chi, 2 D, D)."""

    def __init__(self, psi, H, tol=1e-12, maxiter=100, rng=None):
        self.be = psi.be
        self.H, self.tol, self.maxiter = H, tol, maxiter
        self.rng = np.random.default_rng(0) if rng is None else rng
        self._start(psi)
        self.ws = krylov.KrylovWorkspace(self.be)
        self._cache = {}
        self.recalculate(psi, tol)

    def _start(self, psi):
        """random start environments in the bond spaces of psi (mpohaminfenv.jl:40-44)"""
        n, odim = len(psi), self.H.odim
        self._started = [self._bonds(psi, s) for s in range(n)]
        self.lw = [[self._random_level(self.O(s).chil[i], self._started[s][0]) for s in range(n)] for i in range(odim)]
        self.rw = [[self._random_level(self.O(s).chir[i], self._started[s][1]) for s in range(n)] for i in range(odim)]

    # ---- public ------------------------------------------------------------------------------
    def recalculate(self, psi, tol=None):
        tol = self._solve_tol(psi, tol)
        if self._started != [self._bonds(psi, s) for s in range(len(psi))]:
            self._start(psi)                     # the bond spaces changed (changebonds): the old solutions do not fit
        self._calclw(psi, tol)
        self._calcrw(psi, tol)
        self.dependency = psi
        self._cache = {}
        return self

    def _assemble(self, which, pos, n):
        key = (which, pos % n)
        if key not in self._cache:
            src = self.lw if which == "l" else self.rw
            parts = [src[i][pos % n] for i in range(self.H.odim)]
            W = sum(p.shape[0] for p in parts)
            out = self.be.empty(W, parts[0].shape[1], parts[0].shape[2])
            off = 0
            for p in parts:
                out.buf[off:off + p.size].copy_(p.buf[:p.size])
                off += p.size
            self._cache[key] = out
        return self._cache[key]

    def leftenv(self, pos, psi):
        if self.dependency is not psi:
            self.recalculate(psi)
        return self._assemble("l", pos, len(psi))

    def rightenv(self, pos, psi):
        if self.dependency is not psi:
            self.recalculate(psi)
        return self._assemble("r", pos, len(psi))

    def bytes(self):
        return 8 * sum(t.size for lv in self.lw + self.rw for t in lv) + 8 * sum(t.size for t in self._cache.values())

    # ---- leaves: the arithmetic of real storage --------------------------------------------------
    def O(self, s):
        """the slice of site s"""
        return self.H[s]

    def isid(self, i):
        return self.H.isid(i)

    def _bonds(self, psi, s):
        """(left, right) bond dimension of site s"""
        return psi.AL[s].shape[0], psi.AR[s].shape[2]

    def _solve_tol(self, psi, tol):
        """the tolerance of a recalculation that was asked for with `tol`: None is the constructor's"""
        return self.tol if tol is None else tol

    def _random_level(self, chi, D):
        t = self.be.upload(np.transpose(self.rng.random((chi, D, D)), (1, 2, 0)))
        return DTensor(t.buf, (chi, D, D))

    def _identity_level(self, chi, D):
        return DTensor(self.be.upload(np.transpose(np.stack([np.eye(D)] * chi), (1, 2, 0))).buf, (chi, D, D))

    def _eye(self, D):
        return self.be.upload(np.eye(D))

    def _CCd(self, psi, s):  # r_LL: C C^T of the bond right of site s
        c = psi.CR[s % len(psi)]
        return self.be.gemm(c, c, transB=True)

    def _CdC(self, psi, s):  # l_RR: C^T C of the bond left of site s
        c = psi.CR[(s - 1) % len(psi)]
        return self.be.gemm(c, c, transA=True)

    def _tl(self, v, s, i, j, A):
        """the (i -> j) block of the left transfer through site s: O scalar -> pass-through * O, dense -> MPO block."""
        be, O = self.be, self.O(s).blocks[(i, j)]
        if np.isscalar(O):
            out = be.transfer_left(None, v, A, A)
            if O != 1:
                be.scal(O, out)
            return out
        blk = be.mposlice(1, A.shape[1], [O.shape[0]], [O.shape[3]], {(0, 0): O})
        return be.transfer_left(blk, v, A, A)

    def _tr(self, v, s, i, j, A):
        be, O = self.be, self.O(s).blocks[(i, j)]
        if np.isscalar(O):
            out = be.transfer_right(None, v, A, A)
            if O != 1:
                be.scal(O, out)
            return out
        blk = be.mposlice(1, A.shape[1], [O.shape[0]], [O.shape[3]], {(0, 0): O})
        return be.transfer_right(blk, v, A, A)

    def _solve_identity(self, cell, lvec, rvec, b, x0, tol):
        """(1 - regularised T) x = b for an identity level: x -> x - [x T - <lvec, x T> rvec] with T = `cell`, one unit cell
        of pass-through transfers (transfermatrix.jl:29-33, :70-76)"""
        be = self.be

        def op(x, out):
            y = cell(x)
            be.regularize(y, lvec, rvec)
            be.axpby(1.0, x, 0.0, out)
            be.axpby(-1.0, y, 1.0, out)
            return out
        return krylov.gmres(be, op, b, x0, tol=tol, maxiter=self.maxiter, ws=self.ws)

    def _solve_plain(self, cell, b, x0, tol):
        """(1 - T) x = b for a diagonal level that is not the identity (mpohaminfenv.jl:109-115)"""
        be = self.be

        def op(x, out):
            y = cell(x)
            be.axpby(1.0, x, 0.0, out)
            be.axpby(-1.0, y, 1.0, out)
            return out
        return krylov.gmres(be, op, b, x0, tol=tol, maxiter=self.maxiter, ws=self.ws)

    def project(self, v, lvec, rvec):
        """regularize!(v, lvec, rvec) in place: v - <lvec, v> rvec, the contraction sum_xy lvec[x,y] v[y,x] per slab"""
        return self.be.regularize(v, lvec, rvec)

    # ---- the level solver: storage enters through the leaves above only (be.zeros / be.axpby serve either layout) ----
    def _left_cycle(self, idx, psi):  # mpohaminfenv.jl:177-195
        n, be = len(psi), self.be
        for s in range(n):
            acc = be.zeros(*self.lw[idx][(s + 1) % n].shape)
            for j in range(idx, -1, -1):
                if self.O(s).contains(j, idx):
                    be.axpby(1.0, self._tl(self.lw[j][s], s, j, idx, psi.AL[s]), 1.0, acc)
            self.lw[idx][(s + 1) % n] = acc

    def _right_cycle(self, idx, psi):  # :197-215
        n, be = len(psi), self.be
        for s in range(n - 1, -1, -1):
            acc = be.zeros(*self.rw[idx][(s - 1) % n].shape)
            for j in range(idx, self.H.odim):
                if self.O(s).contains(idx, j):
                    be.axpby(1.0, self._tr(self.rw[j][s], s, idx, j, psi.AR[s]), 1.0, acc)
            self.rw[idx][(s - 1) % n] = acc

    def _calclw(self, psi, tol):  # mpohaminfenv.jl:76-123
        n, odim, be = len(psi), self.H.odim, self.be
        D0 = self._bonds(psi, 0)[0]
        self.lw[0][0] = self._identity_level(self.O(0).chil[0], D0)
        if n > 1:
            self._left_cycle(0, psi)
        for i in range(1, odim):
            prev = self.lw[i][0]
            self.lw[i][0] = be.zeros(*prev.shape)
            self._left_cycle(i, psi)

            def cell(v, i=i):             # the diagonal block of level i through one unit cell; the bare transfer if it is 1
                for s in range(n):
                    v = self._tl(v, s, i, i, psi.AL[s])
                return v
            if self.isid(i):
                # the fixed points of the regulariser: r_LL = C C^dag of the last bond, contracted with v, and the identity
                lvec, rvec = self._CCd(psi, n - 1), self._eye(D0)
                self.lw[i][0] = self._solve_identity(cell, lvec, rvec, self.lw[i][0], prev, tol)
                if n > 1:
                    self._left_cycle(i, psi)
                for s in range(n):  # :103-107 subtract the fixed-point projection at every site
                    self.project(self.lw[i][s], self._CCd(psi, s - 1), self._eye(self._bonds(psi, s)[0]))
            else:
                if all(self.O(s).contains(i, i) for s in range(n)):
                    self.lw[i][0] = self._solve_plain(cell, self.lw[i][0], prev, tol)
                if n > 1:
                    self._left_cycle(i, psi)

    def _calcrw(self, psi, tol):  # :125-175
        n, odim, be = len(psi), self.H.odim, self.be
        DL = self._bonds(psi, n - 1)[1]
        self.rw[odim - 1][n - 1] = self._identity_level(self.O(n - 1).chir[odim - 1], DL)
        if n > 1:
            self._right_cycle(odim - 1, psi)
        for i in range(odim - 2, -1, -1):
            prev = self.rw[i][n - 1]
            self.rw[i][n - 1] = be.zeros(*prev.shape)
            self._right_cycle(i, psi)

            def cell(v, i=i):
                for s in range(n - 1, -1, -1):
                    v = self._tr(v, s, i, i, psi.AR[s])
                return v
            if self.isid(i):
                # l_RR = C^dag C of the bond left of site 0 (as `project` contracts it: lvec[x,y] v[y,x]) and the identity
                lvec, rvec = self._CdC(psi, 0), self._eye(DL)
                self.rw[i][n - 1] = self._solve_identity(cell, lvec, rvec, self.rw[i][n - 1], prev, tol)
                if n > 1:
                    self._right_cycle(i, psi)
                for s in range(n):
                    self.project(self.rw[i][s], self._CdC(psi, s + 1), self._eye(self._bonds(psi, s)[1]))
            else:
                if all(self.O(s).contains(i, i) for s in range(n)):
                    self.rw[i][n - 1] = self._solve_plain(cell, self.rw[i][n - 1], prev, tol)
                if n > 1:
                    self._right_cycle(i, psi)
