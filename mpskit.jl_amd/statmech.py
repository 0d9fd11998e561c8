"""Boundary contraction of 2D tensor networks with the reference's API: DenseMPO (src/operators/densempo.jl:4-17),
PerMPOInfEnv (src/environments/permpoinfenv.jl) and leading_boundary (src/algorithms/statmech/vumps.jl:15-92) for a
single-row InfiniteMPS, plus the classical transfer tensors of the reference's test setup (test/setup.jl:78-130).

Orchestration only: every matvec and transfer runs in libmpsk on dense MPO slices (mpsk_mposlice_create_dense, whose
middle contraction is an fp64 MFMA GEMM).  The leading (:LM) eigensolves are the restarted Arnoldi of
krylov.eigsolve_lm_real on the host.

Environments with above != below (permpoinfenv.jl:29-63, :138-189) serve approximate(psi::InfiniteMPS, (O, above), VOMPS())
(approximate.py): O a DenseMPO or a real SparseMPO, both environments rectangular, the tangent-space projections ac_proj /
c_proj (derivatives.jl:204-219) on mpsk_dAC_proj / mpsk_dC_proj.  Real tensors only.

More than one row: MPSMultiline / MPOMultiline and their environments and algorithms live in multiline.py; every entry point
here (PerMPOInfEnv, environments, calc_galerkin, expectation_value, leading_boundary) hands an MPSMultiline over to it."""
from __future__ import annotations

import math
import time

import numpy as np

from . import krylov
from .backend import DTensor
from .derivatives import MPO_ddAC, MPO_ddC
from .operators import SparseMPO
from .states import InfiniteMPS


class DenseMPO:
    """Periodic list of real MPO tensors O[w, t(out), s(in), v] (densempo.jl:4-17): len, repeat, [i] (periodic)."""

    def __init__(self, tensors):
        if isinstance(tensors, np.ndarray):
            tensors = [tensors]
        opp = []
        for t in tensors:
            a = np.asarray(t)
            if np.iscomplexobj(a):
                if np.abs(a.imag).max(initial=0.0) > 0:
                    raise NotImplementedError("DenseMPO: complex tensors are not supported (real fp64 only)")
                a = a.real
            if a.ndim != 4 or a.shape[1] != a.shape[2]:
                raise ValueError(f"DenseMPO tensor must be [Wl, d, d, Wr], got {a.shape}")
            opp.append(np.array(a, dtype=np.float64))
        for i, a in enumerate(opp):
            if a.shape[3] != opp[(i + 1) % len(opp)].shape[0]:
                raise ValueError("DenseMPO: the right bond of each tensor must match the left bond of the next")
        self.opp = opp
        self._slices = {}

    def __len__(self):
        return len(self.opp)

    def __getitem__(self, i):
        return self.opp[i % len(self.opp)]

    def __iter__(self):
        return iter(self.opp)

    def repeat(self, n):
        return DenseMPO(self.opp * int(n))

    @property
    def d(self):
        return self.opp[0].shape[1]

    def __mul__(self, st):
        """mpo * st  (densempo.jl:31-44): the exact product with an InfiniteMPS, bond dimension W D (the MPO bond is the
        fast index of the fused bond).  Built on the host from the downloaded AL tensors."""
        if not isinstance(st, InfiniteMPS):
            return NotImplemented
        if getattr(st, "cplx", False):
            raise NotImplementedError("DenseMPO * InfiniteMPS: complex states are not supported (real fp64 only)")
        if len(st) % len(self) != 0:
            raise ValueError(f"unit cell of the state ({len(st)}) is not a multiple of the MPO's ({len(self)})")
        out = []
        for i in range(len(st)):
            al, o = st.be.download(st.AL[i]), self[i]
            t = np.einsum("asb,wtsv->watvb", al, o)
            out.append(t.reshape(o.shape[0] * al.shape[0], o.shape[1], o.shape[3] * al.shape[2]))
        return InfiniteMPS.from_tensors(out, be=st.be)

    def slices(self, be):
        """Device slices on backend `be` (built once per backend through be.mposlice_dense)."""
        key = id(be)
        if key not in self._slices:
            self._slices[key] = (be, [be.mposlice_dense(o) for o in self.opp])
        return self._slices[key][1]


def _eig_lm(be, op, x0, tol, krylovdim, maxiter, ws=None):
    """Leading eigenvector of `op` from x0.  KrylovKit's tolerance is an absolute residual norm; the transfer operators
    here carry the partition function per tensor (kappa^(k^2) for a k x k cluster), so the tolerance is taken relative
    to the operator's scale |op x0| / |x0|."""
    y = op(x0)
    scale = be.norm(y) / be.norm(x0)
    return krylov.eigsolve_lm_real(be, op, x0, tol=tol * max(scale, 1e-300), krylovdim=krylovdim, maxiter=maxiter, ws=ws)


def _slab(t: DTensor, w):
    n = t.shape[1] * t.shape[2]
    return DTensor(t.buf[w * n:(w + 1) * n], t.shape[1:])


def dC_proj_composed(be, GL: DTensor, GR: DTensor, c: DTensor):
    """sum_w GL[w] c GR[w] from plain products, one pair per slab: the route of backends without dC_proj."""
    acc = None
    for w in range(GL.shape[0]):
        y = be.gemm(be.gemm(_slab(GL, w), c), _slab(GR, w))
        acc = y if acc is None else be.axpby(1.0, y, 1.0, acc)
    return acc


def _no_cplx_inf(what, *objs):
    if any(getattr(o, "cplx", False) for o in objs):
        raise NotImplementedError(f"{what}: complex states / operators are not supported on uniform states (real fp64 only)")


class PerMPOInfEnv:
    """Environments of a DenseMPO / real SparseMPO on a single-row InfiniteMPS (permpoinfenv.jl): lw[i] / rw[i] are the left /
    right environments of site i in the slab layout, W = the MPO bond at that side of the site.  above = None: above == below,
    slabs (W, D, D).  above = an InfiniteMPS: the state the operator is applied to (permpoinfenv.jl:29-42), fixed for the life
    of the object, lw[i] (W, D_below, D_above) and rw[i] (W, D_above, D_below); `psi` is then the state below."""

    def __new__(cls, psi=None, *args, **kw):
        from .multiline import MPSMultiline, MultilineEnv
        if cls is PerMPOInfEnv and isinstance(psi, MPSMultiline):      # (MPSMultiline, MPOMultiline): the multi-row form
            return object.__new__(MultilineEnv)
        return object.__new__(cls)

    def __init__(self, psi, mpo, tol=1e-12, krylovdim=30, maxiter=100, rng=None, above=None):
        if not isinstance(mpo, (DenseMPO, SparseMPO)):
            raise TypeError(f"PerMPOInfEnv takes a DenseMPO or a SparseMPO, not {type(mpo).__name__}")
        _no_cplx_inf("environments", psi, mpo, above)
        if len(psi) % len(mpo) != 0:
            raise ValueError(f"unit cell of the state ({len(psi)}) is not a multiple of the MPO's ({len(mpo)})")
        if above is not None and len(above) != len(psi):
            raise ValueError(f"unit cells of the states above ({len(above)}) and below ({len(psi)}) differ")
        self.be, self.opp, self.above = psi.be, mpo, above
        self.tol, self.krylovdim, self.maxiter = tol, krylovdim, maxiter
        self.rng = np.random.default_rng(0) if rng is None else rng
        if isinstance(mpo, SparseMPO):
            if mpo.be is None:
                mpo.be = self.be
            if mpo.be is not self.be:
                raise ValueError("the SparseMPO and the state live on different backends")
            self.slices = mpo.slices
        else:
            self.slices = mpo.slices(self.be)
        self.ws = krylov.KrylovWorkspace(self.be)
        self.lw = self.rw = None
        self.dependency = None
        self.recalculate(psi, tol)

    def O(self, pos):
        return self.slices[pos % len(self.slices)]

    # ---- public ------------------------------------------------------------------------------
    def recalculate(self, psi, tol=None):
        """permpoinfenv.jl recalculate!: restart from the previous fixed points when the bond spaces of the state below are
        unchanged, from random start vectors otherwise (gen_init_fps, permpoinfenv.jl:97-136)."""
        tol = self.tol if tol is None else tol
        n = len(psi)
        old = self.dependency
        same = (old is not None and len(old) == n and
                all(a.shape == b.shape for a, b in zip(old.CR, psi.CR)))
        if same:
            L0, R0 = self.be.copy(self.lw[0]), self.be.copy(self.rw[n - 1])
        elif self.above is None:
            L0 = self._random(self.O(0).Wl, psi.AL[0].shape[0])
            R0 = self._random(self.O(n - 1).Wr, psi.AR[n - 1].shape[2])
        else:
            if len(psi) != len(self.above):
                raise ValueError(f"unit cells of the states above ({len(self.above)}) and below ({len(psi)}) differ")
            L0 = self._random(self.O(0).Wl, psi.AL[0].shape[0], self.above.AL[0].shape[0])
            R0 = self._random(self.O(n - 1).Wr, self.above.AR[n - 1].shape[2], psi.AR[n - 1].shape[2])
        self.lw, self.rw = self._mixed_fixpoints(psi, L0, R0, tol)
        self.dependency = psi
        self.tol = tol
        return self

    def leftenv(self, pos, psi):
        if self.dependency is not psi:
            self.recalculate(psi)
        return self.lw[pos % len(psi)]

    def rightenv(self, pos, psi):
        if self.dependency is not psi:
            self.recalculate(psi)
        return self.rw[pos % len(psi)]

    def ddAC(self, pos, psi):
        return MPO_ddAC(self.be, self.O(pos), self.leftenv(pos, psi), self.rightenv(pos, psi))

    def ddC(self, pos, psi):
        return MPO_ddC(self.be, self.leftenv(pos + 1, psi), self.rightenv(pos, psi))

    def ac_proj(self, pos, below):
        """ac_proj(row, col, below, envs)  (derivatives.jl:216-219): dAC of above.AC[pos] on the environments of `below`."""
        be = self.be
        above = below if self.above is None else self.above
        GL, GR, x = self.leftenv(pos, below), self.rightenv(pos, below), above.AC[pos % len(above)]
        if hasattr(be, "dAC_proj"):
            return be.dAC_proj(self.O(pos), GL, GR, x)
        return be.dAC(self.O(pos), GL, GR, x, out=be.empty(GL.shape[1], x.shape[1], GR.shape[2]))

    def c_proj(self, pos, below):
        """c_proj(row, col, below, envs)  (derivatives.jl:204-207): dC of above.CR[pos] on the environments of `below`."""
        above = below if self.above is None else self.above
        return self._dC(self.leftenv(pos + 1, below), self.rightenv(pos, below), above.CR[pos % len(above)])

    # ---- helpers -------------------------------------------------------------------------------
    def _random(self, W, D, D2=None):
        D2 = D if D2 is None else D2
        return self.be.upload(self.rng.standard_normal(W * D * D2)).reshape(W, D, D2)

    def _dC(self, GL, GR, c):
        if hasattr(self.be, "dC_proj"):
            return self.be.dC_proj(GL, GR, c)
        return dC_proj_composed(self.be, GL, GR, c)

    def _mixed_fixpoints(self, psi, L0, R0, tol):  # permpoinfenv.jl:138-189 (one row)
        be, n = self.be, len(psi)
        top = psi if self.above is None else self.above

        def tl(v, out=None):
            for i in range(n):
                v = be.transfer_left(self.O(i), v, top.AL[i], psi.AL[i])
            return v if out is None else be.axpby(1.0, v, 0.0, out)

        def tr(v, out=None):
            for i in range(n - 1, -1, -1):
                v = be.transfer_right(self.O(i), v, top.AR[i], psi.AR[i])
            return v if out is None else be.axpby(1.0, v, 0.0, out)

        _, gl = _eig_lm(be, tl, L0, tol, self.krylovdim, self.maxiter, self.ws)
        _, gr = _eig_lm(be, tr, R0, tol, self.krylovdim, self.maxiter, self.ws)
        GL, GR = [None] * n, [None] * n
        GL[0], GR[n - 1] = gl, gr
        for i in range(1, n):
            GL[i] = be.transfer_left(self.O(i - 1), GL[i - 1], top.AL[i - 1], psi.AL[i - 1])
        for i in range(n - 2, -1, -1):
            GR[i] = be.transfer_right(self.O(i + 1), GR[i + 1], top.AR[i + 1], psi.AR[i + 1])
        if self.above is not None:
            # dot(CR_below, c_proj) = +-1 for every column (permpoinfenv.jl:178-185): both factors by 1 / sqrt|lambda|
            for col in range(n):
                lam = be.dot(psi.CR[col], self._dC(GL[(col + 1) % n], GR[col], top.CR[col]))
                f = 1.0 / math.sqrt(abs(lam))
                be.scal(f, GL[(col + 1) % n])
                be.scal(f, GR[col])
            return GL, GR
        # fix the normalisation: dot(C, dC(GL[col + 1], GR[col]) C) = 1 for every column (the eigenvectors' signs are
        # arbitrary: a negative value flips the sign of GL[col + 1])
        for col in range(n):
            c = psi.CR[col]
            lam = be.dot(c, be.dC(GL[(col + 1) % n], GR[col], c))
            f = 1.0 / math.sqrt(abs(lam))
            be.scal(math.copysign(f, lam), GL[(col + 1) % n])
            be.scal(f, GR[col])
        return GL, GR


def environments(psi, mpo, **kw):
    """environments(psi::InfiniteMPS, opp::DenseMPO)  (permpoinfenv.jl:20-29) and environments(below, (opp, above))
    (permpoinfenv.jl:29-42), opp a DenseMPO or a real SparseMPO.  An MPSMultiline: multiline.environments."""
    from . import multiline
    if isinstance(psi, multiline.MPSMultiline):
        return multiline.environments(psi, mpo, **kw)
    if isinstance(mpo, tuple):
        opp, above = mpo
        if not isinstance(above, InfiniteMPS):
            raise TypeError(f"environments(below, (O, above)) takes an InfiniteMPS above, not {type(above).__name__}")
        return PerMPOInfEnv(psi, opp, above=above, **kw)
    return PerMPOInfEnv(psi, mpo, **kw)


def calc_galerkin(psi, envs: PerMPOInfEnv, pos=None):
    """|| (1 - AL AL^T) normalize(H_AC AC) ||, maximum over the unit cell when pos is None (toolbox.jl:26-38).  Environments
    with a state above: the operator is applied to above.AC and the result projected with the AL of `psi` (the state below)."""
    from .algorithms import _galerkin
    from . import multiline
    if isinstance(psi, multiline.MPSMultiline):
        return multiline.calc_galerkin(psi, envs)
    locs = range(len(psi)) if pos is None else [pos]
    if envs.above is not None:
        return max(_galerkin(psi.be, None, None, psi.AL[loc], g=envs.ac_proj(loc, psi)) for loc in locs)
    return max(_galerkin(psi.be, envs.ddAC(loc, psi), psi.AC[loc], psi.AL[loc]) for loc in locs)


def expectation_value(psi, mpo: DenseMPO, envs: PerMPOInfEnv | None = None):
    """Per-site leading eigenvalue lambda_i = <AC_i, H_AC_i AC_i> on environments normalised per column
    (expval.jl:156-172); an MPSMultiline gives the R x n array of expval.jl:165-173."""
    from . import multiline
    if isinstance(psi, multiline.MPSMultiline):
        return multiline.expectation_value(psi, mpo, envs)
    envs = environments(psi, mpo) if envs is None else envs
    be = psi.be
    out = np.zeros(len(psi))
    for i in range(len(psi)):
        ac = psi.AC[i]
        out[i] = be.dot(ac, envs.ddAC(i, psi)(ac)) / be.dot(ac, ac)
    return out


def leading_boundary(psi, mpo: DenseMPO, alg=None, envs=None):
    """leading_boundary(psi, opp, alg = VUMPS())  (statmech/vumps.jl:15-92): the leading boundary MPS of the column
    transfer operator; returns (psi, envs, eps) with eps the Galerkin error.  alg = VOMPS(): the power method
    (statmech/vomps.jl:27-87), ONE application of H_AC / H_C per site in place of the eigensolves.  An MPSMultiline with an
    MPOMultiline: multiline.leading_boundary."""
    from .algorithms import VOMPS, VUMPS, updatetol, regauge, _log
    from . import multiline, native_cplx
    if isinstance(psi, native_cplx.NativeInfiniteMPS):
        raise NotImplementedError("leading_boundary is not implemented for NativeInfiniteMPS (interleaved complex storage)")
    if isinstance(psi, multiline.MPSMultiline):
        return multiline.leading_boundary(psi, mpo, alg, envs)
    alg = VUMPS() if alg is None else alg
    if not isinstance(alg, (VUMPS, VOMPS)):
        raise TypeError(f"leading_boundary takes VUMPS or VOMPS, not {type(alg).__name__}")
    power = isinstance(alg, VOMPS)
    name = "VOMPS" if power else "VUMPS"
    be = psi.be
    envs = environments(psi, mpo) if envs is None else envs
    eps = calc_galerkin(psi, envs)
    n = len(psi)
    ws = krylov.KrylovWorkspace(be)
    t0 = time.time()
    history = []
    for it in range(1, alg.maxiter + 1):
        newAL = []
        if power:
            for loc in range(n):
                newAL.append(regauge(be, envs.ddAC(loc, psi)(psi.AC[loc]), envs.ddC(loc, psi)(psi.CR[loc])))
        else:
            etol = updatetol(alg.eig_tol_min, alg.eig_tol_max, alg.eig_tol_factor, it, eps)
            for loc in range(n):
                _, AC = _eig_lm(be, envs.ddAC(loc, psi), psi.AC[loc], etol, alg.krylovdim, 100, ws)
                _, C = _eig_lm(be, envs.ddC(loc, psi), psi.CR[loc], etol, alg.krylovdim, 100, ws)
                newAL.append(regauge(be, AC, C))
        gtol = updatetol(alg.gauge_tol_min, alg.gauge_tol_max, alg.gauge_tol_factor, it, eps)
        psi = InfiniteMPS.from_AL(newAL, psi.CR[n - 1], tol=gtol, be=be)
        envs.recalculate(psi, updatetol(alg.env_tol_min, alg.env_tol_max, alg.env_tol_factor, it, eps))
        if alg.finalize is not None:
            psi, envs = alg.finalize(it, psi, mpo, envs)
        eps = calc_galerkin(psi, envs)
        if alg.verbosity >= 3 or eps <= alg.tol or it == alg.maxiter:
            lam = float(np.prod(expectation_value(psi, mpo, envs)))
            history.append((it, lam, eps))
            _log(alg, name, it, lam, eps, t0)
        if eps <= alg.tol:
            break
    envs.history = history
    return psi, envs, eps


def dot(a, b, c=None, krylovdim=30, tol=1e-12, rng=None):
    """dot(psi1, psi2) of two FiniteMPS / NativeFiniteMPS: linalg.dot.
    dot(psi1, psi2)  (infinitemps.jl:258-264): the leading (:LM) eigenvalue of the unit-cell transfer matrix
    TransferMatrix(psi2.AL, psi1.AL); dot(a, mpo, b)  (densempo.jl:89-97): that of TransferMatrix(b.AL, mpo, a.AL).  Real
    states; the start vector is random (rng, default seed 0)."""
    from . import window
    if isinstance(a, window.WindowMPS) and c is None:                       # windowmps.jl:165-176
        return window.dot(a, b)
    from . import linalg, native_cplx
    if c is None and any(isinstance(a, t) and isinstance(b, t) for t in (linalg.FiniteMPS, linalg.NativeFiniteMPS)):
        return linalg.dot(a, b)                                             # finitemps.jl:459-464
    if c is None and isinstance(a, native_cplx.NativeInfiniteMPS) and isinstance(b, native_cplx.NativeInfiniteMPS):
        return native_cplx.dot(a, b, krylovdim=krylovdim, tol=tol, rng=rng)
    mpo, ket = (None, b) if c is None else (b, c)
    bra = a
    if not isinstance(bra, InfiniteMPS) or not isinstance(ket, InfiniteMPS):
        raise TypeError("dot takes (InfiniteMPS, InfiniteMPS) or (InfiniteMPS, DenseMPO, InfiniteMPS)")
    if mpo is not None and not isinstance(mpo, DenseMPO):
        raise TypeError(f"dot(a, mpo, b) takes a DenseMPO, not {type(mpo).__name__}")
    _no_cplx_inf("dot", bra, ket)
    if len(bra) != len(ket) or (mpo is not None and len(bra) % len(mpo) != 0):
        raise ValueError("dot: the unit cells do not match")
    be, n = bra.be, len(bra)
    sl = None if mpo is None else mpo.slices(be)
    W = 1 if sl is None else sl[0].Wl
    Db, Dk = bra.AL[0].shape[0], ket.AL[0].shape[0]
    rng = np.random.default_rng(0) if rng is None else rng
    v0 = be.upload(rng.standard_normal(W * Db * Dk)).reshape(W, Db, Dk)

    def tl(v, out=None):
        for i in range(n):
            v = be.transfer_left(None if sl is None else sl[i % len(sl)], v, ket.AL[i], bra.AL[i])
        return v if out is None else be.axpby(1.0, v, 0.0, out)

    val, _ = _eig_lm(be, tl, v0, tol, krylovdim, 100)
    return val


# ---- models (test/setup.jl:78-130) --------------------------------------------------------------------------------

def _ising_bond_tensor(beta):
    """Square root of the bond Boltzmann matrix [[e^b, e^-b], [e^-b, e^b]] (ising_bond_tensor, test/setup.jl:78-83)."""
    ev, vec = np.linalg.eigh(np.array([[math.exp(beta), math.exp(-beta)], [math.exp(-beta), math.exp(beta)]]))
    return vec @ np.diag(np.sqrt(ev)) @ vec.T


def classical_ising(beta=math.log(1.0 + math.sqrt(2.0)) / 2.0, cluster=1):
    """Transfer tensor of the square-lattice Ising model: one spin per tensor, the square root of the bond Boltzmann
    matrix on each leg (test/setup.jl:85-94).  cluster = k contracts a k x k patch into one tensor with chi = d = 2^k
    (legs fused row by row / column by column); its leading eigenvalue per tensor is kappa^(k^2)."""
    nt = _ising_bond_tensor(beta)
    o = np.einsum("ia,ib,ic,id->abcd", nt, nt, nt, nt)         # delta tensor with a bond root on each leg [w,t,s,v]
    k = int(cluster)
    if k < 1:
        raise ValueError("cluster must be >= 1")
    row = o
    for _ in range(k - 1):                                       # k tensors side by side: v of one = w of the next
        row = np.einsum("atsv,vxyb->atxsyb", row, o)
        row = row.reshape(2, row.shape[1] * 2, row.shape[3] * 2, 2)
    out = row
    for _ in range(k - 1):                                       # stack rows: t (out) of the lower = s (in) of the upper
        out = np.einsum("atsv,bxtc->abxsvc", out, row)
        W, X, S, V = out.shape[0] * 2, out.shape[2], out.shape[3], out.shape[4] * 2
        out = out.reshape(W, X, S, V)
    return DenseMPO(np.ascontiguousarray(out))


def sixvertex(a=1.0, b=1.0, c=1.0):
    """Six-vertex transfer tensor (test/setup.jl:124-130): the 4 x 4 weight matrix on (w t) x (v s)."""
    m = np.array([[a, 0, 0, 0], [0, c, b, 0], [0, b, c, 0], [0, 0, 0, a]], dtype=np.float64)
    t = m.reshape(2, 2, 2, 2, order="F")                          # t[i1, i2, i3, i4] = m[i1 + 2 i2, i3 + 2 i4]
    return DenseMPO(np.ascontiguousarray(np.transpose(t, (0, 1, 3, 2))))   # permute ((1, 2), (4, 3))
