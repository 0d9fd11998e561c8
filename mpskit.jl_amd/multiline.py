"""Multi-row uniform states and operators: MPSMultiline (src/states/mpsmultiline.jl), MPOMultiline
(src/operators/mpomultiline.jl), their PerMPOInfEnv (src/environments/permpoinfenv.jl:23-42, :138-189) and the multi-row forms
of leading_boundary (statmech/vumps.jl:20-84, statmech/vomps.jl:27-87), approximate (approximate/vomps.jl:19-80), calc_galerkin
(toolbox.jl:26-38) and expectation_value (expval.jl:165-173).

Row r of the operator sits between state row r (ket, above) and state row r + 1 (bra, below), periodic in r, so every
environment is a mixed one: lw[r][c] has slabs [D of row r + 1, D of row r].  They are computed row by row by the one-row
PerMPOInfEnv with above = row r and below = row r + 1 (the same transfers and the same per-column normalisation).

A column update acts on the STACKED vector of all rows' AC (or CR): one contiguous device vector of R tensors, so that the
Krylov kernels run on it unchanged.  The map is out[r + shift] = H_AC[r] x[r] (derivatives.jl:163-166, :195-197: shift = 1 is the
reference's circshift, shift = 0 the plain batch of calc_galerkin).  One application is a loop of dAC_proj / dC_proj over the
rows, each result copied into its slot; rows of different bond dimensions are allowed.  A launch chain that batches the rows
of a column is not implemented.  Real fp64 only; GradientGrassmann, changebonds and the IDMRG forms of approximate are not
implemented for more than one row (excitations: quasiparticle.excitations_statmech)."""
from __future__ import annotations

import time

import numpy as np

from . import krylov
from .backend import DTensor
from .states import InfiniteMPS
from .statmech import DenseMPO, PerMPOInfEnv, _eig_lm, _no_cplx_inf, dC_proj_composed


class _Grid:
    """Periodic [row, column] view of one tensor family (AL / AR / AC / CR) of an MPSMultiline; [row] is that row's list."""

    def __init__(self, rows, name):
        self._rows, self._name = rows, name

    def __getitem__(self, key):
        if isinstance(key, tuple):
            r, c = key
            lst = getattr(self._rows[r % len(self._rows)], self._name)
            return lst[c % len(lst)]
        return getattr(self._rows[key % len(self._rows)], self._name)


class MPSMultiline:
    """R InfiniteMPS with the same unit-cell length, physical dimensions and backend (mpsmultiline.jl): psi[r] is a row,
    psi.AL[r, c] / .AR / .AC / .CR index rows and columns periodically, len(psi) is the number of columns."""

    def __init__(self, rows):
        if isinstance(rows, InfiniteMPS):
            rows = [rows]
        rows = list(rows)
        if not rows:
            raise ValueError("MPSMultiline needs at least one row")
        for r, st in enumerate(rows):
            if not isinstance(st, InfiniteMPS):
                raise TypeError(f"MPSMultiline row {r} is a {type(st).__name__}, not an InfiniteMPS")
            if getattr(st, "cplx", False):
                raise NotImplementedError(f"MPSMultiline row {r}: complex states are not supported on uniform states "
                                          "(real fp64 only)")
            if len(st) != len(rows[0]):
                raise ValueError(f"MPSMultiline row {r} has a unit cell of {len(st)} sites, row 0 one of {len(rows[0])}")
            if st.be is not rows[0].be:
                raise ValueError(f"MPSMultiline row {r} lives on another backend than row 0")
            for c in range(len(st)):
                if st.AL[c].shape[1] != rows[0].AL[c].shape[1]:
                    raise ValueError(f"MPSMultiline row {r}, column {c}: physical dimension {st.AL[c].shape[1]}, "
                                     f"row 0 has {rows[0].AL[c].shape[1]}")
        self.rows, self.be, self.cplx = rows, rows[0].be, False
        self.AL, self.AR = _Grid(rows, "AL"), _Grid(rows, "AR")
        self.AC, self.CR = _Grid(rows, "AC"), _Grid(rows, "CR")

    def __len__(self):
        return len(self.rows[0])

    def __getitem__(self, r):
        return self.rows[r % len(self.rows)]

    def __iter__(self):
        return iter(self.rows)

    @property
    def shape(self):
        return (len(self.rows), len(self.rows[0]))

    @classmethod
    def from_AL(cls, ALs, CRs_last, tol=1e-14, maxiter=100, be=None):
        """MPSMultiline(ALs, CR[:, end]; tol, maxiter)  (statmech/vumps.jl:62): ALs[r][c], one start bond matrix per row; every
        row is gauged by InfiniteMPS.from_AL."""
        if len(ALs) != len(CRs_last):
            raise ValueError(f"{len(ALs)} rows of tensors but {len(CRs_last)} bond matrices")
        return cls([InfiniteMPS.from_AL(list(al), c, tol=tol, maxiter=maxiter, be=be) for al, c in zip(ALs, CRs_last)])

    def to_infinitemps(self):
        """convert(InfiniteMPS, psi) of a one-row state."""
        if len(self.rows) != 1:
            raise ValueError(f"only a one-row MPSMultiline converts to an InfiniteMPS, this one has {len(self.rows)} rows")
        return self.rows[0]


class MPOMultiline:
    """R DenseMPO with the same unit cell (mpomultiline.jl); MPOMultiline(dense_mpo) is the one-row form.  mpo[r] is a row,
    mpo[r, c] a tensor, both periodic."""

    def __init__(self, rows):
        if isinstance(rows, DenseMPO):
            rows = [rows]
        rows = list(rows)
        if not rows:
            raise ValueError("MPOMultiline needs at least one row")
        for r, o in enumerate(rows):
            if not isinstance(o, DenseMPO):
                raise TypeError(f"MPOMultiline row {r} is a {type(o).__name__}, not a DenseMPO")
            if len(o) != len(rows[0]):
                raise ValueError(f"MPOMultiline row {r} has a unit cell of {len(o)} tensors, row 0 one of {len(rows[0])}")
        for r, o in enumerate(rows):                  # the physical legs of neighbouring rows meet
            nxt = rows[(r + 1) % len(rows)]
            for c in range(len(o)):
                if o[c].shape[1] != nxt[c].shape[2]:
                    raise ValueError(f"MPOMultiline row {r}, column {c}: output dimension {o[c].shape[1]} does not match the "
                                     f"input dimension {nxt[c].shape[2]} of the row below")
        self.rows = rows

    def __len__(self):
        return len(self.rows[0])

    def __getitem__(self, key):
        if isinstance(key, tuple):
            return self.rows[key[0] % len(self.rows)][key[1]]
        return self.rows[key % len(self.rows)]

    def __iter__(self):
        return iter(self.rows)

    @property
    def shape(self):
        return (len(self.rows), len(self.rows[0]))

    def to_densempo(self):
        if len(self.rows) != 1:
            raise ValueError(f"only a one-row MPOMultiline converts to a DenseMPO, this one has {len(self.rows)} rows")
        return self.rows[0]


# ---- the stacked column operator ------------------------------------------------------------------------------------------

class RowsOp:
    """x -> out with out[(r + shift) % R] = H[r] x[r] on stacked vectors: H[r] the AC map (kind "AC": slices Hs, GL = lw[r][col],
    GR = rw[r][col]) or the C map (kind "C": GL = lw[r][col + 1], GR = rw[r][col]) of row r.  x is one DTensor holding the R
    input tensors back to back (row r: [Dl_r, d, Dr_r]), the result one DTensor holding the R results slot by slot."""

    def __init__(self, be, kind, Hs, GLs, GRs, shift):
        self.be, self.kind, self.Hs, self.GLs, self.GRs = be, kind, Hs, GLs, GRs
        self.R = R = len(GLs)
        self.shift = shift % R
        mid = (Hs[0].d,) if kind == "AC" else ()
        self.in_shapes = [(gl.shape[2],) + mid + (gr.shape[1],) for gl, gr in zip(GLs, GRs)]
        outs = [(gl.shape[1],) + mid + (gr.shape[2],) for gl, gr in zip(GLs, GRs)]
        self.out_shapes = [outs[(s - self.shift) % R] for s in range(R)]          # by slot
        self.in_off = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in self.in_shapes])])
        self.out_off = np.concatenate([[0], np.cumsum([int(np.prod(s)) for s in self.out_shapes])])

    @property
    def n_in(self):
        return int(self.in_off[-1])

    @property
    def n_out(self):
        return int(self.out_off[-1])

    def stack_in(self, tensors):
        assert [t.shape for t in tensors] == self.in_shapes, ([t.shape for t in tensors], self.in_shapes)
        return stack_tensors(self.be, tensors)

    def split_out(self, vec, copy=True):
        """the R result tensors of a stacked result, by slot (fresh buffers by default: a slot may start at an odd offset)"""
        return _split(self.be, vec, self.out_off, self.out_shapes, copy)

    def __call__(self, x: DTensor, out: DTensor = None):
        be, R = self.be, self.R
        assert x.size == self.n_in, (x.shape, self.n_in)
        out = be.empty(self.n_out) if out is None else out
        assert out.size == self.n_out, (out.shape, self.n_out)
        xs = _split(be, x, self.in_off, self.in_shapes, False)
        for r in range(R):
            y = self._one(r, xs[r])
            s = (r + self.shift) % R
            out.buf[int(self.out_off[s]):int(self.out_off[s + 1])].copy_(y.buf[:y.size])
        return out

    __mul__ = __call__

    def _one(self, r, x):
        be, GL, GR = self.be, self.GLs[r], self.GRs[r]
        if self.kind == "AC":
            if hasattr(be, "dAC_proj"):
                return be.dAC_proj(self.Hs[r], GL, GR, x)
            return be.dAC(self.Hs[r], GL, GR, x, out=be.empty(GL.shape[1], x.shape[1], GR.shape[2]))
        if hasattr(be, "dC_proj"):
            return be.dC_proj(GL, GR, x)
        return dC_proj_composed(be, GL, GR, x)


def stack_tensors(be, tensors):
    """one contiguous device vector holding the tensors back to back"""
    out = be.empty(sum(t.size for t in tensors))
    off = 0
    for t in tensors:
        out.buf[off:off + t.size].copy_(t.buf[:t.size])
        off += t.size
    return out


def _split(be, vec, offs, shapes, copy):
    parts = []
    for i, shp in enumerate(shapes):
        v = DTensor(vec.buf[int(offs[i]):int(offs[i + 1])], shp)
        parts.append(be.copy(v) if copy else v)
    return parts


# ---- environments ---------------------------------------------------------------------------------------------------------

class MultilineEnv(PerMPOInfEnv):
    """PerMPOInfEnv of (MPSMultiline, MPOMultiline), optionally with a fixed MPSMultiline `above` (permpoinfenv.jl:23-42).
    lw[r][c] / rw[r][c]: mixed_fixpoints (permpoinfenv.jl:138-189) row by row -- the transfer of above[r] against below[r + 1]
    through mpo[r], normalised per column to |dot(CR_below, c_proj)| = 1 (lines 178-185).  mpo may be the pair
    (MPOMultiline, above), as environments(below, (mpo, above)) takes it."""

    def __init__(self, psi, mpo, tol=1e-12, krylovdim=30, maxiter=100, rng=None, above=None):
        if isinstance(mpo, tuple):
            if above is not None or len(mpo) != 2:
                raise TypeError("environments of an MPSMultiline take (mpo, above) or mpo with above=, not both")
            mpo, above = mpo
        if not isinstance(mpo, MPOMultiline):
            raise TypeError(f"environments of an MPSMultiline take an MPOMultiline, not {type(mpo).__name__}")
        if above is not None and not isinstance(above, MPSMultiline):
            raise TypeError(f"environments(below, (O, above)) of an MPSMultiline take an MPSMultiline above, "
                            f"not {type(above).__name__}")
        _no_cplx_inf("environments", psi, above)
        R, n = psi.shape
        if mpo.shape[0] != R:
            raise ValueError(f"the state has {R} rows, the operator {mpo.shape[0]}")
        if above is not None and above.shape != psi.shape:
            raise ValueError(f"the state above is {above.shape[0]} x {above.shape[1]} (rows x columns), "
                             f"the state below {R} x {n}")
        if n % len(mpo) != 0:
            raise ValueError(f"unit cell of the state ({n}) is not a multiple of the MPO's ({len(mpo)})")
        self.be, self.opp, self.above = psi.be, mpo, above
        self.tol, self.krylovdim, self.maxiter = tol, krylovdim, maxiter
        self.rng = np.random.default_rng(0) if rng is None else rng
        top = psi if above is None else above
        self.sub = [PerMPOInfEnv(psi[r + 1], mpo[r], tol=tol, krylovdim=krylovdim, maxiter=maxiter, rng=self.rng, above=top[r])
                    for r in range(R)]
        self.ws = self.sub[0].ws
        self.dependency = psi
        self._fix_signs(psi)

    @property
    def lw(self):
        return [s.lw for s in self.sub]

    @property
    def rw(self):
        return [s.rw for s in self.sub]

    def O(self, r, c):
        return self.sub[r % len(self.sub)].O(c)

    def recalculate(self, psi, tol=None):
        tol = self.tol if tol is None else tol
        if psi.shape[0] != len(self.sub):
            raise ValueError(f"the state has {psi.shape[0]} rows, the environments {len(self.sub)}")
        top = psi if self.above is None else self.above
        n = len(psi)
        for r, s in enumerate(self.sub):
            a = top[r]
            if s.lw[0].shape[2] != a.AL[0].shape[0] or s.rw[n - 1].shape[1] != a.AR[n - 1].shape[2]:
                s.dependency = None              # the bond spaces of the row above changed: random start vectors
            s.above = a
            s.recalculate(psi[r + 1], tol)
        self.dependency, self.tol = psi, tol
        self._fix_signs(psi)
        return self

    def _fix_signs(self, psi):
        """The eigenvectors' signs are arbitrary and lines 178-185 only fix |dot(CR_below, c_proj)| = 1: a negative value flips
        the sign of lw[r][col + 1] (as the one-row environments do), so that every entry of expectation_value is the positive
        eigenvalue whatever signs the gauge gave the bond matrices of the rows.  One c_proj and one host-read dot per (row,
        column) and recalculate; their cost has not been timed."""
        be, n, top = self.be, len(psi), self._top(psi)
        for r, s in enumerate(self.sub):
            for col in range(n):
                gl = s.lw[(col + 1) % n]
                if be.dot(psi.CR[r + 1, col], s._dC(gl, s.rw[col], top.CR[r, col])) < 0:
                    be.scal(-1.0, gl)

    def _fresh(self, psi):
        if self.dependency is not psi:
            self.recalculate(psi)

    def leftenv(self, r, c, psi):
        self._fresh(psi)
        return self.sub[r % len(self.sub)].lw[c % len(psi)]

    def rightenv(self, r, c, psi):
        self._fresh(psi)
        return self.sub[r % len(self.sub)].rw[c % len(psi)]

    def _top(self, below):
        return below if self.above is None else self.above

    def ac_proj(self, r, c, below):
        """ac_proj(row, col, below, envs)  (derivatives.jl:216-219)"""
        op = RowsOp(self.be, "AC", [self.O(r, c)], [self.leftenv(r, c, below)], [self.rightenv(r, c, below)], 0)
        return op._one(0, self._top(below).AC[r, c])

    def c_proj(self, r, c, below):
        """c_proj(row, col, below, envs)  (derivatives.jl:204-207)"""
        op = RowsOp(self.be, "C", None, [self.leftenv(r, c + 1, below)], [self.rightenv(r, c, below)], 0)
        return op._one(0, self._top(below).CR[r, c])

    def _column_op(self, kind, col, psi, shift):
        self._fresh(psi)
        be, R, n = self.be, len(self.sub), len(psi)
        GLs = [self.sub[r].lw[(col if kind == "AC" else col + 1) % n] for r in range(R)]
        GRs = [self.sub[r].rw[col % n] for r in range(R)]
        Hs = [self.O(r, col) for r in range(R)] if kind == "AC" else None
        return RowsOp(be, kind, Hs, GLs, GRs, shift)

    def ddAC(self, col, psi, shift=1):
        """the AC map of column `col` on the stacked vector of all rows (the RecursiveVec form of derivatives.jl)"""
        return self._column_op("AC", col, psi, shift)

    def ddC(self, col, psi, shift=1):
        return self._column_op("C", col, psi, shift)


def environments(psi, mpo, **kw):
    """environments(psi::MPSMultiline, mpo::MPOMultiline) and environments(below, (mpo, above))  (permpoinfenv.jl:23-42)"""
    return MultilineEnv(psi, mpo, **kw)


# ---- measurements ---------------------------------------------------------------------------------------------------------

def _column_images(psi, envs, col, shift):
    """[H_AC[r] above.AC[r, col]] by slot, as fresh tensors"""
    op = envs.ddAC(col, psi, shift=shift)
    top = envs._top(psi)
    return op.split_out(op(op.stack_in([top.AC[r, col] for r in range(psi.shape[0])])))


def calc_galerkin(psi, envs):
    """toolbox.jl:26-38: || (1 - AL AL^T) normalize(H_AC[r] above.AC[r, c]) || with the AL of row r + 1, maximum over rows
    and columns."""
    from .algorithms import _galerkin
    R, n = psi.shape
    out = 0.0
    for col in range(n):
        g = _column_images(psi, envs, col, 0)
        for r in range(R):
            out = max(out, _galerkin(psi.be, None, None, psi.AL[r + 1, col], g=g[r]))
    return out


def expectation_value(psi, mpo=None, envs=None):
    """expval.jl:165-173: the R x n array <AC[r + 1, c], H_AC[r] AC[r, c]>, one leading eigenvalue per tensor of the network."""
    envs = environments(psi, mpo) if envs is None else envs
    be = psi.be
    R, n = psi.shape
    out = np.zeros((R, n))
    for col in range(n):
        op = envs.ddAC(col, psi, shift=0)
        g = op.split_out(op(op.stack_in([psi.AC[r, col] for r in range(R)])))
        for r in range(R):
            out[r, col] = be.dot(psi.AC[r + 1, col], g[r]) / (be.norm(psi.AC[r + 1, col]) * be.norm(psi.AC[r, col]))
    return out


# ---- algorithms -----------------------------------------------------------------------------------------------------------

def _eig_cyclic(be, op, x0, tol, krylovdim, ws):
    """The fixed point of the cyclic map out[r + 1] = H[r] x[r].  Its spectrum is the R-th roots of that of the product of the
    rows: R eigenvalues mu w^k share the leading modulus, and only the one on the positive real axis has the real eigenvector
    (x[r + 1] = H[r] x[r] / mu) the rows are read from.  The shift by sigma ~ |op| makes that one the single :LM eigenvalue of
    op + sigma, with the same eigenvectors; one row needs none.  This assumes that the leading eigenvalue of the product of
    the rows is real and positive at every iteration, not only at convergence (true for the positive Boltzmann weights of a
    classical partition function; a product with a negative or complex leading eigenvalue would need another selection).
    The tolerance is relative to the scale of the shifted operator, as in _eig_lm; the one application that measures sigma
    serves for that scale too."""
    if op.R == 1:
        return _eig_lm(be, op, x0, tol, krylovdim, 100, ws)
    y, n0 = op(x0), be.norm(x0)
    sigma = be.norm(y) / n0
    scale = be.norm(be.axpby(sigma, x0, 1.0, y)) / n0

    def shifted(x, out=None):
        return be.axpby(sigma, x, 1.0, op(x, out))

    val, vec = krylov.eigsolve_lm_real(be, shifted, x0, tol=tol * max(scale, 1e-300), krylovdim=krylovdim, maxiter=100, ws=ws)
    return val - sigma, vec


def _update_column(psi, envs, col, solve):
    """new (AC, C) of every row of one column -> the regauged AL of that column, by row"""
    from .algorithms import regauge
    be, R = psi.be, psi.shape[0]
    top = envs._top(psi)
    hac, hc = envs.ddAC(col, psi), envs.ddC(col, psi)
    ac = solve(hac, hac.stack_in([top.AC[r, col] for r in range(R)]))
    c = solve(hc, hc.stack_in([top.CR[r, col] for r in range(R)]))
    return [regauge(be, a, b) for a, b in zip(hac.split_out(ac), hc.split_out(c))]


def _iterate(psi, target, alg, envs, name, solve_for):
    from .algorithms import updatetol, _log
    be = psi.be
    R, n = psi.shape
    eps = calc_galerkin(psi, envs)
    t0, history = time.time(), []
    for it in range(1, alg.maxiter + 1):
        solve = solve_for(it, eps)
        cols = [_update_column(psi, envs, col, solve) for col in range(n)]
        gtol = updatetol(alg.gauge_tol_min, alg.gauge_tol_max, alg.gauge_tol_factor, it, eps)
        psi = MPSMultiline.from_AL([[cols[c][r] for c in range(n)] for r in range(R)], [psi.CR[r, n - 1] for r in range(R)],
                                   tol=gtol, be=be)
        envs.recalculate(psi, updatetol(alg.env_tol_min, alg.env_tol_max, alg.env_tol_factor, it, eps))
        if alg.finalize is not None:
            psi, envs = alg.finalize(it, psi, target, envs)
        eps = calc_galerkin(psi, envs)
        if alg.verbosity >= 3 or eps <= alg.tol or it == alg.maxiter:
            lam = float(np.prod(expectation_value(psi, envs=envs))) if envs.above is None else float("nan")
            history.append((it, lam, eps))
            _log(alg, name, it, lam, eps, t0)
        if eps <= alg.tol:
            break
    envs.history = history
    return psi, envs, eps


def leading_boundary(psi, mpo, alg=None, envs=None):
    """leading_boundary(psi::MPSMultiline, O::MPOMultiline, alg)  (statmech/vumps.jl:20-84, statmech/vomps.jl:27-87): per
    column the :LM fixed point (VUMPS) or one application (VOMPS) of the cyclic map on the stacked AC and C of all rows, a
    regauge per (row, column), MPSMultiline.from_AL and recalculate.  Returns (psi, envs, eps)."""
    from .algorithms import VOMPS, VUMPS, updatetol
    alg = VUMPS() if alg is None else alg
    if not isinstance(alg, (VUMPS, VOMPS)):
        raise TypeError(f"leading_boundary takes VUMPS or VOMPS, not {type(alg).__name__}")
    if not isinstance(mpo, MPOMultiline):
        raise TypeError(f"leading_boundary of an MPSMultiline takes an MPOMultiline, not {type(mpo).__name__}")
    envs = environments(psi, mpo) if envs is None else envs
    be = psi.be
    if isinstance(alg, VOMPS):
        return _iterate(psi, mpo, alg, envs, "VOMPS", lambda it, eps: (lambda op, x: op(x)))
    ws = krylov.KrylovWorkspace(be)

    def solve_for(it, eps):
        etol = updatetol(alg.eig_tol_min, alg.eig_tol_max, alg.eig_tol_factor, it, eps)
        return lambda op, x: _eig_cyclic(be, op, x, etol, alg.krylovdim, ws)[1]

    return _iterate(psi, mpo, alg, envs, "VUMPS", solve_for)


def approximate(psi, toapprox, alg, envs=None):
    """approximate(psi::MPSMultiline, (O::MPOMultiline, above::MPSMultiline), alg::VOMPS)  (approximate/vomps.jl:19-80): the
    same loop with the state above fixed -- one ac_proj and one c_proj per (row, column), no eigensolve.  A VUMPS is converted
    as the reference's deprecation does."""
    from .algorithms import VOMPS, VUMPS
    if isinstance(alg, VUMPS):
        alg = VOMPS(tol=alg.tol, maxiter=alg.maxiter, finalize=alg.finalize, verbosity=alg.verbosity,
                    gauge_tol_min=alg.gauge_tol_min, gauge_tol_max=alg.gauge_tol_max, gauge_tol_factor=alg.gauge_tol_factor,
                    env_tol_min=alg.env_tol_min, env_tol_max=alg.env_tol_max, env_tol_factor=alg.env_tol_factor)
    if not isinstance(alg, VOMPS):
        raise TypeError(f"approximate on an MPSMultiline takes VOMPS (or VUMPS), not {type(alg).__name__}")
    if not (isinstance(toapprox, tuple) and len(toapprox) == 2 and isinstance(toapprox[0], MPOMultiline)
            and isinstance(toapprox[1], MPSMultiline)):
        raise TypeError("approximate on an MPSMultiline takes (O, above): an MPOMultiline and an MPSMultiline")
    envs = environments(psi, toapprox) if envs is None else envs
    return _iterate(psi, toapprox, alg, envs, "VOMPS", lambda it, eps: (lambda op, x: op(x)))
