"""Host-side Krylov solvers on DEVICE vectors (the KrylovKit role in the reference:
src/algorithms/fixedpoint.jl:9-30, mpohaminfenv.jl:95).  The loop stays on the host, every
matvec is one call into libmpsk, and the Gram-Schmidt step is the fused multi-dot / multi-axpy
pair fused with the normalisation in `mpsk_vorth_step` (coefficients stay on the device, ONE host sync
per Krylov iteration).
"""
from __future__ import annotations

import numpy as np

from .backend import Backend, DTensor


class KrylovWorkspace:
    """Reusable pool of device vectors so that an eigsolve allocates nothing after warm-up."""

    def __init__(self, be: Backend):
        self.be = be
        self.pool = {}

    def get(self, shape, n, tag=None):
        """n device buffers of `shape`.  Buffers are pooled by (tag, shape): two users with different tags never share
        a buffer even when their shapes coincide (the sweep's galerkin slot (2L-2, 1) and the fixed-budget solver's scalar
        slot (m (2m+1) + 40, 1) have the same shape at L = 39 for m = 4, at L = 89 for m = 8)."""
        shp = tuple(shape)
        lst = self.pool.setdefault((tag, shp), [])
        while len(lst) < n:
            lst.append(self.be.empty(*shp))
        return lst[:n]


def eigsolve_sr(be: Backend, matvec, x0: DTensor, tol=1e-12, krylovdim=30, maxiter=100,
                fixed_matvecs=None, ws: KrylovWorkspace | None = None, first_image: DTensor | None = None,
                values: bool = True):
    """Smallest-real eigenpair of a Hermitian operator: restarted Lanczos/Arnoldi with twice-iterated
    classical Gram-Schmidt and an 'eager' convergence test each step (defaults.jl:33:
    Arnoldi(; tol, maxiter, eager=true)).  matvec(x: DTensor, out: DTensor) -> out.
    first_image: optional buffer that receives A (x0 / |x0|), the very first matvec of the solve, before it is
    orthogonalised -- calc_galerkin of the OLD tensor needs exactly this vector (toolbox.jl:18), so the DMRG sweep
    does not apply the effective Hamiltonian to the same tensor twice.
    values=False (fixed-budget solves only): the caller needs the vector alone -- the Ritz step then runs on the device
    as well (mpsk_vritz_dev) and the solve returns (None, vec, n_matvecs, None) without ever stalling the stream.
    Returns (lambda, vec, n_matvecs, residual)."""
    ws = KrylovWorkspace(be) if ws is None else ws
    shape = x0.shape
    vecs = ws.get(shape, krylovdim + 2)
    V, ritz = vecs[:krylovdim + 1], vecs[krylovdim + 1]
    nmv, lam, res = 0, 0.0, np.inf
    start = x0
    if fixed_matvecs is not None and fixed_matvecs <= krylovdim and hasattr(be, "orth_step_dev"):
        # fixed budget within one Krylov cycle: nothing is decided per step, so the whole recurrence is enqueued
        # without host synchronisation and the projected matrix is read back once (the per-step sync left the GPU
        # idle ~10 % of a site update at D = 1024)
        # a Krylov space cannot be larger than the vector space: beyond x0.size steps the (rounding-level) residual
        # would be renormalised into a noise direction and pollute the projected matrix (chain-edge sites of a
        # benchmark sweep have dimension 4 < 8)
        m = max(1, min(fixed_matvecs, x0.size))
        stride = 2 * m + 1
        steps = m            # applications made, reported as n_matvecs (the host Ritz route shrinks m at its cut)
        if not values and m <= 32 and hasattr(matvec, "eigsolve_fixed"):
            # the whole solve as ONE library call (mpsk_hac_eigsolve_fixed): same kernels in the same order as below,
            # without the ~30 entry-point calls per site the host otherwise makes (they starve the stream at small D)
            out = be.empty(*shape)
            scal = ws.get((m * stride + 40, 1), 1, tag="eigscal")[0]
            if matvec.eigsolve_fixed(start, m, V[:m + 1] + [ritz], scal, out, first_image) is not None:
                return None, out, steps, None
        slot = ws.get((m * stride,), 1, tag="eigslot")[0]
        be.normalize_dev(start, out=V[0])              # no host round trip: the solve has ONE synchronisation, below
        for k in range(m):
            w = V[k + 1]
            matvec(V[k], w)
            if k == 0 and first_image is not None:
                be.axpby(1.0, w, 0.0, first_image)
            be.orth_step_dev(V[:k + 1], w, slot, k * stride)
        if not values and m <= 32 and hasattr(be, "ritz_dev"):
            rb = ws.get((be.RITZ_BUF, 1), 1, tag="ritz")[0]
            be.ritz_dev(m, stride, slot, rb)
            be.lincomb_dev(V[:m], rb, out=ritz)
            out = be.empty(*shape)
            be.normalize_dev(ritz, out=out)
            return None, out, steps, None
        co = be.download(slot)
        Hm = np.zeros((m + 1, m))
        for k in range(m):
            kk = k + 1
            blk = co[k * stride:k * stride + 2 * kk + 1]
            Hm[:kk, k] = blk[:kk] + blk[kk:2 * kk]
            Hm[kk, k] = np.sqrt(max(blk[2 * kk], 0.0))
        # invariant subspace reached before the budget ran out (beta_k at rounding level): the later columns were
        # built from a renormalised rounding residual -> project on the exact part only
        scale = max(np.abs(Hm[:m, :m]).max(), 1e-300)
        for k in range(m):
            if Hm[k + 1, k] <= 1e-13 * scale:
                m = k + 1
                break
        Hk = Hm[:m, :m]
        ev, S = np.linalg.eigh((Hk + Hk.T) / 2)
        lam, sv = ev[0], S[:, 0]
        if sv[0] < 0:                                  # sign: positive component on the start vector, as mpsk_vritz_dev
            sv = -sv
        res = abs(Hm[m, m - 1] * sv[-1])
        be.lincomb(V[:m], sv, out=ritz)
        out = be.empty(*shape)
        be.normalize_dev(ritz, out=out)
        return lam, out, steps, res
    # Thick restart (Krylov-Schur for a Hermitian operator, what KrylovKit's eigsolve does with an Arnoldi / Lanczos
    # factorization; the `keep` rule below is recalled from KrylovKit's source, which is not vendored in the reference:
    # "parity unpinned", only the converged eigenpair is compared anywhere).  After krylovdim steps the basis is SHRUNK to
    # the `keep` lowest Ritz vectors plus the residual direction instead of restarting from the Ritz vector alone:
    #   A Y = Y diag(theta) + v_{m+1} b^T ,   b = beta_m S[m-1, :keep]
    # is again an Arnoldi relation, so the expansion simply continues.  On the first to-tolerance sweep of the benchmark
    # chain the single-vector restart needed 340 matvecs per site (profiles/r03_*), most of them re-learning directions
    # the restart had thrown away.
    m = int(min(krylovdim, max(x0.size, 1)))
    nrm = be.norm(start)
    be.axpby(1.0 / nrm, start, 0.0, V[0])
    basis = list(V[:m + 1])                     # basis[i] = i-th Krylov vector; the remaining pool entries are scratch
    spare = None
    Hm = np.zeros((m + 1, m))
    k, conv = 0, False
    sv = None
    # One-step-ahead expansion (device backends with orth_step_async): step k + 1 (matvec, Gram-Schmidt, normalisation -- none
    # of which needs the host) is enqueued BEFORE the host reads the scalars of step k and takes the eager convergence
    # decision, so the stream does not drain once per Krylov step.  If step k turns out to be the last one, the speculative
    # step is discarded: it only wrote basis[k + 2], which the Ritz vector of step k does not involve (at most one wasted
    # matvec per solve, counted in nmv).
    spec = hasattr(be, "orth_step_async") and fixed_matvecs is None
    agree = getattr(matvec, "agree", None)

    def account(kk, h, beta):
        """column kk of the projected matrix is known: eager convergence test of the (kk + 1)-dimensional space"""
        nonlocal lam, sv, res, S, ev
        Hm[:kk + 1, kk] = h
        Hm[kk + 1, kk] = beta
        Hk = Hm[:kk + 1, :kk + 1]
        ev, S = np.linalg.eigh((Hk + Hk.T) / 2)
        lam, sv = ev[0], S[:, 0]
        res = abs(Hm[kk + 1, :kk + 1] @ sv)               # |(last row of the (k+1) x k matrix) . s| = Ritz residual norm
        done_fixed = fixed_matvecs is not None and nmv >= fixed_matvecs
        # breakdown: the Krylov space is invariant (always the case once k reaches the vector-space dimension)
        breakdown = beta <= 1e-13 * max(np.abs(Hk).max(), 1e-300) or kk + 1 >= x0.size
        ok = (fixed_matvecs is None and res < tol) or breakdown or done_fixed
        # a bond-sharded operator (dist.ShardedSiteOp) makes the ranks AGREE on every data-dependent decision: they hold
        # bit-identical vectors by construction, the tiny all-reduce is insurance against one of them ever seeing another
        # rounding (a rank that stops while its peers enter the next all-gather would hang the job)
        return agree(ok) if (agree is not None and fixed_matvecs is None) else ok

    S = ev = None
    for _restart in range(maxiter):
        pending = None                                    # (column index, handle) whose scalars are still in flight
        while k < m:
            w = basis[k + 1]
            matvec(basis[k], w)
            if nmv == 0 and first_image is not None:
                be.axpby(1.0, w, 0.0, first_image)
            nmv += 1
            if spec:
                hnd = be.orth_step_async(basis[:k + 1], w)
                if pending is not None and account(pending[0], *pending[1].result()):
                    k, conv = pending[0] + 1, True        # converged one step earlier: drop the speculative step
                    pending = None
                    break
                pending = (k, hnd)
                k += 1
                continue
            h, beta = be.orth_step(basis[:k + 1], w)      # CGS2 + normalise, one host sync
            k += 1
            if account(k - 1, h, beta):
                conv = True
                break
        if pending is not None:
            kk = pending[0]
            if account(kk, *pending[1].result()):
                k, conv = kk + 1, True
        if conv or _restart == maxiter - 1:
            break
        # shrink: keep the lowest Ritz vectors (KrylovKit: keep = div(3 krylovdim + 2 converged, 5), converged = 0 here)
        keep = max(1, min(m - 1, (3 * m) // 5))
        if spare is None:
            spare = ws.get(shape, keep, tag="thick-restart")
        if hasattr(be, "multilincomb") and m <= 32:
            be.multilincomb(basis[:m], S[:, :keep], spare[:keep])       # one pass: m + keep vector reads / writes
        else:
            for j in range(keep):
                be.lincomb(basis[:m], S[:, j], out=spare[j])
        resid = basis[m]                                  # v_{m+1}
        coupling = Hm[m, m - 1] * S[m - 1, :keep]
        old = basis[:m]
        basis = list(spare[:keep]) + [resid] + old[:m - keep]      # m + 1 vectors again
        spare = old[m - keep:m]                                       # the other `keep` old vectors: next shrink's targets
        Hm = np.zeros((m + 1, m))
        Hm[:keep, :keep] = np.diag(ev[:keep])
        Hm[keep, :keep] = coupling
        k = keep
    be.lincomb(basis[:k], sv, out=ritz)
    out = be.empty(*shape)
    nrm = be.norm(ritz)
    if nrm == 0.0:
        raise ZeroDivisionError("eigsolve_sr: zero Ritz vector (zero start vector?)")
    be.axpby(1.0 / nrm, ritz, 0.0, out)
    return lam, out, nmv, res


def eigsolve_lm_real(be: Backend, matvec, x0: DTensor, tol=1e-12, krylovdim=30, maxiter=100,
                     ws: KrylovWorkspace | None = None):
    """Dominant (largest-magnitude) eigenpair of a real non-symmetric operator whose dominant
    eigenvector is real (transfer matrices: ortho.jl:184,241).  Restarted Arnoldi."""
    ws = KrylovWorkspace(be) if ws is None else ws
    shape = x0.shape
    vecs = ws.get(shape, krylovdim + 2)
    V, ritz = vecs[:krylovdim + 1], vecs[krylovdim + 1]
    lam = 0.0
    start = x0
    for _restart in range(maxiter):
        nrm = be.norm(start)
        be.axpby(1.0 / nrm, start, 0.0, V[0])
        Hm = np.zeros((krylovdim + 1, krylovdim))
        k, conv = 0, False
        s = None
        while k < krylovdim:
            w = V[k + 1]
            matvec(V[k], w)
            h, beta = be.orth_step(V[:k + 1], w)
            Hm[:k + 1, k] = h
            Hm[k + 1, k] = beta
            k += 1
            ev, S = np.linalg.eig(Hm[:k, :k])
            idx = int(np.argmax(np.abs(ev)))
            lam, sv = ev[idx], S[:, idx]
            res = abs(beta * sv[-1])
            ph = sv[np.argmax(np.abs(sv))]
            s = np.real(sv * np.conj(ph) / abs(ph))
            if res < tol or beta < 1e-300:
                conv = True
                break
        be.lincomb(V[:k], s, out=ritz)
        start = ritz
        if conv:
            break
    out = be.empty(*shape)
    nrm = be.norm(ritz)
    be.axpby(1.0 / nrm, ritz, 0.0, out)
    return float(np.real(lam)), out


def exponentiate(be: Backend, matvec, z: float, x0: DTensor, tol=1e-12, krylovdim=30, maxiter=100,
                 ws: KrylovWorkspace | None = None):
    """y = exp(z A) x0 for a real symmetric operator and REAL z (KrylovKit.exponentiate as called by
    integrators.jl:20-25 with z = -im*dt: imaginary-time steps dt = -i tau give z = -tau).
    Lanczos on device vectors with the fused CGS2 step; the small exp(z T_k) e_1 is formed on the
    host from the eigendecomposition of T_k; a-posteriori estimate beta_k |e_k^T exp(z T_k) e_1|;
    if krylovdim is exhausted the step is cut to the converged fraction and restarted.
    Returns (y, n_matvecs)."""
    ws = KrylovWorkspace(be) if ws is None else ws
    shape = x0.shape
    vecs = ws.get(shape, krylovdim + 2)
    V, cur = vecs[:krylovdim + 1], vecs[krylovdim + 1]
    be.axpby(1.0, x0, 0.0, cur)
    remaining, nmv = 1.0, 0
    for _ in range(maxiter):
        nrm = be.norm(cur)
        if nrm == 0.0 or remaining <= 0.0:
            break
        be.axpby(1.0 / nrm, cur, 0.0, V[0])
        Hm = np.zeros((krylovdim + 1, krylovdim))
        k, s, u = 0, remaining, None
        while k < krylovdim:
            w = V[k + 1]
            matvec(V[k], w)
            nmv += 1
            h, beta = be.orth_step(V[:k + 1], w)
            Hm[:k + 1, k] = h
            Hm[k + 1, k] = beta
            k += 1
            Tk = (Hm[:k, :k] + Hm[:k, :k].T) / 2
            ev, S = np.linalg.eigh(Tk)
            u = S @ (np.exp(remaining * z * ev) * S[0])
            if beta * abs(u[-1]) <= tol * max(remaining, 1e-300) or beta < 1e-300:
                s = remaining
                break
            if k == krylovdim:
                s = remaining
                while True:
                    u = S @ (np.exp(s * z * ev) * S[0])
                    if beta * abs(u[-1]) <= tol * s or s < 1e-12:
                        break
                    s *= 0.5
                break
        be.lincomb(V[:k], nrm * u, out=cur)
        remaining -= s
    out = be.empty(*shape)
    be.axpby(1.0, cur, 0.0, out)
    return out, nmv


def exponentiate_general(be: Backend, gen, x0: DTensor, tol=1e-12, krylovdim=30, maxiter=100,
                         ws: KrylovWorkspace | None = None):
    """y = exp(G) x0 for a general real linear generator gen(x, out) -> out (Arnoldi; the small exp of the
    Hessenberg matrix on the host).  Used for complex time steps on embedded tensors, where
    G = Im(dt) H + Re(dt) (-i H) is neither symmetric nor antisymmetric.  Same a-posteriori estimate and
    step-cutting as `exponentiate`.  Returns (y, n_matvecs)."""
    from scipy.linalg import expm
    ws = KrylovWorkspace(be) if ws is None else ws
    shape = x0.shape
    vecs = ws.get(shape, krylovdim + 2)
    V, cur = vecs[:krylovdim + 1], vecs[krylovdim + 1]
    be.axpby(1.0, x0, 0.0, cur)
    remaining, nmv = 1.0, 0
    for _ in range(maxiter):
        nrm = be.norm(cur)
        if nrm == 0.0 or remaining <= 0.0:
            break
        be.axpby(1.0 / nrm, cur, 0.0, V[0])
        Hm = np.zeros((krylovdim + 1, krylovdim))
        k, s, u = 0, remaining, None
        while k < krylovdim:
            w = V[k + 1]
            gen(V[k], w)
            nmv += 1
            h, beta = be.orth_step(V[:k + 1], w)
            Hm[:k + 1, k] = h
            Hm[k + 1, k] = beta
            k += 1
            u = expm(remaining * Hm[:k, :k])[:, 0]
            if beta * abs(u[-1]) <= tol * max(remaining, 1e-300) or beta < 1e-300:
                s = remaining
                break
            if k == krylovdim:
                s = remaining
                while True:
                    u = expm(s * Hm[:k, :k])[:, 0]
                    if beta * abs(u[-1]) <= tol * s or s < 1e-12:
                        break
                    s *= 0.5
                break
        be.lincomb(V[:k], nrm * u, out=cur)
        remaining -= s
    out = be.empty(*shape)
    be.axpby(1.0, cur, 0.0, out)
    return out, nmv


def gmres(be: Backend, matvec, b: DTensor, x0: DTensor, tol=1e-12, krylovdim=30, maxiter=100,
          ws: KrylovWorkspace | None = None, info: dict | None = None):
    """Restarted GMRES for matvec(x) = b on device vectors (KrylovKit.linsolve stand-in,
    mpohaminfenv.jl:95,113,146,164).  Returns x (new DTensor).  info: a dict that receives the convergence history's
    {"converged", "normres"} (the residual norm the solver stopped on)."""
    ws = KrylovWorkspace(be) if ws is None else ws
    shape = b.shape
    vecs = ws.get(shape, krylovdim + 3)
    V, r, tmp = vecs[:krylovdim + 1], vecs[krylovdim + 1], vecs[krylovdim + 2]
    x = be.copy(x0)
    bnorm = be.norm(b)
    if bnorm == 0:
        if info is not None:
            info.update(converged=True, normres=0.0)
        return be.zeros(*shape)
    res = np.inf
    for _ in range(maxiter):
        matvec(x, tmp)
        be.axpby(1.0, b, 0.0, r)
        be.axpby(-1.0, tmp, 1.0, r)
        beta = be.norm(r)
        if beta <= tol:
            res = beta
            break
        be.axpby(1.0 / beta, r, 0.0, V[0])
        Hm = np.zeros((krylovdim + 1, krylovdim))
        k, y = 0, None
        spec = hasattr(be, "orth_step_async")      # one-step-ahead expansion, as in eigsolve_sr

        def account(kk, h, hn):
            nonlocal y, res
            Hm[:kk + 1, kk] = h
            Hm[kk + 1, kk] = hn
            e1 = np.zeros(kk + 2)
            e1[0] = beta
            y, *_ = np.linalg.lstsq(Hm[:kk + 2, :kk + 1], e1, rcond=None)
            res = np.linalg.norm(Hm[:kk + 2, :kk + 1] @ y - e1)
            return res <= tol or hn < 1e-300

        pending, done = None, False
        while k < krylovdim:
            w = V[k + 1]
            matvec(V[k], w)
            if spec:
                hnd = be.orth_step_async(V[:k + 1], w)
                if pending is not None and account(pending[0], *pending[1].result()):
                    k, done, pending = pending[0] + 1, True, None
                    break
                pending = (k, hnd)
                k += 1
                continue
            h, hn = be.orth_step(V[:k + 1], w)
            k += 1
            if account(k - 1, h, hn):
                break
        if pending is not None and not done:
            if account(pending[0], *pending[1].result()):
                k = pending[0] + 1
        be.lincomb(V[:k], y, out=tmp)
        be.axpby(1.0, tmp, 1.0, x)
        if res <= tol:
            break
    if info is not None:
        info.update(converged=bool(res <= tol), normres=float(res))
    return x


class _RealVec:
    """the vector arithmetic linsolve needs, on real vectors (the backend's own methods)"""

    def __init__(self, be):
        self.be = be
        self.dtype = float

    def dot(self, x, y):
        return self.be.dot(x, y)

    def axpby(self, a, x, b, y):
        return self.be.axpby(float(np.real(a)), x, float(np.real(b)), y)

    def orth_step(self, xs, y):
        return self.be.orth_step(xs, y)

    def lincomb(self, xs, coefs, out):
        return self.be.lincomb(xs, np.real(coefs), out=out)


class ComplexVec:
    """the same on INTERLEAVED complex vectors: conj(x) . y, complex linear combinations, complex CGS2 (mpsk_vdotc /
    mpsk_vaxpby_c / mpsk_vorth_step_c / mpsk_vlincomb_c).  A backend without these entry points (the host stand-in of the
    CPU tests) gets them composed from its real vector methods and times_i: Im conj(x) . y = <i x, y> on the doubles."""

    def __init__(self, be):
        self.be = be
        self.dtype = complex

    def dot(self, x, y):
        be = self.be
        if hasattr(be, "dotc"):
            return be.dotc(x, y)
        return complex(be.dot(x, y), be.dot(be.times_i(x), y))

    def axpby(self, a, x, b, y):
        be = self.be
        a, b = complex(a), complex(b)
        if hasattr(be, "axpby_c"):
            return be.axpby_c(a, x, b, y)
        ix = be.times_i(x) if a.imag != 0.0 else None
        if b == 0:
            be.axpby(a.real, x, 0.0, y)
        else:
            if b.imag != 0.0:
                be.axpby(b.imag, be.times_i(y), b.real, y)
            elif b.real != 1.0:
                be.scal(b.real, y)
            be.axpby(a.real, x, 1.0, y)
        if ix is not None:
            be.axpby(a.imag, ix, 1.0, y)
        return y

    def orth_step(self, xs, y):
        be = self.be
        if hasattr(be, "orth_step_c"):
            return be.orth_step_c(xs, y)
        h = np.zeros(len(xs), dtype=complex)
        for _ in range(2):
            hh = np.array([self.dot(x, y) for x in xs])
            for c, x in zip(hh, xs):
                self.axpby(-c, x, 1.0, y)
            h += hh
        beta = be.norm(y)
        if beta > 0:
            be.scal(1.0 / beta, y)
        return h, beta

    def lincomb(self, xs, coefs, out):
        be = self.be
        if hasattr(be, "lincomb_c"):
            return be.lincomb_c(xs, coefs, out=out)
        self.axpby(coefs[0], xs[0], 0.0, out)
        for c, x in zip(coefs[1:], xs[1:]):
            self.axpby(c, x, 1.0, out)
        return out


class ConvergenceInfo:
    """what KrylovKit's linsolve returns next to the solution: converged (0 / 1), normres, numiter (restart cycles),
    numops (operator applications); hessenberg: the projected matrix of the last cycle."""

    def __init__(self, converged, normres, numiter, numops, hessenberg):
        self.converged, self.normres, self.numiter, self.numops = converged, normres, numiter, numops
        self.hessenberg = hessenberg


def linsolve(be: Backend, op, b: DTensor, x0: DTensor, a0=0.0, a1=1.0, tol=1e-12, krylovdim=30, maxiter=100,
             ws: KrylovWorkspace | None = None, cplx=False):
    """linsolve(op, b, x0, GMRES(; tol, krylovdim, maxiter), a0, a1): solve (a0 + a1 op) x = b by restarted GMRES
    (KrylovKit, as called by corvector.jl:68, :123).  op(x, out) -> out; an operator with `apply_axpby(a1, x, a0, out)`
    (a prepared H_AC, LinearCombination) applies the shifted operator in one call.  cplx: the vectors are interleaved
    complex tensors and a0, a1 may be complex -- the Krylov space is then built over the complex numbers (complex inner
    products, a complex Hessenberg matrix, complex combinations), not over the reals of the 2n-dimensional embedding, in
    which multiplication by i is not a scalar.  Converged when the residual norm is <= tol (absolute, as KrylovKit).
    Never raises on non-convergence.  Returns (x, ConvergenceInfo)."""
    ws = KrylovWorkspace(be) if ws is None else ws
    vs = ComplexVec(be) if cplx else _RealVec(be)
    shape = b.shape
    nvec = b.size // 2 if cplx else b.size
    m = int(max(1, min(krylovdim, nvec)))
    if cplx and hasattr(be, "orth_step_c"):
        m = min(m, 32)                    # mpsk_vorth_step_c orthogonalises against at most 32 vectors: shorter cycles
    vecs = ws.get(shape, m + 3, tag="linsolve")
    V, r, tmp = vecs[:m + 1], vecs[m + 1], vecs[m + 2]
    shifted = getattr(op, "apply_axpby", None)

    def apply(x, out):
        if shifted is not None:
            return shifted(a1, x, a0, out)
        op(x, out)
        return vs.axpby(a0, x, a1, out)

    x = be.copy(x0)
    Hm = np.zeros((m + 1, m), dtype=vs.dtype)
    numops, numiter, res = 0, 0, np.inf
    for numiter in range(1, maxiter + 1):
        apply(x, r)
        numops += 1
        vs.axpby(1.0, b, -1.0, r)                       # r = b - (a0 + a1 op) x
        beta = be.norm(r)
        res = beta
        if beta <= tol:
            break
        be.axpby(1.0 / beta, r, 0.0, V[0])
        Hm = np.zeros((m + 1, m), dtype=vs.dtype)
        k, y = 0, None
        while k < m:
            apply(V[k], V[k + 1])
            numops += 1
            h, hn = vs.orth_step(V[:k + 1], V[k + 1])
            Hm[:k + 1, k] = h
            Hm[k + 1, k] = hn
            k += 1
            e1 = np.zeros(k + 1, dtype=vs.dtype)
            e1[0] = beta
            y, *_ = np.linalg.lstsq(Hm[:k + 1, :k], e1, rcond=None)
            res = float(np.linalg.norm(Hm[:k + 1, :k] @ y - e1))
            if res <= tol or hn <= 1e-14 * max(np.abs(Hm[:k, :k]).max(), 1e-300):
                break
        vs.lincomb(V[:k], y, tmp)
        vs.axpby(1.0, tmp, 1.0, x)
        if res <= tol:
            break
    return x, ConvergenceInfo(int(res <= tol), float(res), numiter, numops, Hm)


def arnoldi_eigvals(be: Backend, matvec, x0: DTensor, num=1, tol=1e-10, krylovdim=60, ws: KrylovWorkspace | None = None):
    """The `num` largest-magnitude eigenvalues (complex in general) of a real non-symmetric operator matvec(x, out): one
    Arnoldi factorisation of dimension <= krylovdim, Ritz values of the Hessenberg matrix on the host; a Ritz value counts
    as converged when |beta * s_last| < tol (KrylovKit eigsolve(..., :LM) stand-in for `transfer_spectrum`, toolbox.jl:44-58).
    Returns (eigenvalues sorted by decreasing magnitude, number converged)."""
    ws = KrylovWorkspace(be) if ws is None else ws
    shape = x0.shape
    krylovdim = int(min(krylovdim, x0.size))
    V = ws.get(shape, krylovdim + 1)
    be.axpby(1.0 / be.norm(x0), x0, 0.0, V[0])
    Hm = np.zeros((krylovdim + 1, krylovdim))
    k = 0
    vals, conv = np.zeros(0, dtype=complex), 0
    while k < krylovdim:
        matvec(V[k], V[k + 1])
        h, beta = be.orth_step(V[:k + 1], V[k + 1])
        Hm[:k + 1, k] = h
        Hm[k + 1, k] = beta
        k += 1
        if k >= num and (k % 5 == 0 or k == krylovdim or beta < 1e-300):
            ev, S = np.linalg.eig(Hm[:k, :k])
            order = np.argsort(-np.abs(ev))
            vals = ev[order]
            res = np.abs(beta * S[-1, order])
            conv = int(np.sum(res[:num] < tol))
            if conv >= min(num, k) or beta < 1e-300:
                break
    return vals[:num], conv


def _planar_times_i(be, x: DTensor, out: DTensor):
    """out = i x on a planar vector [Re | Im]: [-Im | Re]."""
    N = x.size // 2
    be.lincomb([DTensor(x.buf[N:2 * N], (N,))], [-1.0], out=DTensor(out.buf[:N], (N,)))
    be.lincomb([DTensor(x.buf[:N], (N,))], [1.0], out=DTensor(out.buf[N:2 * N], (N,)))
    return out


def eigsolve_lm_planar(be: Backend, matvec, x0: DTensor, num=1, tol=1e-10, krylovdim=30, maxiter=100):
    """The `num` largest-magnitude (:LM) eigenpairs of a COMPLEX-linear, non-Hermitian operator acting on planar complex
    vectors x = [Re | Im] (one real device vector of even length): KrylovKit's eigsolve(f, x0, num, :LM, Arnoldi(...))
    as the statistical-mechanics quasiparticle solver calls it (quasiparticleexcitation.jl:182).

    The arithmetic is complex throughout: the inner product is <x, y> + i <i x, y> from two real dots (i x = [-Im | Re]),
    the Hessenberg matrix is complex and every linear combination a x is Re(a) x + Im(a) (i x), so the basis is kept as
    the pairs (v, i v).  A real Arnoldi on the 2N-dimensional embedding would instead return every eigenvalue together
    with its conjugate and mix their vectors.  Restart: the `keep` leading Ritz vectors are orthonormalised (QR of the
    eigenvector block) and the factorisation A V = V H + v r^H continues from them (a thick restart; H stays a general
    matrix, not Hessenberg, which the Ritz step does not need).

    Returns (complex eigenvalues [num], vectors [num] (planar, unit norm), residuals [num], number converged); a residual
    is |r^H s| for the Ritz pair (theta, V s).  Warns when fewer than `num` converged."""
    n2 = x0.size
    assert n2 % 2 == 0, "a planar complex vector has even length"
    m = int(max(min(krylovdim, n2 // 2), 1))
    num = int(min(num, n2 // 2))
    V = [be.empty(n2) for _ in range(m + 1)]
    IV = [be.empty(n2) for _ in range(m + 1)]
    w, tmp = be.empty(n2), be.empty(n2)
    be.axpby(1.0 / be.norm(x0), x0.reshape(n2), 0.0, V[0])
    _planar_times_i(be, V[0], IV[0])
    H = np.zeros((m + 1, m), dtype=complex)
    k = 0
    vals = S = res = None
    conv = 0
    for _restart in range(maxiter):
        while k < m:
            matvec(V[k], w)
            basis = V[:k + 1] + IV[:k + 1]
            h = np.zeros(k + 1, dtype=complex)
            for _ in range(2):                                       # classical Gram-Schmidt, twice
                dts = be.multidot(basis, w)
                c = dts[:k + 1] + 1j * dts[k + 1:]                   # <v_j, w> = <v_j, w>_R + i <i v_j, w>_R
                be.lincomb([w] + basis, [1.0] + list(-c.real) + list(-c.imag), out=tmp)
                w, tmp = tmp, w
                h += c
            beta = be.norm(w)
            H[:k + 1, k] = h
            H[k + 1, k] = beta
            k += 1
            if beta < 1e-300:
                break
            be.axpby(1.0 / beta, w, 0.0, V[k])
            _planar_times_i(be, V[k], IV[k])
            if k >= num and (k % 3 == 0 or k == m):
                ev, S = np.linalg.eig(H[:k, :k])
                order = np.argsort(-np.abs(ev))
                vals, S = ev[order], S[:, order]
                res = np.abs(H[k, :k] @ S)
                conv = int(np.sum(res[:num] < tol))
                if conv >= num:
                    break
        ev, S = np.linalg.eig(H[:k, :k])
        order = np.argsort(-np.abs(ev))
        vals, S = ev[order], S[:, order]
        res = np.abs(H[k, :k] @ S) if k < H.shape[0] else np.zeros(k)
        conv = int(np.sum(res[:num] < tol))
        if conv >= num or H[k, k - 1].real < 1e-300 or k < m:
            break
        if _restart == maxiter - 1:      # out of restarts: the Ritz pairs above belong to THIS factorisation, keep it
            break
        keep = min(max(num + 2, m // 3), m - 1)
        Q, _ = np.linalg.qr(S[:, :keep])
        newV = [be.lincomb(V[:k] + IV[:k], list(Q[:, j].real) + list(Q[:, j].imag)) for j in range(keep)]
        Hk = Q.conj().T @ H[:k, :k] @ Q
        r = H[k, :k] @ Q
        for j in range(keep):
            be.axpby(1.0, newV[j], 0.0, V[j])
            _planar_times_i(be, V[j], IV[j])
        be.axpby(1.0, V[k], 0.0, V[keep])
        _planar_times_i(be, V[keep], IV[keep])
        H[:] = 0.0
        H[:keep, :keep] = Hk
        H[keep, :keep] = r
        k = keep
    vecs = []
    for j in range(num):
        s = S[:, j]
        v = be.lincomb(V[:k] + IV[:k], list(s.real) + list(s.imag))
        vecs.append(be.scal(1.0 / be.norm(v), v))
    if conv < num:
        import warnings
        warnings.warn(f"eigsolve_lm_planar: {conv} of {num} eigenvalues converged, normres = {res[:num]}")
    return vals[:num], vecs, res[:num], conv
