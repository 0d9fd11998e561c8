"""GradientGrassmann: an MPS in left-canonical form as a product of points on Grassmann manifolds, optimised with a
preconditioned Riemannian conjugate gradient (src/algorithms/grassmann.jl, groundstate/gradient_grassmann.jl).

The geometry restates grassmann.jl: ManifoldPoint (:59-80), PrecGrad (:27-57), fg (:107-118), retract (:154-190),
transport! (:196-202), inner (:207-209), scale! / add! (:214-219), regularize (:227-235).  The two packages the reference
leans on are restated from their published definitions, not from their sources (parity with them is not pinned):
 * TensorKitManifolds.Grassmann.retract / transport!: for the thin SVD Z = U S Vt of the direction at base W,
       W'(alpha) = W Vt^T cos(alpha S) Vt + U sin(alpha S) Vt,   Z' = (-W Vt^T sin(alpha S) + U cos(alpha S)) S Vt,
       Theta'    = Theta + (U (cos(alpha S) - 1) - W Vt^T sin(alpha S)) U^T Theta,
   followed here by a QRpos of W' and a projection of Z' / Theta' on the complement of W' (both are no-ops up to rounding).
 * OptimKit.ConjugateGradient with the Hager-Zhang beta and a bracketing line search that ends on the (approximate) Wolfe
   conditions; iteration-by-iteration parity with OptimKit is not claimed.

Per direction and site P = W Vt^T and U are cached; a trial step at a new alpha is then one coefficient launch
(mpsk_grassmann_coef: no device-to-host copy), one mpsk_gemm_pair (both outputs from one read of P and U), one QRpos and
the projection.  The composed route (plain GEMMs with host-built diagonal matrices) is what the NumPy stand-in backend of
the CPU tests runs and what the device route is measured against.

Real fp64 states only; complex states raise through _no_cplx.  The MPSMultiline variant (grassmann.jl:82-101, :119-149)
and LBFGS are not built."""
from __future__ import annotations

import time
import warnings

import numpy as np

from .backend import DTensor
from .derivatives import ddAC
from .states import FiniteMPS, InfiniteMPS

DEVICE_ROUTE_MIN = 64      # min(Dl d, Dr) up to which the composed route is used: below one 64-wide tile the launches of
                           # either route cost the same and the host diagonal is a few hundred bytes


def _device_route(be, m, n, route=None):
    if route is not None:
        if route not in ("device", "composed"):
            raise ValueError(f"route must be 'device' or 'composed', not {route!r}")
        if route == "device" and not (hasattr(be, "gemm_pair") and hasattr(be, "grassmann_coef")):
            raise RuntimeError("the device route needs a backend with gemm_pair and grassmann_coef")
        return route == "device"
    return hasattr(be, "gemm_pair") and hasattr(be, "grassmann_coef") and min(m, n) > DEVICE_ROUTE_MIN


def _mat(t: DTensor):
    Dl, d, Dr = t.shape
    return t.reshape(Dl * d, Dr)


def _diag(be, v):
    return be.upload(np.diag(np.asarray(v, dtype=float)))


def _project_out(be, W: DTensor, X: DTensor):
    """X -= W (W^T X) in place (Grassmann.project, grassmann.jl:72)."""
    t = be.gemm(W, X, transA=True)
    be.gemm(W, t, alpha=-1.0, beta=1.0, out=X)
    return X


# ---- state accessors: FiniteMPS has lazy views, InfiniteMPS plain lists ----------------------------------------------

def _AL(state, i):
    return state.AL(i) if isinstance(state, FiniteMPS) else state.AL[i]


def _CR(state, i):
    return state.CR(i) if isinstance(state, FiniteMPS) else state.CR[i]


def _AC(state, i):
    return state.AC(i) if isinstance(state, FiniteMPS) else state.AC[i]


def _finite_from_AL(be, ALs, C, cplx=False):
    """the FiniteMPS AL_1 .. AL_L C with C normalised: what `y.AC[i] = (yal, CR[i])` for i = 1 .. L followed by
    normalize!(y) leaves behind (grassmann.jl:178-185: every bond matrix but the last is dropped by the next assignment)."""
    o = object.__new__(FiniteMPS)
    N = len(ALs)
    o.be, o.N, o.cplx = be, N, cplx
    o.ALs, o.ARs, o.ACs, o.CLs = list(ALs), [None] * N, [None] * N, [None] * (N + 1)
    c = be.copy(C)
    be.scal(1.0 / be.norm(c), c)
    o.CLs[N] = c
    return o


# ---- regularised density matrices and tangents -------------------------------------------------------------------------

class Rhoreg:
    """regularize(CR, delta) = U (S^2 + (max(S) delta)^2) U^T for CR = U S Vt (grassmann.jl:227-235; the code at :231, no
    sqrt(eps) floor), kept in factored form: the preconditioned gradient only needs Vt^T diag(s / sreg) U^T."""

    def __init__(self, be, C: DTensor, delta: float, device: bool):
        self.be, self.delta, self.device = be, float(delta), device
        self.U, self.S, self.Vt, _, _ = be.tsvd(C)
        self._matrix = None

    def _s(self):
        return np.asarray(self.be.download(self.S)).reshape(-1)

    def apply_inverse(self, g: DTensor):
        """g Vt^T diag(s / (s^2 + (max(s) delta)^2)) U^T  ==  (g CR^T) inv(Rhoreg)   (grassmann.jl:36, :112)."""
        be = self.be
        if self.device:
            coef = be.grassmann_coef(self.S, self.delta, "precondition")
            XT, _ = be.gemm_pair(self.U, None, self.Vt, coef, two=False)          # X^T = U diag(a) Vt
        else:
            s = self._s()
            a = s / (s ** 2 + (s.max() * self.delta) ** 2)
            XT = be.gemm(be.gemm(self.U, _diag(be, a)), self.Vt)
        return be.gemm(g, XT, transB=True)

    def matrix(self):
        if self._matrix is None:
            be, s = self.be, self._s()
            sreg = s ** 2 + (s.max() * self.delta) ** 2
            self._matrix = be.gemm(be.gemm(self.U, _diag(be, sreg)), self.U, transB=True)
        return self._matrix


class PrecGrad:
    """grassmann.jl:27-36: Pg (the Grassmann tangent that is retracted along), g = Pg rho, rho (None: the identity --
    tangents that come back from retract / transport!)."""
    __slots__ = ("Pg", "g", "rho", "_svd")

    def __init__(self, Pg: DTensor, g: DTensor = None, rho: Rhoreg = None):
        self.Pg, self.g, self.rho = Pg, (Pg if g is None else g), rho
        self._svd = None


def _inner_site(be, g1: PrecGrad, g2: PrecGrad, rho: Rhoreg):  # grassmann.jl:39-48
    if g1.rho is rho:
        return be.dot(g1.g, g2.Pg)
    if g2.rho is rho:
        return be.dot(g1.Pg, g2.g)
    return be.dot(g1.Pg, be.gemm(g2.Pg, rho.matrix()))


def inner(x, g1, g2):
    """grassmann.jl:207-209."""
    return 2.0 * float(sum(_inner_site(x.be, b, c, a) for a, b, c in zip(x.Rhoreg, g1, g2)))


def _scaled(be, x: DTensor, a):
    return be.scal(a, be.copy(x))


def _axpy_new(be, alpha, x: DTensor, y: DTensor):
    out = be.copy(y)
    be.axpby(alpha, x, 1.0, out)
    return out


def scale(be, g, alpha):
    """scale!(g, alpha) = g .* alpha  (grassmann.jl:50, :214)."""
    return [PrecGrad(_scaled(be, t.Pg, alpha), None if t.g is t.Pg else _scaled(be, t.g, alpha), t.rho) for t in g]


def add(be, g1, g2, alpha):
    """add!(g1, g2, alpha) = g1 + g2 .* alpha  (grassmann.jl:51-57, :219): tangents with different rho add up to one
    with the identity rho."""
    out = []
    for a, b in zip(g1, g2):
        Pg = _axpy_new(be, alpha, b.Pg, a.Pg)
        if a.rho is b.rho and a.rho is not None:
            out.append(PrecGrad(Pg, _axpy_new(be, alpha, b.g, a.g), a.rho))
        else:
            out.append(PrecGrad(Pg))
    return out


# ---- the manifold point ------------------------------------------------------------------------------------------------

class ManifoldPoint:
    """grassmann.jl:59-80: state, environments, the site gradients g_i = X_i - AL_i (AL_i^T X_i), X_i = H_AC(AC_i), and the
    regularised density matrices Rhoreg_i = regularize(CR_i, |g_i| / 10).  The environments object is shared by every point
    of an optimisation and follows the state that was evaluated last, so the energy is taken here, while it fits."""

    def __init__(self, state, envs, route=None):
        be = self.be = state.be
        self.state, self.envs, self.route = state, envs, route
        H = envs.H
        n = len(state)
        if isinstance(state, InfiniteMPS) and hasattr(envs, "dependency") and envs.dependency is not state:
            envs.recalculate(state)            # (the terms of a MultipleEnvironments follow the state on their own)
        self.g, self.hac_norm = [], []
        for i in range(n):
            X = _mat(ddAC(i, state, H, envs)(_AC(state, i)))
            self.hac_norm.append(be.norm(X))
            self.g.append(_project_out(be, _mat(_AL(state, i)), X))
        self.gnorm = [be.norm(g) for g in self.g]
        self.Rhoreg = []
        for i in range(n):
            m, k = self.g[i].shape
            self.Rhoreg.append(Rhoreg(be, _CR(state, i), self.gnorm[i] / 10.0, _device_route(be, m, k, route)))
        from .algorithms import expectation_value
        self.f = float(np.sum(expectation_value(state, H, envs)))


def fg(x: ManifoldPoint):
    """grassmann.jl:107-118: the energy and the preconditioned gradient PrecGrad(g_i CR_i^T, Rhoreg_i)."""
    be = x.be
    out = []
    for i, g in enumerate(x.g):
        v = be.gemm(g, _CR(x.state, i), transB=True)
        out.append(PrecGrad(x.Rhoreg[i].apply_inverse(g), v, x.Rhoreg[i]))
    return x.f, out


# ---- retraction and transport --------------------------------------------------------------------------------------------

def _direction_svd(be, W: DTensor, t: PrecGrad):
    """cache of one direction at one site: Z = U S Vt, P = W Vt^T (once per direction, shared by every trial alpha).
    A direction at W has rank <= m - n.  Where that is below n (a bond that grows by less than d) the SVD has zero singular
    values, behind which a one-sided Jacobi may leave zero rows in Vt instead of an orthonormal completion; the formula
    W Vt^T cos(0) Vt = W needs the completion.  LQpos of Vt supplies it: the rows in front (S is descending) are orthonormal
    and come back unchanged, with a unit diagonal in L, the rest are completed -- as tsplit does for its rank-deficient case."""
    if t._svd is None:
        m, n = t.Pg.shape
        U, S, Vt, _, _ = be.tsvd(t.Pg)
        if m - n < n:
            _, Vt = be.lqpos(Vt)
        t._svd = (U, S, Vt, be.gemm(W, Vt, transB=True))
    return t._svd


def _coef_host(s, alpha, mode):
    if mode == "retract":
        return np.cos(alpha * s), np.sin(alpha * s), -s * np.sin(alpha * s), s * np.cos(alpha * s)
    return -np.sin(alpha * s), np.cos(alpha * s) - 1.0


def retract_site(be, W: DTensor, t: PrecGrad, alpha: float, route=None):
    """(W', Z') of Grassmann.retract(W, Z, alpha): W' re-orthonormalised (QRpos, Q kept), Z' projected on its complement."""
    m, n = t.Pg.shape
    if m == n:                                   # a square isometry has no tangent space
        return W, be.zeros(m, n)
    device = _device_route(be, m, n, route)
    U, S, Vt, P = _direction_svd(be, W, t)
    if device:
        coef = be.grassmann_coef(S, alpha, "retract")
        Wn, Zn = be.gemm_pair(P, U, Vt, coef)
    else:
        a1, b1, a2, b2 = _coef_host(np.asarray(be.download(S)).reshape(-1), alpha, "retract")
        Wn = be.gemm(P, be.gemm(_diag(be, a1), Vt))
        be.gemm(U, be.gemm(_diag(be, b1), Vt), beta=1.0, out=Wn)
        Zn = be.gemm(P, be.gemm(_diag(be, a2), Vt))
        be.gemm(U, be.gemm(_diag(be, b2), Vt), beta=1.0, out=Zn)
    Wn, _ = be.qrpos(Wn)
    return Wn, _project_out(be, Wn, Zn)


def transport_site(be, Theta: DTensor, W: DTensor, t: PrecGrad, alpha: float, Wn: DTensor, route=None):
    """Grassmann.transport!(Theta, W, Z, alpha, W') for the direction t at base W; returns a new tensor."""
    m, n = t.Pg.shape
    out = be.copy(Theta)
    if m == n:
        return out
    device = _device_route(be, m, n, route)
    U, S, Vt, P = _direction_svd(be, W, t)
    B = be.gemm(U, Theta, transA=True)
    if device:
        coef = be.grassmann_coef(S, alpha, "transport")
        be.gemm_pair(P, U, B, coef, out1=out, beta1=1.0, two=False)
    else:
        a1, b1 = _coef_host(np.asarray(be.download(S)).reshape(-1), alpha, "transport")
        be.gemm(P, be.gemm(_diag(be, a1), B), beta=1.0, out=out)
        be.gemm(U, be.gemm(_diag(be, b1), B), beta=1.0, out=out)
    return _project_out(be, Wn, out)


def retract_state(x: ManifoldPoint, g, alpha):
    """the state at the end point and the tangent there: InfiniteMPS.from_AL(newAL, CR[end]), or the finite chain of the
    new AL with the old last bond matrix, normalised (grassmann.jl:154-190)."""
    be, state = x.be, x.state
    nal, h = [], []
    for i, t in enumerate(g):
        al = _AL(state, i)
        Wn, Zn = retract_site(be, _mat(al), t, alpha, x.route)
        nal.append(Wn.reshape(*al.shape))
        h.append(PrecGrad(Zn))
    n = len(state)
    if isinstance(state, FiniteMPS):
        return _finite_from_AL(be, nal, _CR(state, n - 1), state.cplx), h
    return InfiniteMPS.from_AL(nal, state.CR[n - 1], be=be), h


def retract(x: ManifoldPoint, g, alpha):
    """grassmann.jl:154-190: the end point (with the environments recalculated for it) and the tangent there."""
    nstate, h = retract_state(x, g, alpha)
    return ManifoldPoint(nstate, x.envs, x.route), h


def transport(h, x: ManifoldPoint, g, alpha, xp: ManifoldPoint):
    """grassmann.jl:196-202."""
    be = x.be
    return [PrecGrad(transport_site(be, h[i].Pg, _mat(_AL(x.state, i)), g[i], alpha, _mat(_AL(xp.state, i)), x.route))
            for i in range(len(h))]


# ---- optimiser: Riemannian conjugate gradient ------------------------------------------------------------------------------

C1, C2, EPS_WOLFE = 0.1, 0.9, 5e-14      # Wolfe constants (Hager-Zhang's delta, sigma); the approximate conditions accept
                                         # f <= f0 + EPS_WOLFE |f0|: near a gradient norm of 1e-8 the decrease (~ 1e-16) is
                                         # below the rounding of the energy and only the slope can be trusted
EXPAND, MAX_LS = 5.0, 24                 # bracket growth factor; function evaluations per line search
HZ_THETA, HZ_ETA = 2.0, 0.4              # Hager-Zhang beta and its lower bound


class LineSearchFailed(RuntimeError):
    pass


def _linesearch(x, f0, g0, eta, df0, alpha0):
    """Bracketing line search along eta from x: returns (alpha, x', f', g', xi) with the (approximate) Wolfe conditions
    met; xi is eta transported to x'.  Bracket [a, b]: phi'(a) < 0 with phi(a) <= phi(0) + eps, and phi'(b) >= 0 or
    phi(b) above that level; inside it secant steps on the slope, bisection when the secant leaves the middle 80 %."""
    eps_k = EPS_WOLFE * abs(f0)

    def phi(alpha):
        xp, xi = retract(x, eta, alpha)
        f, g = fg(xp)
        return f, inner(xp, g, xi), xp, g, xi

    def wolfe(alpha, f, df):
        exact = f <= f0 + C1 * alpha * df0 and df >= C2 * df0
        approx = f <= f0 + eps_k and (2.0 * C1 - 1.0) * df0 >= df >= C2 * df0
        return exact or approx

    a, fa, dfa = 0.0, f0, df0
    b = fb = dfb = None
    alpha = alpha0
    for _ in range(MAX_LS):
        f, df, xp, g, xi = phi(alpha)
        if np.isfinite(f) and wolfe(alpha, f, df):
            return alpha, xp, f, g, xi
        if not np.isfinite(f) or f > f0 + eps_k or df >= 0.0:
            b, fb, dfb = alpha, f, df
        else:
            a, fa, dfa = alpha, f, df
        if b is None:
            alpha = EXPAND * alpha
            continue
        if np.isfinite(fb) and dfb > dfa and dfb >= 0.0 and fb <= f0 + eps_k:
            alpha = a - dfa * (b - a) / (dfb - dfa)                    # secant on the slope
        elif np.isfinite(fb):
            # the value at b is too high: minimiser of the quadratic through phi(a), phi'(a), phi(b)
            den = 2.0 * (fb - fa - dfa * (b - a))
            alpha = a - dfa * (b - a) ** 2 / den if den > 0.0 else 0.5 * (a + b)
        else:
            alpha = 0.5 * (a + b)
        lo, hi = a + 0.1 * (b - a), b - 0.1 * (b - a)
        if not (lo <= alpha <= hi):
            alpha = 0.5 * (a + b)
        if b - a <= 1e-15 * max(1.0, abs(b)):
            break
    raise LineSearchFailed(f"no step with the Wolfe conditions in {MAX_LS} evaluations (bracket [{a:.3e}, {b}])")


def optimize(x: ManifoldPoint, tol, maxiter, verbosity=0, finalize=None):
    """Riemannian nonlinear conjugate gradient (the reference's default method, gradient_grassmann.jl:30): Hager-Zhang
    beta, first trial step from the previous accepted one, restart on a non-descent direction, stop on
    sqrt(inner(g, g)) <= tol.  Returns (x, f, g, history) with history rows (iteration, f, |g|)."""
    be = x.be
    t0 = time.time()
    f, g = fg(x)
    normgrad = np.sqrt(max(inner(x, g, g), 0.0))
    history = [(0, f, normgrad)]
    eta = scale(be, g, -1.0)
    alpha = 1.0
    for it in range(1, maxiter + 1):
        if normgrad <= tol:
            break
        df0 = inner(x, g, eta)
        if df0 >= 0.0:                                           # not a descent direction: restart on the gradient
            eta = scale(be, g, -1.0)
            df0 = inner(x, g, eta)
        try:
            alpha, xn, fn, gn, xi = _linesearch(x, f, g, eta, df0, alpha)
        except LineSearchFailed as e:
            warnings.warn(f"GradientGrassmann stops at iteration {it}, |g| = {normgrad:.3e}: {e}")
            break
        gprev = transport(g, x, eta, alpha, xn)
        x, f, g = xn, fn, gn
        if finalize is not None:
            x, f, g = finalize(x, f, g, it)
        gg = inner(x, g, g)
        normgrad = np.sqrt(max(gg, 0.0))
        history.append((it, f, normgrad))
        if verbosity >= 3:
            print(f"[ Info: CG {it:3d}:\tobj = {f:+.12e}\t|g| = {normgrad:.10e}\talpha = {alpha:.3e}\t"
                  f"time = {time.time() - t0:.2f} sec", flush=True)
        dd, dg, dgprev = inner(x, xi, xi), inner(x, xi, g), inner(x, xi, gprev)
        ggprev, gpgp = inner(x, g, gprev), inner(x, gprev, gprev)
        dy, gy, yy = dg - dgprev, gg - ggprev, gg + gpgp - 2.0 * ggprev
        if dy == 0.0 or dd <= 0.0:
            eta = scale(be, g, -1.0)
            continue
        beta = (gy - HZ_THETA * (yy / dy) * dg) / dy
        beta = max(beta, -1.0 / np.sqrt(dd * min(HZ_ETA ** 2, gpgp))) if gpgp > 0.0 else beta
        eta = add(be, scale(be, g, -1.0), xi, beta)
    return x, f, g, history


def find_groundstate_grassmann(psi, H, alg, envs=None):
    """find_groundstate(psi, H, GradientGrassmann, envs) -> (psi, envs, |g|)   (gradient_grassmann.jl:46-65)."""
    from .algorithms import _no_cplx
    from .environments import environments
    _no_cplx(psi, "GradientGrassmann")
    be = psi.be
    if isinstance(psi, FiniteMPS):
        n = len(psi)
        if psi.CR(n - 1).size != 1:
            warnings.warn("This is not fully supported - split the mps up in a sum of mps's and optimize seperately")
        psi = psi.copy()
        psi = _finite_from_AL(be, [psi.AL(i) for i in range(n)], psi.CR(n - 1), psi.cplx)       # normalize!(psi)
    envs = environments(psi, H) if envs is None else envs
    x, f, g, history = optimize(ManifoldPoint(psi, envs, getattr(alg, "route", None)), alg.tol, alg.maxiter, alg.verbosity,
                                alg.finalize)
    if isinstance(x.state, InfiniteMPS):     # a rejected trial point may have been evaluated last: follow the final state
        for e in getattr(envs, "envs", [envs]):
            if getattr(e, "dependency", x.state) is not x.state:
                e.recalculate(x.state)
    envs.history = history
    return x.state, envs, history[-1][2]
