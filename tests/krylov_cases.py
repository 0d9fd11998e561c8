"""Inputs, dense references and bounds for the Krylov solvers of mpskit_jl_amd/krylov.py driven by a backend: the same
cases run through tests/cpu_backend.py (tests/test_krylov_cases_cpu.py, which proves every bound and every condition on
the host alone) and through the real Backend and its `hide` proxies (tests/test_gpu_krylov_paths.py).  Importable without
a GPU.

Operators are dense matrices Q diag(lambda) Q^T from a seeded orthogonal Q (spectra, gaps and condition numbers known by
construction; the non-symmetric ones add an antisymmetric part or a diagonal similarity), applied on the device as
be.gemm(Ad, x, out=out) on (n, 1) vectors, be.gemm_c on interleaved complex ones and one gemm on the (n, 2) view of a
planar vector.  The one exception is the breakdown case "d": integer data on three coordinates, every step of which is
exact in fp64, so that the third beta is exactly 0.

Bars (u = 2^-53, everything evaluated in longdouble on the downloaded vectors; no figure comes from the device):
  symmetric eigenpair   r = |A v - lam v| / |v|.  |lam - lambda_nearest| <= r and sin(v, v_0) <= r / gap with
                        gap = min_{i > 0} |lambda_i - lam| (Parlett, The Symmetric Eigenvalue Problem, 4.5.1 and 11.7.1).
                        The reference pair is numpy's eigh; its own residual r_ref, measured the same way, is added to both.
  non-normal eigenpair  the same to first order with kappa = 1 / |y^H x| of the dense left / right eigenvectors in front.
  linear systems        |x - x_dense| <= |A^-1|_2 (r + r_ref), r = |b - A x|, |A^-1|_2 from the dense SVD.
  size of r             no theorem: r_device <= max(tol, 4 r_host), the same solver on the host stand-in with the same
                        inputs (two doublings for numpy's pairwise sums against the kernels' blocked ones), and the
                        host run itself is held to r_host <= tol (size_bar), so a solve that stops early on both
                        backends fails.  The same for the error of the exponentiators against scipy's expm applied in
                        longdouble; there the host and the device are both held to 1e-10 max |reference|
                        (tests/test_gpu_algorithms.py::test_exponentiate_matches_dense).
  first_image           A x0 / |x0| (longdouble) within (K + 4) u |A| |x|, the GEMM bound of tests/exact_inputs.py, K = n.
  unit norm             | |v| - 1 | <= (n / 2 + 4) u for a returned vector of n doubles (norm_bar).
"""
from __future__ import annotations

import functools
import zlib

import numpy as np

from exact_inputs import CLD, LD, U
from mpskit_jl_amd import krylov

TOL = 1e-12


# ------------------------------------------------------------------------------------------------------------------
# backends
# ------------------------------------------------------------------------------------------------------------------
class _Hidden:
    """`be` without some of its attributes"""

    def __init__(self, be, names):
        object.__setattr__(self, "_be", be)
        object.__setattr__(self, "_names", frozenset(names))

    def __getattr__(self, name):
        if name in self._names:
            raise AttributeError(name)
        return getattr(self._be, name)

    def __setattr__(self, name, value):
        setattr(self._be, name, value)


def hide(be, *names):
    """a proxy that forwards every attribute to `be` except the named ones, which raise AttributeError:
    hide(be, "orth_step_async") is the same device without the speculation, hide(be, "multilincomb") shrinks with the
    per-vector lincomb loop"""
    for nm in names:
        assert hasattr(be, nm), nm
    return _Hidden(be, names)


def host_backend():
    from cpu_backend import CpuComplexBackend
    return CpuComplexBackend()


def _rng(name):
    return np.random.default_rng(zlib.crc32(("krylov-" + name).encode()))


def orthogonal(rng, n, first=None):
    """seeded orthogonal matrix; first: its first column (normalised)"""
    G = rng.standard_normal((n, n))
    if first is not None:
        G[:, 0] = first
    Q, R = np.linalg.qr(G)
    return Q * np.sign(np.diag(R))


def from_spectrum(rng, lam):
    Q = orthogonal(rng, len(lam))
    A = (Q * np.asarray(lam)) @ Q.T
    return (A + A.T) / 2


def up(be, v):
    return be.upload(np.array(v, dtype=float).reshape(-1, 1))


def down(be, t):
    return be.download(t).reshape(-1)


def dense_op(be, A):
    """(matvec, counter): one be.gemm per application"""
    Ad = be.upload(np.array(A))
    count = [0]

    def mv(x, out):
        count[0] += 1
        return be.gemm(Ad, x, out=out)
    return mv, count


def size_bar(tol, host=None):
    """the bar on the size of a residual or error: the host run (host None) is held to tol alone, which anchors the
    device bar max(tol, 4 host)"""
    return tol if host is None else np.maximum(tol, 4 * np.asarray(host))


def norm_bar(n):
    """| |v| - 1 | of a vector of n doubles scaled by 1 / |v|: a sum of n squares in any order ((n + 1) u on |v|^2, halved
    by the square root, which adds one rounding), a reciprocal, a product: (n / 2 + 3.5) u to first order"""
    return (n / 2 + 4) * U


def nrm(x):
    x = np.asarray(x)
    return float(np.sqrt((np.abs(x.astype(CLD if np.iscomplexobj(x) else LD)) ** 2).sum()))


# ------------------------------------------------------------------------------------------------------------------
# eigsolve_sr, tolerance mode
# ------------------------------------------------------------------------------------------------------------------
EIG = {
    # (a) convergence inside the first cycle: the lowest eigenvalue is far below a band
    "a96": dict(n=96, lam=lambda n: np.r_[-4.0, np.linspace(0.0, 1.0, n - 1)], krylovdim=30, maxiter=100),
    "a257": dict(n=257, lam=lambda n: np.r_[-4.0, np.linspace(0.0, 1.0, n - 1)], krylovdim=30, maxiter=100),
    # (b) thick restarts through multilincomb (m = 8, keep = 4): a cluster just above the lowest eigenvalue
    "b96": dict(n=96, lam=lambda n: np.r_[0.0, 0.25 + 0.004 * np.arange(5), np.linspace(1.5, 3.0, n - 6)], krylovdim=8,
                maxiter=400),
    "b257": dict(n=257, lam=lambda n: np.r_[0.0, 0.25 + 0.004 * np.arange(5), np.linspace(1.5, 3.0, n - 6)], krylovdim=8,
                 maxiter=400),
    # (c) m = 40 > 32: the shrink goes through the lincomb loop
    "c96": dict(n=96, lam=lambda n: np.r_[0.0, np.linspace(0.02, 1.0, n - 1)], krylovdim=40, maxiter=100),
    "c257": dict(n=257, lam=lambda n: np.r_[0.0, np.linspace(0.02, 1.0, n - 1)], krylovdim=40, maxiter=100),
    # (d) exact breakdown at step 3
    "d96": dict(n=96, krylovdim=30, maxiter=100),
    # (e) the vector-space dimension ends the solve
    "e1": dict(n=1, krylovdim=30, maxiter=100),
    "e2": dict(n=2, krylovdim=30, maxiter=100),
}
SPEC_EIG = list(EIG)
D_SUPPORT = (5, 40, 77)
D_BLOCK = np.array([[-8.0, 2.0, 0.0], [2.0, -7.0, 4.0], [0.0, 4.0, -6.0]])


@functools.lru_cache(maxsize=None)
def eig_case(name):
    """A, x0, the dense eigensystem (ew ascending, V), the residual of its lowest pair in longdouble; never modified"""
    c = dict(EIG[name])
    n, rng = c["n"], _rng(name)
    if name.startswith("d"):
        # A = T on the coordinates D_SUPPORT (a tridiagonal integer block whose off-diagonals are powers of two) and a
        # positive definite block on the others; x0 = 4 e_i.  Every Lanczos vector is a coordinate vector: A e_i = -8 e_i
        # + 2 e_j, remainder 2 e_j, |.|^2 = 4, e_j = 0.5 (2 e_j); A e_j leaves 4 e_k, |.|^2 = 16; A e_k = 4 e_j - 6 e_k
        # leaves exactly 0.  No operation rounds, so beta_3 == 0.0 on any backend.
        rest = np.setdiff1d(np.arange(n), D_SUPPORT)
        A = np.zeros((n, n))
        A[np.ix_(rest, rest)] = from_spectrum(rng, np.linspace(1.0, 3.0, n - 3))
        A[np.ix_(D_SUPPORT, D_SUPPORT)] = D_BLOCK
        x0 = np.zeros(n)
        x0[D_SUPPORT[0]] = 4.0
    elif name == "e1":
        A, x0 = np.array([[3.0]]), np.array([-0.7])
    elif name == "e2":
        A, x0 = np.array([[2.0, 1.0], [1.0, 3.0]]), np.array([0.6, -1.1])
    else:
        A = from_spectrum(rng, c["lam"](n))
        x0 = rng.standard_normal(n)
    ew, V = np.linalg.eigh(A)
    v0 = V[:, 0].astype(LD)
    v0 = v0 / np.sqrt((v0 * v0).sum())
    r_ref = nrm(A.astype(LD) @ v0 - LD(ew[0]) * v0)
    for a in (A, x0, ew, V):
        a.setflags(write=False)
    c.update(name=name, A=A, x0=x0, ew=ew, V=V, v0=v0, r_ref=r_ref, gap=float(ew[1] - ew[0]) if n > 1 else np.inf, tol=TOL)
    return c


def run_eig(be, name, ws=None, first=False, x0=None):
    """one tolerance-mode solve -> dict(lam, v, nmv, res, applied, first)"""
    c = eig_case(name)
    mv, count = dense_op(be, c["A"])
    f = up(be, np.full(c["n"], np.nan)) if first else None
    lam, out, nmv, res = krylov.eigsolve_sr(be, mv, up(be, c["x0"] if x0 is None else x0), tol=c["tol"],
                                            krylovdim=c["krylovdim"], maxiter=c["maxiter"], ws=ws, first_image=f)
    return dict(lam=float(lam), v=down(be, out), nmv=nmv, res=float(res), applied=count[0],
                first=None if f is None else down(be, f))


def eig_figures(name, g):
    """the quantities the bars are written in, from the downloaded pair alone"""
    c = eig_case(name)
    A, v = c["A"].astype(LD), g["v"].astype(LD)
    vn = np.sqrt((v * v).sum())
    r = nrm(A @ v - LD(g["lam"]) * v) / float(vn)
    near = int(np.argmin(np.abs(c["ew"] - g["lam"])))
    ov = (c["v0"] * v).sum() / vn
    sin = nrm(v / vn - ov * c["v0"])
    gap = float(np.min(np.abs(c["ew"][1:] - g["lam"]))) - c["r_ref"] if c["n"] > 1 else np.inf
    return dict(r=r, nearest=near, lam_err=abs(g["lam"] - float(c["ew"][near])), sin=sin, gap=gap, norm=float(vn))


def check_eig(name, g, r_host=None):
    """the theorems, and the size of r against the host run (r_host None: this IS the host run, r <= tol is asked)"""
    c, f = eig_case(name), eig_figures(name, g)
    assert np.isfinite(g["v"]).all() and np.isfinite(g["lam"]) and np.isfinite(g["res"]), (name, g)
    assert abs(f["norm"] - 1.0) <= norm_bar(c["n"]), (name, f)
    assert f["nearest"] == 0, (name, f)
    assert f["lam_err"] <= f["r"] + c["r_ref"], (name, f)
    if c["n"] > 1:
        assert f["gap"] > 0 and f["sin"] <= (f["r"] + c["r_ref"]) / f["gap"], (name, f)
    assert g["res"] <= c["tol"], (name, g["res"])
    assert f["r"] <= size_bar(c["tol"], r_host), (name, f, r_host)
    return f


def first_image_bound(name):
    """(reference A x0 / |x0| in longdouble, componentwise bound)"""
    c = eig_case(name)
    A, x = c["A"].astype(LD), c["x0"].astype(LD)
    x = x / np.sqrt((x * x).sum())
    return A @ x, (c["n"] + 4) * U * (np.abs(A) @ np.abs(x))


# ------------------------------------------------------------------------------------------------------------------
# gmres
# ------------------------------------------------------------------------------------------------------------------
GMRES = {
    "one96": dict(n=96, krylovdim=30, maxiter=100),          # converges in one cycle
    "one257": dict(n=257, krylovdim=30, maxiter=100),
    "restart257": dict(n=257, krylovdim=5, maxiter=100),     # forced restarts
    "zero_b": dict(n=96, krylovdim=30, maxiter=100),         # early return
    "exact_x0": dict(n=96, krylovdim=30, maxiter=100),       # the first beta <= tol exit
}
SPEC_GMRES = list(GMRES)


def nonsym(rng, n, lo=1.0, hi=2.0, skew=0.3):
    """S + K: S = Q diag(lambda) Q^T with lambda in [lo, hi], K antisymmetric with |K|_2 = skew.  x^T (S + K) x = x^T S x,
    so sigma_min >= lo, and |A| <= hi + skew: cond <= (hi + skew) / lo"""
    S = from_spectrum(rng, np.linspace(lo, hi, n))
    G = rng.standard_normal((n, n))
    K = G - G.T
    return S, K * (skew / np.linalg.norm(K, 2))


@functools.lru_cache(maxsize=None)
def gmres_case(name):
    c = dict(GMRES[name])
    n, rng = c["n"], _rng("gmres-%d" % c["n"])
    S, K = nonsym(rng, n)
    A = S + K
    xs = rng.standard_normal(n)
    if name == "zero_b":
        b, x0 = np.zeros(n), rng.standard_normal(n)
    elif name == "exact_x0":
        b, x0 = A @ xs, xs.copy()
    else:
        b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    xd = np.linalg.solve(A, b)
    sv = np.linalg.svd(A, compute_uv=False)
    r_ref = nrm(b.astype(LD) - A.astype(LD) @ xd.astype(LD))
    c.update(name=name, A=A, b=b, x0=x0, xd=xd, inv_norm=float(1.0 / sv[-1]), cond=float(sv[0] / sv[-1]), r_ref=r_ref, tol=TOL)
    return c


def run_gmres(be, name, ws=None):
    c = gmres_case(name)
    mv, count = dense_op(be, c["A"])
    info = {}
    x = krylov.gmres(be, mv, up(be, c["b"]), up(be, c["x0"]), tol=c["tol"], krylovdim=c["krylovdim"], maxiter=c["maxiter"],
                     ws=ws, info=info)
    return dict(x=down(be, x), info=info, applied=count[0])


def solve_figures(c, x):
    """r = |b - A x| and |x - x_dense| in longdouble (complex cases alike)"""
    T = CLD if np.iscomplexobj(c["A"]) or np.iscomplexobj(x) else LD
    r = nrm(c["b"].astype(T) - c["A"].astype(T) @ x.astype(T))
    return dict(r=r, err=nrm(x.astype(T) - c["xd"].astype(T)))


def check_solve(c, x, r_host=None):
    f = solve_figures(c, x)
    assert np.isfinite(x).all(), c["name"]
    assert f["err"] <= c["inv_norm"] * (f["r"] + c["r_ref"]), (c["name"], f)
    assert f["r"] <= size_bar(c["tol"], r_host), (c["name"], f, r_host)
    return f


# ------------------------------------------------------------------------------------------------------------------
# nested solve: outer eigsolve_sr whose matvec is an inner gmres with an SPD matrix (the outer operator is S^-1)
# ------------------------------------------------------------------------------------------------------------------
NEST_TOL_OUTER, NEST_TOL_INNER = 1e-9, 1e-13


@functools.lru_cache(maxsize=None)
def nest_case():
    n, rng = 96, _rng("nest")
    S = from_spectrum(rng, np.r_[np.linspace(1.0, 2.0, n - 1), 4.0])
    ew, V = np.linalg.eigh(S)
    return dict(n=n, S=S, x0=rng.standard_normal(n), lam=1.0 / float(ew[-1]), v=V[:, -1], gap=1.0 / float(ew[-2]) - 1.0 / float(ew[-1]))


def run_nest(be):
    """-> dict(lam, v, nmv, res, inner: applications of S, unconverged: inner solves that missed their tolerance)"""
    c = nest_case()
    inner, count = dense_op(be, c["S"])
    zero = be.zeros(c["n"], 1)
    ws_in = krylov.KrylovWorkspace(be)
    missed = [0]

    def mv(x, out):
        info = {}
        y = krylov.gmres(be, inner, x, zero, tol=NEST_TOL_INNER, krylovdim=30, maxiter=20, ws=ws_in, info=info)
        missed[0] += not info["converged"]
        return be.axpby(1.0, y, 0.0, out)
    lam, out, nmv, res = krylov.eigsolve_sr(be, mv, up(be, c["x0"]), tol=NEST_TOL_OUTER, krylovdim=30, maxiter=20)
    return dict(lam=float(lam), v=down(be, out), nmv=nmv, res=float(res), inner=count[0], unconverged=missed[0])


def check_nest(g, rho_host=None):
    """in terms of S itself: with mu = 1 / lam, rho = |S v - mu v| bounds |mu - lambda_max(S)| and the angle as for any
    symmetric pair.  Size of rho: S v - mu v = mu S (lam v - S^-1 v), so an outer residual of tol allows mu |S| tol"""
    c = nest_case()
    S, v = c["S"].astype(LD), g["v"].astype(LD)
    vn = np.sqrt((v * v).sum())
    mu = 1.0 / g["lam"]
    ew, V = np.linalg.eigh(c["S"])
    v0 = V[:, -1].astype(LD)
    v0 = v0 / np.sqrt((v0 * v0).sum())
    r_ref = nrm(S @ v0 - LD(ew[-1]) * v0)
    rho = nrm(S @ v - LD(mu) * v) / float(vn)
    sin = nrm(v / vn - ((v0 * v).sum() / vn) * v0)
    gap = float(np.min(np.abs(ew[:-1] - mu))) - r_ref
    assert np.isfinite(g["v"]).all() and int(np.argmin(np.abs(ew - mu))) == len(ew) - 1
    assert abs(mu - float(ew[-1])) <= rho + r_ref, (mu, ew[-1], rho)
    assert gap > 0 and sin <= (rho + r_ref) / gap, (sin, rho, gap)
    assert rho <= size_bar(mu * float(ew[-1]) * NEST_TOL_OUTER, rho_host), (rho, rho_host)
    return dict(rho=rho, lam_err=abs(g["lam"] - c["lam"]), sin=sin)


# ------------------------------------------------------------------------------------------------------------------
# exponentiate / exponentiate_general
# ------------------------------------------------------------------------------------------------------------------
EXPO = {
    "neg96": dict(n=96, z=-1.0, krylovdim=30),
    "neg257": dict(n=257, z=-1.0, krylovdim=30),
    "pos257": dict(n=257, z=0.5, krylovdim=30),
    "cut257": dict(n=257, z=-4.0, krylovdim=12),             # krylovdim exhausted: the step is cut into sub-steps
    "zero96": dict(n=96, z=-1.0, krylovdim=30),              # x0 = 0
    "eigvec96": dict(n=96, z=-1.0, krylovdim=30),            # x0 an eigenvector
}
EXPO_GENERAL = {
    "rot96": dict(n=96, a=0.0, b=1.0, krylovdim=30),         # a pure rotation
    "mixed96": dict(n=96, a=-0.5, b=1.0, krylovdim=30),
    "mixed257": dict(n=257, a=-0.5, b=1.0, krylovdim=30),
}


def _unit(x):
    return x / np.linalg.norm(x)


@functools.lru_cache(maxsize=None)
def expo_case(name):
    from scipy.linalg import expm
    if name in EXPO:
        c = dict(EXPO[name])
        n, rng = c["n"], _rng("expo-%d" % c["n"])
        A = from_spectrum(rng, np.linspace(-2.0, 2.0, n))
        x0 = _unit(rng.standard_normal(n))
        if name.startswith("zero"):
            x0 = np.zeros(n)
        if name.startswith("eigvec"):
            x0 = np.linalg.eigh(A)[1][:, 7].copy()
        M = c["z"] * A
    else:
        c = dict(EXPO_GENERAL[name])
        n, rng = c["n"], _rng("expog-%d" % c["n"])
        S, K = nonsym(rng, n, lo=-1.0, hi=1.0, skew=2.0)
        A = M = c["a"] * S + c["b"] * K
        x0 = _unit(rng.standard_normal(n))
    ref = expm(M).astype(LD) @ x0.astype(LD)
    c.update(name=name, A=A, x0=x0, ref=ref, tol=TOL, general=name in EXPO_GENERAL)
    return c


def run_expo(be, name):
    c = expo_case(name)
    mv, count = dense_op(be, c["A"])
    if c["general"]:
        y, nmv = krylov.exponentiate_general(be, mv, up(be, c["x0"]), tol=c["tol"], krylovdim=c["krylovdim"])
    else:
        y, nmv = krylov.exponentiate(be, mv, c["z"], up(be, c["x0"]), tol=c["tol"], krylovdim=c["krylovdim"])
    return dict(y=down(be, y), nmv=nmv, applied=count[0])


def check_expo(name, g, err_host=None):
    c = expo_case(name)
    err = nrm(g["y"].astype(LD) - c["ref"])
    assert np.isfinite(g["y"]).all(), name
    assert g["nmv"] == g["applied"], (name, g["nmv"], g["applied"])
    if err_host is not None:            # the host run itself is held to the relative bar below alone: the solver's estimate
        assert err <= size_bar(c["tol"], err_host), (name, err, err_host)      # is no bound, and sub-steps add their roundings
    assert float(np.abs(g["y"].astype(LD) - c["ref"]).max()) <= 1e-10 * float(np.abs(c["ref"]).max()), (name, err)
    return dict(err=err)


# ------------------------------------------------------------------------------------------------------------------
# non-symmetric eigenproblems: eigsolve_lm_real (Perron), arnoldi_eigvals and eigsolve_lm_planar (num = 3)
# ------------------------------------------------------------------------------------------------------------------
def _eig_cond(A):
    """(ew, right vectors, kappa = |y| |x| / |y^H x| per eigenvalue) of the dense matrix"""
    from scipy.linalg import eig
    ew, Yl, Xr = eig(A, left=True, right=True)
    kap = np.array([np.linalg.norm(Yl[:, j]) * np.linalg.norm(Xr[:, j]) / abs(np.vdot(Yl[:, j], Xr[:, j])) for j in range(len(ew))])
    return ew, Xr, kap


@functools.lru_cache(maxsize=None)
def perron_case(n):
    """D M D^-1 with M = Q diag(1, small) Q^T, q_0 = 1 / sqrt(n): positive entries (asserted), dominant eigenvalue 1 with
    the positive vector D 1, not normal"""
    rng = _rng("perron-%d" % n)
    Q = orthogonal(rng, n, first=np.ones(n))
    lam = np.r_[1.0, np.linspace(-0.3, 0.3, n - 1) / np.sqrt(n)]
    M = (Q * lam) @ Q.T
    d = np.exp(0.5 * rng.standard_normal(n))
    P = (M * (1.0 / d)) * d[:, None]
    ew, Xr, kap = _eig_cond(P)
    j = int(np.argmax(np.abs(ew)))
    x = Xr[:, j].real.astype(LD)
    x = x / np.sqrt((x * x).sum())
    r_ref = nrm(P.astype(LD) @ x - LD(ew[j].real) * x)
    return dict(name="perron%d" % n, n=n, A=P, x0=np.abs(rng.standard_normal(n)) + 0.1, lam=float(ew[j].real), kappa=float(kap[j]),
                r_ref=r_ref, second=float(np.sort(np.abs(ew))[-2]), tol=TOL)


def run_perron(be, n):
    c = perron_case(n)
    mv, count = dense_op(be, c["A"])
    lam, out = krylov.eigsolve_lm_real(be, mv, up(be, c["x0"]), tol=c["tol"], krylovdim=30, maxiter=100)
    return dict(lam=lam, v=down(be, out), applied=count[0])


def check_perron(n, g, r_host=None):
    c = perron_case(n)
    v = g["v"].astype(LD)
    vn = float(np.sqrt((v * v).sum()))
    r = nrm(c["A"].astype(LD) @ v - LD(g["lam"]) * v) / vn
    assert abs(vn - 1.0) <= norm_bar(c["n"])
    assert abs(g["lam"] - c["lam"]) <= c["kappa"] * (r + c["r_ref"]), (g["lam"], c["lam"], r)
    assert (g["v"] > 0).all() or (g["v"] < 0).all()
    assert r <= size_bar(c["tol"], r_host), (r, r_host)
    return dict(r=r, lam_err=abs(g["lam"] - c["lam"]))


PLANAR_N, PLANAR_TOL = 40, 1e-10


@functools.lru_cache(maxsize=None)
def pair_case():
    """D (Q B Q^T) D^-1, B = diag(2) + the rotation block 1.5 (cos, sin; -sin, cos)(0.9) + diag(|.| <= 0.5): the three
    largest eigenvalues by magnitude are 2 and 1.5 exp(+- 0.9 i)"""
    n, rng = PLANAR_N, _rng("pair")
    Q = orthogonal(rng, n)
    B = np.diag(np.r_[2.0, 0.0, 0.0, np.linspace(-0.5, 0.5, n - 3)])
    cph, sph = 1.5 * np.cos(0.9), 1.5 * np.sin(0.9)
    B[1:3, 1:3] = [[cph, sph], [-sph, cph]]
    d = np.exp(0.3 * rng.standard_normal(n))
    A = ((Q @ B @ Q.T) * (1.0 / d)) * d[:, None]
    ew, Xr, kap = _eig_cond(A)
    order = np.argsort(-np.abs(ew))[:3]
    r_ref = []
    for j in order:
        x = Xr[:, j].astype(CLD)
        x = x / np.sqrt((np.abs(x) ** 2).sum())
        r_ref.append(nrm(A.astype(CLD) @ x - CLD(ew[j]) * x))
    return dict(n=n, A=A, x0=rng.standard_normal(n), x0p=rng.standard_normal(2 * n), lam=ew[order], kappa=kap[order],
                r_ref=np.array(r_ref), fourth=float(np.sort(np.abs(ew))[-4]), tol=PLANAR_TOL)


def _match(vals, ref):
    """index into ref of the nearest reference eigenvalue for each value; must be a permutation"""
    idx = [int(np.argmin(np.abs(ref - v))) for v in vals]
    assert sorted(idx) == list(range(len(ref))), (vals, ref)
    return idx


def run_arnoldi(be):
    c = pair_case()
    mv, count = dense_op(be, c["A"])
    vals, conv = krylov.arnoldi_eigvals(be, mv, up(be, c["x0"]), num=3, tol=c["tol"], krylovdim=c["n"])
    return dict(vals=np.asarray(vals), conv=conv, applied=count[0])


def check_arnoldi(g, err_host=None):
    """eigenvalues only, so no residual can be formed: a Ritz residual below tol moves the value by kappa tol to first
    order, and the host run stands in for the rest, err <= max(kappa tol, 4 err_host)"""
    c = pair_case()
    assert g["conv"] == 3 and len(g["vals"]) == 3
    err = np.zeros(3)                                   # indexed as the reference eigenvalues
    for v, i in zip(g["vals"], _match(g["vals"], c["lam"])):
        err[i] = abs(v - c["lam"][i])
    bar = c["kappa"] * (c["tol"] + c["r_ref"])
    assert (err <= size_bar(bar, err_host)).all(), (err, bar, err_host)
    return dict(err=err)


def run_planar(be):
    c = pair_case()
    n = c["n"]
    Ad = be.upload(c["A"])
    count = [0]

    def mv(x, out):
        count[0] += 1
        return be.gemm(Ad, x.reshape(n, 2), out=out.reshape(n, 2))
    vals, vecs, res, conv = krylov.eigsolve_lm_planar(be, mv, be.upload(c["x0p"]), num=3, tol=c["tol"], krylovdim=30, maxiter=100)
    vs = [be.download(v).reshape(-1) for v in vecs]
    return dict(vals=np.asarray(vals), vecs=[v[:n] + 1j * v[n:] for v in vs], res=np.asarray(res), conv=conv, applied=count[0])


def check_planar(g, r_host=None):
    c = pair_case()
    assert g["conv"] == 3 and (g["res"] < c["tol"]).all(), g["res"]
    idx = _match(g["vals"], c["lam"])
    A = c["A"].astype(CLD)
    rs = np.zeros(3)                                    # indexed as the reference eigenvalues
    for v, th, i in zip(g["vecs"], g["vals"], idx):
        v = v.astype(CLD)
        vn = float(np.sqrt((np.abs(v) ** 2).sum()))
        rs[i] = nrm(A @ v - CLD(th) * v) / vn
        assert abs(vn - 1.0) <= norm_bar(2 * c["n"])
        assert abs(th - c["lam"][i]) <= c["kappa"][i] * (rs[i] + c["r_ref"][i]), (th, c["lam"][i], rs[i])
    assert (rs <= size_bar(c["tol"], r_host)).all(), (rs, r_host)
    return dict(r=rs)


# ------------------------------------------------------------------------------------------------------------------
# linsolve, complex
# ------------------------------------------------------------------------------------------------------------------
LIN_N = 40
LIN_A0, LIN_A1 = 0.08j - 0.02, 1.0 + 0.25j


def up_c(be, v):
    return be.upload_c(np.asarray(v, dtype=complex).reshape(-1, 1))


def down_c(be, t):
    return be.download_c(t).reshape(-1)


@functools.lru_cache(maxsize=None)
def linsolve_case():
    """(a0 + a1 A) x = b with A Hermitian, eigenvalues spread over [-1, 1]: the shifted spectrum is a segment that passes the
    origin at distance ~|Im(a0 conj(a1))| / |a1|, so full GMRES needs nearly all n = 40 steps -- more than the 32 vectors
    mpsk_vorth_step_c takes, which makes the device restart where the host stand-in (cycles of 40) does not"""
    n, rng = LIN_N, _rng("linsolve")
    G = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    Q, _ = np.linalg.qr(G)
    A = (Q * np.linspace(-1.0, 1.0, n)) @ Q.conj().T
    A = (A + A.conj().T) / 2
    M = LIN_A0 * np.eye(n) + LIN_A1 * A
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    x0 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    xd = np.linalg.solve(M, b)
    sv = np.linalg.svd(M, compute_uv=False)
    return dict(name="linsolve", n=n, op=A, A=M, b=b, x0=x0, xd=xd, inv_norm=float(1.0 / sv[-1]), cond=float(sv[0] / sv[-1]),
                r_ref=nrm(b.astype(CLD) - M.astype(CLD) @ xd.astype(CLD)), tol=TOL)


def run_linsolve(be):
    c = linsolve_case()
    Ad = be.upload_c(c["op"])
    x, info = krylov.linsolve(be, lambda x, out: be.gemm_c(Ad, x, out=out), up_c(be, c["b"]), up_c(be, c["x0"]), a0=LIN_A0, a1=LIN_A1,
                              tol=c["tol"], krylovdim=50, maxiter=100, cplx=True)
    return dict(x=down_c(be, x), info=info)


# the apply_axpby route: a prepared complex Jordan-form operator, D = 8, d = 2
HAC_D, HAC_d = 8, 2
HAC_A0 = 1.5 - 0.5j


@functools.lru_cache(maxsize=None)
def hac_case():
    """the complex twin of the spin-1/2 Heisenberg slice (its operator blocks turned by phases, identity corners real) between
    environments whose GL[0] and GR[W - 1] are identities, as MPSK_HAC_CANONICAL_C128 asks; the dense matrix of H_eff is
    the oracle's dAC applied to the unit vectors.  The system is (a0 + a1 H_eff) x = b with |a1 H_eff|_2 = 0.4 |a0|."""
    import mpskit_jl_amd as mk
    import mpskit_oracle as mo
    hb = host_backend()
    rng = _rng("hac")
    D, d = HAC_D, HAC_d
    Hr = mk.heisenberg_XXX(0.5, be=hb)[1]
    blocks = {k: (complex(v) if np.isscalar(v) else np.asarray(v) * np.exp(0.3j * (k[0] + 2 * k[1]))) for k, v in Hr.blocks.items()}
    W = Hr.Wl
    cr = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    GL = [np.eye(D, dtype=complex)[:, None, :] if w == 0 else cr(D, 1, D) / np.sqrt(D) for w in range(W)]
    GR = [np.eye(D, dtype=complex)[:, None, :] if w == W - 1 else cr(D, 1, D) / np.sqrt(D) for w in range(W)]
    sl = mo.SparseMPOSlice(Hr.odim, d, Hr.chil, Hr.chir, dict(blocks))
    n = D * d * D
    Hd = np.zeros((n, n), dtype=complex)
    for j in range(n):
        e = np.zeros(n, dtype=complex)
        e[j] = 1.0
        Hd[:, j] = np.ravel(mo.dAC(e.reshape((D, d, D), order="F"), sl, GL, GR), order="F")
    a1 = (0.8 + 0.6j) * 0.4 * abs(HAC_A0) / np.linalg.norm(Hd, 2)
    M = HAC_A0 * np.eye(n) + a1 * Hd
    b, x0 = cr(n), cr(n)
    xd = np.linalg.solve(M, b)
    sv = np.linalg.svd(M, compute_uv=False)
    return dict(name="hac", n=n, slice=(Hr.odim, d, tuple(Hr.chil), tuple(Hr.chir)), blocks=blocks, GL=GL, GR=GR, A=M, a0=HAC_A0, a1=a1,
                b=b, x0=x0, xd=xd, inv_norm=float(1.0 / sv[-1]), cond=float(sv[0] / sv[-1]),
                r_ref=nrm(b.astype(CLD) - M.astype(CLD) @ xd.astype(CLD)), tol=TOL)


def run_hac(be):
    c = hac_case()
    odim, d, chil, chir = c["slice"]
    H = be.mposlice(odim, d, list(chil), list(chir), dict(c["blocks"]), cplx=True)
    hac = be.hac_create_ex(H, be.upload_env_c(c["GL"]), be.upload_env_c(c["GR"]), canonical_c128=True)
    mode = hac.info()["mode"]
    D = HAC_D
    shp = lambda v: be.upload_c(np.asarray(v).reshape((D, d, D), order="F"))
    assert getattr(hac, "apply_axpby", None) is not None
    x, info = krylov.linsolve(be, hac, shp(c["b"]), shp(c["x0"]), a0=c["a0"], a1=c["a1"], tol=c["tol"], krylovdim=30, maxiter=100,
                              cplx=True)
    out = dict(x=np.ravel(be.download_c(x), order="F"), info=info, mode=mode)
    hac.close()
    return out
