"""Shared checks of the Grassmann layer (not a test file): tests/test_grassmann_cpu.py runs them on the NumPy stand-in
backend (composed route), tests/test_gpu_grassmann.py on the device."""
import numpy as np

import mpskit_jl_amd as mk
from mpskit_jl_amd import grassmann as gm

EPS = np.finfo(float).eps


def random_site(be, Dl, d, Dr, seed):
    """a left-canonical site W (m x n) and three tangents at W, as device matrices; T2 is correlated with T1"""
    rng = np.random.default_rng(seed)
    m = Dl * d
    W, _ = np.linalg.qr(rng.standard_normal((m, Dr)))
    ts = []
    for _ in range(3):
        Z = rng.standard_normal((m, Dr))
        Z -= W @ (W.T @ Z)
        ts.append(Z / np.linalg.norm(Z))
    ts[1] = ts[0] + 0.5 * ts[1]
    return be.upload(W), [be.upload(t) for t in ts], W, ts


def check_geometry(be, Dl, d, Dr, route, alpha=0.3, tol=1e-13):
    Wd, Td, W, T = random_site(be, Dl, d, Dr, seed=Dl * 100 + d)
    n = Dr
    z = gm.PrecGrad(Td[2])
    Wn, Zn = gm.retract_site(be, Wd, z, alpha, route)
    Wn_h, Zn_h = be.download(Wn), be.download(Zn)
    assert np.abs(Wn_h.T @ Wn_h - np.eye(n)).max() <= tol
    assert np.abs(Wn_h.T @ Zn_h).max() <= tol
    nz = np.linalg.norm(T[2])
    assert abs(np.linalg.norm(Zn_h) - nz) <= tol * nz
    W0, Z0 = gm.retract_site(be, Wd, z, 0.0, route)
    assert np.abs(be.download(W0) - W).max() <= 1e-14
    assert np.abs(be.download(Z0) - T[2]).max() <= 1e-14
    t1 = be.download(gm.transport_site(be, Td[0], Wd, z, alpha, Wn, route))
    t2 = be.download(gm.transport_site(be, Td[1], Wd, z, alpha, Wn, route))
    ip = float(np.sum(T[0] * T[1]))
    assert abs(ip) > 0.5                                  # correlated on purpose: the bound below is relative to it
    assert abs(float(np.sum(t1 * t2)) - ip) <= tol * abs(ip)
    assert np.abs(Wn_h.T @ t1).max() <= tol


def check_galerkin_tie(psi, H, tol=1e-12):
    envs = mk.environments(psi, H)
    x = gm.ManifoldPoint(psi, envs)
    for i in range(len(psi)):
        ref = mk.calc_galerkin(psi, i, envs)
        got = x.gnorm[i] / x.hac_norm[i]
        m, n = x.g[i].shape
        if m == n:             # square isometry (edge of a finite chain): no complement, both are roundings of an exact 0
            assert got <= 100 * EPS and ref <= 100 * EPS, (i, got, ref)
        else:
            assert abs(got - ref) <= tol * ref, (i, got, ref)


def check_slope(be, psi, H):
    """central difference of f along the retraction against inner(x, g, eta), eta = -Pg, h = 1e-4, on a random (unconverged)
    uniform state: they agree to 1e-5 relative (truncation O(h^2), rounding ~ 1e-12 / |slope|, |slope| >= 1e-2 asserted)"""
    x = gm.ManifoldPoint(psi, mk.environments(psi, H))
    _, g = gm.fg(x)
    eta = gm.scale(be, g, -1.0)
    slope = gm.inner(x, g, eta)
    assert abs(slope) >= 1e-2
    h = 1e-4
    fd = (gm.retract(x, eta, h)[0].f - gm.retract(x, eta, -h)[0].f) / (2 * h)
    assert abs(fd - slope) <= 1e-5 * abs(slope), (fd, slope)


def energy(psi, H, envs):
    return float(np.sum(mk.expectation_value(psi, H, envs)))


def check_monotone(history):
    fs = [r[1] for r in history]
    assert len(fs) >= 2
    for a, b in zip(fs[:-1], fs[1:]):
        assert b <= a + 1e-13 * abs(a), (a, b)


def check_uniform_default(be, n, D, seed=0):
    """find_groundstate(psi, H, tol=1e-8) = VUMPS(1e-4) & GradientGrassmann(1e-8) against VUMPS(tol=1e-10), iTFI g = 2"""
    H = mk.transverse_field_ising(g=2.0, be=be)
    psi = mk.InfiniteMPS.random(2, D, np.random.default_rng(seed), n=n, be=be)
    p1, e1, _ = mk.find_groundstate(psi, H, mk.VUMPS(tol=1e-10))
    E1 = energy(p1, H, e1)
    p2, e2, eps = mk.find_groundstate(psi, H, tol=1e-8)
    assert [s[0] for s in e2.stages] == ["VUMPS", "GradientGrassmann"]
    hist = e2.stages[-1][1]
    assert eps == hist[-1][2] and eps <= 1e-8
    assert abs(energy(p2, H, e2) - E1) <= 1e-10
    check_monotone(hist)
    return hist


def check_finite_chain(be, route=None, L=10, D=6):
    """Heisenberg chain (L = 10, D = 6 is the reference's own test size): DMRG(1e-4) & GradientGrassmann(1e-8) against DMRG(tol=1e-10)"""
    H = mk.heisenberg_XXX(0.5, be=be)
    psi = mk.FiniteMPS.random(L, 2, D, np.random.default_rng(1), be=be)
    pa, ea, _ = mk.find_groundstate(psi, H, mk.DMRG(tol=1e-10))
    pb, eb, eps = mk.find_groundstate(psi, H, mk.DMRG(tol=1e-4) & mk.GradientGrassmann(tol=1e-8, route=route))
    assert [s[0] for s in eb.stages] == ["DMRG", "GradientGrassmann"]
    hist = eb.stages[-1][1]
    assert eps <= 1e-8
    assert abs(energy(pb, H, eb) - energy(pa, H, ea)) <= 1e-10
    check_monotone(hist)
    return hist
