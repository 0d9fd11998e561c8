"""leading_boundary / DenseMPO / PerMPOInfEnv host logic on the host stand-in backend: the square-lattice Ising
partition function per site against Onsager's closed form (src/algorithms/statmech/vumps.jl, test/algorithms.jl:185-201)."""
import math

import numpy as np
import pytest

import mpskit_jl_amd as mk
from cpu_backend import CpuBackend, HostSlice

BETA_C = math.log(1.0 + math.sqrt(2.0)) / 2.0


class DenseCpuBackend(CpuBackend):
    """CpuBackend + mposlice_dense: a DenseMPO tensor as a one-level host slice (oracle arithmetic)."""

    def mposlice_dense(self, O):
        O = np.asarray(O)
        return HostSlice(1, O.shape[1], [O.shape[0]], [O.shape[3]], {(0, 0): O})


def onsager_kappa(beta):
    """Partition function per spin: ln k = ln(2 cosh 2b) + (1/2pi) int_0^pi ln[(1 + sqrt(1 - k^2 sin^2 t)) / 2] dt."""
    k = 2.0 * math.sinh(2.0 * beta) / math.cosh(2.0 * beta) ** 2
    x, w = np.polynomial.legendre.leggauss(400)
    th = (x + 1.0) * math.pi / 2.0
    integral = np.sum(w * np.log((1.0 + np.sqrt(1.0 - k * k * np.sin(th) ** 2)) / 2.0)) * math.pi / 2.0
    return math.exp(math.log(2.0 * math.cosh(2.0 * beta)) + integral / (2.0 * math.pi))


def _run(beta, cluster=1, D=6, n=1, tol=1e-9, seed=1):
    be = DenseCpuBackend()
    mpo = mk.classical_ising(beta, cluster)
    if n > 1:
        mpo = mpo.repeat(n)
    psi = mk.InfiniteMPS.random(mpo.d, D, np.random.default_rng(seed), n=n, be=be)
    psi, envs, eps = mk.leading_boundary(psi, mpo, mk.VUMPS(tol=tol, maxiter=200))
    return be, mpo, psi, envs, eps


def test_onsager_quadrature_sanity():
    assert onsager_kappa(BETA_C) == pytest.approx(2.5337, abs=1e-4)
    # high temperature: kappa -> 2 cosh(b)^2 (free spins with independent bonds) to leading order
    assert onsager_kappa(1e-4) == pytest.approx(2.0, rel=1e-6)


@pytest.mark.parametrize("cluster", [1, 2])
def test_disordered_matches_onsager(cluster):
    """beta = 0.3: kappa^(k^2) per k x k cluster tensor to 1e-10 relative at D = 6 (reached: ~2e-14)."""
    _, mpo, psi, envs, eps = _run(0.3, cluster=cluster, D=6)
    assert mpo[0].shape == (2 ** cluster,) * 4
    lam = mk.expectation_value(psi, mpo, envs)
    assert abs(lam[0] / onsager_kappa(0.3) ** (cluster * cluster) - 1.0) < 1e-10
    assert eps <= 1e-9


def test_ordered_matches_onsager():
    """beta = 0.6 (ordered): the boundary fixed point is nearly twofold degenerate (the two magnetised states), but the
    leading eigenvalue is not; D = 6 reaches ~1e-15 from this start, so the bar stays at 1e-10."""
    _, mpo, psi, envs, eps = _run(0.6, D=6)
    lam = mk.expectation_value(psi, mpo, envs)
    assert abs(lam[0] / onsager_kappa(0.6) - 1.0) < 1e-10
    assert eps <= 1e-9


def test_critical_ising_reference_value():
    """test/algorithms.jl:185-201: the critical classical Ising model gives 2.5337 +- 1e-3."""
    _, mpo, psi, envs, eps = _run(BETA_C, D=8, tol=1e-6)
    lam = mk.expectation_value(psi, mpo, envs)
    assert lam[0] == pytest.approx(2.5337, abs=1e-3)
    assert eps <= 1e-6


def test_two_site_unit_cell_same_per_site_value():
    _, mpo, psi, envs, eps = _run(0.3, D=6, n=2)
    lam = mk.expectation_value(psi, mpo, envs)
    assert len(mpo) == 2 and len(psi) == 2
    assert np.all(np.abs(lam / onsager_kappa(0.3) - 1.0) < 1e-10)


def test_environments_normalised_after_convergence():
    """Every column: dot(C, dC(GL[col + 1], GR[col]) C) = 1 (permpoinfenv.jl:180-187), and the environments are the
    transfer fixed points: GL[0] T = lambda GL[0] with the per-site value as lambda."""
    be, mpo, psi, envs, eps = _run(0.3, D=6, n=2)
    assert isinstance(envs, mk.PerMPOInfEnv)
    for col in range(len(psi)):
        c = psi.CR[col]
        val = be.dot(c, be.dC(envs.leftenv(col + 1, psi), envs.rightenv(col, psi), c))
        assert val == pytest.approx(1.0, abs=1e-12)
    gl = envs.leftenv(0, psi)
    t = gl
    for i in range(len(psi)):
        t = be.transfer_left(envs.O(i), t, psi.AL[i], psi.AL[i])
    a, b = be.download(t).ravel(), be.download(gl).ravel()
    ratio = a @ b / (b @ b)
    assert ratio == pytest.approx(onsager_kappa(0.3) ** 2, rel=1e-9)
    assert np.abs(a - ratio * b).max() <= 1e-8 * np.abs(a).max()
    assert mk.calc_galerkin(psi, envs) == pytest.approx(eps, rel=1e-6, abs=1e-12)


def test_recalculate_restarts_and_random_start():
    """recalculate keeps working from the previous fixed points (same bond spaces) and from random vectors (new ones)."""
    be, mpo, psi, envs, _ = _run(0.3, D=6)
    lam0 = mk.expectation_value(psi, mpo, envs)[0]
    envs.recalculate(psi, 1e-12)
    assert mk.expectation_value(psi, mpo, envs)[0] == pytest.approx(lam0, rel=1e-12)
    psi4 = mk.InfiniteMPS.random(2, 4, np.random.default_rng(3), be=be)
    envs.recalculate(psi4, 1e-12)
    assert envs.leftenv(0, psi4).shape == (2, 4, 4)
    fresh = mk.statmech.environments(psi4, mpo)
    assert mk.expectation_value(psi4, mpo, envs)[0] == pytest.approx(mk.expectation_value(psi4, mpo, fresh)[0], rel=1e-9)


def test_models_and_dense_mpo_container():
    mpo = mk.classical_ising(0.3, cluster=3)
    assert len(mpo) == 1 and mpo[5].shape == (8, 8, 8, 8) and mpo.d == 8
    assert len(mpo.repeat(3)) == 3
    # cluster tensors of k x k spins: the k = 2 tensor traced over its own bonds (torus of 2 x 2 spins with every
    # bond doubled) is the brute-force partition function of that torus
    o = mk.classical_ising(0.3, cluster=1)[0]
    o2 = mk.classical_ising(0.3, cluster=2)[0]
    tr2 = np.einsum("atta->", o2)
    brute = 0.0
    for cfg in range(16):
        s = [1 if cfg >> i & 1 else -1 for i in range(4)]          # s[r * 2 + c]
        e = 0.0
        for r in range(2):
            for c in range(2):
                e += s[r * 2 + c] * s[r * 2 + (c + 1) % 2] + s[r * 2 + c] * s[((r + 1) % 2) * 2 + c]
        brute += math.exp(0.3 * e)
    assert tr2 == pytest.approx(brute, rel=1e-12)
    assert np.einsum("atta->", o) == pytest.approx(2 * math.exp(0.6), rel=1e-12)  # one spin on a 1 x 1 torus
    sv = mk.sixvertex(1.0, 2.0, 3.0)[0]
    assert sv.shape == (2, 2, 2, 2)
    assert sv[0, 0, 0, 0] == 1.0 and sv[1, 0, 1, 0] == 2.0 and sv[1, 0, 0, 1] == 3.0
    with pytest.raises(NotImplementedError):
        mk.DenseMPO(np.ones((2, 2, 2, 2)) * 1j)


def test_sixvertex_leading_boundary_runs():
    """The six-vertex tensor (test/algorithms.jl:212-219) through the same driver: a converged boundary with a positive
    per-site eigenvalue."""
    be = DenseCpuBackend()
    mpo = mk.sixvertex()
    psi = mk.InfiniteMPS.random(2, 6, np.random.default_rng(2), be=be)
    psi, envs, eps = mk.leading_boundary(psi, mpo, mk.VUMPS(tol=1e-8, maxiter=300))
    lam = mk.expectation_value(psi, mpo, envs)[0]
    assert eps <= 1e-8 and lam > 0
