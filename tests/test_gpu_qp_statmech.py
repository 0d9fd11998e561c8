"""excitations(H::DenseMPO | MPOMultiline, QuasiparticleAnsatz(), momentum, psi, envs) on the device: the one-particle band of
the square-lattice Ising row transfer matrix against Onsager's exact dispersion, the fused route against the composed one,
two rows against one, the reference's own six-vertex test (test/algorithms.jl:212-219) and the dense GEMM route on a
cluster tensor."""
import math

import numpy as np
import pytest

import mpskit_jl_amd as mk

pytestmark = pytest.mark.gpu

BETA = 0.3
ATOL = 1e-4                                    # the reference's quasiparticle gap test, test/algorithms.jl:209


def onsager(beta, p):
    """exp(-eps(p)), cosh eps(p) = cosh 2 beta coth 2 beta - cos p: the one-particle band of the row transfer matrix"""
    return math.exp(-math.acosh(math.cosh(2 * beta) / math.tanh(2 * beta) - math.cos(p)))


def boundary(be, O, D, n=1, d=2, seed=1, tol=1e-10, maxiter=200):
    psi = mk.InfiniteMPS.random(d, D, np.random.default_rng(seed), n=n, be=be)
    psi, envs, eps = mk.leading_boundary(psi, O, mk.VUMPS(tol=tol, maxiter=maxiter, verbosity=0))
    return psi, envs, eps


@pytest.fixture(scope="module")
def ising(be):
    O = mk.classical_ising(BETA)
    psi, envs, eps = boundary(be, O, 12)
    assert eps <= 1e-10, eps
    return O, psi, envs


@pytest.fixture(scope="module")
def lam0(be, ising):
    """the p = 0 eigenvalue of the one-row problem, shared by the tests that compare against it"""
    O, psi, envs = ising
    E, _ = mk.excitations(O, mk.QuasiparticleAnsatz(), 0.0, psi, envs)
    return E[0]


def test_dispersion_matches_onsager(be, ising):
    """|lambda(p)| = exp(-eps(p)) to 1e-4 at beta = 0.3, p in {0, pi/2, pi}, and |Im lambda| below the same bound.
    Deviations | |lambda| - exact | measured on an MI355X:
        D = 8 :  p = 0: 2.7e-12,  p = pi/2: 4.6e-14,  p = pi: 1.1e-13
        D = 12:  p = 0: 6.9e-13,  p = pi/2: 5.4e-14,  p = pi: 6.4e-15
    (the disordered phase at beta = 0.3 is far from critical: a boundary state of D = 8 already carries the band to the
    eigensolver's tolerance)."""
    O, psi, envs = ising
    ps = [0.0, math.pi / 2, math.pi]
    E, states = mk.excitations(O, mk.QuasiparticleAnsatz(), ps, psi, envs)
    assert E.shape == (3, 1) and len(states) == 3 and isinstance(states[0][0], mk.LeftGaugedQP)
    for p, e in zip(ps, E[:, 0]):
        dev = abs(abs(e) - onsager(BETA, p))
        print("p", p, "lambda", e, "exact", onsager(BETA, p), "deviation", dev)
        assert dev <= ATOL and abs(e.imag) <= ATOL


def test_routes_agree_and_fused_calls(be, ising):
    """device=True and device=False give the same eigenvalue to 10 x the eigensolver's tol, and the fused route runs
    mpsk_qp_half once per site and call, mpsk_qp_apply and both pair transfers (two-site cell, so that the pairs occur)."""
    O = mk.classical_ising(BETA)
    psi, envs, eps = boundary(be, O.repeat(2), 8, n=2)
    alg = mk.QuasiparticleAnsatz()
    before = dict(getattr(be, "qp_calls", {}))
    Ef, _ = mk.excitations(O.repeat(2), alg, 0.7, psi, envs, device=True)
    calls = {k: v - before.get(k, 0) for k, v in be.qp_calls.items()}
    print("fused calls", calls)
    assert calls["qp_half"] == 2 and calls["qp_apply"] > 0 and calls["transfer_left_pair"] > 0 and calls["transfer_right_pair"] > 0
    mid = dict(be.qp_calls)
    Ec, _ = mk.excitations(O.repeat(2), alg, 0.7, psi, envs, device=False)
    assert be.qp_calls == mid
    print("fused", Ef, "composed", Ec, "exact", onsager(BETA, 0.7))
    assert abs(Ef[0] - Ec[0]) <= 10 * alg.tol
    assert abs(abs(Ef[0]) - onsager(BETA, 0.7)) <= ATOL


def test_two_rows_match_one_row(be, ising, lam0):
    """MPOMultiline([O, O]) on two copies of the boundary state: the spectrum is the one-row spectrum times the square
    roots of unity, so the leading |mu| is the one-row |lambda| (both converged to tol = 1e-10): 1e-8."""
    O, psi, _ = ising
    H2, psi2 = mk.MPOMultiline([O, O]), mk.MPSMultiline([psi, psi])
    envs2 = mk.environments(psi2, H2)
    E, states = mk.excitations(H2, mk.QuasiparticleAnsatz(), 0.0, psi2, envs2)
    print("two rows", E, "one row", lam0)
    assert isinstance(states[0], mk.MultilineQP) and len(states[0]) == 2
    assert abs(abs(E[0]) - abs(lam0)) <= 1e-8


def test_sixvertex_reference_case(be):
    """test/algorithms.jl:212-219 "infinite (mpo)": the six-vertex band has its minimum at pi / 2."""
    H = mk.sixvertex().repeat(2)
    psi, envs, _ = boundary(be, H, 10, n=2, maxiter=400, tol=1e-8)
    E, _ = mk.excitations(H, mk.QuasiparticleAnsatz(), [0.0, math.pi / 2], psi, envs)
    print("six-vertex", E[:, 0])
    assert abs(E[0, 0]) > abs(E[1, 0])


def test_cluster_tensor_dense_route(be, lam0):
    """classical_ising(0.3, cluster=2) (chi = d = 4, the GEMM route of the dense slices): one row of 2 x 2 clusters is two
    rows of spins, so the p = 0 eigenvalue magnitude is the square of the one-site value: 1e-4."""
    O = mk.classical_ising(BETA, cluster=2)
    psi, envs, eps = boundary(be, O, 12, d=4)
    E, _ = mk.excitations(O, mk.QuasiparticleAnsatz(), 0.0, psi, envs)
    print("cluster", E, "one-site squared", abs(lam0) ** 2, "galerkin", eps)
    assert abs(abs(E[0]) - abs(lam0) ** 2) <= ATOL


def test_domain_walls_are_refused(be, ising):
    O, psi, envs = ising
    other = mk.InfiniteMPS.random(2, 12, np.random.default_rng(5), be=be)
    with pytest.raises(NotImplementedError, match="phase ambiguity"):
        mk.excitations(O, mk.QuasiparticleAnsatz(), 0.0, psi, envs, other)
