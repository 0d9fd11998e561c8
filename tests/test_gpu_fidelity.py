"""fidelity_susceptibility on the device: the finite chain against the dense expression
chi_ab = <psi| V_a Q (H0 - E0)^-2 Q V_b |psi>, the fused route (mpsk_qp_heff_site, pair transfers) against the composed
one on a finite chain and on uniform states, and excitations(..., device=True) against the default route."""
import warnings

import numpy as np
import pytest

import mpskit_jl_amd as mk
from mpskit_jl_amd import susceptibility as sus
from mpskit_jl_amd.operators import spin_ops

pytestmark = pytest.mark.gpu


WEIGHTS = [1.0, -0.5, 0.25, 0.7, -0.3, 0.9]


def field(ops, be):
    """sum_i ops[i mod len(ops)] as a two-level MPOHamiltonian."""
    return mk.MPOHamiltonian([{(0, 0): 1.0, (1, 1): 1.0, (0, 1): o} for o in ops], be=be)


def site_op(o, i, L):
    d = o.shape[0]
    return np.kron(np.kron(np.eye(d ** i), o), np.eye(d ** (L - i - 1)))


def dense_heisenberg(L):
    Sz, Sp, Sm = spin_ops(0.5)
    H = np.zeros((2 ** L, 2 ** L))
    for i in range(L - 1):
        H += site_op(Sz, i, L) @ site_op(Sz, i + 1, L)
        H += 0.5 * (site_op(Sp, i, L) @ site_op(Sm, i + 1, L) + site_op(Sm, i, L) @ site_op(Sp, i + 1, L))
    return H


def dense_chi(H, Vs):
    """<psi| V_a Q (H - E0)^-2 Q V_b |psi> by full diagonalisation (non-degenerate ground state)."""
    ev, U = np.linalg.eigh(H)
    assert ev[1] - ev[0] > 1e-6
    psi = U[:, 0]
    cols = [(U[:, 1:].T @ (V @ psi)) / (ev[1:] - ev[0]) for V in Vs]
    return np.array([[a @ b for b in cols] for a in cols])


@pytest.fixture(scope="module")
def chain(be):
    """Heisenberg S = 1/2, L = 6 at full bond dimension; the staggered field, the uniform S^x field and an uneven field."""
    L = 6
    Sz, Sp, Sm = spin_ops(0.5)
    Sx = 0.5 * (Sp + Sm)
    H0 = mk.heisenberg_XXX(0.5, be=be)
    psi, envs, _ = mk.find_groundstate(mk.FiniteMPS.random(L, 2, 8, np.random.default_rng(0), be=be), H0,
                                       mk.DMRG(tol=1e-12, maxiter=40))
    # the uniform S^x field annihilates a singlet (its row and column of chi vanish); the third operator, a field of
    # uneven weights, overlaps with the staggered one, so that the off-diagonal of chi carries weight
    Vs = [field([Sz, -Sz], be), field([Sx], be), field([w * Sz for w in WEIGHTS], be)]
    dV = [sum((-1) ** i * site_op(Sz, i, L) for i in range(L)), sum(site_op(Sx, i, L) for i in range(L)),
          sum(WEIGHTS[i] * site_op(Sz, i, L) for i in range(L))]
    return psi, envs, H0, Vs, dense_chi(dense_heisenberg(L), dV)


def tfi_state(be, n):
    X = np.array([[0.0, 1], [1, 0]])
    Z = np.array([[1.0, 0], [0, -1]])
    H0 = mk.transverse_field_ising(1.0, 2.0, be=be)
    Vs = [field([-X], be), mk.MPOHamiltonian({(0, 0): 1.0, (2, 2): 1.0, (0, 1): -Z, (1, 2): Z}, be=be)]
    if n == 2:
        H0 = H0.repeat(2)
        Vs = [V.repeat(2) for V in Vs]
    psi, envs, eps = mk.find_groundstate(mk.InfiniteMPS.random(2, 12, np.random.default_rng(7), n=n, be=be), H0,
                                         mk.VUMPS(tol=1e-11, maxiter=200))
    print("TFI D=12 cell", n, "galerkin error", eps)     # both routes apply one operator to this state, converged or not
    return psi, envs, H0, Vs


def test_finite_chain_exact(be, chain):
    """At full bond dimension the 63 tangent directions span the complement of psi, so chi is the dense expression: 1e-8
    relative to max |chi| (GMRES stops at 1e-12; the margin covers the conditioning of (H0 - E0)^-1 on a six-site chain
    whose gap is of order 1).  A right-hand side from H0's slice between V's environments cannot pass this."""
    psi, envs, H0, Vs, ref = chain
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        chi = mk.fidelity_susceptibility(psi, H0, Vs, envs)
    err = np.abs(chi - ref).max() / np.abs(ref).max()
    print("finite L=6: chi", chi.tolist(), "dense", ref.tolist(), "relative error", err)
    assert ref[0, 0] > 1e-2 and abs(ref[0, 2]) > 1e-2 and ref[2, 2] > 1e-2
    assert err < 1e-8
    assert np.abs(chi - chi.T).max() <= 1e-12 * np.abs(chi).max()
    assert np.linalg.eigvalsh(0.5 * (chi + chi.T)).min() > -1e-12 * np.abs(chi).max()


def check_routes(be, psi, envs, H0, Vs, what):
    """chi of the two routes to 1e-9 relative; the residual of each route's solutions below 1e-10, evaluated through
    effective_excitation_hamiltonian on the OTHER route.  A right-hand side that vanishes by symmetry (|T| < 1e-12: the
    uniform field on a singlet) has no relative residual; there the absolute one is held to the same figure."""
    sols = {}
    for dev in (True, False):
        calls = be.__dict__.get("qp_calls", {}).get("qp_heff_site", 0)
        sols[dev] = sus.tangent_vectors(psi, H0, Vs, envs, device=dev)
        used = be.__dict__.get("qp_calls", {}).get("qp_heff_site", 0) - calls
        assert (used > 0) == dev, (dev, used)
    chi = {dev: mk.fidelity_susceptibility(psi, H0, Vs, envs, device=dev) for dev in (True, False)}
    gram = np.array([[mk.qp_dot(a, b) for b in sols[True][0]] for a in sols[True][0]])
    assert np.abs(gram - chi[True]).max() <= 1e-12 * np.abs(chi[True]).max()
    err = np.abs(chi[True] - chi[False]).max() / np.abs(chi[False]).max()
    print(what, "chi fused", chi[True].tolist(), "composed", chi[False].tolist(), "relative difference", err)
    assert err < 1e-9
    for dev in (True, False):
        for x, T in zip(*sols[dev]):
            r = mk.effective_excitation_hamiltonian(H0, x, envs, device=not dev)
            be.axpby(-1.0, T.vec, 1.0, r.vec)
            nr, nT = be.norm(r.vec), be.norm(T.vec)
            print(what, "route", "fused" if dev else "composed", "|H x - T|", nr, "|T|", nT)
            assert nr < 1e-10 * (nT if nT >= 1e-12 else 1.0)


def test_routes_agree_finite(be, chain):
    psi, envs, H0, Vs, _ = chain
    check_routes(be, psi, envs, H0, Vs, "finite L=6")


@pytest.mark.parametrize("n", [1, 2])
def test_routes_agree_infinite(be, n):
    """Uniform transverse-field Ising ground state (g = 2, D = 12), Vs = [field term, coupling term]."""
    psi, envs, H0, Vs = tfi_state(be, n)
    check_routes(be, psi, envs, H0, Vs, f"TFI D=12 cell {n}")


def test_excitations_device_route(be):
    """excitations(..., device=True) reproduces the energy of the default route: S = 1 Heisenberg at D = 12, momentum pi
    (a state of a few VUMPS sweeps, not the converged Haldane gap: both routes apply the same operator to it)."""
    H = mk.heisenberg_XXX(1.0, be=be)
    psi, envs, _ = mk.find_groundstate(mk.InfiniteMPS.random(3, 12, np.random.default_rng(3), be=be), H,
                                       mk.VUMPS(tol=1e-8, maxiter=60))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        e0, _ = mk.excitations(H, mk.QuasiparticleAnsatz(), float(np.pi), psi, envs)
        calls = be.__dict__.get("qp_calls", {}).get("qp_heff_site", 0)
        e1, _ = mk.excitations(H, mk.QuasiparticleAnsatz(), float(np.pi), psi, envs, device=True)
    assert be.qp_calls.get("qp_heff_site", 0) > calls
    print("S=1 D=12 p=pi: default", e0[0], "device", e1[0], "difference", abs(e0[0] - e1[0]))
    assert abs(e0[0] - e1[0]) < 1e-9
