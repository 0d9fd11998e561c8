"""Shared by tests/test_propagator_cpu.py and tests/test_gpu_propagator.py: the dense resolvent computed with NumPy (H built
by kron from the MPO blocks, psi0^H solve(z - H, psi0)) and the states of the propagator cases.  Not a test module."""
import numpy as np

import mpskit_jl_amd as mk


def dense_hamiltonian(H, n):
    """dense matrix of n sites of an MPOHamiltonian: left boundary level 0, right boundary level odim - 1"""
    dd = H.d
    cur = [None] * H.odim
    cur[0] = np.eye(1)
    for s in range(n):
        new = [None] * H.odim
        for (i, j), b in H[s].blocks.items():
            if cur[i] is None:
                continue
            m = b * np.eye(dd) if np.isscalar(b) else np.asarray(b)[0, :, :, 0]
            t = np.kron(cur[i], m)
            new[j] = t if new[j] is None else new[j] + t
        cur = new
    return cur[H.odim - 1]


def dense_vector(tensors):
    """the dense d^L vector of a list of host site tensors [Dl, d, Dr] (first site slowest, as kron orders it)"""
    v = np.ones((1, 1), dtype=np.result_type(*[t.dtype for t in tensors]))
    for T in tensors:
        v = np.tensordot(v, T, axes=([v.ndim - 1], [0]))
    return v.reshape(-1)


def model(name, be):
    if name == "tfi":
        return mk.transverse_field_ising(1.0, 0.7, be=be)
    return mk.heisenberg_XXX(0.5, be=be)


def excited_state(be, name, L, D, site, sweeps=10):
    """S^z at `site` (0-based) on the DMRG ground state of the model: (host tensors of S^z |gs>, E0, dense H).  `be` runs
    the ground-state search (real fp64)."""
    H = model(name, be)
    psi = mk.FiniteMPS.random(L, 2, D, np.random.default_rng(7), be=be)
    psi, envs, _ = mk.find_groundstate(psi, H, mk.DMRG(tol=1e-12, maxiter=sweeps))
    E0 = float(np.sum(mk.expectation_value(psi, H, envs)))
    ts = psi.to_host()
    Sz = np.diag([0.5, -0.5])
    ts[site] = np.einsum("ts,asb->atb", Sz, ts[site])
    return ts, E0, dense_hamiltonian(H, L)


def dense_resolvent(Hd, v, z):
    """<v| (z - H)^-1 |v>"""
    return complex(np.vdot(v, np.linalg.solve(z * np.eye(Hd.shape[0]) - Hd, v.astype(complex))))


def omegas(E0):
    """five frequencies around the ground-state energy"""
    return [E0 + w for w in (-1.0, -0.4, 0.0, 0.5, 1.2)]


def native_vector(init):
    """dense vector of a NativeFiniteMPS"""
    return dense_vector(init.to_host())
