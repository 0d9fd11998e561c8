"""Cases for the Hamiltonian environments and the uniform drivers on interleaved complex storage
(mpskit_jl_amd.native_cplx.NativeMPOHamInfEnv, VUMPS and TDVP on a NativeInfiniteMPS).  The bodies take a backend:
tests/test_native_ham_inf_cpu.py runs them on the NumPy stand-in (tests/cpu_backend_ham_inf.py, composed route of the
regulariser) and records what it measured in profiles/native_ham_inf_bounds.log; tests/test_gpu_native_ham_inf.py runs them
on the device on both routes and reads its bounds from that file.

Sizes: d = 2, D = 8 and 12, unit cells of 1 and 2 sites.  References: the project's own real VUMPS (energies), the real
MPOHamInfEnv (environments), the embedded complex InfiniteMPS of cplx.py under mk.timestep (real-time TDVP)."""
import os

import numpy as np

import mpskit_jl_amd as mk
from mpskit_jl_amd import native_cplx as nc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUNDS_LOG = os.path.join(ROOT, "profiles", "native_ham_inf_bounds.log")

X = np.array([[0.0, 1.0], [1.0, 0.0]])
Y = np.array([[0.0, -1.0j], [1.0j, 0.0]])
Z = np.diag([1.0, -1.0])
G0, G1 = 0.7, 1.2                     # ground state of g = 0.7, quench to g = 1.2
VUMPS_TOL = 1e-7                      # Galerkin error asked of every VUMPS run here (the energy error is its square)
ENV_TOL = 1e-12                       # solver tolerance of both environment classes in the parity case
SIZES = [(1, 8), (2, 8), (1, 12)]     # (unit cell, D)
MARGIN = 100.0                        # the two GMRES take different Krylov paths to the same tolerance

_cache = {}


def tfi(be, g):
    return mk.transverse_field_ising(1.0, g, be=be)


def tfi_y(be, g):
    """TFI with the field rotated onto Y: Hermitian, not real; the spectrum of transverse_field_ising(1.0, g)"""
    return nc.ComplexMPOHamiltonian({(0, 0): 1, (0, 1): -Z, (1, 2): Z, (0, 2): -g * Y, (2, 2): 1}, be)


def real_groundstate(be, n, D, g=G0):
    """the project's real VUMPS on transverse_field_ising(g), computed once per (backend, n, D, g) and left unchanged"""
    key = (id(be), n, D, g)
    if key not in _cache:
        H = tfi(be, g)
        psi = mk.InfiniteMPS.random(2, D, np.random.default_rng(100 + n), n=n, be=be)
        psi, envs, eps = mk.find_groundstate(psi, H, mk.VUMPS(tol=VUMPS_TOL, maxiter=200))
        assert eps <= VUMPS_TOL, eps
        _cache[key] = (psi, H, float(np.sum(mk.expectation_value(psi, H, envs))) / n, eps)
    return _cache[key]


def levels_host(be, t, cplx):
    """the slabs of one level tensor as a host array [chi, D, D]"""
    chi, D1, D2 = t.shape[0], t.shape[1] // (2 if cplx else 1), t.shape[2]
    flat = t.buf[:t.size].cpu().numpy()
    flat = flat.view(np.complex128) if cplx else flat
    return np.stack([flat[w * D1 * D2:(w + 1) * D1 * D2].reshape((D1, D2), order="F") for w in range(chi)])


def env_difference(be, nat_env, real_env, n):
    """largest |native - real| / |real level| over levels, sites and sides, and the largest |Im native| / |real level|"""
    worst, imag = 0.0, 0.0
    for a, b in ((nat_env.lw, real_env.lw), (nat_env.rw, real_env.rw)):
        for i in range(len(a)):
            for s in range(n):
                x, y = levels_host(be, a[i][s], True), levels_host(be, b[i][s], False)
                nrm = np.linalg.norm(y)
                worst = max(worst, np.linalg.norm(x.real - y) / nrm)
                imag = max(imag, np.linalg.norm(x.imag) / nrm)
    return worst, imag


def case_env_parity(be, n, D, device=None):
    """NativeMPOHamInfEnv(from_real(psi), H) against MPOHamInfEnv(psi, H) on a converged real ground state.  Returns
    (difference of the real parts, imaginary part, the native environment), both relative to the level's norm."""
    psi, H, _, _ = real_groundstate(be, n, D)
    real_env = mk.MPOHamInfEnv(psi, H, tol=ENV_TOL)
    nat = nc.NativeInfiniteMPS.from_real(psi)
    nat_env = nc.NativeMPOHamInfEnv(nat, H, tol=ENV_TOL, device=device)
    assert nat_env.leftenv(0, nat).shape == (H.odim, 2 * D, D) and nat_env.rightenv(n - 1, nat).shape == (H.odim, 2 * D, D)
    assert nat_env.leftenv(0, nat) is nat_env.leftenv(n, nat)                   # assembled once, cached
    worst, imag = env_difference(be, nat_env, real_env, n)
    return worst, imag, nat_env


def route_difference(be, e1, e2, n):
    worst = 0.0
    for a, b in ((e1.lw, e2.lw), (e1.rw, e2.rw)):
        for i in range(len(a)):
            for s in range(n):
                x, y = levels_host(be, a[i][s], True), levels_host(be, b[i][s], True)
                worst = max(worst, np.linalg.norm(x - y) / np.linalg.norm(y))
    return worst


def case_vumps(be, n, D, complex_h, seed=5):
    """VUMPS from a random complex state on the Y-field Hamiltonian (complex_h) or on the real MPOHamiltonian.  Returns
    (energy per site, Galerkin error, reference energy per site, psi, envs)."""
    _, Hreal, E_ref, _ = real_groundstate(be, n, D)
    H = tfi_y(be, G0) if complex_h else Hreal
    psi0 = nc.NativeInfiniteMPS.random(2, D, np.random.default_rng(seed + n), n=n, be=be)
    psi, envs, eps = mk.find_groundstate(psi0, H, mk.VUMPS(tol=VUMPS_TOL, maxiter=200))
    assert isinstance(psi, nc.NativeInfiniteMPS) and isinstance(envs, nc.NativeMPOHamInfEnv)
    ens = mk.expectation_value(psi, H, envs)
    assert ens.dtype == np.complex128 and ens.shape == (n,)
    assert abs(mk.calc_galerkin(psi, envs) - eps) <= 1e-14
    return complex(np.sum(ens)) / n, eps, E_ref, psi, envs


def check_vumps(E, eps, E_ref):
    assert eps <= VUMPS_TOL, eps
    assert abs(E.real - E_ref) <= 1e-10 * abs(E_ref), (E, E_ref)
    assert abs(E.imag) <= 1e-12, E


def observables(be, psi, H, envs):
    """(energy per site, <X>, <Z>) averaged over the unit cell, of either representation"""
    n = len(psi)
    e = np.sum(mk.expectation_value(psi, H, envs)) / n
    loc = psi if isinstance(psi, nc.NativeInfiniteMPS) else nc.NativeInfiniteMPS.from_real(psi)    # the tensors as they are
    one = mk.expectation_value(loc, np.eye(2))       # |AC|^2: 1, or 1/2 for tensors extracted from the embedding
    x = np.sum(mk.expectation_value(loc, X) / one) / n
    z = np.sum(mk.expectation_value(loc, Z) / one) / n
    return np.array([complex(e).real, complex(x).real, complex(z).real])


def embedded_timestep(psi, H, t, dt, alg, envs):
    """tdvp.jl:21-59 on the embedded complex InfiniteMPS of cplx.py, from the package's own pieces (integrate with cplx=True,
    ddAC / ddC, regauge, from_AL): mk.timestep itself integrates a uniform state as a real one and refuses a real dt."""
    from mpskit_jl_amd import algorithms as al, krylov
    be, n = psi.be, len(psi)
    ws = krylov.KrylovWorkspace(be)
    newAL = []
    for loc in range(n):
        ac = al.integrate(be, mk.ddAC(loc, psi, H, envs), psi.AC[loc], t, dt, alg, ws, True)
        c = al.integrate(be, mk.ddC(loc, psi, H, envs), psi.CR[loc], t, dt, alg, ws, True)
        newAL.append(al.regauge(be, ac, c, True))
    psi2 = mk.InfiniteMPS.from_AL(newAL, psi.CR[n - 1], tol=alg.tolgauge, maxiter=alg.gaugemaxiter, be=be, cplx=True)
    envs.recalculate(psi2)
    return psi2, envs


def case_quench(be, n, D, steps=10, dt=0.05, device=None):
    """g = 0.7 ground state under the g = 1.2 Hamiltonian, `steps` TDVP steps on interleaved storage and on the embedded
    route.  Returns (largest difference of (E, <X>, <Z>) over the steps, largest | |dot| - 1 |, drift native, drift embedded)."""
    psi, _, _, _ = real_groundstate(be, n, D)
    H = tfi(be, G1)
    nat = nc.NativeInfiniteMPS.from_real(psi)
    emb = mk.InfiniteMPS.from_tensors([be.download(t).astype(np.complex128) for t in psi.AL], be=be)
    nenv = nc.NativeMPOHamInfEnv(nat, H, device=device)
    eenv = mk.environments(emb, H)
    alg = mk.TDVP()
    o_n0, o_e0 = observables(be, nat, H, nenv), observables(be, emb, H, eenv)
    d_obs, d_dot, drift_n, drift_e = float(np.abs(o_n0 - o_e0).max()), 0.0, 0.0, 0.0
    for k in range(steps):
        nat, nenv = mk.timestep(nat, H, k * dt, dt, alg, nenv)
        emb, eenv = embedded_timestep(emb, H, k * dt, dt, alg, eenv)
        o_n, o_e = observables(be, nat, H, nenv), observables(be, emb, H, eenv)
        d_obs = max(d_obs, float(np.abs(o_n - o_e).max()))
        d_dot = max(d_dot, abs(abs(nc.dot(nat, nc.NativeInfiniteMPS.from_real(emb))) - 1.0))
        drift_n, drift_e = max(drift_n, abs(o_n[0] - o_n0[0])), max(drift_e, abs(o_e[0] - o_e0[0]))
    return d_obs, d_dot, drift_n, drift_e


def case_stationary(be, n, D):
    """a converged ground state under its own Hamiltonian: <X> after 5 steps moves by no more than the Galerkin error"""
    E, eps, _, psi, envs = case_vumps(be, n, D, complex_h=False)
    H = envs.H
    x0 = np.sum(mk.expectation_value(psi, X)).real / n
    psi, envs = mk.time_evolve(psi, H, [0.05 * k for k in range(6)], mk.TDVP(), envs)
    x1 = np.sum(mk.expectation_value(psi, X)).real / n
    return abs(x1 - x0), eps


def case_imaginary_step(be, n, D):
    H = tfi_y(be, G0)
    psi = nc.NativeInfiniteMPS.random(2, D, np.random.default_rng(9), n=n, be=be)
    envs = mk.environments(psi, H)
    assert isinstance(envs, nc.NativeMPOHamInfEnv)
    e0 = np.sum(mk.expectation_value(psi, H, envs)).real / n
    psi, envs = mk.timestep(psi, H, 0.0, -0.05j, mk.TDVP(), envs)
    e1 = np.sum(mk.expectation_value(psi, H, envs)).real / n
    return e0, e1


def case_restart_after_bond_change(be):
    H = tfi_y(be, G0)
    psi = nc.NativeInfiniteMPS.random(2, 4, np.random.default_rng(3), be=be)
    envs = nc.NativeMPOHamInfEnv(psi, H)
    big = nc.NativeInfiniteMPS.random(2, 6, np.random.default_rng(4), be=be)
    envs.recalculate(big)
    assert envs.leftenv(0, big).shape == (3, 12, 6) and envs.rightenv(0, big).shape == (3, 12, 6)
    fresh = nc.NativeMPOHamInfEnv(big, H)
    e1, e2 = mk.expectation_value(big, H, envs), mk.expectation_value(big, H, fresh)
    assert abs(e1 - e2).max() <= 1e-10, (e1, e2)
    assert abs(e1.imag).max() <= 1e-12


def case_refusals(be):
    import pytest
    psi = nc.NativeInfiniteMPS.random(2, 4, np.random.default_rng(1), be=be)
    psi2 = nc.NativeInfiniteMPS.random(2, 4, np.random.default_rng(1), n=3, be=be)
    H = tfi(be, G0)
    with pytest.raises(NotImplementedError, match="LazySum"):
        nc.NativeMPOHamInfEnv(psi, mk.LazySum([H, H]))
    with pytest.raises(NotImplementedError, match="MultipliedOperator"):
        nc.NativeMPOHamInfEnv(psi, mk.MultipliedOperator(H, 2.0))
    with pytest.raises(NotImplementedError, match="MultipliedOperator"):
        mk.timestep(psi, mk.MultipliedOperator(H, lambda t: 1.0 + t), 0.0, 0.05, mk.TDVP())
    with pytest.raises(NotImplementedError, match="DenseMPO"):
        nc.NativeMPOHamInfEnv(psi, mk.classical_ising())
    with pytest.raises(NotImplementedError, match="MPOMultiline"):
        nc.NativeMPOHamInfEnv(psi, mk.MPOMultiline.__new__(mk.MPOMultiline))
    two = nc.ComplexMPOHamiltonian([{(0, 0): 1, (0, 1): -Z, (1, 2): Z, (0, 2): -G0 * Y, (2, 2): 1}] * 2, be)
    with pytest.raises(ValueError, match="multiple"):
        nc.NativeMPOHamInfEnv(psi2, two)
    for alg in (mk.GradientGrassmann(), mk.IDMRG1(), mk.IDMRG2()):
        with pytest.raises(NotImplementedError, match=type(alg).__name__):
            mk.find_groundstate(psi, H, alg)
    with pytest.raises(NotImplementedError, match="GradientGrassmann"):
        mk.find_groundstate(psi, H, tol=1e-8)
    with pytest.raises(NotImplementedError, match="TDVP2"):
        mk.timestep(psi, H, 0.0, 0.05, mk.TDVP2())
    with pytest.raises(NotImplementedError, match="changebonds"):
        mk.changebonds(psi, H, mk.OptimalExpand())
    with pytest.raises(NotImplementedError, match="leading_boundary"):
        mk.leading_boundary(psi, mk.classical_ising())
    with pytest.raises(NotImplementedError, match="excitations"):
        mk.excitations(H, mk.QuasiparticleAnsatz(), 0.0, psi)
    assert two.isid(0) and two.isid(2) and not two.isid(1)
    assert two.contains(1, 0, 2) and not two.contains(0, 1, 0) and two[1].blocks[(0, 2)].shape == (1, 2, 2, 1)


# ---- the bounds file ------------------------------------------------------------------------------------------------------

def write_bounds(records, lines):
    """records: {name: measured value}; the bound of each is MARGIN x the value"""
    with open(BOUNDS_LOG, "w") as f:
        f.write("# written by tests/test_native_ham_inf_cpu.py (NumPy stand-in, composed route); read by "
                "tests/test_gpu_native_ham_inf.py\n")
        f.write(f"# BOUND <name> <bound> = {MARGIN:g} x the largest difference measured on the host at the same solver "
                "tolerance\n")
        for text in lines:
            f.write("NATIVE-HAM-INF host " + text + "\n")
        for name in sorted(records):
            f.write(f"BOUND {name} {MARGIN * records[name]:.6e}\n")


def read_bounds():
    out = {}
    with open(BOUNDS_LOG) as f:
        for line in f:
            if line.startswith("BOUND "):
                _, name, val = line.split()
                out[name] = float(val)
    return out
