"""propagator / DynamicalDMRG (corvector.jl:23-204) on the NumPy stand-in backends (tests/cpu_backend.py): host logic
only, no GPU.  The stand-ins have none of the new entry points (mpsk_hac_apply_axpby, mpsk_v*_c, mpsk_vdiff_nrm2), so every
solve here takes the composed route of mpskit.jl_amd/krylov.py; tests/test_gpu_propagator.py repeats the full-bond case on
the device.  The dense answer is psi0^H solve(z - H, psi0) with H built by kron from the MPO blocks."""
import warnings

import numpy as np
import pytest

import mpskit_jl_amd as mk
from mpskit_jl_amd import krylov
from mpskit_jl_amd.native_cplx import NativeFiniteMPS
from cpu_backend import CpuBackend, CpuComplexBackend
from propagator_cases import dense_resolvent, dense_vector, excited_state, model, native_vector, omegas

ETA = 0.3


@pytest.fixture(scope="module")
def full_bond():
    """L = 6, bond dimensions min(2^i, 2^(L - i)): the centre tensor spans the whole space, the fixed point is exact"""
    be = CpuBackend()
    return {name: excited_state(be, name, 6, 8, 2) for name in ("tfi", "heisenberg")}


@pytest.mark.parametrize("name", ["tfi", "heisenberg"])
def test_full_bond_dimension_against_the_dense_resolvent(full_bond, name):
    ts, E0, Hd = full_bond[name]
    v = dense_vector(ts)
    rbe, cbe = CpuBackend(), CpuComplexBackend()
    psi_r, H_r = mk.FiniteMPS(ts, be=rbe), model(name, rbe)
    psi_c, H_c = mk.FiniteMPS(ts, be=cbe), model(name, cbe)
    for omega in omegas(E0):
        z = omega + 1j * ETA
        want = dense_resolvent(Hd, v, z)
        with warnings.catch_warnings():
            warnings.simplefilter("error")                       # every site solve converges here
            gj, _ = mk.propagator(psi_r, z, H_r, mk.DynamicalDMRG(flavour=mk.Jeckelmann(), tol=1e-8))
            gn, init = mk.propagator(psi_c, z, H_c, mk.DynamicalDMRG(flavour=mk.NaiveInvert(), tol=1e-8))
        print(name, f"omega = {omega:+.4f}: dense {want:.12f}  Jeckelmann err {abs(gj - want):.2e}  "
                    f"NaiveInvert err {abs(gn - want):.2e}  |J - N| {abs(gj - gn):.2e}")
        assert isinstance(gj, complex) and isinstance(gn, complex)
        assert isinstance(init, NativeFiniteMPS)                 # a real FiniteMPS start is converted
        assert abs(gj - want) <= 1e-8, (name, omega, gj, want)
        assert abs(gn - want) <= 1e-8, (name, omega, gn, want)
        assert abs(gj - gn) <= 1e-8, (name, omega, gj, gn)
        # the correction vector itself: (z - H)^-1 psi0
        x = np.linalg.solve(z * np.eye(len(v)) - Hd, v.astype(complex))
        assert np.abs(native_vector(init) - x).max() <= 1e-8


@pytest.mark.parametrize("flavour", ["naive", "jeckelmann"])
def test_truncated_chain_reaches_a_fixed_point(flavour):
    L, D = 10, 8
    be = CpuBackend() if flavour == "jeckelmann" else CpuComplexBackend()
    ts, E0, Hd = excited_state(CpuBackend(), "heisenberg", L, D, 4, sweeps=6)
    psi0, H = mk.FiniteMPS(ts, be=be), model("heisenberg", be)
    before = [t.copy() for t in psi0.to_host()]
    z = E0 + 0.5 + 1j * ETA
    fl = mk.Jeckelmann() if flavour == "jeckelmann" else mk.NaiveInvert()
    tol = 1e-8
    g, init = mk.propagator(psi0, z, H, mk.DynamicalDMRG(flavour=fl, tol=tol, maxiter=60))
    assert init.eps <= tol, init.eps
    g2, again = mk.propagator(psi0, z, H, mk.DynamicalDMRG(flavour=fl, tol=tol, maxiter=1), init=init)
    print(flavour, "value", g, "one more sweep: eps", again.eps, "value change", abs(g2 - g))
    assert again.eps <= tol, again.eps
    assert abs(g2 - g) <= 1e-7
    # init is not normalised: its norm carries the value
    nrm = again.norm() if flavour == "naive" else float(again.norm())
    assert abs(nrm - 1.0) > 1e-3, nrm
    # psi0 is left as it was
    after = psi0.to_host()
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    # D = 8 is a truncation: the value is close to the dense one, not equal to it
    want = dense_resolvent(Hd, dense_vector(ts), z)
    print(flavour, "dense", want, "err", abs(g - want))
    assert abs(g - want) <= 1e-2 * abs(want)


def _cvec(be, a):
    return be.upload_c(np.asarray(a, dtype=complex).reshape(-1, 1))


def _matrix_op(be, A):
    def op(x, out):
        return be._set_c(out, A @ be.download_c(x))
    return op


def test_linsolve_complex_shift_against_numpy():
    rng = np.random.default_rng(3)
    n = 40
    M = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    A = (M + M.conj().T) / np.sqrt(8 * n)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    x0 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    a0, a1 = -(0.4 + 0.3j), 1.0
    be = CpuComplexBackend()
    x, info = krylov.linsolve(be, _matrix_op(be, A), _cvec(be, b), _cvec(be, x0), a0=a0, a1=a1, tol=1e-12, krylovdim=30,
                              maxiter=100, cplx=True)
    want = np.linalg.solve(a0 * np.eye(n) + a1 * A, b)
    err = np.abs(be.download_c(x).reshape(-1) - want).max()
    print("linsolve: err", err, "normres", info.normres, "numops", info.numops)
    assert info.converged == 1 and info.normres <= 1e-12
    assert err <= 1e-10


def test_linsolve_builds_a_complex_krylov_space():
    """n = 8 complex unknowns, complex shift, complex start: the complex Krylov space is exhausted after 8 steps (one cycle),
    the real GMRES of the 16-dimensional embedding -- in which the shift is not a scalar -- needs more."""
    rng = np.random.default_rng(4)
    n = 8
    M = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    A = (M + M.conj().T) / 4
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    x0 = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    a0 = 0.2 + 0.7j
    want = np.linalg.solve(a0 * np.eye(n) + A, b)
    be = CpuComplexBackend()
    x, info = krylov.linsolve(be, _matrix_op(be, A), _cvec(be, b), _cvec(be, x0), a0=a0, a1=1.0, tol=1e-11, krylovdim=30,
                              maxiter=1, cplx=True)
    Hm = info.hessenberg
    assert np.iscomplexobj(Hm) and np.abs(Hm.imag).max() > 1e-3, Hm
    assert info.converged == 1 and info.numops <= n + 1
    assert np.abs(be.download_c(x).reshape(-1) - want).max() <= 1e-10
    # the same system as a REAL-linear operator on the 16 doubles
    xr, info_r = krylov.linsolve(be, _matrix_op(be, a0 * np.eye(n) + A), _cvec(be, b), _cvec(be, x0), tol=1e-11, krylovdim=30,
                                 maxiter=1, cplx=False)
    print("complex space:", info.numops, "applications; real embedding:", info_r.numops)
    assert not np.iscomplexobj(info_r.hessenberg)
    assert info_r.numops > info.numops


def test_linear_combination_is_linear():
    rng = np.random.default_rng(5)
    be = CpuBackend()
    n = 12
    A, B = rng.standard_normal((n, n)), rng.standard_normal((n, n))

    def mat(Mx):
        def op(x, out=None):
            out = be.empty(*x.shape) if out is None else out
            return be._set(out, (Mx @ be.download(x).reshape(-1)).reshape(x.shape))
        return op
    lc = mk.LinearCombination(be, (mat(A), mat(B)), (-2 * 0.7, 1.0))
    x, y = rng.standard_normal((n, 1)), rng.standard_normal((n, 1))
    al, bt = 0.3, -1.7
    lhs = be.download(lc(be.upload(al * x + bt * y)))
    rhs = al * be.download(lc(be.upload(x))) + bt * be.download(lc(be.upload(y)))
    assert np.abs(lhs - rhs).max() <= 1e-13
    assert np.abs(be.download(lc(be.upload(x))) - (-1.4 * A + B) @ x).max() <= 1e-13
    sh = be.download(lc.apply_axpby(0.5, be.upload(x), 2.0, be.empty(n, 1)))
    assert np.abs(sh - (2.0 * x + 0.5 * (-1.4 * A + B) @ x)).max() <= 1e-13


def test_jeckelmann_with_a_complex_state_is_not_implemented():
    cbe = CpuComplexBackend()
    rng = np.random.default_rng(6)
    H = model("tfi", cbe)
    ts = [rng.random(s) + 1j * rng.random(s) for s in ((1, 2, 2), (2, 2, 2), (2, 2, 1))]
    with pytest.raises(NotImplementedError):
        mk.propagator(NativeFiniteMPS(ts, cbe), 0.1 + 0.3j, H, mk.DynamicalDMRG(flavour=mk.Jeckelmann()))
    with pytest.raises(NotImplementedError):
        mk.propagator(mk.FiniteMPS(ts, be=cbe), 0.1 + 0.3j, H, mk.DynamicalDMRG(flavour=mk.Jeckelmann()))


@pytest.mark.parametrize("flavour", ["naive", "jeckelmann"])
def test_a_solve_that_does_not_converge_warns_and_returns(full_bond, flavour):
    ts, E0, _ = full_bond["tfi"]
    be = CpuBackend() if flavour == "jeckelmann" else CpuComplexBackend()
    fl = mk.Jeckelmann() if flavour == "jeckelmann" else mk.NaiveInvert()
    alg = mk.DynamicalDMRG(flavour=fl, solver=mk.GMRES(maxiter=1, krylovdim=2), tol=1e-8, maxiter=1)
    with pytest.warns(RuntimeWarning, match="failed to converge"):
        g, init = mk.propagator(mk.FiniteMPS(ts, be=be), E0 + 0.5 + 1j * ETA, model("tfi", be), alg)
    assert isinstance(g, complex) and np.isfinite(g.real) and np.isfinite(g.imag)


def test_defaults_are_those_of_the_reference():
    alg = mk.DynamicalDMRG()
    assert isinstance(alg.flavour, mk.NaiveInvert) and alg.tol == 1e-11 and alg.maxiter == 100 and alg.verbosity == 0
    assert (alg.solver.tol, alg.solver.maxiter, alg.solver.krylovdim) == (1e-12, 100, 30)


def test_complex_start_state_against_the_dense_resolvent():
    """a complex psi0 (NativeFiniteMPS) at full bond dimension: a spurious conjugation of psi0 in the overlap environments
    or in the value would show here"""
    from propagator_cases import dense_hamiltonian
    rng = np.random.default_rng(71)
    cbe = CpuComplexBackend()
    dims = [1, 2, 4, 8, 4, 2, 1]
    ts = [rng.standard_normal((dims[i], 2, dims[i + 1])) + 1j * rng.standard_normal((dims[i], 2, dims[i + 1])) for i in range(6)]
    psi0 = NativeFiniteMPS(ts, cbe)
    v = native_vector(psi0)
    H = model("heisenberg", cbe)
    Hd = dense_hamiltonian(H, 6)
    z = -0.7 + 0.3j
    g, init = mk.native_cplx.propagator(psi0, z, H, mk.DynamicalDMRG(tol=1e-8))
    x = np.linalg.solve(z * np.eye(64) - Hd, v)
    assert abs(g - complex(np.vdot(v, x))) <= 1e-8
    assert np.abs(native_vector(init) - x).max() <= 1e-8
    assert np.abs(x - np.linalg.solve(z * np.eye(64) - Hd, v.conj())).max() > 1e-2    # the vector check tells psi0 from conj(psi0)


def test_krylovdim_above_the_device_limit_is_clamped():
    """linsolve on a backend with orth_step_c never asks it for more than 32 basis vectors"""
    cbe = CpuComplexBackend()
    seen = []
    vs = krylov.ComplexVec(cbe)

    def orth_step_c(xs, y):
        seen.append(len(xs))
        del cbe.orth_step_c
        try:
            return vs.orth_step(xs, y)
        finally:
            cbe.orth_step_c = orth_step_c
    cbe.orth_step_c = orth_step_c
    rng = np.random.default_rng(8)
    n = 60
    M = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    A = (M + M.conj().T) / np.sqrt(8 * n)
    b = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    x, info = krylov.linsolve(cbe, _matrix_op(cbe, A), _cvec(cbe, b), _cvec(cbe, 0 * b), a0=2.0 + 0.5j, tol=1e-12, krylovdim=50,
                              maxiter=100, cplx=True)
    assert max(seen) <= 32 and info.converged == 1
    assert np.abs(cbe.download_c(x).reshape(-1) - np.linalg.solve((2.0 + 0.5j) * np.eye(n) + A, b)).max() <= 1e-10
