"""Time-dependent TDVP on the host stand-in backend: a timed LazySum whose functions are constant gives the step of the
evaluated sum (the reference's own check and bound, test/algorithms.jl:118-157), and every generator is evaluated at the
reference's time (integrators.jl:20-25 inside tdvp.jl:61-91 / :113-146 / :21-59)."""
import numpy as np
import pytest

import mpskit_oracle as mo
import mpskit_jl_amd as mk
from cpu_backend import CpuBackend


@pytest.fixture()
def cb():
    return CpuBackend()


def _finite(cb, L=5, d=2, D=4, seed=1):
    rng = np.random.default_rng(seed)
    dims = mo.FiniteMPS.random(L, d, D, np.random.default_rng(0)).bond_dims()
    As = [rng.random((1 if i == 0 else dims[i - 1], d, dims[i])) for i in range(L)]
    return mk.FiniteMPS(As, normalize=True, be=cb)


def _energy(psi, H, envs=None):
    envs = mk.environments(psi, H) if envs is None else envs
    return float(np.sum(mk.expectation_value(psi, H, envs)))


def _timed_pair(cb):
    """the reference's construction: Ht = sum of TimedOperators with constant functions, so that Ht(t) is the same sum at
    every t (test/algorithms.jl:121-124)"""
    Ha, Hb = mk.transverse_field_ising(1.0, 0.0, be=cb), mk.transverse_field_ising(0.0, 0.5, be=cb)
    return mk.LazySum([Ha, Hb], [lambda t: 1.0, lambda t: 3.0])


@pytest.mark.parametrize("alg", [mk.TDVP(), mk.TDVP2(trunc_dim=4)], ids=["TDVP", "TDVP2"])
def test_finite_timed_step_equals_the_evaluated_step(cb, alg):
    Ht = _timed_pair(cb)
    psi0 = _finite(cb)
    dt = -0.1j
    pa, _ = mk.timestep(psi0, Ht, 1.0, dt, alg)
    pb, _ = mk.timestep(psi0, Ht(1.0), 0.0, dt, alg)
    Ea, Eb = _energy(pa, Ht(1.0)), _energy(pb, Ht(1.0))
    assert abs(Ea - Eb) <= 1e-8, (Ea, Eb)                    # the reference's bound (algorithms.jl:127)


def test_infinite_timed_step_equals_the_evaluated_step(cb):
    Ht = _timed_pair(cb)
    rng = np.random.default_rng(4)
    psi0 = mk.InfiniteMPS.from_tensors([rng.random((6, 2, 6)), rng.random((6, 2, 6))], be=cb)
    dt = -0.1j
    pa, ea = mk.timestep(psi0, Ht, 1.0, dt, mk.TDVP())
    pb, eb = mk.timestep(psi0, Ht(1.0), 0.0, dt, mk.TDVP())
    Ea, Eb = _energy(pa, Ht(1.0)), _energy(pb, Ht(1.0))
    assert abs(Ea - Eb) <= 1e-8, (Ea, Eb)                    # algorithms.jl:156


def _recorded(cb, t, dt, alg, psi0):
    """times at which the prefactor of a timed term is evaluated during one step, in call order, duplicates removed per visit"""
    seen = []

    def f(tt):
        seen.append(complex(tt))
        return 1.0

    Ht = mk.LazySum([mk.transverse_field_ising(1.0, 0.5, be=cb)], [f])
    mk.timestep(psi0, Ht, t, dt, alg)
    return seen


def test_finite_tdvp_evaluation_times(cb):
    """tdvp.jl:61-91: left-to-right AC at t + dt/4 and C at t - dt/4; right-to-left AC at t + 3dt/4 and C at t + dt/4.  A
    wrong time at any of the four places changes the recorded sequence."""
    L, t, dt = 4, 0.5, -0.2j
    seen = _recorded(cb, t, dt, mk.TDVP(), _finite(cb, L=L, D=4))
    lr = [t + dt / 4, t - dt / 4] * (L - 1) + [t + dt / 4]
    rl = [t + 3 * dt / 4, t + dt / 4] * (L - 1) + [t + 3 * dt / 4]
    assert len(seen) == len(lr + rl)
    assert np.abs(np.array(seen) - np.array(lr + rl)).max() < 1e-15
    assert len({t + dt / 4, t - dt / 4, t + 3 * dt / 4}) == 3


def test_finite_tdvp2_evaluation_times(cb):
    """tdvp.jl:113-146: forward AC2 at t + dt/4 and the backward AC step at t - dt/4; on the way back AC2 at t + 3dt/4 and
    AC at t + dt/4."""
    L, t, dt = 4, 0.5, -0.2j
    seen = _recorded(cb, t, dt, mk.TDVP2(trunc_dim=4), _finite(cb, L=L, D=4))
    lr = ([t + dt / 4, t - dt / 4] * (L - 1))[:-1]
    rl = ([t + 3 * dt / 4, t + dt / 4] * (L - 1))[:-1]
    assert len(seen) == len(lr + rl)
    assert np.abs(np.array(seen) - np.array(lr + rl)).max() < 1e-15


def test_infinite_tdvp_evaluation_times(cb):
    rng = np.random.default_rng(4)
    psi0 = mk.InfiniteMPS.from_tensors([rng.random((6, 2, 6)), rng.random((6, 2, 6))], be=cb)
    t, dt = 0.5, -0.2j
    seen = _recorded(cb, t, dt, mk.TDVP(), psi0)
    assert len(seen) == 4 and np.abs(np.array(seen) - (t + dt / 2)).max() < 1e-15


def test_varying_prefactor_changes_the_step(cb):
    """f(t) = 1 + Re t on a real-time-like argument: the step with the timed operator differs from the step with H(t0)
    frozen at the start time, and equals the step of the sum frozen at the single time a constant-in-time sweep would see
    only when f is constant."""
    Ha, Hb = mk.transverse_field_ising(1.0, 0.0, be=cb), mk.transverse_field_ising(0.0, 0.5, be=cb)
    Ht = mk.LazySum([Ha, Hb], [1.0, lambda t: 1.0 + 4.0 * np.imag(t) ** 2])
    psi0 = _finite(cb)
    pa, _ = mk.timestep(psi0, Ht, 0.0, -0.4j, mk.TDVP())
    pb, _ = mk.timestep(psi0, Ht(0.0), 0.0, -0.4j, mk.TDVP())
    Hm = mk.LazySum([Ha, Hb])
    assert abs(_energy(pa, Hm) - _energy(pb, Hm)) > 1e-6


# ---- a genuinely varying prefactor against the dense restatement (tests/timed_reference.py) ---------------------------------

def _full_bond_state(cb, seed=7, L=4, d=2):
    """complex state at full bond dimension (embedded storage): real-time steps keep the time argument of f real"""
    rng = np.random.default_rng(seed)
    dims = [1, 2, 4, 2, 1]
    As = [rng.standard_normal((dims[i], d, dims[i + 1])) + 1j * rng.standard_normal((dims[i], d, dims[i + 1])) for i in range(L)]
    return As, mk.FiniteMPS(As, normalize=True, be=cb)


def _vector(psi):
    import timed_reference as tr
    L = len(psi)
    return tr.mps_vector([psi.download(psi.AL(i)) if i < L - 1 else psi.download(psi.AC(L - 1)) for i in range(L)])


def _varying_case(cb):
    Ha, Hb = mk.transverse_field_ising(1.0, 0.0, be=cb), mk.transverse_field_ising(0.0, 0.5, be=cb)
    da, db = mo.dense_hamiltonian(mo.tfi_mpo(1.0, 0.0), 4), mo.dense_hamiltonian(mo.tfi_mpo(0.0, 0.5), 4)
    return (Ha, Hb), (da, db)


def test_varying_prefactor_matches_the_dense_restatement(cb):
    """f(t) = 1 + t, L = 4, d = 2, full bond, real time.  Tolerance: 10 x the deviation of the same comparison for a
    constant H through the plain-MPOHamiltonian path.  Measured on the stand-in backend: constant-H deviation 1.99e-15
    (bound 1.99e-14), timed-sum deviation 1.12e-14."""
    import timed_reference as tr
    (Ha, Hb), (da, db) = _varying_case(cb)
    As, psi0 = _full_bond_state(cb)
    t, dt = 0.3, 0.2
    Hc, dc = mk.transverse_field_ising(1.0, 0.5, be=cb), mo.dense_hamiltonian(mo.tfi_mpo(1.0, 0.5), 4)
    pc, _ = mk.timestep(psi0, Hc, t, dt, mk.TDVP())
    dev0 = np.abs(_vector(pc) - tr.tdvp_step_dense(As, [dc], [1.0], t, dt)).max()
    tol = 10 * dev0
    f = lambda s: 1.0 + s
    pt, _ = mk.timestep(psi0, mk.LazySum([Ha, Hb], [1.0, f]), t, dt, mk.TDVP())
    ref = tr.tdvp_step_dense(As, [da, db], [1.0, f], t, dt)
    dev = np.abs(_vector(pt) - ref).max()
    print(f"constant-H deviation {dev0:.3e}, bound {tol:.3e}, timed deviation {dev:.3e}")
    assert 0 < dev0 < 1e-12
    assert dev <= tol, (dev, tol)
    # each of the four evaluation times matters: f(t + dt/4), f(t - dt/4), f(t + 3dt/4) are distinct, and replacing any one
    # time by t breaks the agreement by more than the tolerance
    assert len({f(t + dt / 4), f(t - dt / 4), f(t + 3 * dt / 4)}) == 3
    for k in range(4):
        off = list(tr.OFFSETS)
        off[k] = 0.0
        wrong = tr.tdvp_step_dense(As, [da, db], [1.0, f], t, dt, offsets=tuple(off))
        assert np.abs(_vector(pt) - wrong).max() > tol, k


def test_varying_prefactor_tdvp2_matches_the_dense_restatement(cb):
    """the two-site scheme (tdvp.jl:113-146) at full bond, nothing truncated, against timed_reference.tdvp2_step_dense; bound
    and the one-wrong-time check as above.  Measured: constant-H deviation 3.48e-15 (bound 3.48e-14), timed deviation 2.22e-14."""
    import timed_reference as tr
    (Ha, Hb), (da, db) = _varying_case(cb)
    As, psi0 = _full_bond_state(cb, seed=8)
    t, dt = 0.3, 0.2
    alg = mk.TDVP2(trunc_dim=4)
    Hc, dc = mk.transverse_field_ising(1.0, 0.5, be=cb), mo.dense_hamiltonian(mo.tfi_mpo(1.0, 0.5), 4)
    pc, _ = mk.timestep(psi0, Hc, t, dt, alg)
    dev0 = np.abs(_vector(pc) - tr.tdvp2_step_dense(As, [dc], [1.0], t, dt)).max()
    tol = 10 * dev0
    f = lambda s: 1.0 + s
    pt, _ = mk.timestep(psi0, mk.LazySum([Ha, Hb], [1.0, f]), t, dt, alg)
    dev = np.abs(_vector(pt) - tr.tdvp2_step_dense(As, [da, db], [1.0, f], t, dt)).max()
    print(f"TDVP2: constant-H deviation {dev0:.3e}, bound {tol:.3e}, timed deviation {dev:.3e}")
    assert 0 < dev0 < 1e-12
    assert dev <= tol, (dev, tol)
    for k in range(4):
        off = list(tr.OFFSETS)
        off[k] = 0.0
        wrong = tr.tdvp2_step_dense(As, [da, db], [1.0, f], t, dt, offsets=tuple(off))
        assert np.abs(_vector(pt) - wrong).max() > tol, k
