"""Time-dependent TDVP on the device: the reference's own check (a timed sum with constant functions steps like the
evaluated sum, test/algorithms.jl:118-157, bound 1e-8), the device-side sum (mpsk_hsum) against the composed route on the
same state, and the route the finite / infinite cases really take."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import mpskit_oracle as mo
import timed_reference as tr

# Tolerances are measured inside each test: 10 x the deviation that the same comparison shows for a CONSTANT Hamiltonian on
# the paths that existed before the timed ones (a plain MPOHamiltonian step against the dense restatement; for the
# energy comparisons, a plain MPOHamiltonian step against the step of the untimed LazySum with the same total).
# Measured on an MI355X: the figures beside the assertions.


def _ham(be):
    import mpskit_jl_amd as mk
    Ha, Hb, Hc = (mk.transverse_field_ising(1.0, 0.0, be=be), mk.transverse_field_ising(0.0, 0.5, be=be),
                  mk.heisenberg_XXX(0.5, be=be))
    return Ha, Hb, Hc


def _energy(psi, H):
    import mpskit_jl_amd as mk
    return float(np.sum(mk.expectation_value(psi, H, mk.environments(psi, H))))


def _constant_energy_deviation(psi0, alg, be):
    """the paths from before the timed ones on a constant H: one step with the plain TFI MPOHamiltonian against the same step
    with the untimed LazySum of its two parts; the energy difference is the rounding scale of a sum-against-single comparison"""
    import mpskit_jl_amd as mk
    Hfull = mk.transverse_field_ising(1.0, 0.5, be=be)
    Hsum = mk.LazySum([mk.transverse_field_ising(1.0, 0.0, be=be), mk.transverse_field_ising(0.0, 0.5, be=be)])
    p1, _ = mk.timestep(psi0, Hfull, 0.0, -0.4j, alg)
    p2, _ = mk.timestep(psi0, Hsum, 0.0, -0.4j, alg)
    dev = abs(_energy(p1, Hfull) - _energy(p2, Hfull))
    assert 0 < dev < 1e-10, dev
    return dev


def _spy_routes(monkeypatch):
    from mpskit_jl_amd import derivatives
    routes = []
    orig = derivatives.TimedDerivativeSum.at

    def at(self, t=None):
        op = orig(self, t)
        info = self.info()
        routes.append(None if info is None else info["route"])
        return op
    monkeypatch.setattr(derivatives.TimedDerivativeSum, "at", at)
    return routes


@pytest.mark.parametrize("algname", ["TDVP", "TDVP2"])
def test_finite_timed_step(be, monkeypatch, algname):
    import mpskit_jl_amd as mk
    Ha, Hb, Hc = _ham(be)
    alg = mk.TDVP() if algname == "TDVP" else mk.TDVP2(trunc_dim=8)
    psi0 = mk.FiniteMPS.random(6, 2, 8, np.random.default_rng(2), normalize=True, be=be)
    const = mk.LazySum([Ha, Hb, Hc], [lambda t: 1.0, lambda t: 3.0, lambda t: 0.5])
    dt = -0.1j
    routes = _spy_routes(monkeypatch)
    pa, _ = mk.timestep(psi0, const, 1.0, dt, alg)
    seen = set(routes)
    pb, _ = mk.timestep(psi0, const(1.0), 0.0, dt, alg)
    H1 = const(1.0)
    assert abs(_energy(pa, H1) - _energy(pb, H1)) <= 1e-8                  # algorithms.jl:127
    # every one-site generator of the timed step ran the folded route; the two-site and bond generators are composed
    assert 1 in seen and 2 not in seen, seen
    # a genuinely varying prefactor: device sum against the composed sum
    vary = mk.LazySum([Ha, Hb, Hc], [1.0, lambda t: 1.0 + 4.0 * np.imag(t) ** 2, lambda t: np.cos(np.imag(t))])
    pd, _ = mk.timestep(psi0, vary, 0.0, -0.4j, alg)
    monkeypatch.setenv("MPSK_HSUM", "0")
    del routes[:]
    pc, _ = mk.timestep(psi0, vary, 0.0, -0.4j, alg)
    assert set(routes) == {None}
    Hm = mk.LazySum([Ha, Hb, Hc])
    Ed, Ec = _energy(pd, Hm), _energy(pc, Hm)
    monkeypatch.delenv("MPSK_HSUM")
    tol = 10 * _constant_energy_deviation(psi0, alg, be)
    print(f"device sum / composed sum energies {Ed} {Ec}: difference {abs(Ed - Ec):.3e}, bound {tol:.3e}")
    assert abs(Ed - Ec) <= tol                      # measured: differences 4.0e-15 / 2.7e-15, bounds 6.2e-14 / 5.3e-14


def test_infinite_timed_step(be, monkeypatch):
    import mpskit_jl_amd as mk
    Ha, Hb, _ = _ham(be)
    rng = np.random.default_rng(4)
    psi0 = mk.InfiniteMPS.from_tensors([rng.random((8, 2, 8)), rng.random((8, 2, 8))], be=be)
    const = mk.LazySum([Ha, Hb], [lambda t: 1.0, lambda t: 3.0])
    dt = -0.1j
    routes = _spy_routes(monkeypatch)
    pa, _ = mk.timestep(psi0, const, 1.0, dt, mk.TDVP())
    assert 2 in set(routes) and 1 not in set(routes), routes             # infinite environments: the accumulated route
    pb, _ = mk.timestep(psi0, const(1.0), 0.0, dt, mk.TDVP())
    H1 = const(1.0)
    assert abs(_energy(pa, H1) - _energy(pb, H1)) <= 1e-8                  # algorithms.jl:156
    vary = mk.LazySum([Ha, Hb], [1.0, lambda t: 1.0 + 4.0 * np.imag(t) ** 2])
    pd, _ = mk.timestep(psi0, vary, 0.0, -0.4j, mk.TDVP())
    monkeypatch.setenv("MPSK_HSUM", "0")
    pc, _ = mk.timestep(psi0, vary, 0.0, -0.4j, mk.TDVP())
    Hm = mk.LazySum([Ha, Hb])
    Ed, Ec = _energy(pd, Hm), _energy(pc, Hm)
    monkeypatch.delenv("MPSK_HSUM")
    tol = 10 * _constant_energy_deviation(psi0, mk.TDVP(), be)
    print(f"device sum / composed sum energies {Ed} {Ec}: difference {abs(Ed - Ec):.3e}, bound {tol:.3e}")
    assert abs(Ed - Ec) <= tol                      # measured: difference 2.0e-15, bound 3.8e-14


# ---- a genuinely varying prefactor against the dense restatement (tests/timed_reference.py) ---------------------------------

L6, DIMS6 = 6, [1, 2, 4, 8, 4, 2, 1]
T0, DT = 0.3, 0.2
F = lambda s: 1.0 + s


def _tensors(seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((DIMS6[i], 2, DIMS6[i + 1])) + 1j * rng.standard_normal((DIMS6[i], 2, DIMS6[i + 1]))
            for i in range(L6)]


def _dense_parts():
    return (mo.dense_hamiltonian(mo.tfi_mpo(1.0, 0.0), L6), mo.dense_hamiltonian(mo.tfi_mpo(0.0, 0.5), L6),
            mo.dense_hamiltonian(mo.tfi_mpo(1.0, 0.5), L6))


def _embedded_vector(psi):
    L = len(psi)
    return tr.mps_vector([psi.download(psi.AL(i)) if i < L - 1 else psi.download(psi.AC(L - 1)) for i in range(L)])


def test_embedded_complex_finite_against_dense(be, monkeypatch):
    """FiniteMPS on embedded complex storage, real time, f(t) = 1 + t, L = 6 at full bond (D = 8): accumulated device sum."""
    import mpskit_jl_amd as mk
    Ha, Hb, _ = _ham(be)
    da, db, dc = _dense_parts()
    As = _tensors(11)
    psi0 = mk.FiniteMPS(As, normalize=True, be=be)
    pc, _ = mk.timestep(psi0, mk.transverse_field_ising(1.0, 0.5, be=be), T0, DT, mk.TDVP())
    dev0 = np.abs(_embedded_vector(pc) - tr.tdvp_step_dense(As, [dc], [1.0], T0, DT)).max()
    routes = _spy_routes(monkeypatch)
    pt, _ = mk.timestep(psi0, mk.LazySum([Ha, Hb], [1.0, F]), T0, DT, mk.TDVP())
    assert 2 in set(routes) and 1 not in set(routes), set(routes)
    dev = np.abs(_embedded_vector(pt) - tr.tdvp_step_dense(As, [da, db], [1.0, F], T0, DT)).max()
    print(f"embedded: constant-H deviation {dev0:.3e}, bound {10 * dev0:.3e}, timed deviation {dev:.3e}")
    assert 0 < dev0 < 1e-11
    assert dev <= 10 * dev0, (dev, dev0)         # measured: constant-H 1.73e-14 (bound 1.73e-13), timed 9.17e-14


def test_native_finite_tdvp_against_dense(be):
    """NativeFiniteMPS, real time, f(t) = 1 + t, L = 6 at full bond (D = 8): the folded route (MPSK_HAC_CANONICAL_C128)."""
    import mpskit_jl_amd as mk
    from mpskit_jl_amd import native_cplx as nc
    Ha, Hb, _ = _ham(be)
    da, db, dc = _dense_parts()
    As = _tensors(12)
    pc = nc.NativeFiniteMPS(As, be)
    nc.timestep(pc, mk.transverse_field_ising(1.0, 0.5, be=be), T0, DT, mk.TDVP())
    dev0 = np.abs(tr.mps_vector(pc.to_host()) - tr.tdvp_step_dense(As, [dc], [1.0], T0, DT)).max()
    pt = nc.NativeFiniteMPS(As, be)
    _, envs = nc.timestep(pt, mk.LazySum([Ha, Hb], [1.0, F]), T0, DT, mk.TDVP())
    assert isinstance(envs, nc.NativeMultipleEnv) and envs.routes == {1}, envs.routes
    dev = np.abs(tr.mps_vector(pt.to_host()) - tr.tdvp_step_dense(As, [da, db], [1.0, F], T0, DT)).max()
    print(f"native: constant-H deviation {dev0:.3e}, bound {10 * dev0:.3e}, timed deviation {dev:.3e}")
    assert 0 < dev0 < 1e-11
    assert dev <= 10 * dev0, (dev, dev0)         # measured: constant-H 1.55e-14 (bound 1.55e-13), timed 6.64e-14
    # the timed constant sum steps like the evaluated one
    pa, pb = nc.NativeFiniteMPS(As, be), nc.NativeFiniteMPS(As, be)
    const = mk.LazySum([Ha, Hb], [lambda s: 1.0, lambda s: 3.0])
    _, ea = nc.timestep(pa, const, 1.0, DT, mk.TDVP())
    _, eb = nc.timestep(pb, const(1.0), 0.0, DT, mk.TDVP())
    assert abs(nc.energy(pa, ea, 1.0) - nc.energy(pb, eb)) <= 1e-8           # algorithms.jl:127


def test_native_finite_tdvp2_against_dense(be, monkeypatch):
    """TDVP2 on a NativeFiniteMPS, real time, f(t) = 1 + t, L = 6 at full bond (D = 8, nothing truncated), against the dense
    two-site restatement (timed_reference.tdvp2_step_dense).  Replacing any one of the four evaluation times of the
    restatement by t breaks the agreement, so a wrong time in the driver cannot pass."""
    import mpskit_jl_amd as mk
    from mpskit_jl_amd import native_cplx as nc
    Ha, Hb, _ = _ham(be)
    da, db, dc = _dense_parts()
    As = _tensors(13)
    alg = mk.TDVP2(trunc_dim=8)
    pc = nc.NativeFiniteMPS(As, be)
    nc.timestep(pc, mk.transverse_field_ising(1.0, 0.5, be=be), T0, DT, alg)
    dev0 = np.abs(tr.mps_vector(pc.to_host()) - tr.tdvp2_step_dense(As, [dc], [1.0], T0, DT)).max()
    tol = 10 * dev0
    pt = nc.NativeFiniteMPS(As, be)
    _, envs = nc.timestep(pt, mk.LazySum([Ha, Hb], [1.0, F]), T0, DT, alg)
    assert envs.routes == {1}, envs.routes
    vt = tr.mps_vector(pt.to_host())
    dev = np.abs(vt - tr.tdvp2_step_dense(As, [da, db], [1.0, F], T0, DT)).max()
    print(f"native TDVP2: constant-H deviation {dev0:.3e}, bound {tol:.3e}, timed deviation {dev:.3e}")
    assert 0 < dev0 < 1e-11
    assert dev <= tol, (dev, tol)                 # measured: constant-H 3.70e-14 (bound 3.70e-13), timed 1.15e-13
    for k in range(4):
        off = list(tr.OFFSETS)
        off[k] = 0.0
        wrong = tr.tdvp2_step_dense(As, [da, db], [1.0, F], T0, DT, offsets=tuple(off))
        assert np.abs(vt - wrong).max() > tol, k
    # the term-by-term route of the same step
    monkeypatch.setenv("MPSK_HSUM", "0")
    pq = nc.NativeFiniteMPS(As, be)
    _, eq = nc.timestep(pq, mk.LazySum([Ha, Hb], [1.0, F]), T0, DT, alg)
    assert eq.routes == set()
    assert np.abs(tr.mps_vector(pq.to_host()) - tr.tdvp2_step_dense(As, [da, db], [1.0, F], T0, DT)).max() <= tol
    monkeypatch.delenv("MPSK_HSUM")
    # the timed constant sum steps like the evaluated one
    pa, pb = nc.NativeFiniteMPS(As, be), nc.NativeFiniteMPS(As, be)
    const = mk.LazySum([Ha, Hb], [lambda s: 1.0, lambda s: 3.0])
    _, ea = nc.timestep(pa, const, 1.0, DT, alg)
    _, eb = nc.timestep(pb, const(1.0), 0.0, DT, alg)
    assert abs(nc.energy(pa, ea, 1.0) - nc.energy(pb, eb)) <= 1e-8           # algorithms.jl:127


def _captured_inf_step(be, monkeypatch, psi0, H, t, dt):
    """one infinite TDVP step through the real driver; returns what it handed to regauge: [(ac', c')] per site, downloaded"""
    import mpskit_jl_amd as mk
    from mpskit_jl_amd import algorithms
    got = []
    orig = algorithms.regauge

    def spy(be_, ac, c, *a, **k):
        got.append((be.download(ac), be.download(c)))
        return orig(be_, ac, c, *a, **k)
    with monkeypatch.context() as mp:
        mp.setattr(algorithms, "regauge", spy)
        mk.timestep(psi0, H, t, dt, mk.TDVP(), mk.environments(psi0, H))
    return got


def test_infinite_imaginary_time_against_explicit_matrices(be, monkeypatch):
    """InfiniteMPS, two-site cell, D = 8, imaginary time with a prefactor that varies along the step.  Reference: expm on
    the explicit H_AC / H_C matrices, assembled column by column in numpy from the DOWNLOADED environments of every term with
    the oracle's contraction, summed with f_k(t + dt/2) -- no derivative object and no mpsk_hsum.  Bound: 10 x the
    deviation the same comparison shows for a constant plain MPOHamiltonian."""
    import mpskit_jl_amd as mk
    Ha, Hb, _ = _ham(be)
    oa, ob, oc = mo.tfi_mpo(1.0, 0.0), mo.tfi_mpo(0.0, 0.5), mo.tfi_mpo(1.0, 0.5)
    rng = np.random.default_rng(4)
    psi0 = mk.InfiniteMPS.from_tensors([rng.random((8, 2, 8)), rng.random((8, 2, 8))], be=be)
    t, dt = 0.3, -0.4j
    f = lambda s: 1.0 + 4.0 * np.imag(s) ** 2            # real-valued on the complex midpoint t - 0.2i: 1.16 (1.0 at t)
    n = len(psi0)

    def reference(terms, coefs):
        """terms: [(device H, oracle H)]; the environments are built here, separately from the driver's"""
        out = []
        envs = [mk.environments(psi0, Hg) for Hg, _ in terms]
        for loc in range(n):
            gls = [be.download_env(e.leftenv(loc, psi0), Ho[loc].chil) for e, (_, Ho) in zip(envs, terms)]
            grs = [be.download_env(e.rightenv(loc, psi0), Ho[loc].chir) for e, (_, Ho) in zip(envs, terms)]
            glc = [be.download_env(e.leftenv(loc + 1, psi0), Ho[loc].chir) for e, (_, Ho) in zip(envs, terms)]
            hac = lambda x: sum(c * mo.dAC(x, Ho[loc], gl, gr) for c, (_, Ho), gl, gr in zip(coefs, terms, gls, grs))
            hc = lambda x: sum(c * mo.dC(x, gl, gr) for c, gl, gr in zip(coefs, glc, grs))
            ac = tr.local_expm_step(hac, be.download(psi0.AC[loc]), -1j * dt).real
            c = tr.local_expm_step(hc, be.download(psi0.CR[loc]), -1j * dt).real
            out.append((ac, c))
        return out

    def deviation(got, ref):
        return max(max(np.abs(g[0] - r[0]).max(), np.abs(g[1] - r[1]).max()) for g, r in zip(got, ref))

    Hfull = mk.transverse_field_ising(1.0, 0.5, be=be)
    dev0 = deviation(_captured_inf_step(be, monkeypatch, psi0, Hfull, t, dt), reference([(Hfull, oc)], [1.0]))
    tol = 10 * dev0
    Ht = mk.LazySum([Ha, Hb], [1.0, f])
    got = _captured_inf_step(be, monkeypatch, psi0, Ht, t, dt)
    assert len(got) == n
    dev = deviation(got, reference([(Ha, oa), (Hb, ob)], [1.0, f(t + dt / 2)]))
    print(f"infinite: constant-H deviation {dev0:.3e}, bound {tol:.3e}, timed deviation {dev:.3e}")
    assert 0 < dev0 < 1e-10
    assert dev <= tol, (dev, tol)                 # measured: constant-H 7.88e-15 (bound 7.88e-14), timed 1.18e-14
    for te in (t, t + dt):                               # the start or the end of the step instead of the midpoint
        assert deviation(got, reference([(Ha, oa), (Hb, ob)], [1.0, f(te)])) > tol
