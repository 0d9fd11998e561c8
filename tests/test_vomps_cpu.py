"""approximate / leading_boundary with VOMPS on uniform states, the mixed (above != below) PerMPOInfEnv, dot and
DenseMPO * InfiniteMPS on the NumPy stand-in backend (tests/cpu_backend.py): host logic only, no GPU.  The stand-in has no
dAC_proj / dC_proj, so every projection here takes the composed route.  The case bodies live here; tests/test_gpu_vomps.py
runs the same bodies on the device.  Overlaps and fixed-point residuals are recomputed from downloaded tensors with dense
NumPy (restatements below), independently of the code under test."""
import math

import numpy as np
import pytest

import mpskit_jl_amd as mk
from cpu_backend import CpuBackend, HostSlice


class DenseCpuBackend(CpuBackend):
    """CpuBackend + mposlice_dense: a DenseMPO tensor as a one-level host slice (oracle arithmetic)."""

    def mposlice_dense(self, O):
        O = np.asarray(O)
        return HostSlice(1, O.shape[1], [O.shape[0]], [O.shape[3]], {(0, 0): O})


# ---- NumPy restatements ------------------------------------------------------------------------------------------------

def env_host(be, t):
    """slab layout (W, D1, D2), each slab column-major -> ndarray [w, i, j]"""
    W, D1, D2 = t.shape
    return be.download(t.reshape(t.size)).reshape(W, D2, D1).transpose(0, 2, 1)


def densify(O, site):
    """[Wl, d, d, Wr] tensor of one site of a SparseMPO whose levels have dimension 1 (the block table, densified)"""
    t = np.zeros((O.odim, O.d, O.d, O.odim))
    for (i, j), v in O.data[site % O.period].items():
        t[i, :, :, j] = v * np.eye(O.d) if np.isscalar(v) else np.asarray(v)[0, :, :, 0]
    return t


def to_dense_mpo(O):
    return mk.DenseMPO([densify(O, s) for s in range(O.period)])


def site_tensor(O, site):
    return O[site] if isinstance(O, mk.DenseMPO) else densify(O, site)


def tl_host(gl, o, a, b):
    """gl[w, below, above] -> [v, below', above'] through ket a (above), operator o[w, t, s, v], bra b (below)"""
    return np.einsum("wpq,qsj,wtsv,pti->vij", gl, a, o, b, optimize=True)


def tr_host(gr, o, a, b):
    """gr[v, above', below'] -> [w, above, below]"""
    return np.einsum("qsj,wtsv,pti,vji->wqp", a, o, b, gr, optimize=True)


def lead_host(As, Bs, Os=None):
    """|leading eigenvalue| of the unit-cell transfer matrix with kets As, bras Bs and (optionally) operators Os, dense"""
    n = len(As)
    W = 1 if Os is None else Os[0].shape[0]
    dim = (W, Bs[0].shape[0], As[0].shape[0])
    cols = []
    for k in range(int(np.prod(dim))):
        v = np.zeros(int(np.prod(dim)))
        v[k] = 1.0
        v = v.reshape(dim)
        for i in range(n):
            o = np.eye(As[i].shape[1])[None, :, :, None] if Os is None else Os[i % len(Os)]
            v = tl_host(v, o, As[i], Bs[i])
        cols.append(v.reshape(-1))
    return np.abs(np.linalg.eigvals(np.array(cols).T)).max()


def overlap(be, x, y, mpo=None):
    """|<x | mpo | y>| per unit cell of two normalised uniform states, dense NumPy on the downloaded AL tensors"""
    xs, ys = [be.download(t) for t in x.AL], [be.download(t) for t in y.AL]
    return lead_host(ys, xs, None if mpo is None else [np.asarray(o) for o in mpo])


def parallel_residual(t, ref):
    t, ref = t.reshape(-1), ref.reshape(-1)
    r = (t @ ref) / (ref @ ref)
    return np.linalg.norm(t - r * ref) / np.linalg.norm(t), r


# ---- case bodies (shared with the device tests) ----------------------------------------------------------------------

def mixed_operators(be):
    O2 = mk.make_time_mpo(mk.transverse_field_ising(1.0, 0.7, be=be), -0.05j, mk.WII())
    assert isinstance(O2, mk.SparseMPO) and not O2.cplx
    return [("ising", mk.classical_ising()), ("WII", O2)]


def case_mixed_environments(be):
    """above D = 6, below D = 4, two-site cells: shapes, fixed-point residuals of lw[0] / rw[n - 1] (solver tol 1e-12, bound
    1e-9), exact propagation through the cell, |lambda_col| = 1."""
    n = 2
    above = mk.InfiniteMPS.random(2, 6, np.random.default_rng(11), n=n, be=be)
    below = mk.InfiniteMPS.random(2, 4, np.random.default_rng(12), n=n, be=be)
    for name, O in mixed_operators(be):
        envs = mk.environments(below, (O, above), tol=1e-12)
        assert isinstance(envs, mk.PerMPOInfEnv) and envs.above is above
        W = site_tensor(O, 0).shape[0]
        lw = [env_host(be, envs.leftenv(i, below)) for i in range(n)]
        rw = [env_host(be, envs.rightenv(i, below)) for i in range(n)]
        for i in range(n):
            assert envs.leftenv(i, below).shape == (W, 4, 6) and envs.rightenv(i, below).shape == (W, 6, 4)
        ALa, ALb = [be.download(t) for t in above.AL], [be.download(t) for t in below.AL]
        ARa, ARb = [be.download(t) for t in above.AR], [be.download(t) for t in below.AR]
        t = lw[0]
        for i in range(n):
            t = tl_host(t, site_tensor(O, i), ALa[i], ALb[i])
            if i < n - 1:
                res, _ = parallel_residual(t, lw[i + 1])
                assert res <= 1e-12, (name, "left cell", i, res)
        resl, laml = parallel_residual(t, lw[0])
        t = rw[n - 1]
        for i in range(n - 1, -1, -1):
            t = tr_host(t, site_tensor(O, i), ARa[i], ARb[i])
            if i > 0:
                res, _ = parallel_residual(t, rw[i - 1])
                assert res <= 1e-12, (name, "right cell", i, res)
        resr, lamr = parallel_residual(t, rw[n - 1])
        print(name, "fixed-point residuals", resl, resr, "eigenvalues", laml, lamr)
        assert resl <= 1e-9 and resr <= 1e-9, (name, resl, resr)
        assert abs(laml - lamr) <= 1e-9 * abs(laml), (name, laml, lamr)
        for col in range(n):
            ca, cb = be.download(above.CR[col]), be.download(below.CR[col])
            lam = np.einsum("pq,wpa,ab,wbq->", cb, lw[(col + 1) % n], ca, rw[col], optimize=True)
            print(name, "lambda", col, lam)
            assert abs(abs(lam) - 1.0) <= 1e-12, (name, col, lam)


def case_mixed_equals_plain(be):
    """environments(psi, (O, psi)) against environments(psi, O): the same tensors up to a sign each, to 1e-10."""
    n = 2
    psi = mk.InfiniteMPS.random(2, 6, np.random.default_rng(13), n=n, be=be)
    O = mk.classical_ising()
    plain = mk.environments(psi, O, tol=1e-12)
    mixed = mk.environments(psi, (O, psi), tol=1e-12)
    assert plain.above is None and mixed.above is psi
    for i in range(n):
        for a, b in ((plain.leftenv(i, psi), mixed.leftenv(i, psi)), (plain.rightenv(i, psi), mixed.rightenv(i, psi))):
            assert a.shape == b.shape == (2, 6, 6)
            x, y = env_host(be, a), env_host(be, b)
            err = min(np.abs(x - y).max(), np.abs(x + y).max()) / np.abs(x).max()
            assert err <= 1e-10, (i, err)
    assert mk.calc_galerkin(psi, mixed) == pytest.approx(mk.calc_galerkin(psi, plain), rel=1e-8, abs=1e-12)


def rotation_mpo(theta=0.4):
    r = np.array([[math.cos(theta), -math.sin(theta)], [math.sin(theta), math.cos(theta)]])
    return mk.DenseMPO(r[None, :, :, None])


def case_exact_target(be):
    """W = 1 on-site rotation, above and below random with D = 8: the target is exactly representable.  VOMPS(tol=1e-10,
    maxiter=200) reaches eps <= 1e-10 and 1 - |<result | O above>| <= 1e-8.  3 iterations on the NumPy stand-in (seeds
    21 / 22, eps 1.6e-12, overlap 0.894 before)."""
    O = rotation_mpo()
    above = mk.InfiniteMPS.random(2, 8, np.random.default_rng(21), be=be)
    below = mk.InfiniteMPS.random(2, 8, np.random.default_rng(22), be=be)
    before = overlap(be, below, above, O)
    psi, envs, eps = mk.approximate(below, (O, above), mk.VOMPS(tol=1e-10, maxiter=200))
    target = O * above
    assert target.AL[0].shape == (8, 2, 8)
    ov = mk.dot(psi, target)
    ov_host = overlap(be, psi, target)
    print("exact target: iterations", len(envs.history), "eps", eps, "overlap before", before, "after", ov, ov_host)
    assert eps <= 1e-10
    assert [it for it, _ in envs.history] == list(range(1, len(envs.history) + 1)) and envs.history[-1][1] == eps
    assert 1.0 - abs(ov) <= 1e-8 and 1.0 - ov_host <= 1e-8
    assert abs(mk.dot(psi, O, above)) == pytest.approx(ov_host, abs=1e-8)
    return len(envs.history)


def case_time_step(be):
    """test/algorithms.jl:447-467 in imaginary time: one step of exp(-tau H), tau = 1e-3, by VOMPS with the W^I MPO (sparse)
    and with the densified W^II MPO against TDVP; overlaps equal 1 to atol = tau."""
    tau = 1e-3
    H = mk.transverse_field_ising(1.0, 4.0, be=be)
    psi = mk.InfiniteMPS.random(2, 10, np.random.default_rng(31), n=2, be=be)
    sW1 = mk.make_time_mpo(H, -1j * tau, mk.WI())
    W2 = to_dense_mpo(mk.make_time_mpo(H, -1j * tau, mk.WII()))
    st1, e1, eps1 = mk.approximate(psi, (sW1, psi), mk.VOMPS())
    st2, e2, eps2 = mk.approximate(psi, (W2, psi), mk.VOMPS())
    st5, _ = mk.timestep(psi, H, 0.0, -1j * tau, mk.TDVP())
    o1, o2 = abs(mk.dot(st1, st5)), abs(mk.dot(st2, st5))
    h1, h2 = overlap(be, st1, st5), overlap(be, st2, st5)
    print("time step: eps", eps1, eps2, "iterations", len(e1.history), len(e2.history), "overlaps", o1, o2, h1, h2)
    assert abs(o1 - 1.0) <= tau and abs(o2 - 1.0) <= tau
    assert abs(h1 - 1.0) <= tau and abs(h2 - 1.0) <= tau
    assert overlap(be, st1, psi) < 1.0 - 1e-9 or overlap(be, st1, st5) > overlap(be, psi, st5)   # the step moved the state


def case_leading_boundary(be):
    """test/algorithms.jl:185-199: critical classical Ising from D = 10, VOMPS(tol=1e-5): 2.5337 +- 1e-3, as the reference
    asks, and the VUMPS value from the same start.  At the critical point the power method converges algebraically: on the
    NumPy stand-in it stops at maxiter = 100 with a Galerkin error of 6.5e-5 (the reference's test does not ask for
    convergence either).  Both runs approximate the same D = 10 fixed point and the eigenvalue is stationary there, so the two
    values must agree far better than either agrees with 2.5337: the bar is a tenth of that accuracy, 1e-4."""
    mpo = mk.classical_ising()
    psi0 = mk.InfiniteMPS.random(2, 10, np.random.default_rng(41), be=be)
    eps0 = mk.calc_galerkin(psi0, mk.environments(psi0, mpo))
    psi, envs, eps = mk.leading_boundary(psi0, mpo, mk.VOMPS(tol=1e-5))
    lam = mk.expectation_value(psi, mpo, envs)[0]
    psi_v, envs_v, eps_v = mk.leading_boundary(psi0, mpo, mk.VUMPS(tol=1e-5))
    lam_v = mk.expectation_value(psi_v, mpo, envs_v)[0]
    print("leading_boundary: VOMPS", lam, eps, envs.history, "VUMPS", lam_v, eps_v, "start", eps0)
    assert eps < eps0 and envs.history[-1][2] == eps
    assert lam == pytest.approx(2.5337, abs=1e-3)
    assert lam == pytest.approx(lam_v, abs=1e-4)


def case_compression(be):
    """test/algorithms.jl:478-484 on uniform states: above = classical_ising() * psi (exact, bond 20), below D = 10;
    |dot(below, above)| grows under approximate."""
    rng = np.random.default_rng(51)
    psi = mk.InfiniteMPS.random(2, 10, rng, be=be)
    above = mk.classical_ising() * psi
    assert above.AL[0].shape == (20, 2, 20)
    below = mk.InfiniteMPS.random(2, 10, rng, be=be)
    ident = mk.DenseMPO(np.eye(2)[None, :, :, None])
    before = abs(mk.dot(below, above))
    res, envs, eps = mk.approximate(below, (ident, above), mk.VOMPS(tol=1e-8, maxiter=100))
    after = abs(mk.dot(res, above))
    print("compression: before", before, "after", after, "eps", eps, "iterations", len(envs.history))
    assert res.AL[0].shape == (10, 2, 10)
    assert before < after <= 1.0 + 1e-10
    assert after == pytest.approx(overlap(be, res, above), abs=1e-8)


def case_error_paths(be):
    psi = mk.InfiniteMPS.random(2, 4, np.random.default_rng(61), be=be)
    psi2 = mk.InfiniteMPS.random(2, 4, np.random.default_rng(62), n=2, be=be)
    O = mk.classical_ising()
    with pytest.raises(ValueError, match="unit cells"):
        mk.approximate(psi, (O, psi2), mk.VOMPS())
    with pytest.raises(ValueError, match="unit cells"):
        mk.environments(psi, (O, psi2))
    with pytest.raises(TypeError, match="VOMPS"):
        mk.approximate(psi, (O, psi), mk.DMRG())
    with pytest.raises(TypeError, match="VOMPS"):
        mk.leading_boundary(psi, O, mk.DMRG())
    Oc = mk.make_time_mpo(mk.transverse_field_ising(1.0, 0.7, be=be), 0.05, mk.WII())     # real time: complex storage
    assert Oc.cplx
    with pytest.raises(NotImplementedError, match="complex"):
        mk.approximate(psi, (Oc, psi), mk.VOMPS())
    with pytest.raises(NotImplementedError, match="complex"):
        mk.environments(psi, (Oc, psi))
    psic = mk.InfiniteMPS.random(2, 4, np.random.default_rng(63), be=be)
    psic.cplx = True                                     # what a state built from complex tensors carries
    with pytest.raises(NotImplementedError, match="complex"):
        mk.approximate(psic, (O, psi), mk.VOMPS())
    with pytest.raises(NotImplementedError, match="complex"):
        mk.approximate(psi, (O, psic), mk.VOMPS())
    with pytest.raises(NotImplementedError, match="complex"):
        mk.dot(psic, psi)
    with pytest.raises(TypeError):
        mk.approximate(psi, psi, mk.VOMPS())             # a bare state: the uniform form takes (O, above)


def case_vumps_is_converted(be):
    """approximate/vomps.jl:12-17: a VUMPS passed to the uniform approximate runs as the VOMPS with its fields."""
    O = rotation_mpo()
    above = mk.InfiniteMPS.random(2, 4, np.random.default_rng(71), be=be)
    below = mk.InfiniteMPS.random(2, 4, np.random.default_rng(72), be=be)
    seen = []

    def finalize(it, psi, toapprox, envs):
        seen.append(it)
        return psi, envs
    a = mk.approximate(below, (O, above), mk.VUMPS(tol=1e-6, maxiter=3, finalize=finalize))
    b = mk.approximate(below, (O, above), mk.VOMPS(tol=1e-6, maxiter=3))
    assert seen == [it for it, _ in a[1].history] and len(seen) >= 1
    assert a[1].history == b[1].history and a[2] == b[2]


@pytest.fixture()
def be():
    return DenseCpuBackend()


# ---- tests -------------------------------------------------------------------------------------------------------------

def test_vomps_dataclass_and_exports():
    alg = mk.VOMPS()
    assert (alg.tol, alg.maxiter, alg.finalize, alg.verbosity) == (1e-12, 100, None, 0)
    v = mk.VUMPS()
    for f in ("gauge_tol_min", "gauge_tol_max", "gauge_tol_factor", "env_tol_min", "env_tol_max", "env_tol_factor"):
        assert getattr(alg, f) == getattr(v, f)
    u = mk.VOMPS(tol=1e-6) & mk.VUMPS()
    assert isinstance(u, mk.UnionAlg) and u.alg1.tol == 1e-6
    for name in ("VOMPS", "dot", "ac_proj", "c_proj"):
        assert hasattr(mk, name)


def test_dense_mpo_times_state(be):
    """DenseMPO * InfiniteMPS (densempo.jl:31-44): bond W D, and <O psi | O psi> / <psi | O^T O | psi> consistent: the
    normalised product overlaps with itself as 1 and with psi as the dense value."""
    psi = mk.InfiniteMPS.random(2, 3, np.random.default_rng(5), n=2, be=be)
    O = mk.classical_ising()
    prod = O * psi
    assert len(prod) == 2 and prod.AL[0].shape == (6, 2, 6)
    assert abs(mk.dot(prod, prod)) == pytest.approx(1.0, abs=1e-10)
    # dense check: |<phi | O psi>| / sqrt(<O psi | O psi>) for a third state phi
    phi = mk.InfiniteMPS.random(2, 4, np.random.default_rng(6), n=2, be=be)
    As, Bs = [be.download(t) for t in psi.AL], [be.download(t) for t in phi.AL]
    Ts = [np.einsum("asb,wtsv->watvb", a, O[0]).reshape(6, 2, 6) for a in As]
    want = lead_host(Ts, Bs) / math.sqrt(lead_host(Ts, Ts))
    assert abs(mk.dot(phi, prod)) == pytest.approx(want, rel=1e-9)
    assert abs(mk.dot(phi, O, psi)) == pytest.approx(lead_host(As, Bs, [O[0]]), rel=1e-9)
    with pytest.raises(ValueError):
        mk.classical_ising().repeat(2) * mk.InfiniteMPS.random(2, 3, np.random.default_rng(7), n=3, be=be)


def test_dot_of_uniform_states(be):
    psi = mk.InfiniteMPS.random(2, 5, np.random.default_rng(8), n=2, be=be)
    phi = mk.InfiniteMPS.random(2, 3, np.random.default_rng(9), n=2, be=be)
    assert abs(mk.dot(psi, psi)) == pytest.approx(1.0, abs=1e-10)
    assert abs(mk.dot(psi, phi)) == pytest.approx(overlap(be, psi, phi), rel=1e-9)
    assert abs(mk.dot(phi, psi)) == pytest.approx(abs(mk.dot(psi, phi)), rel=1e-9)


def test_projections_take_the_composed_route(be):
    """the stand-in has neither dAC_proj nor dC_proj: c_proj is gemm products per slab, ac_proj the rectangular dAC; both
    against einsum"""
    assert not hasattr(be, "dC_proj") and not hasattr(be, "dAC_proj")
    above = mk.InfiniteMPS.random(2, 5, np.random.default_rng(14), be=be)
    below = mk.InfiniteMPS.random(2, 3, np.random.default_rng(15), be=be)
    O = mk.classical_ising()
    envs = mk.environments(below, (O, above))
    gl, gr = env_host(be, envs.leftenv(0, below)), env_host(be, envs.rightenv(0, below))
    c = be.download(mk.c_proj(0, below, envs))
    want = np.einsum("wpa,ab,wbq->pq", gl, be.download(above.CR[0]), gr)
    assert c.shape == (3, 3) and np.abs(c - want).max() <= 1e-13 * np.abs(want).max()
    ac = be.download(mk.ac_proj(0, below, envs))
    want = np.einsum("wpa,asb,wtsv,vbq->ptq", gl, be.download(above.AC[0]), O[0], gr, optimize=True)
    assert ac.shape == (3, 2, 3) and np.abs(ac - want).max() <= 1e-13 * np.abs(want).max()


def test_mixed_environments(be):
    case_mixed_environments(be)


def test_mixed_equals_plain(be):
    case_mixed_equals_plain(be)


def test_recalculate_reuses_or_redraws(be):
    """recalculate(below): same bond dimensions restart from the previous fixed points, new ones draw random vectors of the
    new shapes (gen_init_fps)"""
    above = mk.InfiniteMPS.random(2, 5, np.random.default_rng(16), be=be)
    below = mk.InfiniteMPS.random(2, 3, np.random.default_rng(17), be=be)
    O = mk.classical_ising()
    envs = mk.environments(below, (O, above))
    l0 = env_host(be, envs.leftenv(0, below))
    state = envs.rng.bit_generator.state
    envs.recalculate(mk.InfiniteMPS.random(2, 3, np.random.default_rng(18), be=be), 1e-12)
    assert envs.rng.bit_generator.state == state                      # no random draw
    other = mk.InfiniteMPS.random(2, 4, np.random.default_rng(19), be=be)
    assert envs.leftenv(0, other).shape == (2, 4, 5) and envs.rightenv(0, other).shape == (2, 5, 4)
    assert envs.rng.bit_generator.state != state and envs.dependency is other
    envs.recalculate(below, 1e-12)
    l1 = env_host(be, envs.leftenv(0, below))
    assert min(np.abs(l0 - l1).max(), np.abs(l0 + l1).max()) <= 1e-9 * np.abs(l0).max()


def test_exact_target(be):
    """converges in 3 iterations on the NumPy stand-in (seeds 21 / 22), eps 1.6e-12"""
    assert case_exact_target(be) <= 200


def test_time_step_against_tdvp(be):
    case_time_step(be)


def test_leading_boundary_vomps(be):
    case_leading_boundary(be)


def test_compression(be):
    case_compression(be)


def test_error_paths(be):
    case_error_paths(be)


def test_vumps_is_converted(be):
    case_vumps_is_converted(be)
