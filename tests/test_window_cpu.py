"""WindowMPS on the host stand-in backends: constructors, environments from the infinite fixed points, the finite drivers
by delegation, dot and transition (composed route) against dense NumPy contractions (window_helpers.py)."""
import numpy as np
import pytest

import mpskit_jl_amd as mk
from mpskit_jl_amd import window
from cpu_backend import CpuBackend, CpuComplexBackend

from window_helpers import SZ, dense_hac, dense_site_matrices, itfi_groundstate, left_canonical_host


@pytest.fixture(scope="module", params=[1, 2], ids=["cell1", "cell2"])
def itfi(request):
    """(be, H, psi, envs, eps, energy density) of a converged iTFI state, D = 8"""
    be = CpuBackend()
    H, psi, envs, eps = itfi_groundstate(be, 8, request.param)
    e = float(np.mean(mk.expectation_value(psi, H, envs)))
    return be, H, psi, envs, eps, e


def test_constructors_and_edges(itfi):
    be, H, psi, *_ = itfi
    w = mk.WindowMPS(psi, 5)
    assert len(w) == 5 and w.right_gs is w.left_gs is psi and not w.cplx
    assert w.max_Ds() == 8
    rng = np.random.default_rng(1)
    r = mk.WindowMPS.random(4, 2, 6, psi, rng=rng)
    assert abs(r.norm() - 1.0) < 1e-12 and r.window.AL(0).shape[0] == 8 and r.window.AL(3).shape[2] == 8
    As = [rng.random((8, 2, 5)), rng.random((5, 2, 8))]
    assert len(mk.WindowMPS(psi, As)) == 2
    assert isinstance(mk.WindowMPS(psi, mk.FiniteMPS(As, be=be)).window, mk.FiniteMPS)
    with pytest.raises(ValueError):
        mk.WindowMPS(psi, [rng.random((7, 2, 5)), rng.random((5, 2, 8))])
    with pytest.raises(ValueError):
        mk.WindowMPS(psi, [rng.random((8, 2, 5)), rng.random((5, 2, 3))])
    with pytest.raises(NotImplementedError):
        mk.WindowMPS(psi, mk.FiniteMPS([a + 1j * a for a in As], be=be))
    assert np.array_equal(be.download(w.l_LL()), np.eye(8)) and np.array_equal(be.download(w.r_RR()), np.eye(8))


def test_copy_is_independent(itfi):
    be, H, psi, *_ = itfi
    w = mk.WindowMPS(psi, 5)
    c = w.copy()
    before = be.download(w.AC(2)).copy()
    c.set_AC(2, be.upload(np.ones(before.shape)))
    assert np.array_equal(be.download(w.AC(2)), before)
    assert np.array_equal(be.download(psi.AC[2 % len(psi)]), before)
    h = 2.0 * w
    assert abs(h.norm() - 2.0) < 1e-12 and abs(w.norm() - 1.0) < 1e-12
    assert abs(h.normalize().norm() - 1.0) < 1e-12
    with pytest.raises(TypeError):
        1j * w


def test_promoted_window_is_the_uniform_state(itfi):
    be, H, psi, envs, eps, e = itfi
    w = mk.WindowMPS(psi, 5)
    assert abs(w.norm() - 1.0) < 1e-12
    wenvs = mk.environments(w, H, envs, envs)
    assert isinstance(wenvs, mk.FinEnv) and wenvs.window_canonical
    gal = max(mk.calc_galerkin(w, i, wenvs) for i in range(5))
    print("galerkin of the window", gal, "VUMPS residual", eps)
    assert gal < max(10 * eps, 1e-10)
    vals, tot = mk.expectation_value(w, H, wenvs)
    assert np.abs(vals - e).max() < 1e-9
    w2, wenvs2, _ = mk.find_groundstate(w, H, mk.DMRG(maxiter=1, tol=1e-14), wenvs)
    vals2, tot2 = mk.expectation_value(w2, H, wenvs2)
    assert isinstance(w2, mk.WindowMPS) and w2.left_gs is psi
    assert abs(np.sum(vals2) - np.sum(vals)) < 1e-9 and abs(tot2 - tot) < 1e-9
    assert w2.window.AL(0).shape[0] == 8 and w2.window.AR(4).shape[2] == 8


def test_default_environments_and_variance(itfi):
    """the variance of the converged uniform state vanishes: AC is an eigenvector of H_AC up to the residual r of VUMPS, so
    the variance is r^2 <= (10 eps tot)^2 plus the rounding of the difference of two numbers of size tot^2"""
    be, H, psi, envs, eps, e = itfi
    w = mk.WindowMPS(psi, 5)
    vals, tot = mk.expectation_value(w, H)
    assert np.abs(vals - e).max() < 1e-9
    v = mk.variance(w, H)
    gal = max(mk.calc_galerkin(w, i, mk.environments(w, H, envs, envs)) for i in range(5))
    bound = (10 * max(eps, gal) * abs(tot)) ** 2 + 64 * 2.0 ** -53 * tot ** 2
    print("variance", v, "bound", bound, "galerkin", gal, "tot", tot)
    assert abs(v) <= bound


def test_variance_of_a_perturbed_window_against_dense(itfi):
    be, H, psi, envs, *_ = itfi
    w = mk.WindowMPS(psi, 5)
    rng = np.random.default_rng(4)
    ac = be.download(w.AC(2))
    w.set_AC(2, be.upload(ac + 0.2 * rng.standard_normal(ac.shape)))
    wenvs = mk.environments(w, H, envs, envs)
    v = mk.variance(w, H, wenvs)
    x = be.download(w.AC(4)).reshape(-1)
    M = dense_hac(be, H[4], wenvs.leftenv(4, w.window), wenvs.rightenv(4, w.window))
    y = M @ x
    assert np.abs(y - be.download(mk.ddAC(4, w.window, H, wenvs)(w.AC(4))).reshape(-1)).max() < 1e-12 * np.abs(y).max()
    ref = (y @ y) / (x @ x) - ((x @ y) / (x @ x)) ** 2
    print("variance", v, "dense", ref)
    assert ref > 1e-3 and abs(v - ref) < 1e-11 * max(1.0, (y @ y) / (x @ x))
    assert abs(mk.variance(w, H) - v) < 1e-9                      # default environments: the same number


def test_dot_and_transition_of_a_window_with_itself(itfi):
    be, H, psi, *_ = itfi
    w = mk.WindowMPS(psi, 5)
    assert abs(window.dot(w, w) - 1.0) < 1e-12 and abs(mk.dot(w, w) - 1.0) < 1e-12
    sz = mk.expectation_value(w, SZ)
    assert np.abs(mk.transition(w, w, SZ) - sz).max() < 1e-12
    Ms = mk.transition(w, w)
    assert len(Ms) == 5 and all(abs(np.trace(m) - 1.0) < 1e-12 for m in Ms)


def test_dynamics_and_bond_changes_keep_the_outer_bonds(itfi):
    be, H, psi, envs, *_ = itfi
    w = mk.WindowMPS(psi, 5)
    wenvs = mk.environments(w, H, envs, envs)
    cut = mk.changebonds(w, mk.SvdCut(trunc_dim=4))
    assert isinstance(cut, mk.WindowMPS) and cut.window.AL(0).shape[0] == 8 and cut.window.AR(4).shape[2] == 8
    assert cut.max_Ds() == 8 and max(cut.window.bond_dims()[:-1]) <= 4
    grown, _ = mk.changebonds(cut, H, mk.OptimalExpand(trunc_dim=2))
    assert grown.window.AL(0).shape[0] == 8 and grown.window.AR(4).shape[2] == 8
    w2, _, _ = mk.find_groundstate(cut, H, mk.DMRG2(maxiter=1, trunc_dim=8))
    assert w2.window.AL(0).shape[0] == 8 and w2.window.AR(4).shape[2] == 8
    # imaginary-time TDVP step of the uniform state itself: the energy does not move
    w3, wenvs3 = mk.timestep(w, H, 0.0, -0.05j, mk.TDVP(), wenvs)
    assert abs(mk.expectation_value(w3, H, wenvs3)[1] - mk.expectation_value(w, H)[1]) < 1e-8
    assert len(mk.entanglement_spectrum(w, 2)) == 8 and mk.entropy(w, 2) > 0


@pytest.mark.parametrize("kinds", [("real", "real"), ("cplx", "cplx"), ("real", "cplx")], ids=lambda k: "-".join(k))
def test_transition_of_two_random_windows_against_dense(kinds):
    be = CpuComplexBackend()
    rng = np.random.default_rng(11)
    psi = mk.InfiniteMPS.random(2, 3, rng, be=be)
    L, d = 4, 2
    dt = {"real": None, "cplx": np.complex128}
    bra = mk.WindowMPS.random(L, d, 4, psi, rng=rng, dtype=dt[kinds[0]])
    ket = mk.WindowMPS.random(L, d, 6, psi, rng=rng, dtype=dt[kinds[1]])
    ref = dense_site_matrices(left_canonical_host(bra), left_canonical_host(ket))
    Ms = mk.transition(bra, ket)
    assert max(np.abs(m - r).max() for m, r in zip(Ms, ref)) < 1e-12
    ov = window.dot(bra, ket)
    assert abs(ov - np.trace(ref[0])) < 1e-12
    assert abs(window.dot(ket, bra) - np.conj(ov)) < 1e-12
    ops = [rng.standard_normal((d, d)) for _ in range(L)]
    got = mk.transition(bra, ket, ops)
    assert np.abs(got - np.array([np.sum(o * r) for o, r in zip(ops, ref)])).max() < 1e-12


def test_dot_refuses_different_environments():
    be = CpuBackend()
    rng = np.random.default_rng(2)
    a, b = mk.InfiniteMPS.random(2, 3, rng, be=be), mk.InfiniteMPS.random(2, 3, rng, be=be)
    wa, wb = mk.WindowMPS.random(3, 2, 4, a, rng=rng), mk.WindowMPS.random(3, 2, 4, b, rng=rng)
    with pytest.raises(ValueError):
        window.dot(wa, wb)
    neg = mk.InfiniteMPS([be.upload(-be.download(t)) for t in a.AL], [be.upload(-be.download(t)) for t in a.AR], a.CR,
                         [be.upload(-be.download(t)) for t in a.AC], be)       # the same state up to a sign: overlap -1
    neg.cplx = False
    with pytest.raises(ValueError):
        window.dot(wa, mk.WindowMPS(neg, wa.window))
    same = mk.InfiniteMPS(a.AL, a.AR, a.CR, a.AC, be)          # another object, the same state
    same.cplx = False
    assert abs(window.dot(wa, mk.WindowMPS(same, wa.window)) - 1.0) < 1e-12


def test_complex_window_variance_and_complex_scalar():
    """an interleaved complex window built from the tensors of a real one: the same variance and energy; a complex
    scalar multiplies the overlap"""
    be, cbe = CpuBackend(), CpuComplexBackend()
    rng = np.random.default_rng(5)
    H = mk.transverse_field_ising(1.0, 1.5, be=be)
    psi = mk.InfiniteMPS.random(2, 4, rng, be=be)
    envs = mk.environments(psi, H)
    wr = mk.WindowMPS.random(4, 2, 6, psi, rng=rng)
    wenvs = mk.environments(wr, H, envs, envs)
    vr, tr = mk.variance(wr, H, wenvs), mk.expectation_value(wr, H, wenvs)[1]
    psic = mk.InfiniteMPS(psi.AL, psi.AR, psi.CR, psi.AC, cbe)           # host buffers either way
    psic.cplx = False
    envs.be, envs.dependency = cbe, psic
    Hc = mk.transverse_field_ising(1.0, 1.5, be=cbe)
    wc = mk.WindowMPS(psic, [t.astype(np.complex128) for t in wr.to_host()])
    cenvs = mk.environments(wc, Hc, envs, envs)
    vc, tc = mk.variance(wc, Hc, cenvs), mk.expectation_value(wc, Hc, cenvs)[1]
    print("variance real", vr, "complex", vc, "tot", tr, tc)
    assert vr > 1e-3 and abs(vc - vr) < 1e-10 * max(1.0, abs(vr)) and abs(tc - tr) < 1e-10
    z = 0.3 - 0.4j
    assert abs(window.dot(wc, z * wc) - z * window.dot(wc, wc)) < 1e-12
    assert abs((z * wc).norm() - abs(z) * wc.norm()) < 1e-12
