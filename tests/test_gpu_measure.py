"""Local expectation values and correlators on the GPU, fused (device=True) and composed (device=False) routes, against a
dense contraction of the downloaded state done here in NumPy.  Tolerance: the project's 1e-10 on O(1) quantities."""
import numpy as np
import pytest

import mpskit_jl_amd as mk
from mpskit_jl_amd import native_cplx

import measure_reference as mr

pytestmark = pytest.mark.gpu

TOL = 1e-10
ROUTES = pytest.mark.parametrize("device", [True, False], ids=["device", "composed"])


@pytest.fixture(scope="module")
def chain2(be):
    psi = mk.FiniteMPS.random(8, 2, 16, np.random.default_rng(1), be=be)
    return psi, mr.state_vector(psi.to_host())


@pytest.fixture(scope="module")
def chain3(be):
    psi = mk.FiniteMPS.random(6, 3, 9, np.random.default_rng(2), be=be)
    return psi, mr.state_vector(psi.to_host())


@ROUTES
def test_finite_one_site(chain2, device):
    psi, v = chain2
    L = len(psi)
    for O in (mr.SZ2, mr.SX2, mr.SY2, mr.SX2 + 1j * mr.SZ2):
        got = mk.expectation_value(psi, O, device=device)
        ref = np.array([mr.ev1(v, O, i) for i in range(L)])
        assert got.shape == (L,) and np.abs(got - ref).max() < TOL
        assert got.dtype == (np.complex128 if np.iscomplexobj(O) else np.float64)
    per_site = [mr.SZ2 if i % 2 else mr.SX2 for i in range(L)]
    got = mk.expectation_value(psi, per_site, device=device)
    assert np.abs(got - [mr.ev1(v, per_site[i], i).real for i in range(L)]).max() < TOL


@ROUTES
def test_finite_correlators(chain2, device):
    psi, v = chain2
    L = len(psi)
    for i in range(L - 1):
        js = range(i + 1, L)
        got = mk.correlator(psi, mr.SP2, mr.SM2, i, js, device=device)
        assert got.dtype == np.float64
        assert np.abs(got - [mr.ev2(v, mr.SP2, i, mr.SM2, j).real for j in js]).max() < TOL
    # a complex O1 on the real state (Re / Im slabs), a complex O2, and both
    Oc = mr.SX2 + 1j * mr.SZ2
    for A, B in ((Oc, mr.SM2), (mr.SP2, Oc), (Oc, Oc), (mr.SY2, mr.SY2)):
        got = mk.correlator(psi, A, B, 1, range(2, L), device=device)
        assert got.dtype == np.complex128
        assert np.abs(got - [mr.ev2(v, A, 1, B, j) for j in range(2, L)]).max() < TOL
    # strided js, scalar j
    i = 1
    js = range(i + 2, L, 3)
    got = mk.correlator(psi, mr.SZ2, mr.SZ2, i, js, device=device)
    assert np.abs(got - [mr.ev2(v, mr.SZ2, i, mr.SZ2, j).real for j in js]).max() < TOL
    one = mk.correlator(psi, mr.SZ2, mr.SZ2, 2, 5, device=device)
    assert isinstance(one, float) and abs(one - mr.ev2(v, mr.SZ2, 2, mr.SZ2, 5).real) < TOL


@ROUTES
def test_finite_two_site_operator(chain2, device):
    psi, v = chain2
    L = len(psi)
    O12 = mr.twosite([(mr.SP2, mr.SM2), (0.3 * mr.SZ2, mr.SX2), (mr.SX2, mr.SX2)])
    for i in (0, 3):
        js = range(i + 1, L)
        got = mk.correlator(psi, O12, i, js, device=device)
        assert np.abs(got - [mr.ev12(v, O12, i, j).real for j in js]).max() < TOL
    assert abs(mk.correlator(psi, O12, 2, 3, device=device) - mk.expectation_value(psi, O12, 2)) < TOL
    Oc = mr.twosite([(mr.SY2, mr.SZ2 + mr.SX2), (mr.SP2, mr.SM2)])
    assert abs(mk.expectation_value(psi, Oc, 4) - mr.ev12(v, Oc, 4, 5)) < TOL
    O123 = np.einsum("ab,cd,ef->acebdf", mr.SX2, mr.SZ2, mr.SX2) + np.einsum("ab,cd,ef->acebdf", mr.SZ2, mr.SX2, mr.SP2)
    w = np.moveaxis(np.tensordot(O123, v, axes=((3, 4, 5), (2, 3, 4))), (0, 1, 2), (2, 3, 4))
    assert abs(mk.expectation_value(psi, O123, 2) - np.vdot(v, w).real) < TOL
    assert abs(mk.expectation_value(psi, mk.decompose_localmpo(O123), 2) - np.vdot(v, w).real) < TOL


@ROUTES
def test_spin_one(chain3, device):
    psi, v = chain3
    L = len(psi)
    for O in (mr.SZ3, mr.SX3, mr.SY3):
        got = mk.expectation_value(psi, O, device=device)
        assert np.abs(got - [mr.ev1(v, O, i) for i in range(L)]).max() < TOL
    for i in range(L - 1):
        js = range(i + 1, L)
        got = mk.correlator(psi, mr.SP3, mr.SM3, i, js, device=device)
        assert np.abs(got - [mr.ev2(v, mr.SP3, i, mr.SM3, j).real for j in js]).max() < TOL
    h2 = mr.heisenberg_bond(3)
    got = mk.correlator(psi, h2, 1, range(2, L), device=device)
    assert np.abs(got - [mr.ev12(v, h2, 1, j).real for j in range(2, L)]).max() < TOL


@ROUTES
def test_energy_identities(be, chain2, device):
    """for any state: sum of the MPO energies = sum of the bond operators, as expectation values and as correlators"""
    psi, _ = chain2
    h2 = mr.heisenberg_bond(2)
    H = mk.from_twosite(h2, be=be)
    E = float(np.sum(mk.expectation_value(psi, H, mk.environments(psi, H))))
    L = len(psi)
    assert abs(E - sum(mk.expectation_value(psi, h2, i, device=device) for i in range(L - 1))) < TOL
    assert abs(E - sum(mk.correlator(psi, h2, i, i + 1, device=device) for i in range(L - 1))) < TOL


@ROUTES
@pytest.mark.parametrize("n", [1, 2])
def test_infinite(be, n, device):
    psi = mk.InfiniteMPS.random(2, 12, np.random.default_rng(30 + n), n=n, be=be)
    h2 = mr.heisenberg_bond(2)
    H = mk.from_twosite(h2, be=be)
    E = float(np.sum(mk.expectation_value(psi, H, mk.environments(psi, H))))
    assert abs(E - sum(mk.expectation_value(psi, h2, at, device=device) for at in range(n))) < TOL
    AC, AR = [be.download(t) for t in psi.AC], [be.download(t) for t in psi.AR]
    js = range(1, 3 * n + 2)
    for A, B in ((mr.SZ2, mr.SZ2), (mr.SP2, mr.SM2), (mr.SY2, mr.SY2)):
        got = mk.correlator(psi, A, B, 0, js, device=device)
        assert np.abs(got - mr.infinite_correlator(AC, AR, A, B, 0, js)).max() < TOL
    got = mk.expectation_value(psi, mr.SZ2, device=device)
    assert got.shape == (n,) and np.abs(got - [np.einsum("asb,ts,atb->", a, mr.SZ2, a) for a in AC]).max() < TOL


@ROUTES
def test_native_complex(be, device):
    L, d, D = 6, 2, 8
    rng = np.random.default_rng(5)
    dims = [min(d ** i, D, d ** (L - i)) for i in range(L + 1)]
    psi = native_cplx.NativeFiniteMPS([rng.standard_normal((dims[i], d, dims[i + 1]))
                                       + 1j * rng.standard_normal((dims[i], d, dims[i + 1])) for i in range(L)], be)
    psi.move_center(3)
    before = [t.copy() for t in psi.to_host()]
    v = mr.state_vector(before)
    got = native_cplx.expectation_value(psi, mr.SY2, device=device)
    ref = np.array([mr.ev1(v, mr.SY2, i) for i in range(L)])
    assert got.dtype == np.complex128 and np.abs(got - ref).max() < TOL
    assert np.abs(ref.real).max() > 1e-3                               # (a complex state: <S^y> does not vanish)
    O = mr.SX2 + 1j * mr.SZ2                                           # not Hermitian: the imaginary parts carry weight
    got = native_cplx.expectation_value(psi, O, device=device)
    assert np.abs(got - [mr.ev1(v, O, i) for i in range(L)]).max() < TOL
    for i in range(L - 1):
        js = range(i + 1, L)
        got = native_cplx.correlator(psi, mr.SP2, mr.SM2, i, js, device=device)
        ref = np.array([mr.ev2(v, mr.SP2, i, mr.SM2, j) for j in js])
        assert got.dtype == np.complex128 and np.abs(got - ref).max() < TOL
        assert np.abs(got.imag - ref.imag).max() < TOL
    got = native_cplx.correlator(psi, mr.heisenberg_bond(2), 0, range(2, L, 2), device=device)
    assert np.abs(got - [mr.ev12(v, mr.heisenberg_bond(2), 0, j) for j in range(2, L, 2)]).max() < TOL
    # the measured state keeps its centre and its tensors
    assert psi.center == 3 and all(np.array_equal(a, b) for a, b in zip(before, psi.to_host()))


def test_errors_and_old_call_forms(be, chain2):
    psi, v = chain2
    for js in (1, [1, 2], [3, 3], [4, 3], []):
        with pytest.raises(ValueError):
            mk.correlator(psi, mr.SZ2, mr.SZ2, 1, js)
    rng = np.random.default_rng(0)
    emb = mk.FiniteMPS.random(4, 2, 4, rng, be=be, dtype=np.complex128)
    with pytest.raises(NotImplementedError, match="native_cplx"):
        mk.expectation_value(emb, mr.SZ2)
    with pytest.raises(NotImplementedError, match="native_cplx"):
        mk.correlator(emb, mr.SZ2, mr.SZ2, 0, 1)
    # the call forms of tests/test_gpu_algorithms.py: MPOHamiltonian + FinEnv, LazySum + MultipleEnvironments, infinite
    H = mk.heisenberg_XXX(0.5, be=be)
    L = len(psi)
    dense = sum(mr.ev12(v, mr.heisenberg_bond(2), i, i + 1).real for i in range(L - 1))
    ens = mk.expectation_value(psi, H, mk.environments(psi, H))
    assert ens.shape == (L,) and abs(float(np.sum(ens)) - dense) < TOL
    Hl = mk.LazySum([H, H], [0.25, 0.5])
    assert abs(float(np.sum(mk.expectation_value(psi, Hl, mk.environments(psi, Hl)))) - 0.75 * dense) < TOL
    inf = mk.InfiniteMPS.random(2, 6, np.random.default_rng(3), be=be)
    e = mk.expectation_value(inf, H, mk.environments(inf, H))
    assert e.shape == (1,) and abs(float(e[0]) - mk.expectation_value(inf, mr.heisenberg_bond(2), 0)) < TOL
