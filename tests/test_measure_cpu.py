"""Host logic of the local measurements on the CPU stand-in backend (which has neither site_gram nor transfer_left_gram:
every call below takes the composed route), against a dense contraction; the operator split; the dispatch."""
import numpy as np
import pytest

import mpskit_jl_amd as mk
from mpskit_jl_amd import measure, native_cplx

import measure_reference as mr
from cpu_backend import CpuBackend, CpuComplexBackend

TOL = 1e-10


@pytest.fixture(scope="module")
def cbe():
    return CpuBackend()


@pytest.fixture(scope="module")
def chain2(cbe):
    psi = mk.FiniteMPS.random(8, 2, 16, np.random.default_rng(1), be=cbe)
    return psi, mr.state_vector(psi.to_host())


def test_the_stand_in_takes_the_composed_route(cbe):
    assert not hasattr(cbe, "site_gram") and not hasattr(cbe, "transfer_left_gram")
    with pytest.raises(mk.MpskError):
        mk.expectation_value(mk.FiniteMPS.random(3, 2, 2, np.random.default_rng(0), be=cbe), mr.SZ2, device=True)


def test_finite_one_site(chain2):
    psi, v = chain2
    L = len(psi)
    for O in (mr.SZ2, mr.SX2, mr.SY2, mr.SX2 + 1j * mr.SZ2):
        got = mk.expectation_value(psi, O)
        assert got.dtype == (np.complex128 if np.iscomplexobj(O) else np.float64)
        assert np.abs(got - [mr.ev1(v, O, i) for i in range(L)]).max() < TOL


def test_finite_correlators(chain2):
    psi, v = chain2
    L = len(psi)
    for i in range(L - 1):
        js = range(i + 1, L)
        got = mk.correlator(psi, mr.SP2, mr.SM2, i, js)
        assert np.abs(got - [mr.ev2(v, mr.SP2, i, mr.SM2, j).real for j in js]).max() < TOL
    Oc = mr.SX2 + 1j * mr.SZ2
    for A, B in ((Oc, mr.SM2), (mr.SP2, Oc), (Oc, Oc)):
        got = mk.correlator(psi, A, B, 1, range(2, L))
        assert np.abs(got - [mr.ev2(v, A, 1, B, j) for j in range(2, L)]).max() < TOL
    js = range(3, L, 3)
    got = mk.correlator(psi, mr.SZ2, mr.SZ2, 1, js)
    assert np.abs(got - [mr.ev2(v, mr.SZ2, 1, mr.SZ2, j).real for j in js]).max() < TOL
    O12 = mr.twosite([(mr.SP2, mr.SM2), (0.3 * mr.SZ2, mr.SX2)])
    got = mk.correlator(psi, O12, 2, range(3, L))
    assert np.abs(got - [mr.ev12(v, O12, 2, j).real for j in range(3, L)]).max() < TOL
    for js in (1, [4, 3], []):
        with pytest.raises(ValueError):
            mk.correlator(psi, mr.SZ2, mr.SZ2, 1, js)


def test_spin_one_and_energy_identities(cbe):
    psi = mk.FiniteMPS.random(6, 3, 9, np.random.default_rng(2), be=cbe)
    v = mr.state_vector(psi.to_host())
    L = len(psi)
    got = mk.expectation_value(psi, mr.SY3)
    assert np.abs(got - [mr.ev1(v, mr.SY3, i) for i in range(L)]).max() < TOL
    got = mk.correlator(psi, mr.SP3, mr.SM3, 0, range(1, L))
    assert np.abs(got - [mr.ev2(v, mr.SP3, 0, mr.SM3, j).real for j in range(1, L)]).max() < TOL
    h2 = mr.heisenberg_bond(3)
    H = mk.from_twosite(h2, be=cbe)
    E = float(np.sum(mk.expectation_value(psi, H, mk.environments(psi, H))))
    assert abs(E - sum(mk.expectation_value(psi, h2, i) for i in range(L - 1))) < TOL
    assert abs(E - sum(mk.correlator(psi, h2, i, i + 1) for i in range(L - 1))) < TOL


@pytest.mark.parametrize("n", [1, 2])
def test_infinite(cbe, n):
    psi = mk.InfiniteMPS.random(2, 12, np.random.default_rng(30 + n), n=n, be=cbe)
    h2 = mr.heisenberg_bond(2)
    H = mk.from_twosite(h2, be=cbe)
    E = float(np.sum(mk.expectation_value(psi, H, mk.environments(psi, H))))
    assert abs(E - sum(mk.expectation_value(psi, h2, at) for at in range(n))) < TOL
    AC, AR = [cbe.download(t) for t in psi.AC], [cbe.download(t) for t in psi.AR]
    js = range(1, 3 * n + 2)
    for A, B in ((mr.SZ2, mr.SZ2), (mr.SP2, mr.SM2)):
        got = mk.correlator(psi, A, B, 0, js)
        assert np.abs(got - mr.infinite_correlator(AC, AR, A, B, 0, js)).max() < TOL


def test_native_complex_composed():
    be = CpuComplexBackend()
    L, d, D = 5, 2, 4
    rng = np.random.default_rng(5)
    dims = [min(d ** i, D, d ** (L - i)) for i in range(L + 1)]
    psi = native_cplx.NativeFiniteMPS([rng.standard_normal((dims[i], d, dims[i + 1]))
                                       + 1j * rng.standard_normal((dims[i], d, dims[i + 1])) for i in range(L)], be)
    v = mr.state_vector(psi.to_host())
    got = native_cplx.expectation_value(psi, mr.SY2)
    assert np.abs(got - [mr.ev1(v, mr.SY2, i) for i in range(L)]).max() < TOL
    for i in range(L - 1):        # (neighbours only: the stand-in has no complex pass-through transfer)
        assert abs(native_cplx.correlator(psi, mr.SP2, mr.SM2, i, i + 1) - mr.ev2(v, mr.SP2, i, mr.SM2, i + 1)) < TOL


def test_decompose_localmpo_round_trip():
    rng = np.random.default_rng(8)
    for d in (2, 3):
        O = rng.standard_normal((d, d, d, d))
        A, B = mk.decompose_localmpo(O)
        assert A.shape[0] == 1 and B.shape[3] == 1 and A.shape[1:3] == (d, d) and A.shape[3] == B.shape[0]
        assert np.abs(np.einsum("atsw,wurb->tusr", A, B) - O).max() < 1e-13
    O = rng.standard_normal((2,) * 6) + 1j * rng.standard_normal((2,) * 6)
    A, B, C = mk.decompose_localmpo(O)
    assert np.abs(np.einsum("atsw,wurx,xvqb->tuvsrq", A, B, C) - O).max() < 1e-13
    one, = mk.decompose_localmpo(mr.SZ2)
    assert one.shape == (1, 2, 2, 1)


def test_dispatch_tells_local_operators_from_hamiltonians(cbe, chain2):
    psi, v = chain2
    H = mk.heisenberg_XXX(0.5, be=cbe)
    envs = mk.environments(psi, H)
    assert measure.is_local_operator(mr.SZ2, None) and measure.is_local_operator([mr.SZ2] * 8, None)
    assert measure.is_local_operator(mr.heisenberg_bond(2), 3) and measure.is_local_operator(mk.decompose_localmpo(mr.heisenberg_bond(2)), np.int64(3))
    assert not measure.is_local_operator(H, envs) and not measure.is_local_operator(H, None)
    assert not measure.is_local_operator(mk.LazySum([H, H]), None) and not measure.is_local_operator([], None)
    assert not measure.is_local_operator(mr.SZ2, envs)
    ens = mk.expectation_value(psi, H, envs)                       # the old form: per-site energies of the MPO
    dense = sum(mr.ev12(v, mr.heisenberg_bond(2), i, i + 1).real for i in range(len(psi) - 1))
    assert ens.shape == (len(psi),) and abs(float(np.sum(ens)) - dense) < TOL
    emb = mk.FiniteMPS.random(4, 2, 4, np.random.default_rng(0), be=cbe, dtype=np.complex128)
    with pytest.raises(NotImplementedError, match="native_cplx"):
        mk.expectation_value(emb, mr.SZ2)
