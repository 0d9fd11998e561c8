"""FiniteMPS / NativeFiniteMPS linear algebra (linalg.py) on the host stand-in backends, composed route: psi1 + psi2,
psi1 - psi2, a * psi, normalize, dot against the oracle's dense vectors.  Cases, references and the tolerance rule:
finite_linalg_cases.py (e0 measured on the stand-in)."""
import numpy as np
import pytest

import mpskit_jl_amd as mk
from mpskit_jl_amd import linalg
from mpskit_jl_amd.native_cplx import NativeFiniteMPS
from cpu_backend import CpuBackend, CpuComplexBackend

import finite_linalg_cases as fc


@pytest.fixture(scope="module", params=[(k, ch) for k in fc.KINDS for ch in fc.CHAINS],
                ids=[f"{k}-{i}" for k in fc.KINDS for i in fc.CHAIN_IDS])
def case(request):
    kind, chain = request.param
    return fc.Case(CpuComplexBackend() if kind == "native" else CpuBackend(), kind, chain)


def test_stand_in_takes_the_composed_route(case):
    assert not hasattr(case.be, "dsum_site")
    if case.kind != "native":
        with pytest.raises(mk.MpskError):
            linalg.add(case.psi1, case.psi2, fused=True)


def test_sum_and_difference(case):
    fc.check_sum_and_difference(case)


def test_scalars_and_normalize(case):
    fc.check_scalars(case)


def test_canonical_form_of_the_sum(case):
    fc.check_canonical_form(case)


def test_overlap(case):
    fc.check_overlap(case)


def test_norms(case):
    fc.check_norms(case)


def test_real_next_to_embedded():
    fc.check_mixed_overlap(CpuBackend(), fc.CHAINS[0])


def test_rectangular_centre():
    """odd L with bonds that still grow at the centre: the centre matrix of the sum is 4 x 8"""
    c = fc.Case(CpuBackend(), "real", (5, 2, 8, 8))
    s = c.psi1 + c.psi2
    assert s.CLs[2].shape == (4, 8) and fc.sum_bond_dims(5, 2, 8, 8)[1] == (4, 8)
    fc.check_canonical_form(c)
    fc.check_norms(c)


def test_length_two():
    for kind in fc.KINDS:
        c = fc.Case(CpuComplexBackend(), kind, (2, 3, 4, 4))
        c.close_vec(fc.vec(c.psi1 + c.psi2), c.v1 + c.v2, "L = 2")
        c.close_scalar(linalg.dot(c.psi1, c.psi2), np.vdot(c.v1, c.v2), "L = 2 dot")


def test_site_steps_against_einsum():
    """dsum_left / dsum_right (composed) are the block products of the issue, also with a gauge factor that is not [1 1]"""
    be, rng = CpuBackend(), np.random.default_rng(5)
    Dn, D1, D2, E1, E2, d = 5, 3, 4, 2, 6, 3
    A1, A2 = rng.standard_normal((D1, d, E1)), rng.standard_normal((D2, d, E2))
    G = rng.standard_normal((Dn, D1 + D2))
    out = be.download(linalg.dsum_left(be, be.upload(G), be.upload(A1), be.upload(A2)))
    ref = np.concatenate([np.einsum("na,asb->nsb", G[:, :D1], A1), np.einsum("na,asb->nsb", G[:, D1:], A2)], axis=2)
    assert np.allclose(out, ref, rtol=0, atol=1e-13)
    G = rng.standard_normal((E1 + E2, Dn))
    out = be.download(linalg.dsum_right(be, be.upload(G), be.upload(A1), be.upload(A2)))
    ref = np.concatenate([np.einsum("asb,bn->asn", A1, G[:E1]), np.einsum("asb,bn->asn", A2, G[E1:])], axis=0)
    assert np.allclose(out, ref, rtol=0, atol=1e-13)


def test_dispatch_and_errors():
    be, rng = CpuComplexBackend(), np.random.default_rng(2)
    a = mk.FiniteMPS.random(6, 2, 4, rng, be=be)
    with pytest.raises(ValueError, match="Cannot add states of length 6 and 5"):
        a + mk.FiniteMPS.random(5, 2, 4, rng, be=be)
    with pytest.raises(ValueError, match="different length"):
        mk.dot(a, mk.FiniteMPS.random(5, 2, 4, rng, be=be))
    with pytest.raises(ValueError, match="physical dimensions"):
        a + mk.FiniteMPS.random(6, 3, 4, rng, be=be)
    with pytest.raises(ValueError, match="physical dimensions"):
        mk.dot(a, mk.FiniteMPS.random(6, 3, 4, rng, be=be))
    with pytest.raises(ValueError, match="two backends"):
        a + mk.FiniteMPS.random(6, 2, 4, rng, be=CpuBackend())
    with pytest.raises(ValueError, match="length < 2"):
        one = mk.FiniteMPS([rng.random((1, 2, 1))], be=be)
        one + one
    with pytest.raises(TypeError, match="complex number"):
        1j * a
    with pytest.raises(ValueError, match="real and a complex"):
        a + mk.FiniteMPS.random(6, 2, 4, rng, be=be, dtype=np.complex128)
    with pytest.raises(TypeError):
        a + 1.0
    with pytest.raises(TypeError):
        a * "x"
    n = NativeFiniteMPS(fc.host_tensors(6, 2, 4, rng, True), be)
    with pytest.raises(TypeError):
        mk.dot(a, n)
    with pytest.raises(TypeError):
        a + n
    with pytest.raises(ValueError, match="length"):
        n + NativeFiniteMPS(fc.host_tensors(5, 2, 4, rng, True), be)
    assert isinstance(np.float64(2.0) * a, mk.FiniteMPS) and isinstance(np.float64(2.0) * n, NativeFiniteMPS)
    # every earlier dispatch of mk.dot keeps its behaviour
    with pytest.raises(TypeError, match="InfiniteMPS"):
        mk.dot(a, 3)
    assert mk.normalize is linalg.normalize and mk.linalg is linalg
