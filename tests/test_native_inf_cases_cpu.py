"""The cases of tests/native_inf_cases.py without a GPU: the exactness guard and the discriminating power of the
mpsk_dC_proj_c reference, and the host logic of NativeInfiniteMPS / NativePerMPOInfEnv / the VOMPS approximate on the complex
NumPy stand-in (tests/cpu_backend_inf.py).  The NATIVE-INF lines (`pytest -s`) are the figures kept in
profiles/native_inf_bounds.log."""
import numpy as np
import pytest

import mpskit_jl_amd as mk
import native_inf_cases as cs
from cpu_backend_inf import CpuInfBackend
from mpskit_jl_amd import native_cplx as nc


def _log(text):
    print("NATIVE-INF host " + text)


@pytest.fixture(scope="module")
def cbe():
    return CpuInfBackend()


@pytest.mark.parametrize("shape", cs.DC_SHAPES, ids=str)
def test_reference_is_exact_in_any_bracket_order(shape):
    GL, GR, c = cs.dc_operands(shape)
    for x in (GL, GR, c):
        assert np.abs(x.real).max() <= 3 and np.abs(x.imag).max() <= 3
    yr, yi, bound = cs.dc_guard(GL, GR, c)
    assert bound < 2.0 ** 53                      # every partial sum of every ordering is an integer below 2^53
    ref = cs.dc_ref(GL, GR, c)
    assert np.array_equal(ref.real.astype(np.longdouble), yr) and np.array_equal(ref.imag.astype(np.longdouble), yi)
    other = np.einsum("wbq,wpb->pq", GR, np.einsum("wpa,ab->wpb", GL, c))          # another bracket order, the same bits
    assert np.array_equal(other, ref)


@pytest.mark.parametrize("shape", cs.DC_SHAPES, ids=str)
@pytest.mark.parametrize("wrong", sorted(cs.DC_WRONG))
def test_reference_tells_wrong_contractions_apart(shape, wrong):
    GL, GR, c = cs.dc_operands(shape)
    assert not np.array_equal(cs.DC_WRONG[wrong](GL, GR, c), cs.dc_ref(GL, GR, c))


@pytest.mark.parametrize("shape", cs.DC_SHAPES, ids=str)
def test_composed_c_proj_on_the_stand_in(cbe, shape):
    GL, GR, c = cs.dc_operands(shape)
    gl, gr, cm = cs.slabs_c(cbe, GL), cs.slabs_c(cbe, GR), cbe.upload_c(c)
    ref = cs.dc_ref(GL, GR, c)
    assert np.array_equal(cbe.download_c(nc.dC_proj_c_composed(cbe, gl, gr, cm)), ref)
    assert np.array_equal(cbe.download_c(cbe.dC_proj_c(gl, gr, cm)), ref)


def test_split_join_round_trip_on_the_stand_in(cbe):
    z = cbe.upload_c(cs.gauss_int(np.random.default_rng(5), (7, 3)))
    p = cbe.split_c(z)
    assert np.array_equal(p.buf[:21].numpy(), cbe.download_c(z).real.ravel(order="F"))
    assert np.array_equal(cbe.join_c(p, z.shape).buf.numpy(), z.buf.numpy())


@pytest.mark.parametrize("n,D", [(1, 4), (2, 5), (1, 6)])
def test_gauge_contract(cbe, n, D):
    _, worst = cs.case_gauge(cbe, n, D, seed=30 + n)
    _log(f"gauge contract n = {n}, D = {D}: |AL CR - CR AR| / |AC| = {worst:.3e} at gauge tolerance 1e-12")


@pytest.mark.parametrize("n,D", [(1, 4), (2, 6)])
def test_dot_with_itself_is_one(cbe, n, D):
    cs.case_dot_self(cbe, n, D, seed=40 + n)


@pytest.mark.parametrize("n", [1, 2])
def test_imaginary_time_parity_and_real_time(cbe, n):
    r = cs.case_imag_parity(cbe, n, log=_log)
    assert cbe.calls.get("dC_proj_c", 0) > 0                       # the fused route is the default where the backend has it
    cs.case_real_time(cbe, n, r["b_dot"], log=_log)


def test_forced_routes_of_c_proj(cbe):
    before = cbe.calls.get("dC_proj_c", 0)
    r = cs.case_imag_parity(cbe, 1, device=False)
    assert cbe.calls.get("dC_proj_c", 0) == before                 # composed: gemm_c pairs and axpby only
    cs.case_real_time(cbe, 1, r["b_dot"], device=True)
    assert cbe.calls.get("dC_proj_c", 0) > before

    class NoFused:
        pass
    with pytest.raises(mk.MpskError, match="dC_proj_c"):
        nc._c_proj_route(NoFused(), True)
    assert nc._c_proj_route(NoFused(), None) is False


def test_from_real_keeps_the_gauge_and_expectation_values(cbe):
    psi = mk.InfiniteMPS.random(2, 4, np.random.default_rng(3), n=2, be=cbe)
    nat = nc.NativeInfiniteMPS.from_real(psi)
    h = nat.to_host()
    for k in ("AL", "AR", "AC", "CR"):
        for t, ref in zip(h[k], getattr(psi, k)):
            assert np.array_equal(t, cbe.download(ref).astype(np.complex128))
    Z = np.diag([1.0, -1.0])
    Y = np.array([[0, -1j], [1j, 0]])
    for op in (Z, Y):
        got = nc.expectation_value(nat, op)
        want = [np.einsum("ptb,ts,psb->", np.conj(a), op, a) for a in h["AC"]]
        assert np.allclose(got, want, rtol=0, atol=1e-14)
    with pytest.raises(TypeError):
        nc.NativeInfiniteMPS.from_real(nat)


def test_make_time_mpo_storage(cbe):
    H = mk.transverse_field_ising(1.0, 0.7, be=cbe)
    for alg in (mk.WII(), mk.WI()):
        real, cplx = mk.make_time_mpo(H, -0.05j, alg), mk.make_time_mpo(H, 0.05, alg)
        assert isinstance(real, mk.SparseMPO) and not real.cplx
        assert all(np.isrealobj(np.asarray(v)) for blk in real.data for v in blk.values())
        assert isinstance(cplx, mk.SparseMPO) and cplx.cplx
        mixed = mk.make_time_mpo(H, 0.05 - 0.01j, alg)
        assert mixed.cplx


def test_out_of_scope_is_refused_by_name(cbe):
    psi = nc.NativeInfiniteMPS.random(2, 4, np.random.default_rng(1), be=cbe)
    O = cs.tfi_time_mpo(cbe, 0.05)
    with pytest.raises(NotImplementedError, match="DenseMPO"):
        mk.approximate(psi, (mk.classical_ising(), psi), mk.VOMPS())
    with pytest.raises(NotImplementedError, match="MPSMultiline"):
        nc.NativePerMPOInfEnv(psi, (O, mk.MPSMultiline.__new__(mk.MPSMultiline)))
    for alg in (mk.IDMRG1(), mk.IDMRG2()):
        with pytest.raises(NotImplementedError, match=type(alg).__name__):
            mk.approximate(psi, (O, psi), alg)
    with pytest.raises(NotImplementedError, match="leading_boundary"):
        mk.leading_boundary(psi, mk.classical_ising())
    with pytest.raises(NotImplementedError, match="changebonds"):
        mk.changebonds(psi, mk.RandExpand())
    emb = mk.InfiniteMPS.random(2, 2, np.random.default_rng(2), be=cbe)
    emb.cplx = True
    with pytest.raises(NotImplementedError, match="NativeInfiniteMPS"):
        mk.approximate(emb, (mk.make_time_mpo(mk.transverse_field_ising(1.0, 0.7, be=cbe), -0.05j), emb), mk.VOMPS())


def test_planar_arnoldi_out_of_restarts_returns_its_last_ritz_pair(cbe):
    """the uniform gauge asks eigsolve_lm_planar for a tolerance it may not reach within its few restarts: the solver must
    then return the Ritz pair of its last factorisation (residual as reported), with a warning, instead of failing"""
    from mpskit_jl_amd import krylov
    rng = np.random.default_rng(8)
    N = 40
    M = rng.standard_normal((N, N)) + 1j * rng.standard_normal((N, N))

    def mv(p, out):
        v = cbe.download(p)
        w = M @ (v[:N] + 1j * v[N:])
        return cbe._set(out, np.concatenate([w.real, w.imag]))

    x0 = cbe.upload(rng.standard_normal(2 * N))
    with pytest.warns(UserWarning, match="converged"):
        vals, vecs, res, conv = krylov.eigsolve_lm_planar(cbe, mv, x0, num=1, tol=1e-300, krylovdim=8, maxiter=2)
    assert conv == 0
    v = cbe.download(vecs[0])
    z = v[:N] + 1j * v[N:]
    assert abs(np.linalg.norm(z) - 1.0) <= 1e-13
    assert abs(np.linalg.norm(M @ z - vals[0] * z) - res[0]) <= 1e-10 * np.abs(M).sum()


def test_gauge_contract_through_the_eigenvector_step(cbe):
    """a slowly mixing cell (two nearly decoupled blocks): the plain sweeps are not enough, the Arnoldi step of the gauge runs"""
    rng = np.random.default_rng(12)
    D = 6
    A = np.zeros((D, 2, D), dtype=complex)
    A[:3, :, :3] = rng.standard_normal((3, 2, 3)) + 1j * rng.standard_normal((3, 2, 3))
    A[3:, :, 3:] = rng.standard_normal((3, 2, 3)) + 1j * rng.standard_normal((3, 2, 3))
    A += 1e-3 * (rng.standard_normal((D, 2, D)) + 1j * rng.standard_normal((D, 2, D)))
    before = cbe.calls.get("transfer_left_c", 0)
    psi = nc.NativeInfiniteMPS([A], be=cbe, tol=1e-12)
    assert cbe.calls.get("transfer_left_c", 0) > before
    h = psi.to_host()
    al, ar, c = h["AL"][0], h["AR"][0], h["CR"][0]
    assert cs.relnorm(np.einsum("asb,asc->bc", al.conj(), al), np.eye(D)) <= 1e-12
    assert cs.relnorm(np.einsum("ab,bsc->asc", c, ar), np.einsum("asb,bc->asc", al, c)) <= 1e-12
