"""The cases of tests/native_ham_inf_cases.py on the NumPy stand-in (tests/cpu_backend_ham_inf.py): NativeMPOHamInfEnv on the
composed route of the regulariser, VUMPS and TDVP on a NativeInfiniteMPS.  Every bar of the cases is met on the host; what
was measured goes to profiles/native_ham_inf_bounds.log (rewritten when the whole module has run), from which the device
tests read their bounds."""
import numpy as np
import pytest

import mpskit_jl_amd as mk
import native_ham_inf_cases as cs
from cpu_backend_ham_inf import CpuHamInfBackend
from mpskit_jl_amd import native_cplx as nc

_records, _lines = {}, []
EXPECTED = {f"env_{n}_{D}" for n, D in cs.SIZES} | {f"quench_obs_{n}_{D}" for n, D in cs.SIZES[:2]} \
    | {f"quench_dot_{n}_{D}" for n, D in cs.SIZES[:2]}


def _log(text):
    print("NATIVE-HAM-INF host " + text)
    _lines.append(text)


@pytest.fixture(scope="module")
def cbe():
    be = CpuHamInfBackend()
    assert not hasattr(be, "regularize_axpby")            # the stand-in takes the composed route
    yield be
    if set(_records) == EXPECTED:                         # the whole module ran: the file is complete
        cs.write_bounds(_records, _lines)


@pytest.mark.parametrize("n,D", cs.SIZES)
def test_environment_parity(cbe, n, D):
    worst, imag, env = cs.case_env_parity(cbe, n, D)
    _records[f"env_{n}_{D}"] = worst
    _log(f"environment parity n = {n}, D = {D}: |Re native - real| / |level| = {worst:.3e}, |Im| / |level| = {imag:.3e} at solver "
         f"tolerance {cs.ENV_TOL:g} ({env.n_reg} operator applications)")
    assert imag <= cs.MARGIN * worst
    assert worst <= 1e-10                                  # both classes solve to 1e-12: they cannot differ by more


@pytest.mark.parametrize("n,D", cs.SIZES)
def test_vumps_complex_hamiltonian(cbe, n, D):
    E, eps, E_ref, _, _ = cs.case_vumps(cbe, n, D, complex_h=True)
    _log(f"VUMPS Y-field n = {n}, D = {D}: E = {E.real:.14f} {E.imag:+.1e}i, real VUMPS {E_ref:.14f}, galerkin {eps:.2e}")
    cs.check_vumps(E, eps, E_ref)


def test_vumps_unit_cells_agree(cbe):
    E1 = cs.case_vumps(cbe, 1, 8, complex_h=True)[0]
    E2 = cs.case_vumps(cbe, 2, 8, complex_h=True)[0]
    assert abs(E1 - E2) <= 1e-10 * abs(E1), (E1, E2)


@pytest.mark.parametrize("n,D", cs.SIZES[:2])
def test_vumps_real_hamiltonian_from_complex_start(cbe, n, D):
    E, eps, E_ref, _, _ = cs.case_vumps(cbe, n, D, complex_h=False)
    _log(f"VUMPS real H n = {n}, D = {D}: E = {E.real:.14f} {E.imag:+.1e}i, real VUMPS {E_ref:.14f}, galerkin {eps:.2e}")
    cs.check_vumps(E, eps, E_ref)


@pytest.mark.parametrize("n,D", cs.SIZES[:2])
def test_quench_against_the_embedded_route(cbe, n, D):
    d_obs, d_dot, drift_n, drift_e = cs.case_quench(cbe, n, D)
    _records[f"quench_obs_{n}_{D}"] = d_obs
    _records[f"quench_dot_{n}_{D}"] = d_dot
    _log(f"quench n = {n}, D = {D}, 10 steps of 0.05: max |d(E, X, Z)| = {d_obs:.3e}, max ||dot| - 1| = {d_dot:.3e}, energy drift "
         f"native {drift_n:.3e}, embedded {drift_e:.3e}")
    assert drift_n <= 10 * drift_e, (drift_n, drift_e)
    assert d_obs <= 1e-8 and d_dot <= 1e-8                 # the two routes run the same algorithm at tolerance 1e-12


def test_groundstate_is_stationary(cbe):
    moved, eps = cs.case_stationary(cbe, 1, 8)
    _log(f"stationarity n = 1, D = 8: |d<X>| after 5 steps = {moved:.3e}, galerkin error {eps:.3e}")
    assert moved <= eps


def test_imaginary_step_lowers_the_energy(cbe):
    e0, e1 = cs.case_imaginary_step(cbe, 2, 8)
    assert e1 < e0, (e0, e1)


def test_refusals(cbe):
    cs.case_refusals(cbe)


def test_restart_after_the_bonds_change(cbe):
    cs.case_restart_after_bond_change(cbe)


def test_route_switch(cbe):
    class Fused:
        def regularize_axpby(self):
            pass
    assert nc._reg_route(cbe, None) is False and nc._reg_route(cbe, False) is False
    with pytest.raises(mk.MpskError, match="regularize_axpby"):
        nc._reg_route(cbe, True)
    assert nc._reg_route(Fused(), None) is nc.REG_FUSED_DEFAULT and nc._reg_route(Fused(), False) is False


def test_composed_regulariser_is_the_exact_contraction(cbe):
    """the composed route (one dotc with conj(lvec^T), axpby_c) against the exact reference of mpsk_regularize_axpby"""
    import regularize_axpby_cases as rc
    shape = (2, 33, 31)
    t = rc.operands(shape, True)
    op = nc._RegOp(cbe, lambda v: rc.slabs(cbe, t["y"], True), cbe.upload_c(t["lvec"]), cbe.upload_c(t["rvec"]), fused=False)
    x = rc.slabs(cbe, t["x"], True)
    out = op(x, cbe.empty(*x.shape))
    got = rc.unflat(out.buf[:out.size].numpy(), shape, True)
    assert np.array_equal(got, rc.ref(t["y"], t["lvec"], t["rvec"], -1.0, t["x"], 1.0))
    v = rc.slabs(cbe, t["y"], True)
    op.project(v)
    assert np.array_equal(rc.unflat(v.buf[:v.size].numpy(), shape, True), rc.ref(t["y"], t["lvec"], t["rvec"], 1.0))
