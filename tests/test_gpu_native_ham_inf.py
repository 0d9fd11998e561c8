"""The cases of tests/native_ham_inf_cases.py on the device, on both routes of the regulariser (device=True:
mpsk_regularize_axpby, device=False: composed).  The parity bounds are those the host run recorded in
profiles/native_ham_inf_bounds.log (100 x the difference it measured at the same solver tolerance)."""
import numpy as np
import pytest

import native_ham_inf_cases as cs
from mpskit_jl_amd import native_cplx as nc

pytestmark = pytest.mark.gpu
ROUTES = [True, False]
IDS = ["fused", "composed"]


def _log(text):
    print("NATIVE-HAM-INF device " + text)


@pytest.fixture(scope="module")
def bounds():
    return cs.read_bounds()


@pytest.mark.parametrize("n,D", cs.SIZES)
def test_environment_parity_on_both_routes(be, bounds, n, D):
    b = bounds[f"env_{n}_{D}"]
    envs = {}
    for device in ROUTES:
        worst, imag, envs[device] = cs.case_env_parity(be, n, D, device=device)
        _log(f"environment parity n = {n}, D = {D}, {'fused' if device else 'composed'}: |Re native - real| / |level| = "
             f"{worst:.3e}, |Im| / |level| = {imag:.3e} (bound {b:.3e})")
        assert worst <= b and imag <= b, (worst, imag, b)
    diff = cs.route_difference(be, envs[True], envs[False], n)
    _log(f"environment parity n = {n}, D = {D}: fused against composed {diff:.3e}")
    assert diff <= b, (diff, b)
    assert nc._reg_route(be, None) is nc.REG_FUSED_DEFAULT


@pytest.mark.parametrize("n,D", cs.SIZES)
def test_vumps_complex_hamiltonian(be, n, D):
    E, eps, E_ref, _, _ = cs.case_vumps(be, n, D, complex_h=True)
    _log(f"VUMPS Y-field n = {n}, D = {D}: E = {E.real:.14f} {E.imag:+.1e}i, real VUMPS {E_ref:.14f}, galerkin {eps:.2e}")
    cs.check_vumps(E, eps, E_ref)


def test_vumps_unit_cells_agree(be):
    E1 = cs.case_vumps(be, 1, 8, complex_h=True)[0]
    E2 = cs.case_vumps(be, 2, 8, complex_h=True)[0]
    assert abs(E1 - E2) <= 1e-10 * abs(E1), (E1, E2)


@pytest.mark.parametrize("n,D", cs.SIZES[:2])
def test_vumps_real_hamiltonian_from_complex_start(be, n, D):
    E, eps, E_ref, _, _ = cs.case_vumps(be, n, D, complex_h=False)
    cs.check_vumps(E, eps, E_ref)


@pytest.mark.parametrize("device", ROUTES, ids=IDS)
@pytest.mark.parametrize("n,D", cs.SIZES[:2])
def test_quench_against_the_embedded_route(be, bounds, n, D, device):
    d_obs, d_dot, drift_n, drift_e = cs.case_quench(be, n, D, device=device)
    b_obs, b_dot = bounds[f"quench_obs_{n}_{D}"], bounds[f"quench_dot_{n}_{D}"]
    _log(f"quench n = {n}, D = {D}, {'fused' if device else 'composed'}: max |d(E, X, Z)| = {d_obs:.3e} (bound {b_obs:.3e}), max "
         f"||dot| - 1| = {d_dot:.3e} (bound {b_dot:.3e}), energy drift native {drift_n:.3e}, embedded {drift_e:.3e}")
    assert d_obs <= b_obs and d_dot <= b_dot, (d_obs, b_obs, d_dot, b_dot)
    assert drift_n <= 10 * drift_e, (drift_n, drift_e)


def test_groundstate_is_stationary(be):
    moved, eps = cs.case_stationary(be, 1, 8)
    _log(f"stationarity n = 1, D = 8: |d<X>| after 5 steps = {moved:.3e}, galerkin error {eps:.3e}")
    assert moved <= eps


def test_imaginary_step_lowers_the_energy(be):
    e0, e1 = cs.case_imaginary_step(be, 2, 8)
    assert e1 < e0, (e0, e1)


def test_refusals(be):
    cs.case_refusals(be)


def test_restart_after_the_bonds_change(be):
    cs.case_restart_after_bond_change(be)


def test_fused_route_makes_the_recorded_calls(be):
    """one construction at n = 2, D = 4 on the fused route of the regulariser (it has no host stand-in): the backend calls of
    tests/golden/ham_inf_env_calls.json, in that order (tests/test_ham_inf_env_calls_cpu.py holds the other sections)"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    import make_ham_inf_env_calls as gen
    got = gen.record_device(be)[gen.DEVICE_SECTION]
    assert any(c.startswith("regularize_axpby(") for c in got)
    diff = gen.first_difference(got, gen.load()[gen.DEVICE_SECTION])
    assert diff is None, diff
