"""The cases of tests/native_changebonds_cases.py on the NumPy stand-ins: the reference of every entry-level case meets every
bar of the contract with margin, and native_cplx.changebonds runs both routes on the host (the "device" route against the
NumPy reference of mpsk_complement_tsvd).  What was measured goes to profiles/native_changebonds_bounds.log (rewritten when
the whole module has run), from which the device tests read their bounds."""
import numpy as np
import pytest

import mpskit_jl_amd as mk
import native_changebonds_cases as cs
import native_ham_inf_cases as hc
from mpskit_jl_amd import native_cplx as nc

_records, _lines = {}, []
ROUTES = ["device", "composed"]
EXPECTED = {f"gauge_{n}_{D}" for n, D in cs.STATE_SIZES} | {f"dot_{n}_{D}" for n, D in cs.STATE_SIZES} \
    | {"real_operands_imag", "svdcut_dot", "svdcut_schmidt", "real_time_energy"}
HOST_MARGIN = 10.0                    # the NumPy reference sits at least this far inside every bar of the contract


def _log(text):
    print("NATIVE-CHANGEBONDS host " + text)
    _lines.append(text)


def _rec(name, value, floor):
    old = _records.get(name, (0.0, floor))
    _records[name] = (max(old[0], float(value)), floor)


@pytest.fixture(scope="module")
def cbe():
    be = cs.CpuChangebondsDeviceBackend()
    yield be
    if set(_records) == EXPECTED:                         # the whole module ran: the file is complete
        cs.write_bounds(_records, _lines)


@pytest.mark.parametrize("name", cs.ENTRY_CASES)
def test_entry_reference_meets_the_contract_with_margin(name):
    case = cs.entry_case(name)
    u, s, vt = cs.host_entry(case)
    res = cs.check_entry(case, u, s, vt)
    bar = cs.projector_bar(case)
    _log(f"entry {name}: |S - s| / s_0 = {res['S']:.2e}, orthogonality {max(res[k] for k in ('UU', 'VV', 'QLU', 'VQR')):.2e}, "
         f"projectors {res['PU']:.2e} / {res['PV']:.2e} (bar {bar if bar is None else format(bar, '.2e')})")
    assert res["S"] <= cs.S_BAR / HOST_MARGIN
    assert max(res[k] for k in ("UU", "VV", "QLU", "VQR")) <= cs.ORTH_BAR / HOST_MARGIN
    if bar is not None:
        assert max(res["PU"], res["PV"]) <= bar / HOST_MARGIN
    if name in ("zero", "inside_QL"):
        assert np.all(s == 0.0)
    if name == "flat":                                     # what the module docstring claims about the fixed iteration count
        sig = 1.0 - np.arange(76) / 256.0
        assert (sig[72] / sig[7]) ** 9 > 1e-2
    if name == "real_operands":
        # the imaginary part of U U^H on real operands: rounding level on the host; the device bound is 100 x this figure
        im = max(np.abs((u @ u.conj().T).imag).max(), EPS_FLOOR)
        _rec("real_operands_imag", im, EPS_FLOOR)
        _log(f"entry real_operands: |Im U U^H| = {im:.2e}")


EPS_FLOOR = 1e-15                     # one rounding error of entries of size one


def test_zero_threshold_is_below_every_planted_value():
    for name in cs.ENTRY_CASES:
        case = cs.entry_case(name)
        if case["rank"]:
            assert case["sig"][case["rank"] - 1] > 1e3 * cs.zero_threshold(case["Y"]), name


@pytest.mark.parametrize("n,D", cs.STATE_SIZES)
@pytest.mark.parametrize("kind", ["optimal", "random"])
@pytest.mark.parametrize("route", ROUTES)
def test_gauge_and_size(cbe, n, D, kind, route):
    res, dot = cs.case_gauge(cbe, n, D, kind, route)
    _rec(f"gauge_{n}_{D}", res, EPS_FLOOR)
    _rec(f"dot_{n}_{D}", dot, 1e-12)                       # native_cplx.dot solves its eigenvalue to 1e-12
    _log(f"gauge n = {n}, D = {D}, {kind}, {route}: residual {res:.2e}, ||dot| - 1| = {dot:.2e}")
    assert res <= 1e-13 and dot <= 1e-10


@pytest.mark.parametrize("n,D", cs.STATE_SIZES)
def test_singular_values_match_the_literal_algorithm(cbe, n, D):
    worst, between = cs.case_singular_values(cbe, n, D, ROUTES)
    _log(f"singular values n = {n}, D = {D}: |S - S_literal| / S_0 = {worst:.2e}, device against composed {between:.2e}")
    assert worst <= cs.S_BAR / HOST_MARGIN and between <= cs.S_BAR / HOST_MARGIN


@pytest.mark.parametrize("route", ROUTES)
def test_real_groundstate_matches_the_real_state(cbe, route):
    worst, s0, ynorm = cs.case_real_groundstate(cbe, 1, 4, route)
    _log(f"real ground state D = 4, {route}: |S_c - S_r| = {worst:.2e}, S_0 = {s0:.2e}, |Y| = {ynorm:.2e} "
         f"(bar {cs.real_groundstate_bar(s0, ynorm):.2e})")
    assert worst <= cs.real_groundstate_bar(s0, ynorm) / HOST_MARGIN


@pytest.mark.parametrize("n,D", cs.STATE_SIZES[:2])
def test_svdcut_returns_the_state(cbe, n, D):
    for route in ROUTES:
        dot, ds = cs.case_svdcut(cbe, n, D, route)
        _rec("svdcut_dot", dot, 1e-12)
        _rec("svdcut_schmidt", ds, EPS_FLOOR)
        _log(f"SvdCut n = {n}, D = {D}, {route}: ||dot| - 1| = {dot:.2e}, |d Schmidt| = {ds:.2e}")
        assert dot <= 1e-10 and ds <= 1e-12


def test_growing_lowers_the_energy(cbe):
    E4, E8, eps, E_ref = cs.case_growing(cbe)
    _log(f"growing D = 4 -> 8: E4 = {E4.real:.12f}, E8 = {E8.real:.12f}, real VUMPS at D = 8 {E_ref:.12f}, galerkin {eps:.2e}")
    hc.check_vumps(E8, eps, E_ref)
    assert E8.real < E4.real


def test_expansion_does_not_move_the_energy(cbe):
    for route in ROUTES:
        moved, drift = cs.case_real_time(cbe, route)
        _rec("real_time_energy", moved, 1e-12)             # the environments behind the energy are solved to 1e-12
        _log(f"real time D = 4 -> 6, {route}: |E after - E before| = {moved:.2e}, drift over 10 steps {drift:.2e}")
        assert moved <= 1e-10


def test_refusals(cbe):
    cs.case_refusals(cbe)


def test_dispatch(cbe):
    plain = cs.CpuChangebondsBackend()
    assert nc._expand_route(plain, 512, 512, None) is False and nc._expand_route(plain, 512, 512, "composed") is False
    with pytest.raises(mk.MpskError, match="complement_tsvd_c"):
        nc._expand_route(plain, 512, 512, "device")
    from mpskit_jl_amd.changebonds import DEVICE_ROUTE_MIN
    assert nc._expand_route(cbe, DEVICE_ROUTE_MIN, 512, None) is False                    # small tensors: composed
    assert nc._expand_route(cbe, DEVICE_ROUTE_MIN + 1, 512, None) is nc.EXPAND_DEVICE_DEFAULT
    assert nc._expand_route(cbe, 8, 8, "device") is True
    # a backend without the entry still expands (composed route)
    psi = cs.random_state(plain, 1, 4)
    new = nc.changebonds(psi, mk.RandExpand(trunc_dim=2))
    assert new.dims(0) == (6, 2, 6) and "complement_tsvd_c" not in plain.calls and plain.calls["tsvd_c"] >= 1
