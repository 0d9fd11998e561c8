"""The cases of tests/native_changebonds_cases.py on the device: mpsk_complement_tsvd under MPSK_C128 on planted spectra
(small route, range finder, fallback, completion, leading dimensions, NULL sides), the fp64 entry against its pinned output,
and native_cplx.changebonds on both routes.  State-level bounds are those the host run recorded in
profiles/native_changebonds_bounds.log (100 x what it measured)."""
import os

import numpy as np
import pytest

import mpskit_jl_amd as mk
import native_changebonds_cases as cs
import native_ham_inf_cases as hc

pytestmark = pytest.mark.gpu
ROUTES = ["device", "composed"]


def _log(text):
    print("NATIVE-CHANGEBONDS device " + text)


@pytest.fixture(scope="module")
def bounds():
    return cs.read_bounds()


def _run(be, name):
    case = cs.entry_case(name)
    before = be.complement_stats()
    u, s, vt = cs.device_entry(be, case)
    after = be.complement_stats()
    res = cs.check_entry(case, u, s, vt)
    _log(f"entry {name}: |S - s| / s_0 = {res['S']:.2e}, orthogonality {max(res[k] for k in ('UU', 'VV', 'QLU', 'VQR')):.2e}, "
         f"projectors {res['PU']:.2e} / {res['PV']:.2e}")
    assert after["calls"] == before["calls"] + 1
    return case, u, s, vt, {k: after[k] - before[k] for k in after}


@pytest.mark.parametrize("name", ["small_8", "small_12x9"])
def test_small_route(be, name):
    _, _, _, _, d = _run(be, name)
    assert d["full"] == 1 and d["subspace"] == 0


def test_range_finder_and_fallback_are_counted():
    """graded spectra are answered by the accepted range finder, the slowly decaying one by the full SVD; a context of its own,
    because a failed check makes the context back off for the next calls"""
    be = mk.Backend(0)
    try:
        for name in ("range_96x80", "range_80x120", "range_200x180", "range_ld", "left_none", "right_none", "rank3"):
            _, _, _, _, d = _run(be, name)
            assert d["subspace"] == 1 and d["full"] == 0, (name, d)
        _, _, _, _, d = _run(be, "flat")
        assert d["full"] == 1 and d["subspace"] == 0, d
        assert be.split_stats()["path"] == 2
        _, _, _, _, d = _run(be, "range_96x80")           # backing off: the full SVD, and still the contract
        assert d["full"] == 1 and d["subspace"] == 0, d
    finally:
        be.close()


@pytest.mark.parametrize("name", ["zero", "inside_QL"])
def test_completion_of_nothing(be, name):
    _, _, s, _, d = _run(be, name)
    assert np.all(s == 0.0) and d["full"] == 1


def test_real_operands_match_the_fp64_entry(be, bounds):
    case, u, s, _, _ = _run(be, "real_operands")
    _, s64, _ = cs.device_entry(be, case, cplx=False)
    im = np.abs((u @ u.conj().T).imag).max()
    _log(f"entry real_operands: |S_c128 - S_f64| / s_0 = {np.abs(s - s64).max() / s64[0]:.2e}, |Im U U^H| = {im:.2e} "
         f"(bound {bounds['real_operands_imag']:.2e})")
    assert np.abs(s - s64).max() <= cs.S_BAR * s64[0]
    assert im <= bounds["real_operands_imag"]


def test_refuses_non_finite_and_side_sections(be):
    case = cs.entry_case("small_8")
    case["Y"] = case["Y"].copy()
    case["Y"][1, 2] = np.nan
    with pytest.raises(mk.MpskError, match="mpsk_complement_tsvd: Y is not finite"):
        cs.device_entry(be, case)
    good = cs.entry_case("small_8")
    be.side_mark()
    be.side_begin()
    try:
        with pytest.raises(mk.MpskError, match="side-stream"):
            cs.device_entry(be, good)
    finally:
        be.side_end()
    cs.check_entry(good, *cs.device_entry(be, good))


def test_fp64_entry_is_bit_identical():
    """the fp64 entry on one planted case against its output on the commit before the complex entry existed"""
    if not os.path.exists(cs.F64_GOLDEN):
        pytest.fail("tests/golden/complement_tsvd_f64.npz is missing")
    gold = np.load(cs.F64_GOLDEN)
    u, s, vt = cs.f64_golden_run()
    assert np.array_equal(s, gold["S"]) and np.array_equal(u, gold["U"]) and np.array_equal(vt, gold["Vt"])


@pytest.mark.parametrize("n,D", cs.STATE_SIZES)
@pytest.mark.parametrize("kind", ["optimal", "random"])
@pytest.mark.parametrize("route", ROUTES)
def test_gauge_and_size(be, bounds, n, D, kind, route):
    res, dot = cs.case_gauge(be, n, D, kind, route)
    _log(f"gauge n = {n}, D = {D}, {kind}, {route}: residual {res:.2e} (bound {bounds[f'gauge_{n}_{D}']:.2e}), "
         f"||dot| - 1| = {dot:.2e} (bound {bounds[f'dot_{n}_{D}']:.2e})")
    assert res <= bounds[f"gauge_{n}_{D}"] and dot <= bounds[f"dot_{n}_{D}"]


@pytest.mark.parametrize("n,D", cs.STATE_SIZES)
def test_singular_values_match_the_literal_algorithm(be, n, D):
    worst, between = cs.case_singular_values(be, n, D, ROUTES)
    _log(f"singular values n = {n}, D = {D}: |S - S_literal| / S_0 = {worst:.2e}, device against composed {between:.2e}")
    assert worst <= cs.S_BAR and between <= cs.S_BAR


@pytest.mark.parametrize("route", ROUTES)
def test_real_groundstate_matches_the_real_state(be, route):
    worst, s0, ynorm = cs.case_real_groundstate(be, 1, 4, route)
    bar = cs.real_groundstate_bar(s0, ynorm)
    _log(f"real ground state D = 4, {route}: |S_c - S_r| = {worst:.2e}, S_0 = {s0:.2e}, |Y| = {ynorm:.2e} (bar {bar:.2e})")
    assert worst <= bar


@pytest.mark.parametrize("n,D", cs.STATE_SIZES[:2])
def test_svdcut_returns_the_state(be, bounds, n, D):
    for route in ROUTES:
        dot, ds = cs.case_svdcut(be, n, D, route)
        _log(f"SvdCut n = {n}, D = {D}, {route}: ||dot| - 1| = {dot:.2e}, |d Schmidt| = {ds:.2e}")
        assert dot <= bounds["svdcut_dot"] and ds <= bounds["svdcut_schmidt"]


def test_growing_lowers_the_energy(be):
    E4, E8, eps, E_ref = cs.case_growing(be, route="device")
    _log(f"growing D = 4 -> 8: E4 = {E4.real:.12f}, E8 = {E8.real:.12f}, real VUMPS at D = 8 {E_ref:.12f}, galerkin {eps:.2e}")
    hc.check_vumps(E8, eps, E_ref)
    assert E8.real < E4.real


@pytest.mark.parametrize("route", ROUTES)
def test_expansion_does_not_move_the_energy(be, bounds, route):
    moved, drift = cs.case_real_time(be, route)
    _log(f"real time D = 4 -> 6, {route}: |E after - E before| = {moved:.2e} (bound {bounds['real_time_energy']:.2e}), "
         f"drift over 10 steps {drift:.2e}")
    assert moved <= bounds["real_time_energy"]


def test_refusals(be):
    cs.case_refusals(be)
