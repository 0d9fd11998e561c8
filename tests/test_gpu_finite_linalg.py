"""FiniteMPS / NativeFiniteMPS linear algebra (linalg.py) on the device: psi1 + psi2 on the fused route (mpsk_dsum_site) and
on the composed route, psi1 - psi2, a * psi, normalize, dot against the oracle's dense vectors of downloaded tensors.
Cases, references and the tolerance rule: finite_linalg_cases.py (e0 measured on the device's own gauge code).  The
measured e0 and the largest observed error per case are recorded in profiles/finite_linalg_bounds.log."""
import numpy as np
import pytest

import mpskit_jl_amd as mk
from mpskit_jl_amd import linalg

import finite_linalg_cases as fc

pytestmark = pytest.mark.gpu


_CASES = {}


def _case(be, kind, chain):
    """one Case per (kind, chain) for the whole module: the addends and their dense vectors are computed once"""
    if (kind, chain) not in _CASES:
        _CASES[kind, chain] = fc.Case(be, kind, chain)
    return _CASES[kind, chain]


@pytest.fixture(params=[(k, ch) for k in fc.KINDS for ch in fc.CHAINS], ids=[f"{k}-{i}" for k in fc.KINDS for i in fc.CHAIN_IDS])
def case(be, request):
    return _case(be, *request.param)


# the states with two routes: real and bond-embedded tensors (interleaved complex states have the composed route only)
@pytest.fixture(params=[(k, ch, f) for k in fc.KINDS[:2] for ch in fc.CHAINS for f in (True, False)],
                ids=[f"{k}-{i}-{r}" for k in fc.KINDS[:2] for i in fc.CHAIN_IDS for r in ("fused", "composed")])
def routed(be, request):
    kind, chain, fused = request.param
    return _case(be, kind, chain), fused


def test_sum_and_difference(routed):
    fc.check_sum_and_difference(*routed)


def test_sum_and_difference_default_route(case):
    fc.check_sum_and_difference(case)


def test_canonical_form_of_the_sum(routed):
    fc.check_canonical_form(*routed)


def test_canonical_form_of_the_sum_native(be):
    for chain in fc.CHAINS:
        fc.check_canonical_form(_case(be, "native", chain))


def test_module_switch_picks_the_route(routed, monkeypatch):
    """FUSED_BY_DEFAULT = False: no dsum_site call; True: one per site step and one for the centre"""
    case, on = routed
    calls = []
    real = case.be.dsum_site
    monkeypatch.setattr(case.be, "dsum_site", lambda *a, **k: (calls.append(a[0]), real(*a, **k))[1], raising=False)
    monkeypatch.setattr(linalg, "FUSED_BY_DEFAULT", on)
    case.close_vec(fc.vec(case.psi1 + case.psi2), case.v1 + case.v2, f"switch {on}")
    half = case.L // 2
    assert calls == (["left"] * half + ["right"] * (case.L - half) + ["left"] if on else [])


def test_scalars_and_normalize(case):
    fc.check_scalars(case)


def test_overlap(case):
    fc.check_overlap(case)


def test_norms(case):
    fc.check_norms(case)


def test_real_next_to_embedded(be):
    fc.check_mixed_overlap(be, fc.CHAINS[0])


def test_rectangular_centre(be):
    c = fc.Case(be, "real", (5, 2, 8, 8))
    assert (c.psi1 + c.psi2).CLs[2].shape == (4, 8)
    fc.check_canonical_form(c)


def test_dispatch_and_errors(be):
    rng = np.random.default_rng(2)
    a = mk.FiniteMPS.random(6, 2, 4, rng, be=be)
    b = mk.FiniteMPS.random(6, 2, 3, rng, be=be)
    assert mk.dot(a, b) == linalg.dot(a, b) == a.dot(b)
    with pytest.raises(ValueError, match="Cannot add states of length 6 and 5"):
        a + mk.FiniteMPS.random(5, 2, 4, rng, be=be)
    with pytest.raises(ValueError, match="different length"):
        mk.dot(a, mk.FiniteMPS.random(5, 2, 4, rng, be=be))
    with pytest.raises(ValueError, match="physical dimensions"):
        a + mk.FiniteMPS.random(6, 3, 4, rng, be=be)
    with pytest.raises(ValueError, match="physical dimensions"):
        mk.dot(a, mk.FiniteMPS.random(6, 3, 4, rng, be=be))
    with pytest.raises(TypeError, match="complex number"):
        1j * a


def test_record_bounds(be):
    """last in the file: e0, the tolerance and the largest observed error of every case of this module"""
    for kind in fc.KINDS:
        for chain in fc.CHAINS:
            _case(be, kind, chain)
    for (kind, chain), c in _CASES.items():
        print(f"BOUNDS {kind} L={c.L} d={c.d} caps=({c.D1},{c.D2}): e0 {c.e0:.3e} tol {c.tol:.3e} worst/tol {c.worst:.3f}")
        assert c.worst <= 1.0
