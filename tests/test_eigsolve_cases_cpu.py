"""Self-checks of tests/eigsolve_cases.py, without a GPU: the longdouble Lanczos reference finds the true ground vector
when the budget is the whole space, every Gaussian case has a Ritz gap of at least 1e-3 |H_eff|_2, the float64
transcription of the device recurrence stays within the bound of every case, the plausible wrong solves lie more than
100 bounds away (a missing second Gram-Schmidt pass on the near-eigenvector starts, where it shows), the breakdown cases
cut where they should, and the case list holds every budget and every mode."""
import numpy as np
import pytest

import eigsolve_cases as ec
from exact_inputs import LD, U

GAUSS = ec.gauss_cases() + ec.edge_cases() + ec.near_cases()


@pytest.mark.parametrize("c", ec.edge_cases(), ids=ec.case_id)
def test_whole_space_budget_finds_the_ground_vector(c):
    """m = n: theta_1 is the smallest eigenvalue of H_eff and y_ref its eigenvector"""
    t, r = ec.case_operands(c), ec.reference(c)
    ew, S = np.linalg.eigh(t["H"].astype(np.float64))
    v = S[:, 0] * np.sign(S[:, 0] @ t["x0"].ravel())
    cond = r["normH"] / (ew[1] - ew[0])
    assert abs(r["theta"] - ew[0]) <= 64 * U * r["normH"]
    assert float(np.abs(r["y"] - v).max()) <= 64 * U * cond
    assert abs(float(r["y"] @ t["H"] @ r["y"]) - ew[0]) <= 64 * U * r["normH"]


@pytest.mark.parametrize("c", GAUSS, ids=ec.case_id)
def test_reference_gap(c):
    r = ec.reference(c)
    print(f"gap {ec.case_id(c)}: (theta_2 - theta_1) / |H| = {r['gap'] / r['normH']:.3e}")
    assert r["gap"] / r["normH"] >= ec.GAP_MIN
    assert r["m_eff"] == c[2]
    Q = r["Q"]
    assert float(np.abs(Q.T @ Q - np.eye(c[2])).max()) <= 2.0 ** -60


@pytest.mark.parametrize("c", ec.cases(), ids=ec.case_id)
def test_host_transcription_within_the_bound(c):
    r, h = ec.reference(c), ec.host_f64(c)
    B, e_host = ec.bound(c)
    err = float(np.abs(h["y"].astype(LD) - r["y"]).max())
    print(f"host {ec.case_id(c)}: e_host = {e_host:.3e}, B = {B:.3e}, err / B = {err / B:.3f}")
    assert err <= B                      # holds by the construction of B (4 e_host is part of it); the asserts that can
    # fail are the ones below: the cut, lambda, the norm and sign, and the basis inside the reference Krylov space
    assert h["m_eff"] == r["m_eff"]
    assert abs(h["lam"] - r["theta"]) <= B * r["normH"]
    assert abs(float(np.sqrt((h["y"].astype(LD) ** 2).sum())) - 1.0) < 1e-13 and h["y"] @ ec.case_operands(c)["x0"].ravel() > 0
    for k in range(r["m_eff"] if c[3] != "near" else 0):          # near: the basis is conditioned by |H| / beta_0 ~ 1e5
        assert ec.projection_residual(h["V"][k], c, k) <= ec.basis_bound(c, k)


@pytest.mark.parametrize("c", GAUSS, ids=ec.case_id)
def test_wrong_solves_are_far_from_the_reference(c):
    """every wrong solve that applies to the case differs from y_ref by more than 100 B: all but h1_only on the Gaussian
    starts (m > 1), and h1_only, the largest Ritz vector and the stride on the near-eigenvector starts"""
    r = ec.reference(c)
    B, _ = ec.bound(c)
    applied = []
    for how in ec.WRONG:
        w = ec.wrong(c, how)
        if w is None:
            continue
        ratio = float(np.abs(w.astype(LD) - r["y"]).max()) / B
        print(f"wrong {ec.case_id(c)} {how}: {ratio:.3e} B")
        assert ratio > 100, (how, ratio)
        applied.append(how)
    want = {"near": ["largest", "stride_2m", "h1_only"], "gauss": [] if c[2] == 1 else list(ec.WRONG[:4])}[c[3]]
    assert applied == want


def test_near_start_needs_the_second_pass():
    """the near-eigenvector start: first residual of 1e-4 |H x| and less, and one Gram-Schmidt pass alone leaves the
    basis 1e4 times less orthogonal than two"""
    for c in ec.near_cases():
        t, r = ec.case_operands(c), ec.reference(c)
        assert r["m_eff"] == 32 and float(r["betas"][0]) <= 1e-4 * r["normH"]
        V1 = ec._device_recurrence(t, 32, passes=1)[0][:32]
        V2 = ec.host_f64(c)["V"][:32]
        o1, o2 = (float(np.abs(V @ V.T - np.eye(32)).max()) for V in (V1, V2))
        print(f"near {ec.case_id(c)}: |V^T V - I| one pass {o1:.2e}, two passes {o2:.2e}")
        assert o2 <= 64 * U * np.sqrt(t["n"]) and o1 > 1e4 * o2


def test_invariant_subspaces():
    for c in ec.breakdown_cases():
        t, r, h = ec.case_operands(c), ec.reference(c), ec.host_f64(c)
        i, j, k = t["support"]
        e = np.zeros(t["n"])
        if c[3] == "invariant":
            e[i] = 1.0
            assert h["m_eff"] == r["m_eff"] == 3
            assert not h["coef"][3:].any()
            assert float(np.abs(h["y"] - e).max()) <= 64 * U and float(np.abs(r["y"] - e).max()) <= 64 * U
            assert abs(h["lam"] - t["lam"][i]) <= 64 * U * r["normH"]
        else:
            e[j] = 1.0
            assert h["m_eff"] == r["m_eff"] == 1
            assert np.array_equal(h["y"], e) and np.array_equal(r["y"].astype(np.float64), e)
            assert not h["V"][1:].any() and h["lam"] == t["lam"][j]
        assert np.isfinite(h["V"]).all() and np.isfinite(h["slot"]).all() and np.isfinite(h["y"]).all()


def test_case_list():
    cs = ec.cases()
    assert len(set(cs)) == len(cs)
    g = ec.gauss_cases()
    for shape in ("ragged", "aligned"):
        assert {c[1] for c in g if c[0] == shape} == {0, 1, 3, 4}
        full = [c[1] for c in g if c[0] == shape and c[2] == 1]
        assert full == [ec.FULL_MODE[shape]]
        for mode in ec.MODES:
            ms = {c[2] for c in g if c[0] == shape and c[1] == mode}
            assert ms == ({1, 2, 8, 9, 16, 17, 24, 25, 32} if mode == ec.FULL_MODE[shape] else {8, 9, 32})
    assert ec.near_cases() == [("ragged", 3, 32, "near"), ("aligned", 1, 32, "near")]
    assert {(c[0], c[2]) for c in ec.edge_cases()} == {("edge4", 4), ("edge2", 2)}
    assert {(c[1], c[3]) for c in ec.breakdown_cases()} == {(m, k) for m in ec.MODES for k in ("invariant", "eigvec")}
    assert all(c[2] == 8 for c in ec.breakdown_cases())
    assert ec.SHAPES == {"ragged": (9, 2, 14), "aligned": (16, 2, 16), "edge4": (1, 2, 2), "edge2": (1, 2, 1)}


def test_operator_is_the_dAC_contraction():
    """H_eff applied to x0 is exact_proj_inputs.contract("dAC") of the same operands, in longdouble"""
    import exact_inputs as ei
    import exact_proj_inputs as epi
    for shape, family in [("ragged", "sparse"), ("ragged", "jordan"), ("ragged", "dense"), ("edge4", "jordan")]:
        t = ec.operands(shape, family)
        ref = epi.contract("dAC", {"G": t["G"], "R": t["R"], "O": t["O"], "x": t["x0"]}, ei._hp).ravel()
        got = t["H"] @ t["x0"].astype(LD).ravel()
        assert float(np.abs(got - ref).max()) <= 8 * 2.0 ** -64 * float(np.abs(t["Habs"] @ np.abs(t["x0"]).ravel()).max())
