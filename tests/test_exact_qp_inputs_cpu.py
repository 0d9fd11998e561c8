"""CPU self-check of tests/exact_qp_inputs.py (no GPU): the cases of tests/test_gpu_qp_exact.py must pass their own
criteria, and must be able to tell a subtly wrong contraction from the right one.

Every integer case: the 2^50 guard holds for every sub-case (asserted while the case is built), numpy fp64 equals the
longdouble reference bit for bit (while the work stays under ei.LD_MAX_WORK), is integer-valued (a multiple of 1/2 with
E = -2.5) and does not depend on the bracket order.  Every Gaussian case: numpy fp64 evaluated in the SECOND bracket
order lies inside the componentwise bound.  Where mpskit_oracle has the operation -- dAC on rectangular environments for
every term of mpsk_qp_apply, transfer_left / transfer_right for a pair written as the sum of two single transfers -- it
agrees exactly with the references.  Sensitivity: each wrong contraction of `eq.wrong` differs from the reference of
every exact sub-case it applies to."""
import numpy as np
import pytest

import exact_inputs as ei
import exact_proj_inputs as epi
import exact_qp_inputs as eq
import mpskit_oracle as mo

ALL_EXACT = eq.cases_exact() + eq.cases_auto()


def _check_int(t):
    op = t["op"]
    for k in t["keys"]:
        ref = t["refs"][k]
        assert t["bounds"][k] is None and t["magnitude"][k] < ei.LIMIT, (t["name"], k)
        assert np.array_equal(2 * ref, np.round(2 * ref)) and np.abs(ref).max(initial=0.0) <= t["magnitude"][k], (t["name"], k)
        assert np.array_equal(eq.evaluate(op, t, k, order=2), ref), (t["name"], k)
        if t["work"] <= ei.LD_MAX_WORK:
            hp = eq.evaluate(op, t, k, ei._hp)
            assert hp.dtype == ei.LD and np.array_equal(ref.astype(ei.LD), hp), (t["name"], k)


def test_case_lists_are_what_the_issue_states(capsys):
    ex = eq.cases_exact()
    assert len(set(ex)) == len(ex) == 5 * 3 * 2
    assert {c[0] for c in ex} == set(eq.OPS) == {c[0] for c in eq.cases_gauss()}
    assert all(c[1] == "ragged" for c in eq.cases_gauss()) and {c[2] for c in eq.cases_gauss()} == {"sparse", "dense"}
    r, a, m = (eq.SHAPES[k] for k in eq.EXACT_SHAPES)
    assert len(set(r["bonds"])) == 6 and {33, 65} <= set(r["bonds"]) and all(b % 2 == 1 or b in (20, 48) for b in r["bonds"])
    assert all(b == 128 for i, b in enumerate(a["bonds"]) if i not in (2, 4)) and a["bonds"][2] == a["bonds"][4] == 64
    assert m["bonds"][2] % 2 == 1 and m["bonds"][4] % 2 == 1 and all(b == 128 for i, b in enumerate(m["bonds"]) if i not in (2, 4))
    for S in (r, a, m):                                  # qp_heff: the same bonds with Dlo = Dl, Dro = Dr
        assert S["heff"][:4] == S["bonds"][1:5]
    lk = eq.SHAPES["longk"]["bonds"]
    assert lk[3] == lk[4] == 256 and eq.SHAPES["longk"]["levels"] * (256 // 16) >= 64
    assert eq.SHAPES["splitk_pullback"]["heff"] == (512, 64, 64, 512, 512)          # (Dl, d, DrL, Dr) = (512, 2, 512, 64)
    assert eq.SHAPES["maxseg"]["levels"] == eq.MAXSEG + 1 and max(eq.SHAPES["maxseg"]["bonds"]) <= 24
    auto = eq.cases_auto()
    assert {("qp_apply", "longk"), ("tl_pair", "longk_tl"), ("qp_heff", "splitk_pullback"), ("qp_apply", "maxseg"),
            ("tr_pair", "maxseg")} <= {c[:2] for c in auto} and {c[0] for c in auto if c[1] == "d3"} == set(eq.OPS)
    # the counts the pull request states: sub-cases per operation
    with capsys.disabled():
        print()
        for op in eq.OPS:
            n_ex = sum(len(eq.keys(o, s)) for o, s, v in ALL_EXACT if o == op)
            n_dg = sum(len(eq.keys(op, "degenerate")) for _ in eq.DEGENERATE) if op in ("qp_apply", "qp_heff") else 0
            n_ga = sum(len(eq.keys(o, s)) for o, s, v in eq.cases_gauss() if o == op)
            print(f"exact_qp_inputs: {op:9s} exact sub-cases {n_ex:3d} (+ {n_dg:2d} degenerate) in "
                  f"{sum(1 for c in ALL_EXACT if c[0] == op):2d} cases, gaussian {n_ga:2d}, mutants {len(eq.REQUIRED[op]):2d}")


@pytest.mark.parametrize("c", ALL_EXACT, ids=eq.case_id)
def test_exact_cases_are_exact(c):
    t = eq.case(c[0], c[1], "int", c[2])
    _check_int(t)
    if c[1] in ("longk", "longk_tl", "maxseg"):
        assert len(t["chis"]) == eq.SHAPES[c[1]]["levels"] and epi.used_levels(t["O"])[0].all()


def test_qp_heff_ranges_and_magnitudes(capsys):
    """the ranges of the qp_heff cases and their worst-case magnitudes against 2^50 (printed for the pull request)"""
    with capsys.disabled():
        print()
        for c in [c for c in ALL_EXACT if c[0] == "qp_heff"]:
            t = eq.case(c[0], c[1], "int", c[2])
            worst = max(t["magnitude"].values())
            assert worst < ei.LIMIT
            for k, r in t["ranges"].items():
                if k in t:
                    assert np.abs(t[k]).max() <= r, (t["name"], k)
            rg = {k: t["ranges"][k] for k in ("VL", "X", "G", "R", "lB", "AR", "AL", "rB", "O")}
            print(f"exact_qp_inputs: {t['name']:40s} ranges {rg} worst magnitude 2^{np.log2(worst):.1f}")
    t = eq.case("qp_heff", "splitk_pullback", "int", "sparse")
    assert t["ranges"]["VL"] == t["ranges"]["X"] == 1 and np.abs(t["VL"]).max() == 1 and np.abs(t["G"]).max() == 2
    # ... and entries in [-4, 4] would not have fitted there
    rows, n = t["VL"].shape
    Wl, d, _, Wr = t["O"].shape
    assert 4.0 ** 6 * rows * t["G"].shape[2] * n * Wl * d * t["R"].shape[0] * Wr > ei.LIMIT


@pytest.mark.parametrize("c", eq.cases_gauss(), ids=eq.case_id)
def test_gaussian_second_bracket_order_passes_the_bound(c):
    t = eq.case(c[0], c[1], "gauss", c[2])
    for k in t["keys"]:
        b = t["bounds"][k]
        assert (b >= 0).all() and b.dtype == ei.LD and t["refs"][k].dtype == ei.LD
        for order in (2, 1):
            rec = ei.compare(eq.evaluate(c[0], t, k, order=order), t["refs"][k], b, f"{t['name']}-{eq.key_id(k)}-order{order}")
            assert rec is None, rec


def _env(t, k):
    return epi._unstack(t[k], t["chis"])


@pytest.mark.parametrize("c", [c for c in ALL_EXACT if c[1] not in ("splitk_pullback",) and c[0] != "qp_half"], ids=eq.case_id)
def test_oracle_agrees_exactly_on_the_integer_cases(c):
    op = c[0]
    t = eq.case(op, c[1], "int", c[2])
    s = t["s"]
    if op in ("tl_pair", "tr_pair"):
        f = mo.transfer_left if op == "tl_pair" else mo.transfer_right
        got = sum(epi._stack(f(_env(t, "V" + i), s, t["A" + i], t["Ab"])) for i in ("1", "2"))
        assert np.array_equal(got, t["refs"]["pair"]), t["name"]
        return
    d = s.d
    B = eq.site_of(t["VL"], t["X"], d) if op == "qp_heff" else t["B"]
    y = {"B": mo.dAC(B, s, _env(t, "G"), _env(t, "R")), "L": mo.dAC(t["AR"], s, _env(t, "lB"), _env(t, "R")),
         "R": mo.dAC(t["AL"], s, _env(t, "G"), _env(t, "rB"))}
    for k in t["keys"]:
        combo, E = k if op == "qp_heff" else (k, 0.0)
        left, right = eq.has_pairs(combo)
        got = y["B"] + (y["L"] if left else 0) + (y["R"] if right else 0)
        if op == "qp_heff":
            got = t["VL"].T @ got.reshape((t["VL"].shape[0], -1), order="F") - E * t["X"]
        assert np.array_equal(got, t["refs"][k]), (t["name"], k)


@pytest.mark.parametrize("op", ["qp_apply", "qp_heff"])
@pytest.mark.parametrize("which", eq.DEGENERATE)
def test_degenerate_cases(op, which):
    t = eq.degenerate_case(op, which)
    _check_int(t)
    col, row = epi.used_levels(t["O"])
    if which == "b":
        assert [int(i) for i in np.flatnonzero(~col)] == [3] and t["refs"][t["keys"][0]].any()
        return
    assert not col.any() and not row.any() and (len(t["slice_args"][4]) > 0) == (which == "zeros")
    for k in t["keys"]:                              # exact zeros; qp_heff: exactly -E X
        want = -k[1] * t["X"] if op == "qp_heff" else np.zeros_like(t["refs"][k])
        assert np.array_equal(t["refs"][k], want), (t["name"], k)


@pytest.mark.parametrize("op", eq.OPS)
def test_wrong_contractions_are_detected(op, capsys):
    seen, n = {}, 0
    for c in [c for c in ALL_EXACT if c[0] == op]:
        t = eq.case(op, c[1], "int", c[2])
        for k in t["keys"]:
            for how in eq.WRONG:
                w = eq.wrong(op, t, k, how)
                if w is None:
                    continue
                seen[how] = seen.get(how, 0) + 1
                n += 1
                assert w.shape == t["refs"][k].shape and not np.array_equal(w, t["refs"][k]), (how, t["name"], k)
    assert eq.REQUIRED[op] <= set(seen), (op, eq.REQUIRED[op] - set(seen))
    with capsys.disabled():
        print(f"\nexact_qp_inputs: {op}: {len(seen)} mutants, {n} (mutant, sub-case) pairs, none survives: {seen}")


def test_mutants_cover_the_list_of_the_issue():
    need = {"lB_dropped", "lB_twice", "half_with_GR", "half_from_B", "ket2_dropped", "ket2_first_env", "ts_swapped", "E_sign",
            "Z_transposed", "Z_wrong_ld", "pullback_untransposed", "E_before_pullback"}
    assert need <= set(eq.WRONG) and need <= set().union(*eq.REQUIRED.values())
