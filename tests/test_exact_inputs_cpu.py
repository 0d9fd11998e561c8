"""CPU self-check of tests/exact_inputs.py: the references of the GPU tile tests must pass their own criteria.

For every exact case: the 2^50 magnitude guard holds (asserted while the case is built) and numpy's fp64 product equals
the longdouble one bit for bit.  For every Gaussian case: numpy's fp64 result lies inside the componentwise bound around
the longdouble reference -- a bound numpy's own BLAS could not meet would be no bound for the kernels either."""
import numpy as np
import pytest

import exact_inputs as ei


def test_longdouble_is_wider_than_fp64():
    assert np.finfo(np.longdouble).nmant >= 63


def test_case_list_is_what_the_issue_states():
    groups = ei.gemm_case_groups()
    assert {k: len(v) for k, v in groups.items()} == {"aligned": 8, "ragged": 8, "shortk": 10, "edges": 36, "cbuf": 4,
                                                      "complex": 8, "gauss": 8}
    cases = ei.gemm_cases()
    assert len(cases) == 4 * sum(len(v) for v in groups.values()) + 8
    assert len({c.name for c in cases}) == len(cases)
    assert {c.tile for c in cases} == set(ei.TILES) | {(0, 0)}
    # aligned cases stay on the aligned kernel of every tile, ragged ones never do
    for c in groups["aligned"]:
        assert all(c.M % bm == 0 and c.N % bn == 0 for bm, bn in ei.TILES) and c.K % 16 == 0 and c.pa % 2 == 0 and c.pb % 2 == 0
    for c in groups["ragged"]:
        assert c.M % 64 and c.N % 64 and c.K % 16
    # MPSK_SPLITK_F = 3 leaves uneven shares on every split-K shape, 2 and 4 even ones
    for (_, _, K) in ei.SPLITK_SHAPES:
        KT = K // 16
        assert KT % ((KT + 2) // 3) != 0 and KT % 2 == 0 and KT % 4 == 0 and KT // 4 >= 16


@pytest.mark.parametrize("group", list(ei.gemm_case_groups()) + ["splitk", "streamk"])
def test_gemm_references_pass_their_own_criterion(group):
    cases = {"splitk": ei.splitk_cases(), "streamk": ei.streamk_cases()}.get(group) or ei.gemm_case_groups()[group]
    for c in cases:
        _, _, _, _, _, ref, bound = ei.gemm_data(c)                # (building an exact case asserts its 2^50 guard)
        rec = ei.compare(ei.numpy_fp64_gemm(c), ref, bound, c.name)
        assert rec is None, rec
        assert (bound is None) == (c.kind == "int")


@pytest.mark.parametrize("op,shape,cplx,variant", ei.op_cases_exact() + [("dAC", ei.LONGK, False, "")])
def test_exact_operator_cases_are_exact(op, shape, cplx, variant):
    """the oracle's fp64 contraction of integer operands == the same contraction in longdouble, and both are integers"""
    t = ei.op_case(op, shape, "int", cplx, variant)
    assert t["magnitude"] < ei.LIMIT
    if shape is ei.RAGGED:
        hp = ei.contract(op, t, ei._hp)
        assert np.array_equal(t["ref"].astype(hp.dtype), hp)
    assert np.array_equal(t["ref"], np.round(t["ref"].real) + (1j * np.round(t["ref"].imag) if cplx else 0))


@pytest.mark.parametrize("op,shape,cplx,variant", ei.op_cases_gauss())
def test_gaussian_operator_references_pass_their_own_bound(op, shape, cplx, variant):
    t = ei.op_case(op, shape, "gauss", cplx, variant)
    rec = ei.compare(t["oracle"](), t["ref"], t["bound"], t["name"])
    assert rec is None, rec
