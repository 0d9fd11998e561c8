"""The cases of tests/test_gpu_stream_order.py, checked without a GPU: both operand sets of every case pass the exactness
guard of the input module they come from, and a read ahead of the delayed producer would be VISIBLE -- the decoy set, and
the true set with any single operand replaced by its decoy, give a reference result that differs from the true one."""
import numpy as np
import pytest

import stream_order_cases as soc

FAMILIES = {"gemm", "operators", "transfers", "factorizations", "vectors"}


def _differs(a, b):
    return any(not np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def test_every_family_has_cases():
    assert set(soc.by_family()) == FAMILIES
    assert len({c.name for c in soc.CASES}) == len(soc.CASES)


@pytest.mark.parametrize("case", soc.CASES, ids=lambda c: c.name)
def test_both_operand_sets_pass_the_exactness_guard(case):
    true, decoy = case.true(), case.decoy()
    for k in true:
        assert true[k].shape == decoy[k].shape and true[k].dtype == decoy[k].dtype == np.float64, k
        assert np.all(np.isfinite(true[k])) and np.all(np.isfinite(decoy[k])), f"{k}: decoys are finite by design"
    case.guard(true)
    case.guard(decoy)


@pytest.mark.parametrize("case", soc.CASES, ids=lambda c: c.name)
def test_a_premature_read_changes_the_result(case):
    true, decoy = case.true(), case.decoy()
    ref = case.reference(true)
    assert ref and all(np.all(np.isfinite(np.asarray(v, dtype=np.float64))) for v in ref.values())
    assert _differs(ref, case.reference(decoy)), "the decoy set gives the true result"
    for name in true:
        if name in case.extra.get("scratch", ()):           # a pre-filled scratch area the entry only writes into
            continue
        assert _differs(ref, case.reference(dict(true, **{name: decoy[name]}))), f"reading the decoy of {name} would go unseen"
