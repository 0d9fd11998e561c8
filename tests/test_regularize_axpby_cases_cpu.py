"""tests/regularize_axpby_cases.py without a GPU: the reference of mpsk_regularize_axpby is exact (so the device result must
equal it bit for bit whatever the order of its two-phase reduction), and it tells the listed wrong contractions apart on
every shape on which they can differ."""
import numpy as np
import pytest

import regularize_axpby_cases as rc

DTYPES = [False, True]


@pytest.mark.parametrize("cplx", DTYPES, ids=["f64", "c128"])
@pytest.mark.parametrize("shape", rc.SHAPES, ids=str)
def test_reference_is_exact(shape, cplx):
    t = rc.operands(shape, cplx)
    a0, a1 = rc.scalars(shape)
    for v in t.values():
        assert np.abs(v.real).max() <= 3 and np.abs(v.imag).max() <= 3
        assert np.array_equal(v.real, np.round(v.real)) and np.array_equal(v.imag, np.round(v.imag))
    for x in (t["x"], None):
        re, im, dot_bound, upd_bound = rc.guard(t["y"], t["lvec"], t["rvec"], a1, x, a0)
        assert dot_bound < 2.0 ** 53 and upd_bound < 2.0 ** 51         # integers / multiples of 1/2: exact in any order
        got = rc.ref(t["y"], t["lvec"], t["rvec"], a1, x, a0)
        assert np.array_equal(got.real.astype(np.longdouble), re) and np.array_equal(got.imag.astype(np.longdouble), im)
    # another summation order of the dot, the same bits
    coef = np.array([np.sum(t["lvec"].T[::-1] * yw[::-1]) for yw in t["y"]])
    assert np.array_equal(coef, np.einsum("qp,wpq->w", t["lvec"], t["y"]))


def test_the_large_shape_exceeds_one_pass_of_phase_two():
    W, D1, D2 = rc.BIG
    assert rc.BIG in rc.SHAPES and D1 * D2 > rc.PASS_ELEMENTS
    assert all(D1_ * D2_ <= rc.PASS_ELEMENTS for _, D1_, D2_ in rc.SHAPES if (_, D1_, D2_) != rc.BIG)
    assert any(D1_ % rc.TILE and D2_ % rc.TILE for _, D1_, D2_ in rc.SHAPES)


def test_scalars_cover_the_set():
    used = {s for shape in rc.SHAPES for s in rc.scalars(shape)}
    assert used == {1.0, -1.0, 2.0, 0.5}
    assert all(a0 != a1 for a0, a1 in rc.SCALARS)


@pytest.mark.parametrize("cplx", DTYPES, ids=["f64", "c128"])
@pytest.mark.parametrize("shape", rc.SHAPES[1:], ids=str)
@pytest.mark.parametrize("wrong", sorted(rc.WRONG))
def test_reference_tells_wrong_contractions_apart(wrong, shape, cplx):
    t = rc.operands(shape, cplx)
    a0, a1 = rc.scalars(shape)
    right = rc.ref(t["y"], t["lvec"], t["rvec"], a1, t["x"], a0)
    other = rc.WRONG[wrong](t["y"], t["lvec"], t["rvec"], a1, t["x"], a0)
    if rc.applies(wrong, shape, cplx):
        assert not np.array_equal(other, right)
    else:
        assert np.array_equal(other, right)          # the variant is the same contraction here: nothing to tell apart


def test_every_wrong_contraction_is_caught_somewhere():
    for wrong in rc.WRONG:
        assert any(rc.applies(wrong, s, c) for s in rc.SHAPES for c in DTYPES), wrong


def test_layout_helpers_round_trip():
    for cplx in DTYPES:
        t = rc.operands((2, 33, 31), cplx)
        assert np.array_equal(rc.unflat(rc.flat(t["y"], cplx), (2, 33, 31), cplx), t["y"])
