"""CPU self-check of tests/exact_canonical_inputs.py: the references of tests/test_gpu_canonical_exact.py must pass their
own criteria, and the whole case runner must run end to end on the host stand-in.

The guards (asserted while a case is built), the oracle against longdouble on the small shapes, the isometries, the
mirror of the segment counts, every Gaussian bound met by numpy's own fp64 evaluation, and the runner."""
import numpy as np
import pytest

import exact_inputs as ei
import exact_canonical_inputs as eci
from cpu_backend import CpuComplexBackend


def _hac_cases():
    out = [(f, Dl, Dr, False) for f in eci.FAMILIES for (Dl, Dr) in eci.HAC_SHAPES + [(eci.LONGK, eci.LONGK)][: f == "full"]]
    return out + [(f, Dl, Dr, True) for f in eci.HAC_C128_FAMILIES for (Dl, Dr) in eci.HAC_C128_SHAPES]


def _transfer_cases():
    out = [(s, f) + shp for s in "lr" for f in eci.FAMILIES for shp in eci.transfer_shapes(f, s)[:-1]]
    return out + [("l", "full", eci.LONGK, 2, eci.LONGK), ("r", "full", eci.LONGK, 2, eci.LONGK)]


def test_longdouble_is_wider_than_fp64():
    assert np.finfo(np.longdouble).nmant >= 63


@pytest.mark.parametrize("family,cplx", [(f, False) for f in eci.FAMILIES] + [(f, True) for f in eci.HAC_C128_FAMILIES])
def test_slices_are_in_jordan_form_with_the_expected_segment_counts(family, cplx):
    s, O = eci.jordan_slice(family, "int", cplx)
    m = eci.jordan_mirror(O)
    W, d = O.shape[0], O.shape[1]
    assert m["jordan"] and (m["jr_nseg"], m["jl_nseg"]) == eci.NSEG[family], m
    assert (m["jr_padded"], m["jl_padded"]) == eci.PADDED[family]
    assert m["nslabs"] == 2 * d * d
    assert m["tl_dblock"] == (family != "sparse")
    assert s.chil[0] == s.chil[-1] == 1 and O.shape == (W, d, d, W) and W == sum(eci.CHIS[family])
    assert np.array_equal(O.real, np.round(O.real)) and np.abs(O.real).max() <= 4 and np.abs(O.imag).max() <= 4
    assert not np.any(O[0, :, :, 0].imag) and not np.any(O[-1, :, :, -1].imag)      # corners exactly real
    assert np.iscomplexobj(O) == cplx
    if family == "full":                    # both folds use all d^2 slabs
        assert m["r_used"].all() and m["l_used"].all()
    if family == "sparse":                  # different slab sets, one empty slab in each family for the padding
        assert not np.array_equal(m["r_used"], m["l_used"]) and not m["r_used"].all() and not m["l_used"].all()
        assert list(m["r_used"].sum(axis=1)) == [3, 2, 1] and list(m["l_used"].sum(axis=1)) == [1, 2, 3]
    if family == "chi":
        assert s.isscal(0, 3) and s.Os[(0, 3)] == 3.0 and s.Os[(0, 1)].shape == (1, 2, 2, 3) and s.Os[(2, 3)].shape == (2, 2, 2, 1)
    if family == "onsite":
        assert W == 2 and set(s.Os) == {(0, 0), (0, 1), (1, 1)}
    # the Gaussian twin keeps the pattern
    mg = eci.jordan_mirror(eci.jordan_slice(family, "gauss", cplx)[1])
    assert mg["jordan"] and (mg["jr_nseg"], mg["jl_nseg"]) == eci.NSEG[family]


def test_mirror_refuses_what_mposlice_build_refuses():
    O = np.array(eci.jordan_slice("full")[1])
    assert eci.jordan_mirror(O)["jordan"]
    for idx in [(1, 0, 0, 2), (2, 1, 0, 0), (4, 0, 1, 1)]:                      # A block, entry into level 0, exit from level W-1
        B = O.copy(); B[idx] = 1.0
        assert not eci.jordan_mirror(B)["jordan"], idx
    B = O.copy(); B[0, 0, 0, 0] = 2.0
    assert not eci.jordan_mirror(B)["jordan"]


@pytest.mark.parametrize("n", [1, 2, 3, 15, 32, 66, 130, 256, 387, 512])
def test_dyadic_orthogonal_matrices_are_exactly_orthogonal(n):
    Q = eci.dyadic_orthogonal(n, "test")
    assert np.array_equal(Q.T @ Q, np.eye(n))
    assert eci.dyadic_unit(Q) >= 2.0 ** -4
    hp = Q.astype(ei.LD)
    assert np.array_equal(hp.T @ hp, np.eye(n))
    assert (np.count_nonzero(Q, axis=0) > 1).any() == (n >= 4)                  # not a mere permutation


@pytest.mark.parametrize("side,family,Dl,d,Dr", _transfer_cases())
def test_isometries_are_exact(side, family, Dl, d, Dr):
    t = eci.transfer_case(side, family, Dl, d, Dr)
    A = t["A"]
    assert A.shape == (Dl, d, Dr)
    if side == "l":
        assert np.array_equal(np.einsum("ptq,ptb->qb", A, A), np.eye(Dr))
        assert np.array_equal(t["GL"][0][:, 0, :], np.eye(Dl)) and t["ident"] == 0
    else:
        assert np.array_equal(np.einsum("atb,ptb->ap", A, A), np.eye(Dl))
        assert np.array_equal(t["GR"][-1][:, 0, :], np.eye(Dr)) and t["ident"] == sum(t["chis"]) - 1
    assert t["magnitude"] / t["unit"] < ei.LIMIT and t["unit"] == eci.dyadic_unit(A) ** 2


@pytest.mark.parametrize("family,Dl,Dr,cplx", _hac_cases())
def test_exact_hac_cases_are_exact(family, Dl, Dr, cplx):
    """the guard holds, the identities are in place, the oracle's fp64 result is an integer array, equals the longdouble
    contraction on the small shapes and the folded form numpy evaluates in fp64"""
    t = eci.hac_case(family, Dl, Dr, "int", cplx)
    assert t["magnitude"] < ei.LIMIT and t["bound"] is None
    assert np.array_equal(t["GL"][0][:, 0, :], np.eye(Dl)) and np.array_equal(t["GR"][-1][:, 0, :], np.eye(Dr))
    assert t["G"].shape == (Dl, sum(t["chis"]), Dl) and t["R"].shape == (Dr, sum(t["chis"]), Dr)
    ref = t["ref"]
    assert np.array_equal(ref, np.round(ref.real) + (1j * np.round(ref.imag) if cplx else 0))
    if t["work"] <= eci.LD_MAX_WORK:
        hp = eci.hp_reference(t)
        assert np.array_equal(ref.astype(hp.dtype), hp)
    assert eci.check(eci.numpy_folded(t), t, "folded") is None


@pytest.mark.parametrize("side,family,Dl,d,Dr", _transfer_cases())
def test_exact_transfer_cases_are_exact(side, family, Dl, d, Dr):
    t = eci.transfer_case(side, family, Dl, d, Dr)
    ref, n = t["ref"], t["n_out"]
    assert ref.shape == (n, sum(t["chis"]), n) and t["bound"] is None
    assert np.array_equal(ref[:, t["ident"], :], np.eye(n))                     # the oracle computes A^T A = 1 exactly
    assert np.array_equal(ref / t["unit"], np.round(ref / t["unit"]))
    if t["work"] <= eci.LD_MAX_WORK:
        hp = eci.hp_reference(t)
        assert np.array_equal(ref.astype(hp.dtype), hp)
    assert eci.check(eci.numpy_folded(t), t, "folded") is None


@pytest.mark.parametrize("route,family,cplx", eci.GAUSS_CASES)
def test_gaussian_references_pass_their_own_bound(route, family, cplx):
    """numpy's fp64 evaluation -- the oracle's three-stage bracket and the folded form of the route -- inside the bound"""
    t = eci.gauss_case(route, family, cplx)
    W, d = sum(t["chis"]), t["d"]
    if route == "hac":
        Dl, Dr = eci.GAUSS_HAC_SHAPE
        assert t["depth"] == W + W + d * (Dl + Dr)
        assert np.array_equal(t["GL"][0][:, 0, :], np.eye(Dl)) and np.array_equal(t["GR"][-1][:, 0, :], np.eye(Dr))
    else:
        Dk = t["A"].shape[0] if route == "tl" else t["A"].shape[2]
        assert t["depth"] == W + d + 2 * d * Dk
    assert (t["bound"] > 0).all()
    for what, got in (("oracle", t["oracle"]()), ("folded", eci.numpy_folded(t))):
        if route != "hac":                  # the written level: numpy computes A^T A, which is the identity only to rounding
            got = np.array(got)
            assert np.abs(got[:, t["ident"], :] - np.eye(t["n_out"])).max() < 1e-13
            got[:, t["ident"], :] = np.eye(t["n_out"])
        assert eci.check(got, t, what) is None
        print(f"{t['name']} numpy {what}: worst ratio to the bound {eci.bound_ratio(got, t):.4f}")
        assert eci.bound_ratio(got, t) <= 1.0
    # the criterion does notice an error of a few units of the bound, and a wrong written level
    bad = np.array(t["ref"]).astype(np.complex128 if cplx else np.float64)
    idx = (1, 1, 1)
    bad[idx] += 3.0 * float(t["bound"][idx])
    if route != "hac":
        bad[:, t["ident"], :] = np.eye(t["n_out"])
    assert eci.check(bad, t) is not None
    if route != "hac":
        worse = np.array(eci.numpy_folded(t)); worse[0, t["ident"], 0] += 2.0 ** -52
        assert "identity_level_not_exact" in eci.check(worse, t)


@pytest.fixture(scope="module")
def cb():
    return CpuComplexBackend()


@pytest.mark.parametrize("family,Dl,Dr,cplx", [c for c in _hac_cases() if c[1] <= 65])
def test_runner_hac_on_the_host_stand_in(cb, monkeypatch, family, Dl, Dr, cplx):
    t = eci.hac_case(family, Dl, Dr, "int", cplx)
    y, info = eci.run_hac(cb, t)
    assert info == {"mode": 3, "combined_slabs": t["mirror"]["nslabs"]}
    assert eci.check(y, t) is None
    a0, a1 = ((-2 + 0.5j) if cplx else -2.0), 0.5
    y2, _ = eci.run_hac(cb, t, axpby=(a1, a0))
    assert np.array_equal(y2, a0 * t["x"] + a1 * t["ref"])
    if not cplx:
        for mode in ("0", "1"):
            monkeypatch.setenv("MPSK_HAC_MODE", mode)
            y, info = eci.run_hac(cb, t, flag=False)
            assert info["mode"] == int(mode) and eci.check(y, t) is None
    else:
        assert eci.run_hac(cb, t, flag=False)[1]["mode"] == 2


@pytest.mark.parametrize("family", eci.FAMILIES)
@pytest.mark.parametrize("side", ["l", "r"])
def test_runner_transfers_on_the_host_stand_in(cb, monkeypatch, side, family):
    shapes = eci.transfer_shapes(family, side)
    assert shapes[0] == shapes[-1] and len({s for s in shapes}) >= 2
    done = eci.run_transfer_sequence(cb, side, family)
    assert [(t["A"].shape) for t, _ in done] == shapes
    for t, got in done:
        assert eci.check(got, t) is None
    monkeypatch.setenv("MPSK_TRANSFER_MODE", "0")
    t = done[0][0]
    assert eci.check(eci.run_transfer(cb, eci.make_slice(cb, t), t), t) is None


@pytest.mark.parametrize("route,family,cplx", eci.GAUSS_CASES)
def test_runner_gaussian_cases_on_the_host_stand_in(cb, route, family, cplx):
    t = eci.gauss_case(route, family, cplx)
    got = eci.run_hac(cb, t)[0] if route == "hac" else eci.run_transfer(cb, eci.make_slice(cb, t), t)
    assert eci.check(got, t) is None
    assert eci.bound_ratio(got, t) <= 1.0

