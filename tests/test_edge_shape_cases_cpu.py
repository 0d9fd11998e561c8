"""Host checks of tests/edge_shape_cases.py: every case builds, the 2^50 guard holds for every integer case (the builders
assert it), no integer reference is identically zero, and the two independent references -- mpskit_oracle and the
pairwise einsum `contract` -- agree bit for bit on the integer cases and inside the bound on the Gaussian ones.  The case
ids are unique and their number is a literal, so a family that silently drops out shows here."""
import numpy as np

import edge_shape_cases as esc
import exact_canonical_inputs as eci
import exact_inputs as ei
import exact_proj_inputs as epi

N_CASES = 1318


def test_case_ids_are_unique_and_counted():
    ids = esc.case_ids()
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1][:5]
    assert len(ids) == N_CASES, len(ids)


def test_ladder_stays_below_bond_ten():
    for Dl, Dr, d in esc.LADDER + esc.TWO_SITE:
        assert max(Dl, Dr, *esc.other_bonds(Dl, Dr)) <= esc.MAX_BOND and Dl <= d * Dr * d and Dr <= d * Dl * d
    assert [s[:2] for s in esc.LADDER[:7]] == [(1, 1), (1, 2), (2, 4), (4, 8), (8, 4), (4, 2), (2, 1)]


def test_slices_have_the_blocks_they_are_named_for():
    for d in (2, 3):
        for cplx in (False, True):
            for w in (esc.SLICES_C128 if cplx else esc.SLICES):
                s = esc.edge_slice(w, d, "int", cplx)
                assert tuple(s.chil) == esc.CHIS[w] and s.contains(0, 0) and s.contains(s.odim - 1, s.odim - 1)
                assert any(not s.isscal(*k) for k in s.Os)
        s = esc.edge_slice("cscal", d, "int", True)
        assert any(s.isscal(*k) and complex(s.Os[k]).imag != 0 for k in s.Os)
    assert esc.edge_slice("min", 2).odim == 2 and len(esc.edge_slice("min", 2).Os) == 3


def test_gemm_groups_are_exact_and_not_vacuous():
    for g in esc.gemm_groups():
        data = esc.gemm_group_data(g)
        assert len(data["calls"]) == 216
        for (M, N, K, oa, lda, ob, ldb, oc, ldc), (A, B, C0, ref) in zip(data["calls"], data["items"]):
            assert np.any(ref != 0) and ref.shape == (M, N)
            assert oa % 2 == 0 and ob % 2 == 0 and oc % 2 == 0
            opA, opB = (A.conj().T if g.tA else A), (B.conj().T if g.tB else B)
            two = data["alpha"] * np.einsum("mk,kn->mn", opA, opB, optimize=False) + data["beta"] * C0      # not BLAS
            assert np.array_equal(two, ref), (g.name, M, N, K)
            e = data["expect"][oc:oc + ldc * N].reshape(ldc, N, order="F")
            assert np.array_equal(e[:M], ref) and np.array_equal(e[M:], ei._sentinel(ldc, N)[M:])
        assert np.isfinite(data["expect"]).all()
        if g.beta0:
            assert np.isnan(data["C"]).any()
    for c in esc.GEMM_GAUSS:
        _, _, _, _, _, ref, bound = ei.gemm_data(c)
        assert np.all(np.abs(ei.numpy_fp64_gemm(c).astype(ref.dtype) - ref) <= bound)


def test_gemm_pair_cases():
    for key in esc.gemm_pair_keys():
        t = esc.gemm_pair_case(*key)
        assert np.any(t["ref1"] != 0) and np.any(t["ref2"] != 0)
        assert np.array_equal(t["ref1"].astype(np.longdouble), t["ref1_hp"])


def test_operator_cases_two_references_agree_exactly():
    for key in esc.op_keys():
        t = esc.op_case(*key[:5], "int", key[5])
        assert t["bound"] is None and t["magnitude"] < ei.LIMIT
        assert np.any(t["ref"] != 0), t["name"]
        orc = esc.oracle_ref(t)
        assert orc.shape == t["ref"].shape and np.array_equal(orc, t["ref"]), t["name"]
        assert np.array_equal(epi.contract(t["op"], t, ei._hp), t["ref"].astype(np.clongdouble if key[5] else np.longdouble)), t["name"]
        assert max(a.shape[0] for a in (t[k] for k in ("G", "R", "x", "A", "AC") if k in t)) <= esc.MAX_BOND


def test_operator_gaussian_cases_inside_the_bound():
    for key in esc.op_gauss_keys():
        t = esc.op_case(*key[:5], "gauss", key[5])
        err = np.abs(esc.oracle_ref(t).astype(t["ref"].dtype) - t["ref"])
        assert np.all(err <= t["bound"]) and np.all(t["bound"] > 0), t["name"]


def test_expected_hac_mode_is_one_of_the_two_real_modes():
    modes = {esc.expected_hac_mode(esc.op_case("dAC", Dl, Dr, d, w)) for (Dl, Dr, d) in esc.LADDER for w in esc.SLICES}
    assert modes <= {0, 1} and 1 in modes


def test_jordan_cases_build_on_the_ladder():
    for (f, Dl, Dr, cplx) in esc.hac3_keys():
        t = eci.hac_case(f, Dl, Dr, "int", cplx)
        assert t["mirror"]["jordan"] and np.any(t["ref"] != 0)
        assert np.array_equal(ei.contract("dAC", t), t["ref"]) and np.array_equal(eci.numpy_folded(t), t["ref"]), t["name"]
    for (side, f, Dl, d, Dr) in esc.canonical_keys():
        t = eci.transfer_case(side, f, Dl, d, Dr)
        assert np.any(t["ref"] != 0)
        assert np.array_equal(ei.contract(t["op"], t), t["ref"]) and np.array_equal(eci.numpy_folded(t), t["ref"]), t["name"]
        model = esc.pair_model(t["O"], Dl, Dr)
        assert model["route"] == (0, 0), (t["name"], model)         # bonds <= 9: the model stays level by level
        assert (model["pairs"][0] > 0) and (model["pairs"][1] > 0) == (f != "onsite"), (t["name"], model)
    for cplx in (False, True):
        t = eci.hac_case("sparse", *esc.GAUSS_SHAPE[:2], "gauss", cplx)
        assert np.all(np.abs(t["oracle"]().astype(t["ref"].dtype) - t["ref"]) <= t["bound"])
    Dl, Dr, d = esc.GAUSS_SHAPE
    for side, shp in (("l", (Dl, d, Dr)), ("r", (Dr, d, Dl))):
        t = eci.transfer_case(side, "sparse", *shp, "gauss")
        keep = [k for k in range(t["ref"].shape[1]) if k != t["ident"]]
        assert np.all(np.abs(t["oracle"]().astype(t["ref"].dtype) - t["ref"])[:, keep] <= t["bound"][:, keep])


def test_hsum_pair_gram_cases():
    for key in esc.hsum_keys():
        t = esc.hsum_case(*key)
        assert np.any(t["ref"] != 0) and np.array_equal(t["ref"], t["ref2"]), t["name"]
    for key in esc.pair_keys():
        t = esc.pair_case(*key)
        assert np.any(t["ref"] != 0) and np.array_equal(t["ref"], t["oracle"]), t["name"]
    for key in esc.gram_keys():
        t = esc.gram_case(*key)
        e = np.einsum
        assert np.array_equal(t["site"], e("wpsb,ptb->wts", t["X"], np.conj(t["Ab"]), optimize=True).astype(t["site"].dtype))
        T = np.tensordot(t["V"].transpose(1, 0, 2), t["A"], axes=([2], [0]))                # [w, p, s, b]
        assert np.array_equal(t["tgram"], np.tensordot(T, np.conj(t["Ab"]), axes=([1, 3], [0, 2])).transpose(0, 2, 1))
        assert np.array_equal(t["egram"], np.tensordot(np.conj(t["Ab"]), np.tensordot(T[0], t["R"], axes=([2], [0])), axes=([0, 2], [0, 2])))
        import mpskit_oracle as mo
        vo = np.stack([mo.transfer_left_bond(t["V"][:, w, :], t["A"], t["Ab"]) for w in range(t["W"])], axis=1)
        assert np.array_equal(vo, t["vout"])


def test_small_entry_cases():
    for key in esc.reg_keys():
        t = esc.reg_case(*key)
        assert np.array_equal(esc.oracle_ref(t), t["ref"]) and np.any(t["ref"] != t["v"]), t["name"]
    for cplx in (False, True):
        W, D1, D2 = 3, esc.GAUSS_SHAPE[0], esc.GAUSS_SHAPE[1]
        t = esc.reg_case(W, D1, D2, cplx, "gauss")
        assert np.all(np.abs(esc.oracle_ref(t).astype(t["ref"].dtype) - t["ref"]) <= t["bound"])
    for key in esc.dsum_keys():
        t = esc.dsum_case(*key)
        assert np.any(t["ref"] != 0) and np.array_equal(t["ref"].astype(np.longdouble), t["ref_hp"]), t["name"]
    for shp in esc.COPY_SHAPES:
        t = esc.copy_case(*shp)
        assert np.all(t["src"] != 0) and np.all(t["Hd"] != 0) and t["E"].shape == (2 * shp[0], 2 * shp[1])


def test_composite_walk_references_agree_and_stay_exact():
    for which in esc.COMPOSITE_SLICES:
        c = esc.composite(which)
        for k in ("GL", "GR", "dAC", "dC"):
            assert len(c[k]) == len(c["oracle"][k])
            for a, b in zip(c[k], c["oracle"][k]):
                assert np.array_equal(a, b) and np.any(a != 0) and np.abs(a).max() < ei.LIMIT, (which, k)
        assert c["GL"][-1].shape == (1, sum(esc.CHIS[which]), 1) and c["GR"][0].shape == (1, sum(esc.CHIS[which]), 1)


def test_quasiparticle_cases_two_references_agree():
    import exact_qp_inputs as eq
    for key in esc.qp_keys():
        t = esc.qp_case(*key)
        bonds, heff = esc.qp_bonds(*key[1:4])
        assert max(bonds + heff) <= esc.MAX_BOND
        for k in t["keys"]:
            assert np.any(t["refs"][k] != 0) and t["magnitude"][k] < ei.LIMIT, (t["name"], k)
            assert np.array_equal(eq.evaluate(t["op"], t, k, order=2), t["refs"][k]), (t["name"], k)
            orc = esc.qp_oracle(t, k)
            assert orc is None or np.array_equal(orc, t["refs"][k]), (t["name"], k)
    assert esc.qp_bonds(1, 1, 2)[1][0] == 1                         # the smallest bonds the contracts allow
    for key in esc.qp_gauss_keys():
        t = esc.qp_case(*key, "gauss")
        for k in t["keys"]:
            two = [eq.evaluate(t["op"], t, k, order=2)] + ([] if esc.qp_oracle(t, k) is None else [esc.qp_oracle(t, k)])
            for y in two:
                assert np.all(np.abs(y.astype(np.longdouble) - t["refs"][k]) <= t["bounds"][k]), (t["name"], k)


def test_remaining_gaussian_cases_inside_their_bounds():
    """numpy fp64 of every Gaussian case that has no integer twin in the same record, against its own bound"""
    g = esc.gemm_pair_gauss()
    assert np.all(np.abs(g["fp64_1"] - g["ref1"]) <= g["bound1"]) and np.all(np.abs(g["fp64_2"] - g["ref2"]) <= g["bound2"])
    for cplx in (False, True):
        t = esc.gram_gauss(cplx)
        for k in ("site", "tgram", "egram", "vout"):
            assert np.all(np.abs(t["fp64_" + k].astype(t[k].dtype) - t[k]) <= t["bound_" + k]), (t["name"], k)
    for side in ("left", "right"):
        t = esc.dsum_gauss(side)
        assert np.all(np.abs(t["fp64"] - t["ref"]) <= t["bound"]), t["name"]
    for key in esc.hsum_gauss_keys():
        t = esc.hsum_case(*key, "gauss")
        assert np.all(np.abs(t["oracle"].astype(t["ref"].dtype) - t["ref"]) <= t["bound"]), t["name"]
    for cplx, _mode in esc.hac_gauss_keys():
        t = esc.op_case("dAC", *esc.GAUSS_SHAPE, "chi", "gauss", cplx)
        y = esc.oracle_ref(t)
        assert np.all(np.abs(y.astype(t["ref"].dtype) - t["ref"]) <= esc.hac_bound(t))
        a0, a1 = esc.AXPBY_CPLX if cplx else esc.AXPBY_REAL
        assert np.all(np.abs((a0 * t["x"] + a1 * y).astype(t["ref"].dtype) - (a0 * ei._hp(t["x"]) + a1 * t["ref"])) <= esc.axpby_bound(t, a0, a1))
