"""CPU self-check of tests/exact_dense_inputs.py (no GPU): the cases of tests/test_gpu_dense_exact.py must pass their own
criteria, and must be able to tell a subtly wrong dense route from the right one.

Every exact sub-case: the 2^50 guard holds, the left-first bracket, the MPO-first bracket and (while the work stays under
ei.LD_MAX_WORK) the longdouble multiply-out agree bit for bit, and the result is integer-valued (a multiple of 1/2 for
hac_axpby).  Every Gaussian case: numpy fp64 in the library's bracket order lies inside the componentwise bound.  Every O is
generic; the planted zero levels are what the library derives as col_used / row_used; on O == 0 the references are exact
zeros (hac_axpby: exactly a0 x).  mpskit_oracle agrees exactly on one small case per operation.  Sensitivity: each wrong
contraction of `ed.WRONG` differs from the reference on every exact sub-case it applies to."""
import numpy as np
import pytest

import exact_dense_inputs as ed
import exact_inputs as ei
import exact_proj_inputs as epi
import mpskit_oracle as mo

ALL_SITES = ed.sites_exact() + ed.sites_zero() + ed.sites_blk()


def test_case_lists_are_what_the_issue_states(capsys):
    assert ed.SLICES == [(2, 2, 2), (3, 5, 2), (5, 3, 3), (9, 7, 3), (16, 16, 16), (1, 4, 2), (4, 1, 2)]
    assert ed.BONDS == [(1, 1), (7, 13), (64, 64), (65, 33)] and ed.BONDS_WORKLOAD == [(7, 13), (64, 64)]
    assert len(set(ALL_SITES)) == len(ALL_SITES) == 6 * 4 + 2 + 3 * 4 + 2
    for b in ((7, 13), (65, 33), (13, 7)):               # ragged: every bond of a kind differs, dense_stage1 has tabs_even false
        Dlo, Dro, Dlb, Drb, Dl2, Dr2 = ed.AUX[b]
        assert Dlo != b[0] and Dro != b[1] and Dlb != b[0] and Drb != b[1] and Dl2 != b[0] and Dr2 != b[1]
        assert (Dlo * b[0]) % 2 == 1 or b[0] % 2 == 1
    assert set(ed.AUX[(64, 64)]) == {64} and all(ed.BLK_BONDS[0] % n == 0 for n in ed.NBLK)
    assert set(ed.ZERO_SLICES) == {(5, 3, 3), (16, 16, 16)} and ed.ZEROS == ("v0", "w0", "both", "all")
    assert ed.GAUSS == [((5, 3, 3), (65, 33)), ((16, 16, 16), (64, 64))]
    assert {c for c in ed.sites_tiles()} >= {(s, b, "") for s in ed.RECT for b in ((7, 13), (65, 33))} | {(ed.WORKLOAD, (64, 64), "")}
    assert ed.GEMM_BK == 16 and ed.WORKLOAD[2] * ed.WORKLOAD[0] == 256               # stage 2 of the workload: 16 k-tiles
    sub = ed.subcases_exact()
    with capsys.disabled():
        print()
        for op in ed.OPS:
            n_ex = sum(1 for c in sub if c[0] == op) + (sum(len(ed.nblks(ed.site(*c[1:3], "int", c[3]))) - 1 for c in sub if c[0] == op)
                                                         if op == "hac_blk" else 0)
            n_mut = sum(1 for how in ed.WRONG if any(ed.wrong(op, ed.site(*c[1:3], "int", c[3]), how) is not None
                                                      for c in sub if c[0] == op))
            print(f"exact_dense_inputs: {op:9s} exact sub-cases {n_ex:3d}, gaussian {len(ed.GAUSS)}, mutants {n_mut:2d}")


@pytest.mark.parametrize("c", ALL_SITES, ids=ed.site_id)
def test_exact_cases_are_exact(c):
    t = ed.site(c[0], c[1], "int", c[2])
    assert np.array_equal(t["O"], ed.dense_O(c[0], "int", c[2]))
    for k in ed.OPERANDS + ("O",):
        assert np.abs(t[k]).max() <= 4 and np.array_equal(t[k], np.round(t[k])), (t["name"], k)
    for op in ed.ops_of(c):
        r = ed.ref(op, t)
        m = ed.magnitude(op, t)
        assert m < ei.LIMIT and ed.bound_of(op, t) is None, (t["name"], op)
        assert np.array_equal(2 * r, np.round(2 * r)) and np.abs(r).max(initial=0.0) <= m, (t["name"], op)
        assert np.array_equal(ed.evaluate(op, t, order=2), r), (t["name"], op)
        if ed.work(op, t) <= ei.LD_MAX_WORK:
            hp = ed.evaluate(op, t, ei._hp)
            assert hp.dtype == ei.LD and np.array_equal(r.astype(ei.LD), hp), (t["name"], op)
        else:
            assert c[:2] == (ed.WORKLOAD, (64, 64)), t["name"]       # the one site left to the two fp64 brackets


def test_every_O_is_generic_and_shared_between_bonds():
    for slc in ed.SLICES:
        assert ed.is_generic(ed.dense_O(slc)) and ed.is_generic(ed.dense_O(slc, "gauss")), slc
        assert ed.dense_O(slc).shape == (slc[0], slc[2], slc[2], slc[1])
    for slc in ed.ZERO_SLICES:
        for z in ("v0", "w0", "both"):
            assert ed.is_generic(ed.dense_O(slc, "int", z)), (slc, z)
    sym = np.ones((3, 2, 2, 3))
    assert not ed.is_generic(sym) and not ed.is_generic(np.arange(16.0).reshape(2, 2, 2, 2) + np.arange(16.0).reshape(2, 2, 2, 2).transpose(3, 1, 2, 0))
    a, b = ed.site((3, 5, 2), (7, 13)), ed.site((3, 5, 2), (13, 7))
    assert a["O"] is b["O"] and a["x"].shape == (7, 2, 13) and b["x"].shape == (13, 2, 7)


@pytest.mark.parametrize("c", ed.sites_zero(), ids=ed.site_id)
def test_planted_zero_levels_are_what_the_library_derives(c):
    """col_used / row_used as mposlice_build derives them from the values (epi.used_levels) against the planted levels"""
    slc, bonds, z = c
    t = ed.site(slc, bonds, "int", z)
    col, row = epi.used_levels(t["O"])
    zw, zv = ed.zero_levels(slc, z)
    if z == "all":
        assert not col.any() and not row.any()
        for op in ed.ops_of(c):                          # exact +0.0; hac_axpby exactly a0 x
            want = ed.A0 * t["x"] if op == "hac_axpby" else np.zeros_like(ed.ref(op, t))
            assert np.array_equal(ed.ref(op, t), want) and not np.signbit(ed.ref(op, t) + 0.0)[want == 0].any(), (t["name"], op)
        return
    assert [int(i) for i in np.flatnonzero(~col)] == zv and [int(i) for i in np.flatnonzero(~row)] == zw
    assert 0 < min(zw + zv) and (not zw or zw[0] < slc[0] - 1) and (not zv or zv[0] < slc[1] - 1)      # interior levels
    for op in ed.ops_of(c):
        assert ed.ref(op, t).any(), (t["name"], op)


@pytest.mark.parametrize("g", ed.GAUSS, ids=lambda g: ed.site_id(g + ("",)))
@pytest.mark.parametrize("op", ed.OPS)
def test_gaussian_numpy_fp64_passes_the_bound(op, g):
    t = ed.gauss_site(g[0], g[1], op)
    assert ed.applies(op, t)
    b, r = ed.bound_of(op, t), ed.ref(op, t)
    assert b.dtype == ei.LD and r.dtype == ei.LD and (b >= 0).all() and b.shape == r.shape
    # numpy fp64 in the bracket order the bound is derived for: left-first (right transfer: bra first; pair: ket first)
    got = ed.evaluate(op, t) if op != "tr_pair" else ed.tr(t["Rt"], t["x"], t["O"], t["Ab"], 3) + ed.tr(t["V2r"], t["A2r"], t["O"], t["Ab"], 3)
    rec = ei.compare(got, r, b, f"{t['name']}-{op}")
    assert rec is None, rec
    print(f"exact_dense_inputs: {t['name']}-{op}: numpy fp64 max err / bound = {float((np.abs(got.astype(ei.LD) - r) / b).max()):.2e}")


def _env(t, k):
    return [np.array(t[k])]


@pytest.mark.parametrize("op", ed.OPS)
def test_oracle_agrees_exactly_on_one_small_case(op):
    t = ed.site((3, 5, 2), (7, 13)) if op != "hac_blk" else ed.site((3, 5, 2), ed.BLK_BONDS)
    s = ed.oracle_slice(t)
    if op in ("dAC", "hac"):
        got = mo.dAC(t["x"], s, _env(t, "G"), _env(t, "R"))
    elif op == "dAC_proj":
        got = mo.dAC(t["x"], s, _env(t, "G"), _env(t, "Rp"))
    elif op == "hac_blk":
        got = mo.dAC(t["x"], s, _env(t, "Gs"), _env(t, "R"))
        for n in ed.nblks(t):
            assert np.array_equal(epi.from_blocks(epi.to_blocks(t["x"], n), n, t["x"].shape), t["x"])
    elif op == "hac_axpby":
        got = ed.A0 * t["x"] + ed.A1 * mo.dAC(t["x"], s, _env(t, "Gs"), _env(t, "R"))
    elif op in ("tl", "tl_ex"):
        got = mo.transfer_left(_env(t, "Gt"), s, t["x"], t["Ab"])[0]
    elif op in ("tr", "tr_ex"):
        got = mo.transfer_right(_env(t, "Rt"), s, t["x"], t["Ab"])[0]
    elif op == "tl_pair":
        got = mo.transfer_left(_env(t, "Gt"), s, t["x"], t["Ab"])[0] + mo.transfer_left(_env(t, "V2l"), s, t["A2l"], t["Ab"])[0]
    else:
        got = mo.transfer_right(_env(t, "Rt"), s, t["x"], t["Ab"])[0] + mo.transfer_right(_env(t, "V2r"), s, t["A2r"], t["Ab"])[0]
    assert np.array_equal(got, ed.ref(op, t)), (op, t["name"])


@pytest.mark.parametrize("op", ed.OPS)
def test_wrong_contractions_are_detected(op, capsys):
    seen, n = {}, 0
    for c in [c for c in ed.subcases_exact() if c[0] == op]:
        t = ed.site(c[1], c[2], "int", c[3])
        r = ed.ref(op, t)
        for how in ed.WRONG:
            w = ed.wrong(op, t, how)
            if w is None:
                continue
            seen[how] = seen.get(how, 0) + 1
            n += 1
            assert w.shape == r.shape and not np.array_equal(w, r), (how, t["name"], op)
    need = set(ed.WRONG) - {"beta_on_product", "left_tab_right", "Ab_untransposed", "GR_transposed", "zero_from_neighbour"}
    if op == "hac_axpby":
        need |= {"beta_on_product"}
    if op == "tr_pair":
        need |= {"left_tab_right"}
    if op in ("tl", "tl_ex"):
        need |= {"Ab_untransposed"}
    if op in ("dAC", "hac", "hac_axpby", "hac_blk", "tr", "tr_ex"):
        need |= {"GR_transposed"}
    if op not in ("tl_pair", "tr_pair", "hac_blk"):      # these have no structured-zero site
        need |= {"zero_from_neighbour"}
    assert need <= set(seen), (op, need - set(seen))
    with capsys.disabled():
        print(f"\nexact_dense_inputs: {op}: {len(seen)} mutants, {n} (mutant, sub-case) pairs, none survives: {seen}")


def test_the_k_tile_mutant_is_met_at_K_256():
    """the last of the 16 k-tiles of stage 2 of the workload: rows z = 240 .. 255 of Od, i.e. w = 15, every s"""
    t = ed.site(ed.WORKLOAD, (7, 13))
    O = t["O"]
    Ow = np.array(O)
    Ow[15] = 0
    for op in ("dAC", "tl", "tr"):
        w = ed.wrong(op, t, "last_ktile_dropped")
        assert np.array_equal(w, ed.evaluate(op, t, over={"O": Ow})) and not np.array_equal(w, ed.ref(op, t))
