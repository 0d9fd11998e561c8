"""CPU self-check of tests/exact_proj_inputs.py (no GPU): the cases of tests/test_gpu_proj_exact.py must pass their own
criteria, and must be able to tell a subtly wrong contraction from the right one.

Every integer case: the 2^50 guard holds (asserted while the case is built), numpy fp64 equals the longdouble
reference bit for bit and is integer-valued.  Every Gaussian case: numpy fp64 lies inside the componentwise bound.
Where mpskit_oracle has the operation (dAC, dC, dAC2, transfer_left, transfer_right, regularize_env; its tensordot
contractions take rectangular environments as they are) it agrees exactly with the einsum on the integer cases.
Sensitivity: each plausible wrong contraction of `epi.wrong` differs from the reference in at least one element."""
import numpy as np
import pytest

import exact_inputs as ei
import exact_proj_inputs as epi
import mpskit_oracle as mo


def _integer_valued(a):
    return np.array_equal(a, np.round(a.real) + (1j * np.round(a.imag) if np.iscomplexobj(a) else 0))


def _check_int(t):
    assert t["bound"] is None and t["magnitude"] < ei.LIMIT, t["name"]
    hp = epi.contract(t["op"], t, ei._hp)
    assert np.array_equal(t["ref"].astype(hp.dtype), hp), t["name"]
    assert _integer_valued(t["ref"]), t["name"]


def test_case_lists_are_what_the_issue_states():
    ex = epi.cases_exact()
    assert len(set(ex)) == len(ex)
    ops = {c[0] for c in ex}
    assert ops == {"dC_proj", "dAC_proj", "dAC2_proj", "dAC2_product", "dAC2", "dC", "dAC_blocked", "hac_blocked", "tl", "tr",
                   "tl0", "tr0"}
    # every family has a ragged and an aligned shape; dtypes and slice kinds of the table
    for op in ops - {"dAC_blocked", "hac_blocked"}:
        assert {c[1] for c in ex if c[0] == op} == {"ragged", "aligned"}, op
    assert {(c[2], c[3]) for c in ex if c[0] == "dAC2_proj"} == {(False, ""), (True, ""), (False, "dense")}
    assert {(c[2], c[3]) for c in ex if c[0] == "dAC_proj"} == {(True, ""), (False, "dense")}      # f64 sparse: exact_inputs
    assert {(c[2], c[3]) for c in ex if c[0] == "dAC2_product"} == {(False, ""), (False, "dense")}
    assert {c[4] for c in ex if c[0] == "dC_proj"} == {1, 3} == {c[4] for c in epi.reg_cases()}
    for op in ("tl", "tr"):
        assert {(c[2], c[3]) for c in ex if c[0] == op} == {(False, ""), (True, ""), (False, "dense")}
        assert {c[2] for c in ex if c[0] == op + "0"} == {False, True}
    assert {c[0] for c in epi.cases_gauss()} == ops | {"reg"} and all(c[1] in ("ragged", "nblk3") for c in epi.cases_gauss())
    # shapes: ragged extents pairwise distinct, aligned ones multiples of 64; the mixed transfers have Dlb != Dl, Drb != Dr
    r, a = epi.RAGGED, epi.ALIGNED
    assert len({r[k] for k in ("Dlo", "Dl", "Dm", "Dr", "Dro")}) == 5 and r["d1"] != r["d2"]
    assert all(a[k] % 64 == 0 for k in ("Dlo", "Dl", "Dm", "Dr", "Dro"))
    for m in epi.MIXED.values():
        assert m["Dlb"] != m["Dl"] and m["Drb"] != m["Dr"]
    assert all(v % 64 == 0 for v in epi.MIXED["aligned"].values()) and len(set(epi.MIXED["ragged"].values())) == 4
    assert {(b["nblk"], b["Dl"]) for b in epi.BLOCKED.values()} == {(2, 128), (3, 33)}
    assert len(epi.degenerate_cases()) == 7 * 4 + 6 * 2


@pytest.mark.parametrize("c", epi.cases_exact() + epi.reg_cases(), ids=epi.case_id)
def test_exact_cases_are_exact(c):
    op, shape, cplx, variant, W = c
    t = epi.case(op, shape, "int", cplx, variant, W)
    _check_int(t)
    if "s2" in t:                        # H1.chi_r == H2.chi_l; different physical dimensions on the ragged shape
        assert t["s"].chir == t["s2"].chil and (t["s"].d != t["s2"].d) == (shape == "ragged" and variant != "dense")


@pytest.mark.parametrize("c", epi.cases_gauss(), ids=epi.case_id)
def test_gaussian_references_pass_their_own_bound(c):
    op, shape, cplx, variant, W = c
    t = epi.case(op, shape, "gauss", cplx, variant, W)
    assert (t["bound"] >= 0).all() and t["bound"].dtype == ei.LD
    rec = ei.compare(epi.contract(op, t), t["ref"], t["bound"], t["name"])
    assert rec is None, rec


def _oracle(t):
    """the oracle's result in the layout of epi.contract, or None where it has no such operation"""
    op = t["op"]
    chis = t["chis"]
    env = lambda k: epi._unstack(t[k], chis)
    if op in ("dAC", "dAC_proj", "dAC_blocked", "hac_blocked"):
        return mo.dAC(t["x"], t["s"], env("G"), env("R"))
    if op in ("dC", "dC_proj"):
        return mo.dC(t["x"], env("G"), env("R"))
    if op == "dAC2":
        return mo.dAC2(t["x"], t["s"], t["s2"], env("G"), env("R"))
    if op in ("dAC2_proj", "dAC2_product"):                      # the oracle has no factorised form: on theta = AC AR
        theta = np.einsum("asm,mrb->asbr", t["AC"], t["AR"], optimize=False)
        return mo.dAC2(theta, t["s"], t["s2"], env("G"), env("R"))
    if op == "tl":
        return epi._stack(mo.transfer_left(env("G"), t["s"], t["A"], t["Ab"]))
    if op == "tr":
        return epi._stack(mo.transfer_right(env("R"), t["s"], t["A"], t["Ab"]))
    if op == "tl0":
        return np.stack([mo.transfer_left_bond(t["G"][:, w, :], t["A"], t["Ab"]) for w in range(len(chis))], axis=1)
    if op == "tr0":
        return np.stack([mo.transfer_right_bond(t["R"][:, w, :], t["A"], t["Ab"]) for w in range(len(chis))], axis=1)
    if op == "reg":
        return mo.regularize_env(t["v"], t["lvec"], t["rvec"])
    return None


@pytest.mark.parametrize("c", epi.cases_exact() + epi.reg_cases(), ids=epi.case_id)
def test_oracle_agrees_exactly_on_the_integer_cases(c):
    op, shape, cplx, variant, W = c
    t = epi.case(op, shape, "int", cplx, variant, W)
    got = _oracle(t)
    assert got is not None and got.shape == t["ref"].shape, t["name"]
    assert np.array_equal(got, t["ref"]), t["name"]


@pytest.mark.parametrize("c", epi.degenerate_cases(), ids=lambda c: f"{c[0]}-{c[1]}-{'c128' if c[2] else 'f64'}")
def test_degenerate_cases(c):
    op, which, cplx = c
    t = epi.degenerate_case(op, which, cplx)
    _check_int(t)
    no_in, no_out = epi.DEGENERATE_UNUSED[which]
    for k in ("O", "O2"):
        if k in t:
            col, row = epi.used_levels(t[k])
            assert [int(i) for i in np.flatnonzero(~col)] == no_in and [int(i) for i in np.flatnonzero(~row)] == no_out, (k, col, row)
    s = t["s"]
    if which == "c":
        assert s.Os and all(np.isscalar(v) for v in s.Os.values())
    if which == "d":
        assert not s.Os and not t["ref"].any()
    else:
        assert t["ref"].any()
        got = _oracle(t)
        assert np.array_equal(got, t["ref"]), t["name"]
    # a level the slice marks unused must be able to show: its environment slab is non-zero, so a block into it (out of
    # it) changes the result
    for how in ("unused_level_contributes", "unused_row_contributes"):
        w = epi.wrong(op, t, how)
        assert (w is None) == (which == "c"), (how, t["name"])
        if w is not None:
            assert not np.array_equal(w, t["ref"]), (how, t["name"])


@pytest.mark.parametrize("c", epi.long_cases() + [("dAC", epi.HAC_LONG_W, False)], ids=lambda c: f"{c[0]}-W{c[1]}-{'c128' if c[2] else 'f64'}")
def test_long_segment_cases(c):
    op, W, cplx = c
    t = epi.long_case(op, W, cplx)
    _check_int(t)
    assert np.array_equal(_oracle(t), t["ref"])
    if W == epi.HAC_LONG_W:
        assert epi.rc_nseg(t["O"]) > epi.MAXSEG
    else:
        assert W * (2 if cplx else 1) > epi.MAXSEG               # segments of the stage over the levels (two planes per complex level)
    for how in ("last_level_skipped", "level_counted_twice", "levels_reversed"):
        w = epi.wrong(op, t, how)
        assert w is not None and not np.array_equal(w, t["ref"]), (how, t["name"])
    # the first launch of a chunked list alone (segments 0 .. 31), and the chunks with the second one overwriting
    k = "R" if "R" in t else "G"
    per = 2 if cplx else 1
    if W * per > epi.MAXSEG and op in ("dAC", "dC", "tr"):
        cut = epi.MAXSEG // per
        head, tail = dict(t), dict(t)
        a = t[k].copy(); a[:, cut:, :] = 0; head[k] = a
        b = t[k].copy(); b[:, :cut, :] = 0; tail[k] = b
        assert not np.array_equal(epi.contract(op, head), t["ref"]) and not np.array_equal(epi.contract(op, tail), t["ref"])


# what each operation's inputs must be able to detect (at least one case of the operation where the mistake applies)
REQUIRED = {
    "dC_proj": {"levels_reversed", "last_level_skipped", "level_counted_twice"},
    "dC": {"levels_reversed", "GR_transposed", "last_level_skipped"},
    "dAC_proj": {"ts_swapped", "levels_reversed", "last_level_skipped", "level_counted_twice"},
    "dAC2": {"ts_swapped", "ts_swapped_site2", "GR_transposed", "levels_reversed", "d1_d2_swapped"},
    "dAC2_proj": {"ts_swapped", "ts_swapped_site2", "levels_reversed", "d1_d2_swapped"},
    "dAC2_product": {"ts_swapped", "ts_swapped_site2", "GR_transposed", "GL_transposed", "levels_reversed", "d1_d2_swapped"},
    "dAC_blocked": {"blocks_permuted", "ts_swapped", "GR_transposed", "GL_transposed", "levels_reversed"},
    "hac_blocked": {"blocks_permuted", "ts_swapped", "GR_transposed", "GL_transposed", "levels_reversed"},
    "tl": {"ts_swapped", "conj_dropped", "levels_reversed"},
    "tr": {"ts_swapped", "conj_dropped", "levels_reversed"},
    "tl0": {"conj_dropped", "levels_reversed"},
    "tr0": {"conj_dropped", "levels_reversed"},
    "reg": {"reg_sign", "reg_shared_coef"},
}


@pytest.mark.parametrize("op", sorted(REQUIRED))
def test_wrong_contractions_are_detected(op):
    seen = set()
    for c in [c for c in epi.cases_exact() + epi.reg_cases() if c[0] == op]:
        _, shape, cplx, variant, W = c
        t = epi.case(op, shape, "int", cplx, variant, W)
        for how in epi.WRONG:
            w = epi.wrong(op, t, how)
            if w is None:
                continue
            seen.add(how)
            assert w.shape == t["ref"].shape and not np.array_equal(w, t["ref"]), (how, t["name"])
    assert REQUIRED[op] <= seen, (op, REQUIRED[op] - seen)


@pytest.mark.parametrize("nblk,shape", [(2, (128, 2, 64)), (3, (33, 2, 65)), (1, (5, 3, 4))])
def test_blocked_layout_round_trips(nblk, shape):
    rng = np.random.default_rng(nblk)
    x = ei.int_array(rng, *shape)
    flat = epi.to_blocks(x, nblk)
    assert flat.shape == (x.size,) and np.array_equal(epi.from_blocks(flat, nblk, shape), x)
    n = shape[0] // nblk
    for q in range(nblk):                # block q is the contiguous column-major [n, d, Dr] tensor at offset q n d Dr
        blk = flat[q * n * shape[1] * shape[2]:(q + 1) * n * shape[1] * shape[2]].reshape((n,) + shape[1:], order="F")
        assert np.array_equal(blk, x[q * n:(q + 1) * n])
    if nblk == 1:
        assert np.array_equal(flat, np.ravel(x, order="F"))
    else:
        assert not np.array_equal(flat, np.ravel(x, order="F"))
