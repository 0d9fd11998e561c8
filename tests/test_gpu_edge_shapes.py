"""Exact tests at the shapes both ends of a finite chain pass (bonds 1 to 9), on the cases of tests/edge_shape_cases.py:
the GEMM core (mpsk_gemm in fp64 and complex128, all transpose pairs, beta = 0 over NaN and beta = 1, tight and padded
leading dimensions; mpsk_gemm_pair), the operators on sparse slices (mpsk_dAC, mpsk_dC, mpsk_dAC2, the projections and the
two-site product), the prepared operators in every mode (0, 1, 2, 3; blocked vectors; axpby; the summed operator on both
routes), the transfers (plain, canonical on both routes, pair, Gram) and the small memory-bound entries (regularize,
dsum_site, copy2d, cx_embed / cx_half) -- and one walk over the seven sites of the d = 2 chain edge on ONE ctx, where
every call meets workspaces and tables sized by the call before it.

Integer operands: every route returns the same bits, the comparison is np.array_equal on the four forced GEMM tiles and
on the automatic one, every output buffer is NaN-filled (or carries a sentinel padding row) first.  One Gaussian case per
entry at (3, 7), d = 3 inside the componentwise bound.  The self-checks of the cases are in test_edge_shape_cases_cpu.py."""
import numpy as np
import pytest

import edge_shape_cases as esc
import exact_canonical_inputs as eci
import exact_inputs as ei
import exact_proj_inputs as epi

pytestmark = pytest.mark.gpu

TILES = ei.TILES + [(0, 0)]                                 # (0, 0): the automatic choice
TILE_IDS = [f"{t[0]}x{t[1]}" if t[0] else "auto" for t in TILES]


@pytest.fixture(params=TILES, ids=TILE_IDS)
def tile(request, be):
    be.lib.mpsk_ctx_force_tile(be.ctx, *request.param)
    try:
        yield request.param
    finally:
        be.lib.mpsk_ctx_force_tile(be.ctx, 0, 0)           # process-wide knob


def _nan_like(be, shape, cplx):
    if cplx:
        return be.upload_c(np.full(shape, complex(np.nan, np.nan)))
    return be.upload(np.full(shape, np.nan))


def _slice(be, s, cplx):
    return be.mposlice(s.odim, s.d, s.chil, s.chir, dict(s.Os), cplx=cplx)


def _env_out(be, shape, cplx):
    Db, W, Dk = shape
    nan = complex(np.nan, np.nan) if cplx else np.nan
    return (be.upload_env_c if cplx else be.upload_env)([np.full((Db, 1, Dk), nan) for _ in range(W)])


def _apply(be, t):
    """entry t["entry"] on the operands of case `t`, in the layout of epi.contract, over NaN-filled outputs"""
    entry, op, cplx, chis = t["entry"], t["op"], t["cplx"], t["chis"]
    up, down = (be.upload_c, be.download_c) if cplx else (be.upload, be.download)
    env = lambda k: (be.upload_env_c if cplx else be.upload_env)(epi._unstack(t[k], chis))
    down_env = lambda y: np.concatenate((be.download_env_c if cplx else be.download_env)(y, chis), axis=1)
    out = lambda: _nan_like(be, t["ref"].shape, cplx)
    H = _slice(be, t["s"], cplx) if "s" in t else None
    H2 = _slice(be, t["s2"], cplx) if "s2" in t else None
    if entry == "dC":
        return down(be.dC(env("G"), env("R"), up(t["x"]), out=out(), cplx=cplx))
    if entry == "dC_proj":
        return down(be.dC_proj(env("G"), env("R"), up(t["x"]), out=out()))
    if entry == "dC_proj_c":
        return down(be.dC_proj_c(env("G"), env("R"), up(t["x"]), out=out()))
    if entry == "dAC":
        return down(be.dAC(H, env("G"), env("R"), up(t["x"]), out=out()))
    if entry == "dAC_proj":
        return down(be.dAC_proj(H, env("G"), env("R"), up(t["x"]), out=out()))
    if entry == "dAC2":
        return down(be.dAC2(H, H2, env("G"), env("R"), up(t["x"]), out=out()))
    if entry == "dAC2_proj":
        return down(be.dAC2_proj(H, H2, env("G"), env("R"), up(t["AC"]), up(t["AR"]), out=out()))
    if entry == "dAC2_product":
        return down(be.dAC2_product(H, H2, env("G"), env("R"), up(t["AC"]), up(t["AR"]), out=out()))
    if entry == "tl":
        return down_env(be.transfer_left(H, env("G"), up(t["A"]), up(t["Ab"]), out=_env_out(be, t["ref"].shape, cplx), cplx=cplx))
    if entry == "tr":
        return down_env(be.transfer_right(H, env("R"), up(t["A"]), up(t["Ab"]), out=_env_out(be, t["ref"].shape, cplx), cplx=cplx))
    raise KeyError(entry)


def _refused(fn, code, text):
    import mpskit_jl_amd as mk
    with pytest.raises(mk.MpskError) as e:
        fn()
    assert f"(code {code})" in str(e.value) and text in str(e.value), str(e.value)


# ---- 1. GEMM core --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", esc.gemm_groups(), ids=lambda g: g.name[10:])
def test_gemm_every_shape_below_one_fragment(be, tile, g):
    """216 shapes (M, N, K) in {1, 2, 3, 4, 8, 9}^3 per group, packed: one upload, 216 launches, one download; the whole C
    buffer -- results, sentinel padding rows, gaps between the matrices -- must be what the builder expects"""
    data = esc.gemm_group_data(g)
    up, down = (be.upload_c, be.download_c) if g.cplx else (be.upload, be.download)
    dA, dB, dC = up(data["A"]), up(data["B"]), up(data["C"])
    sz = 16 if g.cplx else 8
    be._set_dtype(g.cplx)
    try:
        for (M, N, K, oa, lda, ob, ldb, oc, ldc) in data["calls"]:
            be.gemm_raw(g.tA, g.tB, M, N, K, data["alpha"], dA.ptr + sz * oa, lda, dB.ptr + sz * ob, ldb, data["beta"],
                        dC.ptr + sz * oc, ldc)
    finally:
        be._set_dtype(False)
    rec = esc.gemm_mismatch(g, down(dC))
    assert rec is None, (rec, tile)


@pytest.mark.parametrize("c", esc.GEMM_GAUSS, ids=lambda c: c.name)
def test_gemm_gaussian_within_the_componentwise_bound(be, tile, c):
    rec = ei.run_gemm_case(be, ei.replace(c, tile=tuple(tile)))
    assert rec is None, rec


def _padded(a, fill):
    s = np.full((a.shape[0] + 1, a.shape[1]), fill)
    s[:a.shape[0]] = a
    return s


def _gemm_pair(be, t, c2):
    """mpsk_gemm_pair with one padding row in every leading dimension: (out1 over NaN, out2 over c2, what the buffers held)"""
    M, K = t["P"].shape
    N = t["B"].shape[1]
    P, B, coef = be.upload(_padded(t["P"], np.nan)), be.upload(_padded(t["B"], np.nan)), be.upload(_padded(t["coef"], np.nan))
    Q = None if t["Q"] is None else be.upload(_padded(t["Q"], np.nan))
    s1, s2 = ei._sentinel(M + 1, N), ei._sentinel(M + 1, N)
    s1[:M], s2[:M] = np.nan, c2
    o1, o2 = be.upload(s1), be.upload(s2)
    be.gemm_pair_raw(M, N, K, P.ptr, M + 1, None if Q is None else Q.ptr, M + 1, B.ptr, K + 1, coef.ptr, K + 1, 0.0, o1.ptr,
                     M + 1, 1.0, o2.ptr, M + 1)
    return be.download(o1), be.download(o2), s1, s2


def test_gemm_pair_gaussian_within_the_componentwise_bound(be, tile):
    t = esc.gemm_pair_gauss()
    M = t["P"].shape[0]
    g1, g2, s1, s2 = _gemm_pair(be, t, t["C2"])
    assert ei.compare(g1[:M], t["ref1"], t["bound1"], t["name"] + "-out1") is None
    assert ei.compare(g2[:M], t["ref2"], t["bound2"], t["name"] + "-out2") is None
    assert np.array_equal(g1[M:], s1[M:]) and np.array_equal(g2[M:], s2[M:])


def test_gemm_pair_exact(be, tile):
    bad = []
    for key in esc.gemm_pair_keys():
        t = esc.gemm_pair_case(*key)
        M = t["P"].shape[0]
        g1, g2, s1, s2 = _gemm_pair(be, t, t["C2"])
        e1, e2 = s1.copy(), s2.copy()
        e1[:M], e2[:M] = t["ref1"], t["ref2"]
        if not (np.array_equal(g1, e1) and np.array_equal(g2, e2)):
            bad.append(t["name"])
    assert not bad, (bad, tile)


# ---- 2. operators on sparse slices, 4. plain transfers ------------------------------------------------------------------
@pytest.mark.parametrize("entry,cplx", [(e, c) for e, (_, dts, _) in esc.ENTRIES.items() for c in dts],
                         ids=lambda v: v if isinstance(v, str) else ("c128" if v else "f64"))
def test_operator_exact_on_the_whole_ladder(be, tile, entry, cplx):
    bad = []
    for key in esc.op_keys():
        if key[0] != entry or key[5] != cplx:
            continue
        t = esc.op_case(*key[:5], "int", cplx)
        rec = ei.compare(_apply(be, t), t["ref"], None, f"{t['name']}@{tile}")
        if rec is not None:
            bad.append(rec)
    assert not bad, bad[:8]


@pytest.mark.parametrize("key", esc.op_gauss_keys(), ids=esc.key_id)
def test_operator_gaussian_within_the_componentwise_bound(be, tile, key):
    t = esc.op_case(*key[:5], "gauss", key[5])
    rec = ei.compare(_apply(be, t), t["ref"], t["bound"], f"{t['name']}@{tile}")
    assert rec is None, rec


def test_refusals_by_contract(be):
    """the table of edge_shape_cases.REFUSALS: error code and message, nothing launched"""
    t = esc.op_case("dAC", 3, 9, 3, "chi")
    env = lambda k: be.upload_env(epi._unstack(t[k], t["chis"]))
    hac = be.hac_create(_slice(be, t["s"], False), env("G"), env("R"))
    code, text, _ = esc.REFUSALS[("hac_apply", "nblk does not divide Dl")]
    _refused(lambda: hac.apply(be.upload(t["x"]), nblk=2), code, text)
    tc = esc.op_case("dAC", 2, 4, 2, "chi", "int", True)
    envc = lambda k: be.upload_env_c(epi._unstack(tc[k], tc["chis"]))
    hc = be.hac_create(_slice(be, tc["s"], True), envc("G"), envc("R"))
    assert hc.info()["mode"] == 2
    code, text, _ = esc.REFUSALS[("hac_apply", "nblk > 1 on a complex operator")]
    _refused(lambda: hc.apply(be.upload_c(tc["x"]), nblk=2), code, text)
    tj = eci.hac_case("full", 2, 4)
    hj = be.hac_create_ex(eci.make_slice(be, tj), be.upload_env(tj["GL"]), be.upload_env(tj["GR"]), canonical=True)
    assert hj.info()["mode"] == 3
    code, text, _ = esc.REFUSALS[("hac_apply", "nblk > 1 in mode 3")]
    _refused(lambda: hj.apply(be.upload(tj["x"]), nblk=2), code, text)
    # a complex operand 8 bytes into its buffer: refused, and this is the one place a misaligned complex pointer is made
    from mpskit_jl_amd.backend import DTensor
    r = esc.reg_case(1, 1, 2, True)
    big = be.upload_c(np.concatenate([[0j], np.ravel(r["v"], order="F"), [0j]]))
    off = DTensor(big.buf[1:1 + 2 * r["v"].size], (1, 2, 2))
    code, text, _ = esc.REFUSALS[("regularize_axpby", "complex operand at an 8-byte offset")]
    _refused(lambda: be.regularize_axpby(off, be.upload_c(r["lvec"]), be.upload_c(r["rvec"]), cplx=True), code, text)
    tp = esc.op_case("dC_proj", 1, 2, 2, "min")
    envp = lambda k: be.upload_env(epi._unstack(tp[k], tp["chis"]))
    code, text, _ = esc.REFUSALS[("dC_proj", "ctx set to MPSK_C128")]
    be._set_dtype(True)
    try:
        _refused(lambda: be.dC_proj(envp("G"), envp("R"), be.upload(tp["x"])), code, text)
    finally:
        be._set_dtype(False)


# ---- 3. prepared operators -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [None, "0", "1"], ids=["model", "mode0", "mode1"])
def test_prepared_operator_real_modes_0_and_1(be, monkeypatch, tile, mode):
    """mpsk_hac_create on the real sparse slices of the whole ladder: the mode is asserted (forced: what MPSK_HAC_MODE asks
    for, mode 1 only where the slice has a right-combined form; unset: the cost model, mirrored in expected_hac_mode), then
    apply with nblk = 1, nblk = 2 where Dl is even, and apply_axpby with a dyadic real pair"""
    if mode is None:
        monkeypatch.delenv("MPSK_HAC_MODE", raising=False)
    else:
        monkeypatch.setenv("MPSK_HAC_MODE", mode)
    bad, seen = [], set()
    for (Dl, Dr, d) in esc.LADDER:
        for w in esc.SLICES:
            t = esc.op_case("dAC", Dl, Dr, d, w)
            env = lambda k: be.upload_env(epi._unstack(t[k], t["chis"]))
            hac = be.hac_create(_slice(be, t["s"], False), env("G"), env("R"))
            want = esc.expected_hac_mode(t) if mode is None else (1 if mode == "1" and epi.rc_nseg(t["O"]) > 0 else 0)
            got = hac.info()["mode"]
            assert got == want, (t["name"], got, want)
            seen.add(got)
            x = be.upload(t["x"])
            recs = [ei.compare(be.download(hac.apply(x, out=_nan_like(be, t["ref"].shape, False))), t["ref"], None, t["name"])]
            if Dl % 2 == 0:
                xb = be.upload(epi.to_blocks(t["x"], 2), shape=t["x"].shape)
                recs.append(ei.compare(be.download(hac.apply(xb, out=_nan_like(be, t["ref"].shape, False), nblk=2)), t["ref"], None,
                                       t["name"] + "-nblk2"))
            a0, a1 = esc.AXPBY_REAL
            y = be.download(hac.apply_axpby(a1, x, a0, out=_nan_like(be, t["ref"].shape, False)))
            recs.append(ei.compare(y, a0 * t["x"] + a1 * t["ref"], None, t["name"] + "-axpby"))
            bad += [r for r in recs if r is not None]
            hac.close()
    print("modes seen:", mode, tile, sorted(seen))
    assert not bad, bad[:8]


def test_prepared_operator_complex_mode_2(be, tile):
    bad = []
    for (Dl, Dr, d) in esc.LADDER:
        for w in esc.SLICES_C128:
            t = esc.op_case("dAC", Dl, Dr, d, w, "int", True)
            env = lambda k: be.upload_env_c(epi._unstack(t[k], t["chis"]))
            hac = be.hac_create(_slice(be, t["s"], True), env("G"), env("R"))
            assert hac.info()["mode"] == 2, (t["name"], hac.info())
            x = be.upload_c(t["x"])
            bad.append(ei.compare(be.download_c(hac.apply(x, out=_nan_like(be, t["ref"].shape, True))), t["ref"], None, t["name"]))
            a0, a1 = esc.AXPBY_CPLX
            y = be.download_c(hac.apply_axpby(a1, x, a0, out=_nan_like(be, t["ref"].shape, True)))
            bad.append(ei.compare(y, a0 * t["x"] + a1 * t["ref"], None, t["name"] + "-axpby"))
            hac.close()
    bad = [r for r in bad if r is not None]
    assert not bad, bad[:8]


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_prepared_operator_mode_3_on_the_ladder(be, monkeypatch, tile, cplx):
    """Jordan-form slices on canonical environments: mode 3 asserted, apply and apply_axpby against the general oracle"""
    monkeypatch.delenv("MPSK_HAC_MODE", raising=False)
    bad = []
    for (f, Dl, Dr, c) in esc.hac3_keys():
        if c != cplx:
            continue
        t = eci.hac_case(f, Dl, Dr, "int", cplx)
        y, info = eci.run_hac(be, t)
        assert info["mode"] == 3, (t["name"], info)
        bad.append(eci.check(y, t, f"@{tile}"))
        a0, a1 = esc.AXPBY_CPLX if cplx else esc.AXPBY_REAL
        y, _ = eci.run_hac(be, t, axpby=(a1, a0))
        bad.append(ei.compare(y, a0 * t["x"] + a1 * t["ref"], None, t["name"] + "-axpby"))
    bad = [r for r in bad if r is not None]
    assert not bad, bad[:8]


@pytest.mark.parametrize("key", esc.hsum_keys(), ids=lambda k: f"route{k[0]}-{'c128' if k[4] else 'f64'}-{k[1]}x{k[3]}x{k[2]}")
def test_summed_operator_two_terms_on_both_routes(be, monkeypatch, tile, key):
    monkeypatch.delenv("MPSK_HAC_MODE", raising=False)
    t = esc.hsum_case(*key)
    y = _hsum(be, t)
    rec = ei.compare(y, t["ref"], None, f"{t['name']}@{tile}")
    assert rec is None, rec


@pytest.mark.parametrize("cplx,mode", esc.hac_gauss_keys(), ids=["f64-mode0", "f64-mode1", "c128-mode2"])
def test_prepared_operator_gaussian_modes_0_1_2(be, monkeypatch, tile, cplx, mode):
    """apply and apply_axpby on the Gaussian dAC case at (3, 7), d = 3, inside esc.hac_bound / esc.axpby_bound"""
    if mode is None:
        monkeypatch.delenv("MPSK_HAC_MODE", raising=False)
    else:
        monkeypatch.setenv("MPSK_HAC_MODE", mode)
    t = esc.op_case("dAC", *esc.GAUSS_SHAPE, "chi", "gauss", cplx)
    up, down = (be.upload_c, be.download_c) if cplx else (be.upload, be.download)
    env = lambda k: (be.upload_env_c if cplx else be.upload_env)(epi._unstack(t[k], t["chis"]))
    hac = be.hac_create(_slice(be, t["s"], cplx), env("G"), env("R"))
    assert hac.info()["mode"] == (2 if cplx else int(mode)), hac.info()
    x = up(t["x"])
    rec = ei.compare(down(hac.apply(x, out=_nan_like(be, t["ref"].shape, cplx))), t["ref"], esc.hac_bound(t), t["name"])
    assert rec is None, rec
    a0, a1 = esc.AXPBY_CPLX if cplx else esc.AXPBY_REAL
    y = down(hac.apply_axpby(a1, x, a0, out=_nan_like(be, t["ref"].shape, cplx)))
    rec = ei.compare(y, a0 * ei._hp(t["x"]) + a1 * t["ref"], esc.axpby_bound(t, a0, a1), t["name"] + "-axpby")
    assert rec is None, rec
    hac.close()


def _hsum(be, t):
    cplx = t["cplx"]
    up_env = be.upload_env_c if cplx else be.upload_env
    Hs = [_slice(be, p[0], cplx) for p in t["parts"]]
    GLs, GRs = [up_env(p[1]) for p in t["parts"]], [up_env(p[2]) for p in t["parts"]]
    folded = t["route"] == 1                                # the promise of canonical environments holds for route 1 only
    hs = be.hsum_create(Hs, GLs, GRs, canonical=folded and not cplx, canonical_c128=folded and cplx)
    try:
        assert hs.info()["route"] == t["route"], (t["name"], hs.info())
        hs.set_coefs(esc.HSUM_COEFS)
        x = (be.upload_c if cplx else be.upload)(t["x"])
        return (be.download_c if cplx else be.download)(hs.apply(x, out=_nan_like(be, t["ref"].shape, cplx)))
    finally:
        hs.close()


@pytest.mark.parametrize("key", esc.hsum_gauss_keys(), ids=lambda k: f"route{k[0]}-{'c128' if k[4] else 'f64'}")
def test_summed_operator_gaussian_on_both_routes(be, monkeypatch, tile, key):
    monkeypatch.delenv("MPSK_HAC_MODE", raising=False)
    t = esc.hsum_case(*key, "gauss")
    rec = ei.compare(_hsum(be, t), t["ref"], t["bound"], f"{t['name']}@{tile}")
    assert rec is None, rec


# ---- quasiparticle entries -------------------------------------------------------------------------------------------
def _qp_run(be, t):
    """every sub-case of one exact_qp_inputs record: {key: result}.  Outputs and the half buffer are NaN-filled first."""
    import ctypes as C
    import exact_qp_inputs as eq
    op, chis = t["op"], t["chis"]
    H = be.mposlice(*t["slice_args"])
    env = lambda k: be.upload_env(epi._unstack(t[k], chis))
    nan = lambda *shape: be.upload(np.full(shape, np.nan))
    if op in ("tl_pair", "tr_pair"):
        ref = t["refs"]["pair"]
        f = be.transfer_left_pair if op == "tl_pair" else be.transfer_right_pair
        out = f(H, env("V1"), be.upload(t["A1"]), env("V2"), be.upload(t["A2"]), be.upload(t["Ab"]), out=_env_out(be, ref.shape, False))
        return {"pair": np.concatenate(be.download_env(out, chis), axis=1)}
    G, AL = env("G"), be.upload(t["AL"])
    Dlo, d, Dr2, Wr = t["G"].shape[0], t["O"].shape[1], t["AL"].shape[2], t["O"].shape[3]
    n = C.c_size_t()
    assert be.lib.mpsk_qp_half_size(H.handle, Dlo, Dr2, C.byref(n)) == 0 and n.value == Wr * d * Dlo * Dr2
    half = nan(n.value)
    assert be.lib.mpsk_qp_half(be.ctx, H.handle, Dlo, t["G"].shape[2], Dr2, G.ptr, AL.ptr, half.ptr) == 0, be.lib.mpsk_last_error()
    if op == "qp_half":                                      # sparse slice: the mix route's layout, Wr slabs [Dlo, d, Dr2]
        return {"half": be.download(half).reshape((Dlo, d, Dr2, Wr), order="F")}
    R, lB, AR, rB = env("R"), env("lB"), be.upload(t["AR"]), env("rB")
    out = {}
    for key in t["keys"]:
        left, right = eq.has_pairs(key if op == "qp_apply" else key[0])
        kw = dict(lB=lB, AR=AR) if left else {}
        if right:
            kw.update(half=half, rB=rB)
        if op == "qp_apply":
            y = be.qp_apply(H, G, R, be.upload(t["B"]), out=nan(Dlo, d, t["R"].shape[2]), **kw)
        else:
            y = be.qp_heff_site(H, G, R, be.upload(t["VL"]), be.upload(t["X"]), key[1], out=nan(*t["X"].shape), **kw)
        out[key] = be.download(y)
    return out


@pytest.mark.parametrize("op", esc.QP_OPS)
def test_quasiparticle_entries_on_the_ladder(be, monkeypatch, tile, op):
    """mpsk_qp_half, mpsk_qp_apply (with and without each optional pair) and mpsk_qp_heff_site (the same, E = 0 and dyadic)
    down to Dl = Dr = 1, on the three real slices"""
    monkeypatch.delenv("MPSK_DENSE_ROUTE", raising=False)
    bad = []
    for key in esc.qp_keys():
        if key[0] != op:
            continue
        t = esc.qp_case(*key)
        for k, got in _qp_run(be, t).items():
            bad.append(ei.compare(got, t["refs"][k], None, f"{t['name']}-{k}@{tile}"))
    bad = [r for r in bad if r is not None]
    assert not bad, bad[:8]


@pytest.mark.parametrize("key", esc.qp_gauss_keys(), ids=lambda k: k[0])
def test_quasiparticle_and_pair_entries_gaussian(be, monkeypatch, tile, key):
    monkeypatch.delenv("MPSK_DENSE_ROUTE", raising=False)
    t = esc.qp_case(*key, "gauss")
    for k, got in _qp_run(be, t).items():
        rec = ei.compare(got, t["refs"][k], t["bounds"][k], f"{t['name']}-{k}@{tile}")
        assert rec is None, rec


# ---- 4. canonical, pair and Gram transfers ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [None, "2"], ids=["model", "pairgram"])
@pytest.mark.parametrize("side", ["l", "r"])
def test_canonical_transfers_on_the_ladder(be, monkeypatch, tile, side, mode):
    """mpsk_transfer_left_ex / _right_ex with MPSK_TRANSFER_CANONICAL on dyadic isometries.  mpsk_ctx_transfer_stats says
    which route ran, mpsk_transfer_pair_model (host only) which one to expect: unset, the model's choice -- level by level
    at every bond of the ladder; MPSK_TRANSFER_MODE=2, the pair-Gram route wherever the slice has pairs on that side."""
    if mode is None:
        monkeypatch.delenv("MPSK_TRANSFER_MODE", raising=False)
    else:
        monkeypatch.setenv("MPSK_TRANSFER_MODE", mode)
    bad = []
    for (s_, f, Dl, d, Dr) in esc.canonical_keys():
        if s_ != side:
            continue
        t = eci.transfer_case(side, f, Dl, d, Dr)
        before = be.transfer_stats()["pair"]
        got = eci.run_transfer(be, eci.make_slice(be, t), t)
        took_pair = be.transfer_stats()["pair"] - before
        model = esc.pair_model(t["O"], Dl, Dr)
        k = 0 if side == "l" else 1
        want = model["route"][k] if mode is None else int(model["pairs"][k] > 0)
        assert took_pair == want and (mode is not None or want == 0), (t["name"], mode, took_pair, model)
        bad.append(eci.check(got, t, f"@{tile}"))
        assert np.array_equal(got[:, t["ident"], :], np.eye(t["n_out"])), t["name"]
    bad = [r for r in bad if r is not None]
    assert not bad, bad[:8]


def test_pair_transfers_on_the_ladder(be, tile):
    bad = []
    for key in esc.pair_keys():
        t = esc.pair_case(*key)
        chis = t["chis"]
        H = _slice(be, t["s"], False)
        env = lambda a: be.upload_env(epi._unstack(a, chis))
        out = _env_out(be, t["ref"].shape, False)
        fn = be.transfer_left_pair if t["side"] == "l" else be.transfer_right_pair
        y = fn(H, env(t["V1"]), be.upload(t["A1"]), env(t["V2"]), be.upload(t["A2"]), be.upload(t["Ab"]), out=out)
        bad.append(ei.compare(np.concatenate(be.download_env(y, chis), axis=1), t["ref"], None, f"{t['name']}@{tile}"))
    bad = [r for r in bad if r is not None]
    assert not bad, bad[:8]


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_gram_entries_on_the_ladder(be, tile, cplx):
    """mpsk_site_gram, mpsk_transfer_left_gram and mpsk_transfer_left_gram_env; the Gram outputs are W column-major d x d
    matrices (t fastest), written over NaN"""
    up = be.upload_c if cplx else be.upload
    down = be.download_c if cplx else be.download
    bad = []
    cases = [esc.gram_case(*key) for key in esc.gram_keys() if key[3] == cplx] + [esc.gram_gauss(cplx)]
    for t in cases:
        bd = lambda k: t.get("bound_" + k)                               # None: exact
        W, d = t["W"], t["A"].shape[1]
        Dr = t["A"].shape[2]
        gram = lambda n: _nan_like(be, (d, d, n), cplx)                  # [t, s, w] column-major = n matrices, t fastest
        host = lambda g, n: np.moveaxis(down(g).reshape(d, d, n), 2, 0)
        X = up(np.moveaxis(t["X"], 0, 3))                                # [p, s, b, w]: W contiguous tensors
        g = be.site_gram(X, up(t["Ab"]), out=gram(W), cplx=cplx)
        bad.append(ei.compare(host(g, W), t["site"], bd("site"), t["name"] + "-site"))
        env = (be.upload_env_c if cplx else be.upload_env)([t["V"][:, w:w + 1, :] for w in range(W)])
        g2 = gram(W)
        vout = be.transfer_left_gram(env, up(t["A"]), up(t["Ab"]), g2, out=_env_out(be, t["vout"].shape, cplx), cplx=cplx)
        bad.append(ei.compare(host(g2, W), t["tgram"], bd("tgram"), t["name"] + "-tgram"))
        vo = np.concatenate((be.download_env_c if cplx else be.download_env)(vout, [1] * W), axis=1)
        bad.append(ei.compare(vo, t["vout"], bd("vout"), t["name"] + "-vout"))
        g3 = gram(1)
        lin = (be.upload_env_c if cplx else be.upload_env)([t["V"][:, :1, :]])
        lout = be.transfer_left_gram_env(lin, up(t["A"]), up(t["Ab"]), up(t["R"]), g3, out=_env_out(be, (Dr, 1, Dr), cplx), cplx=cplx)
        bad.append(ei.compare(host(g3, 1)[0], t["egram"], bd("egram"), t["name"] + "-egram"))
        lo = np.concatenate((be.download_env_c if cplx else be.download_env)(lout, [1]), axis=1)
        bad.append(ei.compare(lo, t["vout"][:, :1, :], None if bd("vout") is None else bd("vout")[:, :1, :], t["name"] + "-lout"))
    bad = [r for r in bad if r is not None]
    assert not bad, (bad[:8], tile)


# ---- 5. small memory-bound entries ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_regularize_on_the_ladder(be, cplx):
    """mpsk_regularize and mpsk_regularize_axpby launch no GEMM: no tile to force, they run once"""
    up_env = be.upload_env_c if cplx else be.upload_env
    down_env = be.download_env_c if cplx else be.download_env
    up = be.upload_c if cplx else be.upload
    bad = []
    keys = [k for k in esc.reg_keys() if k[3] == cplx]
    cases = [esc.reg_case(*k) for k in keys] + [esc.reg_case(3, *esc.GAUSS_SHAPE[:2], cplx, "gauss")]
    for t in cases:
        chis = t["chis"]
        a0, a1 = esc.REG_SCALARS
        if not cplx:
            v = up_env(epi._unstack(t["v"], chis))
            be.regularize(v, up(t["lvec"]), up(t["rvec"]))
            bad.append(ei.compare(np.concatenate(down_env(v, chis), axis=1), t["ref"], t["bound"], t["name"]))
        y, xs = up_env(epi._unstack(t["v"], chis)), up_env(epi._unstack(t["xs"], chis))
        out = _env_out(be, t["v"].shape, cplx)
        be.regularize_axpby(y, up(t["lvec"]), up(t["rvec"]), a1=a1, x=xs, a0=a0, out=out, cplx=cplx)
        bad.append(ei.compare(np.concatenate(down_env(out, chis), axis=1), t["ref_axpby"], t.get("bound_axpby"), t["name"] + "-axpby"))
    bad = [r for r in bad if r is not None]
    assert not bad, bad[:8]


def test_dsum_site_on_the_ladder(be, tile):
    bad = []
    cases = [esc.dsum_case(*key) for key in esc.dsum_keys()] + [esc.dsum_gauss(side) for side in ("left", "right")]
    for t in cases:
        out = _nan_like(be, t["ref"].shape, False)
        y = be.download(be.dsum_site(t["side"], be.upload(t["G"]), be.upload(t["A1"]), be.upload(t["A2"]), out=out))
        bad.append(ei.compare(y, t["ref"], t.get("bound"), f"{t['name']}@{tile}"))
    bad = [r for r in bad if r is not None]
    assert not bad, bad[:8]


@pytest.mark.parametrize("shape", esc.COPY_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_copy2d_cx_embed_cx_half_with_padded_leading_dimensions(be, shape):
    """memory-bound copies, no GEMM and no tile: they run once"""
    t = esc.copy_case(*shape)
    rows, cols = shape

    def run(fn, src, out_rows, out_cols, want):
        """src with one NaN padding row -> destination with one sentinel padding row (and one sentinel column behind)"""
        s = np.full((src.shape[0] + 1, src.shape[1]), np.nan)
        s[:src.shape[0]] = src
        dst = ei._sentinel(out_rows + 1, out_cols + 1)
        dS, dD = be.upload(s), be.upload(dst)
        fn(dS.ptr, s.shape[0], dD.ptr, dst.shape[0])
        exp = dst.copy()
        exp[:out_rows, :out_cols] = want
        assert np.array_equal(be.download(dD), exp), (t["name"], fn)

    run(lambda sp, lds, dp, ldd: be.copy2d(rows, cols, sp, lds, dp, ldd), t["src"], rows, cols, t["src"])
    run(lambda sp, lds, dp, ldd: be.cx_embed_raw(rows, cols, sp, lds, dp, ldd), t["Hd"], 2 * rows, 2 * cols, t["E"])
    run(lambda sp, lds, dp, ldd: be.cx_half_raw(rows, cols, sp, lds, dp, ldd), t["E"], 2 * rows, cols, t["Hd"])
    run(lambda sp, lds, dp, ldd: be.cx_half_raw(rows, cols, sp, lds, dp, ldd), t["Ep"], 2 * rows, cols, t["half"])


# ---- Gaussian cases of the Jordan-form routes -------------------------------------------------------------------------
def test_jordan_routes_gaussian_at_3_7(be, monkeypatch, tile):
    monkeypatch.delenv("MPSK_HAC_MODE", raising=False)
    monkeypatch.delenv("MPSK_TRANSFER_MODE", raising=False)
    Dl, Dr, d = esc.GAUSS_SHAPE
    for cplx in (False, True):
        t = eci.hac_case("sparse", Dl, Dr, "gauss", cplx)
        y, info = eci.run_hac(be, t)
        assert info["mode"] == 3, info
        assert eci.check(y, t) is None, (t["name"], eci.bound_ratio(y, t))
    for side, shp in (("l", (Dl, d, Dr)), ("r", (Dr, d, Dl))):
        t = eci.transfer_case(side, "sparse", *shp, "gauss")
        got = eci.run_transfer(be, eci.make_slice(be, t), t)
        assert eci.check(got, t) is None, (t["name"], eci.bound_ratio(got, t))


# ---- the whole-edge composite ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", esc.COMPOSITE_SLICES)
def test_whole_edge_walk_on_one_ctx(be, tile, which):
    """seven sites, bonds 1-1-2-4-8-4-2-1, in chain order on one ctx: transfer_left site by site, transfer_right back, then
    dAC at every site and dC at every bond, each from the environments the DEVICE carried -- a workspace or table cached at
    one edge shape and reused at the next shows as a mismatch at the step after it"""
    c = esc.composite(which)
    chis = c["chis"]
    Hs = [_slice(be, st["s"], False) for st in c["sites"]]
    As = [be.upload(st["A"]) for st in c["sites"]]
    L = len(Hs)
    host = lambda e: np.concatenate(be.download_env(e, chis), axis=1)
    bad = []
    GL = [be.upload_env(epi._unstack(c["GL"][0], chis))]
    for i in range(L):
        GL.append(be.transfer_left(Hs[i], GL[i], As[i], As[i], out=_env_out(be, c["GL"][i + 1].shape, False)))
        bad.append(ei.compare(host(GL[i + 1]), c["GL"][i + 1], None, f"{c['name']}-GL[{i + 1}]"))
    GR = [None] * L + [be.upload_env(epi._unstack(c["GR"][L], chis))]
    for i in range(L - 1, -1, -1):
        GR[i] = be.transfer_right(Hs[i], GR[i + 1], As[i], As[i], out=_env_out(be, c["GR"][i].shape, False))
        bad.append(ei.compare(host(GR[i]), c["GR"][i], None, f"{c['name']}-GR[{i}]"))
    for i, st in enumerate(c["sites"]):
        y = be.dAC(Hs[i], GL[i], GR[i + 1], be.upload(st["x"]), out=_nan_like(be, c["dAC"][i].shape, False))
        bad.append(ei.compare(be.download(y), c["dAC"][i], None, f"{c['name']}-dAC[{i}]"))
        y = be.dC(GL[i + 1], GR[i + 1], be.upload(st["c"]), out=_nan_like(be, c["dC"][i].shape, False))
        bad.append(ei.compare(be.download(y), c["dC"][i], None, f"{c['name']}-dC[{i}]"))
    bad = [r for r in bad if r is not None]
    assert not bad, (bad[:8], tile)
