"""Exact tests of the quasiparticle family of the C ABI on the cases of tests/exact_qp_inputs.py: mpsk_qp_half,
mpsk_qp_apply, mpsk_qp_heff_site, mpsk_transfer_left_pair and mpsk_transfer_right_pair.

Integer-valued operands: every route returns the same bits and the comparison is np.array_equal.  The shapes ragged,
aligned and mixed_parity run on the four forced GEMM tiles and on the automatic one, for every operation and pair
combination, on the sparse slice and on the dense [4, 2, 2, 4] slice forced down its GEMM route (MPSK_DENSE_ROUTE=1) and
its mix route (MPSK_DENSE_ROUTE=0).  Every output buffer is NaN-filled first: an element the library does not write
shows.  On the automatic tile only: d = 3, the long-K shapes (both stage-3 launches of mpsk_qp_apply under split-K, the
second with beta = 1), the split-K pull-back with gamma Z, 33 used levels (both segment lists chunked by gemm_segments)
and the degenerate slices.  Invariants that are exact on integers: both pairs absent is mpsk_dAC_proj bit for bit; E = 0
and no pairs is gemm(VL^T, dAC_proj(gemm(VL, X))) bit for bit; a pair transfer with a zero second environment is the
single transfer; the two kets of a pair transfer may be exchanged; inputs, X and half are unchanged; a repeat call
returns the same bits.  One Gaussian case per operation at tile (128, 64) inside the componentwise bound derived in
tests/exact_qp_inputs.py.  The self-checks of the cases (2^50 guard, references, bound, sensitivity to wrong
contractions) are in tests/test_exact_qp_inputs_cpu.py."""
import ctypes as C

import numpy as np
import pytest

import exact_inputs as ei
import exact_proj_inputs as epi
import exact_qp_inputs as eq

pytestmark = pytest.mark.gpu

TILES = ei.TILES + [(0, 0)]                                 # (0, 0): the automatic choice
TILE_IDS = [f"{t[0]}x{t[1]}" if t[0] else "auto" for t in TILES]
ROUTES = [("sparse", None), ("dense", "1"), ("dense", "0")]     # (variant, MPSK_DENSE_ROUTE)
ROUTE_IDS = ["sparse", "dense-gemm", "dense-mix"]
ENVS = ("G", "R", "lB", "rB", "V1", "V2")


@pytest.fixture(params=TILES, ids=TILE_IDS)
def tile(request, be):
    be.lib.mpsk_ctx_force_tile(be.ctx, *request.param)
    try:
        yield request.param
    finally:
        be.lib.mpsk_ctx_force_tile(be.ctx, 0, 0)           # process-wide knob


def _route(monkeypatch, flag):
    if flag is None:
        monkeypatch.delenv("MPSK_DENSE_ROUTE", raising=False)
    else:
        monkeypatch.setenv("MPSK_DENSE_ROUTE", flag)       # read per call


def _nan(be, *shape):
    return be.upload(np.full(shape, np.nan))


def _slice(be, t):
    if t["dense"]:
        return be.mposlice_dense(t["O"])
    return be.mposlice(*t["slice_args"])


def _upload(be, t):
    """the slice and every operand of case `t` on the device: environments as W slabs, the rest column-major"""
    dv = {"H": _slice(be, t)}
    for k in ("G", "R", "lB", "rB", "V1", "V2", "B", "AR", "AL", "VL", "X", "A1", "A2", "Ab"):
        if k in t:
            dv[k] = be.upload_env(epi._unstack(t[k], t["chis"])) if k in ENVS else be.upload(t[k])
    return dv


def _assert_inputs_unchanged(be, t, dv):
    for k, x in dv.items():
        if k in ENVS:
            assert np.array_equal(np.concatenate(be.download_env(x, t["chis"]), axis=1), t[k]), (t["name"], k)
        elif k != "H":
            assert np.array_equal(be.download(x), t[k]), (t["name"], k)


def _qp_half(be, dv):
    """mpsk_qp_half into a NaN-filled buffer of mpsk_qp_half_size doubles"""
    H, GL, AL = dv["H"], dv["G"], dv["AL"]
    _, Dlo, Dl = GL.shape
    n = C.c_size_t()
    assert be.lib.mpsk_qp_half_size(H.handle, Dlo, AL.shape[2], C.byref(n)) == 0
    half = _nan(be, n.value)
    rc = be.lib.mpsk_qp_half(be.ctx, H.handle, Dlo, Dl, AL.shape[2], GL.ptr, AL.ptr, half.ptr)
    assert rc == 0, be.lib.mpsk_last_error()
    return half


def _half_host(be, half, t, dense_gemm):
    """the opaque half buffer as [a, t, m, u]: W slabs [Dlo, d, Dr2] on the mix route, [(a, m), (t, u)] on the dense one"""
    Dlo, (_, d, Dr2), Wr = t["G"].shape[0], t["AL"].shape, t["O"].shape[3]
    flat = be.download(half)
    if dense_gemm:
        return flat.reshape((Dlo, Dr2, d, Wr), order="F").transpose(0, 2, 1, 3)
    return flat.reshape((Dlo, d, Dr2, Wr), order="F")


def _apply(be, t, dv, half, combo):
    left, right = eq.has_pairs(combo)
    Dlo, d, Dro = t["G"].shape[0], t["O"].shape[1], t["R"].shape[2]
    kw = dict(lB=dv["lB"], AR=dv["AR"]) if left else {}
    if right:
        kw.update(half=half, rB=dv["rB"])
    return be.download(be.qp_apply(dv["H"], dv["G"], dv["R"], dv["B"], out=_nan(be, Dlo, d, Dro), **kw))


def _heff(be, t, dv, half, key):
    combo, E = key
    left, right = eq.has_pairs(combo)
    kw = dict(lB=dv["lB"], AR=dv["AR"]) if left else {}
    if right:
        kw.update(half=half, rB=dv["rB"])
    return be.download(be.qp_heff_site(dv["H"], dv["G"], dv["R"], dv["VL"], dv["X"], E, out=_nan(be, *t["X"].shape), **kw))


def _env_out(be, ref):
    Db, W, Dk = ref.shape
    return be.upload_env([np.full((Db, 1, Dk), np.nan) for _ in range(W)])


def _pair(be, t, dv, swap=False, V2=None):
    """the pair transfer of case `t` in the layout of its reference; swap: the two kets exchanged; V2: another second
    environment"""
    ref = t["refs"]["pair"]
    f = be.transfer_left_pair if t["op"] == "tl_pair" else be.transfer_right_pair
    a = (dv["V1"], dv["A1"]), (dv["V2"] if V2 is None else V2, dv["A2"])
    (Va, Aa), (Vb, Ab_) = a[::-1] if swap else a
    out = f(dv["H"], Va, Aa, Vb, Ab_, dv["Ab"], out=_env_out(be, ref))
    return np.concatenate(be.download_env(out, [1] * ref.shape[1]), axis=1)


def _same(got, ref, bound, name):
    rec = ei.compare(got, ref, bound, name)
    assert rec is None, rec


def _profiled(be, fn):
    be.prof_enable(True)
    try:
        y = fn()
        prof = be.prof_summary()
    finally:
        be.prof_enable(False)
    return y, {r["kernel"]: r["launches"] for r in prof}


# ---- one operation on one uploaded case: every sub-case and the invariants -----------------------------------------
def _run_qp_half(be, t, flag, where=""):
    dv = _upload(be, t)
    used = epi.used_levels(t["O"])[0]                        # levels nothing enters are never read: not compared
    got = _half_host(be, _qp_half(be, dv), t, t["dense"] and flag == "1")
    _same(got[..., used], t["refs"]["half"][..., used], t["bounds"]["half"] if t["bounds"]["half"] is None
          else t["bounds"]["half"][..., used], f"{t['name']}{where}")
    if t["kind"] == "int":
        assert np.array_equal(_half_host(be, _qp_half(be, dv), t, t["dense"] and flag == "1")[..., used], got[..., used])
        _assert_inputs_unchanged(be, t, dv)


def _run_qp_apply(be, t, where=""):
    dv = _upload(be, t)
    half = _qp_half(be, dv)
    half0 = be.download(half)
    got = {}
    for k in t["keys"]:
        got[k] = _apply(be, t, dv, half, k)
        _same(got[k], t["refs"][k], t["bounds"][k], f"{t['name']}-{k}{where}")
    if t["kind"] != "int":
        return
    # both pairs absent: mpsk_dAC_proj bit for bit
    Dlo, d, Dro = got["plain"].shape
    assert np.array_equal(got["plain"], be.download(be.dAC_proj(dv["H"], dv["G"], dv["R"], dv["B"], out=_nan(be, Dlo, d, Dro))))
    assert np.array_equal(_apply(be, t, dv, half, "all"), got["all"])                # a repeat call returns the same bits
    assert np.array_equal(be.download(half), half0, equal_nan=True)                  # half is read, not consumed
    _assert_inputs_unchanged(be, t, dv)


def _run_qp_heff(be, t, where=""):
    dv = _upload(be, t)
    half = _qp_half(be, dv)
    half0 = be.download(half)
    got = {}
    for k in t["keys"]:
        got[k] = _heff(be, t, dv, half, k)
        _same(got[k], t["refs"][k], t["bounds"][k], f"{t['name']}-{eq.key_id(k)}{where}")
    if t["kind"] != "int":
        return
    # E = 0 and no pairs: VL^T dAC_proj(VL X) from the existing entries, bit for bit
    Dl, d, Dr = t["G"].shape[0], t["O"].shape[1], t["R"].shape[0]
    Bd = be.gemm(dv["VL"], dv["X"]).reshape(Dl, d, Dr)
    yd = be.dAC_proj(dv["H"], dv["G"], dv["R"], Bd, out=_nan(be, Dl, d, Dr))
    comp = be.download(be.gemm(dv["VL"], yd.reshape(Dl * d, Dr), transA=True))
    assert np.array_equal(got[("plain", 0.0)], comp), t["name"]
    for k in (("all", eq.E_DYADIC), ("plain", eq.E_DYADIC)):
        assert np.array_equal(_heff(be, t, dv, half, k), got[k]), (t["name"], k)     # a repeat call returns the same bits
    assert np.array_equal(be.download(half), half0, equal_nan=True)
    _assert_inputs_unchanged(be, t, dv)                                              # X among them


def _run_pair(be, t, where=""):
    dv = _upload(be, t)
    got = _pair(be, t, dv)
    _same(got, t["refs"]["pair"], t["bounds"]["pair"], f"{t['name']}{where}")
    if t["kind"] != "int":
        return
    assert np.array_equal(_pair(be, t, dv, swap=True), got), t["name"]               # the kets exchanged: the same bits
    assert np.array_equal(_pair(be, t, dv), got), t["name"]
    # a zero second environment: the single transfer (signed zeros do not matter)
    zero = be.upload_env(epi._unstack(np.zeros_like(t["V2"]), t["chis"]))
    single = be.transfer_left_ex if t["op"] == "tl_pair" else be.transfer_right_ex
    one = single(dv["H"], dv["V1"], dv["A1"], dv["Ab"], out=_env_out(be, t["refs"]["pair"]))
    one = np.concatenate(be.download_env(one, [1] * got.shape[1]), axis=1)
    first = eq.site_terms(t["op"], t)["1"][0]
    assert np.array_equal(one + 0.0, first) and np.array_equal(_pair(be, t, dv, V2=zero) + 0.0, one + 0.0), t["name"]
    _assert_inputs_unchanged(be, t, dv)


def _run(be, t, flag=None, where=""):
    op = t["op"]
    if op == "qp_half":
        return _run_qp_half(be, t, flag, where)
    if op == "qp_apply":
        return _run_qp_apply(be, t, where)
    if op == "qp_heff":
        return _run_qp_heff(be, t, where)
    return _run_pair(be, t, where)


# ---- ragged / aligned / mixed_parity on every tile, slice kind and route ---------------------------------------------
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("shape", eq.EXACT_SHAPES)
@pytest.mark.parametrize("op", eq.OPS)
def test_exact_on_every_tile(be, monkeypatch, tile, op, shape, route):
    variant, flag = route
    _route(monkeypatch, flag)
    _run(be, eq.case(op, shape, "int", variant), flag, f"@{tile}-{flag}")


# ---- the automatic tile only ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", eq.OPS)
def test_d3_sparse(be, monkeypatch, op):
    _route(monkeypatch, None)
    _run(be, eq.case(op, "d3", "int", "sparse"))


def test_longk_qp_apply_splits_both_stage3_launches(be, monkeypatch):
    """Dr = Dr2 = 256 on five used levels, Dlo d = 128 rows, Dro = 64: both stage-3 launches have 80 k-tiles on 2 tiles of
    64 x 64 and go through split-K, the second one (half rB) with beta = 1 onto the first one's result.  Run under the
    event profile, which names the tagged launches: two stage-1 products (4 k-tiles: no split) and the two stage-3 ones."""
    _route(monkeypatch, None)
    t = eq.case("qp_apply", "longk", "int", "sparse")
    dv = _upload(be, t)
    half = _qp_half(be, dv)
    for combo, n_sk in (("all", 2), ("no_left", 2), ("no_right", 1), ("plain", 1)):
        got, kernels = _profiled(be, lambda: _apply(be, t, dv, half, combo))
        print("kernels:", t["name"], combo, kernels)
        _same(got, t["refs"][combo], None, f"{t['name']}-{combo}")
        sk = sum(n for k, n in kernels.items() if "_sk_" in k)
        assert sk >= n_sk and sum(kernels.values()) - sk == (2 if eq.has_pairs(combo)[0] else 1), (combo, kernels)
    _run_qp_apply(be, t)


def test_longk_transfer_left_pair(be, monkeypatch):
    """Dlb = 512: stage 3 contracts (p, t), K = Dlb d = 1024 = 64 k-tiles on 5 tiles of 64 x 64 over the sum of the two
    stage-1 products.  The launches of the transfers are untagged, so the event profile does not name them: the split
    rests on the documented heuristic (64 x 64 tiles, KT >= 64, at most 4096 tiles)."""
    _route(monkeypatch, None)
    _run_pair(be, eq.case("tl_pair", "longk_tl", "int", "sparse"))


def test_splitk_pullback(be, monkeypatch):
    """(Dl, d, DrL, Dr) = (512, 2, 512, 64), the shape of test_split_k_pullback, on reduced-range integers with E = 0 and
    E = -2.5: the pull-back is M = 512, N = 64, K = 1024, 8 tiles of 64 x 64 and 64 k-tiles.  The share that starts a tile
    adds gamma Z, the others write partial tiles: a Z added twice, dropped or read at a wrong offset is an unequal
    element.  The pull-back GEMM is untagged and cannot be observed in the event profile: its split rests on the
    documented heuristic (64 x 64 tiles, KT >= 64, at most 4096 tiles), as in the existing test."""
    _route(monkeypatch, None)
    _run_qp_heff(be, eq.case("qp_heff", "splitk_pullback", "int", "sparse"))


@pytest.mark.parametrize("op", ["qp_apply", "tr_pair"])
def test_more_used_levels_than_one_launch_takes(be, monkeypatch, op):
    """33 used levels of chi 1: gemm_segments splits both segment lists of mpsk_qp_apply (T2 GR and half rB) into launches
    of 32 + 1 segments; the first launch of the second list must keep the caller's beta = 1, every later one accumulates.
    Tagged launches with both pairs: 2 (stage 1) + 2 + 2."""
    _route(monkeypatch, None)
    t = eq.case(op, "maxseg", "int", "sparse")
    assert len(t["chis"]) == eq.MAXSEG + 1
    if op == "qp_apply":
        dv = _upload(be, t)
        half = _qp_half(be, dv)
        got, kernels = _profiled(be, lambda: _apply(be, t, dv, half, "all"))
        print("kernels:", t["name"], kernels)
        _same(got, t["refs"]["all"], None, t["name"])
        assert sum(kernels.values()) == 6, kernels
    _run(be, t)


@pytest.mark.parametrize("which", eq.DEGENERATE)
@pytest.mark.parametrize("op", ["qp_apply", "qp_heff"])
def test_degenerate_slices(be, monkeypatch, op, which):
    """"zeros": dense blocks whose entries are all zero (no level is used on the way out), "empty": no blocks at all, "b":
    an interior level nothing enters.  Neither entry refuses such a slice: dAC_impl zero-fills y when level_segs finds no
    used level (the half term has the same, empty, list), so mpsk_qp_apply gives exact zeros and mpsk_qp_heff_site exactly
    -E X, written over the NaN of the output."""
    _route(monkeypatch, None)
    t = eq.degenerate_case(op, which)
    _run(be, t)
    if which != "b":
        dv = _upload(be, t)
        half = _qp_half(be, dv)
        if op == "qp_apply":
            got = _apply(be, t, dv, half, "all")
            assert not got.any() and np.isfinite(got).all()
        else:
            got = _heff(be, t, dv, half, ("all", eq.E_DYADIC))
            assert np.array_equal(got, -eq.E_DYADIC * t["X"])


# ---- Gaussian cases and cache revisits ---------------------------------------------------------------------------
@pytest.mark.parametrize("route", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("op", eq.OPS)
def test_gaussian_within_the_componentwise_bound(be, monkeypatch, op, route):
    variant, flag = route
    _route(monkeypatch, flag)
    t = eq.case(op, "ragged", "gauss", variant)
    be.lib.mpsk_ctx_force_tile(be.ctx, 128, 64)
    try:
        _run(be, t, flag, f"-{flag}")
    finally:
        be.lib.mpsk_ctx_force_tile(be.ctx, 0, 0)


@pytest.mark.parametrize("op", ["qp_apply", "qp_heff", "tl_pair", "tr_pair"])
def test_offset_table_caches_are_revisited(be, monkeypatch, op):
    """ONE dense slice handle on its GEMM route: ragged bonds, then aligned bonds, then the ragged ones again.  The
    per-slice offset tables (dense_tab for GL / lB / the left kets, dtabR for the right kets) are cached by bond
    dimensions, and this family looks them up with two keys per call (Dl and Dl2, Dr and Dr2): a table found under the
    wrong key is an unequal element on the revisit.  (The ctx-wide prod_tabs serve the two-site product alone.)"""
    _route(monkeypatch, "1")
    tr_, ta = eq.case(op, "ragged", "int", "dense"), eq.case(op, "aligned", "int", "dense")
    ta = dict(ta, O=tr_["O"], name=ta["name"] + "-slice-of-ragged")       # the aligned operands on the ragged case's slice
    keys = [t for t in (tr_["keys"][0], tr_["keys"][-1])]
    H = _slice(be, tr_)
    first = None
    for t in (tr_, ta, tr_):
        dv = dict(_upload(be, t), H=H)
        out = []
        for k in keys:
            assert eq._magnitude(op, t, k) < ei.LIMIT
            if op in ("tl_pair", "tr_pair"):
                got = _pair(be, dict(t, refs={"pair": eq.evaluate(op, t, k)}), dv)
            else:
                got = (_apply if op == "qp_apply" else _heff)(be, t, dv, _qp_half(be, dv), k)
            _same(got, eq.evaluate(op, t, k), None, f"{t['name']}-{eq.key_id(k)}")
            out.append(got)
        if t is tr_ and first is None:
            first = out
    assert all(np.array_equal(a, b) for a, b in zip(first, out))
