"""Exact tests of the entry points behind approximate / VOMPS / changebonds / multiline / the multi-GPU path, on the
cases of tests/exact_proj_inputs.py: mpsk_dC_proj, mpsk_dAC_proj (complex sparse, real dense), mpsk_dAC2_proj (the
factorised fp64 route on both slice kinds and the complex theta route), mpsk_dAC2_product, the complex mpsk_dAC2 and
mpsk_dC, mpsk_dAC_blocked and mpsk_hac_apply(nblk > 1) (whole operator and one rank's row block of GL), the transfers
with Ab of other bonds than A (sparse, dense and H == NULL) and mpsk_regularize.

Integer-valued operands: every route returns the same bits, the comparison is np.array_equal, on the four forced GEMM
tiles and on the automatic one.  One Gaussian case per operation at tile (128, 64) inside the componentwise bound.
Then the degenerate slices (levels nothing enters / nothing leaves, scalar blocks only, no blocks at all: the result
is exactly zero over a NaN-filled output), and the K-segment lists longer than MAXSEG = 32: the chunked launches of
gemm_segments and the per-batch device table of the right-combined prepared operator.  The self-checks of the cases
(2^50 guard, references, sensitivity to wrong contractions) are in tests/test_exact_proj_inputs_cpu.py."""
import numpy as np
import pytest

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
    """device tensor of logical `shape` filled with NaN (interleaved complex: first dimension doubled)"""
    if cplx:
        return be.upload_c(np.full(shape, complex(np.nan, np.nan)))
    return be.upload(np.full(shape, np.nan))


def _device_slice(be, s, cplx, dense):
    if dense:
        return be.mposlice_dense(s.full())
    return be.mposlice(s.odim, s.d, s.chil, s.chir, dict(s.Os), cplx=cplx)


def _apply(be, t, mode=None, rows=False):
    """operation t["op"] on the operands of case `t`, in the layout of epi.contract.  Every output buffer is NaN-filled
    first: an element the library does not write shows.  rows (blocked operations): the operator of one rank, built
    from the second row block of every GL slab."""
    op, cplx = t["op"], t["cplx"]
    chis = t["chis"]
    up, down = (be.upload_c, be.download_c) if cplx else (be.upload, be.download)
    env = lambda k: (be.upload_env_c if cplx else be.upload_env)(epi._unstack(t[k], chis))
    down_env = lambda y: np.concatenate((be.download_env_c if cplx else be.download_env)(y, chis), axis=1)
    out = lambda: _nan_like(be, t["ref"].shape, cplx)
    dense = t.get("dense", False)
    H = _device_slice(be, t["s"], cplx, dense) if "s" in t else None
    H2 = _device_slice(be, t["s2"], cplx, dense) if "s2" in t else None
    if op == "dC_proj":
        return down(be.dC_proj(env("G"), env("R"), up(t["x"]), out=out()))
    if op == "dC":
        return down(be.dC(env("G"), env("R"), up(t["x"]), out=out(), cplx=cplx))
    if op == "dAC":
        return down(be.dAC(H, env("G"), env("R"), up(t["x"]), out=out()))
    if op == "dAC_proj":
        return down(be.dAC_proj(H, env("G"), env("R"), up(t["x"]), out=out()))
    if op == "dAC2":
        return down(be.dAC2(H, H2, env("G"), env("R"), up(t["x"]), out=out()))
    if op == "dAC2_proj":
        return down(be.dAC2_proj(H, H2, env("G"), env("R"), up(t["AC"]), up(t["AR"]), out=out()))
    if op == "dAC2_product":
        return down(be.dAC2_product(H, H2, env("G"), env("R"), up(t["AC"]), up(t["AR"]), out=out()))
    if op in ("dAC_blocked", "hac_blocked"):
        nblk = t["nblk"]
        Dl = t["x"].shape[0]
        n = Dl // nblk
        G = t["G"][n:2 * n] if rows else t["G"]                  # Dlo = Dl / nblk: one rank's rows of every slab
        dG = be.upload_env(epi._unstack(G, chis))
        xb = be.upload(epi.to_blocks(t["x"], nblk), shape=t["x"].shape)
        y = _nan_like(be, (G.shape[0],) + t["x"].shape[1:], False)
        if op == "dAC_blocked":
            return down(be.dAC_blocked(H, dG, env("R"), xb, nblk, out=y))
        hac = be.hac_create(H, dG, env("R"))
        assert hac.info()["mode"] == int(mode), hac.info()
        return down(hac.apply(xb, out=y, nblk=nblk))
    if op in ("tl", "tl0"):
        return down_env(be.transfer_left(H, env("G"), up(t["A"]), up(t["Ab"]), out=_env_out(be, t, cplx), cplx=cplx))
    if op in ("tr", "tr0"):
        return down_env(be.transfer_right(H, env("R"), up(t["A"]), up(t["Ab"]), out=_env_out(be, t, cplx), cplx=cplx))
    if op == "reg":
        v = env("v")
        be.regularize(v, up(t["lvec"]), up(t["rvec"]))
        return down_env(v)
    raise KeyError(op)


def _env_out(be, t, cplx):
    """NaN-filled environment of the shape of the reference [Db, W, Dk], as W slabs"""
    Db, W, Dk = t["ref"].shape
    nan = complex(np.nan, np.nan) if cplx else np.nan
    return (be.upload_env_c if cplx else be.upload_env)([np.full((Db, 1, Dk), nan) for _ in range(W)])


def _profiled(be, fn):
    be.prof_enable(True)
    try:
        y = fn()
        prof = be.prof_summary()
    finally:
        be.prof_enable(False)
    return y, {r["kernel"]: r["launches"] for r in prof}


def _run(be, t, tile, **kw):
    """_apply; on the automatic tile under the event profile, which names the tagged kernels the heuristic chose (the
    untagged launches -- transfers, complex family -- are not in it)"""
    if tuple(tile) != (0, 0):
        return _apply(be, t, **kw)
    got, kernels = _profiled(be, lambda: _apply(be, t, **kw))
    print("kernels:", t["name"], kw, "auto", kernels)
    return got


@pytest.mark.parametrize("c", [c for c in epi.cases_exact() if c[0] not in ("dAC_blocked", "hac_blocked")], ids=epi.case_id)
def test_exact_on_every_tile(be, monkeypatch, tile, c):
    op, shape, cplx, variant, W = c
    if variant == "dense":
        monkeypatch.setenv("MPSK_DENSE_ROUTE", "1")        # read per call: the GEMM route at Wl = Wr = 4, d = 2
    t = epi.case(op, shape, "int", cplx, variant, W)
    rec = ei.compare(_run(be, t, tile), t["ref"], None, f"{t['name']}@{tile}")
    assert rec is None, rec


@pytest.mark.parametrize("c", [c for c in epi.cases_exact() if c[3] == "dense" and c[1] == "ragged"], ids=epi.case_id)
def test_dense_slice_on_the_mix_route(be, monkeypatch, c):
    """MPSK_DENSE_ROUTE=0: the same dense slices through the slab mix, once, at tile (128, 64)"""
    op, shape, cplx, variant, W = c
    monkeypatch.setenv("MPSK_DENSE_ROUTE", "0")
    t = epi.case(op, shape, "int", cplx, variant, W)
    be.lib.mpsk_ctx_force_tile(be.ctx, 128, 64)
    try:
        got = _apply(be, t)
    finally:
        be.lib.mpsk_ctx_force_tile(be.ctx, 0, 0)
    rec = ei.compare(got, t["ref"], None, t["name"])
    assert rec is None, rec


@pytest.mark.parametrize("rows", [False, True], ids=["whole", "rowblock"])
@pytest.mark.parametrize("shape", ["nblk2", "nblk3"])
def test_dAC_blocked_exact_on_every_tile(be, tile, shape, rows):
    """x in nblk row blocks against the unblocked einsum; rowblock: Dlo = Dl / nblk, the second row block of GL"""
    t = epi.case("dAC_blocked", shape, "int", False, "", 0)
    n = t["x"].shape[0] // t["nblk"]
    ref = t["ref"][n:2 * n] if rows else t["ref"]
    rec = ei.compare(_run(be, t, tile, rows=rows), ref, None, f"{t['name']}-{rows}@{tile}")
    assert rec is None, rec


@pytest.mark.parametrize("rows", [False, True], ids=["whole", "rowblock"])
@pytest.mark.parametrize("mode", ["0", "1"])
@pytest.mark.parametrize("shape", ["nblk2", "nblk3"])
def test_hac_apply_blocked_exact_on_every_tile(be, monkeypatch, tile, shape, mode, rows):
    monkeypatch.setenv("MPSK_HAC_MODE", mode)              # read by every mpsk_hac_create
    t = epi.case("hac_blocked", shape, "int", False, "", 0)
    n = t["x"].shape[0] // t["nblk"]
    ref = t["ref"][n:2 * n] if rows else t["ref"]
    rec = ei.compare(_run(be, t, tile, mode=mode, rows=rows), ref, None, f"{t['name']}-mode{mode}-{rows}@{tile}")
    assert rec is None, rec


@pytest.mark.parametrize("c", epi.reg_cases(), ids=epi.case_id)
def test_regularize_exact(be, c):
    """no GEMM, no tile: the dot <lvec^T, v[w]> of integers and the update are exact in any reduction order"""
    op, shape, cplx, variant, W = c
    t = epi.case(op, shape, "int", cplx, variant, W)
    rec = ei.compare(_apply(be, t), t["ref"], None, t["name"])
    assert rec is None, rec


@pytest.mark.parametrize("c", epi.cases_gauss(), ids=epi.case_id)
def test_gaussian_within_the_componentwise_bound(be, monkeypatch, c):
    op, shape, cplx, variant, W = c
    if variant == "dense":
        monkeypatch.setenv("MPSK_DENSE_ROUTE", "1")
    modes = ["0", "1"] if op == "hac_blocked" else [None]
    t = epi.case(op, shape, "gauss", cplx, variant, W)
    for mode in modes:
        if mode is not None:
            monkeypatch.setenv("MPSK_HAC_MODE", mode)
        be.lib.mpsk_ctx_force_tile(be.ctx, 128, 64)
        try:
            got = _apply(be, t, mode=mode)
        finally:
            be.lib.mpsk_ctx_force_tile(be.ctx, 0, 0)
        rec = ei.compare(got, t["ref"], t["bound"], f"{t['name']}-mode{mode}")
        assert rec is None, rec


# ---- degenerate slices ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", epi.degenerate_cases(), ids=lambda c: f"{c[0]}-{c[1]}-{'c128' if c[2] else 'f64'}")
def test_degenerate_slices_exact_on_every_tile(be, tile, c):
    """(a) nothing enters the last level, (b) an interior level nothing enters and one nothing leaves, (c) scalar blocks
    only, (d) no blocks at all -- mpsk_mposlice_create accepts the empty slice and the result is exactly zero, written
    over the NaN the output is pre-filled with"""
    op, which, cplx = c
    t = epi.degenerate_case(op, which, cplx)
    got = _run(be, t, tile)
    rec = ei.compare(got, t["ref"], None, f"{t['name']}@{tile}")
    assert rec is None, rec
    if which == "d":
        assert not got.any() and np.isfinite(got).all()


# ---- more K-segments than MAXSEG -----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", epi.long_cases(), ids=lambda c: f"{c[0]}-W{c[1]}-{'c128' if c[2] else 'f64'}")
def test_more_segments_than_one_launch_takes(be, tile, c):
    """33 real levels / 17 complex levels (34 plane segments) of chi 1 on tiny bonds: gemm_segments splits the list of the
    stage over the levels into launches of at most 32 segments, the later ones with beta = 1.  The event profile counts
    the tagged launches (the real dAC and dC: stage 1, then TWO launches of the stage over the levels)."""
    op, W, cplx = c
    t = epi.long_case(op, W, cplx)
    got, kernels = _profiled(be, lambda: _apply(be, t))
    print("kernels:", t["name"], tile, kernels)
    rec = ei.compare(got, t["ref"], None, f"{t['name']}@{tile}")
    assert rec is None, rec
    if op in ("dAC", "dC") and not cplx:
        assert sum(kernels.values()) == 3 and all(k.startswith("dac_gemm_f64_kernel") for k in kernels), kernels


def test_right_combined_operator_with_more_than_32_segments(be, monkeypatch, tile):
    """MPSK_HAC_MODE=1 on 20 levels, d = 2: rc_nseg = 39 K-segments per t, read from the per-batch device table in ONE
    launch of dac_gemm_zs_f64_kernel (the inline tables stop at 32)"""
    monkeypatch.setenv("MPSK_HAC_MODE", "1")
    t = epi.long_case("dAC", epi.HAC_LONG_W, False)
    ns = epi.rc_nseg(t["O"])
    assert ns > epi.MAXSEG, ns
    s = t["s"]
    H = be.mposlice(s.odim, s.d, s.chil, s.chir, dict(s.Os))
    hac = be.hac_create(H, be.upload_env(epi._unstack(t["G"], t["chis"])), be.upload_env(epi._unstack(t["R"], t["chis"])))
    assert hac.info()["mode"] == 1, hac.info()
    y, kernels = _profiled(be, lambda: be.download(hac.apply(be.upload(t["x"]), out=_nan_like(be, t["ref"].shape, False))))
    print("kernels:", t["name"], "rc_nseg", ns, tile, kernels)
    rec = ei.compare(y, t["ref"], None, f"hac-mode1-{t['name']}@{tile}")
    assert rec is None, rec
    zs = {k: n for k, n in kernels.items() if k.startswith("dac_gemm_zs_f64_kernel")}
    assert sum(zs.values()) == 1 and sum(kernels.values()) == 2, kernels
