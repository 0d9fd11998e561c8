"""The operator family (dAC, dC, dAC2, the transfers, the rectangular projection, the dense-MPO slice; real and
complex128) on every GEMM tile, against mpskit_oracle on integer-valued inputs -- exact comparison, see
tests/exact_inputs.py -- plus one Gaussian case per operator at tile (128, 64) inside the componentwise bound.

These are the launches mpsk_gemm cannot reach: the tagged dac_gemm_f64_kernel / dac_gemm_zs_f64_kernel bodies (stage 1 and
stage 3 of mpsk_dAC / mpsk_hac_apply, K-segments over the MPO levels, batch offset tables of the dense route) and the
complex128 family cgemm_f64_kernel (J-aware loader: segJ = 1 in stage 1, segJ = 2 under TB in transfer_right, the
transposed K-contiguous loader with segJ = 0 / 1 and row-strided C in transfer_left).  Mode 3 of the prepared operator
and the canonical transfers get the same exact treatment in test_gpu_canonical_exact.py (identity levels are integer
data, dyadic Hadamard blocks are exact isometries: tests/exact_canonical_inputs.py)."""
import numpy as np
import pytest

import exact_inputs as ei

pytestmark = pytest.mark.gpu

TILE_IDS = [f"{t[0]}x{t[1]}" for t in ei.TILES]


@pytest.fixture(params=ei.TILES, ids=TILE_IDS)
def tile(request, be):
    be.lib.mpsk_ctx_force_tile(be.ctx, *request.param)
    try:
        yield request.param
    finally:
        be.lib.mpsk_ctx_force_tile(be.ctx, 0, 0)           # process-wide knob


def _apply(be, t, op, cplx, variant, via="abi"):
    """run operator `op` on the operands of case `t`; result in the oracle's layout (transfers stacked over levels)"""
    s = t["s"]
    up, down = (be.upload_c, be.download_c) if cplx else (be.upload, be.download)
    up_env, down_env = (be.upload_env_c, be.download_env_c) if cplx else (be.upload_env, be.download_env)
    if variant == "dense":
        H = be.mposlice_dense(t["O"])
    elif op != "dC":
        H = be.mposlice(s.odim, s.d, s.chil, s.chir, dict(s.Os), cplx=cplx)
    if op == "dAC":
        GL, GR, x = up_env(t["GL"]), up_env(t["GR"]), up(t["x"])
        if variant == "proj":
            return down(be.dAC_proj(H, GL, GR, x))
        if via == "hac":
            hac = be.hac_create(H, GL, GR)
            return down(hac.apply(x)), hac.info()["mode"]
        return down(be.dAC(H, GL, GR, x))
    if op == "dC":
        return down(be.dC(up_env(t["GL"]), up_env(t["GR"]), up(t["x"]), cplx=cplx))
    if op == "dAC2":
        s2 = t["s2"]
        H2 = be.mposlice(s2.odim, s2.d, s2.chil, s2.chir, dict(s2.Os), cplx=cplx)
        return down(be.dAC2(H, H2, up_env(t["GL"]), up_env(t["GR"]), up(t["x"])))
    if op == "tl":
        return np.concatenate(down_env(be.transfer_left(H, up_env(t["GL"]), up(t["A"]), up(t["Ab"])), t["chis"]), axis=1)
    if op == "tr":
        return np.concatenate(down_env(be.transfer_right(H, up_env(t["GR"]), up(t["A"]), up(t["Ab"])), t["chis"]), axis=1)
    raise KeyError(op)


def _id(c):
    op, shape, cplx, variant = c
    return f"{op}{'-' + variant if variant else ''}-{'c128' if cplx else 'f64'}-{shape[0]}x{shape[1]}"


@pytest.mark.parametrize("case", ei.op_cases_exact(), ids=_id)
def test_operator_exact_on_every_tile(be, monkeypatch, tile, case):
    op, shape, cplx, variant = case
    if variant == "dense":
        monkeypatch.setenv("MPSK_DENSE_ROUTE", "1")        # read per call: the GEMM route at Wl = Wr = 4, d = 2
    t = ei.op_case(op, shape, "int", cplx, variant)
    rec = ei.compare(_apply(be, t, op, cplx, variant), t["ref"], None, f"{t['name']}@{tile}")
    assert rec is None, rec


@pytest.mark.parametrize("mode", ["0", "1"])
@pytest.mark.parametrize("shape", [ei.RAGGED, ei.ALIGNED], ids=["ragged", "aligned"])
def test_prepared_operator_exact_on_every_tile(be, monkeypatch, tile, shape, mode):
    """mpsk_hac_create / mpsk_hac_apply with the mix form (MPSK_HAC_MODE=0) and the MPO folded into the right environment
    (=1: two GEMM launches with per-batch K-segment tables, dac_gemm_zs_f64_kernel) -- the same bits either way"""
    monkeypatch.setenv("MPSK_HAC_MODE", mode)              # read by every mpsk_hac_create
    t = ei.op_case("dAC", shape, "int", False, "")
    y, got_mode = _apply(be, t, "dAC", False, "", via="hac")
    assert got_mode == int(mode), got_mode
    rec = ei.compare(y, t["ref"], None, f"hac-mode{mode}-{t['name']}@{tile}")
    assert rec is None, rec


@pytest.mark.parametrize("via,mode", [("abi", None), ("hac", "0"), ("hac", "1")])
def test_dAC_long_k_on_the_automatic_tile(be, monkeypatch, via, mode):
    """D = 256: stage 3 has 80 k-tiles on 32 tiles of 64x64, where the cost model may split K -- the tagged split bodies
    (dac_gemm_sk_f64_kernel, dac_gemm_sk_zs_f64_kernel) that a forced tile never takes.  The event profile names the
    kernels that ran; which ones is the cost model's business, the result is exact either way."""
    if mode is not None:
        monkeypatch.setenv("MPSK_HAC_MODE", mode)
    t = ei.op_case("dAC", ei.LONGK, "int", False, "")
    be.prof_enable(True)
    try:
        y = _apply(be, t, "dAC", False, "", via=via)
        kernels = sorted(r["kernel"] for r in be.prof_summary())
    finally:
        be.prof_enable(False)
    print("kernels:", via, mode, kernels)
    rec = ei.compare(y[0] if via == "hac" else y, t["ref"], None, f"{via}-{mode}-{t['name']}")
    assert rec is None, rec


@pytest.mark.parametrize("case", ei.op_cases_gauss(), ids=_id)
def test_operator_gaussian_within_the_componentwise_bound(be, monkeypatch, case):
    op, shape, cplx, variant = case
    if variant == "dense":
        monkeypatch.setenv("MPSK_DENSE_ROUTE", "1")
    t = ei.op_case(op, shape, "gauss", cplx, variant)
    be.lib.mpsk_ctx_force_tile(be.ctx, 128, 64)
    try:
        got = _apply(be, t, op, cplx, variant)
    finally:
        be.lib.mpsk_ctx_force_tile(be.ctx, 0, 0)
    rec = ei.compare(got, t["ref"], t["bound"], t["name"])
    assert rec is None, rec
