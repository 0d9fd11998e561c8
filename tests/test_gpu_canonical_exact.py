"""The Jordan-form H_AC (mpsk_hac_create_ex with MPSK_HAC_CANONICAL / MPSK_HAC_CANONICAL_C128, mode 3) and the canonical
environment transfers (mpsk_transfer_left_ex / mpsk_transfer_right_ex with MPSK_TRANSFER_CANONICAL) against the general
oracle on inputs whose result is exact -- integer environments with identity levels, integer Jordan-form slices, dyadic
isometries; see tests/exact_canonical_inputs.py -- so the comparison is np.array_equal, on every forced GEMM tile, at odd
extents (odd segment tables, the unaligned loader, the scalar mix_kernel<false>), on slices whose per-t slab lists are
padded, with one and with two launches, at D = 256 on the automatic tile (split-K territory), through
mpsk_hac_apply_axpby, under MPSK_HAC_CHECK=1, and with the per-shape table caches of one slice handle revisited.
One Gaussian case per route at tile (128, 64) is held to the componentwise bound."""
import numpy as np
import pytest

import exact_inputs as ei
import exact_canonical_inputs as eci

pytestmark = pytest.mark.gpu

TILE_IDS = [f"{t[0]}x{t[1]}" for t in ei.TILES]
SHAPE_IDS = lambda s: "x".join(str(v) for v in s)


@pytest.fixture(params=ei.TILES, ids=TILE_IDS)
def tile(request, be):
    be.lib.mpsk_ctx_force_tile(be.ctx, *request.param)
    try:
        yield request.param
    finally:
        be.lib.mpsk_ctx_force_tile(be.ctx, 0, 0)           # process-wide knob


def _ok(got, t, what=""):
    rec = eci.check(got, t, what)
    assert rec is None, rec


# ---- 1. mode 3, real ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", eci.HAC_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("family", eci.FAMILIES)
def test_mode3_exact_on_every_tile(be, monkeypatch, tile, family, shape):
    """(128, 128): one launch, aligned; (65, 65): one launch, odd tables; (34, 66): two launches; (33, 65): two, odd.
    The same operands under MPSK_HAC_MODE=0 / 1 (identities in place, no promise used): the same bits."""
    t = eci.hac_case(family, *shape)
    y, info = eci.run_hac(be, t)
    assert info["mode"] == 3, info
    # nslabs of mpsk_hac_info is jr.n_out + jl.n_out = 2 d^2 for every Jordan-form slice: all it pins is that both folds
    # were planned.  The library does not report jr_nseg / jl_nseg; the mirror's counts are held on the CPU only, and a
    # wrong count or list here shows as wrong bits (sparse: padded lists).
    assert info["combined_slabs"] == t["mirror"]["nslabs"], info
    _ok(y, t, f"@{tile}")
    for mode in ("0", "1"):
        monkeypatch.setenv("MPSK_HAC_MODE", mode)                       # read by every mpsk_hac_create_ex
        y, info = eci.run_hac(be, t, flag=False)
        assert info["mode"] == int(mode), info
        _ok(y, t, f"MPSK_HAC_MODE={mode} @{tile}")


# ---- 2. MPSK_HAC_LAUNCHES=2 ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", eci.HAC_LAUNCH2_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("family", eci.FAMILIES)
def test_two_launch_form_gives_the_bits_of_the_one_launch_form(be, monkeypatch, tile, family, shape):
    t = eci.hac_case(family, *shape)
    y1, i1 = eci.run_hac(be, t)
    monkeypatch.setenv("MPSK_HAC_LAUNCHES", "2")                         # read by every mpsk_hac_create_ex
    y2, i2 = eci.run_hac(be, t)
    assert i1["mode"] == i2["mode"] == 3
    _ok(y1, t, f"one launch @{tile}")
    _ok(y2, t, f"MPSK_HAC_LAUNCHES=2 @{tile}")
    assert np.array_equal(y1, y2)


# ---- 3. long K on the automatic tile ----------------------------------------------------------------------------------
@pytest.mark.parametrize("launches", ["1", "2"])
def test_mode3_long_k_on_the_automatic_tile(be, monkeypatch, launches):
    """D = 256, `full`: the one-launch K loop has 4 segments of 16 k-tiles on 32 tiles of 64 x 64, where the cost model
    may split K (the tagged split bodies a forced tile never takes).  The event profile names the kernels that ran; which
    ones is the cost model's business, the result is exact either way."""
    monkeypatch.setenv("MPSK_HAC_LAUNCHES", launches)
    t = eci.hac_case("full", eci.LONGK, eci.LONGK)
    be.prof_enable(True)
    try:
        y, info = eci.run_hac(be, t)
        kernels = sorted(r["kernel"] for r in be.prof_summary())
    finally:
        be.prof_enable(False)
    print("kernels:", "launches", launches, kernels)
    assert info["mode"] == 3
    _ok(y, t, f"launches={launches}")


# ---- 4. mode 3, complex -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", eci.HAC_C128_SHAPES, ids=SHAPE_IDS)
@pytest.mark.parametrize("family", eci.HAC_C128_FAMILIES)
def test_mode3_complex_exact_on_every_tile(be, tile, family, shape):
    """the library checks the identities of a complex candidate itself: mode 3, not 2, says that it accepted them"""
    t = eci.hac_case(family, *shape, "int", True)
    y, info = eci.run_hac(be, t)
    assert info["mode"] == 3, info
    _ok(y, t, f"@{tile}")
    y, info = eci.run_hac(be, t, flag=False)                             # the mix form of the same operands
    assert info["mode"] == 2, info
    _ok(y, t, f"mode 2 @{tile}")


# ---- 5. mpsk_hac_apply_axpby -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,shape,cplx", [("chi", (33, 65), False), ("full", (128, 128), False),
                                               ("sparse", (33, 65), True), ("full", (128, 128), True)])
def test_apply_axpby_on_mode3_is_exact(be, family, shape, cplx):
    t = eci.hac_case(family, *shape, "int", cplx)
    a0, a1 = ((-2 + 0.5j) if cplx else -2.0), 0.5                        # dyadic: a0 x + a1 (H x) is never rounded
    y, info = eci.run_hac(be, t, axpby=(a1, a0))
    assert info["mode"] == 3
    rec = ei.compare(y, a0 * t["x"] + a1 * t["ref"], None, f"axpby-{t['name']}")
    assert rec is None, rec


# ---- 6. canonical transfers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", eci.FAMILIES)
@pytest.mark.parametrize("side", ["l", "r"])
def test_canonical_transfers_exact_on_every_tile(be, monkeypatch, tile, side, family):
    """Every shape of the family through ONE slice handle, the first shape again at the end (jtabL / jtabR must hand back
    the table of the shape asked for).  Every level equals the oracle's, so the written level is exactly the identity.
    MPSK_TRANSFER_MODE=0 (the dense three-stage route) on the same operands: the same bits."""
    be.prof_enable(True)
    try:
        done = eci.run_transfer_sequence(be, side, family)
        prof = be.prof_summary()
    finally:
        be.prof_enable(False)
    # the canonical route did run: its fold application is the only tagged launch with per-batch tables (one a call)
    assert prof and all("_zs_" in r["kernel"] for r in prof), prof
    assert sum(r["launches"] for r in prof) == len(done), prof
    assert len(done) >= 3 and done[0][0] is done[-1][0]
    for k, (t, got) in enumerate(done):
        _ok(got, t, f"#{k} @{tile}")
        assert np.array_equal(got[:, t["ident"], :], np.eye(t["n_out"]))
    monkeypatch.setenv("MPSK_TRANSFER_MODE", "0")                        # read per call
    H = eci.make_slice(be, done[0][0])
    be.prof_enable(True)
    try:
        dense = [(t, eci.run_transfer(be, H, t)) for t, _ in done[:-1]]
        prof = be.prof_summary()
    finally:
        be.prof_enable(False)
    assert prof == [], prof                                              # the dense route has no tagged launch
    for t, got in dense:
        _ok(got, t, f"MPSK_TRANSFER_MODE=0 @{tile}")


# ---- 7. transfers at D = 256 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["l", "r"])
def test_canonical_transfer_long_k_on_the_automatic_tile(be, side):
    t = eci.transfer_case(side, "full", eci.LONGK, 2, eci.LONGK)
    be.prof_enable(True)
    try:
        got = eci.run_transfer(be, eci.make_slice(be, t), t)
        kernels = sorted(r["kernel"] for r in be.prof_summary())
    finally:
        be.prof_enable(False)
    print("kernels:", side, kernels)
    _ok(got, t)


# ---- 8. the library's own checks accept the constructed inputs -------------------------------------------------------------
def test_constructed_inputs_pass_the_library_checks(be, monkeypatch):
    """MPSK_HAC_CHECK=1: identity levels and isometries verified to 1e-10 by the library at every call (a broken promise
    raises "not canonical")"""
    monkeypatch.setenv("MPSK_HAC_CHECK", "1")
    for family in eci.FAMILIES:
        t = eci.hac_case(family, 33, 65)
        y, info = eci.run_hac(be, t)
        assert info["mode"] == 3
        _ok(y, t, "MPSK_HAC_CHECK=1")
        for side in ("l", "r"):
            shapes = eci.transfer_shapes(family, side)[:2]
            H = None
            for shp in shapes:
                tt = eci.transfer_case(side, family, *shp)
                H = eci.make_slice(be, tt) if H is None else H
                _ok(eci.run_transfer(be, H, tt), tt, "MPSK_HAC_CHECK=1")
    for family in eci.HAC_C128_FAMILIES:
        t = eci.hac_case(family, 33, 65, "int", True)
        y, info = eci.run_hac(be, t)
        assert info["mode"] == 3
        _ok(y, t, "MPSK_HAC_CHECK=1")


# ---- 9. Gaussian cases ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,family,cplx", eci.GAUSS_CASES,
                         ids=[f"{r}-{f}-{'c128' if c else 'f64'}" for r, f, c in eci.GAUSS_CASES])
def test_gaussian_within_the_componentwise_bound(be, route, family, cplx):
    t = eci.gauss_case(route, family, cplx)
    be.lib.mpsk_ctx_force_tile(be.ctx, 128, 64)
    try:
        if route == "hac":
            got, info = eci.run_hac(be, t)
            assert info["mode"] == 3, info
        else:
            got = eci.run_transfer(be, eci.make_slice(be, t), t)
    finally:
        be.lib.mpsk_ctx_force_tile(be.ctx, 0, 0)
    print(f"bound ratio: {t['name']} depth {t['depth']} worst |got - ref| / bound = {eci.bound_ratio(got, t):.4f}")
    _ok(got, t)
