"""Exact tests of the dense-MPO GEMM route (slices of mpsk_mposlice_create_dense, mpsk_hac_info mode 4) on the cases of
tests/exact_dense_inputs.py: mpsk_dAC, mpsk_dAC_proj, mpsk_hac_apply (plain and nblk = 2 / 3), mpsk_hac_apply_axpby,
mpsk_transfer_left / _right, their _ex forms with MPSK_TRANSFER_CANONICAL set and the pair transfers.

Integer-valued operands: every route returns the same bits and the comparison is np.array_equal.  Every slice shape --
rectangular both ways, odd W, odd d, W = 1, the workload's (16, 16, 16) -- runs at every bond of the list with the route
forced (MPSK_DENSE_ROUTE=1); the ragged rectangular slices and (16, 16, 16) at (64, 64) on the four forced GEMM tiles
and on the automatic one; the ragged cases once more on the mix route of the same slice (MPSK_DENSE_ROUTE=0) and the two
ends of the crossover with the variable unset, all against the same expected bits.  Structured zeros: one output level,
one input level, both, and O == 0 (exact +0.0; mpsk_hac_apply_axpby exactly a0 x).  Every output lies in front of eight
sentinel doubles and is NaN-filled first, so an unwritten element and a write past the end both show; the inputs are
compared with their uploads afterwards.  Invariants that are exact on integers: mpsk_hac_apply is mpsk_dAC bit for bit,
the _ex transfers are the plain ones bit for bit.  One slice handle revisited at three sets of bonds and back (the
per-slice dense_tab cache).  Gaussian cases inside the componentwise bound derived in tests/exact_dense_inputs.py, run
twice for the same bits.  The self-checks of the cases are in tests/test_exact_dense_inputs_cpu.py."""
import numpy as np
import pytest

import exact_dense_inputs as ed
import exact_inputs as ei
import exact_proj_inputs as epi
import mpskit_jl_amd as mk

pytestmark = pytest.mark.gpu

TILES = ei.TILES + [(0, 0)]                                 # (0, 0): the automatic choice
TILE_IDS = [f"{t[0]}x{t[1]}" if t[0] else "auto" for t in TILES]
SENTINEL, NGUARD = -7.25, 8


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


class Guarded:
    """an output of `shape` filled with NaN in front of NGUARD sentinel doubles"""

    def __init__(self, be, *shape):
        self.n = int(np.prod(shape))
        self.full = be.upload(np.concatenate([np.full(self.n, np.nan), np.full(NGUARD, SENTINEL)]))
        self.view = mk.DTensor(self.full.buf, tuple(shape))

    def check(self, be, what):
        tail = be.download(self.full)[self.n:]
        assert tail.shape == (NGUARD,) and np.array_equal(tail, np.full(NGUARD, SENTINEL)), (what, tail)


def _upload(be, t, H=None):
    dv = {"H": be.mposlice_dense(t["O"]) if H is None else H}
    for k in ed.OPERANDS:
        dv[k] = be.upload_env([t[k]]) if k in ed.ENVS else be.upload(t[k])
    return dv


def _assert_inputs_unchanged(be, t, dv):
    for k in ed.OPERANDS:
        got = be.download_env(dv[k], [t[k].shape[1]])[0] if k in ed.ENVS else be.download(dv[k])
        assert np.array_equal(got, t[k]), (t["name"], k)


def _env_host(be, g):
    W = g.view.shape[0]
    return np.concatenate(be.download_env(g.view, [1] * W), axis=1)


def _call(be, t, dv, op, nblk=1, mode4=None):
    """one call of `op` on the uploaded site, in the layout of its reference; guards checked"""
    H, D = dv["H"], t["dims"]
    Wl, d, _, Wr = t["O"].shape
    Dl, Dr = D["Dl"], D["Dr"]
    what = f"{t['name']}-{op}"
    if op in ("dAC", "dAC_proj", "hac", "hac_axpby", "hac_blk"):
        Dlo = Dl if op in ("hac_axpby", "hac_blk") else D["Dlo"]
        g = Guarded(be, Dlo, d, D["Dro"] if op == "dAC_proj" else Dr)
        if op == "dAC":
            be.dAC(H, dv["G"], dv["R"], dv["x"], out=g.view)
        elif op == "dAC_proj":
            be.dAC_proj(H, dv["G"], dv["Rp"], dv["x"], out=g.view)
        else:
            h = be.hac_create(H, dv["G" if op == "hac" else "Gs"], dv["R"])
            if mode4 is not None:
                assert (h.info()["mode"] == 4) == mode4, (what, h.info())
            if op == "hac":
                h.apply(dv["x"], out=g.view)
            elif op == "hac_axpby":
                h.apply_axpby(ed.A1, dv["x"], ed.A0, out=g.view)
            else:
                h.apply(be.upload(epi.to_blocks(t["x"], nblk), shape=t["x"].shape), out=g.view, nblk=nblk)
            h.close()
        got = be.download(g.view)
    else:
        left = op.startswith("tl")
        g = Guarded(be, Wr, D["Drb"], Dr) if left else Guarded(be, Wl, Dl, D["Dlb"])
        if op in ("tl", "tl_ex"):
            be.transfer_left(H, dv["Gt"], dv["x"], dv["Ab"], out=g.view, canonical=op == "tl_ex")
        elif op in ("tr", "tr_ex"):
            be.transfer_right(H, dv["Rt"], dv["x"], dv["Ab"], out=g.view, canonical=op == "tr_ex")
        elif op == "tl_pair":
            be.transfer_left_pair(H, dv["Gt"], dv["x"], dv["V2l"], dv["A2l"], dv["Ab"], out=g.view)
        else:
            be.transfer_right_pair(H, dv["Rt"], dv["x"], dv["V2r"], dv["A2r"], dv["Ab"], out=g.view)
        got = _env_host(be, g)
    g.check(be, what)
    return got


def _same(got, ref, bound, name):
    rec = ei.compare(got, ref, bound, name)
    assert rec is None, rec


def _run_site(be, c, mode4=None, where="", H=None):
    """every operation of site c against its reference, with the invariants; returns {op: result}"""
    t = ed.site(c[0], c[1], "int", c[2], *c[3:])
    dv = _upload(be, t, H)
    got = {}
    for op in ed.ops_of(c[:3]):
        for nblk in (ed.nblks(t) if op == "hac_blk" else [1]):
            y = _call(be, t, dv, op, nblk, mode4)
            _same(y, ed.ref(op, t), None, f"{t['name']}-{op}{'-nblk%d' % nblk if op == 'hac_blk' else ''}{where}")
            got[op] = y
        if t["zeros"] == "all":                              # exact +0.0 over the NaN fill; hac_axpby exactly a0 x
            want = ed.A0 * t["x"] if op == "hac_axpby" else np.zeros_like(y)
            assert np.array_equal(y, want) and not np.signbit(y[want == 0]).any(), (t["name"], op)
    if "hac" in got:
        assert np.array_equal(got["hac"], got["dAC"]), t["name"]                     # mpsk_hac_apply is mpsk_dAC bit for bit
    for op in ("tl", "tr"):
        if op + "_ex" in got:
            assert np.array_equal(got[op + "_ex"], got[op]), (t["name"], op)         # a dense slice falls through to the plain route
    _assert_inputs_unchanged(be, t, dv)
    return got


# ---- every slice shape at every bond, the route forced -------------------------------------------------------------
@pytest.mark.parametrize("c", ed.sites_exact() + ed.sites_zero() + ed.sites_blk(), ids=ed.site_id)
def test_exact_on_the_forced_route(be, monkeypatch, c):
    _route(monkeypatch, "1")
    _run_site(be, c, mode4=True)


@pytest.mark.parametrize("c", ed.sites_tiles(), ids=ed.site_id)
def test_exact_on_every_tile(be, monkeypatch, tile, c):
    _route(monkeypatch, "1")
    _run_site(be, c, mode4=True, where=f"@{tile}")


@pytest.mark.parametrize("c", ed.sites_ragged(), ids=ed.site_id)
def test_mix_route_of_the_same_slice_gives_the_same_bits(be, monkeypatch, c):
    _route(monkeypatch, "0")
    _run_site(be, c, mode4=False, where="-mix")


@pytest.mark.parametrize("c", [(ed.WORKLOAD, b, "") for b in ed.BONDS_WORKLOAD] + [((2, 2, 2), b, "") for b in ed.BONDS],
                         ids=ed.site_id)
def test_both_sides_of_the_automatic_crossover(be, monkeypatch, c):
    """MPSK_DENSE_ROUTE unset: min(Wl, Wr) d = 256 takes the GEMM route (mode 4), 4 stays below MPSK_DENSE_MIN_CHID = 8;
    both return the expected bits"""
    _route(monkeypatch, None)
    _run_site(be, c, mode4=c[0] == ed.WORKLOAD, where="-auto")


# ---- the per-slice offset-table cache --------------------------------------------------------------------------------
def test_offset_table_cache_is_revisited(be, monkeypatch):
    """ONE slice handle (5, 3, 3) on its GEMM route at bonds (7, 13), (13, 7), (64, 64), (7, 13) again -- square
    environments, dense_tab keys (Dl Dl, Dl) -- and (7, 13) with Dlo != Dl, a key of its own.  A table found under a wrong
    key is an unequal element; the fourth visit returns the bits of the first."""
    _route(monkeypatch, "1")
    slc = (5, 3, 3)
    H = be.mposlice_dense(ed.dense_O(slc))
    visits = [(7, 13), (13, 7), (64, 64), (7, 13)]
    out = []
    for b in visits:
        t = ed.site(slc, b, "int", "", ed.square_aux(b))
        dv = _upload(be, t, H)
        got = {op: _call(be, t, dv, op, mode4=None) for op in ("dAC", "tl")}
        for op, y in got.items():
            _same(y, ed.ref(op, t), None, f"{t['name']}-{op}-visit{len(out) + 1}")
        _assert_inputs_unchanged(be, t, dv)
        out.append(got)
    assert all(np.array_equal(out[0][op], out[3][op]) for op in ("dAC", "tl"))
    t = ed.site(slc, (7, 13))
    assert t["dims"]["Dlo"] != t["dims"]["Dl"] and t["dims"]["Dlb"] != t["dims"]["Dl"]
    dv = _upload(be, t, H)
    for op in ("dAC", "tl"):
        _same(_call(be, t, dv, op), ed.ref(op, t), None, f"{t['name']}-{op}-visit5")
    _assert_inputs_unchanged(be, t, dv)


# ---- Gaussian cases --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", ed.GAUSS, ids=lambda g: ed.site_id(g + ("",)))
@pytest.mark.parametrize("op", ed.OPS)
def test_gaussian_within_the_componentwise_bound(be, monkeypatch, op, g):
    _route(monkeypatch, "1")
    t = ed.gauss_site(g[0], g[1], op)
    dv = _upload(be, t)
    ref, bound = ed.ref(op, t), ed.bound_of(op, t)
    for nblk in (ed.nblks(t) if op == "hac_blk" else [1]):
        y = _call(be, t, dv, op, nblk, mode4=True)
        ratio = float((np.abs(y.astype(ei.LD) - ref) / bound).max())
        print(f"dense exact: {t['name']}-{op}{'-nblk%d' % nblk if op == 'hac_blk' else ''}: max err / bound = {ratio:.2e}")
        _same(y, ref, bound, f"{t['name']}-{op}")
        assert np.array_equal(_call(be, t, dv, op, nblk), y), (t["name"], op)        # a repeat call returns the same bits
    _assert_inputs_unchanged(be, t, dv)


# ---- error path --------------------------------------------------------------------------------------------------------
def test_nblk_that_does_not_divide_Dl_is_refused_on_a_mode4_handle(be, monkeypatch):
    _route(monkeypatch, "1")
    t = ed.site((5, 3, 3), (65, 33))
    dv = _upload(be, t)
    h = be.hac_create(dv["H"], dv["Gs"], dv["R"])
    assert h.info()["mode"] == 4
    g = Guarded(be, *t["x"].shape)
    for nblk in (2, 3):
        rc = be.lib.mpsk_hac_apply(h.handle, dv["x"].ptr, nblk, g.view.ptr)
        assert rc != 0 and b"nblk must divide Dl (and be <= 32)" in be.lib.mpsk_last_error(), (rc, be.lib.mpsk_last_error())
    with pytest.raises(mk.MpskError):
        h.apply(dv["x"], out=g.view, nblk=2)
    assert np.isnan(be.download(g.view)).all()               # a refused call writes nothing
    g.check(be, "refused nblk")
    h.close()
