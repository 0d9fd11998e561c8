"""mpsk_regularize_axpby on the device, both dtypes: bit-equal to the exact reference of tests/regularize_axpby_cases.py
(checked without a GPU in test_regularize_axpby_cases_cpu.py) in the general form, with x == NULL and with out aliasing y
or x, into NaN-filled outputs between guard words; repeatable bits; the refusals; the order on a user stream."""
import types

import numpy as np
import pytest

import regularize_axpby_cases as rc
from mpskit_jl_amd.backend import DTensor

pytestmark = pytest.mark.gpu
GUARD = 32            # doubles before and after the output (256 bytes: the output keeps its alignment)
GUARD_WORD = -4242.0
DTYPES = [False, True]
IDS = ["f64", "c128"]


def _guarded(be, n, fill=None):
    """n doubles between guard words: NaN, or `fill` (an in/out operand)"""
    import torch
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float64, device=be.device)
    buf[:GUARD] = GUARD_WORD
    buf[GUARD + n:] = GUARD_WORD
    if fill is not None:
        buf[GUARD:GUARD + n] = torch.from_numpy(np.ascontiguousarray(fill)).to(be.device)
    return buf


def _run(be, shape, cplx, form):
    W, D1, D2 = shape
    m = 2 if cplx else 1
    t = rc.operands(shape, cplx)
    a0, a1 = rc.scalars(shape)
    n = m * W * D1 * D2
    dshape = (W, m * D1, D2)
    up = (lambda a: be.upload_c(a)) if cplx else (lambda a: be.upload(a))
    lvec, rvec = up(t["lvec"]), up(t["rvec"])
    y, x = rc.slabs(be, t["y"], cplx), rc.slabs(be, t["x"], cplx)
    if form == "general":
        buf = _guarded(be, n)
        want = rc.ref(t["y"], t["lvec"], t["rvec"], a1, t["x"], a0)
    elif form == "x is NULL":
        buf, x = _guarded(be, n), None
        a0 = float("nan")                                  # not read
        want = rc.ref(t["y"], t["lvec"], t["rvec"], a1)
    elif form == "out is y":
        buf = _guarded(be, n, rc.flat(t["y"], cplx))
        y = DTensor(buf[GUARD:GUARD + n], dshape)
        want = rc.ref(t["y"], t["lvec"], t["rvec"], a1, t["x"], a0)
    elif form == "out is x":
        buf = _guarded(be, n, rc.flat(t["x"], cplx))
        x = DTensor(buf[GUARD:GUARD + n], dshape)
        want = rc.ref(t["y"], t["lvec"], t["rvec"], a1, t["x"], a0)
    else:                                                  # regularize! in place: x == NULL, a1 = 1, out == y
        buf, x, a1 = _guarded(be, n, rc.flat(t["y"], cplx)), None, 1.0
        y = DTensor(buf[GUARD:GUARD + n], dshape)
        want = rc.ref(t["y"], t["lvec"], t["rvec"], 1.0)
    out = DTensor(buf[GUARD:GUARD + n], dshape)
    r = be.regularize_axpby(y, lvec, rvec, a1=a1, x=x, a0=a0, out=out, cplx=cplx)
    assert r is out
    be.synchronize()
    host = buf.cpu().numpy()
    assert np.all(host[:GUARD] == GUARD_WORD) and np.all(host[-GUARD:] == GUARD_WORD)
    return rc.unflat(host[GUARD:GUARD + n], shape, cplx), want


@pytest.mark.parametrize("cplx", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", rc.SHAPES, ids=str)
@pytest.mark.parametrize("form", ["general", "x is NULL", "out is y", "out is x", "in place"])
def test_exact_behind_guard_words(be, form, shape, cplx):
    got, want = _run(be, shape, cplx, form)
    assert np.array_equal(got, want)


def test_the_symbol_is_exported(be):
    assert hasattr(be.lib, "mpsk_regularize_axpby")


def test_in_place_form_is_mpsk_regularize(be):
    """x == NULL, a1 = 1, out == y against mpsk_regularize (fp64 only) on the same operands: the same bits"""
    shape = (3, 64, 64)
    t = rc.operands(shape, False, seed=3)
    v1, v2 = rc.slabs(be, t["y"], False), rc.slabs(be, t["y"], False)
    l, r = be.upload(t["lvec"]), be.upload(t["rvec"])
    be.regularize(v1, l, r)
    be.regularize_axpby(v2, l, r, out=v2)
    be.synchronize()
    assert np.array_equal(be.download(v1), be.download(v2))


@pytest.mark.parametrize("cplx", DTYPES, ids=IDS)
def test_two_calls_give_the_same_bits(be, cplx):
    """non-integer operands (the order of the reduction matters): the fixed order makes two runs bit-identical"""
    W, D1, D2 = 2, 257, 129
    rng = np.random.default_rng(17)
    z = (lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)) if cplx else (lambda *s: rng.standard_normal(s))
    yh, xh, lh, rh = z(W, D1, D2), z(W, D1, D2), z(D2, D1), z(D1, D2)
    up = be.upload_c if cplx else be.upload
    y, x, l, r = rc.slabs(be, yh, cplx), rc.slabs(be, xh, cplx), up(lh), up(rh)
    a = be.regularize_axpby(y, l, r, a1=-1.0, x=x, a0=1.0, cplx=cplx)
    b = be.regularize_axpby(y, l, r, a1=-1.0, x=x, a0=1.0, cplx=cplx)
    be.synchronize()
    ha, hb = a.buf.cpu().numpy(), b.buf.cpu().numpy()
    assert np.array_equal(ha, hb)
    want = rc.ref(yh, lh, rh, -1.0, xh, 1.0)
    got = rc.unflat(ha[:a.size], (W, D1, D2), cplx)
    # D1 D2 products of O(1) numbers summed in fp64, then one product with rvec: (D1 D2 + 4) u |lvec| |y| |rvec|_max
    bound = (D1 * D2 + 4) * 2.0 ** -53 * np.einsum("qp,wpq->w", np.abs(lh), np.abs(yh)).max() * np.abs(rh).max() \
        + 4 * 2.0 ** -53 * np.abs(want).max()
    assert np.abs(got - want).max() <= bound


def test_refusals(be):
    shape = (2, 33, 31)
    W, D1, D2 = shape
    t = rc.operands(shape, False)
    y, x, out = rc.slabs(be, t["y"], False), rc.slabs(be, t["x"], False), be.empty(W, D1, D2)
    l, r = be.upload(t["lvec"]), be.upload(t["rvec"])
    call = lambda *a: be.lib.mpsk_regularize_axpby(be.ctx, *a)
    msg = lambda: be.lib.mpsk_last_error().decode()
    good = [W, D1, D2, y.ptr, l.ptr, r.ptr, 1.0, x.ptr, 1.0, out.ptr]
    for k in (3, 4, 5, 9):                                 # y, lvec, rvec, out
        bad = list(good)
        bad[k] = None
        assert call(*bad) == 1 and "mpsk_regularize_axpby" in msg() and "NULL" in msg()
    assert be.lib.mpsk_regularize_axpby(None, *good) == 1
    for k in range(3):
        for v in (0, -1):
            bad = list(good)
            bad[k] = v
            assert call(*bad) == 1 and "dimensions" in msg()
    bad = list(good)
    bad[7] = None                                          # x may be NULL
    assert call(*bad) == 0
    assert call(*good) == 0
    be.synchronize()
    got = rc.unflat(out.buf[:out.size].cpu().numpy(), shape, False)
    assert np.array_equal(got, rc.ref(t["y"], t["lvec"], t["rvec"], 1.0, t["x"], 1.0))


@pytest.mark.parametrize("cplx", DTYPES, ids=IDS)
def test_ordered_on_a_user_stream(be, cplx):
    """the delayed producer of tests/stream_order.py: the entry on a non-blocking user stream must return while the producer
    of its operands is pending and still give the exact result of the true operands, not of the decoys"""
    import torch
    import mpskit_jl_amd as mk
    import stream_order as so
    shape = (3, 33, 65)
    W, D1, D2 = shape
    m = 2 if cplx else 1
    true, decoy = rc.operands(shape, cplx, seed=1), rc.operands(shape, cplx, seed=2)
    be2 = mk.Backend(0, stream=torch.cuda.Stream(0))
    try:
        def run(b, dev, _):
            view = lambda name, *s: DTensor(dev[name].buf, s)
            b.regularize_axpby(view("y", W, m * D1, D2), view("lvec", m * D2, D1), view("rvec", m * D1, D2), a1=-1.0,
                               x=view("x", W, m * D1, D2), a0=2.0, out=view("out", W, m * D1, D2), cplx=cplx)
        case = types.SimpleNamespace(
            name="regularize_axpby", family="transfers", setup=None, run=run, sync=False,
            operands={k: (rc.flat(true[k], cplx), rc.flat(decoy[k], cplx)) for k in ("y", "x", "lvec", "rvec")},
            outputs={"out": m * W * D1 * D2})
        got, info = so.Staged(be2, case).delayed(be2, so.Delay(be2.torch_stream))
        assert info["returned_before_produced"]
        out = rc.unflat(got["out"], shape, cplx)
        ref = lambda t: rc.ref(t["y"], t["lvec"], t["rvec"], -1.0, t["x"], 2.0)
        assert np.array_equal(out, ref(true))
        assert not np.array_equal(out, ref(decoy))
    finally:
        be2.synchronize()
        be2.close()
