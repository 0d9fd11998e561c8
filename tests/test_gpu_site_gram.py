"""mpsk_site_gram and mpsk_transfer_left_gram through the backend, both dtypes.

Exact cases: small integer inputs (|x| <= 4), so every partial sum is an exact double whatever the order; the expected value
is a NumPy int64 einsum and the assertion is equality of bits.  Gaussian cases: the any-order summation bound
n 2^-53 sum |Ab| |X| per entry (n terms), reference in long double; the same call twice returns the same bits."""
import numpy as np
import pytest
import torch

import mpskit_jl_amd as mk
from mpskit_jl_amd.backend import DTensor

from exact_vector_inputs import DOT_BLOCKS, THREADS

pytestmark = pytest.mark.gpu

GUARD = 8
SENTINEL = -7.25
U = 2.0 ** -53


def _ints(rng, shape, cplx):
    a = rng.integers(-4, 5, size=shape)
    return a + 1j * rng.integers(-4, 5, size=shape) if cplx else a


def _gauss(rng, shape, cplx):
    a = rng.standard_normal(shape)
    return a + 1j * rng.standard_normal(shape) if cplx else a


def _dev(be, a, cplx):
    """host [.., p, s, b] tensor or stack of tensors [w, p, s, b] -> device slabs, interleaved when complex"""
    a = np.asarray(a, dtype=np.complex128 if cplx else np.float64)
    slabs = a.reshape((-1,) + a.shape[-3:]) if a.ndim == 4 else a[None]
    flat = np.concatenate([np.ravel(s, order="F") for s in slabs])
    if cplx:
        flat = flat.view(np.float64)
    buf = torch.from_numpy(np.ascontiguousarray(flat)).to(be.device)
    c = 2 if cplx else 1
    shape = (c * a.shape[-3],) + a.shape[-2:]
    return DTensor(buf, shape if a.ndim == 3 else (a.shape[0],) + shape)


def _guarded(be, W, d, cplx):
    n = W * d * d * (2 if cplx else 1)
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.float64, device=be.device)
    return DTensor(buf[:n], (W, (2 if cplx else 1) * d, d)), buf


def _host(buf, W, d, cplx):
    """(gram[w, t, s], guard words)"""
    n = W * d * d * (2 if cplx else 1)
    h = buf.cpu().numpy()
    g = h[:n].view(np.complex128) if cplx else h[:n]
    return g.reshape(W, d, d).transpose(0, 2, 1).copy(), h[n:]


def _int_ref(X, Ab, cplx):
    """out[w,t,s] = sum_{p,b} conj(Ab[p,t,b]) X[w,p,s,b] in int64"""
    if not cplx:
        return np.einsum("ptb,wpsb->wts", Ab.astype(np.int64), X.astype(np.int64)).astype(np.float64)
    ar, ai = Ab.real.astype(np.int64), Ab.imag.astype(np.int64)
    xr, xi = X.real.astype(np.int64), X.imag.astype(np.int64)
    re = np.einsum("ptb,wpsb->wts", ar, xr) + np.einsum("ptb,wpsb->wts", ai, xi)
    im = np.einsum("ptb,wpsb->wts", ar, xi) - np.einsum("ptb,wpsb->wts", ai, xr)
    return re.astype(np.float64) + 1j * im.astype(np.float64)


def _same_bits(got, ref):
    got, ref = np.ascontiguousarray(got) + 0.0, np.ascontiguousarray(ref, dtype=got.dtype)
    return np.array_equal(got.view(np.uint64), (ref + 0.0).view(np.uint64))     # (+ 0.0: no negative zeros from int64)


def _run(be, X, Ab, cplx):
    W, d = X.shape[0], X.shape[2]
    out, buf = _guarded(be, W, d, cplx)
    be.site_gram(_dev(be, X, cplx), _dev(be, Ab, cplx), out=out, cplx=cplx)
    g, guard = _host(buf, W, d, cplx)
    assert np.all(guard == SENTINEL), "guard words after the W d^2 outputs were written"
    return g


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("d", [1, 2, 3, 4, 5])
def test_site_gram_exact(be, d, cplx):
    """every d from 1 to 5 (5: the tiled path), even / odd / single-row Dl, more than one block"""
    rng = np.random.default_rng(100 * d + cplx)
    for Dl in (1, 3, 17, 64, 65):
        for Dr in (1, 5, 33):
            for W in (1, 3):
                X, Ab = _ints(rng, (W, Dl, d, Dr), cplx), _ints(rng, (Dl, d, Dr), cplx)
                g = _run(be, X, Ab, cplx)
                assert _same_bits(g, _int_ref(X, Ab, cplx)), (W, d, Dl, Dr)


def _beyond_one_trip(kind):
    """(Dl, Dr) whose item count is one trip of the capped grid (THREADS * DOT_BLOCKS items) plus an odd tail.  An item is a
    p-pair (real, even Dl), one p (real, odd Dl) or one complex element."""
    trip = THREADS * DOT_BLOCKS
    Dr = 513
    rows = 513
    assert rows * Dr > trip and (rows * Dr - trip) % 2 == 1 and rows * Dr < 2 * trip
    return (2 * rows if kind == "pair" else rows), Dr


@pytest.mark.parametrize("kind", ["pair", "single", "c128"])
def test_site_gram_exact_beyond_one_grid_trip(be, kind):
    cplx = kind == "c128"
    Dl, Dr = _beyond_one_trip(kind)
    rng = np.random.default_rng(7)
    X, Ab = _ints(rng, (1, Dl, 2, Dr), cplx), _ints(rng, (Dl, 2, Dr), cplx)
    assert _same_bits(_run(be, X, Ab, cplx), _int_ref(X, Ab, cplx))


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("d", [2, 3, 4, 5])
def test_site_gram_gaussian(be, d, cplx):
    W, Dl, Dr = 2, 65, 33
    rng = np.random.default_rng(200 * d + cplx)
    X, Ab = _gauss(rng, (W, Dl, d, Dr), cplx), _gauss(rng, (Dl, d, Dr), cplx)
    g1, g2 = _run(be, X, Ab, cplx), _run(be, X, Ab, cplx)
    assert _same_bits(g1.view(np.float64), g2.view(np.float64)), "two runs of the same call differ"
    ld = np.clongdouble if cplx else np.longdouble
    ref = np.einsum("ptb,wpsb->wts", np.conj(Ab.astype(ld)), X.astype(ld))
    if cplx:
        n = 2 * Dl * Dr
        a_r, a_i, x_r, x_i = np.abs(Ab.real), np.abs(Ab.imag), np.abs(X.real), np.abs(X.imag)
        b_re = n * U * (np.einsum("ptb,wpsb->wts", a_r, x_r) + np.einsum("ptb,wpsb->wts", a_i, x_i))
        b_im = n * U * (np.einsum("ptb,wpsb->wts", a_r, x_i) + np.einsum("ptb,wpsb->wts", a_i, x_r))
        err = g1 - ref
        print("max err / bound:", float(np.max(np.abs(err.real) / b_re)), float(np.max(np.abs(err.imag) / b_im)))
        assert np.all(np.abs(err.real) <= b_re) and np.all(np.abs(err.imag) <= b_im)
    else:
        bound = Dl * Dr * U * np.einsum("ptb,wpsb->wts", np.abs(Ab), np.abs(X))
        err = np.abs(g1 - ref)
        print("max err / bound:", float(np.max(err / bound)))
        assert np.all(err <= bound)


def _transfer_case(be, cplx):
    W, d, Dl, Dr, Dlb = 2, 3, 5, 6, 7
    rng = np.random.default_rng(11 + cplx)
    Vin, A, Ab = _ints(rng, (W, Dlb, Dl), cplx), _ints(rng, (Dl, d, Dr), cplx), _ints(rng, (Dlb, d, Dr), cplx)
    c = 2 if cplx else 1
    dt = np.complex128 if cplx else np.float64
    flat = np.concatenate([np.ravel(v, order="F") for v in Vin.astype(dt)])
    vin = DTensor(torch.from_numpy(np.ascontiguousarray(flat.view(np.float64))).to(be.device), (W, c * Dlb, Dl))
    return (W, d, Dl, Dr, Dlb), (Vin, A, Ab), (vin, _dev(be, A, cplx), _dev(be, Ab, cplx))


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_transfer_left_gram(be, cplx):
    (W, d, Dl, Dr, Dlb), (Vin, A, Ab), (vin, a, ab) = _transfer_case(be, cplx)
    c = 2 if cplx else 1
    plain = be.transfer_left(None, vin, a, ab, cplx=cplx)
    gram, gbuf = _guarded(be, W, d, cplx)
    vout = be.transfer_left_gram(vin, a, ab, gram, cplx=cplx)
    n = W * c * Dr * Dr
    assert torch.equal(vout.buf[:n].view(torch.int64), plain.buf[:n].view(torch.int64)), "Vout differs from transfer_left"
    g, guard = _host(gbuf, W, d, cplx)
    assert np.all(guard == SENTINEL)
    # the integer einsum: T1[w,p,s,b] = sum_a Vin[w,p,a] A[a,s,b] is exact in doubles
    T1 = np.einsum("wpa,asb->wpsb", Vin, A)
    ref = _int_ref(T1, Ab, cplx)
    assert _same_bits(g, ref)
    # site_gram on a T1 made by gemm
    mm = be.gemm_c if cplx else be.gemm
    x = be.empty(W, c * Dlb, d, Dr)
    slab = c * Dlb * d * Dr
    for w in range(W):                                      # (each slab from its own 16-byte aligned upload)
        vw = DTensor(vin.buf[w * c * Dlb * Dl:(w + 1) * c * Dlb * Dl].clone(), (c * Dlb, Dl))
        t1 = mm(vw, a.reshape(c * Dl, d * Dr))
        x.buf[w * slab:(w + 1) * slab].copy_(t1.buf[:slab])
    out2, buf2 = _guarded(be, W, d, cplx)
    be.site_gram(x, ab, out=out2, cplx=cplx)
    assert _same_bits(_host(buf2, W, d, cplx)[0], ref)
    # last site: the same Gram, nothing transferred
    poison = DTensor(torch.full((n,), SENTINEL, dtype=torch.float64, device=be.device), (W, c * Dr, Dr))
    gram3, gbuf3 = _guarded(be, W, d, cplx)
    assert be.transfer_left_gram(vin, a, ab, gram3, out=poison, last=True, cplx=cplx) is None
    assert _same_bits(_host(gbuf3, W, d, cplx)[0], ref)
    assert bool(torch.all(poison.buf == SENTINEL)), "last=True wrote a Vout"


def test_transfer_left_gram_needs_equal_right_bonds(be):
    rng = np.random.default_rng(3)
    vin = be._upload_slabs([_ints(rng, (4, 3), False) for _ in range(2)])
    a, ab = be.upload(_ints(rng, (3, 2, 5), False)), be.upload(_ints(rng, (4, 2, 6), False))
    with pytest.raises(mk.MpskError):
        be.transfer_left_gram(vin, a, ab, be.empty(2, 2, 2))
