"""mpsk_transfer_left_gram_env (the fused closing product of window.transition) and WindowMPS on the device.

Kernel cases.  Exact: small integer inputs (|x| <= 2), so every partial sum of the three nested contractions is an exact
double whatever the order (the largest case stays below 2^40); the expected value is a NumPy int64 contraction and the
assertion is equality of bits.  Gaussian: the any-order summation bound.  gram[t,s] is a sum over (p, a, b, q) evaluated as
three nested sums of lengths Dl, Dr and Dlb Drb; each real product / sum rounds once, a complex one is two real sums of twice
the length, so every computed entry is within  n u sum |Ab| |Lin| |A| |R|  of the exact one with
n = c (Dl + Dr + Dlb Drb) + 8  (c = 2 for complex; the 8 covers the products and the two closing partial-sum stages), u = 2^-53,
to first order in u.  The reference is a long double einsum."""
import numpy as np
import pytest
import torch

import mpskit_jl_amd as mk
from mpskit_jl_amd.backend import DTensor

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
GUARD = 8
SENTINEL = -7.25

# (Dl, Dr, Dlb, Drb): one 16-wide corner of a tile; ragged edges on every side; several tiles with Dl != Dlb, Dr != Drb;
# odd sizes above two tiles; exact multiples of the 64 x 64 tile and of the 16-deep k-tile (the vector-load kernels, real
# and complex)
SHAPES = [(16, 16, 16, 16), (17, 33, 19, 35), (64, 48, 80, 64), (130, 66, 96, 131), (32, 48, 64, 128)]


def _ints(rng, shape, cplx):
    a = rng.integers(-2, 3, size=shape)
    return a + 1j * rng.integers(-2, 3, size=shape) if cplx else a


def _gauss(rng, shape, cplx):
    a = rng.standard_normal(shape)
    return a + 1j * rng.standard_normal(shape) if cplx else a


def _dev(be, a, cplx):
    """host array (logical index order) -> device column-major, interleaved when complex (first dimension doubled)"""
    a = np.asarray(a, dtype=np.complex128 if cplx else np.float64)
    flat = np.ravel(a, order="F")
    if cplx:
        flat = flat.view(np.float64)
    buf = torch.from_numpy(np.ascontiguousarray(flat)).to(be.device)
    return DTensor(buf, ((2 if cplx else 1) * a.shape[0],) + a.shape[1:])


def _guarded(be, d, cplx):
    n = d * d * (2 if cplx else 1)
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.float64, device=be.device)
    return DTensor(buf[:n], ((2 if cplx else 1) * d, d)), buf


def _host(buf, d, cplx):
    """(gram[t, s], guard words)"""
    n = d * d * (2 if cplx else 1)
    h = buf.cpu().numpy()
    g = h[:n].view(np.complex128) if cplx else h[:n]
    return g.reshape(d, d, order="F").copy(), h[n:]


def _parts(z):
    return (z.real.astype(np.int64), z.imag.astype(np.int64)) if np.iscomplexobj(z) else (z.astype(np.int64), None)


def _imul(path, x, y):
    """integer (Gaussian-integer) einsum of two operands"""
    xr, xi = _parts(x)
    yr, yi = _parts(y)
    if xi is None and yi is None:
        return np.einsum(path, xr, yr)
    xi = np.zeros_like(xr) if xi is None else xi
    yi = np.zeros_like(yr) if yi is None else yi
    return (np.einsum(path, xr, yr) - np.einsum(path, xi, yi)) + 1j * (np.einsum(path, xr, yi) + np.einsum(path, xi, yr))


def _int_ref(Lin, A, Ab, R):
    """gram[t,s] = sum conj(Ab[p,t,q]) Lin[p,a] A[a,s,b] R[b,q], exact"""
    X = _imul("psb,bq->psq", _imul("pa,asb->psb", Lin, A), R)
    return _imul("ptq,psq->ts", np.conj(Ab), X)


def _same_bits(got, ref):
    got = np.ascontiguousarray(got) + 0.0
    ref = np.ascontiguousarray(ref, dtype=got.dtype) + 0.0          # (+ 0.0: no negative zeros)
    return np.array_equal(got.view(np.uint64), ref.view(np.uint64))


def _operands(be, gen, rng, shape, d, cplx):
    Dl, Dr, Dlb, Drb = shape
    host = gen(rng, (Dlb, Dl), cplx), gen(rng, (Dl, d, Dr), cplx), gen(rng, (Dlb, d, Drb), cplx), gen(rng, (Dr, Drb), cplx)
    return host, tuple(_dev(be, h, cplx) for h in host)


def _run(be, dev, d, cplx, last=False, out=None):
    gram, buf = _guarded(be, d, cplx)
    y = be.transfer_left_gram_env(*dev, gram, out=out, last=last, cplx=cplx)
    g, guard = _host(buf, d, cplx)
    assert np.all(guard == SENTINEL), "guard words after the d^2 outputs were written"
    return g, y


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("d", [2, 3, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gram_env_exact(be, shape, d, cplx):
    rng = np.random.default_rng(sum(shape) + 10 * d + cplx)
    host, dev = _operands(be, _ints, rng, shape, d, cplx)
    g, lout = _run(be, dev, d, cplx)
    assert _same_bits(g, _int_ref(*host)), (shape, d)
    # Lout: the bits of the plain pass-through transfer
    Dl, Dr, Dlb, Drb = shape
    c = 2 if cplx else 1
    lin1 = DTensor(dev[0].buf, (1,) + dev[0].shape)
    plain = be.transfer_left(None, lin1, dev[1], dev[2], cplx=cplx)
    n = c * Drb * Dr
    assert torch.equal(lout.buf[:n].view(torch.int64), plain.buf[:n].view(torch.int64)), "Lout differs from transfer_left"
    # last site: nothing transferred, the same Gram bit for bit
    poison = DTensor(torch.full((n,), SENTINEL, dtype=torch.float64, device=be.device), (1, c * Drb, Dr))
    g2, none = _run(be, dev, d, cplx, last=True, out=poison)
    assert none is None and bool(torch.all(poison.buf == SENTINEL)), "last=True wrote an Lout"
    assert _same_bits(g2.view(np.float64), g.view(np.float64)), "the Gram depends on Lout"


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_gram_env_exact_more_tiles_than_workgroups(be, cplx):
    """33 x 32 tiles of 64 x 64 (complex: 66 x 32) against at most 1024 workgroups per physical index: workgroups that walk
    more than one tile add to their own partial"""
    shape, d = (2, 16, 2112, 2048), 2
    rng = np.random.default_rng(5 + cplx)
    host, dev = _operands(be, _ints, rng, shape, d, cplx)
    g, _ = _run(be, dev, d, cplx, last=True)
    assert _same_bits(g, _int_ref(*host))


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("d", [2, 3, 5])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gram_env_gaussian(be, shape, d, cplx):
    Dl, Dr, Dlb, Drb = shape
    rng = np.random.default_rng(1000 + sum(shape) + 10 * d + cplx)
    (Lin, A, Ab, R), dev = _operands(be, _gauss, rng, shape, d, cplx)
    g1, _ = _run(be, dev, d, cplx)
    g2, _ = _run(be, dev, d, cplx)
    assert _same_bits(g1.view(np.float64), g2.view(np.float64)), "two runs of the same call differ"
    ld = np.clongdouble if cplx else np.longdouble
    X = np.einsum("psb,bq->psq", np.einsum("pa,asb->psb", Lin.astype(ld), A.astype(ld)), R.astype(ld))
    ref = np.einsum("ptq,psq->ts", np.conj(Ab.astype(ld)), X)
    mag = np.einsum("ptq,psq->ts", np.abs(Ab), np.einsum("psb,bq->psq", np.einsum("pa,asb->psb", np.abs(Lin), np.abs(A)),
                                                          np.abs(R)))
    n = (2 if cplx else 1) * (Dl + Dr + Dlb * Drb) + 8
    bound = n * U * mag
    err = np.abs(g1 - ref).astype(np.float64)
    print("max err / bound:", float(np.max(err / bound)))
    assert np.all(err <= bound)


def test_gram_env_rejects_mismatched_operands(be):
    rng = np.random.default_rng(3)
    lin, a, ab = be.upload(_ints(rng, (4, 3), False)), be.upload(_ints(rng, (3, 2, 5), False)), be.upload(_ints(rng, (4, 2, 6), False))
    with pytest.raises(mk.MpskError):
        be.transfer_left_gram_env(lin, a, ab, be.upload(_ints(rng, (5, 7), False)), be.empty(2, 2))


# ---- WindowMPS on the device -------------------------------------------------------------------------------------------------

import json
import os

from mpskit_jl_amd import window
from window_helpers import dense_site_matrices, itfi_groundstate, left_canonical_host, quench


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "cplx"])
def test_transition_device_route_equals_composed(be, cplx):
    """L = 6, D = 24 (bra) / 32 (ket) between environments of D = 16: the fused closing product against gemm + site Gram,
    and both against the dense NumPy contraction.  The tolerance is the kernel bound above with the largest shapes of the
    window, n u sum |.|, taken with sum |.| <= sqrt(Dlb Drb) for tensors of unit Frobenius norm per open index."""
    rng = np.random.default_rng(21 + cplx)
    psi = mk.InfiniteMPS.random(2, 16, rng, be=be)
    dt = np.complex128 if cplx else None
    bra = mk.WindowMPS.random(6, 2, 24, psi, rng=rng, dtype=dt)
    ket = mk.WindowMPS.random(6, 2, 32, psi, rng=rng, dtype=dt)
    fused = window.transition(bra, ket, device=True)
    composed = window.transition(bra, ket, device=False)
    ref = dense_site_matrices(left_canonical_host(bra), left_canonical_host(ket))
    n = (2 if cplx else 1) * (32 + 32 + 24 * 24) + 8
    tol = n * U * np.sqrt(24 * 24)
    for f, c, r in zip(fused, composed, ref):
        print("fused - composed", np.abs(f - c).max(), "fused - dense", np.abs(f - r).max(), "tol", tol)
        assert np.abs(f - c).max() <= tol and np.abs(f - r).max() <= 6 * tol      # (dense: six sites of such sums)
    again = window.transition(bra, ket, device=True)
    assert all(np.array_equal(a, f) for a, f in zip(again, fused))
    assert abs(window.dot(bra, ket) - np.trace(ref[0])) <= 6 * tol


def test_real_window_takes_the_canonical_routes(be, monkeypatch):
    """mode 3 at every site, and a DMRG sweep under MPSK_HAC_CHECK=1: the library itself verifies the identity levels at
    both infinite edges and the isometries on every canonical call"""
    H, psi, envs, eps = itfi_groundstate(be, 16, 1, tol=1e-10)
    w = mk.WindowMPS(psi, 6)
    wenvs = mk.environments(w, H, envs, envs)
    assert wenvs.window_canonical and wenvs._canonical(w.window)
    monkeypatch.setenv("MPSK_HAC_CHECK", "1")
    for pos in (0, 3, 5):
        op = mk.ddAC(pos, w.window, H, wenvs)
        op(w.window.AC(pos))
        assert op._hac.info()["mode"] == 3, pos
    vals, tot = mk.expectation_value(w, H, wenvs)
    w2, wenvs2, _ = mk.find_groundstate(w, H, mk.DMRG(maxiter=1, tol=1e-14), wenvs)
    vals2, tot2 = mk.expectation_value(w2, H, wenvs2)
    assert abs(tot2 - tot) < 1e-9 and np.abs(vals2 - vals).max() < 1e-8


def test_quench_overlaps_against_the_host_backend(be):
    """S^+ at site 4 of a Heisenberg window, five real-time TDVP steps on an interleaved complex window; |<w0|w(t)>| against
    the same algorithm on the host stand-in backend (tests/golden/make_window_quench.py), energy conserved"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_quench.json")) as f:
        gold = json.load(f)
    overlaps, tots = quench(be)
    print("overlaps", overlaps, "golden", gold["abs_overlap"], "tot", tots)
    assert np.abs(np.array(overlaps) - np.array(gold["abs_overlap"])).max() < 1e-8
    assert np.abs(np.array(tots) - tots[0]).max() < 1e-9
