"""Dense MPO slices (mpsk_mposlice_create_dense): the GEMM route of mpsk_dAC / mpsk_hac_apply / mpsk_transfer_left /
mpsk_transfer_right against numpy.einsum, against the mix route of the same O, the route choice, workspace growth on a
fresh context, and leading_boundary end to end on the classical Ising model."""
import math

import numpy as np
import pytest

import mpskit_jl_amd as mk

pytestmark = pytest.mark.gpu

RTOL = 2e-13
SLICES = [(2, 2, 2), (3, 5, 2), (4, 4, 4), (9, 7, 3), (16, 16, 16)]          # (Wl, Wr, d)
BONDS = [(1, 1), (7, 13), (64, 64), (130, 96), (256, 256)]                   # (Dl, Dr)


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _slabs(be, arr):
    """host [D1, D2, W] (slab w = arr[:, :, w]) -> device environment (W, D1, D2)."""
    return be.upload(arr).reshape(arr.shape[2], arr.shape[0], arr.shape[1])


def _env_host(be, t):
    W, D1, D2 = t.shape
    return be.download(t.reshape(D1, D2, W))


def DTensorView(t, W):
    """the first W slabs of an environment."""
    return mk.DTensor(t.buf, (W,) + t.shape[1:])


def _ops(be, Hs, O, Dl, Dr, rng):
    """All four operators with slice Hs; returns (results, references)."""
    Wl, d, _, Wr = O.shape
    G = rng.standard_normal((Dl, Dl, Wl))
    R = rng.standard_normal((Dr, Dr, Wr))
    x = rng.standard_normal((Dl, d, Dr))
    Ab = rng.standard_normal((Dl, d, Dr))
    dG, dR, dx, dAb = _slabs(be, G), _slabs(be, R), be.upload(x), be.upload(Ab)
    got = {
        "dAC": be.download(be.dAC(Hs, dG, dR, dx)),
        "hac": be.download(be.hac_create(Hs, dG, dR).apply(dx)),
        "tl": _env_host(be, be.transfer_left(Hs, dG, dx, dAb)),
        "tr": _env_host(be, be.transfer_right(Hs, dR, dx, dAb)),
    }
    return got, reference(G, R, x, Ab, O)


def reference(G, R, x, Ab, O):
    """numpy.einsum of the three contractions, evaluated pairwise (a four-operand einsum of these shapes does not finish
    in reasonable time on the host):
      dAC  y[p,t,q]     = G[p,a,w] x[a,s,b] O[w,t,s,v] R[b,q,v]
      tl   out[q,b,v]   = G[p,a,w] x[a,s,b] O[w,t,s,v] Ab[p,t,q]
      tr   out[a,p,w]   = x[a,s,b] O[w,t,s,v] Ab[p,t,q] R[b,q,v]"""
    T1 = np.einsum("paw,asb->pwsb", G, x, optimize=True)
    T2 = np.einsum("pwsb,wtsv->pbtv", T1, O, optimize=True)
    S1 = np.einsum("ptq,bqv->ptbv", Ab, R, optimize=True)
    S2 = np.einsum("ptbv,wtsv->pbws", S1, O, optimize=True)
    y = np.einsum("pbtv,bqv->ptq", T2, R, optimize=True)
    return {"dAC": y, "hac": y,
            "tl": np.einsum("pbtv,ptq->qbv", T2, Ab, optimize=True),
            "tr": np.einsum("asb,pbws->apw", x, S2, optimize=True)}


@pytest.mark.parametrize("Wl,Wr,d", SLICES)
def test_dense_route_parity_einsum(be, monkeypatch, Wl, Wr, d):
    """The GEMM route (forced on for every shape) against numpy.einsum, and against the mix route of the same O built
    through mpsk_mposlice_create: 2e-13 D relative."""
    monkeypatch.setenv("MPSK_DENSE_ROUTE", "1")
    rng = np.random.default_rng(100 * Wl + 10 * Wr + d)
    O = rng.standard_normal((Wl, d, d, Wr))
    Hd = be.mposlice_dense(O)
    Hm = be.mposlice(1, d, [Wl], [Wr], {(0, 0): O})
    for Dl, Dr in BONDS:
        bar = RTOL * max(Dl, Dr)
        got, ref = _ops(be, Hd, O, Dl, Dr, np.random.default_rng(Dl * 1000 + Dr))
        for k in got:
            assert relerr(got[k], ref[k]) < bar, (k, Wl, Wr, d, Dl, Dr, relerr(got[k], ref[k]))
        if Dl * Dr <= 130 * 96:
            gm, _ = _ops(be, Hm, O, Dl, Dr, np.random.default_rng(Dl * 1000 + Dr))
            for k in got:
                assert relerr(got[k], gm[k]) < bar, ("routes", k, Wl, Wr, d, Dl, Dr)


def test_routes_agree_and_choice(be, monkeypatch):
    """Automatic route: dense slices at chi d >= 8 report mode 4 and agree with the mix route of mpsk_mposlice_create; the
    plain Ising tensor (chi = d = 2) is prepared like the mpsk_mposlice_create slice (mode 0 / 1); MPSK_DENSE_ROUTE forces
    either."""
    monkeypatch.delenv("MPSK_DENSE_ROUTE", raising=False)
    rng = np.random.default_rng(7)
    D = 64
    G = _slabs(be, rng.standard_normal((D, D, 16)))
    R = _slabs(be, rng.standard_normal((D, D, 16)))
    for chi, d, mode in [(2, 2, None), (2, 4, 4), (4, 2, 4), (4, 4, 4), (16, 16, 4)]:
        O = rng.standard_normal((chi, d, d, chi))
        Hd, Hm = be.mposlice_dense(O), be.mposlice(1, d, [chi], [chi], {(0, 0): O})
        g, r = DTensorView(G, chi), DTensorView(R, chi)
        x = be.upload(rng.standard_normal((D, d, D)))
        hd, hm = be.hac_create(Hd, g, r), be.hac_create(Hm, g, r)
        assert hm.info()["mode"] in (0, 1)
        assert hd.info()["mode"] == (hm.info()["mode"] if mode is None else mode), (chi, d, hd.info())
        assert relerr(be.download(hd.apply(x)), be.download(hm.apply(x))) < RTOL * D
    O = rng.standard_normal((16, 16, 16, 16))
    Hd = be.mposlice_dense(O)
    g, r = DTensorView(G, 16), DTensorView(R, 16)
    monkeypatch.setenv("MPSK_DENSE_ROUTE", "0")
    assert be.hac_create(Hd, g, r).info()["mode"] == 0
    monkeypatch.setenv("MPSK_DENSE_ROUTE", "1")
    H2 = be.mposlice_dense(np.ones((2, 2, 2, 2)))
    assert be.hac_create(H2, DTensorView(G, 2), DTensorView(R, 2)).info()["mode"] == 4


def test_complex_dense_slice_refused(be):
    import ctypes as C
    h = C.c_void_p()
    O = np.zeros(2 * 16)
    rc = be.lib.mpsk_mposlice_create_dense(be.ctx, 1, 2, 2, 2, O.ctypes.data, C.byref(h))
    assert rc == 1 and b"MPSK_F64" in be.lib.mpsk_last_error()
    with pytest.raises(mk.MpskError):
        be.mposlice_dense(np.ones((2, 2, 2, 2)) * 1j)


@pytest.mark.parametrize("order", ["small_then_large", "large_then_small"])
def test_workspace_fresh_context(monkeypatch, order):
    """A fresh context sizes the dense route's intermediates through its workspace in both orders of use."""
    monkeypatch.setenv("MPSK_DENSE_ROUTE", "1")
    b = mk.Backend(0)
    try:
        rng = np.random.default_rng(5)
        shapes = [((3, 5, 2), (7, 13)), ((16, 16, 16), (256, 256))]
        if order == "large_then_small":
            shapes = shapes[::-1]
        for (Wl, Wr, d), (Dl, Dr) in shapes + shapes:
            O = rng.standard_normal((Wl, d, d, Wr))
            got, ref = _ops(b, b.mposlice_dense(O), O, Dl, Dr, rng)
            for k in got:
                assert relerr(got[k], ref[k]) < RTOL * max(Dl, Dr), (order, k, Dl, Dr)
    finally:
        b.synchronize()
        b.close()


def test_leading_boundary_cluster4_matches_onsager(be):
    """beta = 0.3, 4 x 4 clusters (chi = d = 16, the GEMM route), D = 32: kappa^16 per tensor to 1e-9."""
    from test_statmech_cpu import onsager_kappa
    mpo = mk.classical_ising(0.3, cluster=4)
    psi = mk.InfiniteMPS.random(16, 32, np.random.default_rng(1), be=be)
    psi, envs, eps = mk.leading_boundary(psi, mpo, mk.VUMPS(tol=1e-9, maxiter=100))
    assert envs.ddAC(0, psi)._prepare().info()["mode"] == 4
    lam = mk.expectation_value(psi, mpo, envs)[0]
    assert abs(lam / onsager_kappa(0.3) ** 16 - 1.0) < 1e-9, (lam, eps)


def test_leading_boundary_critical_ising(be):
    """test/algorithms.jl:185-201 on the device: 2.5337 +- 1e-3 at D = 24."""
    beta = math.log(1.0 + math.sqrt(2.0)) / 2.0
    mpo = mk.classical_ising(beta)
    psi = mk.InfiniteMPS.random(2, 24, np.random.default_rng(1), be=be)
    psi, envs, eps = mk.leading_boundary(psi, mpo, mk.VUMPS(tol=1e-6, maxiter=200))
    lam = mk.expectation_value(psi, mpo, envs)[0]
    assert lam == pytest.approx(2.5337, abs=1e-3)
    assert eps <= 1e-6
    xi = mk.correlation_length(psi)
    assert xi > 1.0
