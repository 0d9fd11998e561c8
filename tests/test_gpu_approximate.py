"""mpsk_dAC_proj / mpsk_dAC2_proj / mpsk_vdiff_nrm2 against numpy.einsum, their argument checks, and approximate end to end
on the device (same assertions as tests/test_approximate_cpu.py, plus device route == composed route)."""
import ctypes as C

import numpy as np
import pytest
import torch

import mpskit_jl_amd as mk
from mpskit_jl_amd import native_cplx as nc

import test_approximate_cpu as ac         # the shared NumPy restatements and case bodies (module attributes: not collected twice)

pytestmark = pytest.mark.gpu

RTOL = 2e-13
SEED = 20240213


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _slabs(be, arr):
    """host [D1, D2, W] (slab w = arr[:, :, w]) -> device environment (W, D1, D2)."""
    return be.upload(arr).reshape(arr.shape[2], arr.shape[0], arr.shape[1])


def _slabs_c(be, arr):
    return be.upload_env_c([arr[:, None, :, w] for w in range(arr.shape[2])])


def full_O(H):
    """the [Wl, d, d, Wr] tensor of a device slice from its host block table"""
    ol, orr = np.concatenate([[0], np.cumsum(H.chil)]), np.concatenate([[0], np.cumsum(H.chir)])
    cplx = any(np.iscomplexobj(v) for v in H.blocks.values())
    O = np.zeros((H.Wl, H.d, H.d, H.Wr), dtype=complex if cplx else float)
    for (i, j), v in H.blocks.items():
        blk = v * np.einsum("wv,ts->wtsv", np.eye(H.chil[i], H.chir[j]), np.eye(H.d)) if np.isscalar(v) else np.asarray(v)
        O[ol[i]:ol[i + 1], :, :, orr[j]:orr[j + 1]] = blk
    return O


def ref_dAC(G, R, x, O):
    """y[p,t,q] = G[p,a,w] x[a,s,b] O[w,t,s,v] R[b,q,v], pairwise"""
    T1 = np.einsum("paw,asb->pwsb", G, x, optimize=True)
    T2 = np.einsum("pwsb,wtsv->pbtv", T1, O, optimize=True)
    return np.einsum("pbtv,bqv->ptq", T2, R, optimize=True)


def ref_dAC2(G, R, th, O1, O2):
    """derivatives.jl:156-157 on the formed two-site tensor th[a,s1,b,s2]: y[p,t1,q,t2]"""
    T1 = np.einsum("paw,axbz->pwxbz", G, th, optimize=True)
    T2 = np.einsum("pwxbz,wtxu->ptubz", T1, O1, optimize=True)
    T3 = np.einsum("ptubz,uyzv->ptbyv", T2, O2, optimize=True)
    return np.einsum("ptbyv,bqv->ptqy", T3, R, optimize=True)


def spin1_slice(be):
    return mk.heisenberg_XXX(1.0, be=be)[0]


# ---- mpsk_dAC_proj ---------------------------------------------------------------------------------------------------

PROJ_SHAPES = [(3, 5, 7, 2), (24, 40, 56, 20), (48, 20, 24, 40), (130, 200, 136, 72)]


def _proj_case(be, H, O, Dlo, Dl, Dr, Dro, rng):
    G, R, x = rng.random((Dlo, Dl, H.Wl)), rng.random((Dr, Dro, H.Wr)), rng.random((Dl, H.d, Dr))
    y = be.download(be.dAC_proj(H, _slabs(be, G), _slabs(be, R), be.upload(x)))
    assert y.shape == (Dlo, H.d, Dro)
    e = relerr(y, ref_dAC(G, R, x, O))
    print("dAC_proj", (Dlo, Dl, Dr, Dro), (H.Wl, H.Wr, H.d), e)
    assert e < RTOL * max(Dlo, Dl, Dr, Dro), (Dlo, Dl, Dr, Dro, e)


@pytest.mark.parametrize("model", ["heisenberg", "spin1"])
def test_dac_proj_sparse(be, model):
    H = mk.heisenberg_XXX(0.5, be=be)[0] if model == "heisenberg" else spin1_slice(be)
    assert (H.Wl, H.d) == ((5, 2) if model == "heisenberg" else (5, 3))
    rng = np.random.default_rng(SEED)
    for shp in PROJ_SHAPES:
        _proj_case(be, H, full_O(H), *shp, rng)


@pytest.mark.parametrize("route", ["1", "0"])
def test_dac_proj_dense(be, monkeypatch, route):
    monkeypatch.setenv("MPSK_DENSE_ROUTE", route)
    rng = np.random.default_rng(SEED)
    O = rng.random((4, 4, 4, 4))
    _proj_case(be, be.mposlice_dense(O), O, 24, 40, 56, 20, rng)
    for (Wl, Wr), shp in (((1, 4), (1, 1, 8, 6)), ((4, 1), (6, 8, 1, 1))):       # chain edges
        O = rng.random((Wl, 4, 4, Wr))
        _proj_case(be, be.mposlice_dense(O), O, *shp, rng)


def _cplx_heisenberg(be, rng):
    Sz, Sp, Sm = (np.array(m) for m in ([[0.5, 0], [0, -0.5]], [[0, 1.0], [0, 0]], [[0, 0], [1.0, 0]]))
    ph = lambda: rng.random() + 1j * rng.random()
    blocks = {(0, 0): 1.0, (4, 4): 1.0, (0, 1): ph() * Sz, (1, 4): ph() * Sz, (0, 2): ph() * Sp, (2, 4): ph() * Sm,
              (0, 3): ph() * Sm, (3, 4): ph() * Sp, (0, 4): ph() * Sz}
    blocks = {k: (v if np.isscalar(v) else v[None, :, :, None]) for k, v in blocks.items()}
    return be.mposlice(5, 2, [1] * 5, [1] * 5, blocks, cplx=True)


def test_dac_proj_c128(be):
    rng = np.random.default_rng(SEED)
    H = _cplx_heisenberg(be, rng)
    O = full_O(H)
    cr = lambda *s: rng.random(s) + 1j * rng.random(s)
    for Dlo, Dl, Dr, Dro in PROJ_SHAPES[:2]:
        G, R, x = cr(Dlo, Dl, 5), cr(Dr, Dro, 5), cr(Dl, 2, Dr)
        y = be.download_c(be.dAC_proj(H, _slabs_c(be, G), _slabs_c(be, R), be.upload_c(x)))
        assert y.shape == (Dlo, 2, Dro)
        e = relerr(y, ref_dAC(G, R, x, O))
        print("dAC_proj c128", (Dlo, Dl, Dr, Dro), e)
        assert e < RTOL * max(Dlo, Dl, Dr, Dro)


def test_dac_proj_square_is_dac_bitwise(be, monkeypatch):
    rng = np.random.default_rng(SEED)
    Dlo, Dl, Dr = 24, 40, 56
    Od = rng.random((4, 4, 4, 4))
    for route, mkH in (("sparse", lambda: mk.heisenberg_XXX(0.5, be=be)[0]), ("1", lambda: be.mposlice_dense(Od)),
                       ("0", lambda: be.mposlice_dense(Od))):
        if route != "sparse":
            monkeypatch.setenv("MPSK_DENSE_ROUTE", route)
        H = mkH()
        G, R, x = (_slabs(be, rng.random((Dlo, Dl, H.Wl))), _slabs(be, rng.random((Dr, Dr, H.Wr))),
                   be.upload(rng.random((Dl, H.d, Dr))))
        a, b = be.dAC(H, G, R, x), be.dAC_proj(H, G, R, x)
        assert torch.equal(a.buf[:a.size], b.buf[:b.size]), route
    Hc = _cplx_heisenberg(be, rng)
    cr = lambda *s: rng.random(s) + 1j * rng.random(s)
    G, R, x = _slabs_c(be, cr(Dlo, Dl, 5)), _slabs_c(be, cr(Dr, Dr, 5)), be.upload_c(cr(Dl, 2, Dr))
    a, b = be.dAC(Hc, G, R, x), be.dAC_proj(Hc, G, R, x)
    assert torch.equal(a.buf[:a.size], b.buf[:b.size])


# ---- mpsk_dAC2_proj --------------------------------------------------------------------------------------------------

PROJ2_SHAPES = [(3, 5, 4, 7, 2), (24, 40, 36, 56, 20), (72, 136, 100, 130, 40)]


@pytest.mark.parametrize("model", ["hubbard", "heisenberg", "dense"])
def test_dac2_proj_f64(be, monkeypatch, model):
    monkeypatch.delenv("MPSK_DENSE_ROUTE", raising=False)
    rng = np.random.default_rng(SEED)
    if model == "dense":
        O1, O2 = rng.random((4, 4, 4, 4)), rng.random((4, 4, 4, 4))
        H1, H2 = be.mposlice_dense(O1), be.mposlice_dense(O2)
    else:
        H1 = H2 = (mk.hubbard(be=be) if model == "hubbard" else mk.heisenberg_XXX(0.5, be=be))[0]
        O1 = O2 = full_O(H1)
        assert (H1.d, H1.Wl) == ((4, 6) if model == "hubbard" else (2, 5))
    d = H1.d
    for Dlo, Dl, Dm, Dr, Dro in PROJ2_SHAPES:
        G, R = rng.random((Dlo, Dl, H1.Wl)), rng.random((Dr, Dro, H2.Wr))
        AC, AR = rng.random((Dl, d, Dm)), rng.random((Dm, d, Dr))
        y = be.download(be.dAC2_proj(H1, H2, _slabs(be, G), _slabs(be, R), be.upload(AC), be.upload(AR)))
        assert y.shape == (Dlo, d, Dro, d)
        e = relerr(y, ref_dAC2(G, R, np.einsum("axm,mzb->axbz", AC, AR), O1, O2))
        print("dAC2_proj", model, (Dlo, Dl, Dm, Dr, Dro), e)
        assert e < RTOL * max(Dlo, Dl, Dm, Dr, Dro), (model, Dlo, Dl, Dm, Dr, Dro, e)


def test_dac2_proj_square_matches_product(be):
    rng = np.random.default_rng(SEED)
    H = mk.hubbard(be=be)[0]
    Dl, Dm, Dr = 24, 36, 56
    G, R = _slabs(be, rng.random((Dl, Dl, 6))), _slabs(be, rng.random((Dr, Dr, 6)))
    AC, AR = be.upload(rng.random((Dl, 4, Dm))), be.upload(rng.random((Dm, 4, Dr)))
    a, b = be.download(be.dAC2_product(H, H, G, R, AC, AR)), be.download(be.dAC2_proj(H, H, G, R, AC, AR))
    assert relerr(b, a) < RTOL * max(Dl, Dm, Dr)


def test_dac2_proj_c128(be):
    rng = np.random.default_rng(SEED)
    H = _cplx_heisenberg(be, rng)
    O = full_O(H)
    cr = lambda *s: rng.random(s) + 1j * rng.random(s)
    for Dlo, Dl, Dm, Dr, Dro in PROJ2_SHAPES[:2]:
        G, R, AC, AR = cr(Dlo, Dl, 5), cr(Dr, Dro, 5), cr(Dl, 2, Dm), cr(Dm, 2, Dr)
        y = be.download_c(be.dAC2_proj(H, H, _slabs_c(be, G), _slabs_c(be, R), be.upload_c(AC), be.upload_c(AR)))
        assert y.shape == (Dlo, 2, Dro, 2)
        e = relerr(y, ref_dAC2(G, R, np.einsum("axm,mzb->axbz", AC, AR), O, O))
        print("dAC2_proj c128", (Dlo, Dl, Dm, Dr, Dro), e)
        assert e < RTOL * max(Dlo, Dl, Dm, Dr, Dro)


# ---- mpsk_vdiff_nrm2 -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_vdiff_nrm2(be, cplx):
    rng = np.random.default_rng(SEED)
    for n in (1, 63, 64, 65, 4097, 1 << 20):
        m = 2 * n if cplx else n
        x, y = rng.random(m), rng.random(m)
        dx, dy = be.upload(x), be.upload(y)
        out = (C.c_double * 2)()
        be._set_dtype(cplx)
        try:
            mk._lib.check(be.lib.mpsk_vdiff_nrm2(be.ctx, n, dx.ptr, dy.ptr, out), "mpsk_vdiff_nrm2")
            assert abs(out[0] - np.sum((x - y) ** 2)) <= 1e-13 * np.sum((x - y) ** 2), (n, out[0])
            assert abs(out[1] - np.sum(x * x)) <= 1e-13 * np.sum(x * x), (n, out[1])
            mk._lib.check(be.lib.mpsk_vdiff_nrm2(be.ctx, n, dx.ptr, dx.ptr, out), "mpsk_vdiff_nrm2")
            assert out[0] == 0.0
        finally:
            be._set_dtype(False)
    d2, n2 = be.vdiff_nrm2(dx, dy)
    assert abs(d2 - np.sum((x - y) ** 2)) <= 1e-13 * d2 and abs(n2 - np.sum(x * x)) <= 1e-13 * n2


# ---- argument checks -------------------------------------------------------------------------------------------------

def test_argument_checks(be):
    lib, ctx = be.lib, be.ctx
    H5, H6 = mk.heisenberg_XXX(0.5, be=be)[0], mk.hubbard(be=be)[0]
    t = be.zeros(4096)
    p = t.ptr

    def invalid(rc):
        assert rc == 1 and len(lib.mpsk_last_error()) > 0, (rc, lib.mpsk_last_error())
    invalid(lib.mpsk_dAC_proj(ctx, H5.handle, 2, 2, 2, 0, p, p, p, p))
    invalid(lib.mpsk_dAC_proj(ctx, H5.handle, 2, 2, 2, -3, p, p, p, p))
    invalid(lib.mpsk_dAC_proj(ctx, H5.handle, 2, 2, 2, 2, None, p, p, p))
    invalid(lib.mpsk_dAC_proj(ctx, None, 2, 2, 2, 2, p, p, p, p))
    invalid(lib.mpsk_dAC2_proj(ctx, H5.handle, H5.handle, 2, 2, 2, 2, 0, p, p, p, p, p))
    invalid(lib.mpsk_dAC2_proj(ctx, H5.handle, H6.handle, 2, 2, 2, 2, 2, p, p, p, p, p))      # H1->Wr != H2->Wl
    invalid(lib.mpsk_dAC2_proj(ctx, H5.handle, H5.handle, 2, 2, 2, 2, 2, p, p, p, None, p))
    out = (C.c_double * 2)()
    invalid(lib.mpsk_vdiff_nrm2(ctx, 0, p, p, out))
    invalid(lib.mpsk_vdiff_nrm2(ctx, 8, None, p, out))
    invalid(lib.mpsk_vdiff_nrm2(ctx, 8, p, p, None))
    be.synchronize()


# ---- approximate on the device ---------------------------------------------------------------------------------------

class Composed:
    """The backend with the three new entry points hidden, so that approximate takes its composed route; dAC / dAC2 with
    rectangular environments are restated in NumPy here (Backend.dAC / dAC2 are the square Krylov matvecs)."""

    def __init__(self, be):
        self._be = be

    def __getattr__(self, name):
        if name in ("dAC_proj", "dAC2_proj", "vdiff_nrm2"):
            raise AttributeError(name)
        return getattr(self._be, name)

    def _env(self, t):
        W, D1, D2 = t.shape
        return self._be.download(t.reshape(D1, D2, W))

    def dAC(self, H, GL, GR, x, out=None):
        y = ref_dAC(self._env(GL), self._env(GR), self._be.download(x), full_O(H))
        return self._be.upload(y)

    def dAC2(self, H1, H2, GL, GR, x2, out=None):
        y = ref_dAC2(self._env(GL), self._env(GR), self._be.download(x2), full_O(H1), full_O(H2))
        return self._be.upload(y)


def test_state_to_state_and_routes(be):
    dev = ac.case_state_to_state(be)
    comp = ac.case_state_to_state(Composed(be))
    for a, b in zip(dev, comp):
        assert np.linalg.norm(a - b) <= 1e-10 * np.linalg.norm(a)


def test_mpo_exact_and_routes(be):
    dev = ac.case_mpo_exact(be)
    comp = ac.case_mpo_exact(Composed(be))
    for a, b in zip(dev, comp):
        assert np.linalg.norm(a - b) <= 1e-10 * np.linalg.norm(a)


def test_mpo_truncating(be):
    ac.case_truncating(be)


def test_list_of_targets(be):
    ac.case_list(be)


# ---- complex states / real time: native_cplx.approximate -------------------------------------------------------------

def _native_random(be, D, rng):
    dims = mk.FiniteMPS.random(ac.L, ac.d, D, np.random.default_rng(0), be=be).bond_dims()
    dims = [1] + list(dims)
    return nc.NativeFiniteMPS([rng.random((dims[i], ac.d, dims[i + 1])) + 1j * rng.random((dims[i], ac.d, dims[i + 1]))
                               for i in range(ac.L)], be)


def _native_vec(psi):
    v = np.ones((1, 1), dtype=complex)
    for T in psi.to_host():
        v = np.tensordot(v, T, axes=([v.ndim - 1], [0]))
    return v.reshape(-1)


@pytest.mark.parametrize("alg", ["DMRG", "DMRG2"])
def test_complex_time_mpo_exact(be, alg):
    """O = W^II of TFI at real dt = 0.05 (complex), above complex with D = 8, target D = 16: exactly representable"""
    rng = np.random.default_rng(8)
    O = mk.make_time_mpo(mk.transverse_field_ising(1.0, 0.7, be=be), 0.05, mk.WII())
    assert O.cplx
    above, psi0 = _native_random(be, 8, rng), _native_random(be, 16, rng)
    t = ac.sparse_dense(O, ac.L, 0, dtype=complex) @ _native_vec(above)
    a = mk.DMRG(tol=1e-12, maxiter=10) if alg == "DMRG" else mk.DMRG2(tol=1e-12, maxiter=10, trunc_dim=16)
    psi, envs, eps = nc.approximate(psi0, (O, above), a)
    err = np.linalg.norm(t - _native_vec(psi)) / np.linalg.norm(t)
    print(alg, "complex MPO.MPS: err", err, "eps", eps, envs.history)
    assert err <= 1e-10, (alg, err)


@pytest.mark.parametrize("alg", ["DMRG", "DMRG2"])
def test_wi_step_against_tdvp(be, alg):
    """the reference's own acceptance test (test/algorithms.jl:487-499): one approximate step with WI at tau = 1e-3 against
    one TDVP step; |<psi2, psi2'>| agrees with <psi1, psi1> = 1 to atol = 1e-3 after normalisation"""
    rng = np.random.default_rng(9)
    H = mk.transverse_field_ising(1.0, 4.0, be=be)
    tau = 1e-3
    psi1, psi2 = _native_random(be, 8, rng), _native_random(be, 16, rng)
    O = mk.make_time_mpo(H, tau, mk.WI())
    a = mk.DMRG(tol=1e-12, maxiter=10) if alg == "DMRG" else mk.DMRG2(tol=1e-12, maxiter=10, trunc_dim=16)
    phi, _, _ = nc.approximate(psi2, (O, psi1), a)
    v = _native_vec(phi)
    v /= np.linalg.norm(v)
    ref, _ = nc.timestep(psi1.copy(), H, 0.0, tau, mk.TDVP())
    w = _native_vec(ref)
    n1 = np.linalg.norm(_native_vec(psi1)) ** 2
    print(alg, "WI vs TDVP: overlap", abs(np.vdot(v, w)), "norm", n1)
    assert abs(n1 - abs(np.vdot(v, w))) <= 1e-3
