"""Native complex128 truncated SVD (mpsk_tsvd under MPSK_C128: complex one-sided block Jacobi) and the truncerr scheme of the
complex two-site split (mpsk_tsplit under MPSK_C128, trunc_err > 0), against NumPy's complex SVD and the oracle; the
interleaved-storage DMRG2 / TDVP2 drivers on the reference defaults truncerr(1e-6) / truncerr(1e-3) (dmrg.jl:75,
tdvp.jl:111)."""
import numpy as np
import pytest

import mpskit_oracle as mo

pytestmark = pytest.mark.gpu


def crand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def unitary(rng, n, k):
    q, r = np.linalg.qr(crand(rng, n, k))
    return q * (np.diag(r) / np.abs(np.diag(r)))


def graded(rng, m, n, s):
    k = len(s)
    return (unitary(rng, m, k) * s) @ unitary(rng, n, k).conj().T


def csvd(be, a, max_keep=0, trunc_err=0.0):
    U, S, Vh, k, disc = be.tsvd_c(be.upload_c(a), max_keep=max_keep, trunc_err=trunc_err)
    return be.download_c(U), be.download(S), be.download_c(Vh), k, disc


@pytest.mark.parametrize("m,n,kind", [(20, 16, "rand"), (64, 64, "rand"), (96, 80, "rand"), (80, 96, "rand"), (192, 160, "rand"),
                                      (200, 136, "rand"), (512, 384, "rand"), (1024, 1024, "graded")])
def test_complex_tsvd_full(be, m, n, kind):
    rng = np.random.default_rng(m * 7 + n)
    if kind == "graded":
        a = graded(rng, m, n, np.logspace(0, -12, min(m, n)))
    else:
        a = crand(rng, m, n)
    s = np.linalg.svd(a, compute_uv=False)
    U, S, Vh, k, disc = csvd(be, a)
    kmax = min(m, n)
    assert k == kmax and disc == 0.0
    assert U.shape == (m, kmax) and Vh.shape == (kmax, n)
    assert np.abs(U.conj().T @ U - np.eye(kmax)).max() < 1e-12
    assert np.abs(Vh @ Vh.conj().T - np.eye(kmax)).max() < 1e-12
    assert np.linalg.norm((U * S) @ Vh - a) <= 1e-12 * np.linalg.norm(a)
    assert np.abs(S - s).max() <= 1e-12 * s[0]
    assert np.all(np.diff(S) <= 0.0)


@pytest.mark.parametrize("m,n", [(48, 40), (160, 96), (96, 160)])
def test_complex_tsvd_of_real_input_gives_the_fp64_values(be, m, n):
    rng = np.random.default_rng(11 + m)
    a = rng.standard_normal((m, n))
    _, Sr, _, _, _ = be.tsvd(be.upload(a))
    Sr = be.download(Sr)
    _, S, _, _, _ = csvd(be, a.astype(complex))
    assert np.abs(S - Sr).max() <= 1e-13 * Sr[0]


def test_complex_tsvd_truncation(be):
    rng = np.random.default_rng(23)
    m, n = 150, 110
    a = graded(rng, m, n, np.logspace(0, -8, n))
    s = np.linalg.svd(a, compute_uv=False)
    cases = [dict(max_keep=40), dict(trunc_err=1e-5), dict(max_keep=40, trunc_err=1e-5), dict(max_keep=90, trunc_err=1e-5)]
    for kw in cases:
        U, S, Vh, k, disc = csvd(be, a, **kw)
        _, So, _, erro = mo.tsvd(a.reshape(m, 1, n, 1), truncdim=kw.get("max_keep"), truncerr=kw.get("trunc_err"))
        assert k == len(So), (kw, k, len(So))
        assert abs(disc - erro) < 1e-13, kw
        assert np.abs(S - s).max() <= 1e-12 * s[0]
    # truncerr is ABSOLUTE (TensorKit 0.12), not scale invariant: the test_gpu_ops.py tsvd scale check, on complex data
    eps = 1e-6
    for scale in (1.0, 3.7e3):
        _, _, _, k2, disc2 = csvd(be, scale * a, trunc_err=eps)
        _, So, _, erro = mo.tsvd((scale * a).reshape(m, 1, n, 1), truncerr=eps)
        assert k2 == len(So) == int(np.sum(np.sqrt(np.cumsum((scale * s[::-1]) ** 2))[::-1] > eps))
        assert abs(disc2 - erro) < 1e-13 * scale
    import mpskit_jl_amd as mk
    with pytest.raises(mk.MpskError):
        be.tsvd_c(be.upload_c(a), trunc_err=-1.0)


def test_complex_tsvd_workspace_plan_on_a_fresh_ctx():
    """small call, then large ones (tall and wide) on a fresh ctx: the single workspace plan of the call must cover the
    preconditioning QR and the Jacobi (run once)"""
    import mpskit_jl_amd as mk
    b = mk.Backend(0)
    try:
        rng = np.random.default_rng(31)
        for m, n in [(20, 16), (640, 384), (384, 704)]:
            a = crand(rng, m, n)
            U, S, Vh, k, _ = csvd(b, a)
            assert k == min(m, n)
            assert np.linalg.norm((U * S) @ Vh - a) <= 1e-12 * np.linalg.norm(a)
            assert np.abs(U.conj().T @ U - np.eye(k)).max() < 1e-12
            assert np.abs(Vh @ Vh.conj().T - np.eye(k)).max() < 1e-12
    finally:
        b.close()


@pytest.mark.parametrize("m,n,k0", [(192, 160, 50), (160, 192, 50), (512, 512, 120), (40, 24, 10)])
def test_complex_tsplit_truncerr(be, m, n, k0):
    rng = np.random.default_rng(m + 3 * n)
    kf = min(m, n)
    s = np.concatenate([np.logspace(0, -3, k0), np.logspace(-8, -10, kf - k0)])   # cut in the gap: eps = 1e-5
    a = graded(rng, m, n, s)
    eps = 1e-5
    _, So, _, erro = mo.tsvd(a.reshape(m, 1, n, 1), truncerr=eps)
    th = be.upload_c(a)
    al, c, ar, S, disc = be.tsplit_c(th, trunc_err=eps)
    k = c.shape[1]
    assert k == len(So) == k0
    al, c, ar = be.download_c(al), be.download_c(c), be.download_c(ar)
    assert np.abs(al.conj().T @ al - np.eye(k)).max() < 1e-12
    assert np.abs(ar @ ar.conj().T - np.eye(k)).max() < 1e-12
    assert np.abs(np.triu(c, 1)).max() == 0.0
    assert np.all(np.diag(c).real > 0.0) and np.abs(np.diag(c).imag).max() == 0.0
    res = np.linalg.norm(a - al @ c @ ar)
    assert abs(res - erro) <= 1e-12 * s[0]
    assert abs(disc - erro) <= 1e-13
    assert np.abs(S[:k] - So).max() <= 1e-12 * s[0]
    # max_keep below the truncerr count wins
    _, c2, _, _, _ = be.tsplit_c(th, max_keep=k0 // 2, trunc_err=eps)
    assert c2.shape[1] == k0 // 2
    # trunc_err = 0 is the truncdim path, unchanged (two calls of it agree to rounding, not bitwise: the ctx keeps the
    # subspace-iteration count of the last split of a shape as the next one's start)
    r1 = be.tsplit_c(th, max_keep=k0)
    r2 = be.tsplit_c(th, max_keep=k0, trunc_err=0.0)
    p1, p2 = [be.download_c(r[0]) @ be.download_c(r[1]) @ be.download_c(r[2]) for r in (r1, r2)]
    assert r1[1].shape == r2[1].shape == (2 * k0, k0)
    assert np.linalg.norm(p1 - p2) <= 1e-12 * np.linalg.norm(a)
    # (the truncdim path's discarded norm is sqrt(|theta|^2 - |M|^2): rounding noise of ~sqrt(eps) |theta| for small tails)
    assert np.abs(r1[3] - r2[3]).max() <= 1e-13 and abs(r1[4] - r2[4]) <= 1e-7 * np.linalg.norm(a)


def _heisenberg_start(be, seed, D0):
    import mpskit_jl_amd as mk
    rng = np.random.default_rng(seed)
    L, d = 8, 2
    dims = mo.FiniteMPS.random(L, d, D0, np.random.default_rng(0)).bond_dims()
    As = [crand(rng, 1 if i == 0 else dims[i - 1], d, dims[i]) for i in range(L)]
    return mk, As, mk.heisenberg_XXX(0.5, be=be), mo.heisenberg_mpo(0.5), L


def test_native_dmrg2_on_the_reference_default(be):
    """DMRG2() without trunc_dim = truncerr(1e-6): follows mo.dmrg2(truncerr=1e-6) sweep by sweep with the same bond
    dimensions and reaches the ED energy.  Seed 8: no singular value of the oracle run lies within 1e-10 of the threshold."""
    from mpskit_jl_amd import native_cplx as nc
    mk, As, H, Ho, L = _heisenberg_start(be, 8, 4)
    eig = mk.Arnoldi(tol=1e-12, krylovdim=20, maxiter=50)
    psi = nc.NativeFiniteMPS(As, be)
    po = mo.FiniteMPS(As, normalize=True)
    envs = None
    for sweep in range(4):
        psi, envs, _ = nc.find_groundstate(psi, H, mk.DMRG2(tol=1e-10, maxiter=1, eigalg=eig), envs)
        po, _, _, log = mo.dmrg2(po, Ho, truncerr=1e-6, maxiter=1, eig_tol=1e-12, krylovdim=20, eig_maxiter=50)
        E = nc.energy(psi, envs)
        assert abs(E - log[-1][1]) < 1e-9 * abs(E), (sweep, E, log[-1][1])
        assert [psi.dims(i)[2] for i in range(L)] == po.bond_dims()
    E0 = np.linalg.eigvalsh(mo.dense_hamiltonian(Ho, L))[0]
    assert abs(E - E0) < 1e-8 * abs(E0)
    psi2, envs2, dE = nc.find_groundstate(nc.NativeFiniteMPS(As, be), H, mk.DMRG2(tol=1e-10, maxiter=4, eigalg=eig))
    assert abs(nc.energy(psi2, envs2) - E0) < 1e-8 * abs(E0)


def test_native_tdvp2_on_the_reference_default(be):
    """TDVP2() without trunc_dim = truncerr(1e-3): the same state as mo.tdvp2_timestep(truncerr=1e-3) (overlap 1 - 1e-9),
    same bond dimensions.  Seed 12: no singular value of the oracle run lies within 1e-10 of the threshold."""
    from mpskit_jl_amd import native_cplx as nc
    mk, As, H, Ho, L = _heisenberg_start(be, 12, 4)
    psi = nc.NativeFiniteMPS(As, be)
    psi, envs = nc.timestep(psi, H, 0.0, 0.05, mk.TDVP2(tol=1e-12, krylovdim=20))
    po2, _ = mo.tdvp2_timestep(mo.FiniteMPS(As, normalize=True), Ho, 0.0, 0.05, truncerr=1e-3, tol=1e-12, krylovdim=20)
    vo = mo.mps_to_vector(po2)
    ts = psi.to_host()
    vn = ts[0]
    for t in ts[1:]:
        vn = np.tensordot(vn, t, axes=([-1], [0]))
    vn = vn.reshape(-1)
    assert abs(np.vdot(vo, vn)) / (np.linalg.norm(vo) * np.linalg.norm(vn)) >= 1.0 - 1e-9
    assert [psi.dims(i)[2] for i in range(L)] == po2.bond_dims()
