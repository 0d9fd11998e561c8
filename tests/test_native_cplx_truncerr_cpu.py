"""Host logic of the truncerr scheme of the interleaved-storage two-site drivers (native_cplx.dmrg2_sweep / tdvp2_step behind
find_groundstate / timestep) on the complex CPU stand-in: DMRG2() and TDVP2() with the reference defaults (truncerr(1e-6),
truncerr(1e-3): dmrg.jl:75, tdvp.jl:111) split through tsplit_c(trunc_err=...) and follow the oracle; with trunc_dim set the
split is called exactly as before (max_keep only)."""
import numpy as np

import mpskit_oracle as mo
from cpu_backend import CpuComplexBackend


class TruncerrBackend(CpuComplexBackend):
    """CpuComplexBackend + tsvd_c and tsplit_c(trunc_err=...) by NumPy's complex SVD (the oracle's truncation rule); records
    the keyword arguments of every split."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.split_kwargs = []

    @staticmethod
    def _cut(S, max_keep, trunc_err):
        k = len(S) if not max_keep else min(len(S), int(max_keep))
        if trunc_err > 0.0:
            while k > 1 and np.linalg.norm(S[k - 1:]) <= trunc_err:
                k -= 1
        return k

    def tsvd_c(self, theta, max_keep=0, trunc_err=0.0):
        U, S, Vh = np.linalg.svd(self.download_c(theta), full_matrices=False)
        k = self._cut(S, max_keep, trunc_err)
        return (self.upload_c(U), self.upload(S), self.upload_c(Vh), k, float(np.linalg.norm(S[k:])))

    def tsplit_c(self, theta, max_keep=0, **kw):
        self.split_kwargs.append(dict(kw))
        trunc_err = kw.get("trunc_err", 0.0)
        if not trunc_err:
            return super().tsplit_c(theta, max_keep=max_keep)
        self._count("tsplit_c")
        U, S, Vh = np.linalg.svd(self.download_c(theta), full_matrices=False)
        k = self._cut(S, max_keep, trunc_err)
        return (self.upload_c(U[:, :k]), self.upload_c(np.diag(S[:k]).astype(complex)), self.upload_c(Vh[:k, :]), S[:k].copy(),
                float(np.linalg.norm(S[k:])))


def _setup(seed, D0):
    import mpskit_jl_amd as mk
    from mpskit_jl_amd import native_cplx as nc
    cb = TruncerrBackend()
    rng = np.random.default_rng(seed)
    L, d = 6, 2
    dims = mo.FiniteMPS.random(L, d, D0, np.random.default_rng(0)).bond_dims()
    As = [rng.standard_normal((1 if i == 0 else dims[i - 1], d, dims[i])) + 1j * rng.standard_normal((1 if i == 0 else dims[i - 1], d, dims[i]))
          for i in range(L)]
    X = np.array([[0, 1], [1, 0]], dtype=complex); Y = np.array([[0, -1j], [1j, 0]]); Z = np.array([[1, 0], [0, -1]], dtype=complex)
    H = nc.ComplexMPOHamiltonian({(0, 0): 1.0, (4, 4): 1.0, (0, 1): X, (1, 4): X, (0, 2): Y, (2, 4): Y, (0, 3): Z, (3, 4): Z}, cb)
    return mk, nc, cb, As, H, mo.heisenberg_pauli_mpo(), L


def test_dmrg2_default_takes_the_truncerr_scheme():
    mk, nc, cb, As, H, Ho, L = _setup(5, 2)
    eig = mk.Arnoldi(tol=1e-12, krylovdim=16, maxiter=40)
    psi = nc.NativeFiniteMPS(As, cb)
    po = mo.FiniteMPS(As, normalize=True)
    envs = None
    for sweep in range(2):
        psi, envs, _ = nc.find_groundstate(psi, H, mk.DMRG2(tol=1e-10, maxiter=1, eigalg=eig), envs)
        po, _, _, log = mo.dmrg2(po, Ho, truncerr=1e-6, maxiter=1, eig_tol=1e-12, krylovdim=16, eig_maxiter=40)
        E = nc.energy(psi, envs)
        assert abs(E - log[-1][1]) < 1e-9 * abs(E), (sweep, E, log[-1][1])
        assert [psi.dims(i)[2] for i in range(L)] == po.bond_dims()
    assert cb.split_kwargs and all(kw == {"trunc_err": 1e-6} for kw in cb.split_kwargs)


def test_dmrg2_truncdim_calls_the_split_as_before():
    mk, nc, cb, As, H, Ho, L = _setup(5, 2)
    eig = mk.Arnoldi(tol=1e-12, krylovdim=16, maxiter=40)
    psi = nc.NativeFiniteMPS(As, cb)
    nc.find_groundstate(psi, H, mk.DMRG2(tol=1e-10, maxiter=1, trunc_dim=8, eigalg=eig))
    # trunc_dim > 0 wins over the default trunc_err, as in the real host
    nc.find_groundstate(psi, H, mk.DMRG2(tol=1e-10, maxiter=1, trunc_dim=8, trunc_err=1e-3, eigalg=eig))
    assert cb.split_kwargs and all(kw == {} for kw in cb.split_kwargs)
    cb.split_kwargs.clear()
    envs = nc.NativeFinEnv(psi, H)
    nc.dmrg2_sweep(psi, H, envs, eig, trunc_dim=8)
    assert cb.split_kwargs and all(kw == {} for kw in cb.split_kwargs)


def test_tdvp2_default_takes_the_truncerr_scheme():
    mk, nc, cb, As, H, Ho, L = _setup(7, 4)
    psi = nc.NativeFiniteMPS(As, cb)
    psi, envs = nc.timestep(psi, H, 0.0, 0.05, mk.TDVP2(tol=1e-12, krylovdim=16))
    po2, _ = mo.tdvp2_timestep(mo.FiniteMPS(As, normalize=True), Ho, 0.0, 0.05, truncerr=1e-3, tol=1e-12, krylovdim=16)
    vo = mo.mps_to_vector(po2)
    vn = psi.to_host()[0]
    for t in psi.to_host()[1:]:
        vn = np.tensordot(vn, t, axes=([-1], [0]))
    vn = vn.reshape(-1)
    assert abs(abs(np.vdot(vo, vn)) / (np.linalg.norm(vo) * np.linalg.norm(vn)) - 1.0) < 1e-9
    assert [psi.dims(i)[2] for i in range(L)] == po2.bond_dims()
    assert cb.split_kwargs and all(kw == {"trunc_err": 1e-3} for kw in cb.split_kwargs)
    cb.split_kwargs.clear()
    psi = nc.NativeFiniteMPS(As, cb)
    nc.timestep(psi, H, 0.0, 0.05, mk.TDVP2(tol=1e-12, krylovdim=16, trunc_dim=4))
    assert cb.split_kwargs and all(kw == {} for kw in cb.split_kwargs)


def test_stand_in_tsvd_c_matches_the_oracle_truncation():
    cb = TruncerrBackend()
    rng = np.random.default_rng(3)
    a = rng.standard_normal((30, 20)) + 1j * rng.standard_normal((30, 20))
    s = np.linalg.svd(a, compute_uv=False)
    for eps in (1e-3, 1.0, 5.0):
        _, _, _, k, disc = cb.tsvd_c(cb.upload_c(a), trunc_err=eps)
        _, So, _, erro = mo.tsvd(a.reshape(30, 1, 20, 1), truncerr=eps)
        assert k == len(So) and abs(disc - erro) < 1e-12 * s[0]
