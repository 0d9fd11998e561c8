"""approximate / make_time_mpo / the two-state environments on the NumPy stand-in backend (tests/cpu_backend.py): host
logic only, no GPU.  The stand-in has no dAC_proj / dAC2_proj / vdiff_nrm2, so every sweep here takes the composed route.
The NumPy restatements (dense vectors / matrices built from downloaded tensors) and the bodies of the approximate cases live
here; tests/test_gpu_approximate.py runs the same cases on the device.  L = 8, d = 2: the largest possible bond is 16, so the
"exact" cases are exactly representable."""
import numpy as np
import pytest
from scipy.linalg import expm

import mpskit_jl_amd as mk
from cpu_backend import CpuBackend



L, d = 8, 2
X = np.array([[0.0, 1.0], [1.0, 0.0]])
Z = np.diag([1.0, -1.0])


def vec(psi):
    """the dense 2^L vector of a FiniteMPS"""
    v = np.ones((1, 1))
    for T in psi.to_host():
        v = np.tensordot(v, T, axes=([v.ndim - 1], [0]))
    return v.reshape(-1)


def sparse_dense(O, n, right, dtype=float):
    """dense matrix of n sites of a block-sparse MPO (MPOHamiltonian / SparseMPO): left boundary level 0, right `right`"""
    data = O.data if hasattr(O, "data") else [sl.blocks for sl in O.slices]
    dd = O.d
    cur = [None] * O.odim
    cur[0] = np.eye(1, dtype=dtype)
    for s in range(n):
        new = [None] * O.odim
        for (i, j), b in data[s % len(data)].items():
            if cur[i] is None:
                continue
            m = b * np.eye(dd) if np.isscalar(b) else np.asarray(b)[0, :, :, 0]
            t = np.kron(cur[i], m)
            new[j] = t if new[j] is None else new[j] + t
        cur = new
    return cur[right]


def list_dense(ts):
    """dense matrix of a finite dense MPO (list of [Wl, d, d, Wr], edges 1)"""
    cur = np.ones((1, 1, 1))
    for t in ts:
        cur = np.einsum("wab,wtsv->vatbs", cur, t).reshape(t.shape[3], cur.shape[1] * t.shape[1], cur.shape[2] * t.shape[2])
    return cur[0]


def tfi_dense(n, g):
    def kron(ops):
        o = np.eye(1)
        for a in ops:
            o = np.kron(o, a)
        return o
    I2 = np.eye(2)
    H = sum(-kron([Z if k in (i, i + 1) else I2 for k in range(n)]) for i in range(n - 1))
    return H + sum(-g * kron([X if k == i else I2 for k in range(n)]) for i in range(n))


def svd_truncate(v, D):
    """sequential-SVD truncation of a dense 2^L vector to bond dimension D: host tensors [Dl, d, Dr]"""
    As, rest, Dl = [], v.reshape(1, -1), 1
    for _ in range(L - 1):
        U, S, Vh = np.linalg.svd(rest.reshape(Dl * d, -1), full_matrices=False)
        k = min(D, len(S))
        As.append(U[:, :k].reshape(Dl, d, k))
        rest, Dl = S[:k, None] * Vh[:k], k
    As.append(rest.reshape(Dl, d, 1))
    return As


def algs():
    return [mk.DMRG(tol=1e-12, maxiter=10), mk.DMRG2(tol=1e-12, maxiter=10, trunc_dim=16)]


def operators(be, rng):
    """(name, O, dense matrix) of case 2: W^II of TFI at dt = -0.05i (real), a random finite dense MPO with W = 3, Heisenberg"""
    O = mk.make_time_mpo(mk.transverse_field_ising(1.0, 0.7, be=be), -0.05j, mk.WII())
    assert not O.cplx
    W = 3
    dm = [rng.random((1 if i == 0 else W, d, d, 1 if i == L - 1 else W)) for i in range(L)]
    Hh = mk.heisenberg_XXX(be=be)
    return [("WII", O, sparse_dense(O, L, 0)), ("dense", dm, list_dense(dm)), ("H", Hh, sparse_dense(Hh, L, Hh.odim - 1))]


def case_state_to_state(be):
    rng = np.random.default_rng(1)
    above = mk.FiniteMPS.random(L, d, 16, rng, be=be)
    psi0 = mk.FiniteMPS.random(L, d, 16, rng, be=be)
    a = vec(above)
    out = []
    for alg in algs():
        psi, envs, eps = mk.approximate(psi0, above, alg)
        b = vec(psi)
        infid = 1 - abs(a @ b) / (np.linalg.norm(a) * np.linalg.norm(b))
        print(type(alg).__name__, "state->state: infidelity", infid, "eps", eps)
        assert infid <= 1e-10 and eps < alg.tol, (type(alg).__name__, infid, eps)
        out.append(b)
    return out


def case_mpo_exact(be):
    rng = np.random.default_rng(2)
    above = mk.FiniteMPS.random(L, d, 8, rng, be=be)
    psi0 = mk.FiniteMPS.random(L, d, 16, rng, be=be)
    a = vec(above)
    out = []
    for name, O, Od in operators(be, rng):
        t = Od @ a
        for alg in algs():
            psi, envs, eps = mk.approximate(psi0, (O, above), alg)
            b = vec(psi)
            err = np.linalg.norm(t - b) / np.linalg.norm(t)
            print(name, type(alg).__name__, "MPO.MPS exact: err", err, "eps", eps)
            assert err <= 1e-10, (name, type(alg).__name__, err)
            out.append(b)
    return out


def case_truncating(be):
    rng = np.random.default_rng(3)
    above = mk.FiniteMPS.random(L, d, 8, rng, be=be)
    O = mk.make_time_mpo(mk.transverse_field_ising(1.0, 0.7, be=be), -0.05j, mk.WII())
    t = sparse_dense(O, L, 0) @ vec(above)
    psi0 = mk.FiniteMPS(svd_truncate(t, 6), be=be)
    err0 = np.linalg.norm(t - vec(psi0))
    assert err0 > 1e-8 * np.linalg.norm(t)          # the case truncates
    for alg in [mk.DMRG(tol=1e-12, maxiter=6), mk.DMRG2(tol=1e-12, maxiter=6, trunc_dim=6)]:
        psi, envs, eps = mk.approximate(psi0, (O, above), alg)
        err1 = np.linalg.norm(t - vec(psi))
        hist = [e for _, e in envs.history]
        print(type(alg).__name__, "truncating: err_start", err0, "err_after", err1, "eps history", hist)
        assert max(psi.bond_dims()) <= 6
        assert err1 <= err0 * (1 + 1e-8), (type(alg).__name__, err0, err1)
        assert all(hist[i + 1] <= hist[i] * (1 + 1e-8) + 1e-15 for i in range(len(hist) - 1)), hist


def case_list(be):
    rng = np.random.default_rng(4)
    above = mk.FiniteMPS.random(L, d, 8, rng, be=be)
    psi0 = mk.FiniteMPS.random(L, d, 16, rng, be=be)
    O1 = mk.make_time_mpo(mk.transverse_field_ising(1.0, 0.7, be=be), -0.05j, mk.WII())
    O2 = mk.heisenberg_XXX(be=be)
    t = (sparse_dense(O1, L, 0) + sparse_dense(O2, L, O2.odim - 1)) @ vec(above)
    psi, envs, eps = mk.approximate(psi0, [(O1, above), (O2, above)], mk.DMRG2(tol=1e-12, maxiter=10, trunc_dim=16))
    err = np.linalg.norm(t - vec(psi)) / np.linalg.norm(t)
    print("list of targets: err", err, "eps", eps)
    assert isinstance(envs, list) and len(envs) == 2
    assert err <= 1e-10, err


@pytest.fixture()
def be():
    return CpuBackend()


# ---- make_time_mpo ---------------------------------------------------------------------------------------------------

def _errors(alg, fac):
    """spectral-norm error of the L = 6 TFI evolution MPO against expm(tau H) at tau = fac * (0.02, 0.01)"""
    be = CpuBackend()
    H = mk.transverse_field_ising(1.0, 0.7, be=be)
    Hd = tfi_dense(6, 0.7)
    out = []
    for t in (0.02, 0.01):
        tau = t * fac
        O = mk.make_time_mpo(H, 1j * tau, alg)                  # tau = -i dt
        assert O.cplx == (fac != 1.0)
        out.append(np.linalg.norm(sparse_dense(O, 6, 0, dtype=complex) - expm(tau * Hd), 2))
    return out


@pytest.mark.parametrize("fac", [1.0, -1j], ids=["real_tau", "imag_tau"])
def test_wii_dense_contraction(fac):
    """issue figures (throw-away restatement): 1.1e-3, 2.6e-4 (real tau) / 1.0e-3, 2.5e-4 (imaginary); order 2.00-2.15"""
    e2, e1 = _errors(mk.WII(), fac)
    print("WII", fac, e2, e1, np.log2(e2 / e1))
    assert np.log2(e2 / e1) >= 1.8
    assert e1 <= 5e-4


@pytest.mark.parametrize("fac", [1.0, -1j], ids=["real_tau", "imag_tau"])
def test_wi_dense_contraction(fac):
    """TaylorCluster(1): a consistent first-order cluster expansion has local error O(tau^2).  Measured: 1.109e-3, 2.633e-4
    (real tau), 1.0004e-3, 2.5003e-4 (imaginary tau); no magnitude asserted beyond err(0.01) < err(0.02)."""
    e2, e1 = _errors(mk.WI(), fac)
    print("WI", fac, e2, e1, np.log2(e2 / e1))
    assert np.log2(e2 / e1) >= 1.8
    assert e1 < e2
    assert mk.WI() == mk.TaylorCluster(1)


def test_time_mpo_storage_and_levels():
    be = CpuBackend()
    for H in (mk.transverse_field_ising(1.0, 0.7, be=be), mk.heisenberg_XXX(be=be)):
        for alg in (mk.WII(), mk.WI()):
            O = mk.make_time_mpo(H, -0.05j, alg)                # tau = -0.05: imaginary-time evolution, real storage
            assert isinstance(O, mk.SparseMPO) and O.odim == H.odim - 1 and not O.cplx
            for blk in O.data:
                for v in blk.values():
                    assert not np.iscomplexobj(v)
            assert mk.make_time_mpo(H, 0.05, alg).cplx          # real time: complex storage
    with pytest.raises(NotImplementedError):
        mk.make_time_mpo(H, 0.05, mk.TaylorCluster(2))


# ---- environments ----------------------------------------------------------------------------------------------------

def test_pair_start_tensors(be):
    """FinEnv.jl:48-66, :72-81, :91-99: left level 0 everywhere; right level odim - 1 (MPOHamiltonian), 0 (SparseMPO)"""
    rng = np.random.default_rng(5)
    below = mk.FiniteMPS.random(L, d, 6, rng, be=be)
    above = mk.FiniteMPS.random(L, d, 8, rng, be=be)
    H = mk.heisenberg_XXX(be=be)
    O = mk.make_time_mpo(H, -0.05j, mk.WII())
    dm = [rng.random((1 if i == 0 else 3, 2, 2, 1 if i == L - 1 else 3)) for i in range(L)]
    for op, odim, ract in ((H, 5, 4), (O, 4, 0), (dm, 1, 0), (None, 1, 0)):
        env = mk.environments(below, above if op is None else (op, above))
        assert isinstance(env, mk.FinEnvPair) and isinstance(env, mk.FinEnv) and env.above is above
        gl, gr = be.download(env.leftenvs[0]), be.download(env.rightenvs[L])
        assert gl.shape == (odim, 1, 1) and gr.shape == (odim, 1, 1)
        assert np.array_equal(gl.reshape(-1), np.eye(odim)[0]) and np.array_equal(gr.reshape(-1), np.eye(odim)[ract])
    assert type(mk.environments(below, H)) is mk.FinEnv      # the plain environments are what they were


def test_environment_bookkeeping(be):
    """FinEnv.jl:114-145: a one-site sweep of L sites performs 2L - 2 mixed transfers per target (L - 1 left, L - 1 right).
    The first sweep builds the L - 1 right environments first, and the right transfer of site 1 that its last visit makes
    necessary is only computed when the next sweep asks for it: 3L - 4.  Writing below.AC[pos] invalidates only what depends
    on it."""
    rng = np.random.default_rng(6)
    above = mk.FiniteMPS.random(L, d, 8, rng, be=be)
    psi0 = mk.FiniteMPS.random(L, d, 8, rng, be=be)
    H = mk.heisenberg_XXX(be=be)
    counts = []

    def finalize(it, psi, squash, envs):
        counts.append([e.n_transfers for e in envs])
        return psi, envs
    psi, envs, _ = mk.approximate(psi0, [(H, above), above], mk.DMRG(tol=0.0, maxiter=3, finalize=finalize))
    n = 2 * L - 2
    assert counts[0] == [3 * L - 4] * 2
    assert [b - a for a, b in zip(counts[0], counts[1])] == [n, n] and [b - a for a, b in zip(counts[1], counts[2])] == [n, n]
    # after the sweep the centre is at site 0; a write at pos = 3 invalidates the left environments right of it only
    env = envs[0]
    env.leftenv(L - 1, psi), env.rightenv(0, psi)
    c0 = env.n_transfers
    psi.set_AC(3, be.copy(psi.AC(3)))
    env.rightenv(3, psi)
    assert env.n_transfers == c0                                   # AR[4:] are the same objects
    env.leftenv(3, psi)
    assert env.n_transfers == c0                                   # AL[:3] as well
    env.leftenv(L - 1, psi)
    assert env.n_transfers == c0 + (L - 1 - 3)                  # sites 3 .. L-2 were rebuilt


# ---- approximate -----------------------------------------------------------------------------------------------------

def test_state_to_state(be):
    case_state_to_state(be)


def test_mpo_exact(be):
    case_mpo_exact(be)
    assert be.calls.get("dAC", 0) > 0 and be.calls.get("dAC2", 0) > 0      # the composed route


def test_mpo_truncating(be):
    case_truncating(be)


def test_list_of_targets(be):
    case_list(be)


def test_rejects_what_it_cannot_do(be):
    rng = np.random.default_rng(7)
    above = mk.FiniteMPS.random(L, d, 4, rng, be=be)
    with pytest.raises(TypeError):
        mk.approximate(above, above, mk.VUMPS())
    Oc = mk.make_time_mpo(mk.transverse_field_ising(1.0, 0.7, be=be), 0.05, mk.WII())
    with pytest.raises(NotImplementedError):
        mk.approximate(above, (Oc, above), mk.DMRG())
