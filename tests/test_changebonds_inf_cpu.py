"""changebonds for InfiniteMPS (optimalexpand.jl:16-67, randexpand.jl:15-34, svdcut.jl:35-46, changebonds.jl:13-38) on the
host stand-in backend: the composed route (dAC2, null-space bases by QRpos / LQpos, tsvd) and the device-tensor _expand."""
import math

import numpy as np
import pytest

import mpskit_jl_amd as mk
import mpskit_oracle as mo
from mpskit_jl_amd.changebonds import expansion_directions
from mpskit_jl_amd.environments import MPOHamInfEnv, environments
from cpu_backend import CpuBackend, HostSlice
from test_statmech_cpu import onsager_kappa

BETA_C = math.log(1.0 + math.sqrt(2.0)) / 2.0


class DenseCpuBackend(CpuBackend):
    """CpuBackend + mposlice_dense: a DenseMPO tensor as a one-level host slice (oracle arithmetic)."""

    def mposlice_dense(self, O):
        O = np.asarray(O)
        return HostSlice(1, O.shape[1], [O.shape[0]], [O.shape[3]], {(0, 0): O})


def _bond_dims(psi):
    return [c.shape[0] for c in psi.CR]


def _mixed_transfer_lambda(be, new, old):
    """leading |eigenvalue| of the mixed transfer matrix sum_s AL_new[s] (x) AL_old[s] over the unit cell (NumPy)"""
    T = None
    for a, b in zip(new.AL, old.AL):
        A, B = be.download(a), be.download(b)
        E = np.einsum("asb,psq->apbq", A, B).reshape(A.shape[0] * B.shape[0], A.shape[2] * B.shape[2])
        T = E if T is None else T @ E
    return np.abs(np.linalg.eigvals(T)).max()


def _check_mixed_gauge(be, psi, tol=1e-12):
    n = len(psi)
    for i in range(n):
        al, ar, ac = be.download(psi.AL[i]), be.download(psi.AR[i]), be.download(psi.AC[i])
        c, cm = be.download(psi.CR[i]), be.download(psi.CR[(i - 1) % n])
        Dl, d, Dr = al.shape
        assert al.shape == ar.shape == ac.shape and c.shape == (Dr, Dr) and cm.shape == (Dl, Dl)
        L = al.reshape(Dl * d, Dr)
        R = ar.reshape(Dl, d * Dr)
        assert np.abs(L.T @ L - np.eye(Dr)).max() < tol
        assert np.abs(R @ R.T - np.eye(Dl)).max() < tol
        assert np.abs(np.einsum("asb,bc->asc", al, c) - ac).max() < tol
        assert np.abs(np.einsum("ab,bsc->asc", cm, ar) - ac).max() < tol


# ---- 1: fails at the parent commit (NotImplementedError) ------------------------------------------------------------------

def test_optimal_expand_hamiltonian_grows_every_bond():
    be = CpuBackend()
    H = mk.heisenberg_XXX(1.0, be=be)
    psi = mk.InfiniteMPS.random(3, 6, np.random.default_rng(0), n=2, be=be)
    new, envs = mk.changebonds(psi, H, mk.OptimalExpand(trunc_dim=4))
    assert _bond_dims(new) == [10, 10] and _bond_dims(psi) == [6, 6]
    assert isinstance(envs, MPOHamInfEnv)


def test_optimal_expand_dense_mpo_rand_expand_and_svd_cut():
    be = DenseCpuBackend()
    mpo = mk.classical_ising()
    psi = mk.InfiniteMPS.random(2, 4, np.random.default_rng(1), be=be)
    new, envs = mk.changebonds(psi, mpo, mk.OptimalExpand(trunc_dim=3))
    assert _bond_dims(new) == [7] and isinstance(envs, mk.PerMPOInfEnv)
    rnd = mk.changebonds(psi, mk.RandExpand(trunc_dim=2))
    assert _bond_dims(rnd) == [6]
    _check_mixed_gauge(be, rnd)
    assert abs(_mixed_transfer_lambda(be, rnd, psi) - 1.0) < 1e-12
    cut = mk.changebonds(new, mk.SvdCut(trunc_dim=4))
    assert _bond_dims(cut) == [4]
    # trunc_dim is capped by the complement: d D - D directions exist on each side
    big, _ = mk.changebonds(psi, mpo, mk.OptimalExpand(trunc_dim=100))
    assert _bond_dims(big) == [8]


def test_complex_states_are_refused():
    be = CpuBackend()
    psi = mk.InfiniteMPS.random(2, 4, np.random.default_rng(1), be=be)
    psi.cplx = True
    with pytest.raises(NotImplementedError):
        mk.changebonds(psi, mk.RandExpand(trunc_dim=2))


# ---- 2: the expansion changes nothing physical --------------------------------------------------------------------------

@pytest.mark.parametrize("model", ["heisenberg", "tfi"])
@pytest.mark.parametrize("n", [1, 2])
def test_expansion_is_a_gauge_preserving_embedding(model, n):
    be = CpuBackend()
    if model == "heisenberg":
        H, d = mk.heisenberg_XXX(1.0, be=be), 3
    else:
        H, d = mk.transverse_field_ising(be=be), 2
    psi = mk.InfiniteMPS.random(d, 6, np.random.default_rng(7 + n), n=n, be=be)
    envs = environments(psi, H)
    e0 = mk.expectation_value(psi, H, envs)
    new, envs2 = mk.changebonds(psi, H, mk.OptimalExpand(trunc_dim=4), envs)
    assert _bond_dims(new) == [10] * n
    _check_mixed_gauge(be, new)
    e1 = mk.expectation_value(new, H, envs2)
    assert np.abs(np.asarray(e1) - np.asarray(e0)).max() < 1e-12
    assert abs(_mixed_transfer_lambda(be, new, psi) - 1.0) < 1e-12


def test_dense_mpo_expectation_value_unchanged():
    be = DenseCpuBackend()
    mpo = mk.classical_ising(0.3)
    psi = mk.InfiniteMPS.random(2, 6, np.random.default_rng(3), be=be)
    envs = mk.PerMPOInfEnv(psi, mpo)
    lam0 = mk.statmech.expectation_value(psi, mpo, envs)
    new, envs = mk.changebonds(psi, mpo, mk.OptimalExpand(trunc_dim=4), envs)
    assert _bond_dims(new) == [10]
    _check_mixed_gauge(be, new)
    lam1 = mk.statmech.expectation_value(new, mpo, envs)
    assert np.abs(lam1 / lam0 - 1.0).max() < 1e-12
    assert abs(_mixed_transfer_lambda(be, new, psi) - 1.0) < 1e-12


# ---- 3: optimality against a NumPy restatement of optimalexpand.jl:22-29 --------------------------------------------------

def gap_rank(s, kmax=6):
    """largest k <= kmax with (s_k - s_{k+1}) >= 1e-3 s_1 (1-based), 0 if none"""
    best = 0
    for k in range(1, min(kmax, len(s) - 1) + 1):
        if s[k - 1] - s[k] >= 1e-3 * s[0]:
            best = k
    return best


def test_directions_are_the_optimal_ones():
    be = CpuBackend()
    H = mk.transverse_field_ising(g=0.9, be=be)
    psi = mk.InfiniteMPS.random(2, 8, np.random.default_rng(5), be=be)
    psi, envs, eps = mk.find_groundstate(psi, H, mk.VUMPS(tol=1e-4, maxiter=50))
    assert 1e-7 < eps <= 1e-4
    U, Vt, S, kept = expansion_directions(psi, H, envs, 0, 6)
    assert kept == 6
    # NumPy restatement: complete-QR null spaces, the oracle's dAC2, LAPACK SVD
    al, ar, ac = (be.download(t) for t in (psi.AL[0], psi.AR[0], psi.AC[0]))
    GL = be._env(envs.leftenv(0, psi), H[0].chil)
    GR = be._env(envs.rightenv(1, psi), H[1].chir)
    ac2 = np.einsum("asm,mtb->asbt", ac, ar)
    y = mo.dAC2(ac2, H[0].oracle, H[1].oracle, GL, GR)
    VL, VR = mo.leftnull(al), mo.rightnull(ar)
    inter = np.einsum("asn,asbt,mtb->nm", VL, y, VR)
    u, s, vh = np.linalg.svd(inter)
    assert np.abs(S - s[:6]).max() <= 1e-10 * s[0]
    k = gap_rank(s)
    assert k >= 2, f"no spectral gap among the leading values {s[:7]}"
    Uref = np.transpose(VL, (1, 0, 2)).reshape(-1, VL.shape[2]) @ u[:, :k]      # rows a + Dl s (column-major (a, s))
    Ug = be.download(U)[:, :k]
    assert np.abs(Ug @ Ug.T - Uref @ Uref.T).max() <= 1e-8
    Vref = vh[:k] @ VR.reshape(VR.shape[0], -1)                                 # columns b + Dr s
    Vg = be.download(Vt)[:k]
    assert np.abs(Vg.T @ Vg - Vref.T @ Vref).max() <= 1e-8


# ---- 4: grow and converge -----------------------------------------------------------------------------------------------

def _grow_boundary(be, mpo, Ds, tol, seed=1):
    psi = mk.InfiniteMPS.random(mpo.d, Ds[0], np.random.default_rng(seed), be=be)
    psi, envs, eps = mk.leading_boundary(psi, mpo, mk.VUMPS(tol=tol, maxiter=200))
    for D in Ds[1:]:
        psi, envs = mk.changebonds(psi, mpo, mk.OptimalExpand(trunc_dim=D - _bond_dims(psi)[0]), envs)
        assert _bond_dims(psi) == [D]
        psi, envs, eps = mk.leading_boundary(psi, mpo, mk.VUMPS(tol=tol, maxiter=200), envs)
    return psi, envs, eps


def test_ising_boundary_grown_matches_onsager():
    be = DenseCpuBackend()
    mpo = mk.classical_ising(0.3)
    psi, envs, eps = _grow_boundary(be, mpo, [2, 4, 6], 1e-9)
    lam = mk.statmech.expectation_value(psi, mpo, envs)
    assert abs(lam[0] / onsager_kappa(0.3) - 1.0) < 1e-10
    assert eps <= 1e-9


def test_critical_ising_grown_reference_value():
    be = DenseCpuBackend()
    mpo = mk.classical_ising(BETA_C)
    psi, envs, eps = _grow_boundary(be, mpo, [4, 8], 1e-6)
    lam = mk.statmech.expectation_value(psi, mpo, envs)
    assert lam[0] == pytest.approx(2.5337, abs=1e-3)


def test_itfi_grown_reaches_the_random_start_energy():
    be = CpuBackend()
    H = mk.transverse_field_ising(be=be)
    alg = mk.VUMPS(tol=1e-10, maxiter=300)
    psi = mk.InfiniteMPS.random(2, 4, np.random.default_rng(2), be=be)
    psi, envs, _ = mk.find_groundstate(psi, H, alg)
    energies = {}
    for D in (8, 12):
        psi, envs = mk.changebonds(psi, H, mk.OptimalExpand(trunc_dim=D - _bond_dims(psi)[0]), envs)
        psi, envs, eps = mk.find_groundstate(psi, H, alg, envs)
        assert eps <= 1e-10
        energies[D] = float(np.sum(mk.expectation_value(psi, H, envs)))
    ref = mk.InfiniteMPS.random(2, 12, np.random.default_rng(9), be=be)
    ref, renvs, _ = mk.find_groundstate(ref, H, alg)
    Eref = float(np.sum(mk.expectation_value(ref, H, renvs)))
    assert abs(energies[12] - Eref) < 1e-8
    assert energies[12] < energies[8]


# ---- 5: SvdCut ----------------------------------------------------------------------------------------------------------

def test_svd_cut_removes_an_empty_expansion():
    be = DenseCpuBackend()
    mpo = mk.classical_ising(0.3)
    psi = mk.InfiniteMPS.random(2, 8, np.random.default_rng(4), be=be)
    psi, envs, _ = mk.leading_boundary(psi, mpo, mk.VUMPS(tol=1e-10, maxiter=200))
    big, envs = mk.changebonds(psi, mpo, mk.OptimalExpand(trunc_dim=4), envs)
    assert _bond_dims(big) == [12]
    cut = mk.changebonds(big, mk.SvdCut(trunc_dim=8))
    assert _bond_dims(cut) == [8]
    _check_mixed_gauge(be, cut, tol=1e-10)
    assert abs(_mixed_transfer_lambda(be, cut, psi) - 1.0) < 1e-10


def test_svd_cut_truncerr_rule():
    """k from the singular values of CR and the rule of mpsk_tsvd (drop the tail while its 2-norm stays <= trunc_err)."""
    be = CpuBackend()
    psi = mk.InfiniteMPS.random(2, 10, np.random.default_rng(6), n=2, be=be)
    err = 0.05
    want = []
    for c in psi.CR:
        s = np.linalg.svd(be.download(c), compute_uv=False)
        k = len(s)
        while k > 1 and np.sqrt(np.sum(s[k - 1:] ** 2)) <= err:
            k -= 1
        want.append(k)
    assert any(k < 10 for k in want)
    cut = mk.changebonds(psi, mk.SvdCut(trunc_err=err))
    assert _bond_dims(cut) == want
