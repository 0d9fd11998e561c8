"""Bond expansion of a uniform state on the device: mpsk_dAC2_product against mpsk_dAC2 on the formed product (and against
numpy.einsum where mpsk_dAC2 is not feasible), mpsk_complement_tsvd against NumPy on planted spectra, the device route of
changebonds against the composed one, and growing runs end to end."""
import numpy as np
import pytest

import mpskit_jl_amd as mk
from mpskit_jl_amd.changebonds import expansion_directions

pytestmark = pytest.mark.gpu

RTOL = 2e-13          # tests/test_gpu_ops.py: mpsk_dAC2 is held to RTOL * max(Dl, Dr) * d against the oracle


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _slabs(be, arr):
    """host [D1, D2, W] (slab w = arr[:, :, w]) -> device environment (W, D1, D2)."""
    return be.upload(arr).reshape(arr.shape[2], arr.shape[0], arr.shape[1])


def _product_inputs(be, Wl, Wr, Dl, Dm, Dr, d1, d2, rng):
    G = rng.standard_normal((Dl, Dl, Wl))
    R = rng.standard_normal((Dr, Dr, Wr))
    ac = rng.standard_normal((Dl, d1, Dm))
    ar = rng.standard_normal((Dm, d2, Dr))
    return G, R, ac, ar, _slabs(be, G), _slabs(be, R), be.upload(ac), be.upload(ar)


def _formed(be, ac, ar):
    return be.upload(np.einsum("asm,mtb->asbt", ac, ar))


# ---- 10: both entries first on a fresh context (workspace sized inside the entry) -----------------------------------------

def test_fresh_context_first_calls():
    be = mk.Backend(0)
    try:
        rng = np.random.default_rng(10)
        H = mk.heisenberg_XXX(1.0, be=be)
        G, R, ac, ar, dG, dR, dac, dar = _product_inputs(be, 5, 5, 96, 96, 96, 3, 3, rng)
        y = be.download(be.dAC2_product(H[0], H[1], dG, dR, dac, dar))
        ref = be.download(be.dAC2(H[0], H[1], dG, dR, _formed(be, ac, ar)))
        assert relerr(y, ref) < RTOL * 96 * 3
    finally:
        be.close()
    be = mk.Backend(0)
    try:
        _complement_case(be, 300, 280, 100, 90, 24, np.random.default_rng(11))
    finally:
        be.close()


# ---- 6: mpsk_dAC2_product --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("model,Dl,Dm,Dr", [("tfi5", 48, 48, 48), ("heis", 130, 130, 130), ("heis", 70, 33, 51)])
def test_product_matches_dAC2_hamiltonian_slices(be, model, Dl, Dm, Dr):
    rng = np.random.default_rng(Dl + Dm)
    H = mk.heisenberg_XXX(1.0 if model == "heis" else 0.5, be=be)          # W = 5; d = 3 / d = 2
    d = H[0].d
    G, R, ac, ar, dG, dR, dac, dar = _product_inputs(be, 5, 5, Dl, Dm, Dr, d, d, rng)
    y = be.download(be.dAC2_product(H[0], H[1], dG, dR, dac, dar))
    ref = be.download(be.dAC2(H[0], H[1], dG, dR, _formed(be, ac, ar)))
    assert y.shape == (Dl, d, Dr, d)
    assert relerr(y, ref) < RTOL * max(Dl, Dm, Dr) * d


@pytest.mark.parametrize("chi,D", [(2, 40), (4, 48), (9, 33)])
def test_product_matches_dAC2_dense_slices(be, chi, D):
    rng = np.random.default_rng(chi)
    O1, O2 = rng.standard_normal((chi, chi, chi, chi)), rng.standard_normal((chi, chi, chi, chi))
    H1, H2 = be.mposlice_dense(O1), be.mposlice_dense(O2)
    G, R, ac, ar, dG, dR, dac, dar = _product_inputs(be, chi, chi, D, D + 3, D - 5, chi, chi, rng)
    y = be.download(be.dAC2_product(H1, H2, dG, dR, dac, dar))
    ref = be.download(be.dAC2(H1, H2, dG, dR, _formed(be, ac, ar)))
    err = relerr(y, ref)
    print(f"dAC2_product dense chi={chi} D={D}: relerr {err:.3e} (bar {RTOL * (D + 3) * chi:.3e})")
    assert err < RTOL * (D + 3) * chi                      # max(Dl, Dm, Dr) = D + 3, d = chi


def test_product_dense_16_against_einsum(be):
    """chi = d = 16, D = 64: the slab mix of mpsk_dAC2 is not asked to run; numpy.einsum, evaluated pairwise."""
    chi, D = 16, 64
    rng = np.random.default_rng(16)
    O1, O2 = rng.standard_normal((chi,) * 4), rng.standard_normal((chi,) * 4)
    H1, H2 = be.mposlice_dense(O1), be.mposlice_dense(O2)
    G, R, ac, ar, dG, dR, dac, dar = _product_inputs(be, chi, chi, D, D, D, chi, chi, rng)
    y = be.download(be.dAC2_product(H1, H2, dG, dR, dac, dar))
    L1 = np.einsum("paw,asm->pwsm", G, ac, optimize=True)
    L2 = np.einsum("pwsm,wtsu->ptmu", L1, O1, optimize=True)
    R1 = np.einsum("msb,bqv->msqv", ar, R, optimize=True)
    R2 = np.einsum("msqv,utsv->mtqu", R1, O2, optimize=True)
    ref = np.einsum("ptmu,mxqu->ptqx", L2, R2, optimize=True)
    err = relerr(y, ref)
    print(f"dAC2_product dense chi=16 D=64: relerr {err:.3e} (bar {RTOL * D * chi:.3e})")
    assert err < RTOL * D * chi


# ---- 7: mpsk_complement_tsvd -----------------------------------------------------------------------------------------------

def _planted(m, n, pl, pr, sig, rng):
    """Y whose complement part is NL diag(sig) NR^T, plus components inside span(QL) / span(QR) that the projectors remove"""
    Qm, _ = np.linalg.qr(rng.standard_normal((m, m)))
    Qn, _ = np.linalg.qr(rng.standard_normal((n, n)))
    QL, NL = Qm[:, :pl], Qm[:, pl:]
    QR, NR = Qn[:, :pr].T, Qn[:, pr:].T
    r = min(m - pl, n - pr, len(sig))
    X = (NL[:, :r] * sig[:r]) @ NR[:r]
    Y = X + QL @ rng.standard_normal((pl, n)) + rng.standard_normal((m, pr)) @ QR
    return Y, QL, QR


def _check_contract(be, U, S, Vt, kept, QL, QR, sig, k):
    m, n = QL.shape[0], QR.shape[1]
    want = min(k, m - QL.shape[1], n - QR.shape[0])
    assert kept == want
    u, s, vt = be.download(U), be.download(S), be.download(Vt)
    assert u.shape == (m, kept) and vt.shape == (kept, n) and s.shape == (kept,)
    ref = np.zeros(kept)
    ref[:min(kept, len(sig))] = sig[:kept]
    scale = max(ref[0], s[0])
    assert np.all(np.diff(s) <= 0), "S is not descending"
    assert np.abs(s - ref).max() <= 1e-10 * scale
    assert np.abs(u.T @ u - np.eye(kept)).max() <= 1e-12
    assert np.abs(vt @ vt.T - np.eye(kept)).max() <= 1e-12
    assert np.abs(QL.T @ u).max() <= 1e-12
    assert np.abs(vt @ QR.T).max() <= 1e-12
    return u, s, vt


def _complement_case(be, m, n, pl, pr, k, rng, sig=None):
    if sig is None:
        sig = 2.0 ** (-np.arange(min(m - pl, n - pr)) / 4.0)
    Y, QL, QR = _planted(m, n, pl, pr, sig, rng)
    U, S, Vt, kept = be.complement_tsvd(be.upload(Y), be.upload(QL), be.upload(QR), k)
    return _check_contract(be, U, S, Vt, kept, QL, QR, sig, k)


@pytest.mark.parametrize("m,n,p,k", [(96, 96, 48, 16), (260, 390, 130, 32), (2048, 2048, 1024, 64), (2048, 2048, 1024, 256),
                                     (260, 390, 130, 1), (96, 96, 48, 60), (40, 56, 20, 8)])
def test_complement_tsvd_graded(be, m, n, p, k):
    _complement_case(be, m, n, p, p, k, np.random.default_rng(m + k))


def test_complement_tsvd_leading_vectors(be):
    """the leading, well separated directions are the planted ones (sigma_j = 2^(-j/4): gaps of 16 %)"""
    m, n, p, k = 260, 390, 130, 8
    rng = np.random.default_rng(3)
    sig = 2.0 ** (-np.arange(130) / 4.0)
    Y, QL, QR = _planted(m, n, p, p, sig, rng)
    U, S, Vt, kept = be.complement_tsvd(be.upload(Y), be.upload(QL), be.upload(QR), k)
    u, s, vt = _check_contract(be, U, S, Vt, kept, QL, QR, sig, k)
    X = (np.eye(m) - QL @ QL.T) @ Y @ (np.eye(n) - QR.T @ QR)
    assert np.abs(u.T @ X @ vt.T - np.diag(sig[:k])).max() <= 1e-10


def test_complement_tsvd_edge_cases(be):
    rng = np.random.default_rng(5)
    # m = pl: the complement is empty, kept = 0
    Q, _ = np.linalg.qr(rng.standard_normal((80, 80)))
    Qn, _ = np.linalg.qr(rng.standard_normal((120, 120)))
    U, S, Vt, kept = be.complement_tsvd(be.upload(rng.standard_normal((80, 120))), be.upload(Q), be.upload(Qn[:40]), 5)
    assert kept == 0 and U is None
    # Y = 0: S = 0 and isometries inside the complement all the same
    Y, QL, QR = _planted(150, 140, 50, 40, np.zeros(4), rng)
    U, S, Vt, kept = be.complement_tsvd(be.zeros(150, 140), be.upload(QL), be.upload(QR), 12)
    _check_contract(be, U, S, Vt, kept, QL, QR, np.zeros(12), 12)
    # rank of X below k: the missing directions are completed with S = 0
    _complement_case(be, 200, 180, 60, 60, 20, rng, sig=np.array([3.0, 2.0, 1.0]))


def test_complement_tsvd_full_iteration_is_counted(be):
    """flat spectrum, k close to the dimension of the complement: no subspace of r > k columns fits below 5/8 of the
    matrix, so the full iteration runs -- and the counter shows it"""
    before = be.complement_stats()
    _complement_case(be, 260, 390, 130, 130, 120, np.random.default_rng(8), sig=np.ones(130))
    after = be.complement_stats()
    assert after["calls"] == before["calls"] + 1
    assert after["full"] == before["full"] + 1 and after["subspace"] == before["subspace"]
    assert be.split_stats()["path"] in (0, 2)


# ---- 8: device route == composed route -------------------------------------------------------------------------------------

def gap_rank(s, kmax=6):
    best = 0
    for k in range(1, min(kmax, len(s) - 1) + 1):
        if s[k - 1] - s[k] >= 1e-3 * s[0]:
            best = k
    return best


@pytest.mark.parametrize("model,n,k", [("heis1", 1, 16), ("tfi", 2, 16)])
def test_device_route_equals_composed_route(be, model, n, k):
    # The bar 1e-10 S[0] can only be resolved in fp64 while S[0] >~ 1e-6 |Y|: both routes carry rounding errors of
    # ~1e-16 |Y|.  S[0] is of the order of the first Schmidt value the state lacks.  A TFI state that VUMPS has touched has
    # S[0] ~ 1e-9 (measured: 1.6e-9 at D = 64 converged to 1e-4, 4.0e-9 at D = 48 after 3 iterations), and
    # InfiniteMPS.random (entries in [0, 1): a transfer matrix with a large gap) has numerical Schmidt rank << 64, so its
    # expansion block is rounding noise (S[0] = 1.3e-15).  The TFI state is therefore a uniform state of Gaussian tensors,
    # whose Schmidt spectrum is flat.
    from mpskit_jl_amd.environments import environments
    if model == "heis1":
        H, d, D = mk.heisenberg_XXX(1.0, be=be), 3, 64
        psi = mk.InfiniteMPS.random(d, D, np.random.default_rng(21), n=n, be=be)
        psi, envs, _ = mk.find_groundstate(psi, H, mk.VUMPS(tol=1e-4, maxiter=30))
    else:
        H, d, D = mk.transverse_field_ising(be=be), 2, 64
        rng = np.random.default_rng(21)
        psi = mk.InfiniteMPS.from_tensors([rng.standard_normal((D, d, D)) for _ in range(n)], be=be)
        envs = environments(psi, H)
    for i in range(n):
        Ud, Vd, Sd, kd = expansion_directions(psi, H, envs, i, k, route="device")
        Uc, Vc, Sc, kc = expansion_directions(psi, H, envs, i, k, route="composed")
        assert kd == kc == k
        assert np.abs(Sd - Sc).max() <= 1e-10 * Sc[0]
        g = gap_rank(Sc)
        assert g >= 2, Sc[:7]
        ud, uc = be.download(Ud)[:, :g], be.download(Uc)[:, :g]
        assert np.abs(ud @ ud.T - uc @ uc.T).max() <= 1e-8
        vd, vc = be.download(Vd)[:g], be.download(Vc)[:g]
        assert np.abs(vd.T @ vd - vc.T @ vc).max() <= 1e-8


# ---- 9: end to end ---------------------------------------------------------------------------------------------------------

def test_cluster4_ising_grown_matches_onsager(be):
    """4 x 4 clusters (chi = d = 16), beta = 0.3: D = 16 -> 32 by OptimalExpand, then leading_boundary: kappa^16 to 1e-9"""
    from test_statmech_cpu import onsager_kappa
    mpo = mk.classical_ising(0.3, cluster=4)
    psi = mk.InfiniteMPS.random(16, 16, np.random.default_rng(1), be=be)
    psi, envs, _ = mk.leading_boundary(psi, mpo, mk.VUMPS(tol=1e-6, maxiter=100))
    psi, envs = mk.changebonds(psi, mpo, mk.OptimalExpand(trunc_dim=16), envs)
    assert [c.shape[0] for c in psi.CR] == [32]
    assert be.complement_stats()["calls"] >= 1                 # 256 x 256 bond matrices: the device route
    psi, envs, eps = mk.leading_boundary(psi, mpo, mk.VUMPS(tol=1e-9, maxiter=100), envs)
    lam = float(mk.statmech.expectation_value(psi, mpo, envs)[0])
    assert abs(lam / onsager_kappa(0.3) ** 16 - 1.0) < 1e-9, (lam, eps)


def test_itfi_grown_through_finalize_energy_is_monotone(be):
    H = mk.transverse_field_ising(be=be)
    grown = {}

    def finalize(it, psi, H_, envs):
        D = psi.CR[0].shape[0]
        if it in (12, 24) and D < 128:
            grown[D] = float(np.sum(mk.expectation_value(psi, H_, envs)))
            psi, envs = mk.changebonds(psi, H_, mk.OptimalExpand(trunc_dim=D), envs)
        return psi, envs

    psi = mk.InfiniteMPS.random(2, 32, np.random.default_rng(4), be=be)
    # tol below what the run can reach: every iteration of the schedule runs, whatever D = 32 / 64 converge to
    psi, envs, eps = mk.find_groundstate(psi, H, mk.VUMPS(tol=1e-14, maxiter=36, finalize=finalize))
    assert [c.shape[0] for c in psi.CR] == [128] and sorted(grown) == [32, 64]
    E = float(np.sum(mk.expectation_value(psi, H, envs)))
    assert E < grown[64] < grown[32], (grown, E)
