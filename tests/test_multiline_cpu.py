"""MPSMultiline / MPOMultiline, their environments, leading_boundary and approximate on the NumPy stand-in backend
(tests/cpu_backend.py): host logic only, no GPU.  The stand-in has no dAC_proj / dC_proj, so every row of a column
operator takes the composed route.  The NumPy restatements and the case bodies live here;
tests/test_gpu_multiline.py runs the same bodies on the device."""
import numpy as np
import pytest

import mpskit_jl_amd as mk
from test_vomps_cpu import DenseCpuBackend, env_host, parallel_residual, tl_host, tr_host

KAPPA_C = 2.5337            # test/algorithms.jl:199, to 1e-3


# ---- NumPy restatements (ac_proj / c_proj / the mixed transfers) -------------------------------------

def dAC_host(gl, o, gr, x):
    """y[p,t,q] = sum GL[w][p,a] x[a,s,b] O[w,t,s,v] GR[v][b,q]"""
    return np.einsum("wpa,asb,wtsv,vbq->ptq", gl, x, o, gr, optimize=True)


def dC_host(gl, gr, c):
    return np.einsum("wpa,ab,wbq->pq", gl, c, gr, optimize=True)


def fuse_rows(O1, O2):
    """the one-row MPO of O2 applied after O1, bond chi^2: F[(w2 w1), t, s, (v2 v1)] = sum_m O2[w2,t,m,v2] O1[w1,m,s,v1]"""
    f = np.einsum("atmb,cmsd->actsbd", np.asarray(O2), np.asarray(O1))
    return f.reshape(f.shape[0] * f.shape[1], f.shape[2], f.shape[3], f.shape[4] * f.shape[5])


def random_rows(be, D, R, n=1, seed=3, d=2):
    Ds = [D] * R if np.isscalar(D) else list(D)
    return mk.MPSMultiline([mk.InfiniteMPS.random(d, Ds[r], np.random.default_rng(seed + r), n=n, be=be) for r in range(R)])


# ---- case bodies (shared with the device tests) -----------------------------------------------------------------------

def case_structure(be):
    psi = random_rows(be, 5, 3, n=2)
    assert psi.shape == (3, 2) and len(psi) == 2
    for r in range(3):
        for c in range(2):
            al, ar, ac = be.download(psi.AL[r, c]), be.download(psi.AR[r, c]), be.download(psi.AC[r, c])
            cl, cr = be.download(psi.CR[r, c - 1]), be.download(psi.CR[r, c])
            assert np.abs(np.einsum("asb,bc->asc", al, cr) - ac).max() <= 1e-12
            assert np.abs(np.einsum("ab,bsc->asc", cl, ar) - ac).max() <= 1e-10
            assert psi.AL[r + 3, c - 2] is psi.AL[r, c] and psi.CR[r - 3, c + 4] is psi.CR[r, c]
        assert psi[r] is psi.rows[r] and psi[r + 3] is psi[r]
    again = mk.MPSMultiline.from_AL([[psi.AL[r, c] for c in range(2)] for r in range(3)], [psi.CR[r, 1] for r in range(3)],
                                    tol=1e-12, be=be)
    for r in range(3):
        for c in range(2):
            ac = be.download(again.AC[r, c])
            assert np.abs(np.einsum("asb,bc->asc", be.download(again.AL[r, c]), be.download(again.CR[r, c])) - ac).max() <= 1e-12
            assert np.abs(np.einsum("ab,bsc->asc", be.download(again.CR[r, c - 1]), be.download(again.AR[r, c])) - ac).max() <= 1e-10
    one = mk.InfiniteMPS.random(2, 4, np.random.default_rng(1), be=be)
    assert mk.MPSMultiline(one).to_infinitemps() is one and mk.MPSMultiline([one]).shape == (1, 1)
    O = mk.classical_ising()
    assert mk.MPOMultiline(O).to_densempo() is O and mk.MPOMultiline([O, O]).shape == (2, 1)
    assert mk.MPOMultiline([O, O])[3, 5] is O[0]
    with pytest.raises(ValueError):
        psi.to_infinitemps()


def case_environments(be, above_too=False):
    """every (r, c): lw / rw propagate exactly through the row's mixed transfer and close up to the eigenvalue (solver tol
    1e-12, bound 1e-9, as test_vomps_cpu.case_mixed_environments), |dot(CR_below, c_proj)| = 1, and ac_proj / c_proj are the
    einsum restatements."""
    R, n = 2, 2
    below = random_rows(be, [4, 5], R, n=n, seed=21)
    above = random_rows(be, [6, 3], R, n=n, seed=31) if above_too else None
    mpo = mk.MPOMultiline([mk.classical_ising(0.3).repeat(n), mk.classical_ising(0.4).repeat(n)])
    envs = mk.environments(below, mpo if above is None else (mpo, above), tol=1e-12)
    assert isinstance(envs, mk.PerMPOInfEnv) and isinstance(envs, mk.MultilineEnv)
    top = below if above is None else above
    for r in range(R):
        ka, kb = top[r], below[r + 1]
        lw = [env_host(be, envs.leftenv(r, c, below)) for c in range(n)]
        rw = [env_host(be, envs.rightenv(r, c, below)) for c in range(n)]
        assert lw[0].shape == (2, kb.AL[0].shape[0], ka.AL[0].shape[0]) and envs.lw[r][0] is envs.leftenv(r, 0, below)
        t = lw[0]
        for c in range(n):
            t = tl_host(t, mpo[r, c], be.download(ka.AL[c]), be.download(kb.AL[c]))
            if c < n - 1:
                assert parallel_residual(t, lw[c + 1])[0] <= 1e-12
        resl, laml = parallel_residual(t, lw[0])
        t = rw[n - 1]
        for c in range(n - 1, -1, -1):
            t = tr_host(t, mpo[r, c], be.download(ka.AR[c]), be.download(kb.AR[c]))
            if c > 0:
                assert parallel_residual(t, rw[c - 1])[0] <= 1e-12
        resr, lamr = parallel_residual(t, rw[n - 1])
        print("row", r, "residuals", resl, resr, "eigenvalues", laml, lamr)
        assert resl <= 1e-9 and resr <= 1e-9 and abs(laml - lamr) <= 1e-9 * abs(laml)
        for c in range(n):
            ca, cb = be.download(ka.CR[c]), be.download(kb.CR[c])
            cp = dC_host(lw[(c + 1) % n], rw[c], ca)
            assert abs(abs(np.sum(cb * cp)) - 1.0) <= 1e-12, (r, c)
            got = be.download(envs.c_proj(r, c, below))
            assert np.abs(got - cp).max() <= 1e-12 * max(1.0, np.abs(cp).max())
            ap = dAC_host(lw[c], mpo[r, c], rw[c], be.download(ka.AC[c]))
            got = be.download(mk.ac_proj(r, c, below, envs))
            assert np.abs(got - ap).max() <= 1e-12 * max(1.0, np.abs(ap).max())
    eps = mk.calc_galerkin(below, envs)
    assert np.isfinite(eps) and 0.0 < eps <= 1.0 + 1e-12
    if above is not None:                                    # the pair form of the constructor itself
        again = mk.PerMPOInfEnv(below, (mpo, above), tol=1e-12)
        assert isinstance(again, mk.MultilineEnv) and again.above is above
        with pytest.raises(TypeError):
            mk.PerMPOInfEnv(below, (mpo, above), above=above)


def case_identical_rows(be, D=8, alg=None):
    """MPOMultiline([O, O]) at the critical point on two copies of one random row: every entry 2.5337 +- 1e-3
    (test/algorithms.jl:199), and the product over a cell agrees with the one-row leading_boundary of the same start state:
    both runs stop at a Galerkin error of 1e-6 and the eigenvalue error is of second order in it, so 1e-6 relative is the
    solver tolerance."""
    O = mk.classical_ising()
    alg = mk.VUMPS(tol=1e-6, maxiter=200) if alg is None else alg
    row = lambda: mk.InfiniteMPS.random(2, D, np.random.default_rng(1), be=be)
    psi, envs, eps = mk.leading_boundary(mk.MPSMultiline([row(), row()]), mk.MPOMultiline([O, O]), alg)
    ev = mk.expectation_value(psi, mk.MPOMultiline([O, O]), envs)
    print("identical rows", ev.tolist(), eps)
    assert ev.shape == (2, 1) and np.all(np.abs(ev - KAPPA_C) <= 1e-3), ev
    one, e1, eps1 = mk.leading_boundary(row(), O, alg)
    lam1 = mk.expectation_value(one, O, e1)[0]
    assert eps <= alg.tol and eps1 <= alg.tol
    assert abs(np.prod(ev[:, 0]) / lam1 ** 2 - 1.0) <= alg.tol, (ev, lam1)
    return float(np.prod(ev[:, 0]))


# |prod_r expectation_value[r, 0] / lambda(fused O2 O1) - 1| measured on the NumPy backend with VUMPS(tol = 1e-12, maxiter = 100)
# and the seeds below: D = 8: 3.5e-11, D = 12: 5.6e-13, D = 16: 7.9e-14 (and 2.9e-15 / 3.6e-14 at D = 20 / 24: nothing is gained
# beyond 16).  The difference still falls 7x from D = 12 to D = 16 and then scatters between 1e-15 and 1e-13, so D = 16 is the
# smallest D on the plateau.  The bound of a run is 10 x the value measured at its D.
DIFFERENT_ROWS_MEASURED = {8: 3.5e-11, 12: 5.6e-13, 16: 7.9e-14}
# Galerkin errors at which those runs end (two rows / fused): D = 8: 9e-13 / 8e-13 after 53 / 38 iterations (tol met); D = 12:
# 2.7e-12 / 6e-13 (the two-row run stops at maxiter); D = 16: 1.8e-11 / 9e-11, both at maxiter -- there the Galerkin error
# stays between 7e-11 and 3e-10 from iteration 10 on (Schmidt values at rounding level), so tol = 1e-12 cannot be met and the
# runs are asserted to end below 1e-9.  The eigenvalue error is of second order in the Galerkin error: 1e-18, far below the
# differences above, which are therefore truncation and rounding, not solver error.
DIFFERENT_ROWS_EPS = 1e-9


def different_rows_run(be, D, tol):
    """(expectation_value of the two-row run, eigenvalue of the fused chi = 4 MPO O2 O1, the two-row state, Galerkin errors)"""
    O1, O2 = mk.classical_ising(0.3), mk.classical_ising(0.4)
    mpo = mk.MPOMultiline([O1, O2])
    psi, envs, eps = mk.leading_boundary(random_rows(be, D, 2), mpo, mk.VUMPS(tol=tol, maxiter=100))
    ev = mk.expectation_value(psi, mpo, envs)
    fused = mk.DenseMPO(fuse_rows(O1[0], O2[0]))
    f, fe, feps = mk.leading_boundary(mk.InfiniteMPS.random(2, D, np.random.default_rng(5), be=be), fused,
                                      mk.VUMPS(tol=tol, maxiter=100))
    return ev, float(mk.expectation_value(f, fused, fe)[0]), psi, (eps, feps)


def case_different_rows(be, D=16):
    """O1 = classical_ising(0.3) above O2 = classical_ising(0.4): the product over the two rows of expectation_value[:, 0]
    against the leading eigenvalue of the fused chi = 4 MPO O2 O1 from the one-row leading_boundary, both with tol = 1e-12.
    Measured differences: D = 8: 3.5e-11, D = 12: 5.6e-13, D = 16: 7.9e-14; D = 16 is the smallest D on the plateau.
    Asserted: 10 x the value of the D in use (7.9e-13 at D = 16), and that both runs end at a Galerkin error below 1e-9 (at
    D = 12 and 16 they stop at maxiter = 100, see DIFFERENT_ROWS_EPS)."""
    ev, lam, psi, (eps, feps) = different_rows_run(be, D, 1e-12)
    diff = abs(np.prod(ev[:, 0]) / lam - 1.0)
    print("different rows D", D, ev.tolist(), lam, "difference", diff, "galerkin", eps, feps)
    assert np.all(ev > 0)
    assert eps <= DIFFERENT_ROWS_EPS and feps <= DIFFERENT_ROWS_EPS, (eps, feps)
    assert diff <= 10 * DIFFERENT_ROWS_MEASURED[D], (diff, ev, lam)
    return float(np.prod(ev[:, 0]))


def case_vomps_same_eigenvalue(be, D=8):
    """the power method reaches the eigenvalue of the fused MPO: it stops at a Galerkin error of 1e-9, the eigenvalue error
    is of second order in it plus the D = 8 truncation measured above (3.5e-11), so 1e-9 relative is a loose solver bound"""
    O1, O2 = mk.classical_ising(0.3), mk.classical_ising(0.4)
    mpo = mk.MPOMultiline([O1, O2])
    psi, envs, eps = mk.leading_boundary(random_rows(be, D, 2), mpo, mk.VOMPS(tol=1e-9, maxiter=400))
    ev = mk.expectation_value(psi, mpo, envs)
    fused = mk.DenseMPO(fuse_rows(O1[0], O2[0]))
    f, fe, _ = mk.leading_boundary(mk.InfiniteMPS.random(2, D, np.random.default_rng(5), be=be), fused,
                                   mk.VUMPS(tol=1e-11, maxiter=100))
    lam = mk.expectation_value(f, fused, fe)[0]
    print("VOMPS", ev.tolist(), lam, eps)
    assert eps <= 1e-9 and abs(np.prod(ev[:, 0]) / lam - 1.0) <= 1e-9


def case_approximate_identity(be):
    """O = identity MPO and below started from above: approximate returns above, dot = 1 per row (the rows shift by one: row
    r + 1 of the result is row r of above)."""
    d = 2
    eye = mk.DenseMPO(np.eye(d).reshape(1, d, d, 1))
    above = random_rows(be, 5, 2, seed=41)
    below = mk.MPSMultiline([above[1], above[0]])            # row r + 1 below approximates row r above
    out, envs, eps = mk.approximate(below, (mk.MPOMultiline([eye, eye]), above), mk.VOMPS(tol=1e-10, maxiter=20))
    assert eps <= 1e-10
    for r in range(2):
        assert abs(abs(mk.dot(out[r + 1], above[r])) - 1.0) <= 1e-9, r


def case_approximate_ising(be, D=8):
    """approximate of (two-row Ising MPO, its converged boundary) at the same D: the result is again the fixed point, and
    the normalisation of its environments carries the eigenvalue found by leading_boundary"""
    ev, lam, psi, (eps0, _) = different_rows_run(be, D, 1e-11)
    lam2 = float(np.prod(ev[:, 0]))
    assert eps0 <= 1e-11
    O1, O2 = mk.classical_ising(0.3), mk.classical_ising(0.4)
    mpo = mk.MPOMultiline([O1, O2])
    start = mk.MPSMultiline([psi[0], psi[1]])
    out, envs, eps = mk.approximate(start, (mpo, psi), mk.VOMPS(tol=1e-9, maxiter=50))
    assert eps <= 1e-9
    for r in range(2):
        assert abs(abs(mk.dot(out[r], psi[r])) - 1.0) <= 1e-8, r
    e2 = mk.environments(out, mpo, tol=1e-11)
    got = float(np.prod(mk.expectation_value(out, mpo, e2)[:, 0]))
    print("approximate ising", got, lam2, lam)
    assert abs(got / lam - 1.0) <= 1e-8


def case_mixed_D(be):
    """rows of different D: a finite Galerkin error that the iteration brings below its tolerance"""
    mpo = mk.MPOMultiline([mk.classical_ising(0.3), mk.classical_ising(0.4)])
    psi = random_rows(be, [4, 6], 2)
    envs = mk.environments(psi, mpo)
    e0 = mk.calc_galerkin(psi, envs)
    out, envs, eps = mk.leading_boundary(psi, mpo, mk.VUMPS(tol=1e-8, maxiter=50), envs)
    assert np.isfinite(e0) and np.isfinite(eps) and eps <= 1e-8 < e0
    assert [out[r].AL[0].shape[0] for r in range(2)] == [4, 6]


# ---- tests -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def be():
    return DenseCpuBackend()


def test_structure(be):
    case_structure(be)


@pytest.mark.parametrize("above_too", [False, True])
def test_environments(be, above_too):
    case_environments(be, above_too)


def test_identical_rows(be):
    case_identical_rows(be)


def test_different_rows(be):
    case_different_rows(be, D=16)


def test_vomps_same_eigenvalue(be):
    case_vomps_same_eigenvalue(be)


def test_approximate_identity(be):
    case_approximate_identity(be)


def test_approximate_ising(be):
    case_approximate_ising(be)


def test_mixed_bond_dimensions(be):
    case_mixed_D(be)


def test_finalize_hook_is_called(be):
    seen = []

    def fin(it, psi, mpo, envs):
        seen.append((it, psi.shape))
        return psi, envs

    mpo = mk.MPOMultiline([mk.classical_ising(0.3), mk.classical_ising(0.4)])
    mk.leading_boundary(random_rows(be, 4, 2), mpo, mk.VUMPS(tol=1e-6, maxiter=3, finalize=fin))
    assert seen and seen[0] == (1, (2, 1))


def test_one_row_path_is_unchanged(be):
    """leading_boundary(InfiniteMPS, DenseMPO) keeps its code path: it never builds a MultilineEnv"""
    O = mk.classical_ising(0.3)
    psi, envs, eps = mk.leading_boundary(mk.InfiniteMPS.random(2, 4, np.random.default_rng(1), be=be), O,
                                         mk.VUMPS(tol=1e-8, maxiter=50))
    assert type(envs) is mk.PerMPOInfEnv and isinstance(psi, mk.InfiniteMPS)


def test_errors(be):
    a = mk.InfiniteMPS.random(2, 4, np.random.default_rng(1), n=1, be=be)
    b = mk.InfiniteMPS.random(2, 4, np.random.default_rng(2), n=2, be=be)
    with pytest.raises(ValueError, match="row 1"):
        mk.MPSMultiline([a, b])
    O = mk.classical_ising(0.3)
    with pytest.raises(ValueError, match="row 1"):
        mk.MPOMultiline([O, O.repeat(2)])
    with pytest.raises(ValueError, match="2 rows"):
        mk.environments(mk.MPSMultiline([a, a]), mk.MPOMultiline([O]))
    with pytest.raises(ValueError, match="2 rows"):
        mk.MPSMultiline([a, a]).to_infinitemps()
    cx = mk.InfiniteMPS.random(2, 4, np.random.default_rng(1), be=be)
    cx.cplx = True
    with pytest.raises(NotImplementedError, match="row 1"):
        mk.MPSMultiline([a, cx])
    with pytest.raises(TypeError):
        mk.leading_boundary(mk.MPSMultiline([a, a]), mk.MPOMultiline([O, O]), mk.DMRG())
    with pytest.raises(TypeError):
        mk.leading_boundary(mk.MPSMultiline([a, a]), O)
    with pytest.raises(TypeError):
        mk.approximate(mk.MPSMultiline([a, a]), (mk.MPOMultiline([O, O]), a), mk.VOMPS())
