"""Host logic of the statistical-mechanics quasiparticle excitations on the NumPy stand-in backend (tests/cpu_backend.py,
which has none of the new entries, so everything here takes the composed route): the effective operator against a dense
NumPy restatement of quasiparticleexcitation.jl:258-293 and qpenv.jl:171-303 written below, its leading eigenvalue, and
the planar complex Arnoldi on its own."""
import math
import warnings

import numpy as np
import pytest

import mpskit_jl_amd as mk
from mpskit_jl_amd import krylov, quasiparticle as qpm
from mpskit_jl_amd.backend import DTensor
from test_vomps_cpu import DenseCpuBackend, env_host, tl_host, tr_host

BETA, D = 0.3, 4


def proj_host(gl, x, o, gr):
    return np.einsum("wpa,asb,wtsv,vbq->ptq", gl, x, o, gr, optimize=True)


def dense_heff(be, ctx, phi, p):
    """The N x N complex matrix of the effective operator, one row (:258-293 with the environments of qpenv.jl:171-303):
    every contraction an einsum, the two geometric sums numpy.linalg.solve on the explicit regularised transfer matrices."""
    psi = ctx.psi[0]
    n = len(psi)
    q = phi.rows[0]
    AL, AR, AC, C = ([be.download(t) for t in getattr(psi, nm)] for nm in ("AL", "AR", "AC", "CR"))
    O = [np.asarray(ctx.O[0][c].blocks[(0, 0)]) for c in range(n)]
    GL = [env_host(be, ctx.GL[0][c]) for c in range(n)]          # [w, below, above]
    GR = [env_host(be, ctx.GR[0][c]) for c in range(n)]          # [w, above, below]
    VL = [be.download(v) for v in q.VLs]
    lam = [np.sum(AC[c] * proj_host(GL[c], AC[c], O[c], GR[c])) for c in range(n)]
    ren = [1.0 / l for l in lam]
    el, er = np.exp(-1j * p), np.exp(1j * p)
    Cn = C[n - 1]
    lvecL = np.einsum("wba,ac->wbc", GL[0], Cn)                   # left fixed point of T(AR, O, AL)      :261-262
    rvecL = np.einsum("wab,cb->wac", GR[n - 1], Cn)               # its right fixed point                 :259-260
    rvecR = np.einsum("ac,wcb->wab", Cn, GR[n - 1])               # right fixed point of T(AL, O, AR)     :266-267
    lvecR = np.einsum("bc,wba->wca", Cn, GL[0])                   # its left fixed point (bra leg with C)
    shape = GL[0].shape
    dim = int(np.prod(shape))

    def cell_left(v):
        for c in range(n):
            v = tl_host(v, O[c], AR[c], AL[c])
        return v - np.einsum("wba,wab->", v, rvecL) * lvecL

    def cell_right(v):
        for c in range(n - 1, -1, -1):
            v = tr_host(v, O[c], AL[c], AR[c])
        return v - np.einsum("wab,wba->", v, lvecR) * rvecR

    def matrix(f, shp):
        cols = []
        for k in range(int(np.prod(shp))):
            e = np.zeros(int(np.prod(shp)))
            e[k] = 1.0
            cols.append(f(e.reshape(shp)).reshape(-1))
        return np.array(cols).T

    ML, MR = matrix(cell_left, shape), matrix(cell_right, GR[n - 1].shape)
    prod = np.prod(ren)
    N = q.N
    out = np.zeros((N, N), dtype=complex)
    for j in range(N):
        x = np.zeros(N)
        x[j] = 1.0
        Bs = [(VL[c] @ x[q.offs[c]:q.offs[c + 1]].reshape(q.xshapes[c], order="F")).reshape(AL[c].shape, order="F")
              for c in range(n)]
        lBs, rBs = [None] * n, [None] * n
        cur = np.zeros(shape, dtype=complex)
        for c in range(n):
            cur = (tl_host(cur, O[c], AR[c], AL[c]) + tl_host(GL[c], O[c], Bs[c], AL[c])) * ren[c] * el
            lBs[c] = cur
        cur = np.zeros(GR[n - 1].shape, dtype=complex)
        for c in range(n - 1, -1, -1):
            cur = (tr_host(cur, O[c], AL[c], AR[c]) + tr_host(GR[c], O[c], Bs[c], AR[c])) * ren[c] * er
            rBs[c] = cur
        lBs[n - 1] = np.linalg.solve(np.eye(dim) - el ** n * prod * ML, lBs[n - 1].reshape(-1)).reshape(shape)
        rBs[0] = np.linalg.solve(np.eye(dim) - er ** n * prod * MR, rBs[0].reshape(-1)).reshape(GR[n - 1].shape)
        cur = lBs[n - 1]
        for c in range(n - 1):
            cur = tl_host(cur, O[c], AR[c], AL[c]) * ren[c] * el
            lBs[c] = lBs[c] + cur
        cur = rBs[0]
        for c in range(n - 1, 0, -1):
            cur = tr_host(cur, O[c], AL[c], AR[c]) * ren[c] * er
            rBs[c] = rBs[c] + cur
        col = np.zeros(N, dtype=complex)
        for c in range(n):
            T = (proj_host(GL[c], Bs[c], O[c], GR[c]) + proj_host(lBs[(c - 1) % n], AR[c], O[c], GR[c])
                 + proj_host(GL[c], AL[c], O[c], rBs[(c + 1) % n])) / lam[c]
            Dl, d, Dr = T.shape
            col[q.offs[c]:q.offs[c + 1]] = (VL[c].T @ T.reshape((Dl * d, Dr), order="F")).reshape(-1, order="F")
        out[:, j] = col
    return out


@pytest.fixture(scope="module", params=[1, 2], ids=["n1", "n2"])
def setup(request):
    n = request.param
    be = DenseCpuBackend()
    O = mk.classical_ising(BETA).repeat(n)
    psi = mk.InfiniteMPS.random(2, D, np.random.default_rng(3), n=n, be=be)
    psi, envs, eps = mk.leading_boundary(psi, O, mk.VUMPS(tol=1e-11, maxiter=300, verbosity=0))
    assert eps <= 1e-10
    alg = mk.QuasiparticleAnsatz()
    ctx = qpm._StatmechContext(mk.MPSMultiline(psi), [envs], alg, False)
    assert not ctx.fused
    return be, O, psi, envs, alg, ctx


def product_matrix(be, ctx, phi):
    N = phi.N
    M = np.zeros((N, N), dtype=complex)
    for j in range(N):
        x = np.zeros(2 * N)
        x[j] = 1.0
        y = be.download(qpm._statmech_heff(ctx, phi, be.upload(x), be.empty(2 * N)))
        M[:, j] = y[:N] + 1j * y[N:]
    return M


@pytest.mark.parametrize("p", [0.0, 0.7, math.pi])
def test_effective_operator_matches_dense_restatement(setup, p):
    """the composed effective operator on every basis vector against the restatement: 1e-10 relative to the norm of the
    matrix (the project's agreement level for energies; the GMRES solves run at solver_tol = 1e-12)."""
    be, O, psi, envs, alg, ctx = setup
    rng = np.random.default_rng(11)
    q = mk.LeftGaugedQP.random(psi, p, rng)
    phi = qpm.MultilineQP([mk.LeftGaugedQP(psi, q.VLs, q.xshapes, p, be.upload(rng.random(2 * q.N)), 2)], p)
    got, ref = product_matrix(be, ctx, phi), dense_heff(be, ctx, phi, p)
    # complex-linear: the image of i e_j is i times the image of e_j
    x = np.zeros(2 * phi.N)
    x[phi.N + 1] = 1.0
    y = be.download(qpm._statmech_heff(ctx, phi, be.upload(x), be.empty(2 * phi.N)))
    assert np.abs((y[:phi.N] + 1j * y[phi.N:]) - 1j * got[:, 1]).max() <= 1e-12 * np.linalg.norm(got)
    err = np.linalg.norm(got - ref) / np.linalg.norm(ref)
    print("n", len(psi), "p", p, "N", phi.N, "relative error", err, "cond", np.linalg.cond(ref))
    assert err <= 1e-10
    # the solver's leading eigenvalue is that of the same matrix, to the solver's tol
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        E, states = mk.excitations(O, alg, p, psi, envs)
    ev = np.linalg.eigvals(ref)
    lead = ev[np.argmax(np.abs(ev))]
    print("leading", E[0], lead)
    assert abs(abs(E[0]) - abs(lead)) <= alg.tol and min(abs(E[0] - lead), abs(E[0] - np.conj(lead))) <= 10 * alg.tol
    assert isinstance(states[0], mk.LeftGaugedQP) and states[0].nparts == 2


ARNOLDI_SEED = 248


def test_planar_arnoldi_against_numpy():
    """eigsolve_lm_planar on a random real non-symmetric 40 x 40 matrix acting on planar complex vectors: the three
    largest-magnitude eigenvalues against numpy.linalg.eigvals.  The seed is one whose top three magnitudes are separated
    by more than 1 % (asserted), so their order is well defined.  Bound 1e-8: the residuals are below tol = 1e-10 and
    the eigenvalue condition numbers of such a matrix are of order 10 (asserted below 100)."""
    be = DenseCpuBackend()
    rng = np.random.default_rng(ARNOLDI_SEED)
    A = rng.standard_normal((40, 40))
    ev, S = np.linalg.eig(A)
    order = np.argsort(-np.abs(ev))
    top = ev[order][:4]
    mags = np.abs(top)
    assert np.all(mags[:3] / mags[1:4] > 1.01), mags
    Sinv = np.linalg.inv(S)
    conds = [np.linalg.norm(S[:, k]) * np.linalg.norm(Sinv[k, :]) for k in order[:3]]
    assert max(conds) < 100, conds

    def matvec(x, out):
        v = be.download(x)
        return be._set(out, np.concatenate([A @ v[:40], A @ v[40:]]))

    x0 = be.upload(rng.standard_normal(80))
    vals, vecs, res, conv = krylov.eigsolve_lm_planar(be, matvec, x0, num=3, tol=1e-10, krylovdim=30, maxiter=200)
    print("arnoldi", vals, top[:3], res, conv)
    assert conv == 3
    assert np.abs(vals - top[:3]).max() <= 1e-8
    for lam, v in zip(vals, vecs):
        z = be.download(v)
        z = z[:40] + 1j * z[40:]
        assert np.linalg.norm(A @ z - lam * z) <= 1e-8 * np.linalg.norm(A)


def test_domain_walls_and_types_are_refused(setup):
    be, O, psi, envs, alg, ctx = setup
    other = mk.InfiniteMPS.random(2, D, np.random.default_rng(9), n=len(psi), be=be)
    with pytest.raises(NotImplementedError, match="phase ambiguity"):
        mk.excitations(O, alg, 0.0, psi, envs, other)
    with pytest.raises(TypeError):
        mk.excitations(mk.MPOMultiline(O), alg, 0.0, psi, envs)
