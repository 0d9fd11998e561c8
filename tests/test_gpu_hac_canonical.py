"""The prepared effective Hamiltonian in Jordan form (mpsk_hac_create_ex with MPSK_HAC_CANONICAL, mode 3) on the
environments of real canonical chains: same matvec as the dense operator (mode 1 / oracle), same fixed-budget
eigensolve, and every ineligible case keeps its old mode bit for bit."""
import numpy as np
import pytest

import mpskit_oracle as mo

pytestmark = pytest.mark.gpu

RTOL = 2e-13      # the test_gpu_ops bar: RTOL * D


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def _model(name, be):
    import mpskit_jl_amd as mk
    return {"heis": (lambda: mk.heisenberg_XXX(0.5, be=be), lambda: mo.heisenberg_mpo(0.5), 2),
            "heis1": (lambda: mk.heisenberg_XXX(1.0, be=be), lambda: mo.heisenberg_mpo(1.0), 3),
            "tfi": (lambda: mk.transverse_field_ising(1.0, 0.7, be=be), lambda: mo.tfi_mpo(1.0, 0.7), 2),
            "hubbard": (lambda: mk.hubbard(1.0, 4.0, be=be), lambda: mo.hubbard_mpo(1.0, 4.0), 4)}[name]


def _chain(be, name, L, D, seed):
    import mpskit_jl_amd as mk
    mg, mo_, d = _model(name, be)
    H, Ho = mg(), mo_()
    psi = mk.FiniteMPS.random(L, d, D, np.random.default_rng(seed), normalize=True, be=be)
    return H, Ho[0], psi, mk.FinEnv(psi, H), d


def _y(hac, be, x):
    return be.download(hac.apply(be.upload(x)))


@pytest.mark.parametrize("name,L,D", [("heis", 14, 64), ("heis1", 10, 48), ("tfi", 14, 40), ("hubbard", 8, 32)])
def test_mode3_matches_dense_on_canonical_chain(be, name, L, D):
    H, Ho, psi, envs, d = _chain(be, name, L, D, seed=7)
    rng = np.random.default_rng(11)
    shapes = set()
    for pos in range(L):                     # edges (Dl != Dr: two launches) and bulk (Dl == Dr: one launch)
        GL, GR = envs.leftenv(pos, psi), envs.rightenv(pos, psi)
        Dl, Dr = GL.shape[2], GR.shape[2]
        x = rng.standard_normal((Dl, d, Dr))
        h3 = be.hac_create_ex(H[pos], GL, GR, canonical=True)
        h1 = be.hac_create(H[pos], GL, GR)
        assert h3.info()["mode"] == 3, (pos, h3.info())
        assert h1.info()["mode"] != 3
        y3, y1 = _y(h3, be, x), _y(h1, be, x)
        ref = mo.dAC(x, Ho, be.download_env(GL, Ho.chil), be.download_env(GR, Ho.chir))
        bar = RTOL * max(Dl, Dr)
        assert relerr(y3, y1) < bar, (pos, relerr(y3, y1))
        assert relerr(y3, ref) < bar, (pos, relerr(y3, ref))
        shapes.add(Dl == Dr)
        h3.close(); h1.close()
    assert shapes == {True, False}


def test_mode3_eigsolve_fixed_matches_mode1(be):
    from mpskit_jl_amd.derivatives import MPO_ddAC
    H, _, psi, envs, d = _chain(be, "heis", 14, 64, seed=3)
    for pos in (1, 6):
        GL, GR = envs.leftenv(pos, psi), envs.rightenv(pos, psi)
        x0 = psi.AC(pos)
        n, m = x0.size, 8
        outs = []
        for canonical in (True, False):
            op = MPO_ddAC(be, H[pos], GL, GR, canonical=canonical)
            vecs = [be.empty(*x0.shape) for _ in range(m + 2)]
            scal, out = be.empty(m * (2 * m + 1) + 40), be.empty(*x0.shape)
            first = be.empty(*x0.shape)
            assert op.eigsolve_fixed(x0, m, vecs, scal, out, first) is not None
            assert op._hac.info()["mode"] == (3 if canonical else 1)
            outs.append((be.download(out), be.download(first)))
        (y3, f3), (y1, f1) = outs
        assert relerr(f3, f1) < RTOL * 64
        assert relerr(y3, y1) < 1e-10, relerr(y3, y1)
        assert n == y3.size


def test_ineligible_cases_keep_their_mode_bit_for_bit(be):
    import mpskit_jl_amd as mk
    rng = np.random.default_rng(5)
    D = 48
    # random environments: without the flag the operator is what it was
    Ho = mo.heisenberg_mpo(0.5)[0]
    Hg = mk.heisenberg_XXX(0.5, be=be)[0]
    GL = be.upload_env([rng.standard_normal((D, c, D)) for c in Ho.chil])
    GR = be.upload_env([rng.standard_normal((D, c, D)) for c in Ho.chir])
    x = be.upload(rng.standard_normal((D, 2, D)))
    a, b = be.hac_create(Hg, GL, GR), be.hac_create_ex(Hg, GL, GR, canonical=False)
    assert a.info()["mode"] == b.info()["mode"] == 1
    assert np.array_equal(_y(a, be, be.download(x)), _y(b, be, be.download(x)))
    # Dlo != Dl (a row block of a sharded left environment): no mode 3 even with the flag
    GLr = mk.DTensor(GL.buf[: 5 * 24 * D].clone(), (5, 24, D))
    c = be.hac_create_ex(Hg, GLr, GR, canonical=True)
    assert c.info()["mode"] != 3
    # slices outside the Jordan form: A blocks between the middle levels, chi > 1 on the first level
    Sz = np.diag([0.5, -0.5])[None, :, :, None]
    for odim, chis, blocks in [
            (4, [1, 1, 1, 1], {(0, 0): 1.0, (3, 3): 1.0, (0, 1): Sz, (1, 2): Sz, (2, 3): Sz, (0, 3): Sz}),
            (3, [2, 1, 1], {(0, 0): 1.0, (2, 2): 1.0, (0, 1): np.ones((2, 2, 2, 1)), (1, 2): Sz})]:
        s = be.mposlice(odim, 2, chis, chis, blocks)
        gl = be.upload_env([np.stack([np.eye(D)] * c, axis=1) if i == 0 else rng.standard_normal((D, c, D))
                            for i, c in enumerate(chis)])
        gr = be.upload_env([np.stack([np.eye(D)] * c, axis=1) if i == odim - 1 else rng.standard_normal((D, c, D))
                            for i, c in enumerate(chis)])
        p, q = be.hac_create(s, gl, gr), be.hac_create_ex(s, gl, gr, canonical=True)
        assert q.info()["mode"] == p.info()["mode"] != 3
        assert np.array_equal(_y(p, be, be.download(x)), _y(q, be, be.download(x)))
    # complex slice: mode 2 with or without the flag
    Z = np.array([[1.0, 0], [0, -1]], dtype=complex)[None, :, :, None]
    sc = be.mposlice(3, 2, [1, 1, 1], [1, 1, 1], {(0, 0): 1.0, (2, 2): 1.0, (0, 1): 1j * Z, (1, 2): Z}, cplx=True)
    crand = lambda: rng.standard_normal((D, 1, D)) + 1j * rng.standard_normal((D, 1, D))
    gl, gr = be.upload_env_c([crand() for _ in range(3)]), be.upload_env_c([crand() for _ in range(3)])
    assert be.hac_create_ex(sc, gl, gr, canonical=True).info()["mode"] == 2


def test_check_rejects_non_canonical_environments(be, monkeypatch):
    H, _, psi, envs, d = _chain(be, "heis", 8, 16, seed=2)
    pos = 4
    GL, GR = envs.leftenv(pos, psi), envs.rightenv(pos, psi)
    monkeypatch.setenv("MPSK_HAC_CHECK", "1")
    assert be.hac_create_ex(H[pos], GL, GR, canonical=True).info()["mode"] == 3     # the chain's own: accepted
    bad = be.download(GL).copy()
    bad[0, 0, 0] += 1e-6                                                           # level 0 no longer the identity
    GLb = be.upload(bad)
    with pytest.raises(Exception, match="not canonical"):
        be.hac_create_ex(H[pos], GLb, GR, canonical=True)
    monkeypatch.delenv("MPSK_HAC_CHECK")
    assert be.hac_create_ex(H[pos], GLb, GR, canonical=True).info()["mode"] == 3


def test_dmrg_sweeps_run_through_mode3(be, monkeypatch):
    """Fixed-budget DMRG sweeps on a canonical chain prepare every site operator in mode 3 under MPSK_HAC_CHECK=1 (level 0
    of GL and level W-1 of GR are identities to 1e-10 at every visit) and reach the energy of the dense operator."""
    import mpskit_jl_amd as mk
    from mpskit_jl_amd import algorithms as alg, derivatives, krylov

    def run(hac_mode):
        modes = set()
        with monkeypatch.context() as mp:
            mp.setenv("MPSK_HAC_CHECK", "1")
            if hac_mode:
                mp.setenv("MPSK_HAC_MODE", hac_mode)
            orig = derivatives.MPO_ddAC._prepare

            def spy(self):
                h = orig(self)
                modes.add(h.info()["mode"])
                return h
            mp.setattr(derivatives.MPO_ddAC, "_prepare", spy)
            H, _, psi, envs, _ = _chain(be, "heis", 16, 32, seed=9)
            eig = mk.Arnoldi(fixed_matvecs=8, krylovdim=8)
            ws = krylov.KrylovWorkspace(be)
            for _ in range(3):
                alg.dmrg_sweep(psi, H, envs, eig, ws)
            E = float(np.sum(alg.expectation_value(psi, H, envs)))
        return E, modes

    e3, m3 = run(None)
    e1, m1 = run("1")
    assert m3 == {3} and m1 == {1}, (m3, m1)
    assert abs(e3 - e1) <= 1e-10 * abs(e1), (e3, e1)
