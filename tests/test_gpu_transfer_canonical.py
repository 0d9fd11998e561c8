"""Canonical environment transfers (mpsk_transfer_left_ex / mpsk_transfer_right_ex with MPSK_TRANSFER_CANONICAL) on the
environments and isometries of real canonical chains: same result as the dense three-stage route of the same library to
1e-10 (relative max norm, the bar of test_gpu_hac_canonical for mode 3), the identity level written exactly, every
ineligible case the dense route bit for bit, workspace sized on a fresh ctx, the debug check, and whole sweeps."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BAR = 1e-10


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def slabs(t):
    """device environment (W, Db, Dk) -> host array [w, bra, ket]"""
    W, Db, Dk = t.shape
    return t.buf[: t.size].cpu().numpy().reshape(W, Dk, Db).transpose(0, 2, 1).copy()


def _model(name, be):
    import mpskit_jl_amd as mk
    return {"heis": (lambda: mk.heisenberg_XXX(0.5, be=be), 2),
            "tfi": (lambda: mk.transverse_field_ising(1.0, 0.7, be=be), 2),
            "hubbard": (lambda: mk.hubbard(1.0, 4.0, be=be), 4)}[name]


def _chain(be, name, L, D, seed):
    """a random canonical chain with all of its left and right environments built"""
    import mpskit_jl_amd as mk
    mg, d = _model(name, be)
    H = mg()
    psi = mk.FiniteMPS.random(L, d, D, np.random.default_rng(seed), normalize=True, be=be)
    envs = mk.FinEnv(psi, H)
    envs.leftenv(L - 1, psi)
    envs.rightenv(0, psi)
    return H, psi, envs


def _left_cases(H, psi, envs):
    return [(H[j], envs.leftenvs[j], psi.AL(j)) for j in range(len(psi) - 1)]


def _right_cases(H, psi, envs):
    return [(H[j], envs.rightenvs[j + 1], psi.AR(j)) for j in range(len(psi) - 1, 0, -1)]


def _check_side(be, cases, left, want_bulk):
    shapes = set()
    for Hs, G, A in cases:
        Dl, d, Dr = A.shape
        f = be.transfer_left if left else be.transfer_right
        yc = slabs(f(Hs, G, A, A, canonical=True))
        yd = slabs(f(Hs, G, A, A))
        n = Dr if left else Dl
        assert yc.shape == yd.shape == (Hs.Wr if left else Hs.Wl, n, n)
        e = relerr(yc, yd)
        print(f"{'left' if left else 'right'} W={yc.shape[0]} Dl={Dl} d={d} Dr={Dr}: rel. max-norm error {e:.3e}")
        assert e <= BAR, (Dl, Dr, e)
        lvl = 0 if left else yc.shape[0] - 1
        assert np.array_equal(yc[lvl], np.eye(n)), (Dl, Dr)          # written, not computed
        shapes.add(Dl == Dr)
    assert shapes == ({True, False} if want_bulk else {False}), shapes


@pytest.mark.parametrize("name,L,D", [("heis", 14, 64), ("heis", 18, 256), ("tfi", 14, 40), ("hubbard", 8, 32)])
def test_canonical_matches_dense_on_canonical_chain(be, name, L, D):
    """bulk shapes (Dl == Dr = D) and every chain-edge shape (Dl != Dr) of the chain, left and right; Heisenberg (W = 5),
    transverse-field Ising (W = 3) and Hubbard (W = 6, d = 4)"""
    H, psi, envs = _chain(be, name, L, D, seed=7)
    lc, rc = _left_cases(H, psi, envs), _right_cases(H, psi, envs)
    assert any(A.shape[0] == A.shape[2] == D for _, _, A in lc) and any(A.shape[0] == A.shape[2] == D for _, _, A in rc)
    _check_side(be, lc, True, True)
    _check_side(be, rc, False, True)


def test_every_edge_shape_of_a_short_chain(be):
    """L = 8, D = 64: the bond dimensions 1, 2, 4, 8, 16, 8, 4, 2, 1 never reach D, so every site has Dl != Dr"""
    H, psi, envs = _chain(be, "heis", 8, 64, seed=5)
    lc, rc = _left_cases(H, psi, envs), _right_cases(H, psi, envs)
    assert all(A.shape[0] != A.shape[2] for _, _, A in lc + rc)
    _check_side(be, lc, True, False)
    _check_side(be, rc, False, False)


def _raw(be, side, H, W, d, Dl, Dr, Dlb, Drb, G, A, Ab, out, flags=None):
    """the C entry points themselves (Backend.transfer_left sends complex operands to the plain entry)"""
    from mpskit_jl_amd._lib import check
    h = H.handle if H is not None else None
    if side == "l":
        if flags is None:
            check(be.lib.mpsk_transfer_left(be.ctx, h, W, d, Dl, Dr, Dlb, Drb, G.ptr, A.ptr, Ab.ptr, out.ptr), "left")
        else:
            check(be.lib.mpsk_transfer_left_ex(be.ctx, h, W, d, Dl, Dr, Dlb, Drb, G.ptr, A.ptr, Ab.ptr, flags, out.ptr), "left_ex")
    else:
        if flags is None:
            check(be.lib.mpsk_transfer_right(be.ctx, h, W, d, Dl, Dr, Dlb, Drb, A.ptr, Ab.ptr, G.ptr, out.ptr), "right")
        else:
            check(be.lib.mpsk_transfer_right_ex(be.ctx, h, W, d, Dl, Dr, Dlb, Drb, A.ptr, Ab.ptr, G.ptr, flags, out.ptr), "right_ex")
    return out.buf[: out.size].cpu().numpy().copy()


def test_ineligible_inputs_take_the_dense_route_bit_for_bit(be):
    import mpskit_jl_amd as mk
    rng = np.random.default_rng(5)
    D, d = 48, 2
    eye_env = lambda chis, lvl: be.upload_env([np.stack([np.eye(D)] * c, axis=1) if i == lvl else rng.standard_normal((D, c, D))
                                              for i, c in enumerate(chis)])
    A = be.upload(rng.standard_normal((D, d, D)))
    A2 = be.copy(A)                                                   # same values, another pointer
    Sz = np.diag([0.5, -0.5])[None, :, :, None]
    heis = mk.heisenberg_XXX(0.5, be=be)[0]
    ablk = be.mposlice(4, 2, [1, 1, 1, 1], [1, 1, 1, 1],
                       {(0, 0): 1.0, (3, 3): 1.0, (0, 1): Sz, (1, 2): Sz, (2, 3): Sz, (0, 3): Sz})      # A block (1, 2)
    Od = rng.standard_normal((5, 2, 2, 5))
    dense = be.mposlice_dense(Od)
    for side in ("l", "r"):
        lvl = lambda W: 0 if side == "l" else W - 1
        cases = [("flag not set", heis, 5, A, A, 0),
                 ("A != Ab", heis, 5, A, A2, 1),
                 ("A blocks", ablk, 4, A, A, 1),
                 ("dense-MPO slice", dense, 5, A, A, 1),
                 ("H == NULL", None, 3, A, A, 1)]
        for what, H, W, a, ab, flags in cases:
            G = eye_env([1] * W, lvl(W))
            y0 = _raw(be, side, H, W, d, D, D, D, D, G, a, ab, be.zeros(W, D, D))
            y1 = _raw(be, side, H, W, d, D, D, D, D, G, a, ab, be.zeros(W, D, D), flags=flags)
            assert np.array_equal(y0, y1), (side, what)
        # the eligible call of the same inputs does take the other route (the written level is exact there only)
        G = eye_env([1] * 5, lvl(5))
        y0 = _raw(be, side, heis, 5, d, D, D, D, D, G, A, A, be.zeros(5, D, D))
        y1 = _raw(be, side, heis, 5, d, D, D, D, D, G, A, A, be.zeros(5, D, D), flags=1)
        assert not np.array_equal(y0, y1)
        # complex slice: complex operands, the plain complex route with or without the flag
        Z = np.array([[1.0, 0], [0, -1]], dtype=complex)[None, :, :, None]
        sc = be.mposlice(3, 2, [1, 1, 1], [1, 1, 1], {(0, 0): 1.0, (2, 2): 1.0, (0, 1): 1j * Z, (1, 2): Z}, cplx=True)
        crand = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
        Gc = be.upload_env_c([crand(D, 1, D) for _ in range(3)])
        Ac = be.upload_c(crand(D, d, D))
        y0 = _raw(be, side, sc, 3, d, D, D, D, D, Gc, Ac, Ac, be.zeros(3, 2 * D, D))
        y1 = _raw(be, side, sc, 3, d, D, D, D, D, Gc, Ac, Ac, be.zeros(3, 2 * D, D), flags=1)
        assert np.array_equal(y0, y1), (side, "complex slice")
    # unknown flags are refused
    with pytest.raises(Exception, match="unknown flags"):
        _raw(be, "l", heis, 5, d, D, D, D, D, eye_env([1] * 5, 0), A, A, be.zeros(5, D, D), flags=2)


@pytest.mark.parametrize("side", ["l", "r"])
def test_fresh_ctx_first_call_is_the_largest_canonical_transfer(be, side):
    """workspace regression: the first workspace user of a new ctx is a canonical transfer at D = 256 (fold + W-1 slabs)"""
    import mpskit_jl_amd as mk
    H, psi, envs = _chain(be, "heis", 18, 256, seed=7)
    cases = _left_cases(H, psi, envs) if side == "l" else _right_cases(H, psi, envs)
    _, G, A = next(c for c in cases if c[2].shape[0] == c[2].shape[2] == 256)
    f = be.transfer_left if side == "l" else be.transfer_right
    j = next(j for j in range(len(psi)) if (psi.AL(j) if side == "l" else psi.AR(j)) is A)
    ref = slabs(f(H[j], G, A, A))
    be.synchronize()
    b2 = mk.Backend(0)
    try:
        H2 = mk.heisenberg_XXX(0.5, be=b2)
        f2 = b2.transfer_left if side == "l" else b2.transfer_right
        y = slabs(f2(H2[j], G, A, A, canonical=True))
        assert relerr(y, ref) <= BAR, relerr(y, ref)
        assert np.array_equal(y[0 if side == "l" else 4], np.eye(256))
        # and a larger inner shape afterwards grows it: d = 4, W = 6
        Hh, ph, eh = _chain(b2, "hubbard", 8, 64, seed=1)
        for Hs, Gh, Ah in (_left_cases(Hh, ph, eh) if side == "l" else _right_cases(Hh, ph, eh)):
            yc, yd = slabs(f2(Hs, Gh, Ah, Ah, canonical=True)), slabs(f2(Hs, Gh, Ah, Ah))
            assert relerr(yc, yd) <= BAR
    finally:
        b2.close()


def test_check_rejects_broken_promises(be, monkeypatch):
    H, psi, envs = _chain(be, "heis", 8, 16, seed=2)
    j = 4
    GL, AL = envs.leftenvs[j], psi.AL(j)
    GR, AR = envs.rightenvs[j + 1], psi.AR(j)
    monkeypatch.setenv("MPSK_HAC_CHECK", "1")
    be.transfer_left(H[j], GL, AL, AL, canonical=True)                # the chain's own: accepted
    be.transfer_right(H[j], GR, AR, AR, canonical=True)
    bad = be.download_env(GL, [1] * 5)
    bad[0][1, 0, 1] += 1e-6                                           # level 0 no longer the identity
    GLb = be.upload_env(bad)
    with pytest.raises(Exception, match="not canonical"):
        be.transfer_left(H[j], GLb, AL, AL, canonical=True)
    bad = be.download_env(GR, [1] * 5)
    bad[4][1, 0, 1] += 1e-6                                           # level W-1 no longer the identity
    GRb = be.upload_env(bad)
    with pytest.raises(Exception, match="not canonical"):
        be.transfer_right(H[j], GRb, AR, AR, canonical=True)
    a = be.download(AL).copy()
    a[0, 0, 0] += 1e-6                                                # A no longer an isometry
    ALb = be.upload(a)
    with pytest.raises(Exception, match="not canonical"):
        be.transfer_left(H[j], GL, ALb, ALb, canonical=True)
    be.transfer_left(H[j], GLb, AL, AL)                               # the dense route does not care
    monkeypatch.delenv("MPSK_HAC_CHECK")
    be.transfer_left(H[j], GLb, AL, AL, canonical=True)               # unchecked: the caller's promise is taken as given


def test_dmrg_sweeps_with_canonical_transfers(be, monkeypatch):
    """Fixed-budget DMRG sweeps: FinEnv asks for the canonical route at every update (under MPSK_HAC_CHECK=1 every promise
    is verified at every call) and reaches the energy of MPSK_TRANSFER_MODE=0 with the same number of transfers."""
    import mpskit_jl_amd as mk
    from mpskit_jl_amd import algorithms as alg, krylov

    def run(mode):
        asked = []
        with monkeypatch.context() as mp:
            if mode is not None:
                mp.setenv("MPSK_TRANSFER_MODE", mode)
            else:
                mp.setenv("MPSK_HAC_CHECK", "1")
            for nm in ("mpsk_transfer_left_ex", "mpsk_transfer_right_ex"):
                orig = getattr(be.lib, nm)

                def spy(*a, _o=orig, _n=nm):
                    asked.append((_n, a[11]))
                    return _o(*a)
                mp.setattr(be.lib, nm, spy)
            mg, d = _model("heis", be)
            H = mg()
            psi = mk.FiniteMPS.random(20, d, 48, np.random.default_rng(9), normalize=True, be=be)
            envs = mk.FinEnv(psi, H)
            eig = mk.Arnoldi(fixed_matvecs=8, krylovdim=8)
            ws = krylov.KrylovWorkspace(be)
            for _ in range(3):
                alg.dmrg_sweep(psi, H, envs, eig, ws)
            E = float(np.sum(alg.expectation_value(psi, H, envs)))
        return E, envs.n_transfers, asked

    ec, nc, ac = run(None)
    ed, nd, ad = run("0")
    print(f"energy canonical {ec:.15f} dense {ed:.15f} rel. diff {abs(ec - ed) / abs(ed):.3e}; transfers {nc} / {nd}")
    assert nc == nd > 0
    assert len(ac) == nc and all(flags == 1 for _, flags in ac), (len(ac), nc)
    assert {n for n, _ in ac} == {"mpsk_transfer_left_ex", "mpsk_transfer_right_ex"}
    assert abs(ec - ed) <= 1e-10 * abs(ed), (ec, ed)
