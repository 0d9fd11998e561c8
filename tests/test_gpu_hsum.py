"""The summed prepared operator of the C ABI (mpsk_hsum_*): y = sum_k c_k H_k x against the host sum of c_k times the dense
contraction (the oracle's dAC).  Every input is a small integer or a dyadic fraction, so every product and every partial
sum is exact in fp64 whatever the summation order: the comparisons are EXACT.  Route 1 (folded, mode 3) on hand-built
canonical environments (identity corners), route 2 (accumulated) on generic ones."""
import numpy as np
import pytest

import mpskit_oracle as mo

pytestmark = pytest.mark.gpu

SHAPES = [(16, 16, 2), (17, 17, 3), (40, 40, 2), (20, 12, 2)]       # (Dl, Dr, d); the last: the two-launch form
COEFS = [1.0, -2.0, 0.5]


def _terms(be, d, n):
    """n (device operator, oracle operator) pairs of physical dimension d with different W and (s, t) patterns: a
    Heisenberg-like W = 5 operator, a TFI-like W = 3 one with an off-diagonal D block and a diagonal W = 3 one.  Integer and
    dyadic entries only (the spin-1 ladder operators carry sqrt(2), so the models are spelled out here)."""
    import mpskit_jl_amd as mk
    A = np.diag(np.linspace(1, -1, d)) if d == 3 else np.diag([1.0, -1.0])
    B = np.diag(np.ones(d - 1), 1)
    C = B.T.copy()
    data = [{(0, 0): 1.0, (4, 4): 1.0, (0, 1): A, (1, 4): A, (0, 2): 0.5 * B, (2, 4): C, (0, 3): 0.5 * C, (3, 4): B},
            {(0, 0): 1.0, (2, 2): 1.0, (0, 1): -A, (1, 2): A, (0, 2): -0.5 * (B + C)},
            {(0, 0): 1.0, (2, 2): 1.0, (0, 1): 2.0 * A, (1, 2): A}]
    return [(mk.MPOHamiltonian(dict(blk), be=be), mo.MPOHamiltonian([mo.mpoham_from_chain(dict(blk), d)])) for blk in data[:n]]


def _ints(rng, shape, cplx):
    a = rng.integers(-3, 4, shape).astype(float)
    return a + 1j * rng.integers(-3, 4, shape) if cplx else a


def _envs(rng, chis, Dl, Dr, cplx, canonical):
    GL = [_ints(rng, (Dl, c, Dl), cplx) for c in chis]
    GR = [_ints(rng, (Dr, c, Dr), cplx) for c in chis]
    if canonical:
        GL[0] = np.eye(Dl)[:, None, :].astype(GL[0].dtype)
        GR[-1] = np.eye(Dr)[:, None, :].astype(GR[-1].dtype)
    return GL, GR


def _dense(Ho, x, GL, GR):
    """the oracle's contraction, term by term over the real and imaginary parts (it is trilinear): exact for integers"""
    if not np.iscomplexobj(x):
        return mo.dAC(x, Ho, GL, GR)
    y = 0
    for gl, cl in ((np.real, 1), (np.imag, 1j)):
        for xx, cx in ((np.real, 1), (np.imag, 1j)):
            for gr, cr in ((np.real, 1), (np.imag, 1j)):
                y = y + cl * cx * cr * mo.dAC(xx(x), Ho, [gl(g) for g in GL], [gr(g) for g in GR])
    return y


def _device_slice(be, Hg, cplx):
    s = Hg[0]
    return be.mposlice(Hg.odim, s.d, s.chil, s.chir, dict(s.blocks), cplx=True) if cplx else s


class _Case:
    def __init__(self, be, Dl, Dr, d, n, cplx, canonical, seed=0):
        rng = np.random.default_rng(1000 * Dl + 10 * n + seed)
        self.be, self.cplx, self.n = be, cplx, n
        terms = _terms(be, d, n)
        self.Ho = [o[0] for _, o in terms]
        self.slices = [_device_slice(be, g, cplx) for g, _ in terms]
        self.envs = [_envs(rng, o.chil, Dl, Dr, cplx, canonical) for o in self.Ho]
        up = be.upload_env_c if cplx else be.upload_env
        self.GL, self.GR = [up(e[0]) for e in self.envs], [up(e[1]) for e in self.envs]
        self.x = _ints(rng, (Dl, d, Dr), cplx)
        self.xd = (be.upload_c if cplx else be.upload)(self.x)
        self.flag = {"canonical_c128": True} if cplx else {"canonical": True}

    def hsum(self, flagged=True):
        return self.be.hsum_create(self.slices, self.GL, self.GR, **(self.flag if flagged else {}))

    def get(self, t):
        return (self.be.download_c if self.cplx else self.be.download)(t)

    def ref(self, coefs):
        return sum(c * _dense(o, self.x, e[0], e[1]) for c, o, e in zip(coefs, self.Ho, self.envs))


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("Dl,Dr,d", SHAPES)
def test_folded_route_is_exact(be, Dl, Dr, d, n, cplx):
    c = _Case(be, Dl, Dr, d, n, cplx, canonical=True)
    h = c.hsum()
    info = h.info()
    assert info["route"] == 1, info
    assert info["launches"] == (2 if (cplx or Dl != Dr) else 1), info          # independent of n
    assert np.array_equal(c.get(h.apply(c.xd)), c.ref([1.0] * n))               # the coefficients start as 1
    h.set_coefs([7.0, 7.0, 7.0][:n])                                            # discarded: a stale fold would show below
    h.set_coefs(COEFS[:n])
    assert np.array_equal(c.get(h.apply(c.xd)), c.ref(COEFS[:n]))
    zc = ([3.0, 0.0, -1.0] if n == 3 else [0.0, 2.0] if n == 2 else [0.0])      # one coefficient 0
    h.set_coefs(zc)
    assert np.array_equal(c.get(h.apply(c.xd)), c.ref(zc))
    h.close()


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("Dl,Dr,d", SHAPES)
def test_accumulated_route_is_exact(be, Dl, Dr, d, n, cplx):
    c = _Case(be, Dl, Dr, d, n, cplx, canonical=False)
    for flagged in (False, True):            # generic environments: route 2 without the flag; with it, F64 trusts the promise
        if flagged and not cplx:
            continue
        h = c.hsum(flagged)
        assert h.info()["route"] == 2, h.info()
        assert np.array_equal(c.get(h.apply(c.xd)), c.ref([1.0] * n))
        h.set_coefs([7.0] * n)
        h.set_coefs(COEFS[:n])
        assert np.array_equal(c.get(h.apply(c.xd)), c.ref(COEFS[:n]))
        zc = ([3.0, 0.0, -1.0] if n == 3 else [0.0, 2.0] if n == 2 else [0.0])
        h.set_coefs(zc)
        assert np.array_equal(c.get(h.apply(c.xd)), c.ref(zc))
        h.close()


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("canonical", [True, False], ids=["route1", "route2"])
def test_single_term_is_hac_apply_bit_for_bit(be, canonical, cplx):
    c = _Case(be, 17, 17, 3, 1, cplx, canonical=canonical)
    rng = np.random.default_rng(3)
    x = rng.standard_normal((17, 3, 17)) + (1j * rng.standard_normal((17, 3, 17)) if cplx else 0)    # generic values
    xd = (be.upload_c if cplx else be.upload)(x)
    flag = c.flag if canonical else {}
    h, a = c.hsum(canonical), be.hac_create_ex(c.slices[0], c.GL[0], c.GR[0], **flag)
    assert h.info()["route"] == (1 if canonical else 2) and (a.info()["mode"] == 3) == canonical
    h.set_coefs([1.0])
    assert np.array_equal(be.download(h.apply(xd)), be.download(a.apply(xd)))


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("canonical", [True, False], ids=["route1", "route2"])
def test_apply_axpby(be, canonical, cplx):
    c = _Case(be, 16, 16, 2, 3, cplx, canonical=canonical)
    h = c.hsum(canonical).set_coefs(COEFS)
    a0, a1 = (2.0 - 1.0j, 0.5 + 2.0j) if cplx else (2.0, -0.5)
    y = c.get(h.apply_axpby(a1, c.xd, a0))
    assert np.array_equal(y, a0 * c.x + a1 * c.ref(COEFS))
    assert np.array_equal(c.get(h.apply_axpby(1.0, c.xd, 0.0)), c.ref(COEFS))


def test_a_block_slice_takes_route2_under_the_flag(be):
    import mpskit_jl_amd as mk
    D = 16
    rng = np.random.default_rng(8)
    Sz = np.diag([0.5, -0.5])[None, :, :, None]
    chis = [1, 1, 1, 1]
    sA = be.mposlice(4, 2, chis, chis, {(0, 0): 1.0, (3, 3): 1.0, (0, 1): Sz, (1, 2): Sz, (2, 3): Sz, (0, 3): Sz})
    Hh = mk.heisenberg_XXX(0.5, be=be)
    can = lambda ch: [be.upload_env(e) for e in _envs(rng, ch, D, D, False, True)]
    (gl1, gr1), (gl2, gr2) = can(chis), can([1] * 5)
    h = be.hsum_create([sA, Hh[0]], [gl1, gl2], [gr1, gr2], canonical=True)
    assert h.info()["route"] == 2, h.info()
    x = be.upload(_ints(rng, (D, 2, D), False))
    ya = be.download(be.hac_create(sA, gl1, gr1).apply(x))
    yh = be.download(be.hac_create(Hh[0], gl2, gr2).apply(x))
    h.set_coefs([2.0, -1.0])
    assert np.array_equal(be.download(h.apply(x)), 2.0 * ya - yh)


def test_error_returns(be, monkeypatch):
    import mpskit_jl_amd as mk
    c = _Case(be, 16, 16, 2, 2, False, canonical=True)
    with pytest.raises(mk.MpskError, match="n <= 8"):
        be.hsum_create(c.slices * 5, c.GL * 5, c.GR * 5, canonical=True)
    import ctypes as C
    h = C.c_void_p()
    empty = (C.c_void_p * 1)()
    rc = be.lib.mpsk_hsum_create(be.ctx, 0, empty, 16, 16, 16, empty, empty, 0, C.byref(h))
    assert rc != 0 and b"n <= 8" in be.lib.mpsk_last_error()
    # mismatched d / dtype
    c3 = _Case(be, 16, 16, 3, 1, False, canonical=True)
    with pytest.raises(mk.MpskError, match="share d and dtype"):
        be.hsum_create([c.slices[0], c3.slices[0]], [c.GL[0], c.GL[0]], [c.GR[0], c.GR[0]])
    cc = _Case(be, 16, 16, 2, 1, True, canonical=True)
    with pytest.raises(mk.MpskError, match="share d and dtype"):
        be.hsum_create([c.slices[0], cc.slices[0]], [c.GL[0], c.GL[0]], [c.GR[0], c.GR[0]])
    # MPSK_HAC_CHECK=1: non-identity corners are refused
    bad = _Case(be, 16, 16, 2, 2, False, canonical=False)
    monkeypatch.setenv("MPSK_HAC_CHECK", "1")
    with pytest.raises(mk.MpskError, match="not canonical"):
        bad.hsum()
    assert c.hsum().info()["route"] == 1


@pytest.mark.parametrize("mode", [0, 1, 4])
def test_accumulated_route_in_every_real_mode(be, monkeypatch, mode):
    """alpha / beta in the last GEMM of each mode of the prepared operator: mix form (0), right-combined form (1) and the
    dense-slice GEMM route (4); complex mode 2 and both mode-3 forms are covered above.  The mode is asserted on a handle
    prepared the same way; the reference is the host combination of the terms' own mpsk_hac_apply (exact on integers)."""
    D, d, n = 16, 2, 3
    rng = np.random.default_rng(40 + mode)
    if mode == 4:
        monkeypatch.setenv("MPSK_DENSE_ROUTE", "1")
        Ws = [3, 2, 4]
        slices = [be.mposlice_dense(rng.integers(-2, 3, (W, d, d, W)).astype(float)) for W in Ws]
        chis = [[1] * W for W in Ws]
    else:
        monkeypatch.setenv("MPSK_HAC_MODE", str(mode))
        slices = [g[0] for g, _ in _terms(be, d, n)]
        chis = [s.chil for s in slices]
    envs = [_envs(rng, ch, D, D, False, False) for ch in chis]
    GL, GR = [be.upload_env(e[0]) for e in envs], [be.upload_env(e[1]) for e in envs]
    x = be.upload(_ints(rng, (D, d, D), False))
    singles = [be.hac_create(s, gl, gr) for s, gl, gr in zip(slices, GL, GR)]
    assert [a.info()["mode"] for a in singles] == [mode] * n
    ys = [be.download(a.apply(x)) for a in singles]
    h = be.hsum_create(slices, GL, GR)
    assert h.info()["route"] == 2
    h.set_coefs(COEFS)
    assert np.array_equal(be.download(h.apply(x)), sum(c * y for c, y in zip(COEFS, ys)))
    if mode != 4:                                         # and against the dense contraction
        Ho = [o[0] for _, o in _terms(be, d, n)]
        ref = sum(c * mo.dAC(be.download(x), o, e[0], e[1]) for c, o, e in zip(COEFS, Ho, envs))
        assert np.array_equal(be.download(h.apply(x)), ref)
