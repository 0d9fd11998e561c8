"""The device side of propagator / DynamicalDMRG: mpsk_hac_apply_axpby in every mode of the prepared operator, the complex
forms of the Krylov vector protocol (mpsk_vdotc / mpsk_vaxpby_c / mpsk_vorth_step_c / mpsk_vlincomb_c) against NumPy, and
the full-bond case of tests/test_propagator_cpu.py end to end against the dense resolvent.

Tolerances are those of the tests of the real counterparts: the operator parity of tests/test_gpu_ops.py::test_dAC
(RTOL max(Dl, Dr)) and the levels of test_orth_step_every_basis_length."""
import numpy as np
import pytest

import mpskit_jl_amd as mk
from mpskit_jl_amd import krylov
from mpskit_jl_amd.native_cplx import NativeFiniteMPS
from propagator_cases import dense_resolvent, dense_vector, excited_state, model, native_vector, omegas

pytestmark = pytest.mark.gpu

RTOL = 2e-13                        # tests/test_gpu_ops.py
SHAPES = [(16, 16), (24, 40), (65, 33)]
A0, A1 = 1.7 - 0.45j, -0.6 + 1.2j


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def chain(be):
    """a real S = 1 chain in canonical form whose sites 3, 5, 7 have the bonds of SHAPES; its Heisenberg environments"""
    dims = [1, 3, 9, 16, 16, 24, 40, 65, 33, 11, 4, 2, 1]
    rng = np.random.default_rng(21)
    psi = mk.FiniteMPS([rng.standard_normal((dims[i], 3, dims[i + 1])) for i in range(len(dims) - 1)], normalize=True, be=be)
    H = mk.heisenberg_XXX(1.0, be=be)
    envs = mk.FinEnv(psi, H)
    sites = {}
    for pos in (3, 5, 7):
        GL, GR = envs.leftenv(pos, psi), envs.rightenv(pos, psi)
        sites[(GL.shape[2], GR.shape[2])] = (H[pos], GL, GR)
    assert set(sites) == set(SHAPES)
    return sites


def _check_real(be, hac, Dl, Dr, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((Dl, d, Dr))
    dx = be.upload(x)
    y = be.download(hac.apply(dx))
    plain = be.download(hac.apply_axpby(1.0, dx, 0.0))
    assert np.array_equal(plain, y)                                       # a0 = 0, a1 = 1: mpsk_hac_apply exactly
    for a0, a1 in [(A0.real, A1.real), (0.0, A1.real), (A0.real, 1.0), (A0, A1)]:   # imaginary parts are ignored
        got = be.download(hac.apply_axpby(a1, dx, a0))
        want = np.real(a0) * x + np.real(a1) * y
        err = relerr(got, want)
        print(f"apply_axpby mode {hac.info()['mode']} ({Dl}, {Dr}) a0 = {a0} a1 = {a1}: relerr {err:.2e}")
        assert err < RTOL * max(Dl, Dr), (a0, a1, err)


@pytest.mark.parametrize("Dl,Dr", SHAPES)
@pytest.mark.parametrize("mode", [1, 3])
def test_apply_axpby_real_modes(be, chain, Dl, Dr, mode):
    H, GL, GR = chain[(Dl, Dr)]
    hac = be.hac_create_ex(H, GL, GR, canonical=True) if mode == 3 else be.hac_create(H, GL, GR)
    assert hac.info()["mode"] == mode
    _check_real(be, hac, Dl, Dr, 3, 100 * mode + Dl)
    hac.close()


def test_apply_axpby_dense_slice(be):
    Dl, Dr, d, W = 24, 40, 3, 4
    rng = np.random.default_rng(31)
    H = be.mposlice_dense(rng.standard_normal((W, d, d, W)))
    GL = be.upload_env([rng.standard_normal((Dl, W, Dl))])
    GR = be.upload_env([rng.standard_normal((Dr, W, Dr))])
    hac = be.hac_create(H, GL, GR)
    assert hac.info()["mode"] == 4
    _check_real(be, hac, Dl, Dr, d, 32)
    hac.close()


def test_apply_axpby_complex(be):
    Dl, Dr, d = 24, 40, 3
    rng = np.random.default_rng(41)
    Hr = mk.heisenberg_XXX(1.0, be=be)[0]
    blocks = {k: (complex(v) if np.isscalar(v) else np.asarray(v) * np.exp(0.3j * (k[0] + 2 * k[1]))) for k, v in Hr.blocks.items()}
    H = be.mposlice(Hr.odim, d, Hr.chil, Hr.chir, blocks, cplx=True)
    cr = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    GL = be.upload_env_c([cr(Dl, 1, Dl) for _ in range(H.Wl)])
    GR = be.upload_env_c([cr(Dr, 1, Dr) for _ in range(H.Wr)])
    hac = be.hac_create(H, GL, GR)
    assert hac.info()["mode"] == 2
    x = cr(Dl, d, Dr)
    dx = be.upload_c(x)
    y = be.download_c(hac.apply(dx))
    assert np.array_equal(be.download_c(hac.apply_axpby(1.0, dx, 0.0)), y)
    for a0, a1 in [(A0, A1), (0.0, A1), (A0, 1.0), (2.5, -1.0)]:
        got = be.download_c(hac.apply_axpby(a1, dx, a0))
        err = relerr(got, a0 * x + a1 * y)
        print(f"apply_axpby complex ({Dl}, {Dr}) a0 = {a0} a1 = {a1}: relerr {err:.2e}")
        assert err < RTOL * max(Dl, Dr), (a0, a1, err)
    hac.close()


def _up(be, v):
    return be.upload_c(np.asarray(v, dtype=complex).reshape(-1, 1))


def _down(be, t):
    return be.download_c(t).reshape(-1)


@pytest.mark.parametrize("n", [1, 63, 255, 4097])
@pytest.mark.parametrize("k", [1, 5, 32])
def test_complex_vector_kernels(be, n, k):
    rng = np.random.default_rng(1000 * n + k)
    cr = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    X, y = cr(n, k), cr(n)
    dxs, dy = [_up(be, X[:, j]) for j in range(k)], _up(be, y)
    scale = np.linalg.norm(y)
    # conj(x) . y (the bar of the real dot in tests/test_gpu_ops.py)
    got = be.dotc(dxs[0], dy)
    assert abs(got - np.vdot(X[:, 0], y)) < 1e-12 * n
    assert be.dotc(dxs[0], dy) == got                                        # run to run
    # y = alpha x + beta y, also with beta = 0 on an uninitialised target
    z = be.copy(dy)
    be.axpby_c(A0, dxs[0], A1, z)
    assert relerr(_down(be, z), A0 * X[:, 0] + A1 * y) < 1e-14
    z = be.empty(2 * n, 1)
    z.buf.fill_(float("nan"))
    be.axpby_c(A1, dxs[0], 0.0, z)
    assert relerr(_down(be, z), A1 * X[:, 0]) < 1e-14
    # linear combination with complex coefficients
    c = cr(k)
    assert relerr(_down(be, be.lincomb_c(dxs, c)), X @ c) < 1e-13
    # CGS2 + normalise against a basis that is only roughly orthonormal: two rounds of classical Gram-Schmidt in numpy
    if n >= k:
        Q, _ = np.linalg.qr(cr(n, k))
        Xr = Q + 1e-3 * cr(n, k)
    else:
        Q, Xr = None, X
    for basis, exact in ((Xr, False), (Q, True)):
        if basis is None:
            continue
        h1 = basis.conj().T @ y; y1 = y - basis @ h1
        h2 = basis.conj().T @ y1; y2 = y1 - basis @ h2
        db = [_up(be, basis[:, j]) for j in range(k)]
        runs = []
        for _ in range(2):
            w = _up(be, y)
            h, beta = be.orth_step_c(db, w)
            runs.append((h.copy(), beta, _down(be, w)))
        (h, beta, w), (hb, betab, wb) = runs
        assert np.array_equal(h, hb) and beta == betab and np.array_equal(w, wb)      # bit-identical from run to run
        assert np.abs(h - (h1 + h2)).max() < 1e-12 * scale, (n, k)
        assert abs(beta - np.linalg.norm(y2)) < 1e-12 * scale, (n, k)
        if np.linalg.norm(y2) > 1e-8 * scale:
            assert np.abs(w - y2 / np.linalg.norm(y2)).max() < 1e-11, (n, k)
            if exact:                                                                # orthonormal basis: h = V^H y, w orthogonal to V
                assert np.abs(h - basis.conj().T @ y).max() < 1e-12 * scale
                assert np.abs(basis.conj().T @ w).max() < 1e-11, (n, k)


def test_linsolve_on_the_device_uses_the_complex_entry_points(be):
    rng = np.random.default_rng(51)
    n = 40
    M = rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n))
    A = (M + M.conj().T) / np.sqrt(8 * n)
    b, x0 = rng.standard_normal(n) + 1j * rng.standard_normal(n), rng.standard_normal(n) + 1j * rng.standard_normal(n)
    dA = be.upload_c(A)

    def op(x, out):
        return be.gemm_c(dA, x, out=out)
    a0 = -(0.4 + 0.3j)
    x, info = krylov.linsolve(be, op, _up(be, b), _up(be, x0), a0=a0, a1=1.0, tol=1e-12, krylovdim=30, maxiter=100, cplx=True)
    assert info.converged == 1 and np.iscomplexobj(info.hessenberg)
    assert np.abs(_down(be, x) - np.linalg.solve(a0 * np.eye(n) + A, b)).max() <= 1e-10


@pytest.fixture(scope="module")
def full_bond(be):
    return {name: excited_state(be, name, 6, 8, 2) for name in ("tfi", "heisenberg")}


@pytest.mark.parametrize("iw", range(5))
@pytest.mark.parametrize("name", ["tfi", "heisenberg"])
def test_full_bond_dimension_against_the_dense_resolvent(be, full_bond, name, iw):
    ts, E0, Hd = full_bond[name]
    v = dense_vector(ts)
    z = omegas(E0)[iw] + 0.3j
    want = dense_resolvent(Hd, v, z)
    psi0, H = mk.FiniteMPS(ts, be=be), model(name, be)
    gj, _ = mk.propagator(psi0, z, H, mk.DynamicalDMRG(flavour=mk.Jeckelmann(), tol=1e-8))
    gn, init = mk.propagator(psi0, z, H, mk.DynamicalDMRG(flavour=mk.NaiveInvert(), tol=1e-8))
    print(name, f"z = {z:.4f}: dense {want:.12f}  Jeckelmann err {abs(gj - want):.2e}  NaiveInvert err {abs(gn - want):.2e}"
                f"  sweeps {init.sweeps}  GMRES applications per site {init.solver_stats['matvecs'] / init.solver_stats['solves']:.1f}")
    assert isinstance(init, NativeFiniteMPS)
    assert abs(gj - want) <= 1e-8, (gj, want)
    assert abs(gn - want) <= 1e-8, (gn, want)
    assert abs(gj - gn) <= 1e-8, (gj, gn)
    x = np.linalg.solve(z * np.eye(len(v)) - Hd, v.astype(complex))
    assert np.abs(native_vector(init) - x).max() <= 1e-8


def test_spectral_function_example(be):
    """the spectral-function example of the README, executed as printed: -Im G(omega + i eta) / pi over a frequency grid.
    L = 8, D = 16 is the full bond dimension, so the values can be held to the dense resolvent."""
    import os
    import re
    readme = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "README.md")).read()
    block = [b for b in re.findall(r"```python\n(.*?)```", readme, flags=re.S) if "mk.propagator(" in b]
    assert len(block) == 1
    ns = {}
    exec(block[0], ns)
    A, ts, E0 = ns["A"], ns["ts"], ns["E0"]
    from propagator_cases import dense_hamiltonian
    Hd, v = dense_hamiltonian(ns["H"], 8), dense_vector(ts)
    want = [-dense_resolvent(Hd, v, E0 + w + 0.1j).imag / np.pi for w in np.linspace(0.0, 3.0, 7)]
    print("spectral function", A)
    assert len(A) == 7 and all(a > 0 for a in A)
    assert np.abs(np.array(A) - np.array(want)).max() <= 1e-8


# ---- complex Jordan-form operator (MPSK_HAC_CANONICAL_C128) ---------------------------------------------------------------

def _complex_chain(be, spin, dims, seed):
    from mpskit_jl_amd.native_cplx import NativeFinEnv
    rng = np.random.default_rng(seed)
    d = int(2 * spin + 1)
    ts = [rng.standard_normal((dims[i], d, dims[i + 1])) + 1j * rng.standard_normal((dims[i], d, dims[i + 1]))
          for i in range(len(dims) - 1)]
    psi = NativeFiniteMPS(ts, be)
    H = mk.heisenberg_XXX(spin, be=be)
    for pos in range(len(ts)):
        psi.move_center(pos)
        envs = NativeFinEnv(psi, H)
        yield pos, d, envs.opp[pos], envs.GL[pos], envs.GR[pos + 1]


@pytest.mark.parametrize("spin,dims", [(0.5, [1, 2, 4, 8, 16, 8, 4, 2, 1]), (1.0, [1, 3, 9, 24, 40, 24, 9, 3, 1])],
                         ids=["D16", "D24-40"])
def test_complex_mode3_matches_mode2_on_canonical_chain(be, spin, dims):
    """canonical environments of a complex L = 8 chain: apply with MPSK_HAC_CANONICAL_C128 equals apply without it, to the
    bar tests/test_gpu_hac_canonical.py holds the real mode 3 to; mpsk_hac_info says 3"""
    rng = np.random.default_rng(61)
    for pos, d, H, GL, GR in _complex_chain(be, spin, dims, 60):
        Dl, Dr = GL.shape[2], GR.shape[2]
        x = be.upload_c(rng.standard_normal((Dl, d, Dr)) + 1j * rng.standard_normal((Dl, d, Dr)))
        h3, h2 = be.hac_create_ex(H, GL, GR, canonical_c128=True), be.hac_create(H, GL, GR)
        assert h3.info()["mode"] == 3 and h3.info()["combined_slabs"] == 2 * d * d, (pos, h3.info())
        assert h2.info()["mode"] == 2
        assert be.hac_create_ex(H, GL, GR, canonical=True).info()["mode"] == 2       # the real flag keeps its meaning
        y3, y2 = be.download_c(h3.apply(x)), be.download_c(h2.apply(x))
        err = relerr(y3, y2)
        print(f"complex mode 3 site {pos} ({Dl}, {Dr}): relerr vs mode 2 {err:.2e}")
        assert err < RTOL * max(Dl, Dr), (pos, err)
        got = be.download_c(h3.apply_axpby(A1, x, A0))
        assert relerr(got, A0 * be.download_c(x) + A1 * y3) < RTOL * max(Dl, Dr)
        h3.close(); h2.close()


def test_complex_mode3_falls_back_when_GL0_is_not_an_identity(be, monkeypatch):
    monkeypatch.delenv("MPSK_HAC_CHECK", raising=False)
    rng = np.random.default_rng(62)
    pos, d, H, GL, GR = list(_complex_chain(be, 0.5, [1, 2, 4, 8, 16, 8, 4, 2, 1], 63))[4]
    Dl, Dr = GL.shape[2], GR.shape[2]
    bad = be.copy(GL)
    bad.buf[2] += 1e-3                                   # an off-diagonal entry of level 0
    x = be.upload_c(rng.standard_normal((Dl, d, Dr)) + 1j * rng.standard_normal((Dl, d, Dr)))
    h, ref = be.hac_create_ex(H, bad, GR, canonical_c128=True), be.hac_create(H, bad, GR)
    assert h.info()["mode"] == 2
    assert np.array_equal(be.download_c(h.apply(x)), be.download_c(ref.apply(x)))
    monkeypatch.setenv("MPSK_HAC_CHECK", "1")
    with pytest.raises(mk.MpskError):
        be.hac_create_ex(H, bad, GR, canonical_c128=True)
    assert be.hac_create_ex(H, GL, GR, canonical_c128=True).info()["mode"] == 3


def test_naive_invert_flag_on_and_off_agree(be):
    """Heisenberg L = 12, D = 16: the sweeps with the Jordan-form operator and with the general complex one give the same
    value (1e-8) in the same number of sweeps"""
    ts, E0, _ = excited_state(be, "heisenberg", 12, 16, 5, sweeps=4)
    psi0, H = mk.FiniteMPS(ts, be=be), model("heisenberg", be)
    alg = mk.DynamicalDMRG(flavour=mk.NaiveInvert(), tol=1e-8, maxiter=40)
    g_on, i_on = mk.propagator(psi0, E0 + 0.6 + 0.3j, H, alg, canonical=True)
    g_off, i_off = mk.propagator(psi0, E0 + 0.6 + 0.3j, H, alg, canonical=False)
    print("flag on", g_on, i_on.sweeps, "flag off", g_off, i_off.sweeps)
    assert i_on.eps <= 1e-8 and i_off.eps <= 1e-8
    assert abs(g_on - g_off) <= 1e-8
    assert i_on.sweeps == i_off.sweeps


def test_complex_start_state_against_the_dense_resolvent(be):
    """a complex psi0 (NativeFiniteMPS) at full bond dimension: a spurious conjugation of psi0 in the overlap environments
    or in the value would show here"""
    rng = np.random.default_rng(71)
    dims = [1, 2, 4, 8, 4, 2, 1]
    ts = [rng.standard_normal((dims[i], 2, dims[i + 1])) + 1j * rng.standard_normal((dims[i], 2, dims[i + 1])) for i in range(6)]
    psi0 = NativeFiniteMPS(ts, be)
    v = native_vector(psi0)
    H = model("heisenberg", be)
    from propagator_cases import dense_hamiltonian
    Hd = dense_hamiltonian(H, 6)
    z = -0.7 + 0.3j
    g, init = mk.native_cplx.propagator(psi0, z, H, mk.DynamicalDMRG(tol=1e-8))
    want = complex(np.vdot(v, np.linalg.solve(z * np.eye(64) - Hd, v)))
    print("complex psi0: dense", want, "err", abs(g - want))
    assert abs(g - want) <= 1e-8
    assert np.abs(native_vector(init) - np.linalg.solve(z * np.eye(64) - Hd, v)).max() <= 1e-8
