"""mpsk_hac_eigsolve_fixed, the whole fixed-budget solve of a site update in one library call, against the independent
longdouble Lanczos of tests/eigsolve_cases.py (self-checked in tests/test_eigsolve_cases_cpu.py).

Every case calls hac.eigsolve_fixed(x0, m, vecs, scal, out, first_image) on a hac_create / hac_create_ex handle whose
mode is forced and asserted; the m + 2 work vectors, `out` and `first_image` are NaN-filled and `scal` holds a sentinel
beforehand.  Checked: the Ritz vector within B = max(4 e_host, 64 u) |H_eff|_2 / gap of y_ref, its norm, its sign and its
Rayleigh quotient (also non-increasing over the budgets of one operator); the orthonormality of V[0..m) and each V[k]
inside the reference Krylov space of dimension k + 1; the projected matrix and the betas read back from `scal` in the
documented layout, lambda and m_eff of the info block, the sentinel in every word the call does not own; first_image
inside the componentwise bound of dAC, and the same bits of y without it; x0 bit for bit; the two breakdown kinds;
the chain-edge sites, directly and through the clamp of krylov.eigsolve_sr; the three routes of eigsolve_sr; the
rejection of a sharded operator.  The two near-eigenvector starts (kind "near" of eigsolve_cases, m = 32) are what pins
the second pass of the long CGS2 kernels: without it y is more than 300 B off and the basis is not orthonormal.

Modes that ran: 0 (slab mix), 1 (rc form), 3 (Jordan form, one and two launches), 4 (dense-slice GEMM route).
Measured on an MI355X (largest ratio to the bound per check, over all cases):
    Ritz vector |y - y_ref| / B                  0.041   (ragged, mode 1, m = 32)
    Rayleigh quotient / (B |H|)                  0.035   (edge (1, 2, 1), mode 3)
    |V^T V - I| / (64 u sqrt(n))                 0.019   (edge (1, 2, 2), mode 1)
    V[k] outside the reference Krylov space / B_k  0.021 (aligned, mode 1, m = 8)
    projected matrix / (B |H|)                   0.052;  betas 0.017;  lambda of the info block 0.101
    first_image / componentwise bound            0.064   (edge (1, 2, 1), mode 1)
    invariant: |y - e_min|                       2.0 u of the 64 u allowed;  eigvec: y == e_j bitwise in every mode
    near-eigenvector starts, m = 32              y 0.003 B, |V^T V - I| 0.003 of its bound (one Gram-Schmidt pass alone:
                                                 y 340 B and 363 B away, |V^T V - I| 1e3 times over its bound)
    host error scale e_host                      3.1e-18 .. 1.4e-16 (so B is its 64 u floor times |H| / gap in every case)
Routes of krylov.eigsolve_sr on the ragged shape, m = 8, 9, 32, modes 3 and 1: each route at most 0.041 B from y_ref;
the one-call route and the orth_step_dev + ritz_dev route gave the SAME BITS in all six cases (y and first_image), as
krylov.py states.  The host Ritz route used to leave the sign numpy's eigh happened to give; it now takes the sign of
the device routes (positive component on the start vector).
"""
import contextlib
import os

import numpy as np
import pytest

import eigsolve_cases as ec
from exact_inputs import LD, U

pytestmark = pytest.mark.gpu

SENT = 1234.5
GAUSS = ec.gauss_cases() + ec.edge_cases() + ec.near_cases()


@contextlib.contextmanager
def _forced(mode):
    """the environment that makes mpsk_hac_create(_ex) take `mode` (read when the operator is created)"""
    want = {"MPSK_HAC_MODE": None if mode == 4 else str(mode), "MPSK_DENSE_ROUTE": "1" if mode == 4 else None}
    old = {k: os.environ.get(k) for k in want}
    try:
        for k, v in want.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


def _operator(be, t, mode):
    s = t["s"]
    H = be.mposlice_dense(t["O"]) if mode == 4 else be.mposlice(s.odim, s.d, s.chil, s.chir, dict(s.Os))
    GL, GR = be.upload_env(t["GL"]), be.upload_env(t["GR"])
    with _forced(mode):
        hac = be.hac_create_ex(H, GL, GR, canonical=True) if mode == 3 else be.hac_create(H, GL, GR)
    assert hac.info()["mode"] == mode, (mode, hac.info())
    return hac


def _solve(be, c, first=True):
    """one call on the operands of case c; everything it wrote, downloaded"""
    t = ec.case_operands(c)
    mode, m = c[1], c[2]
    shape = t["x0"].shape
    hac = _operator(be, t, mode)
    nan = np.full(shape, np.nan)
    x0 = be.upload(t["x0"])
    vecs = [be.upload(nan) for _ in range(m + 2)]
    scal = be.upload(np.full(m * (2 * m + 1) + 40, SENT))
    y, f = be.upload(nan), (be.upload(nan) if first else None)
    assert hac.eigsolve_fixed(x0, m, vecs, scal, y, f) is not None
    out = {"V": np.stack([be.download(v).ravel() for v in vecs[:m + 1]]), "scal": be.download(scal), "y": be.download(y).ravel(),
           "first": None if f is None else be.download(f).ravel(), "x0": be.download(x0)}
    hac.close()
    return out


@pytest.fixture(scope="module")
def solve(be):
    """solve(c, first=True): the downloaded outputs of _solve, run once per (case, first) and shared by the tests of this
    module that look at the same solve from different sides (per case, over the budgets, against the krylov routes)"""
    done = {}

    def run(c, first=True):
        if (c, first) not in done:
            done[(c, first)] = _solve(be, c, first)
        return done[(c, first)]
    return run


def _slot(scal, m):
    """(h [m, m] upper triangle = h1 + h2, n2 [m], coef [m], info [3], the words the call does not own)"""
    stride = 2 * m + 1
    h, n2 = np.zeros((m, m)), np.zeros(m)
    free = np.ones(scal.size, dtype=bool)
    for k in range(m):
        kk = k + 1
        blk = scal[k * stride:k * stride + 2 * kk + 1]
        h[:kk, k] = blk[:kk] + blk[kk:2 * kk]
        n2[k] = blk[2 * kk]
        free[k * stride:k * stride + 2 * kk + 1] = False
    r = m * stride
    free[r:r + m] = False
    free[r + 32:r + 35] = False
    return h, n2, scal[r:r + m], scal[r + 32:r + 35], scal[free]


def _rayleigh(t, y):
    y = y.astype(LD)
    return float(y @ t["H"] @ y)


@pytest.mark.parametrize("c", GAUSS, ids=ec.case_id)
def test_solve_against_the_longdouble_lanczos(solve, c):
    t, r = ec.case_operands(c), ec.reference(c)
    m, n = c[2], t["n"]
    B, e_host = ec.bound(c)
    g = solve(c)
    x0 = t["x0"].ravel()
    # ---- the Ritz vector
    y = g["y"]
    err = float(np.abs(y.astype(LD) - r["y"]).max())
    rq = _rayleigh(t, y)
    ratios = {"y": err / B, "rayleigh": abs(rq - r["theta"]) / (B * r["normH"])}
    assert np.isfinite(g["V"]).all() and np.isfinite(y).all()
    # ---- the basis
    V = g["V"].astype(LD)
    orth = float(np.abs(V[:m] @ V[:m].T - np.eye(m)).max())
    ratios["orth"] = orth / (64 * U * np.sqrt(n))
    # (near: basis, projected matrix and betas are conditioned by |H| / beta_0 ~ 1e5 -- see eigsolve_cases -- and any two
    # float64 runs differ by far more than B there; y, theta, the orthonormality and the side outputs are what is held)
    near = c[3] == "near"
    ratios["krylov"] = 0.0 if near else max(ec.projection_residual(g["V"][k], c, k) / ec.basis_bound(c, k) for k in range(m))
    # ---- the projected matrix, the betas and the info block
    h, n2, coef, info, free = _slot(g["scal"], m)
    sg = np.sign(np.einsum("kn,nk->k", V[:m], r["Q"]).astype(np.float64))
    Tref = r["T"].astype(np.float64) * np.outer(sg, sg)
    slack = B * r["normH"]
    ratios["T"] = 0.0 if near else float(np.abs(np.triu(h - Tref)).max()) / slack
    ratios["beta"] = 0.0 if near else float(np.abs(np.sqrt(np.maximum(n2, 0.0)) - r["betas"].astype(np.float64)).max()) / slack
    ratios["lambda"] = abs(info[0] - r["theta"]) / slack
    # ---- first_image
    fb = ec.first_image_bound(t)
    ferr = np.abs(g["first"].astype(LD) - r["first"])
    ratios["first_image"] = float((ferr[fb > 0] / fb[fb > 0]).max())
    print(f"eigsolve {ec.case_id(c)}: e_host = {e_host:.3e}, B = {B:.3e}, err / bound = "
          + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert err <= B, ratios
    assert abs(float(np.sqrt((y.astype(LD) ** 2).sum())) - 1.0) < 1e-13 and y @ x0 > 0
    assert abs(rq - r["theta"]) <= slack, ratios
    assert orth <= 64 * U * np.sqrt(n), ratios
    assert ratios["krylov"] <= 1.0, ratios
    assert ratios["T"] <= 1.0 and ratios["beta"] <= 1.0 and ratios["lambda"] <= 1.0, ratios
    assert info[2] == m, info
    assert np.array_equal(free, np.full(free.size, SENT))
    assert bool((ferr <= fb).all()), ratios
    # ---- the start vector, and the same solve without first_image
    assert np.array_equal(g["x0"], t["x0"])
    g0 = solve(c, first=False)
    assert np.array_equal(g0["y"], y) and np.array_equal(g0["scal"], g["scal"], equal_nan=True)


@pytest.mark.parametrize("shape,mode", [(s, md) for s in ("ragged", "aligned") for md in ec.MODES])
def test_rayleigh_quotient_does_not_increase_with_the_budget(solve, shape, mode):
    """same operator, same x0: the Krylov spaces nest, so theta_1 of budget m' > m is not above that of m"""
    cs = sorted((c for c in ec.gauss_cases() if c[0] == shape and c[1] == mode), key=lambda c: c[2])
    t = ec.case_operands(cs[0])
    rq = [_rayleigh(t, solve(c)["y"]) for c in cs]
    for a, b, c in zip(rq, rq[1:], cs[1:]):
        assert b <= a + ec.bound(c)[0] * t["normH"], (c, a, b)


@pytest.mark.parametrize("mode", ec.MODES)
def test_invariant_subspace_is_cut(solve, mode):
    c = ("ragged", mode, ec.BREAKDOWN_M, "invariant")
    t, m = ec.case_operands(c), ec.BREAKDOWN_M
    g = solve(c)
    h, n2, coef, info, free = _slot(g["scal"], m)
    e = np.zeros(t["n"])
    e[t["support"][0]] = 1.0
    assert np.isfinite(g["V"]).all() and np.isfinite(g["y"]).all() and np.isfinite(g["first"]).all()
    assert np.isfinite(h).all() and np.isfinite(n2).all() and np.isfinite(coef).all() and np.isfinite(info).all()
    assert info[2] == 3, info
    assert not coef[3:].any(), coef
    err = float(np.abs(g["y"] - e).max())
    print(f"eigsolve {ec.case_id(c)}: |y - e_min| = {err / U:.2f} u")
    assert err <= 64 * U
    assert abs(info[0] - t["lam"][t["support"][0]]) <= 64 * U * t["normH"]
    assert np.array_equal(free, np.full(free.size, SENT)) and np.array_equal(g["x0"], t["x0"])


@pytest.mark.parametrize("mode", ec.MODES)
def test_exact_eigenvector_start(solve, mode):
    """x0 = 2 e_j: the first residual is exactly zero, scal_rsqrt_dev_kernel takes its n2 <= 0 branch and the Ritz step
    cuts after one vector"""
    c = ("ragged", mode, ec.BREAKDOWN_M, "eigvec")
    t, m = ec.case_operands(c), ec.BREAKDOWN_M
    g = solve(c)
    h, n2, coef, info, free = _slot(g["scal"], m)
    j = t["support"][1]
    e = np.zeros(t["n"])
    e[j] = 1.0
    assert np.isfinite(g["V"]).all() and np.isfinite(g["y"]).all() and np.isfinite(g["first"]).all()
    assert np.isfinite(h).all() and np.isfinite(n2).all() and np.isfinite(coef).all() and np.isfinite(info).all()
    assert info[2] == 1 and info[0] == t["lam"][j], info
    assert np.array_equal(g["V"][0], e) and not g["V"][1].any()
    assert np.array_equal(g["y"], e)
    assert np.array_equal(g["first"], t["lam"][j] * e)
    assert np.array_equal(free, np.full(free.size, SENT)) and np.array_equal(g["x0"], t["x0"])


def _krylov_operator(be, t, mode):
    import mpskit_jl_amd as mk
    s = t["s"]
    H = be.mposlice(s.odim, s.d, s.chil, s.chir, dict(s.Os))
    return mk.MPO_ddAC(be, H, be.upload_env(t["GL"]), be.upload_env(t["GR"]), canonical=mode == 3)


@pytest.mark.parametrize("shape", ["edge4", "edge2"])
def test_edge_site_through_the_clamp_of_eigsolve_sr(be, shape):
    """fixed_matvecs = 8 on a vector space of dimension 4 (2): m = min(8, x0.size) steps reach the library, and the result
    is the ground vector of the 4 x 4 (2 x 2) H_eff"""
    from mpskit_jl_amd import krylov
    n = int(np.prod(ec.SHAPES[shape]))
    c = (shape, 3, n, "gauss")
    t, r = ec.case_operands(c), ec.reference(c)
    with _forced(3):
        op = _krylov_operator(be, t, 3)
        ws = krylov.KrylovWorkspace(be)
        none, out, nmv, res = krylov.eigsolve_sr(be, op, be.upload(t["x0"]), fixed_matvecs=8, krylovdim=8, values=False, ws=ws)
    assert op._hac.info()["mode"] == 3
    assert none is None and res is None and nmv == n
    assert [k for k in ws.pool if k[0] == "eigscal"] == [("eigscal", (n * (2 * n + 1) + 40, 1))]
    y = be.download(out).ravel()
    ew, S = np.linalg.eigh(t["H"].astype(np.float64))
    v = S[:, 0] * np.sign(S[:, 0] @ t["x0"].ravel())
    B = ec.bound(c)[0]
    print(f"eigsolve clamp {shape}: err / B = {float(np.abs(y - r['y']).max()) / B:.3f}")
    assert float(np.abs(y.astype(LD) - r["y"]).max()) <= B
    assert float(np.abs(y - v).max()) <= B + 64 * U * t["normH"] / (ew[1] - ew[0])


@pytest.mark.parametrize("m", [8, 9, 32])
@pytest.mark.parametrize("mode", [3, 1])
def test_routes_of_eigsolve_sr(be, solve, mode, m):
    """the one-call route, orth_step_dev + ritz_dev and the host Ritz route each stay within B of y_ref; the first two
    run the same kernels in the same order (krylov.py) and give the same bits"""
    from mpskit_jl_amd import krylov
    c = ("ragged", mode, m, "gauss")
    t, r = ec.case_operands(c), ec.reference(c)
    B = ec.bound(c)[0]
    ys, firsts = [], []
    with _forced(mode):
        for route in ("one_call", "orth_step_dev", "host_ritz"):
            op = _krylov_operator(be, t, mode)
            mv = op if route == "one_call" else (lambda x, out=None, op=op: op(x, out=out))
            f = be.upload(np.full(t["x0"].shape, np.nan))
            lam, out, nmv, _ = krylov.eigsolve_sr(be, mv, be.upload(t["x0"]), fixed_matvecs=m, krylovdim=m,
                                                  values=route == "host_ritz", first_image=f)
            assert op._hac.info()["mode"] == mode and nmv == m
            assert (lam is None) == (route != "host_ritz")
            ys.append(be.download(out).ravel())
            firsts.append(be.download(f).ravel())
    errs = [float(np.abs(y.astype(LD) - r["y"]).max()) / B for y in ys]
    print(f"eigsolve routes {ec.case_id(c)}: err / B = {errs}, one-call == orth_step_dev bitwise: {np.array_equal(ys[0], ys[1])}")
    assert max(errs) <= 1.0, errs
    assert abs(lam - r["theta"]) <= B * r["normH"]
    assert np.array_equal(ys[0], ys[1])
    assert np.array_equal(firsts[0], firsts[1]) and np.array_equal(firsts[0], firsts[2])
    assert np.array_equal(ys[0], solve(c)["y"])


def test_sharded_operator_is_rejected(be):
    """Dlo != Dl (one rank's rows of GL): the entry point refuses"""
    t = ec.operands("aligned", "sparse")
    s = t["s"]
    H = be.mposlice(s.odim, s.d, s.chil, s.chir, dict(s.Os))
    hac = be.hac_create(H, be.upload_env([g[:8] for g in t["GL"]]), be.upload_env(t["GR"]))
    m = 2
    vecs = [be.empty(*t["x0"].shape) for _ in range(m + 2)]
    with pytest.raises(Exception, match="square"):
        hac.eigsolve_fixed(be.upload(t["x0"]), m, vecs, be.empty(m * (2 * m + 1) + 40), be.empty(*t["x0"].shape))
    hac.close()
