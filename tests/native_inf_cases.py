"""Cases for the uniform states on interleaved complex storage (mpskit_jl_amd.native_cplx.NativeInfiniteMPS, NativePerMPOInfEnv,
the VOMPS approximate) and for mpsk_dC_proj_c.  The bodies take a backend: tests/test_native_inf_cases_cpu.py runs them on the
NumPy stand-in (tests/cpu_backend_inf.py), tests/test_gpu_native_inf.py on the device.

mpsk_dC_proj_c operands are Gaussian integers with |Re|, |Im| <= 3: every partial sum is then an exact double whatever the
bracket order (dc_guard checks that in longdouble), so the device result must be bit-equal to the reference.

The driver cases are checked against dense NumPy restatements below (`vomps_numpy`, `lead_host`), which share no code with
the product.  Tolerances the issue leaves open are MEASURED: the deviation of the real-fp64 route (approximate._approximate_inf)
from the restatement on the same case, floored at the restatement's own rounding resolution, times 10 (`measured_bounds`)."""
import math

import numpy as np

import mpskit_jl_amd as mk
import mpskit_oracle as mo
from mpskit_jl_amd import native_cplx as nc
from mpskit_jl_amd.approximate import _approximate_inf

# (W; Dlo, Dl, Dr, Dro)
DC_SHAPES = [(1, 5, 3, 7, 2), (3, 5, 3, 7, 2), (3, 65, 17, 33, 70), (2, 4, 4, 4, 4)]
U = 2.0 ** -53


def gauss_int(rng, shape):
    return (rng.integers(-3, 4, shape) + 1j * rng.integers(-3, 4, shape)).astype(np.complex128)


def dc_operands(shape, seed=0):
    W, Dlo, Dl, Dr, Dro = shape
    rng = np.random.default_rng(1000 + seed)
    return gauss_int(rng, (W, Dlo, Dl)), gauss_int(rng, (W, Dr, Dro)), gauss_int(rng, (Dl, Dr))


def dc_ref(GL, GR, c):
    """y[p,q] = sum_w GL[w][p,a] c[a,b] GR[w][b,q], nothing conjugated"""
    return np.einsum("wpa,ab,wbq->pq", GL, c, GR, optimize=False)


def dc_guard(GL, GR, c):
    """the same sum in longdouble, real and imaginary parts apart, and the largest |partial sum| bound"""
    ld = np.longdouble
    glr, gli, grr, gri, cr, ci = (x.astype(ld) for x in (GL.real, GL.imag, GR.real, GR.imag, c.real, c.imag))
    tr = np.einsum("wpa,ab->wpb", glr, cr) - np.einsum("wpa,ab->wpb", gli, ci)
    ti = np.einsum("wpa,ab->wpb", glr, ci) + np.einsum("wpa,ab->wpb", gli, cr)
    yr = np.einsum("wpb,wbq->pq", tr, grr) - np.einsum("wpb,wbq->pq", ti, gri)
    yi = np.einsum("wpb,wbq->pq", tr, gri) + np.einsum("wpb,wbq->pq", ti, grr)
    bound = np.einsum("wpa,ab,wbq->pq", np.abs(glr) + np.abs(gli), np.abs(cr) + np.abs(ci), np.abs(grr) + np.abs(gri)).max()
    return yr, yi, float(bound)


def _relayout(G, rows, cols):
    """the slabs of G read with the two dimensions swapped (same memory, column-major), then transposed back in shape"""
    return np.stack([g.ravel(order="F").reshape((cols, rows), order="F").T for g in G])


# wrong contractions a correct reference must tell apart
DC_WRONG = {
    "GR conjugated": lambda GL, GR, c: dc_ref(GL, np.conj(GR), c),
    "GL transposed": lambda GL, GR, c: dc_ref(_relayout(GL, GL.shape[1], GL.shape[2]), GR, c),
    "one level dropped": lambda GL, GR, c: dc_ref(GL[:-1], GR[:-1], c) if GL.shape[0] > 1 else np.zeros((GL.shape[1], GR.shape[2])),
    "Dro and Dr swapped": lambda GL, GR, c: dc_ref(GL, _relayout(GR, GR.shape[1], GR.shape[2]), c),
}


def slabs_c(be, G):
    """[W, rows, cols] complex -> interleaved device slabs (W, 2 rows, cols)"""
    return be.upload_env_c([np.transpose(G, (1, 0, 2))])


def mat_c(be, t):
    """interleaved (2 m, n) device matrix -> complex [m, n]"""
    return be.download_c(t)


# ---- NumPy restatements ----------------------------------------------------------------------------------------------------

def densify(O, site):
    t = np.zeros((O.odim, O.d, O.d, O.odim), dtype=np.complex128)
    for (i, j), v in O.data[site % O.period].items():
        t[i, :, :, j] = v * np.eye(O.d) if np.isscalar(v) else np.asarray(v)[0, :, :, 0]
    return t


def tl_host(gl, o, a, b):
    """gl[w, below, above] -> [v, below', above'] through ket a (above), operator o[w, t, s, v], bra b (below, conjugated)"""
    return np.einsum("wpq,qsj,wtsv,pti->vij", gl, a, o, np.conj(b), optimize=True)


def tr_host(gr, o, a, b):
    """gr[v, above', below'] -> [w, above, below]"""
    return np.einsum("qsj,wtsv,pti,vji->wqp", a, o, np.conj(b), gr, optimize=True)


def _lead(apply, dim):
    n = int(np.prod(dim))
    M = np.array([apply(np.eye(n, dtype=np.complex128)[k].reshape(dim)).reshape(-1) for k in range(n)]).T
    ev, V = np.linalg.eig(M)
    k = int(np.argmax(np.abs(ev)))
    return ev[k], V[:, k].reshape(dim)


def lead_host(As, Bs, Os=None):
    """(leading eigenvalue, transfer-matrix dimension) of the unit-cell transfer with kets As, bras Bs, operators Os, dense"""
    n = len(As)
    W = 1 if Os is None else Os[0].shape[0]
    dim = (W, Bs[0].shape[0], As[0].shape[0])
    eye = lambda i: np.eye(As[i].shape[1])[None, :, :, None]

    def cell(v):
        for i in range(n):
            v = tl_host(v, eye(i) if Os is None else Os[i % len(Os)], As[i], Bs[i])
        return v
    return _lead(cell, dim)[0], int(np.prod(dim))


def product_state(Os, As):
    """the exact O * above at bond W D: B[(w, a), t, (v, b)] = sum_s O[w, t, s, v] A[a, s, b]"""
    out = []
    for o, a in zip(Os, As):
        t = np.einsum("wtsv,asb->watvb", o, a)
        out.append(t.reshape(o.shape[0] * a.shape[0], o.shape[1], o.shape[3] * a.shape[2]))
    return out


def vomps_numpy(below0, Os, above, alg):
    """approximate/vomps.jl restated on dense NumPy: below0 / above = dicts of host tensors (AL, AR, AC, CR), Os dense
    [W, d, d, W] per site; fixed points by a dense eigendecomposition.  Returns (AL list, eps history)."""
    n = len(Os)
    psi = mo.InfiniteMPS(list(below0["AL"]), list(below0["AR"]), list(below0["CR"]), list(below0["AC"]))

    def envs(psi):
        W = Os[0].shape[0]

        def tl(v):
            for i in range(n):
                v = tl_host(v, Os[i], above["AL"][i], psi.AL[i])
            return v

        def tr(v):
            for i in range(n - 1, -1, -1):
                v = tr_host(v, Os[i], above["AR"][i], psi.AR[i])
            return v
        GL, GR = [None] * n, [None] * n
        GL[0] = _lead(tl, (W, psi.AL[0].shape[0], above["AL"][0].shape[0]))[1]
        GR[n - 1] = _lead(tr, (W, above["AR"][n - 1].shape[2], psi.AR[n - 1].shape[2]))[1]
        for i in range(1, n):
            GL[i] = tl_host(GL[i - 1], Os[i - 1], above["AL"][i - 1], psi.AL[i - 1])
        for i in range(n - 2, -1, -1):
            GR[i] = tr_host(GR[i + 1], Os[i + 1], above["AR"][i + 1], psi.AR[i + 1])
        for col in range(n):
            lam = np.einsum("pq,wpa,ab,wbq->", np.conj(psi.CR[col]), GL[(col + 1) % n], above["CR"][col], GR[col])
            GL[(col + 1) % n] = GL[(col + 1) % n] / math.sqrt(abs(lam))
            GR[col] = GR[col] / math.sqrt(abs(lam))
        return GL, GR

    ac_proj = lambda GL, GR, i: np.einsum("wpa,asb,wtsv,vbq->ptq", GL[i], above["AC"][i], Os[i], GR[i], optimize=True)
    c_proj = lambda GL, GR, i: np.einsum("wpa,ab,wbq->pq", GL[(i + 1) % n], above["CR"][i], GR[i], optimize=True)

    def galerkin(psi, GL, GR):
        out = 0.0
        for i in range(n):
            g = ac_proj(GL, GR, i)
            g = g / np.linalg.norm(g)
            al = psi.AL[i].reshape(-1, psi.AL[i].shape[2])
            gm = g.reshape(al.shape[0], -1)
            out = max(out, np.linalg.norm(gm - al @ (al.conj().T @ gm)))
        return out

    GL, GR = envs(psi)
    eps, hist = galerkin(psi, GL, GR), []
    for it in range(1, alg.maxiter + 1):
        newAL = [mo.regauge(ac_proj(GL, GR, i), c_proj(GL, GR, i)) for i in range(n)]
        gtol = mo.updatetol(alg.gauge_tol_min, alg.gauge_tol_max, alg.gauge_tol_factor, it, eps)
        psi = mo.InfiniteMPS.from_AL(newAL, psi.CR[n - 1], tol=gtol)
        GL, GR = envs(psi)
        eps = galerkin(psi, GL, GR)
        hist.append((it, eps))
        if eps <= alg.tol:
            break
    return psi.AL, hist


# ---- case bodies ---------------------------------------------------------------------------------------------------------

def relnorm(x, ref):
    return np.linalg.norm(x - ref) / np.linalg.norm(ref)


def case_gauge(be, n, D, seed, tol=1e-12):
    """the gauge contract of a random state built with gauge tolerance `tol`: AL^dag AL = 1 and AR AR^dag = 1 to 1e-12,
    AL CR = CR AR to tol, |CR| = 1 (relative Frobenius norms); to_host returns complex arrays"""
    rng = np.random.default_rng(seed)
    psi = nc.NativeInfiniteMPS([rng.standard_normal((D, 2, D)) + 1j * rng.standard_normal((D, 2, D)) for _ in range(n)],
                               be=be, tol=tol)
    h = psi.to_host()
    assert all(t.dtype == np.complex128 for k in h for t in h[k])
    worst = 0.0
    for i in range(n):
        al, ar, ac, c, cm = h["AL"][i], h["AR"][i], h["AC"][i], h["CR"][i], h["CR"][(i - 1) % n]
        eye = np.eye(D)
        assert relnorm(np.einsum("asb,asc->bc", al.conj(), al), eye) <= 1e-12
        assert relnorm(np.einsum("asb,csb->ac", ar, ar.conj()), eye) <= 1e-12
        alc = np.einsum("asb,bc->asc", al, c)
        g = relnorm(np.einsum("ab,bsc->asc", cm, ar), alc)
        worst = max(worst, g)
        assert g <= tol, (i, g)
        assert relnorm(ac, alc) <= 1e-13
        assert abs(np.linalg.norm(c) - 1.0) <= 1e-14
    return psi, worst


def case_dot_self(be, n, D, seed):
    psi = nc.NativeInfiniteMPS.random(2, D, np.random.default_rng(seed), n=n, be=be)
    val = mk.dot(psi, psi)
    assert abs(val - 1.0) <= 1e-10, val
    return val


def tfi_time_mpo(be, dt):
    return mk.make_time_mpo(mk.transverse_field_ising(1.0, 0.7, be=be), dt, mk.WII())


PARITY_ALG = dict(tol=1e-9, maxiter=12, env_tol_max=1e-11, gauge_tol_max=1e-13)   # tight inner solves: the histories are comparable


def _host_real(be, psi):
    return {k: [be.download(t).astype(np.complex128) for t in getattr(psi, k)] for k in ("AL", "AR", "AC", "CR")}


def measured_bounds(be, n, log=None):
    """The real-fp64 route on the imaginary-time case (dt = -0.05i, above D = 2, below D = 4) against vomps_numpy from the
    same start.  Returns the case's pieces and the two bounds: 10 x the measured deviation, each floored at the resolution
    of the restatement (a dense eigenvalue of an m x m matrix: m u; a Galerkin norm of D d D numbers: D d D u).
    D_below = 4 = W D_above: the target is representable with a bond matrix of full rank.  (With D_below = 6 two singular
    values of CR vanish at the fixed point, the QR of regauge is then ill-conditioned and the small eps of the later
    iterations scatter by tens of percent between ANY two implementations, the restatement included.)"""
    O = tfi_time_mpo(be, -0.05j)
    assert isinstance(O, mk.SparseMPO) and not O.cplx
    above = mk.InfiniteMPS.random(2, 2, np.random.default_rng(21), n=n, be=be)
    below = mk.InfiniteMPS.random(2, 4, np.random.default_rng(22), n=n, be=be)
    alg = mk.VOMPS(**PARITY_ALG)
    phi, envs, eps = _approximate_inf(below, (O, above), alg)
    Os = [densify(O, s) for s in range(n)]
    AL_np, hist_np = vomps_numpy(_host_real(be, below), Os, _host_real(be, above), alg)
    AL_real = [be.download(t).astype(np.complex128) for t in phi.AL]
    lam, m = lead_host(AL_np, AL_real)
    dev_dot = abs(abs(lam) - 1.0)
    hist = envs.history
    assert len(hist) == len(hist_np), (hist, hist_np)
    dev_eps = max(abs(a[1] - b[1]) for a, b in zip(hist, hist_np))
    b_dot = 10 * max(dev_dot, m * U)
    b_eps = 10 * max(dev_eps, 4 * 2 * 4 * U)
    if log is not None:
        log(f"imaginary-time parity, unit cell {n}: real route vs NumPy restatement: | |dot| - 1 | = {dev_dot:.3e}, "
            f"max |d eps| = {dev_eps:.3e} over {len(hist)} iterations; bounds (10x, floored) dot {b_dot:.3e}, eps {b_eps:.3e}")
    return dict(O=O, above=above, below=below, alg=alg, phi=phi, hist=hist, AL_real=AL_real, b_dot=b_dot, b_eps=b_eps)


def case_imag_parity(be, n, log=None, device=None):
    """dt = -0.05i with the operator forced to complex storage: the same state as the real route from the same start
    (|dot| per unit cell = 1) and the same eps history, to the measured bounds"""
    r = measured_bounds(be, n, log)
    Oc = nc.as_complex_mpo(r["O"])
    assert Oc.cplx and Oc is not r["O"]
    above, below = nc.NativeInfiniteMPS.from_real(r["above"]), nc.NativeInfiniteMPS.from_real(r["below"])
    phi, envs, eps = nc.approximate(below, (Oc, above), r["alg"], device=device)
    assert isinstance(phi, nc.NativeInfiniteMPS) and isinstance(envs, nc.NativePerMPOInfEnv)
    W = Oc.odim                                         # left slabs [D_below, D_above], right slabs [D_above, D_below]
    assert envs.lw[0].shape == (W, 8, 2) and envs.rw[0].shape == (W, 4, 4), (envs.lw[0].shape, envs.rw[0].shape)
    hist = envs.history
    assert eps == hist[-1][1] and len(hist) == len(r["hist"]), (hist, r["hist"])
    lam, _ = lead_host(r["AL_real"], phi.to_host()["AL"])
    d_dot = abs(abs(lam) - 1.0)
    d_eps = max(abs(a[1] - b[1]) for a, b in zip(hist, r["hist"]))
    via_mk = mk.dot(phi, nc.NativeInfiniteMPS.from_real(r["phi"]))
    if log is not None:
        log(f"imaginary-time parity, unit cell {n}: interleaved route vs real route: | |dot| - 1 | = {d_dot:.3e}, "
            f"max |d eps| = {d_eps:.3e}; native_cplx.dot gives | |dot| - 1 | = {abs(abs(via_mk) - 1.0):.3e}")
    assert d_dot <= r["b_dot"], (d_dot, r["b_dot"])
    assert abs(abs(via_mk) - 1.0) <= r["b_dot"], (via_mk, r["b_dot"])
    assert d_eps <= r["b_eps"], (d_eps, r["b_eps"], hist, r["hist"])
    return r


def case_real_time(be, n, b_dot, log=None, device=None):
    """dt = 0.05, TFI g = 0.7, above D = 2, below D = 6 = W D: eps <= 1e-9 within maxiter, and |<phi| O above>| per cell equals
    the norm per cell of the exact product state (NumPy, bond W D) to the measured bound"""
    O = tfi_time_mpo(be, 0.05)
    assert O.cplx
    above = nc.NativeInfiniteMPS.from_real(mk.InfiniteMPS.random(2, 2, np.random.default_rng(21), n=n, be=be))
    below = nc.NativeInfiniteMPS.random(2, 6, np.random.default_rng(23), n=n, be=be)
    alg = mk.VOMPS(tol=1e-9, maxiter=30)
    if device is None:
        phi, envs, eps = mk.approximate(below, (O, above), alg)          # the package-level entry dispatches the new state
    else:
        phi, envs, eps = nc.approximate(below, (O, above), alg, device=device)
    assert eps <= 1e-9 and len(envs.history) <= 30, envs.history
    B = product_state([densify(O, s) for s in range(n)], above.to_host()["AL"])
    nrm2, _ = lead_host(B, B)
    ov, _ = lead_host(B, phi.to_host()["AL"])
    norm = math.sqrt(abs(nrm2))
    if log is not None:
        log(f"real time, unit cell {n}: eps {eps:.3e} after {len(envs.history)} iterations; |<phi|O above>| = {abs(ov):.15f}, "
            f"|O above| = {norm:.15f}, difference {abs(abs(ov) - norm):.3e} (bound {b_dot:.3e})")
    assert abs(abs(ov) - norm) <= b_dot * max(norm, 1.0), (abs(ov), norm, b_dot)
    return phi, envs
