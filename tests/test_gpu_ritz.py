"""ritz_small_kernel (through mpsk_vritz_dev, on synthesised slot data) against mpmath at 40 digits, and the one-call
mpsk_hac_eigsolve_fixed against the dense eigh of the operator projected on the Krylov basis it returns.

The Ritz bound is measured, not chosen: exact_vector_inputs.RITZ_BOUND = 8 x numpy eigh's own worst error ratio against
mpmath on the same matrices (3.594 u-units; profiles/vector_kernel_bounds.log lists the ratios of numpy and of the
kernel for every case).  Cases: every m = 1..32 at stride 2m + 1 and at stride 70; a cut after step 0, 1, m - 2, m - 1
(beta exactly 0 and 1e-14 max|H|); a twofold-degenerate lowest eigenvalue (value, Rayleigh quotient and residual only);
a start vector without a component on the lowest Ritz vector; H = 0; the matrix scaled by 1e+150 and 1e-150; a zero
diagonal entry next to an off-diagonal of 1e-160 max|H| (theta^2 overflows)."""
import numpy as np
import pytest

import exact_vector_inputs as ev

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(ev.ritz_cases()))
def test_ritz_step(be, name):
    coef, info = ev.run_ritz(be, name)
    out, ratios = ev.check_ritz(name, coef, info, ev.RITZ_BOUND)
    print(f"ritz {name}: {ratios}")
    assert not out, out


@pytest.mark.parametrize("m", [1, 2, 7, 8, 9, 31, 32])
def test_one_call_eigsolve_against_the_projected_operator(be, m):
    """D = 48, d = 2 Heisenberg site, random symmetric environments.  V orthonormal to 1e-13 (the issue's figure);
    first_image = H V[0] and y = the normalised Ritz vector of V^T H V inside Gaussian bounds built from the dense
    operator: a matvec is three nested contractions (extents D, W d, D: gamma_{2 D + W d + 8} |H| |v|, the rule of
    tests/exact_inputs.py), the Ritz coefficients carry RITZ_BOUND u |T| / gap, the assembly gamma_{m+1}."""
    import mpskit_jl_amd as mk
    import mpskit_oracle as mo
    rng = np.random.default_rng(1000 + m)
    D, d, W = 48, 2, 5
    n = D * d * D
    H = mk.heisenberg_XXX(0.5, be=be)
    Ho = mo.heisenberg_mpo(0.5)
    g = rng.standard_normal((W, D, D))
    g = g + np.transpose(g, (0, 2, 1))
    GLh, GRh = [m_[:, None, :] for m_ in g], [m_[:, None, :] for m_ in g[::-1]]
    GL, GR = be.upload_env(GLh), be.upload_env(GRh)
    x0h = rng.standard_normal((D, d, D))
    x0 = be.upload(x0h)
    op = mk.MPO_ddAC(be, H[1], GL, GR)
    vecs = [be.empty(D, d, D) for _ in range(m + 2)]
    scal = be.empty(m * (2 * m + 1) + 40)
    y, first = be.empty(D, d, D), be.empty(D, d, D)
    assert op.eigsolve_fixed(x0, m, vecs, scal, y, first) is not None
    LD = np.longdouble
    V = np.stack([be.download(v).ravel() for v in vecs[:m + 1]]).astype(LD)
    yh, fh = be.download(y).ravel(), be.download(first).ravel()
    # the operator in longdouble through the oracle's contraction, and the same contraction of the absolute values
    GLd, GRd = [a_.astype(LD) for a_ in GLh], [a_.astype(LD) for a_ in GRh]
    Habs = mo.SparseMPOSlice(Ho[1].odim, d, Ho[1].chil, Ho[1].chir, {k_: np.abs(v_) for k_, v_ in Ho[1].Os.items()})

    def apply(v, absolute=False):
        t = np.asarray(v, dtype=LD).reshape(D, d, D)
        if absolute:
            return mo.dAC(np.abs(t), Habs, [np.abs(a_) for a_ in GLd], [np.abs(a_) for a_ in GRd]).ravel()
        return mo.dAC(t, Ho[1], GLd, GRd).ravel()

    G = V @ V.T
    assert float(np.abs(G - np.eye(m + 1)).max()) < 1e-13
    u = ev.U
    gam = (2 * D + W * d + 8) * u
    HV = np.stack([apply(V[k]) for k in range(m)])
    aHV = np.stack([apply(V[k], absolute=True) for k in range(m)])
    out = []
    ev.within(fh, HV[0], gam * aHV[0] + 2 * u * np.abs(HV[0]), "first_image", out)
    T = V[:m] @ HV.T
    T = (T + T.T) / 2
    ew, S = np.linalg.eigh(T.astype(np.float64))
    s = S[:, 0] * (1.0 if S[0, 0] >= 0 else -1.0)
    gap = (ew[1] - ew[0]) if m > 1 else 1.0
    nT = np.linalg.norm(T.astype(np.float64))
    # the device built T from its own dots (error <= 2 gamma_n |V|^T |H v| per entry + the matvec's) before the Ritz step
    dT = float((np.abs(V[:m]) @ (gam * aHV + 2 * ev.n2_factor(n) * np.abs(HV)).T).max()) * m
    ds = (ev.RITZ_BOUND * u * max(nT, 1e-300) + dT) / gap if m > 1 else 4 * u
    ref = s.astype(LD) @ V[:m]
    ref = ref / np.sqrt(ref @ ref)
    bound = (ds * np.sqrt(m) + (m + 4) * u + ev.beta_factor(n)) * (np.abs(V[:m]).sum(axis=0) + np.abs(ref))
    ev.within(yh, ref, bound, "Ritz vector", out)
    assert abs(float(np.sqrt((yh.astype(LD) ** 2).sum())) - 1.0) <= ev.beta_factor(n) + 2 * u
    assert yh @ x0h.ravel() > 0
    assert not out, out
