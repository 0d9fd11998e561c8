"""Inputs and references for the fixed-budget eigensolve mpsk_hac_eigsolve_fixed (tests/test_gpu_eigsolve_fixed.py); the
self-checks of this module are in tests/test_eigsolve_cases_cpu.py.  NumPy only.

A case is (shape, mode, m, kind).  Its operands -- an MPO slice, GL, GR and the start vector x0 -- depend on (shape, mode,
kind) only, so the solves of one operator at growing m share x0 and their Krylov spaces nest.  GL and GR are symmetric
per level and every block of the slice is symmetric in its physical indices, which makes

    H_eff[(p,t,q), (a,s,b)] = sum_{w,v} GL[w][p,a] O[w,t,s,v] GR[v][b,q]           (exact_proj_inputs.contract("dAC"))

symmetric.  It is formed densely in np.longdouble by ONE plain einsum(optimize=False); vectors are the C-order ravel of the
logical [Dl, d, Dr] tensor on the host (dots and norms do not depend on the order).

reference(case)   m-step Lanczos in longdouble, full re-orthogonalisation applied twice, T = Q^T H Q; eigh of T in
                  float64 (T is at most 32 x 32: the eigenvector error of that step is u |T| / gap, inside the bound).
host_f64(case)    the recurrence as the device runs it, in plain float64 NumPy: CGS2 with h = h1 + h2, beta =
                  sqrt(max(n2, 0)), scaling by 0 if n2 <= 0, the cut at beta <= 1e-13 max|H|, eigh of the symmetrised
                  square part, sign by component 0.  A second reference, not the code under test: it sets the SIZE of
                  the allowed error,
                      B = max(4 e_host, 64 u) |H_eff|_2 / gap ,   e_host = |host_f64 - y_ref|_max gap / |H_eff|_2
                  (the device may be four times further from the longdouble reference than a plain float64 run of the
                  same recurrence, because it sums in another order; 64 u is the floor where the host run is exact).
wrong(case, how)  plausible wrong solves on the same operands: the largest Ritz vector, m - 1 steps, a start vector that
                  is not normalised, projected columns read with stride 2m, and h1 alone (no second Gram-Schmidt pass)
                  at m = 32.  Each differs from y_ref by more than 100 B on every case it applies to (asserted on the
                  CPU).  From a Gaussian start one pass of classical Gram-Schmidt stays orthogonal to rounding at these
                  sizes (dropping the second moves y by under 1e-2 B), so h1 alone is held against the kind "near"
                  below, where it is 340 B and 360 B away.

Shapes (Dl, d, Dr): ragged (9, 2, 14), n = 252; aligned (16, 2, 16), n = 512; the chain-edge sites (1, 2, 2), n = 4 and
(1, 2, 1), n = 2, where the budget is the whole space (m = n).  Budgets on the two full shapes: 1, 2, 8, 9, 16, 17, 24,
25, 32 (the MD = 8 boundary of vec_cgs2 and the three instances of its long kernels).

Modes.  All four fp64 modes mpsk_hac_info can report for a square operator are reachable at these shapes:
  0  slab mix          sparse slice, MPSK_HAC_MODE=0
  1  rc form           the same slice, MPSK_HAC_MODE=1
  3  Jordan form       Jordan-form slice, canonical environments (GL[0] = GR[W-1] = 1), hac_create_ex(canonical=True)
                       with MPSK_HAC_MODE=3
  4  dense-slice GEMM  one dense tensor [4, 2, 2, 4] through mpsk_mposlice_create_dense, MPSK_DENSE_ROUTE=1
The full list of budgets runs on mode 3 at the ragged shape (two launches per matvec, the benchmark's operator) and on
mode 1 at the aligned shape; every other (shape, mode) runs m = 8, 9, 32.  The edge shapes run modes 3 and 1.

Kinds.  gauss: Gaussian operands.  invariant / eigvec: integer operands with H_eff diagonal (diagonal integer
environments, scalar blocks = identity physical operators, on a three-level Jordan-form slice with canonical environments,
which every mode accepts: MPSK_DENSE_ROUTE=1 takes its dense form through mode 4).  invariant: x0 = e_i + 2 e_j + 2 e_k on
three distinct eigenvalues, m = 8: the Krylov space closes after three steps.  eigvec: x0 = 2 e_j, so |x0|, V[0], H V[0]
and h1 are exact and the first residual is exactly zero.  near: the Gaussian operator with x0 = its ground vector +
1e-7 x Gaussian noise, the start a converged sweep gives, at m = 32 on the full-list mode of each shape.  The first
residual is 1e-5 |H x|, so one Gram-Schmidt pass leaves V[1] with a component u |H x| / |r| along V[0]: this is the kind
that needs the second pass of the long kernels.  The same factor |H| / beta_0 ~ 1e5 conditions the basis and the
projected matrix themselves: the float64 transcription is already 90 to 3000 B |H| away from the reference T and betas
(any two float64 evaluations differ that much), so for this kind only y, its Rayleigh quotient, lambda, m_eff, the
orthonormality of V and the side outputs are compared, not T, the betas or the Krylov-space residuals.  One step fewer
and an unnormalised start (|x0| = 1 + 1e-12) move a converged solve by less than 100 B; they do not apply to it."""
from __future__ import annotations

import functools

import numpy as np

import exact_inputs as ei
from exact_inputs import LD, U

SHAPES = {"ragged": (9, 2, 14), "aligned": (16, 2, 16), "edge4": (1, 2, 2), "edge2": (1, 2, 1)}
CHIS = {"ragged": (1, 3, 2, 1), "aligned": (1, 1, 1, 1, 1), "edge4": (1, 3, 2, 1), "edge2": (1, 3, 2, 1)}
M_FULL = (1, 2, 8, 9, 16, 17, 24, 25, 32)
M_SHORT = (8, 9, 32)
MODES = (0, 1, 3, 4)
FULL_MODE = {"ragged": 3, "aligned": 1}
EDGE_MODES = (3, 1)
FAMILY = {0: "sparse", 1: "sparse", 3: "jordan", 4: "dense"}
DENSE_W = 4
BREAKDOWN_M = 8
NEAR_NOISE = 1e-7
CUT = 1e-13
WRONG = ("largest", "m_minus_1", "unnormalised_start", "stride_2m", "h1_only")
GAP_MIN = 1e-3          # (theta_2 - theta_1) / |H_eff|_2 of every Gaussian case, in the reference alone (asserted on the CPU)

_e = functools.partial(np.einsum, optimize=False)


def gauss_cases():
    out = []
    for shape in ("ragged", "aligned"):
        for mode in MODES:
            out += [(shape, mode, m, "gauss") for m in (M_FULL if mode == FULL_MODE[shape] else M_SHORT)]
    return out


def edge_cases():
    return [(shape, mode, int(np.prod(SHAPES[shape])), "gauss") for shape in ("edge4", "edge2") for mode in EDGE_MODES]


def breakdown_cases():
    return [("ragged", mode, BREAKDOWN_M, kind) for kind in ("invariant", "eigvec") for mode in MODES]


def near_cases():
    """the start a converged sweep gives: x0 = ground vector of H_eff + NEAR_NOISE x Gaussian, at the long budget"""
    return [(shape, FULL_MODE[shape], 32, "near") for shape in ("ragged", "aligned")]


def cases():
    return gauss_cases() + edge_cases() + near_cases() + breakdown_cases()


def case_id(c):
    return f"{c[0]}-mode{c[1]}-m{c[2]}-{c[3]}"


# ------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------
def _sym_ts(b):
    return (b + np.transpose(b, (0, 2, 1, 3))) / 2


def _sym_env(rng, D, chis, ident=None):
    """[D, chi, D] per level, every slab symmetric; level `ident` (chi = 1) the identity"""
    out = []
    for i, c in enumerate(chis):
        g = ei.gauss_array(rng, D, c, D)
        g = (g + np.transpose(g, (2, 1, 0))) / 2
        if i == ident:
            g = np.eye(D)[:, None, :].copy()
        out.append(g)
    return out


def _diag_env(rng, D, chis, ident):
    out = []
    for i, c in enumerate(chis):
        g = np.zeros((D, c, D))
        for k in range(c):
            g[:, k, :] = np.diag(np.ones(D) if i == ident else ei.int_array(rng, D))
        out.append(g)
    return out


@functools.lru_cache(maxsize=None)
def operands(shape, family, kind="gauss"):
    """{"s": oracle slice, "O": dense [Wl, d, d, Wr], "chis", "GL", "GR": lists of [D, chi, D], "x0": [Dl, d, Dr],
    "H": H_eff [n, n] in longdouble, "Habs": the same contraction of the absolute values, "normH": |H_eff|_2}; built
    once, shared, never modified.  family: "sparse" / "jordan" / "dense" (gauss), "diag" (invariant, eigvec)."""
    import mpskit_oracle as mo
    Dl, d, Dr = SHAPES[shape]
    name = f"eigsolve-{shape}-{family}-{'diag' if family == 'diag' else 'gauss'}"          # near: the operator of gauss
    rng = ei._rng(name)
    t = {"name": name, "shape": shape, "family": family, "dense": family == "dense"}
    if family == "diag":
        chis = (1, 1, 1)
        s = mo.SparseMPOSlice(3, d, list(chis), list(chis), {(0, 0): 1.0, (2, 2): 1.0, (0, 1): 2.0, (1, 2): 3.0, (0, 2): -1.0})
        GL, GR = _diag_env(rng, Dl, chis, 0), _diag_env(rng, Dr, chis, 2)
    elif family == "sparse":
        chis = CHIS[shape]
        r = ei.rand_slice(rng, len(chis), d, chis, ei.gauss_array)
        s = mo.SparseMPOSlice(r.odim, d, list(chis), list(chis), {k: v if np.isscalar(v) else _sym_ts(v) for k, v in r.Os.items()})
        GL, GR = _sym_env(rng, Dl, chis), _sym_env(rng, Dr, chis)
    elif family == "jordan":
        chis = CHIS[shape]
        W = len(chis)
        blocks = {(0, 0): 1.0, (W - 1, W - 1): 1.0, (0, W - 1): _sym_ts(ei.gauss_array(rng, 1, d, d, 1))}
        for w in range(1, W - 1):
            blocks[(0, w)] = _sym_ts(ei.gauss_array(rng, 1, d, d, chis[w]))
            blocks[(w, W - 1)] = _sym_ts(ei.gauss_array(rng, chis[w], d, d, 1))
        s = mo.SparseMPOSlice(W, d, list(chis), list(chis), blocks)
        GL, GR = _sym_env(rng, Dl, chis, 0), _sym_env(rng, Dr, chis, W - 1)
    elif family == "dense":
        chis = (DENSE_W,)
        s = mo.SparseMPOSlice(1, d, [DENSE_W], [DENSE_W], {(0, 0): _sym_ts(ei.gauss_array(rng, DENSE_W, d, d, DENSE_W))})
        GL, GR = _sym_env(rng, Dl, chis), _sym_env(rng, Dr, chis)
    else:
        raise KeyError(family)
    O = np.asarray(s.full(), dtype=np.float64)
    G, R = ei._stack(GL), ei._stack(GR)
    n = Dl * d * Dr
    H = _e("pwa,wtsv,bvq->ptqasb", ei._hp(G), ei._hp(O), ei._hp(R)).reshape(n, n)
    Habs = _e("pwa,wtsv,bvq->ptqasb", ei._abs_hp(G), ei._abs_hp(O), ei._abs_hp(R)).reshape(n, n)
    assert float(np.abs(H - H.T).max()) <= 4 * U * float(np.abs(Habs).max()), name
    H = (H + H.T) / 2
    t.update(s=s, O=O, chis=list(chis), GL=GL, GR=GR, G=G, R=R, H=H, Habs=Habs, n=n,
             normH=float(np.abs(np.linalg.eigvalsh(H.astype(np.float64))).max()))
    if family == "diag":
        lam = np.diag(H).astype(np.float64)
        assert not np.any(H - np.diag(np.diag(H))) and np.array_equal(lam, np.round(lam)), name
        order = np.argsort(lam, kind="stable")
        i, j, k = int(order[0]), int(order[n // 2]), int(order[-1])
        # (H_eff does not depend on t: every eigenvalue is at least twofold, the space of x0 holds one vector of each)
        assert lam[i] < lam[j] < lam[k] and lam[j] != 0, (name, lam[[i, j, k]])
        t.update(lam=lam, support=(i, j, k))
        x = np.zeros(n)
        if kind == "invariant":
            x[[i, j, k]] = (1.0, 2.0, 2.0)
        else:
            x[j] = 2.0
        t["x0"] = x.reshape(Dl, d, Dr)
    elif kind == "near":
        ground = np.linalg.eigh(H.astype(np.float64))[1][:, 0]
        t["x0"] = (ground + NEAR_NOISE * ei.gauss_array(ei._rng(name + "-near"), n)).reshape(Dl, d, Dr)
    else:
        t["x0"] = ei.gauss_array(rng, Dl, d, Dr)
    for v in t.values():
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return t


def case_operands(case):
    shape, mode, _, kind = case
    return operands(shape, FAMILY[mode] if kind in ("gauss", "near") else "diag", kind)


def first_image_bound(t):
    """componentwise bound of H_eff x0 / |x0| as the project holds dAC to (exact_proj_inputs): (depth + 2 stages + 2) u
    times the contraction of the absolute values, depth the largest over the bracket orders of the four modes, plus one
    rounding for the normalisation of x0"""
    Dl, d, Dr = t["x0"].shape
    Wl, _, _, Wr = t["O"].shape
    depth = max(Dl + Wl * d + Dr * Wr, Wr + Dl + Wl * d * Dr, Wl + Wr + d * (Dl + Dr))
    x = np.abs(t["x0"]).astype(LD).ravel()
    return (depth + 2 * 3 + 2 + 1) * LD(U) * (t["Habs"] @ (x / np.sqrt(x @ x)))


# ------------------------------------------------------------------------------------------------------------------
# the longdouble reference
# ------------------------------------------------------------------------------------------------------------------
def _cut(T, betas, m):
    """effective dimension: the first k with beta_k <= 1e-13 max|H| over the square part ends the space after k + 1"""
    scale = max(float(np.abs(T).max()), 1e-300)
    for k in range(m):
        if betas[k] <= CUT * scale:
            return k + 1
    return m


def _ritz(T, col=0):
    ev, S = np.linalg.eigh(np.asarray((T + T.T) / 2, dtype=np.float64))
    s = S[:, col]
    return ev, s * (1.0 if s[0] >= 0 else -1.0)


@functools.lru_cache(maxsize=None)
def reference(case):
    """{"Q": [n, m_eff], "T": Q^T H Q, "betas": [m], "theta": theta_1, "y": y_ref (|y| = 1, y . x0 > 0), "gap": theta_2 -
    theta_1 (|H_eff|_2 where the space is one-dimensional), "normH", "first": H_eff x0 / |x0|, "m_eff"}"""
    t = case_operands(case)
    m = case[2]
    H, n = t["H"], t["n"]
    x0 = t["x0"].astype(LD).ravel()
    q = x0 / np.sqrt(x0 @ x0)
    first = H @ q
    Q = np.zeros((n, m), dtype=LD)
    betas = np.zeros(m, dtype=LD)
    for k in range(m):
        Q[:, k] = q
        w = H @ q
        for _ in range(2):
            w = w - Q[:, :k + 1] @ (Q[:, :k + 1].T @ w)
        betas[k] = np.sqrt(w @ w)
        q = w / betas[k] if betas[k] > 0 else w * 0
    T = Q.T @ H @ Q
    T = (T + T.T) / 2
    me = _cut(T[:m, :m].astype(np.float64), betas.astype(np.float64), m)
    Q, T = Q[:, :me], T[:me, :me]
    ev, s = _ritz(T)
    y = Q @ s.astype(LD)
    y = y / np.sqrt(y @ y)
    if y @ x0 < 0:
        y = -y
    out = {"Q": Q, "T": T, "betas": betas, "theta": float(ev[0]), "y": y, "m_eff": me, "normH": t["normH"], "first": first,
           "gap": float(ev[1] - ev[0]) if me > 1 else t["normH"]}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------------------
# the recurrence as the device runs it, in float64
# ------------------------------------------------------------------------------------------------------------------
def _device_recurrence(t, m, normalise=True, passes=2):
    """V [m + 1, n] and the slot of mpsk_hac_eigsolve_fixed: block k at k (2m + 1) holds h1[0..k], h2[0..k], |r|^2"""
    H = t["H"].astype(np.float64)
    x0 = t["x0"].astype(np.float64).ravel()
    stride = 2 * m + 1
    V = np.zeros((m + 1, t["n"]))
    slot = np.zeros(m * stride)
    n2 = x0 @ x0
    V[0] = x0 * ((1.0 / np.sqrt(n2)) if n2 > 0 else 0.0) if normalise else x0
    for k in range(m):
        kk = k + 1
        w = H @ V[k]
        h1 = V[:kk] @ w
        w = w - h1 @ V[:kk]
        h2 = V[:kk] @ w if passes == 2 else np.zeros(kk)
        if passes == 2:
            w = w - h2 @ V[:kk]
        n2 = w @ w
        slot[k * stride:k * stride + 2 * kk + 1] = np.concatenate([h1, h2, [n2]])
        V[k + 1] = w * ((1.0 / np.sqrt(n2)) if n2 > 0 else 0.0)
    return V, slot


def _device_ritz(slot, m, stride, largest=False):
    """ritz_small_kernel in NumPy: (coef [m], lambda, m_eff)"""
    A, beta = np.zeros((m, m)), np.zeros(m)
    for k in range(m):
        kk = k + 1
        blk = slot[k * stride:]
        A[:kk, k] = blk[:kk] + blk[kk:2 * kk]
        beta[k] = np.sqrt(max(blk[2 * kk], 0.0))
    scale = max(np.abs(A).max(), np.abs(beta[:m - 1]).max(initial=0.0), 1e-300)
    me = m
    for k in range(m):
        if beta[k] <= CUT * scale:
            me = k + 1
            break
    A = A[:me, :me].copy()
    for k in range(me - 1):
        A[k + 1, k] = beta[k]
    ev, s = _ritz(A, -1 if largest else 0)
    coef = np.zeros(m)
    coef[:me] = s
    return coef, float(ev[-1 if largest else 0]), me


def _assemble(V, coef, m):
    y = coef @ V[:m]
    n2 = y @ y
    return y * ((1.0 / np.sqrt(n2)) if n2 > 0 else 0.0)


@functools.lru_cache(maxsize=None)
def host_f64(case):
    """{"V": [m + 1, n], "slot", "coef", "lam", "m_eff", "y"} of the float64 transcription"""
    t = case_operands(case)
    m = case[2]
    V, slot = _device_recurrence(t, m)
    coef, lam, me = _device_ritz(slot, m, 2 * m + 1)
    out = {"V": V, "slot": slot, "coef": coef, "lam": lam, "m_eff": me, "y": _assemble(V, coef, m)}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


def bound(case):
    """(B, e_host): B = max(4 e_host, 64 u) |H_eff|_2 / gap"""
    r, h = reference(case), host_f64(case)
    cond = r["normH"] / r["gap"]
    e_host = float(np.abs(h["y"].astype(LD) - r["y"]).max()) / cond
    return max(4 * e_host, 64 * U) * cond, e_host


def _residual(v, Q):
    v = np.asarray(v, dtype=LD)
    return v - Q @ (Q.T @ v)


def basis_bound(case, k):
    """B_k, built like B from the host run: 4 x the projection residual of the host's V[k] against Q[:, :k + 1], with the
    same floor"""
    r, h = reference(case), host_f64(case)
    res = float(np.abs(_residual(h["V"][k], r["Q"][:, :k + 1])).max())
    return max(4 * res, 64 * U * r["normH"] / r["gap"])


def projection_residual(v, case, k):
    return float(np.abs(_residual(v, reference(case)["Q"][:, :k + 1])).max())


# ------------------------------------------------------------------------------------------------------------------
# plausible wrong solves
# ------------------------------------------------------------------------------------------------------------------
def wrong(case, how):
    """the Ritz vector of a solve with one plausible mistake, on the operands of `case`; None where the mistake does not
    apply: nothing changes at m = 1; h1_only needs the near-eigenvector start at m = 32; a converged solve (near) does
    not notice one step fewer or the norm 1 + 1e-12 of its start"""
    t = case_operands(case)
    m, near = case[2], case[3] == "near"
    stride = 2 * m + 1
    if (how == "h1_only") != near and how in ("h1_only", "m_minus_1", "unnormalised_start"):
        return None
    if how == "h1_only":
        if m != 32:
            return None
        V, slot = _device_recurrence(t, m, passes=1)
        return _assemble(V, _device_ritz(slot, m, stride)[0], m)
    if m == 1:
        return None
    if how == "m_minus_1":
        V, slot = _device_recurrence(t, m - 1)
        return _assemble(V, _device_ritz(slot, m - 1, 2 * m - 1)[0], m - 1)
    if how == "unnormalised_start":
        V, slot = _device_recurrence(t, m, normalise=False)
        return _assemble(V, _device_ritz(slot, m, stride)[0], m)
    V, slot = _device_recurrence(t, m)
    if how == "largest":
        return _assemble(V, _device_ritz(slot, m, stride, largest=True)[0], m)
    if how == "stride_2m":
        return _assemble(V, _device_ritz(np.concatenate([slot, np.zeros(stride)]), m, 2 * m)[0], m)
    raise KeyError(how)
