"""Pair-Gram form of the canonical transfers, restated in numpy and held against the oracle's transfer_left /
transfer_right on canonical chains (bar 1e-10 relative max norm, the bar of tests/test_gpu_transfer_canonical.py), and the
pair / coefficient tables and the route model of the library (mpsk_transfer_pair_model: host only, runs without a GPU)
against the same restatement.

    GLout[v] = sum_{t,s} O[0,t,s,v] P_ts,      P_ts = A[:,t,:]^T A[:,s,:],   P_st = P_ts^T      0 < v < W-1, D block of W-1
    GRout[w] = sum_{t,s} O[w,t,s,W-1] Q_st,    Q_st = A[:,s,:] A[:,t,:]^T,   Q_ts = Q_st^T      0 < w < W-1
"""
import ctypes as C

import numpy as np
import pytest

import mpskit_oracle as mo

BAR = 1e-10

MODELS = {"heis": (lambda: mo.heisenberg_mpo(0.5), 2), "heis1": (lambda: mo.heisenberg_mpo(1.0), 3),
          "tfi": (lambda: mo.tfi_mpo(1.0, 0.7), 2), "hubbard": (lambda: mo.hubbard_mpo(1.0, 4.0), 4)}


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def pair_plan(O, left):
    """the unordered pairs {i, j} with a coefficient on some output level (symmetric ones first) and coef[l][p] =
    (direct, transposed); levels: left v = 1 .. W-2 (and W-1 when the slice has a D block), right w = 1 .. W-2"""
    Wl, d, _, Wr = O.shape
    if left:
        lv = list(range(1, Wr - 1)) + ([Wr - 1] if np.any(O[0, :, :, Wr - 1]) else [])
        c = lambda l, i, j: O[0, i, j, lv[l]]
    else:
        lv = list(range(1, Wl - 1))
        c = lambda l, i, j: O[lv[l], j, i, Wr - 1]
    used = lambda i, j: any(c(l, i, j) != 0 or c(l, j, i) != 0 for l in range(len(lv)))
    pairs = [(i, i) for i in range(d) if used(i, i)] + [(i, j) for i in range(d) for j in range(i + 1, d) if used(i, j)]
    coef = np.array([[(c(l, i, j), 0.0 if i == j else c(l, j, i)) for (i, j) in pairs] for l in range(len(lv))]).reshape(len(lv), len(pairs), 2)
    return pairs, lv, coef


def pairgram_levels(O, A, left):
    """{level: matrix} from the pair products alone; a symmetric product is read through its upper triangle"""
    pairs, lv, coef = pair_plan(O, left)
    M = []
    for i, j in pairs:
        m = A[:, i, :].T @ A[:, j, :] if left else A[:, i, :] @ A[:, j, :].T
        M.append(np.triu(m) + np.triu(m, 1).T if i == j else m)
    return {v: sum(coef[l, p, 0] * M[p] + coef[l, p, 1] * M[p].T for p in range(len(pairs))) for l, v in enumerate(lv)}


def canonical_chain(name, L, D, seed):
    mg, d = MODELS[name]
    H = mg()
    psi = mo.FiniteMPS.random(L, d, D, np.random.default_rng(seed))
    envs = mo.FinEnv(psi, H)
    envs.leftenv(L - 1, psi)
    envs.rightenv(0, psi)
    return H, psi, envs


@pytest.mark.parametrize("name,L,D", [("heis", 10, 16), ("heis1", 8, 12), ("tfi", 10, 13), ("hubbard", 6, 16)])
def test_pair_formulas_match_the_oracle_on_canonical_chains(name, L, D):
    H, psi, envs = canonical_chain(name, L, D, seed=3)
    worst = 0.0
    for j in range(L - 1):
        s, A, O = H[j], psi.AL(j), H[j].full()
        W = O.shape[3]
        ref = mo.transfer_left(envs.leftenvs[j], s, A, A)                     # [q, chi, b] per level
        lev = pairgram_levels(O, A, True)
        assert set(range(1, W - 1)) <= set(lev)
        for v, m in lev.items():
            if v == W - 1:          # finished level: the D-block term on top of the fold application
                GLc = np.einsum("wts,pwa->stpa", O[1:, :, :, W - 1], np.stack([g[:, 0, :] for g in envs.leftenvs[j]], 1)[:, 1:, :])
                m = m + np.einsum("ptq,stpa,asb->qb", A, GLc, A)
            worst = max(worst, relerr(m, ref[v][:, 0, :]))
    for j in range(L - 1, 0, -1):
        s, A, O = H[j], psi.AR(j), H[j].full()
        ref = mo.transfer_right(envs.rightenvs[j + 1], s, A, A)               # [a, chi, p] per level
        for w, m in pairgram_levels(O, A, False).items():
            worst = max(worst, relerr(m, ref[w][:, 0, :]))
    print(f"{name}: pair-Gram levels against the oracle, worst rel. max-norm error {worst:.3e}")
    assert worst <= BAR


def _model(O, Dl, Dr):
    from mpskit_jl_amd import _lib
    lib = _lib.load()
    Of = np.asfortranarray(O, dtype=np.float64)
    out = [(C.c_int * 2)() for _ in range(4)]
    _lib.check(lib.mpsk_transfer_pair_model(O.shape[0], O.shape[3], O.shape[1], Of.ctypes.data_as(C.c_void_p), Dl, Dr, *out),
               "mpsk_transfer_pair_model")
    return [tuple(o) for o in out]                  # pairs, diagonal, levels, route: (left, right) each


# pairs (symmetric among them) and output levels per side.  Heisenberg: Sz gives the symmetric products of its non-zero
# diagonal entries (S = 1: m = 0 drops out), S+ and S- share their unordered pairs; no D block.  Ising: Z on the C / B
# blocks, X on the D block, which only the left transfer's combination sees.  Hubbard: see the restatement.
EXPECT = {"heis": ((3, 3), (2, 2), (3, 3)), "heis1": ((4, 4), (2, 2), (3, 3)), "tfi": ((3, 2), (2, 2), (2, 1))}


@pytest.mark.parametrize("name", sorted(MODELS))
def test_pair_tables_of_the_library(name):
    O = MODELS[name][0]()[0].full()
    pairs, diag, levels, _ = _model(O, 64, 64)
    for side, left in enumerate((True, False)):
        pp, lv, _ = pair_plan(O, left)
        assert pairs[side] == len(pp) and diag[side] == sum(i == j for i, j in pp) and levels[side] == len(lv), (name, side)
    if name in EXPECT:
        assert (pairs, diag, levels) == EXPECT[name], (name, pairs, diag, levels)
    else:
        assert all(p <= 10 for p in pairs) and levels == (5, 4)               # Hubbard: d (d + 1) / 2 at most; D block U n n


@pytest.mark.parametrize("name,D,want", [("heis", 1024, 1), ("heis1", 1024, 1), ("hubbard", 1024, 1), ("tfi", 1024, 0),
                                         ("heis", 256, 0), ("heis1", 256, 0), ("heis", 64, 0), ("tfi", 64, 0)])
def test_route_model(name, D, want):
    """Heisenberg S = 1/2, S = 1 and Hubbard take the pair route in the bulk of a large-D chain; the Ising slice (one
    interior level) never does; D = 256 and below stays launch-bound on today's route"""
    O = MODELS[name][0]()[0].full()
    route = _model(O, D, D)[3]
    assert route == (want, want), (name, D, route)


def test_route_model_follows_its_formula():
    """pairs at 2 K n^2 (symmetric: 0.55 of that) + 6 us against (W-2) levels of 2 d K n^2, both at 50 TFLOP/s"""
    for name in ("heis", "heis1", "hubbard"):
        O = MODELS[name][0]()[0].full()
        d, W = O.shape[1], O.shape[0]
        for Dl, Dr in ((300, 300), (352, 352), (400, 400), (128, 1024), (1024, 128), (700, 350)):
            route = _model(O, Dl, Dr)[3]
            for side, left in enumerate((True, False)):
                pp, _, _ = pair_plan(O, left)
                nd = sum(i == j for i, j in pp)
                K, n = (Dl, Dr) if left else (Dr, Dl)
                unit = 2.0 * K * n * n / 50e12
                assert route[side] == int((0.55 * nd + len(pp) - nd) * unit + 6e-6 < (W - 2) * d * unit), (name, Dl, Dr, side)
