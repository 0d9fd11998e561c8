"""Matrices whose SVD / QRpos factors are known exactly, the case lists of tests/test_gpu_factor_paths.py, and a Python
mirror of the few host lines that choose the path of mpsk_svd.hip and mpsk_cholqr.hip.

SVD input.  With H_k the Sylvester Hadamard matrix (entries +-1, H_k H_k^T = k I) and d small integers or dyadics,
    A = H_m[:, :n] diag(d) H_n                                  (m, n powers of two, m >= n)
has the singular values sqrt(m n) |d_i| EXACTLY, and every entry of A is an integer or a dyadic, so the fp64 matrix IS
the mathematical one.  Sizes that are no power of two are block sums: n = sum of powers of two k_b (its binary digits), one
square block H_k diag(d_b) H_k per digit (singular values k_b |d_i|), the blocks placed on the diagonal of an m x n zero
matrix and then rows and columns shuffled by fixed permutations ("orthogonal integer selections": the singular values do
not move, the blocks are interleaved over all 64-column pairs of the solver).  Rows beyond n stay zero.  Wide cases are
the transposes.  Complex cases multiply rows and columns by units from {1, i, -1, -i}: still exact, same singular values.
The builder checks what it claims: max |A| < 2^50, and (up to LD_MAX_WORK) the fp64 product equals the longdouble one
bit for bit.  The singular values are evaluated in numpy.longdouble.

Families of d:  "int" a permutation of 1..n;  "graded" 2^-(i mod 40) (1 + i // 40), 40 binades;  "rankdef" the integers
with the last quarter set to 0 (exact rank deficiency);  "cluster" four values, each n / 4 times (value and reconstruction
checks only: a singular vector inside a cluster is not defined).

QR input.  A = Q0 R0: Q0 the same block sum of Hadamard matrices (orthogonal integer columns of norm sqrt(k_b)), rows
shuffled; R0 = D (I + N) upper triangular with D a positive dyadic diagonal graded over log2(grade) binades and N a narrow
band of quarters.  QRpos is unique at full rank, so the factors are exactly Q0 diag(1 / norm) and diag(norm) R0 (longdouble).
`cond` is the measured 2-norm condition number of A.

Bounds (every one from LAPACK on the SAME inputs, never from the kernels; tests/test_exact_factor_inputs_cpu.py measures
them again and fails when a constant below is stale):
  SVD   |S - S_exact| <= C_SVD sqrt(max(m, n)) u sigma_max, the same figure componentwise for (U S) Vh - A.
        (max(m, n) are the rows of the tall orientation of the INPUT.  In svd modes 1-3 the iteration itself runs on the
        min(m, n)-square factor of a QRpos, but that QRpos of the tall matrix is part of the computation whose error is
        bounded, so the input's rows are kept: for 640 x 256 and 120 x 100 this is up to 1.6 x wider than sqrt(min).
        LAPACK's ratio is normalised by the same figure, so the constant and the bound are consistent.)
        numpy.linalg.svd (LAPACK gesdd) over svd_cases() + svd_child_cases(): worst ratio
        err / (sqrt(max(m, n)) u sigma_max) = LAPACK_SVD_RATIO (recorded below); C_SVD = 8 x that, rounded up.
  QR    |R - R_exact| <= C_QR u cond max|R_exact| and |Q - Q_exact| <= C_QR u cond.
        numpy.linalg.qr (LAPACK Householder geqrf) with the QRpos sign fix over qr_cases(): worst ratio LAPACK_QR_RATIO;
        C_QR = 8 x that, rounded up.
  Tall QR family (qr_stacked: t = m // n permuted, unit-scaled copies of the Hadamard block sum, so that every row stripe
        of a tall input holds weight; real and complex; house_cases() of tests/test_gpu_house_exact.py).  LAPACK's error
        against the exact factors grows like sqrt(m) there, so
        |R - R_exact| / max|R_exact| and |Q - Q_exact| <= C_QR_TALL sqrt(m) u cond,  |Q^H Q - I| <= C_ORTH_TALL sqrt(m) u,
        |Q R - A| <= C_RES_TALL sqrt(m) u max|R_exact|,  each constant 8 x LAPACK's worst ratio over the list, rounded up;
        complex R: strictly lower triangle and imag(diag) exactly 0.  house_plan() mirrors the host lines of the blocked
        Householder QRpos (mpsk_gauge.hip) that choose the outer blocks and inner panels; the case ids name them.
u = 2^-53 throughout.
"""
from __future__ import annotations

import functools
import os
import zlib
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -53
LIMIT = 2.0 ** 50
LD = np.longdouble
LD_MAX_WORK = 15 * 10 ** 7
J2 = 64                                  # columns of a Jacobi pair (mpsk_svd.hip)
CB = 64                                  # Cholesky block (mpsk_cholqr.hip)

# measured on the CPU with LAPACK on the case lists of this file (tests/test_exact_factor_inputs_cpu.py repeats the
# measurement): worst err / (sqrt(max(m, n)) u sigma_max) resp. worst err / (u cond), and 8 x that
LAPACK_SVD_RATIO = 1.021                 # 384 x 384 "int" (1024 x 1024 "int": 1.000)
C_SVD = 8.2
LAPACK_QR_RATIO = 0.186                  # 192 x 130, error of Q
C_QR = 1.5
# the tall family (qr_stacked) over house_cases(): worst ratios of LAPACK with the sign fix in the units of house_ratios()
# (err / (sqrt(m) u cond), |Q^H Q - I| / (sqrt(m) u), |Q R - A| / (sqrt(m) u max|R_exact|)), and 8 x each.  The factor
# ratio of the tall cases for comparison: 0.054 at 5000 x 13, 0.037 at 10000 x 5, 0.010 at 19712 x 3, 0.020 at complex 9856 x 3
LAPACK_QR_TALL_RATIO = 0.231             # 33 x 1, error of Q (2 x 2: 0.227)
C_QR_TALL = 1.9
LAPACK_ORTH_TALL_RATIO = 3.130           # 2 x 2 (4 x 4: 2.250, complex 9 x 8: 1.829)
C_ORTH_TALL = 25.1
LAPACK_RES_TALL_RATIO = 1.506            # 2 x 2 (complex 9 x 8: 1.093)
C_RES_TALL = 12.1


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


@functools.lru_cache(maxsize=None)
def hadamard(k):
    assert k >= 1 and k & (k - 1) == 0, k
    h = np.ones((1, 1))
    while h.shape[0] < k:
        h = np.block([[h, h], [h, -h]])
    h.setflags(write=False)
    return h


def pow2_blocks(n):
    """the powers of two of the binary digits of n, largest first"""
    return [1 << b for b in range(n.bit_length() - 1, -1, -1) if n >> b & 1]


def family_d(family, n):
    i = np.arange(n)
    if family == "int":
        return _rng(f"d-int-{n}").permutation(n).astype(np.float64) + 1.0
    if family == "graded":
        return 2.0 ** -(i % 40) * (1 + i // 40)
    if family == "rankdef":
        d = _rng(f"d-int-{n}").permutation(n).astype(np.float64) + 1.0
        d[n - n // 4:] = 0.0
        return d
    if family == "cluster":
        return np.array([8.0, 4.0, 2.0, 1.0])[i % 4]
    raise KeyError(family)


def _exact_product(L, d, R, what):
    """(L diag(d)) R in fp64, with the guard and the self-check of tests/exact_inputs.py"""
    A = (L * d) @ R
    assert float(np.abs(L).max() * np.abs(d).max() * np.abs(R).max() * L.shape[1]) < LIMIT, what
    assert np.abs(A).max() < LIMIT, what
    if L.shape[0] * L.shape[1] * R.shape[1] <= LD_MAX_WORK:
        assert np.array_equal(A.astype(LD), (L.astype(LD) * d.astype(LD)) @ R.astype(LD)), f"{what}: fp64 product is not exact"
    else:                                # too slow in longdouble: integers below 2^50 cannot round
        assert np.array_equal(d, np.round(d)), what
    return A


@functools.lru_cache(maxsize=None)
def svd_matrix(m, n, family, cplx=False):
    """(A, S_exact longdouble descending, rank).  m >= n builds the tall matrix; m < n its transpose."""
    if m < n:
        A, S, rank = svd_matrix(n, m, family, cplx)
        A = np.ascontiguousarray(A.T)
        A.setflags(write=False)
        return A, S, rank
    name = f"svd-{m}x{n}-{family}"
    d = family_d(family, n)
    if n & (n - 1) == 0 and m & (m - 1) == 0:
        A = _exact_product(hadamard(m)[:, :n], d, hadamard(n), name)
        S = np.sqrt(LD(m) * LD(n)) * np.abs(d).astype(LD)
    else:
        A = np.zeros((m, n))
        S, o = [], 0
        for k in pow2_blocks(n):
            A[o:o + k, o:o + k] = _exact_product(hadamard(k), d[o:o + k], hadamard(k), name)
            S.append(LD(k) * np.abs(d[o:o + k]).astype(LD))
            o += k
        S = np.concatenate(S)
        rng = _rng(name)
        A = A[rng.permutation(m)][:, rng.permutation(n)]
    if cplx:
        rng = _rng(name + "-units")
        units = np.array([1, 1j, -1, -1j])
        A = units[rng.integers(0, 4, m)][:, None] * A * units[rng.integers(0, 4, n)][None, :]
    A = np.ascontiguousarray(A)
    A.setflags(write=False)
    S = np.sort(S)[::-1]
    return A, S, int(np.count_nonzero(d))


@functools.lru_cache(maxsize=None)
def qr_matrix(m, n, log2grade):
    """(A, Q_exact, R_exact (longdouble), cond): A = Q0 R0 with the diagonal of R0 graded over log2grade binades"""
    name = f"qr-{m}x{n}-{log2grade}"
    rng = _rng(name)
    Q0 = np.zeros((m, n))
    norms, o = np.zeros(n, dtype=LD), 0
    for k in pow2_blocks(n):
        Q0[o:o + k, o:o + k] = hadamard(k)
        norms[o:o + k] = np.sqrt(LD(k))
        o += k
    perm = rng.permutation(n)            # columns too: the block norms (and so the diagonal of R) are interleaved
    Q0, norms = Q0[rng.permutation(m)][:, perm], norms[perm]
    dd = 2.0 ** -np.round(log2grade * np.arange(n) / max(n - 1, 1))
    R0 = np.eye(n)
    for off in (1, 2, 3):
        R0 += np.diag(rng.integers(-2, 3, n - off) / 4.0, off)
    R0 = dd[:, None] * R0
    A = Q0 @ R0
    assert np.abs(A).max() < LIMIT
    if m * n * n <= LD_MAX_WORK:
        assert np.array_equal(A.astype(LD), Q0.astype(LD) @ R0.astype(LD)), f"{name}: fp64 product is not exact"
    else:                                # a row of Q0 has one block's +-1, a column of R0 four dyadics within 2^-log2grade .. 1
        assert log2grade + 12 < 50
    Qx = Q0.astype(LD) / norms[None, :]
    Rx = norms[:, None] * R0.astype(LD)
    cond = float(np.linalg.cond(A))
    for a in (A, Qx, Rx):
        a.setflags(write=False)
    return A, Qx, Rx, cond


@functools.lru_cache(maxsize=None)
def qr_stacked(m, n, log2grade, cplx=False):
    """(A, Q_exact, R_exact (longdouble / clongdouble), cond) of the tall family: every row stripe of Q0 is occupied.
    Q0 = t = m // n copies of the block sum of Hadamard matrices of pow2_blocks(n), the rows of each copy permuted and
    multiplied by units (+-1; {1, i, -1, -i} for complex), m - t n zero rows appended, then all rows and the columns
    permuted: orthogonal columns of norm sqrt(t k_b) exactly.  R0 as in qr_matrix (a super-diagonal that does not exist is
    skipped, so n = 1, 2, 3 work); complex: the quarters are Gaussian integers / 4."""
    assert m >= n >= 1
    name = f"qrs-{m}x{n}-{log2grade}" + ("-c" if cplx else "")
    rng = _rng(name)
    t = m // n
    H, kcol, o = np.zeros((n, n)), np.zeros(n), 0
    for k in pow2_blocks(n):
        H[o:o + k, o:o + k] = hadamard(k)
        kcol[o:o + k] = k
        o += k
    units = np.array([1, 1j, -1, -1j]) if cplx else np.array([1.0, -1.0])
    Q0 = np.zeros((m, n), dtype=np.complex128 if cplx else np.float64)
    for i in range(t):
        Q0[i * n:(i + 1) * n] = units[rng.integers(0, len(units), n)][:, None] * H[rng.permutation(n)]
    perm = rng.permutation(n)
    Q0 = Q0[rng.permutation(m)][:, perm]
    norms = np.sqrt(LD(t) * kcol[perm].astype(LD))
    dd = 2.0 ** -np.round(log2grade * np.arange(n) / max(n - 1, 1))
    R0 = np.eye(n, dtype=Q0.dtype)
    for off in (1, 2, 3):
        if off < n:
            q = rng.integers(-2, 3, n - off) / 4.0
            if cplx:
                q = q + 1j * (rng.integers(-2, 3, n - off) / 4.0)
            R0 += np.diag(q, off)
    R0 = dd[:, None] * R0
    A = Q0 @ R0
    assert np.abs(A).max() < LIMIT and log2grade + 12 < 50
    ldt = np.clongdouble if cplx else LD
    assert m * n * n <= LD_MAX_WORK, name               # every shape of this family is small enough for the longdouble product
    assert np.array_equal(A.astype(ldt), Q0.astype(ldt) @ R0.astype(ldt)), f"{name}: fp64 product is not exact"
    Qx = Q0.astype(ldt) / norms[None, :]
    Rx = norms[:, None] * R0.astype(ldt)
    cond = float(np.linalg.cond(A))
    A = np.ascontiguousarray(A)
    for a in (A, Qx, Rx):
        a.setflags(write=False)
    return A, Qx, Rx, cond


@functools.lru_cache(maxsize=None)
def gauss_small(kind):
    """48 x 40 Gaussian ("gauss") / graded Gaussian over 12 decades ("graded"): the inputs checked against mpmath"""
    rng = _rng("gauss-small-" + kind)
    A = rng.standard_normal((48, 40))
    if kind == "graded":
        A = A * np.logspace(0, -12, 40)[None, :]
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def gauss_small_reference(kind):
    """singular values of gauss_small(kind) from mpmath at 40 digits (about a second), as longdouble"""
    import mpmath
    with mpmath.workdps(40):
        S = mpmath.svd_r(mpmath.matrix(gauss_small(kind).tolist()), compute_uv=False)
        return np.array([LD(mpmath.nstr(s, 25)) for s in S])


# ------------------------------------------------------------------------------------------------------------------
# the plan, as the library makes it (mpsk_svd.hip: svd_plan, csvd_plan, svd_default_chains, the clamps of tsvd();
# mpsk_api_factor.hip: which matrix the Jacobi iteration sees; mpsk_cholqr.hip: cq_use_trsm, cq_bufs)
# ------------------------------------------------------------------------------------------------------------------
N_XSTREAMS = 3                           # extra streams a ctx hands to tsvd(): at most 4 chains


def _q_of(rows, target):
    for c in range(target, 1, -1):
        if rows % c == 0 and (rows // c) % 2 == 0 and rows // c >= 128:
            return c
    return 1


def jacobi_shape(m, n, mode):
    """the (rows, columns) the Jacobi iteration runs on: svd modes 1-3 and mpsk_tsplit factor the tall orientation first
    and iterate on the square R^T (min(m, n) > 64); mode 0 iterates on the matrix itself"""
    mm, nn = max(m, n), min(m, n)
    return (nn, nn) if (mode != 0 and nn > 64) else (mm, nn)


def svd_plan(m, n, mode=3, env=None, cplx=False):
    """{"P", "Q", "kq", "kq_even", "NC", "pc"} of one mpsk_tsvd / mpsk_tsplit call under the MPSK_SVD_* settings of env"""
    env = env or {}
    mm, nn = jacobi_shape(m, n, mode)
    npad = (nn + J2 - 1) // J2 * J2
    P = npad // J2
    target = min(max(1024 // P, 1), 16)
    if cplx:                             # csvd_plan reads no environment and has no chains
        Q = _q_of(2 * mm, target)
        return {"P": P, "Q": Q, "kq": 2 * mm // Q, "kq_even": True, "NC": 1, "pc": P}
    if "MPSK_SVD_Q" in env and 1 <= int(env["MPSK_SVD_Q"]) <= 16:
        target = int(env["MPSK_SVD_Q"])
    Q = _q_of(mm, target)
    kq = mm // Q
    nc = 4 if (P >= 64 and P % 4 == 0) else (2 if (P >= 32 and P % 2 == 0) else 1)
    if "MPSK_SVD_CHAINS" in env and 1 <= int(env["MPSK_SVD_CHAINS"]) <= 8:
        nc = int(env["MPSK_SVD_CHAINS"])
    if nc > 1 and (P % nc != 0 or P // nc < 2):
        nc = 1
    if nc > 1 + N_XSTREAMS:
        nc = 4
    if nc > 1 and (P % nc != 0 or P // nc < 2):
        nc = 1
    return {"P": P, "Q": Q, "kq": kq, "kq_even": kq % 2 == 0 and mm % 2 == 0 and nn % 2 == 0, "NC": nc, "pc": P // nc}


def qr_plan(m, n, env=None):
    """{"npad", "nb", "route": "solve" | "gemm", "gram", "levels"}: the CholeskyQR route of an m x n QRpos (n > 64)"""
    env = env or {}
    nb = (n + CB - 1) // CB
    p2 = 1
    while p2 < nb:
        p2 <<= 1
    npad = p2 * CB
    trsm = int(env.get("MPSK_CQ_TRSM", "1")) != 0 and (npad // CB) * ((m + CB - 1) // CB) <= 768
    gram = trsm and int(env.get("MPSK_CQ_GRAM", "1")) != 0
    levels, b = 0, 2 * CB
    while b < npad:
        levels, b = levels + 1, b << 1
    mt = (m + CB - 1) // CB
    chunk = (mt + 16 - 1) // 16          # row tiles per K-split of the in-step Gram (CQ_GS = 16 splits)
    return {"npad": npad, "nb": nb, "route": "solve" if trsm else "gemm", "gram": gram, "levels": levels,
            "gram_splits_used": (mt + chunk - 1) // chunk}


QR_NB, QR_NBI, QR_PANEL_DOUBLES = 32, 8, 19712   # mpsk_gauge.hip: outer block, inner panel, LDS doubles of one panel
HOUSE_MAX_ROWS = QR_PANEL_DOUBLES                # one panel column must fit: m <= 19712 (complex: 2 m <= 19712)


def house_plan(m, n):
    """((j0, nbo, nbi, ragged_last_panel), ...): the outer blocks of the blocked Householder QRpos of a real m x n matrix
    (qrpos() in mpsk_gauge.hip): nbo columns from j0, inner panels of nbi columns that share the LDS with PS = m - j0 rows,
    the last panel narrower than nbi when nbi does not divide nbo"""
    assert n <= m <= HOUSE_MAX_ROWS
    out = []
    for j0 in range(0, n, QR_NB):
        nbo = min(n - j0, QR_NB)
        nbi = max(1, min(QR_PANEL_DOUBLES // (m - j0), QR_NBI))
        out.append((j0, nbo, nbi, nbo % nbi != 0))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------------
# case lists
# ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class SvdCase:
    """call: "tsvd" (svd mode `mode`), "tsvd_c" (complex, mode `mode`), "tsplit" (mode 2: the V-free iteration).
    env: the per-call MPSK_SVD_* settings; plan: what the id claims (checked on the CPU against svd_plan())."""
    m: int
    n: int
    family: str
    call: str = "tsvd"
    mode: int = 3
    env: tuple = ()
    plan: tuple = ()

    @property
    def envd(self):
        return dict(self.env)

    @property
    def cplx(self):
        return self.call == "tsvd_c"

    @property
    def name(self):
        e = ",".join(f"{k[9:]}={v}" for k, v in self.env) or "default"
        p = "-".join(f"{k}{v}" for k, v in self.plan)
        return f"{self.call}{self.mode}-{self.m}x{self.n}-{self.family}-{e}-{p}"

    def default(self):
        return SvdCase(self.m, self.n, self.family, self.call, self.mode)


def _c(m, n, family, call="tsvd", mode=3, env=None, **plan):
    return SvdCase(m, n, family, call, mode, tuple(sorted((env or {}).items())), tuple(sorted(plan.items())))


CH = "MPSK_SVD_CHAINS"


def chain_cases():
    """every chained schedule in the accumulated-V form (mode 3), the plain form (mode 0) and the V-free form (tsplit)"""
    out = []
    for call, mode in (("tsvd", 3), ("tsplit", 2)):
        fams = ("int", "graded") if call == "tsvd" else ("int",)
        for f in fams:
            out += [_c(256, 256, f, call, mode, {CH: "2"}, P=4, NC=2, pc=2),         # the smallest legal schedule
                    _c(512, 512, f, call, mode, {CH: "2"}, P=8, NC=2, pc=4),
                    _c(512, 512, f, call, mode, {CH: "4"}, P=8, NC=4, pc=2)]
        out += [_c(384, 384, "int", call, mode, {CH: "3"}, P=6, NC=3, pc=2),          # 384 = 256 + 128: block sum
                _c(1024, 1024, "int", call, mode, {CH: "8"}, P=16, NC=4, pc=4),       # 8 chains asked, 4 streams: clamps to 4
                _c(512, 512, "int", call, mode, {CH: "8"}, P=8, NC=1, pc=8),          # 8 does not leave 2 pairs a chain: unchained
                _c(320, 320, "int", call, mode, {CH: "2"}, P=5, NC=1, pc=5),          # 2 does not divide 5: unchained
                _c(200, 200, "int", call, mode, {CH: "2"}, P=4, NC=2, pc=2)]          # 56 zero-padded columns travel
    out += [_c(512, 512, "cluster", "tsvd", 3, {CH: "2"}, P=8, NC=2, pc=4),
            _c(640, 256, "rankdef", "tsvd", 3, {CH: "2"}, P=4, NC=2, pc=2)]
    # plain mode: mm != nn, so the G and V destination tables differ
    out += [_c(1024, 256, "int", "tsvd", 0, {CH: "2"}, P=4, NC=2, pc=2, Q=8),
            _c(256, 1024, "int", "tsvd", 0, {CH: "2"}, P=4, NC=2, pc=2, Q=8),
            _c(1024, 512, "int", "tsvd", 0, {CH: "4"}, P=8, NC=4, pc=2, Q=8),         # more than two chains with mm != nn
            _c(257, 200, "int", "tsvd", 0, {CH: "2"}, P=4, NC=2, pc=2, Q=1, kq=257, kq_even=False)]
    return out


def q_cases():
    """the K-splits of the Gram product: plain mode at 2048 x 256 (default Q = 16), and an odd kq with P > 1"""
    QV = "MPSK_SVD_Q"
    return [_c(2048, 256, "int", "tsvd", 0, {QV: "1"}, P=4, Q=1, kq=2048),
            _c(2048, 256, "int", "tsvd", 0, {QV: "3"}, P=4, Q=2, kq=1024),            # 3 does not divide 2048
            _c(2048, 256, "int", "tsvd", 0, {QV: "16"}, P=4, Q=16, kq=128),
            _c(2048, 256, "int", "tsvd", 0, None, P=4, Q=16, kq=128),
            _c(257, 200, "int", "tsvd", 0, None, P=4, Q=1, kq=257, kq_even=False, NC=1),
            _c(256, 256, "graded", "tsvd", 3, {"MPSK_SVD_INNER": "3"}, P=4)]


def complex_cases():
    """csvd_plan reads no environment: shapes that give Q = 1, an odd Q and Q = 16 by themselves"""
    return [_c(120, 100, "int", "tsvd_c", 3, None, P=2, Q=1, kq=200),                 # 2 mm = 200: no split leaves 128 rows
            _c(320, 320, "int", "tsvd_c", 3, None, P=5, Q=5, kq=128),
            _c(256, 256, "graded", "tsvd_c", 3, None, P=4, Q=4, kq=128),
            _c(1024, 128, "int", "tsvd_c", 0, None, P=2, Q=16, kq=128),
            _c(128, 1024, "int", "tsvd_c", 0, None, P=2, Q=16, kq=128)]


def svd_cases():
    return chain_cases() + q_cases() + complex_cases()


def svd_child_cases():
    """what every load-time child runs (MPSK_SVD_EIG / _INTRA / _LAG): the default plan unless the child's environment
    says otherwise; P > 1 throughout (the intra-block skip is only allowed with more than one pair)"""
    return [_c(256, 256, "int"), _c(256, 256, "graded"), _c(512, 512, "graded"), _c(200, 200, "int"),
            _c(640, 256, "rankdef"), _c(512, 512, "cluster"), _c(1024, 256, "int", "tsvd", 0), _c(257, 200, "int", "tsvd", 0),
            _c(256, 256, "int", "tsplit", 2), _c(512, 512, "graded", "tsplit", 2), _c(256, 256, "graded", "tsvd_c")]


@dataclass(frozen=True)
class QrCase:
    m: int
    n: int
    log2grade: int                       # binades of the diagonal of R0

    @property
    def name(self):
        return f"qr-{self.m}x{self.n}-grade2^{self.log2grade}"


# (1000, 130): 16 row tiles, so every one of the CQ_GS = 16 K-splits of the in-step Gram holds rows, the last one a ragged
# tile; at the other shapes ceil(m / 64) is no multiple of 16 and the last splits are empty
QR_SHAPES = [(65, 65), (129, 65), (257, 256), (640, 193), (900, 899), (1100, 700), (192, 130), (1000, 130)]
CQ_GS = 16


def qr_cases():
    """every shape at cond ~ 1e2, and the graded ones (cond ~ 1e6, 1e10) at two shapes"""
    return [QrCase(m, n, 3) for m, n in QR_SHAPES] + [QrCase(640, 193, 16), QrCase(640, 193, 32),
                                                     QrCase(257, 256, 16), QrCase(257, 256, 32)]


@dataclass(frozen=True)
class HouseCase:
    """One input of tests/test_gpu_house_exact.py.  family "stacked": qr_stacked (bounds C_*_TALL); "matrix": qr_matrix
    (bound C_QR, as in qr_cases()).  mode: the qr mode of the call (0 default, 1 Householder at every n).  route: what the id
    claims, checked on the CPU against house_route(): the outer blocks "nbo/nbi" of house_plan ("r": ragged last panel,
    "k x" k equal blocks in a row) of the real matrix the Householder kernels see -- for complex input the 2m x 2n
    embedding --, or "cholqr" where the dispatcher takes the CholeskyQR ladder (default mode, more than 64 real columns)."""
    m: int
    n: int
    log2grade: int = 3
    cplx: bool = False
    mode: int = 0
    family: str = "stacked"
    route: str = ""

    @property
    def name(self):
        return (f"{'c' if self.cplx else ''}house{self.mode}-{self.family}-{self.m}x{self.n}-grade2^{self.log2grade}"
                f"-{self.route}")

    @property
    def real_shape(self):
        return (2 * self.m, 2 * self.n) if self.cplx else (self.m, self.n)

    @property
    def householder(self):
        return self.mode == 1 or self.real_shape[1] <= 64

    def matrix(self):
        if self.family == "matrix":
            return qr_matrix(self.m, self.n, self.log2grade)
        return qr_stacked(self.m, self.n, self.log2grade, self.cplx)


def house_route(case: HouseCase):
    if not case.householder:
        return "cholqr"
    tags = [f"{nbo}/{nbi}{'r' if rg else ''}" for _, nbo, nbi, rg in house_plan(*case.real_shape)]
    out, i = [], 0
    while i < len(tags):
        k = 1
        while i + k < len(tags) and tags[i + k] == tags[i]:
            k += 1
        out.append(tags[i] if k == 1 else f"{k}x{tags[i]}")
        i += k
    return "+".join(out)


def _h(m, n, route, grade=3, **kw):
    return HouseCase(m, n, grade, route=route, **kw)


def house_real_cases():
    """default qr mode, n <= 64: the Householder route; every case on the tall family"""
    return [_h(1, 1, "1/8r"), _h(33, 1, "1/8r"), _h(2, 2, "2/8r"), _h(4, 4, "4/8r"),   # smallest n: skipped super-diagonals
            _h(9, 8, "8/8"), _h(17, 9, "9/8r"),                         # one full panel; a full panel and a panel of one
            _h(40, 31, "31/8r"), _h(64, 32, "32/8"), _h(65, 33, "32/8+1/8r"),   # ragged / exact block, a second block of one column
            _h(100, 37, "32/8+5/8r"), _h(100, 37, "32/8+5/8r", 16), _h(100, 37, "32/8+5/8r", 32),
            _h(64, 64, "2x32/8"), _h(64, 64, "2x32/8", 16), _h(64, 64, "2x32/8", 32),
            _h(200, 63, "32/8+31/8r"), _h(200, 63, "32/8+31/8r", 16), _h(200, 63, "32/8+31/8r", 32),
            _h(2465, 16, "16/7r"),                                      # the first row count with nbi = 7
            _h(2465, 40, "32/7r+8/8"), _h(2465, 40, "32/7r+8/8", 32),   # nbi changes between the outer blocks
            _h(5000, 12, "12/3"), _h(5000, 13, "13/3r"),                # nbi = 3: four full panels; a ragged fifth
            _h(10000, 5, "5/1"),                                        # nbi = 1
            _h(19712, 3, "3/1")]                                        # the row limit


def house_mode1_cases():
    """qr mode 1 at n > 64 (WY trailing updates and back-accumulation over many outer blocks): shapes of qr_cases()"""
    kw = dict(mode=1, family="matrix")
    return [_h(129, 65, "2x32/8+1/8r", **kw), _h(640, 193, "6x32/8+1/8r", **kw),
            _h(257, 256, "8x32/8", **kw), _h(257, 256, "8x32/8", 32, **kw)]


def house_complex_cases():
    """qrpos_c / lqpos_c: the route of the 2m x 2n embedding"""
    kw = dict(cplx=True)
    return [_h(1, 1, "2/8r", **kw), _h(9, 8, "16/8", **kw), _h(40, 31, "32/8+30/8r", **kw),
            _h(64, 32, "2x32/8", **kw),                                 # 2n = 64: the last Householder size
            _h(66, 33, "cholqr", **kw), _h(130, 65, "cholqr", **kw),    # 2n = 66: the first CholeskyQR size
            _h(100, 37, "cholqr", **kw), _h(100, 37, "cholqr", 32, **kw),
            _h(2465, 16, "32/3r", **kw),                                # tall: 4930 embedded rows
            _h(9856, 3, "6/1", **kw)]                                   # the complex row limit: 19712 embedded rows


def house_cases():
    return house_real_cases() + house_mode1_cases() + house_complex_cases()


# ------------------------------------------------------------------------------------------------------------------
# checks (shared by the GPU tests, the child runner and -- with LAPACK in place of the library -- the CPU test)
# ------------------------------------------------------------------------------------------------------------------
def svd_bound(case: SvdCase):
    _, S, _ = svd_matrix(case.m, case.n, case.family, case.cplx)
    return C_SVD * np.sqrt(max(case.m, case.n)) * U * float(S[0])


def check_svd_factors(case: SvdCase, Uf, S, Vh, what=None):
    """list of failed properties of a full (untruncated) factorisation U diag(S) Vh of the case's matrix"""
    A, Sx, rank = svd_matrix(case.m, case.n, case.family, case.cplx)
    bound, bad = svd_bound(case), []
    k = min(case.m, case.n)
    if not np.all(np.diff(S) <= 0):
        bad.append("S not sorted")
    es = float(np.abs(S.astype(LD) - Sx).max())
    if not es <= bound:
        bad.append(f"|S - S_exact| = {es:.3e} > {bound:.3e}")
    r = rank if case.family == "rankdef" else k      # the vectors of an exactly zero singular value are not defined
    eu = np.abs(Uf[:, :r].conj().T @ Uf[:, :r] - np.eye(r)).max()
    ev = np.abs(Vh[:r] @ Vh[:r].conj().T - np.eye(r)).max()
    if not (eu < 1e-12 and ev < 1e-12):
        bad.append(f"orthogonality U {eu:.3e} Vh {ev:.3e} >= 1e-12")
    er = float(np.abs((Uf * S) @ Vh - A).max())
    if not er <= bound:
        bad.append(f"|(U S) Vh - A| = {er:.3e} > {bound:.3e}")
    return [f"{what or case.name}: {b}" for b in bad]


def check_split_factors(case: SvdCase, al, c, ar, S):
    A, Sx, _ = svd_matrix(case.m, case.n, case.family)
    bound, bad = svd_bound(case), []
    k = len(S)
    if k != min(case.m, case.n):
        bad.append(f"kept {k}")
    if not np.all(np.diff(S) <= 0):
        bad.append("S not sorted")
    es = float(np.abs(S.astype(LD) - Sx[:k]).max())
    if not es <= bound:
        bad.append(f"|S - S_exact| = {es:.3e} > {bound:.3e}")
    sc = np.linalg.svd(c, compute_uv=False)          # c carries the same singular values
    if not np.abs(sc.astype(LD) - Sx[:k]).max() <= bound:
        bad.append(f"|svd(c) - S_exact| = {float(np.abs(sc - Sx[:k]).max()):.3e} > {bound:.3e}")
    eu, ev = np.abs(al.T @ al - np.eye(k)).max(), np.abs(ar @ ar.T - np.eye(k)).max()
    if not (eu < 1e-12 and ev < 1e-12):
        bad.append(f"isometry al {eu:.3e} ar {ev:.3e} >= 1e-12")
    er = float(np.abs(al @ c @ ar - A).max())
    if not er <= bound:
        bad.append(f"|al c ar - A| = {er:.3e} > {bound:.3e}")
    return [f"{case.name}: {b}" for b in bad]


def run_svd_case(be, case: SvdCase, keep=None):
    """one case through the library under the environment of the caller; returns (failures, sweeps, raw outputs)"""
    A, _, _ = svd_matrix(case.m, case.n, case.family, case.cplx)
    be.set_svd_mode(case.mode)
    try:
        if case.call == "tsplit":
            al, c, ar, S, _ = be.tsplit(be.upload(A))
            out = (be.download(al), be.download(c), be.download(ar), S)
            bad = check_split_factors(case, *out)
        else:
            if case.cplx:
                Uf, S, Vh, kept, disc = be.tsvd_c(be.upload_c(A))
                out = (be.download_c(Uf), be.download(S), be.download_c(Vh))
            else:
                Uf, S, Vh, kept, disc = be.tsvd(be.upload(A))
                out = (be.download(Uf), be.download(S), be.download(Vh))
            bad = check_svd_factors(case, *out)
            if kept != min(case.m, case.n) or disc != 0.0:
                bad.append(f"{case.name}: kept {kept}, disc {disc} without truncation")
        return bad, be.svd_sweeps(), out
    finally:
        be.set_svd_mode(3)


def lapack_qrpos(A):
    Q, R = np.linalg.qr(A)
    if np.iscomplexobj(A):               # divide by the phase of the diagonal; the diagonal itself becomes |diag| exactly
        d = np.diag(R).copy()
        ph = np.where(d == 0, 1.0, d / np.where(d == 0, 1.0, np.abs(d)))
        Q, R = Q * ph, R / ph[:, None]
        R[np.diag_indices_from(R)] = np.abs(d)
        return Q, R
    sg = np.sign(np.diag(R))
    sg[sg == 0] = 1
    return Q * sg, sg[:, None] * R


def house_ratios(case: HouseCase, Q, R):
    """(factor, orthogonality, residual) errors of Q R = A of a tall-family case in the units of their bounds:
    max(|R - Rx| / max|Rx|, |Q - Qx|) / (sqrt(m) u cond), |Q^H Q - I| / (sqrt(m) u), |Q R - A| / (sqrt(m) u max|Rx|);
    the products are formed in longdouble, so the figures hold the factors' own error only"""
    A, Qx, Rx, cond = case.matrix()
    ldt = Qx.dtype
    Ql, Rl = Q.astype(ldt), R.astype(ldt)
    rmax, su = float(np.abs(Rx).max()), np.sqrt(case.m) * U
    ef = max(float(np.abs(Rl - Rx).max()) / rmax, float(np.abs(Ql - Qx).max()))
    eo = float(np.abs(Ql.conj().T @ Ql - np.eye(case.n)).max())
    ea = float(np.abs(Ql @ Rl - A.astype(ldt)).max())
    return ef / (su * cond), eo / su, ea / (su * rmax)


def check_house_factors(case: HouseCase, Q, R, what="qrpos"):
    """list of failed properties of Q R = A against the exact factors (LQpos: pass Q^H, L^H)"""
    if case.family == "matrix":
        return check_qr_factors(QrCase(case.m, case.n, case.log2grade), Q, R, what)
    bad = []
    if Q.shape != (case.m, case.n) or R.shape != (case.n, case.n) or np.iscomplexobj(Q) != case.cplx:
        return [f"{case.name} {what}: shapes {Q.shape} {R.shape}"]
    if not (np.all(np.isfinite(Q)) and np.all(np.isfinite(R))):
        return [f"{case.name} {what}: not finite"]
    if np.abs(np.tril(R, -1)).max(initial=0.0) != 0.0:
        bad.append("tril(R, -1) != 0")
    if np.abs(np.diag(R).imag).max() != 0.0:
        bad.append("imag(diag(R)) != 0")
    if not np.all(np.diag(R).real > 0):
        bad.append("diag(R) not positive")
    rf, ro, ra = house_ratios(case, Q, R)
    if not rf <= C_QR_TALL:
        bad.append(f"factor error / (sqrt(m) u cond) = {rf:.3f} > {C_QR_TALL}")
    if not ro <= C_ORTH_TALL:
        bad.append(f"|Q^H Q - I| / (sqrt(m) u) = {ro:.3f} > {C_ORTH_TALL}")
    if not ra <= C_RES_TALL:
        bad.append(f"|Q R - A| / (sqrt(m) u max|R|) = {ra:.3f} > {C_RES_TALL}")
    return [f"{case.name} {what}: {b}" for b in bad]


def inner_factorizations(s0, s1):
    """real factorizations between two qr_stats() readings: every pass through the dispatcher ends in exactly one of these"""
    return sum(s1[k] - s0[k] for k in ("cholqr3", "robust", "householder"))


def run_house_case(be, case: HouseCase):
    """QRpos of the case and LQpos of its (conjugate) transpose under the case's qr mode: (failures, stats before, between,
    after).  The caller restores the qr mode."""
    A = case.matrix()[0]
    At = np.ascontiguousarray(A.conj().T)
    be.set_qr_mode(case.mode)
    s0 = be.qr_stats()
    if case.cplx:
        Q, R = (be.download_c(t) for t in be.qrpos_c(be.upload_c(A)))
        s1 = be.qr_stats()
        L, Ql = (be.download_c(t) for t in be.lqpos_c(be.upload_c(At)))
    else:
        Q, R = (be.download(t) for t in be.qrpos(be.upload(A)))
        s1 = be.qr_stats()
        L, Ql = (be.download(t) for t in be.lqpos(be.upload(At)))
    s2 = be.qr_stats()
    bad = check_house_factors(case, Q, R)
    bad += check_house_factors(case, np.ascontiguousarray(Ql.conj().T), np.ascontiguousarray(L.conj().T), "lqpos")
    return bad, s0, s1, s2


def check_qr_factors(case: QrCase, Q, R, what="qrpos"):
    """list of failed properties of Q R = A against the exact factors (LQpos: pass Q^T, L^T)"""
    A, Qx, Rx, cond = qr_matrix(case.m, case.n, case.log2grade)
    n, bad = case.n, []
    bound = C_QR * U * cond
    if np.abs(np.tril(R, -1)).max(initial=0.0) != 0.0:
        bad.append("tril(R, -1) != 0")
    if not np.all(np.diag(R) > 0):
        bad.append("diag(R) not positive")
    er = float(np.abs(R.astype(LD) - Rx).max() / np.abs(Rx).max())
    eq = float(np.abs(Q.astype(LD) - Qx).max())
    if not er <= bound:
        bad.append(f"|R - R_exact| / max|R| = {er:.3e} > {bound:.3e}")
    if not eq <= bound:
        bad.append(f"|Q - Q_exact| = {eq:.3e} > {bound:.3e}")
    eo = np.abs(Q.T @ Q - np.eye(n)).max()
    if not eo < 1e-13:
        bad.append(f"|Q^T Q - I| = {eo:.3e} >= 1e-13")
    ea = np.abs(Q @ R - A).max()
    if not ea < 1e-14 * np.abs(A).max():
        bad.append(f"|Q R - A| = {ea:.3e} >= 1e-14 |A|_max = {1e-14 * np.abs(A).max():.3e}")
    return [f"{case.name} {what}: {b}" for b in bad]


def run_qr_case(be, case: QrCase):
    """qrpos and lqpos of the transpose against the exact factors.  A CholeskyQR pass that goes wrong is caught by the
    library's own flags and the call silently finished by the next rung of the ladder (retry, cholqr_robust, Householder),
    so a correct result alone proves nothing about the route: Householder must not run at all, and at cond ~ 1e2 (grade
    2^3) not even the robust variant -- CholeskyQR3 has no excuse there."""
    A = qr_matrix(case.m, case.n, case.log2grade)[0]
    s0 = be.qr_stats()
    Q, R = (be.download(t) for t in be.qrpos(be.upload(A)))
    bad = check_qr_factors(case, Q, R)
    L, Ql = (be.download(t) for t in be.lqpos(be.upload(np.ascontiguousarray(A.T))))
    bad += check_qr_factors(case, np.ascontiguousarray(Ql.T), np.ascontiguousarray(L.T), "lqpos")
    s1 = be.qr_stats()
    if s1["householder"] != s0["householder"] or (case.log2grade <= 3 and s1["fallback"] != s0["fallback"]):
        bad.append(f"{case.name}: left the CholeskyQR3 route: {s0} -> {s1}")
    return bad


def setting_names():
    return ["MPSK_SVD_EIG", "MPSK_SVD_INTRA", "MPSK_SVD_CHAINS", "MPSK_SVD_Q", "MPSK_SVD_INNER", "MPSK_SVD_LAG",
            "MPSK_CQ_TRSM", "MPSK_CQ_GRAM", "MPSK_SVD_DEBUG"]


def clean_env():
    env = dict(os.environ)
    for k in setting_names():
        env.pop(k, None)
    return env
