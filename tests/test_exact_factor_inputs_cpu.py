"""CPU self-checks of tests/exact_factor_inputs.py: the builders against their own criteria, the constants of the bounds
against LAPACK and mpmath on the same inputs, and every case of tests/test_gpu_factor_paths.py on the path its id names."""
import os

import numpy as np
import pytest

import exact_factor_inputs as fi

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mpskit.jl_amd", "csrc")
ALL_SVD = fi.svd_cases() + fi.svd_child_cases()


def _matrices():
    return sorted({(c.m, c.n, c.family, c.cplx) for c in ALL_SVD})


def test_the_mirrored_plan_lines_are_still_in_the_library():
    """svd_plan() / qr_plan() restate these host lines; if one changes, the mirror (and the case ids) must follow"""
    svd = open(os.path.join(CSRC, "mpsk_svd.hip")).read()
    cq = open(os.path.join(CSRC, "mpsk_cholqr.hip")).read()
    for line in ("int target = 1024 / p.P;", "if (target > 16) target = 16;",
                 "if (p.mm % c == 0 && (p.mm / c) % 2 == 0 && p.mm / c >= 128) { q = c; break; }",
                 "if (mr % c == 0 && (mr / c) % 2 == 0 && mr / c >= 128) { q = c; break; }",
                 "int nc = (P >= 64 && P % 4 == 0) ? 4 : ((P >= 32 && P % 2 == 0) ? 2 : 1);",
                 "if (v >= 1 && v <= 8) nc = v;", "if (nc > 1 && (P % nc != 0 || P / nc < 2)) nc = 1;",
                 "if (NC > 1 + nxs) NC = (1 + nxs >= 4) ? 4 : ((1 + nxs >= 2) ? 2 : 1);",
                 "const bool kq_even = (kq % 2 == 0) && (mm % 2 == 0) && (nn % 2 == 0);"):
        assert line in svd, line
    assert "(int64_t)(npad / CB) * ((m + CB - 1) / CB) <= 768" in cq
    assert "for (int b = 2 * CB; b < npad; b <<= 1)" in cq


def test_every_case_is_on_the_path_its_id_names():
    assert fi.chain_cases() and fi.q_cases() and fi.complex_cases() and fi.svd_child_cases() and fi.qr_cases()
    assert len({c.name for c in fi.svd_cases()}) == len(fi.svd_cases())
    for c in ALL_SVD:
        p = fi.svd_plan(c.m, c.n, c.mode, c.envd, c.cplx)
        for k, v in c.plan:
            assert p[k] == v, (c.name, k, v, p)
    plans = [(c, fi.svd_plan(c.m, c.n, c.mode, c.envd, c.cplx)) for c in fi.svd_cases()]
    real = [(c, p) for c, p in plans if not c.cplx]
    for call, mode in (("tsvd", 3), ("tsvd", 0), ("tsplit", 2)):
        got = {(p["NC"], p["pc"]) for c, p in real if (c.call, c.mode) == (call, mode)}
        assert (2, 2) in got, (call, mode, got)                          # the smallest legal schedule in every form
        if mode != 0:
            assert {(2, 4), (4, 2), (3, 2), (4, 4)} <= got, (call, mode, got)
        else:                                                            # plain mode: two and four chains with mm != nn
            assert (4, 2) in got, got
    # asked-for chains that must NOT be used, and the clamp 8 -> 4
    assert any(c.envd.get(fi.CH) == "2" and p["NC"] == 1 and p["P"] == 5 for c, p in real)
    assert any(c.envd.get(fi.CH) == "8" and p["NC"] == 4 for c, p in real)
    assert any(c.envd.get(fi.CH) == "8" and p["NC"] == 1 for c, p in real)
    # ragged n under chains, odd rows (kq_even false) with more than one pair, mm != nn under chains
    assert any(c.n % 64 and p["NC"] == 2 for c, p in real)
    assert any(not p["kq_even"] and p["P"] > 1 and p["NC"] == 2 for c, p in real)
    assert any(not p["kq_even"] and p["P"] > 1 and p["NC"] == 1 for c, p in real)
    assert any(c.mode == 0 and c.m > c.n and p["NC"] == 2 for c, p in real) and any(c.mode == 0 and c.m < c.n and p["NC"] == 2 for c, p in real)
    # K-splits: Q = 1 on a multi-pair problem, the fall from 3 to 2, the largest Q, forced and by default
    qs = {(c.envd.get("MPSK_SVD_Q"), p["Q"]) for c, p in real if c.mode == 0 and (c.m, c.n) == (2048, 256)}
    assert qs == {("1", 1), ("3", 2), ("16", 16), (None, 16)} and all(p["P"] == 4 for c, p in real if (c.m, c.n) == (2048, 256))
    assert any("MPSK_SVD_INNER" in c.envd and p["P"] > 1 for c, p in real)
    cq = {p["Q"] for c, p in plans if c.cplx and p["P"] > 1}
    assert 1 in cq and 16 in cq and any(q > 1 and q % 2 for q in cq), cq
    for c in fi.svd_child_cases():                                        # the intra-block skip needs more than one pair
        assert fi.svd_plan(c.m, c.n, c.mode, {}, c.cplx)["P"] > 1, c.name
    # CholeskyQR: the suite's default route is the in-step solve everywhere; MPSK_CQ_TRSM=0 sends every case to the GEMM
    # route, MPSK_CQ_GRAM=0 keeps the solve and drops the in-step Gram
    for c in fi.qr_cases():
        assert c.n > 64
        assert fi.qr_plan(c.m, c.n) == dict(fi.qr_plan(c.m, c.n), route="solve", gram=True), c.name
        assert fi.qr_plan(c.m, c.n, {"MPSK_CQ_TRSM": "0"})["route"] == "gemm"
        g = fi.qr_plan(c.m, c.n, {"MPSK_CQ_GRAM": "0"})
        assert g["route"] == "solve" and not g["gram"]
    assert {(c.m, c.n) for c in fi.qr_cases()} == set(fi.QR_SHAPES)
    assert "constexpr int CQ_GS = 16;" in open(os.path.join(CSRC, "mpsk_cholqr.hip")).read()
    assert fi.qr_plan(1000, 130)["gram_splits_used"] == 16 and fi.qr_plan(1000, 130)["gram"]     # the last K-split holds rows
    big = fi.qr_plan(1100, 700)
    assert big["npad"] == 1024 and big["levels"] == 3 and big["nb"] == 11    # even and odd step launches carry the pair workgroup
    assert fi.qr_plan(192, 130) == dict(fi.qr_plan(192, 130), npad=256, nb=3)
    assert fi.qr_plan(4096, 1024)["route"] == "gemm" and fi.qr_plan(2048, 1024)["route"] == "solve"   # the earlier suite's only GEMM case


def test_svd_builders_and_the_constant_of_the_svd_bound():
    """exactness is asserted inside the builder (2^50 guard, fp64 == longdouble); here: the stated singular values against
    LAPACK within 1e-14 sigma_max, and C_SVD = 8 x LAPACK's worst ratio over the whole list (value and reconstruction)"""
    worst = 0.0
    for m, n, family, cplx in _matrices():
        A, S, rank = fi.svd_matrix(m, n, family, cplx)
        assert A.shape == (m, n) and len(S) == min(m, n) and np.iscomplexobj(A) == cplx
        assert np.count_nonzero(S) == rank and (rank < min(m, n)) == (family == "rankdef")
        Uf, Sl, Vh = np.linalg.svd(A, full_matrices=False)
        Sv = np.linalg.svd(A, compute_uv=False)                           # (LAPACK's values-only driver differs)
        es = max(float(np.abs(Sl.astype(fi.LD) - S).max()), float(np.abs(Sv.astype(fi.LD) - S).max()))
        assert es <= 1e-14 * float(S[0]), (m, n, family, es / float(S[0]))
        er = float(np.abs((Uf * Sl) @ Vh - A).max())
        worst = max(worst, max(es, er) / (np.sqrt(max(m, n)) * fi.U * float(S[0])))
    for kind in ("gauss", "graded"):                                      # unstructured input: LAPACK against mpmath
        A, S = fi.gauss_small(kind), fi.gauss_small_reference(kind)
        assert A.shape == (48, 40)
        Sl = np.linalg.svd(A, compute_uv=False)
        worst = max(worst, float(np.abs(Sl.astype(fi.LD) - S).max()) / (np.sqrt(48) * fi.U * float(S[0])))
    print(f"LAPACK worst ratio {worst:.4f}; 8 x = {8 * worst:.3f}; C_SVD = {fi.C_SVD}")
    assert fi.C_SVD == np.ceil(80 * fi.LAPACK_SVD_RATIO) / 10             # 8 x the recorded ratio, rounded up
    assert fi.C_SVD / 16 <= worst <= 1.5 * fi.C_SVD / 8, worst            # (LAPACK builds and thread counts move it by percents)


def test_qr_builders_and_the_constant_of_the_qr_bound():
    worst, conds = 0.0, {}
    for c in fi.qr_cases():
        A, Qx, Rx, cond = fi.qr_matrix(c.m, c.n, c.log2grade)
        assert np.abs(np.tril(Rx, -1)).max() == 0 and np.all(np.diag(Rx) > 0)
        if c.n <= 256:                                                    # (longdouble products of the large ones take seconds)
            assert np.abs(Qx.T @ Qx - np.eye(c.n)).max() < 4 * 2.0 ** -64    # orthonormal to longdouble rounding
            assert np.abs(Qx @ Rx - A).max() <= 8 * 2.0 ** -64 * np.abs(A).max()
        Q, R = fi.lapack_qrpos(A)
        er = float(np.abs(R.astype(fi.LD) - Rx).max() / np.abs(Rx).max())
        eq = float(np.abs(Q.astype(fi.LD) - Qx).max())
        worst = max(worst, er / (fi.U * cond), eq / (fi.U * cond))
        conds.setdefault(c.log2grade, []).append(cond)
    assert all(1e1 < x < 1e3 for x in conds[3]) and all(1e5 < x < 1e7 for x in conds[16]) and all(1e9 < x < 1e11 for x in conds[32]), conds
    print(f"LAPACK worst ratio {worst:.4f}; 8 x = {8 * worst:.3f}; C_QR = {fi.C_QR}")
    assert fi.C_QR == np.ceil(80 * fi.LAPACK_QR_RATIO) / 10
    assert fi.C_QR / 16 <= worst <= 1.5 * fi.C_QR / 8, worst


def test_the_checks_accept_lapack_and_reject_a_wrong_factor():
    """the assertions of the GPU tests, run on LAPACK's factors: they pass, and a swapped pair of columns, a lost singular
    value or a factor off by 1e-11 does not"""
    c = fi.SvdCase(256, 256, "int")
    A, S, _ = fi.svd_matrix(256, 256, "int")
    Uf, Sl, Vh = np.linalg.svd(A)
    assert fi.check_svd_factors(c, Uf, Sl, Vh) == []
    S2 = Sl.copy(); S2[100] *= 1 + 1e-11
    assert any("S_exact" in b for b in fi.check_svd_factors(c, Uf, S2, Vh))
    U2 = Uf.copy(); U2[:, [3, 4]] = U2[:, [4, 3]]
    assert any("(U S) Vh" in b for b in fi.check_svd_factors(c, U2, Sl, Vh))
    q = fi.QrCase(192, 130, 3)
    Q, R = fi.lapack_qrpos(fi.qr_matrix(192, 130, 3)[0])
    assert fi.check_qr_factors(q, Q, R) == []
    R2 = R.copy(); R2[5, 70] += 1e-11 * np.abs(R).max()
    assert any("R_exact" in b for b in fi.check_qr_factors(q, Q, R2))
    assert any("diag" in b for b in fi.check_qr_factors(q, -Q, -R))


# ------------------------------------------------------------------------------------------------------------------
# the Householder route and the complex gauge steps (tests/test_gpu_house_exact.py)
# ------------------------------------------------------------------------------------------------------------------
TALL = [c for c in fi.house_cases() if c.family == "stacked"]


def test_house_plan_lines_are_still_in_the_library_and_every_case_is_on_its_route():
    """house_plan() restates the host lines of qrpos() in mpsk_gauge.hip and the two dispatch conditions of mpsk_api_factor.hip"""
    g = open(os.path.join(CSRC, "mpsk_gauge.hip")).read()
    api = open(os.path.join(CSRC, "mpsk_api_factor.hip")).read()
    for line in ("constexpr int QR_T = 512;", "constexpr int QR_NW = QR_T / 64;", "constexpr int QR_NBI = 8;",
                 "constexpr int QR_NB = 32;", "constexpr int QR_LDS_DOUBLES = 19968;", "constexpr int QR_SCRATCH = 32 * QR_NW;",
                 "if (m > QR_LDS_DOUBLES - QR_SCRATCH) {", "const int nbo = (n - j0 < QR_NB) ? n - j0 : QR_NB;",
                 "const int PS = m - j0;", "int nbi = (QR_LDS_DOUBLES - QR_SCRATCH) / PS;", "if (nbi > QR_NBI) nbi = QR_NBI;"):
        assert line in g, line
    assert 19968 - 32 * (512 // 64) == fi.QR_PANEL_DOUBLES == fi.HOUSE_MAX_ROWS
    for line in ("if (c->qr_mode != 1 && n > 64) {", "if (c->qr_mode == 1 || n <= 64) {", "const int m2 = 2 * m, n2 = 2 * n;",
                 "if (defect <= 1.0e-13 * std::sqrt((double)n2)) {"):
        assert line in api, line
    cases = fi.house_cases()
    assert len({c.name for c in cases}) == len(cases) == 39
    for c in cases:
        assert fi.house_route(c) == c.route, (c.name, fi.house_route(c))
        assert c.householder == (c.route != "cholqr")
    real = {(c.m, c.n): fi.house_plan(c.m, c.n) for c in fi.house_real_cases()}
    assert all(n <= 64 for _, n in real) and all(c.n > 64 and c.mode == 1 for c in fi.house_mode1_cases())
    # the branches the ids name: nbi below 8 from 2465 rows on, 1 above 9856, a change between outer blocks, ragged
    # inner panels (also narrower than one panel), ragged and exact outer blocks, a block of one column, the row limit
    assert fi.house_plan(2464, 16) == ((0, 16, 8, False),) and real[(2465, 16)] == ((0, 16, 7, True),)
    assert real[(2465, 40)] == ((0, 32, 7, True), (32, 8, 8, False))
    assert real[(5000, 12)] == ((0, 12, 3, False),) and real[(5000, 13)] == ((0, 13, 3, True),)
    assert fi.house_plan(9856, 5)[0][2] == 2 and real[(10000, 5)] == ((0, 5, 1, False),)
    assert real[(19712, 3)] == ((0, 3, 1, False),) and max(m for m, _ in real) == fi.HOUSE_MAX_ROWS
    assert real[(9, 8)] == ((0, 8, 8, False),) and real[(17, 9)] == ((0, 9, 8, True),)
    assert real[(40, 31)] == ((0, 31, 8, True),) and real[(64, 32)] == ((0, 32, 8, False),)
    assert real[(65, 33)] == ((0, 32, 8, False), (32, 1, 8, True))
    assert {n for _, n in real} >= {1, 2, 4} and {33, 37, 63} <= {n for _, n in real} and (2465, 16) in real    # transposes
    assert (129, 65) in {(c.m, c.n) for c in fi.house_mode1_cases()}
    # complex: 2n = 64 is the last Householder size, 2n = 66 the first on the CholeskyQR ladder; the halved row limit
    cx = {(c.m, c.n, c.log2grade): c for c in fi.house_complex_cases()}
    assert cx[(64, 32, 3)].householder and not cx[(66, 33, 3)].householder and not cx[(130, 65, 3)].householder
    assert cx[(9856, 3, 3)].real_shape == (fi.HOUSE_MAX_ROWS, 6) and cx[(2465, 16, 3)].route == "32/3r"
    for c in fi.house_mode1_cases():                                      # the shapes and grades the C_QR measurement covers
        assert fi.QrCase(c.m, c.n, c.log2grade) in fi.qr_cases()


def test_tall_builder_and_the_constants_of_the_tall_bounds():
    """exactness of A = Q0 R0 is asserted inside qr_stacked (2^50 guard, fp64 == longdouble for every shape); here: the
    stated factors are a QRpos (orthonormal to longdouble rounding, triangular, positive real diagonal, every row stripe of
    a tall input occupied), LAPACK lies inside every bound of every case, and the three constants are 8 x its worst ratio"""
    worst = np.zeros(3)
    for c in TALL:
        A, Qx, Rx, cond = c.matrix()
        assert A.shape == (c.m, c.n) and np.iscomplexobj(A) == c.cplx and Qx.dtype == (np.clongdouble if c.cplx else fi.LD)
        t = c.m // c.n
        assert np.count_nonzero(np.abs(A).sum(axis=1)) == t * c.n       # only the m - t n appended rows are zero
        assert np.abs(np.tril(Rx, -1)).max(initial=0) == 0 and np.all(np.diag(Rx).real > 0) and np.all(np.diag(Rx).imag == 0)
        assert np.abs(Qx.conj().T @ Qx - np.eye(c.n)).max() <= max(c.m, 4) * 2.0 ** -64     # (a longdouble sum of m equal terms)
        assert np.abs(Qx @ Rx - A).max() <= 8 * 2.0 ** -64 * np.abs(A).max()
        lo, hi = {3: (1, 1e3), 16: (1e4, 1e7), 32: (1e9, 1e11)}[c.log2grade]
        assert lo <= cond < hi, (c.name, cond)
        Q, R = fi.lapack_qrpos(A)
        assert fi.check_house_factors(c, Q, R) == [], c.name
        worst = np.maximum(worst, fi.house_ratios(c, Q, R))
    for c in fi.house_mode1_cases():                                      # LAPACK stays inside C_QR at the mode 1 shapes
        Q, R = fi.lapack_qrpos(c.matrix()[0])
        assert fi.check_house_factors(c, Q, R) == [], c.name
    print(f"LAPACK worst ratios (factor, orthogonality, residual) {worst}; 8 x = {8 * worst}")
    for const, ratio, w in ((fi.C_QR_TALL, fi.LAPACK_QR_TALL_RATIO, worst[0]), (fi.C_ORTH_TALL, fi.LAPACK_ORTH_TALL_RATIO, worst[1]),
                            (fi.C_RES_TALL, fi.LAPACK_RES_TALL_RATIO, worst[2])):
        assert const == np.ceil(80 * ratio) / 10
        assert const / 16 <= w <= 1.5 * const / 8, (const, w)


def _numpy_householder(A, skip=None):
    """unblocked Householder QRpos in the order of qr_block_kernel; skip = (c, k): reflector c is not applied to column k"""
    W = A.astype(np.float64).copy()
    m, n = W.shape
    Q = np.eye(m)
    for c in range(n):
        x = W[c:, c].copy()
        sigma = float(x[1:] @ x[1:])
        if sigma == 0.0:
            continue
        beta = -np.copysign(np.sqrt(x[0] ** 2 + sigma), x[0])
        v = x / (x[0] - beta)
        v[0] = 1.0
        tau = (beta - x[0]) / beta
        cols = [k for k in range(c, n) if skip != (c, k)]
        W[c:, cols] -= tau * np.outer(v, v @ W[c:, cols])
        Q[:, c:] -= tau * np.outer(Q[:, c:] @ v, v)
    R = np.triu(W[:n])
    sg = np.where(np.diag(R) < 0, -1.0, 1.0)
    return Q[:, :n] * sg, sg[:, None] * R


def test_the_house_checks_reject_plausible_wrong_factorizations():
    case = next(c for c in TALL if (c.m, c.n, c.cplx) == (2465, 16, False))
    assert fi.house_plan(2465, 16) == ((0, 16, 7, True),)                 # panels of 7, 7 and 2 columns
    A = case.matrix()[0]
    Q, R = _numpy_householder(A)
    assert fi.check_house_factors(case, Q, R) == []
    # a dropped row stripe: one row at index >= 512 (the second trip of a 512-thread loop) never read
    A1 = A.copy()
    r = 512 + int(np.flatnonzero(np.abs(A[512:]).sum(axis=1))[0])
    A1[r] = 0.0
    bad = fi.check_house_factors(case, *fi.lapack_qrpos(A1))
    assert any("factor error" in b for b in bad) and any("Q R - A" in b for b in bad), bad
    # the same input, and the last column of the ragged panel (column 15) left unreflected by its neighbour
    bad = fi.check_house_factors(case, *_numpy_householder(A1, skip=(14, 15)))
    assert any("Q R - A" in b for b in bad), bad
    bad = fi.check_house_factors(case, *_numpy_householder(A, skip=(14, 15)))     # (alone it is caught too)
    assert any("Q R - A" in b for b in bad) and any("factor error" in b for b in bad), bad
    # one column's sign fix omitted
    for c in (case, next(c for c in TALL if (c.m, c.n, c.cplx) == (9, 8, False))):
        Q, R = fi.lapack_qrpos(c.matrix()[0])
        Q2, R2 = Q.copy(), R.copy()
        Q2[:, 5] *= -1; R2[5] *= -1
        bad = fi.check_house_factors(c, Q2, R2)
        assert any("diag(R) not positive" in b for b in bad) and any("factor error" in b for b in bad), bad
    # complex: conj(Q); an LQ whose factors were transposed back without the conjugate; an imaginary rounding error left on
    # the diagonal of R; an entry of rounding size below the diagonal
    cc = next(c for c in TALL if (c.m, c.n, c.cplx) == (40, 31, True))
    Ac = cc.matrix()[0]
    Q, R = fi.lapack_qrpos(Ac)
    assert fi.check_house_factors(cc, Q, R) == []
    bad = fi.check_house_factors(cc, Q.conj(), R)
    assert any("factor error" in b for b in bad) and any("Q R - A" in b for b in bad), bad
    L, Ql = R.T, Q.T                                                      # of A^H = L Ql: should be R^H, Q^H
    assert np.abs(L @ Ql - Ac.conj().T).max() > 0.1
    bad = fi.check_house_factors(cc, Ql.conj().T, L.conj().T, "lqpos")
    assert any("factor error" in b for b in bad), bad
    R2 = R.copy(); R2[7, 7] += 1j * 2.0 ** -60 * abs(R[7, 7])
    assert [b for b in fi.check_house_factors(cc, Q, R2) if "imag(diag(R))" in b]
    assert not [b for b in fi.check_house_factors(cc, Q, R2) if "factor error" in b]     # (only the exact condition sees it)
    R2 = R.copy(); R2[8, 7] = 2.0 ** -60
    assert [b for b in fi.check_house_factors(cc, Q, R2) if "tril" in b]
