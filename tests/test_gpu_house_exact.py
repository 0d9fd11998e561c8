"""The blocked Householder QRpos (qrpos() in mpsk_gauge.hip: qr_block_kernel, wy_solve_kernel, set_identity_kernel,
qr_finish_kernel, transpose_kernel behind LQpos) and the complex gauge steps (qrpos_c128 / lqpos_c128 in mpsk_api_factor.hip:
cx_embed_kernel, cx_half_kernel, cx_ctranspose_kernel) on inputs whose factors are known exactly
(tests/exact_factor_inputs.py: qr_stacked, house_cases).

Each case id names the outer blocks "nbo/nbi" the kernels run ("r": ragged last inner panel) or "cholqr" where the
dispatcher takes the CholeskyQR ladder; tests/test_exact_factor_inputs_cpu.py pins the ids to house_plan(), the mirror of
the host lines, and here the route is read from the library's own counters (qr_stats): exactly one Householder run per
real factorization, no CholeskyQR and no fallback; exactly one inner real factorization per well-conditioned complex one.

Bounds.  None comes from the kernels: C_QR_TALL / C_ORTH_TALL / C_RES_TALL x sqrt(m) u (x cond resp. max|R|) with the
constants 8 x the worst ratio of LAPACK with the sign fix on the same inputs (1.9, 25.1, 12.1); the mode 1 shapes are
the qr_matrix inputs under C_QR.  Degenerate inputs: expectations follow from the algorithm (a column that is already
e_j times a number is not reflected: tau = 0; the sign fix then makes the diagonal positive).

Repair branch of qrpos_c128 (test_degenerate_columns_complex): with a zero column and a column that is i times another
one the embedding has a rank deficiency of 4, the completion of Q_E by the real kernels is no embedding, and the call DOES
take the repair branch: 2 inner factorizations at 70 x 20 (Householder route of the embedding, both Householder), 3 at
70 x 40 (the ladder: CholeskyQR3 fails, cholqr_robust; one Householder run that shows the rank; CholeskyQR3 of the
repaired input).  The counts are printed by the test; only the result is asserted.

Found by this test and fixed with it: the repair branch took the structured part of Q_E, orthonormalised it again and set
R = triu(Q^H A).  With exactly dependent columns IN FRONT of other columns that is wrong: the plane of a completed pair
is not invariant under J, every later column is orthogonalised against it, the structured part no longer spans what the
leading columns of A span, and triu() drops weight: at 70 x 20 the call returned |Q R - A| = 6e-3 max|R| (7.2e12 x the
bound) with Q orthonormal.  qrpos_c128 now reads the rank from the diagonal of the Householder factor, replaces the
dependent columns by fixed independent ones -- the QRpos of that input is unique, hence an embedding, and spans the same
spaces at every other column -- and takes R = triu(Q^H A) from its Q: |Q R - A| = 0.40 / 0.12 x sqrt(m) u max|R| at
70 x 20 / 70 x 40.  Inputs without an exactly dependent column take the branch as before."""
import numpy as np
import pytest

import exact_factor_inputs as fi
from mpskit_jl_amd import MpskError

pytestmark = pytest.mark.gpu


@pytest.fixture
def qrmode(be):
    """be with the default qr mode restored afterwards"""
    try:
        yield be
    finally:
        be.set_qr_mode(0)


def _moved(s0, s1):
    return {k: s1[k] - s0[k] for k in s1 if s1[k] != s0[k]}


@pytest.mark.parametrize("case", fi.house_real_cases() + fi.house_mode1_cases(), ids=lambda c: c.name)
def test_real_qrpos_lqpos(qrmode, case):
    """every real case through qrpos, its transpose through lqpos (transpose_kernel: ragged tiles at 1 .. 4, 33, 37, 63, 65,
    2465); the route: one Householder run per call and nothing else"""
    bad, s0, s1, s2 = fi.run_house_case(qrmode, case)
    print(f"{case.name}: counters moved by {_moved(s0, s1)} (qrpos), {_moved(s1, s2)} (lqpos)")
    assert not bad, bad
    assert _moved(s0, s1) == {"householder": 1} and _moved(s1, s2) == {"householder": 1}, (s0, s1, s2)


@pytest.mark.parametrize("case", fi.house_complex_cases(), ids=lambda c: c.name)
def test_complex_qrpos_lqpos(qrmode, case):
    """every complex case through qrpos_c, its conjugate transpose through lqpos_c.  At cond ~ 1e2 a call makes exactly one
    inner real factorization (two would be the repair branch), on the rung the id names and without a fallback."""
    bad, s0, s1, s2 = fi.run_house_case(qrmode, case)
    print(f"{case.name}: counters moved by {_moved(s0, s1)} (qrpos_c), {_moved(s1, s2)} (lqpos_c)")
    assert not bad, bad
    if case.log2grade == 3:
        want = {"householder": 1} if case.householder else {"cholqr3": 1}
        assert _moved(s0, s1) == want and _moved(s1, s2) == want, (s0, s1, s2)
    if case.householder:                                # (a graded input on the ladder may use its later rungs)
        assert fi.inner_factorizations(s0, s1) == 1 and fi.inner_factorizations(s1, s2) == 1


def _second_input(case):
    """another input of the same shape and family: the same case one binade of grading apart"""
    return fi.HouseCase(case.m, case.n, case.log2grade + 1, case.cplx, case.mode, case.family, case.route)


PAIRS = [c for c in fi.house_cases() if not c.cplx and (c.m, c.n, c.log2grade) in {(100, 37, 3), (64, 64, 3), (129, 65, 3)}]


@pytest.mark.parametrize("case", PAIRS, ids=lambda c: c.name)
def test_pairs_on_the_sequential_branch(qrmode, case):
    """qrpos2 / qrlq_pair where they run their two factorizations one after the other (n <= 64, or qr mode 1): both results
    pass the exact check and equal the single calls bit for bit"""
    assert len(PAIRS) == 3 and case.householder
    be, other = qrmode, _second_input(case)
    A1, A2 = case.matrix()[0], other.matrix()[0]
    assert A1.shape == A2.shape and not np.array_equal(A1, A2)
    A2t = np.ascontiguousarray(A2.T)
    be.set_qr_mode(case.mode)
    d1, d2, d2t = be.upload(A1), be.upload(A2), be.upload(A2t)
    Q1, R1 = (be.download(t) for t in be.qrpos(d1))
    Q2, R2 = (be.download(t) for t in be.qrpos(d2))
    L2, Ql2 = (be.download(t) for t in be.lqpos(d2t))
    s0 = be.qr_stats()
    P = [be.download(t) for t in be.qrpos2(d1, d2)]
    s1 = be.qr_stats()
    G = [be.download(t) for t in be.qrlq_pair(d1, d2t)]
    s2 = be.qr_stats()
    bad = fi.check_house_factors(case, P[0], P[1], "qrpos2[0]") + fi.check_house_factors(other, P[2], P[3], "qrpos2[1]")
    bad += fi.check_house_factors(case, G[0], G[1], "qrlq_pair[0]")
    bad += fi.check_house_factors(other, np.ascontiguousarray(G[3].T), np.ascontiguousarray(G[2].T), "qrlq_pair[1]")
    assert not bad, bad
    for got, want in zip(P + G, (Q1, R1, Q2, R2, Q1, R1, L2, Ql2)):
        assert np.array_equal(got, want)
    assert _moved(s0, s1) == {"householder": 2} and _moved(s1, s2) == {"householder": 2}, (s0, s1, s2)


def test_a_deferral_is_consumed_on_the_sequential_branch(qrmode):
    """after qr_defer a qrpos2 at 100 x 37 (n <= 64) is final when it returns; qr_commit has nothing to do, and tsvd -- which
    refuses to run while a deferred factorization is pending -- runs"""
    be = qrmode
    case = next(c for c in fi.house_real_cases() if (c.m, c.n, c.log2grade) == (100, 37, 3))
    other = _second_input(case)
    d1, d2 = be.upload(case.matrix()[0]), be.upload(other.matrix()[0])
    be.qr_defer()
    out = [be.download(t) for t in be.qrpos2(d1, d2)]                   # downloaded BEFORE the commit
    bad = fi.check_house_factors(case, out[0], out[1], "deferred qrpos2[0]")
    bad += fi.check_house_factors(other, out[2], out[3], "deferred qrpos2[1]")
    assert be.qr_commit() == 0
    assert not bad, bad
    Uf, S, Vh, kept, _ = be.tsvd(d1)
    assert kept == 37
    Uf, S, Vh = be.download(Uf), be.download(S), be.download(Vh)
    A = case.matrix()[0]
    assert np.abs((Uf * S) @ Vh - A).max() <= fi.C_SVD * np.sqrt(100) * fi.U * S[0]


def _plain_checks(A, Q, R, cplx=False):
    """orthogonality and residual of a factorization without exact factors, in the units of C_ORTH_TALL / C_RES_TALL; the
    scale max|R| is LAPACK's on the same input"""
    m, n = A.shape
    ldt = np.clongdouble if cplx else fi.LD
    Ql, Rl = Q.astype(ldt), R.astype(ldt)
    su = np.sqrt(m) * fi.U
    rmax = float(np.abs(np.linalg.qr(A)[1]).max())
    eo = float(np.abs(Ql.conj().T @ Ql - np.eye(n)).max()) / su
    ea = float(np.abs(Ql @ Rl - A.astype(ldt)).max()) / (su * rmax)
    return eo, ea, rmax


def test_degenerate_columns_real(be):
    m, n = 70, 40
    # all zero: no column is reflected (sigma == 0, alpha == 0)
    s0 = be.qr_stats()
    Q, R = (be.download(t) for t in be.qrpos(be.upload(np.zeros((m, n)))))
    assert np.array_equal(R, np.zeros((n, n))) and np.array_equal(Q, np.eye(m, n))
    # sigma == 0 with a negative alpha in every column: R = diag(1 .. n) and Q = [-I; 0] after the sign fix
    A = np.zeros((m, n))
    A[:n, :n] = -np.diag(np.arange(1.0, n + 1))
    Q, R = (be.download(t) for t in be.qrpos(be.upload(A)))
    assert np.array_equal(R, np.diag(np.arange(1.0, n + 1))) and np.array_equal(Q, -np.eye(m, n))
    assert np.array_equal(Q @ R, A)
    # a zero column and a duplicated column inside a full stacked input
    A = fi.qr_stacked(m, n, 3)[0].copy()
    A[:, 11] = 0.0
    A[:, 29] = A[:, 5]
    Q, R = (be.download(t) for t in be.qrpos(be.upload(A)))
    assert _moved(s0, be.qr_stats()) == {"householder": 3}
    assert np.all(np.isfinite(Q)) and np.all(np.isfinite(R)) and np.abs(np.tril(R, -1)).max() == 0
    eo, ea, rmax = _plain_checks(A, Q, R)
    print(f"zero + duplicated column: |Q^T Q - I| / (sqrt(m) u) = {eo:.3f}, |Q R - A| / (sqrt(m) u max|R|) = {ea:.3f}, "
          f"R[11, 11] = {R[11, 11]:.3e}, R[29, 29] = {R[29, 29]:.3e}")
    assert eo <= fi.C_ORTH_TALL and ea <= fi.C_RES_TALL
    assert np.all(np.diag(R) >= 0) and abs(R[29, 29]) <= fi.C_RES_TALL * np.sqrt(m) * fi.U * rmax


@pytest.mark.parametrize("n", [20, 40])
def test_degenerate_columns_complex(be, n):
    """a zero column and a column that is i times another one: the embedding loses rank 4.  n = 20: Householder route of
    the embedding; n = 40: the CholeskyQR ladder.  Either may take the repair branch (two inner factorizations)."""
    m = 70
    A = fi.qr_stacked(m, n, 3, True)[0].copy()
    A[:, 11] = 0.0
    A[:, 17] = 1j * A[:, 5]
    s0 = be.qr_stats()
    Q, R = (be.download_c(t) for t in be.qrpos_c(be.upload_c(A)))
    s1 = be.qr_stats()
    eo, ea, rmax = _plain_checks(A, Q, R, True)
    print(f"complex 70 x {n}, zero column + i x column: {fi.inner_factorizations(s0, s1)} inner factorizations "
          f"({_moved(s0, s1)}); |Q^H Q - I| / (sqrt(m) u) = {eo:.3f}, |Q R - A| / (sqrt(m) u max|R|) = {ea:.3f}, "
          f"R[11, 11] = {R[11, 11]:.3e}, R[17, 17] = {R[17, 17]:.3e}")
    assert np.all(np.isfinite(Q)) and np.all(np.isfinite(R))
    assert np.abs(np.tril(R, -1)).max() == 0 and np.all(np.diag(R).imag == 0) and np.all(np.diag(R).real >= 0)
    assert eo <= fi.C_ORTH_TALL and ea <= fi.C_RES_TALL


SCALED = [c for c in fi.house_cases() if not c.cplx and (c.m, c.n, c.log2grade) in {(100, 37, 32), (129, 65, 3)}]


@pytest.mark.parametrize("case", SCALED, ids=lambda c: c.name)
def test_scale_covariance(qrmode, case):
    """qrpos(2^k A), k = +-300, returns the bits of Q and R scaled by exactly 2^k: every step of the route is a sum, product,
    quotient or square root of quantities that scale by powers of two, and 2^(+-600 - 64) stays in range -- an absolute
    threshold anywhere in the route would break it"""
    assert len(SCALED) == 2
    be, A = qrmode, case.matrix()[0]
    be.set_qr_mode(case.mode)
    Q, R = (be.download(t) for t in be.qrpos(be.upload(A)))
    assert not fi.check_house_factors(case, Q, R)
    for k in (300, -300):
        s0 = be.qr_stats()
        Qk, Rk = (be.download(t) for t in be.qrpos(be.upload(np.ldexp(A, k))))
        assert _moved(s0, be.qr_stats()) == {"householder": 1}
        assert np.array_equal(Qk, Q), k
        assert np.array_equal(Rk, np.ldexp(R, k)), k


def test_row_limit(be):
    """one row above the limit is refused with a message that names it; the same ctx then factors 9 x 8"""
    with pytest.raises(MpskError) as ei:
        be.qrpos(be.zeros(fi.HOUSE_MAX_ROWS + 1, 3))
    assert "row limit" in str(ei.value) and "m <= 19712" in str(ei.value), ei.value
    with pytest.raises(MpskError) as ei:
        be.qrpos_c(be.zeros(2 * (fi.HOUSE_MAX_ROWS // 2 + 1), 3))
    assert "row limit" in str(ei.value) and "complex m <= 9856" in str(ei.value), ei.value
    for case in (c for c in fi.house_cases() if (c.m, c.n) == (9, 8)):
        bad, s0, s1, s2 = fi.run_house_case(be, case)
        assert not bad, bad
