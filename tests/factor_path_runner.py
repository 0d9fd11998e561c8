"""Child-process runner of the SVD / QR case lists (not a test file): `python factor_path_runner.py svd|qr|qr_gemm`.

MPSK_SVD_EIG, MPSK_SVD_INTRA, MPSK_SVD_LAG, MPSK_CQ_TRSM and MPSK_CQ_GRAM are read once per process, so each setting
needs a process of its own: tests/test_gpu_factor_paths.py starts this module with the environment extended by one of
them.  It runs svd_child_cases() or qr_cases() of tests/exact_factor_inputs.py with the accuracy assertions of the
in-process tests (the sweep counts go back to the parent, which compares them with the default plan) and prints ONE JSON line
    {"set": ..., "cases": n, "failures": [...], "n_failures": n, "sweeps": {case: count}, "stats": {...}, "wall_s": ...}
"qr_gemm" (meant for MPSK_CQ_TRSM=0) adds the inputs that send cholqr_robust, the shift retry and the two-stream pair
through the GEMM route.  Exit status 0 when every case passed, 1 otherwise."""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def gemm_route_extras(be, fi):
    """rank-deficient and cond-1e12 inputs, and the qrpos2 pair; bounds: those of tests/test_gpu_ops.py for the same
    properties on the default route (test_qrpos_fallback_counts, test_cholqr_shift_retry, test_qrpos2_pair)"""
    bad = []
    m, n = 257, 256
    A = fi.qr_matrix(m, n, 3)[0].copy()
    A[:, 7] = 0.0
    A[:, 9] = A[:, 3]
    s0 = be.qr_stats()
    Q, R = (be.download(t) for t in be.qrpos(be.upload(A)))
    s1 = be.qr_stats()
    if not (s1["fallback"] == s0["fallback"] + 1 and s1["robust"] == s0["robust"] + 1):
        bad.append(f"rank-deficient input did not take cholqr_robust: {s0} -> {s1}")
    if not (np.abs(Q.T @ Q - np.eye(n)).max() < 1e-12 and relerr(Q @ R, A) < 1e-13
            and np.all(np.diag(R) >= 0) and np.abs(np.tril(R, -1)).max() == 0.0):
        bad.append(f"rank-deficient: |Q^T Q - I| {np.abs(Q.T @ Q - np.eye(n)).max():.2e}, |QR - A| rel {relerr(Q @ R, A):.2e}")
    rng = np.random.default_rng(8)
    m2, n2 = 640, 192
    Uo, _ = np.linalg.qr(rng.standard_normal((m2, n2)))
    Vo, _ = np.linalg.qr(rng.standard_normal((n2, n2)))
    B = (Uo * np.logspace(0, -12, n2)) @ Vo.T
    r0, f0 = be.qr_retries(), be.qr_stats()["fallback"]
    Q, R = (be.download(t) for t in be.qrpos(be.upload(B)))
    if not (be.qr_retries() > r0 or be.qr_stats()["fallback"] > f0):
        bad.append("cond-1e12 input took neither the shift retry nor the robust variant")
    if not (np.abs(Q.T @ Q - np.eye(n2)).max() < 1e-13 and np.abs(Q @ R - B).max() < 1e-14
            and np.all(np.diag(R) > 0) and np.abs(np.tril(R, -1)).max() == 0.0):
        bad.append(f"cond 1e12: |Q^T Q - I| {np.abs(Q.T @ Q - np.eye(n2)).max():.2e}, |QR - A| {np.abs(Q @ R - B).max():.2e}")
    A1 = fi.qr_matrix(m, n, 3)[0]
    Q1, R1, Q2, R2 = (be.download(t) for t in be.qrpos2(be.upload(A1), be.upload(A)))
    Qs, Rs = (be.download(t) for t in be.qrpos(be.upload(A1)))
    Qd, Rd = (be.download(t) for t in be.qrpos(be.upload(A)))
    if not (relerr(Q1, Qs) < 1e-12 and relerr(R1, Rs) < 1e-12):
        bad.append(f"qrpos2 first != single call: Q {relerr(Q1, Qs):.2e} R {relerr(R1, Rs):.2e}")
    # the rank-deficient one: column 7 is zero, so q_7 is an arbitrary completion, every later q_j is orthogonalised against
    # it, and neither Q nor the rows of R from 7 on are unique: there only the product is compared with the single call.
    # The rows above the first zero pivot are determined (r_ij = q_i . a_j with q_0 .. q_6 unique) and must agree.
    rows = np.arange(7)
    if not (relerr(Q2 @ R2, A) < 1e-12 and np.abs(Q2.T @ Q2 - np.eye(n)).max() < 1e-12 and relerr(Q2 @ R2, Qd @ Rd) < 1e-12
            and relerr(R2[rows], Rd[rows]) < 1e-12):
        bad.append(f"qrpos2 rank-deficient: |QR - A| rel {relerr(Q2 @ R2, A):.2e}, R rows above the first zero pivot {relerr(R2[rows], Rd[rows]):.2e}")
    return bad


def main(which):
    t0 = time.time()
    import exact_factor_inputs as fi
    import mpskit_jl_amd as mk
    be = mk.Backend(0)
    bad, sweeps = [], {}
    try:
        if which == "svd":
            cases = fi.svd_child_cases()
            for c in cases:
                b, sw, _ = fi.run_svd_case(be, c)
                bad += b
                sweeps[c.name] = sw
        else:
            cases = fi.qr_cases()
            for c in cases:
                bad += fi.run_qr_case(be, c)
            if which == "qr_gemm":
                bad += gemm_route_extras(be, fi)
        stats = dict(be.qr_stats(), retries=be.qr_retries())
    finally:
        be.close()
    print(json.dumps({"set": which, "cases": len(cases), "failures": bad[:20], "n_failures": len(bad), "sweeps": sweeps,
                      "stats": stats, "wall_s": round(time.time() - t0, 2)}), flush=True)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1] if len(sys.argv) > 1 else "svd"))
