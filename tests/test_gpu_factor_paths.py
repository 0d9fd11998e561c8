"""Every schedule and route of the block-Jacobi SVD (mpsk_svd.hip) and of CholeskyQR (mpsk_cholqr.hip) on inputs whose
factors are known exactly (tests/exact_factor_inputs.py).

Paths reached (each case id names its plan; tests/test_exact_factor_inputs_cpu.py pins the ids to the plan on the CPU,
and here the library's own MPSK_SVD_DEBUG summary line is parsed to confirm P, Q and the number of chains it used):
  chained tournament  MPSK_SVD_CHAINS = 2 (pc = 2, 4), 3 (P = 6), 4 (pc = 2), 8 (clamped to 4 at P = 16; unchained at
                      P = 8), 2 at P = 5 (unchained); accumulated V (svd mode 3), plain (mode 0: the G and V tables
                      differ) tall / wide with 2 chains and 1024 x 512 with 4, V-free (mpsk_tsplit, mode 2); ragged n = 200, odd rows 257 x 200 (kq_even false);
                      one bit-for-bit repeat per form (a missing barrier is a race)
  Gram K-splits       MPSK_SVD_Q = 1, 3 (falls to 2), 16 and the default at 2048 x 256 plain; complex shapes with
                      Q = 1, 5, 4 and 16 (csvd_plan reads no environment)
  MPSK_SVD_INNER = 3  on a P = 4 case (the debug line reports the inner sweeps the call used)
  children            MPSK_SVD_EIG=1 (jacobi_eig_kernel), MPSK_SVD_INTRA=0 / 1e6, MPSK_SVD_LAG=0 with 2 chains,
                      MPSK_CQ_TRSM=0 (GEMM route: recursive doubling, pair-inverse workgroup, b_upper product; robust,
                      retry and the two-stream pair through it), MPSK_CQ_GRAM=0 (in-step Gram off)

Bounds.  None comes from the kernels.  Singular values and the reconstruction: C_SVD sqrt(max(m, n)) u sigma_max with
C_SVD = 8.2 = 8 x 1.021, the worst ratio numpy.linalg.svd (LAPACK) shows on the same inputs.  QR factors against the exact
ones: C_QR u cond with C_QR = 1.5 = 8 x 0.186, the worst ratio of Householder LAPACK with the sign fix on the same inputs.
Orthogonality 1e-12 (SVD) / 1e-13 (QR) and |Q R - A| < 1e-14 |A|_max are the figures of tests/test_gpu_ops.py.
Sweep counts: a forced schedule or split visits the same block pairs once per sweep, so it may need at most 2 sweeps more
than the default plan on the same input; both counts are printed.

Found by these tests and fixed with them: the sweep loop skipped its verification sweep from max |cos| <= 1e-9 on, which
holds the rounding floor only for separated singular values.  The "graded" family has exact multiplicities (up to 4 at
n = 512), where a sweep shrinks the cosines only by a constant: 512 x 512 in svd mode 3 was left with |U^T U - I| = 1.5e-11
on the default plan and complex 256 x 256 with |Vh Vh^H - I| = 1.8e-12, against the suite's 1e-12.  The loop now skips the
verification sweep only from 1e-12 on (SVD_EXIT_COS in mpsk_svd.hip)."""
import json
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import exact_factor_inputs as fi

pytestmark = pytest.mark.gpu

RUNNER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "factor_path_runner.py")
_default_sweeps = {}
PLAN_LINE = re.compile(r"\[mpsk_tsvd( c128)?\] \d+ x \d+: P=(\d+) Q=(\d+) rounds/sweep=\d+ sweeps=(\d+)(?: chains=(\d+) inner=(\d+))?")


def _clear(monkeypatch):
    for k in fi.setting_names():
        monkeypatch.delenv(k, raising=False)


def _run_with_plan(be, case, monkeypatch, capfd, env):
    """the case under `env` (+ MPSK_SVD_DEBUG): (failures, sweeps, outputs, plan the library reported)"""
    _clear(monkeypatch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("MPSK_SVD_DEBUG", "1")
    capfd.readouterr()
    bad, sweeps, out = fi.run_svd_case(be, case)
    err = capfd.readouterr().err
    lines = PLAN_LINE.findall(err)
    assert lines, f"no plan line from the library: {err[-500:]!r}"
    _, P, Q, sw, nc, inner = lines[-1]
    return bad, sweeps, out, {"P": int(P), "Q": int(Q), "NC": int(nc) if nc else 1, "sweeps": int(sw),
                              "inner": int(inner) if inner else None}


@pytest.mark.parametrize("case", fi.svd_cases(), ids=lambda c: c.name)
def test_svd_path(be, case, monkeypatch, capfd):
    want = fi.svd_plan(case.m, case.n, case.mode, case.envd, case.cplx)
    sw0 = None
    if case.env:                                      # the default plan on the same input, once
        key = case.default()
        if key not in _default_sweeps:
            b0, s0, _, _ = _run_with_plan(be, key, monkeypatch, capfd, {})
            assert not b0, b0
            _default_sweeps[key] = s0
        sw0 = _default_sweeps[key]
    bad, sweeps, _, got = _run_with_plan(be, case, monkeypatch, capfd, case.envd)
    print(f"{case.name}: plan {got}, sweeps {sweeps} (default plan: {sw0})")
    # the C side saw the setting: it reports the plan the mirror predicts
    assert (got["P"], got["Q"], got["NC"]) == (want["P"], want["Q"], want["NC"]), (got, want)
    assert got["sweeps"] == sweeps
    if not case.cplx:                                 # MPSK_SVD_INNER reached the C side (default with P > 1: one inner sweep)
        assert got["inner"] == int(case.envd.get("MPSK_SVD_INNER", 1)), got
    assert not bad, bad
    if sw0 is not None:
        assert sweeps <= sw0 + 2, (sweeps, sw0)


REPEATS = [c for c in fi.chain_cases() if (c.m, c.n, c.family, c.call, c.mode, c.envd[fi.CH]) in
           {(256, 256, "graded", "tsvd", 3, "2"), (512, 512, "int", "tsvd", 3, "4"), (384, 384, "int", "tsvd", 3, "3"),
            (1024, 256, "int", "tsvd", 0, "2"), (200, 200, "int", "tsplit", 2, "2")}]


@pytest.mark.parametrize("case", REPEATS, ids=lambda c: c.name)
def test_chained_run_repeats_bit_for_bit(be, case, monkeypatch, capfd):
    assert len(REPEATS) == 5
    _, s1, out1, p1 = _run_with_plan(be, case, monkeypatch, capfd, case.envd)
    _, s2, out2, p2 = _run_with_plan(be, case, monkeypatch, capfd, case.envd)
    assert p1["NC"] == p2["NC"] == dict(case.plan)["NC"] > 1 and s1 == s2
    for a, b in zip(out1, out2):
        assert np.array_equal(a, b)


def test_rank_deficient_kept_and_disc_under_chains(be, monkeypatch):
    """exact rank 192 of 256 (svd mode 3, two chains): truncerr below the smallest non-zero value keeps exactly the rank and
    discards (numerically) nothing; truncdim below the rank discards exactly the tail"""
    case = next(c for c in fi.chain_cases() if c.family == "rankdef")
    A, Sx, rank = fi.svd_matrix(case.m, case.n, case.family)
    bound = fi.svd_bound(case)
    assert rank == 192 and float(Sx[rank - 1]) > 1e6 * bound
    _clear(monkeypatch)
    monkeypatch.setenv(fi.CH, "2")
    dA = be.upload(A)
    _, S, _, kept, disc = be.tsvd(dA, trunc_err=0.5 * float(Sx[rank - 1]))
    assert kept == rank and disc <= np.sqrt(case.n - rank) * bound, (kept, disc)
    k = rank - 50
    Uf, S, Vh, kept, disc = be.tsvd(dA, max_keep=k)
    tail = float(np.sqrt(np.sum(Sx[k:] ** 2)))
    assert kept == k and abs(disc - tail) <= np.sqrt(case.n - k) * bound, (kept, disc, tail)
    Uf, S, Vh = be.download(Uf)[:, :k], be.download(S), be.download(Vh)[:k]
    assert np.abs(S.astype(fi.LD) - Sx).max() <= bound
    assert np.abs(Uf.T @ Uf - np.eye(k)).max() < 1e-12 and np.abs(Vh @ Vh.T - np.eye(k)).max() < 1e-12


@pytest.mark.parametrize("kind", ["gauss", "graded"])
@pytest.mark.parametrize("mode", [3, 0])
def test_small_gaussian_against_mpmath(be, kind, mode, monkeypatch):
    """unstructured input: 48 x 40 Gaussian and graded Gaussian, singular values from mpmath at 40 digits"""
    _clear(monkeypatch)
    A, Sx = fi.gauss_small(kind), fi.gauss_small_reference(kind)
    bound = fi.C_SVD * np.sqrt(48) * fi.U * float(Sx[0])
    be.set_svd_mode(mode)
    try:
        Uf, S, Vh, kept, disc = be.tsvd(be.upload(A))
    finally:
        be.set_svd_mode(3)
    Uf, S, Vh = be.download(Uf), be.download(S), be.download(Vh)
    assert kept == 40 and np.all(np.diff(S) <= 0)
    assert np.abs(S.astype(fi.LD) - Sx).max() <= bound
    assert np.abs(Uf.T @ Uf - np.eye(40)).max() < 1e-12 and np.abs(Vh @ Vh.T - np.eye(40)).max() < 1e-12
    assert np.abs((Uf * S) @ Vh - A).max() <= bound


@pytest.mark.parametrize("case", fi.qr_cases(), ids=lambda c: c.name)
def test_qr_default_route(be, case, monkeypatch):
    """the in-step solve with the in-step Gram (what the plan picks at these shapes) against the exact factors"""
    _clear(monkeypatch)
    bad = fi.run_qr_case(be, case)                      # (includes: the calls stayed on the CholeskyQR3 route)
    assert not bad, bad


# one fresh interpreter per load-time setting: (environment, case set, time limit in s).  Limits: 5 x the wall time of
# the first measured run of each child on an MI355X (interpreter start, torch import, context creation, the builders
# and the numpy checks included):
#   svd list 4.1 - 6.5 s (11 cases), qr list 2.8 s (11 cases), qr_gemm list 2.9 s
LIMIT_SVD, LIMIT_QR, LIMIT_QR_GEMM = 33, 14, 15
CHILDREN = [({"MPSK_SVD_EIG": "1"}, "svd", LIMIT_SVD),                              # jacobi_eig_kernel
            ({"MPSK_SVD_INTRA": "0"}, "svd", LIMIT_SVD),                            # never skip the intra-block steps
            ({"MPSK_SVD_INTRA": "1e6"}, "svd", LIMIT_SVD),                          # skip whenever allowed: must still converge
            ({"MPSK_SVD_LAG": "0", "MPSK_SVD_CHAINS": "2"}, "svd", LIMIT_SVD),      # chains in lockstep
            ({"MPSK_CQ_TRSM": "0"}, "qr_gemm", LIMIT_QR_GEMM),                      # GEMM route, robust / retry / pair through it
            ({"MPSK_CQ_GRAM": "0"}, "qr", LIMIT_QR)]                                # in-step solve without the in-step Gram


# children whose sweep counts are held to the default plan's + 2 (MPSK_SVD_INTRA=1e6 skips rotations on purpose: it must
# converge, its counts are recorded only)
SWEEPS_HELD = ("MPSK_SVD_EIG=1", "MPSK_SVD_INTRA=0", "MPSK_SVD_LAG=0,MPSK_SVD_CHAINS=2")


def test_load_time_settings_in_child_processes(be, monkeypatch):
    """The case lists under every load-time setting, one child at a time (the parent holds the GPU too: two processes at
    most).  A child that dies by a signal, aborts, or runs into its time limit fails the test AND ends the loop: nothing
    more is started on a device that may be in trouble.  The parent runs the SVD list once on the default plan: a child
    under SWEEPS_HELD may need at most 2 sweeps more per case."""
    _clear(monkeypatch)
    default = {}
    for c in fi.svd_child_cases():
        b0, default[c.name], _ = fi.run_svd_case(be, c)
        assert not b0, b0
    failures, walls, sweeps = [], {}, {}
    for extra, which, limit in CHILDREN:
        tag = ",".join(f"{k}={v}" for k, v in extra.items())
        env = fi.clean_env()
        env.update(extra)
        if "MPSK_SVD_CHAINS" in extra:
            env["MPSK_SVD_DEBUG"] = "1"
        t0 = time.time()
        try:
            p = subprocess.run([sys.executable, RUNNER, which], env=env, timeout=limit, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            failures.append((tag, f"time limit of {limit} s"))
            break
        walls[tag] = round(time.time() - t0, 1)
        if p.returncode < 0 or p.returncode in (134, 139):
            failures.append((tag, f"died with status {p.returncode}", p.stderr[-2000:]))
            break
        try:
            rec = json.loads(p.stdout.strip().splitlines()[-1])
        except (IndexError, ValueError):
            failures.append((tag, f"no record, status {p.returncode}", p.stderr[-2000:]))
            break                                          # (a HIP error surfaces as a Python exception: same rule)
        if p.returncode != 0 or rec["n_failures"] or rec["cases"] == 0:
            failures.append((tag, rec))
        sweeps[tag] = rec["sweeps"]
        if which == "svd":
            print(f"{tag}: sweeps (child / default plan):", {k: (v, default.get(k)) for k, v in rec["sweeps"].items()})
            if set(rec["sweeps"]) != set(default):
                failures.append((tag, "the child ran another case list", sorted(rec["sweeps"])))
            elif tag in SWEEPS_HELD:
                slow = {k: (v, default[k]) for k, v in rec["sweeps"].items() if v > default[k] + 2}
                if slow:
                    failures.append((tag, "more than 2 sweeps above the default plan (child, default)", slow))
        if "MPSK_SVD_CHAINS" in extra and "chains=2" not in p.stderr:
            failures.append((tag, "no call of the child ran with 2 chains"))
        if which == "qr_gemm" and not rec["stats"]["robust"] >= 1:
            failures.append((tag, "cholqr_robust never ran on the GEMM route", rec["stats"]))
    print("child wall times (s):", walls)
    print("child sweep counts:", json.dumps(sweeps))
    assert not failures, failures
