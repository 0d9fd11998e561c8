"""Every tile, loader and split path of the GEMM core (mpsk_gemm.hip) against an exact reference.

The four tiles are forced through mpsk_ctx_force_tile; the inputs of tests/exact_inputs.py make the result exact (small
integers, dyadic scalars), so the comparison is np.array_equal and a defect shows in the one tile / transpose / loader /
share that has it.  One Gaussian case per tile and transpose is held to the componentwise gamma_K bound.  The knobs the
library reads once at load time (MPSK_SPLITK, MPSK_XCDGRID, MPSK_SPLITK_F, MPSK_STREAMK) are covered by running the
whole list again in a fresh child process per setting (tests/gemm_tile_runner.py).

Kernel families reached (gemm_f64_kernel<BM, BN, TA, TB, ALIGNED> unless noted), per forced tile:
  aligned  : ALIGNED = true, NN / TN / NT / TT, ld == rows and rows + 2
  ragged   : ALIGNED = false, NN / TN / NT / TT, partial tiles in M and N, K tail, ld odd and rows + 3
  shortk   : K < BK, K == BK, K == BK + 1 (one k-tile, prologue-only paths of both accumulate loops), NN / TT
  edges    : M, N one below / on / one above the 64 and 128 tile widths
  cbuf     : padding rows of C untouched (ldc = M + 5); beta == 0 never reads C (NaN-filled)
  complex  : mpsk_gemm under MPSK_C128 = cx_embed + ONE real GEMM with TB = false: NN / TN kernels at 2M x N x 2K
  splitk   : gemm_sk_f64_kernel<64, 64, *, *, *> + gemm_sk_fixup_kernel<64, 64> when the heuristic (or MPSK_SPLITK_F
             in a child: even shares f = 2, 4 -> sk_split_major; uneven f = 3 -> slot == share index) splits: NN / TN
             aligned at the three shapes of the issue, NT / TT unaligned at 193 x 131 x 1109 (KT = 70)
  streamk  : gemm_sk_f64_kernel<128, 128, false, false, true> + gemm_sk_fixup_kernel<128, 128> (child, MPSK_STREAMK=1)
The tagged dac_gemm* / *_zs bodies and cgemm_f64_kernel are not reachable through mpsk_gemm: tests/test_gpu_ops_tiles.py."""
import json
import os
import subprocess
import sys
import time
from dataclasses import replace

import pytest

import exact_inputs as ei

pytestmark = pytest.mark.gpu

RUNNER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_tile_runner.py")
GROUPS = list(ei.gemm_case_groups())


@pytest.mark.parametrize("tile", ei.TILES, ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("group", GROUPS)
def test_gemm_tile(be, group, tile):
    cases = [replace(c, tile=tuple(tile)) for c in ei.gemm_case_groups()[group]]
    try:
        bad = ei.run_gemm_cases(be, cases)
    finally:
        be.lib.mpsk_ctx_force_tile(be.ctx, 0, 0)           # process-wide knob: never leave a tile forced
    assert not bad, (len(bad), bad[:5])


def test_gemm_splitk_default_heuristic(be):
    """Long-K shapes on the automatic 64x64 tile.  Whether the cost model splits is not observable through the ABI
    (mpsk_prof_* records the tagged matvec launches only), so only the result is asserted here; the forced splits run in
    the child processes below."""
    bad = ei.run_gemm_cases(be, ei.splitk_cases())
    assert not bad, bad


# one fresh interpreter per load-time setting; (environment, case set, time limit in s).  Limits: 5x the wall time of the
# first measured run of each child on an MI355X (interpreter start, torch import and context creation included):
#   tiles list 4.2 - 4.4 s (334 cases), stream-K 2.2 s
LIMIT_TILES, LIMIT_STREAMK = 22, 11
CHILDREN = [({"MPSK_SPLITK": "0"}, "tiles", LIMIT_TILES),
            ({"MPSK_XCDGRID": "0"}, "tiles", LIMIT_TILES),
            ({"MPSK_SPLITK_F": "2"}, "tiles", LIMIT_TILES),       # even shares: (256, 128, 4096) has KT = 256
            ({"MPSK_SPLITK_F": "3"}, "tiles", LIMIT_TILES),       # uneven shares: K = 1600 -> KT = 100 = 34 + 34 + 32
            ({"MPSK_SPLITK_F": "4"}, "tiles", LIMIT_TILES),
            ({"MPSK_STREAMK": "1"}, "streamk", LIMIT_STREAMK)]    # M = N = 1536, K = 1024: Tb = 144, Ub / 512 = 18


def test_gemm_load_time_knobs_in_child_processes(be):
    """The case list under every load-time knob, one child at a time (the parent holds the GPU too: two processes at
    most).  A child that dies by a signal, aborts, or runs into its time limit fails the test AND ends the loop: nothing
    more is started on a device that may be in trouble."""
    failures, walls = [], {}
    for extra, which, limit in CHILDREN:
        tag = ",".join(f"{k}={v}" for k, v in extra.items())
        env = dict(os.environ)
        for k in ("MPSK_SPLITK", "MPSK_XCDGRID", "MPSK_SPLITK_F", "MPSK_STREAMK"):
            env.pop(k, None)
        env.update(extra)
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
        if p.returncode != 0 or rec["n_mismatches"] or rec["cases"] == 0:
            failures.append((tag, rec))
    print("child wall times (s):", walls)
    assert not failures, failures
