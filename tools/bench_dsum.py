"""Time psi1 + psi2 of two FiniteMPS on the fused route (mpsk_dsum_site: one grouped launch per site step) and on the
composed route (two GEMMs, plus two strided copies on the right half), and dot(psi1, psi2); no thresholds.

    python tools/bench_dsum.py [--L 32] [--d 2] [--D 64,256,1024] [--reps 5] [--out profiles/dsum_timings.json]

Per bond dimension D1 = D2 = D: one warm-up (it also brings the gauges of both addends in place), then the median of --reps
synchronised wall times of the whole sum on each route and of dot; and, because the two factorisations per site dominate the
sum, the site step alone at the bulk shape (Dn = 2 D, D1 = D2 = E1 = E2 = D) on both sides and routes (median of 4 --reps)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mpskit_jl_amd as mk  # noqa: E402
from mpskit_jl_amd import linalg  # noqa: E402


def median_ms(be, fn, reps):
    fn()
    be.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        be.synchronize()
        ts.append(time.perf_counter() - t0)
    return round(1e3 * statistics.median(ts), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=32)
    ap.add_argument("--d", type=int, default=2)
    ap.add_argument("--D", default="64,256,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dsum_timings.json"))
    a = ap.parse_args()
    be = mk.Backend(0)
    rows = []
    for D in [int(x) for x in a.D.split(",")]:
        rng = np.random.default_rng(D)
        psi1 = mk.FiniteMPS.random(a.L, a.d, D, rng, be=be)
        psi2 = mk.FiniteMPS.random(a.L, a.d, D, rng, be=be)
        row = {"L": a.L, "d": a.d, "D1": D, "D2": D, "reps": a.reps}
        for name, fused in (("fused", True), ("composed", False)):
            row[f"add_{name}_ms"] = median_ms(be, lambda: linalg.add(psi1, psi2, fused=fused), a.reps)
        row["dot_ms"] = median_ms(be, lambda: linalg.dot(psi1, psi2), a.reps)
        d = a.d
        G = {"left": be.upload(rng.standard_normal((2 * D, 2 * D))), "right": be.upload(rng.standard_normal((2 * D, 2 * D)))}
        A1, A2 = be.upload(rng.standard_normal((D, d, D))), be.upload(rng.standard_normal((D, d, D)))
        for side, step in (("left", linalg.dsum_left), ("right", linalg.dsum_right)):
            for name, fused in (("fused", True), ("composed", False)):
                row[f"site_{side}_{name}_ms"] = median_ms(be, lambda: step(be, G[side], A1, A2, fused), 4 * a.reps)
        row["site_flops"] = 2 * d * (2 * D) * 2 * D * D
        rows.append(row)
        print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_dsum.py", "rows": rows}, f, indent=1)
        f.write("\n")
    be.close()


if __name__ == "__main__":
    main()
