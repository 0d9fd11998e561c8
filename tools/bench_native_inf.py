"""Timings behind the uniform-state table of the README (profiles/native_inf_timings.json), D = 256 and 1024, d = 2, the WII
evolution MPO of the transverse-field Ising model (g = 0.7, dt = 0.05), interleaved complex128:
  - c_proj by its two routes: fused (mpsk_dC_proj_c) and composed (native_cplx.dC_proj_c_composed: two mpsk_gemm under
    MPSK_C128 per MPO level and mpsk_vaxpby);
  - one VOMPS iteration of native_cplx.approximate (per site mpsk_dAC_proj + mpsk_dC_proj_c + regauge, then from_AL,
    recalculate and the Galerkin error), wall time per iteration with the device drained -- the iteration synchronises by
    itself in every eigensolve.  The same step on bond-embedded tensors is not measured here.
c_proj: windows of 20 asynchronous calls between two device events, the two routes alternating window by window, median
of 9 windows after warm-up (as tools/bench_window.py).
Usage: python tools/bench_native_inf.py [--D 256 1024] [--iters 3] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpskit_jl_amd as mk  # noqa: E402
from mpskit_jl_amd import native_cplx as nc  # noqa: E402
from bench_correlator import BATCH, alternate_ms  # noqa: E402


def c_proj_timing(be, D, W):
    rng = np.random.default_rng(D)
    z = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    GL, GR, c = be.upload_env_c([z(D, W, D)]), be.upload_env_c([z(D, W, D)]), be.upload_c(z(D, D))
    y = be.empty(2 * D, D)
    fused = lambda: be.dC_proj_c(GL, GR, c, out=y)
    composed = lambda: nc.dC_proj_c_composed(be, GL, GR, c)
    a, b = be.download(fused()).reshape(-1), be.download(composed()).reshape(-1)
    t = alternate_ms(be, [fused, composed], BATCH)
    return {"what": "c_proj", "D": D, "W": W, "dtype": "c128", "fused_ms": t[0], "composed_ms": t[1],
            "composed_over_fused": t[1] / t[0], "max_rel_difference": float(np.abs(a - b).max() / np.abs(b).max())}


def vomps_timing(be, D, O, iters):
    above = nc.NativeInfiniteMPS.random(2, D, np.random.default_rng(D + 1), be=be)
    below = nc.NativeInfiniteMPS.random(2, D, np.random.default_rng(D + 2), be=be)
    envs = nc.NativePerMPOInfEnv(below, (O, above))
    below, envs, _ = nc.approximate(below, (O, above), mk.VOMPS(tol=0.0, maxiter=1), envs=envs)   # warm-up: tables, workspace
    be.synchronize()
    t0 = time.perf_counter()
    _, envs, eps = nc.approximate(below, (O, above), mk.VOMPS(tol=0.0, maxiter=iters), envs=envs)
    be.synchronize()
    return {"what": "vomps_iteration", "D": D, "W": O.odim, "dtype": "c128", "route": "interleaved",
            "ms_per_iteration": 1e3 * (time.perf_counter() - t0) / iters, "iterations": iters, "eps": eps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    be = mk.Backend(0)
    O = mk.make_time_mpo(mk.transverse_field_ising(1.0, 0.7, be=be), 0.05, mk.WII())
    rows = []
    for D in a.D:
        rows.append(c_proj_timing(be, D, O.odim))
        print(json.dumps(rows[-1]), flush=True)
        rows.append(vomps_timing(be, D, O, a.iters))
        print(json.dumps(rows[-1]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")
    be.close()


if __name__ == "__main__":
    main()
