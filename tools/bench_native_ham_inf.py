"""Timings behind the "VUMPS and TDVP on interleaved storage" tables of the README (profiles/native_ham_inf_timings.json),
d = 2, D = 256 and 1024, transverse-field Ising model (W = 3), interleaved complex128:
  (a) reg_op: one application of the regularised operator of an identity level of NativeMPOHamInfEnv, x -> x - reg(T x), by
      its two routes: fused (the pass-through transfer + ONE mpsk_regularize_axpby) and composed (the transfer + dotc with
      the uploaded conj(lvec^T) + three mpsk_vaxpby_c).  This decides native_cplx.REG_FUSED_DEFAULT.
  (b) regularize_axpby: the entry alone, in GB/s over the bytes it must move (y, x, lvec, rvec read once, out written once:
      80 D^2 bytes for one complex slab).  Every operand fits the 256 MiB Infinity Cache at these sizes: the figure is a
      cache-resident rate, not an HBM rate.
  (c) vumps_iteration / tdvp_step: one VUMPS iteration and one TDVP step (dt = 0.05) on a NativeInfiniteMPS against the same
      step on the bond-embedded InfiniteMPS of cplx.py, wall time with the device drained, and the bytes of state +
      environments of both.
      The embedded real-time step runs the general Arnoldi exponentiator on 2D x 2D tensors and took 49 s at D = 256; the
      drivers are therefore timed at --driver-D (default 256 only), and every row is printed and saved as soon as it exists.
(a), (b): windows of 20 asynchronous calls between two device events, the variants alternating window by window, median of
9 windows after warm-up (tools/bench_correlator.py).
Usage: python tools/bench_native_ham_inf.py [--D 256 1024] [--driver-D 256] [--out FILE] [--no-drivers]"""
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
from mpskit_jl_amd import algorithms as al, krylov, native_cplx as nc  # noqa: E402
from bench_correlator import BATCH, alternate_ms  # noqa: E402


def reg_timing(be, D):
    rng = np.random.default_rng(D)
    z = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    A = be.upload_c(np.linalg.qr(z(2 * D, D))[0].reshape(D, 2, D))                 # a left isometry
    C = z(D, D)
    C /= np.linalg.norm(C)
    c = be.upload_c(C)
    lvec, rvec = be.gemm_c(c, c, transB=True), be.upload_c(np.eye(D, dtype=np.complex128))
    x, out = be.upload_env_c([z(D, 1, D)]), be.empty(1, 2 * D, D)
    cell = lambda v: be.transfer_left(None, v, A, A, cplx=True)
    fused, composed = nc._RegOp(be, cell, lvec, rvec, True), nc._RegOp(be, cell, lvec, rvec, False)
    a = be.download(fused(x, out)).reshape(-1)
    b = be.download(composed(x, be.empty(1, 2 * D, D))).reshape(-1)
    t = alternate_ms(be, [lambda: fused(x, out), lambda: composed(x, out)], BATCH)
    rows = [{"what": "reg_op", "D": D, "dtype": "c128", "fused_ms": t[0], "composed_ms": t[1], "composed_over_fused": t[1] / t[0],
             "max_rel_difference": float(np.abs(a - b).max() / np.abs(b).max()),
             "note": "composed synchronises once per application (the dotc coefficient is read on the host)"}]
    y = cell(x)
    alone = alternate_ms(be, [lambda: be.regularize_axpby(y, lvec, rvec, a1=-1.0, x=x, a0=1.0, out=out, cplx=True)] * 2, BATCH)
    ms = min(alone)
    rows.append({"what": "regularize_axpby", "D": D, "W": 1, "dtype": "c128", "ms": ms, "bytes": 80 * D * D,
                 "GB_per_s": 80 * D * D / ms / 1e6, "note": "operands resident in the Infinity Cache"})
    return rows


def _embedded_step(psi, H, dt, alg, envs):
    be, n = psi.be, len(psi)
    ws = krylov.KrylovWorkspace(be)
    newAL = []
    for loc in range(n):
        ac = al.integrate(be, mk.ddAC(loc, psi, H, envs), psi.AC[loc], 0.0, dt, alg, ws, True)
        c = al.integrate(be, mk.ddC(loc, psi, H, envs), psi.CR[loc], 0.0, dt, alg, ws, True)
        newAL.append(al.regauge(be, ac, c, True))
    psi2 = mk.InfiniteMPS.from_AL(newAL, psi.CR[n - 1], tol=alg.tolgauge, maxiter=alg.gaugemaxiter, be=be, cplx=True)
    envs.recalculate(psi2)
    return psi2, envs


def _wall(be, fn):
    be.synchronize()
    t0 = time.perf_counter()
    r = fn()
    be.synchronize()
    return 1e3 * (time.perf_counter() - t0), r


def driver_timing(be, D):
    H = mk.transverse_field_ising(1.0, 0.7, be=be)
    rng = np.random.default_rng(D + 1)
    A = rng.standard_normal((D, 2, D)) + 1j * rng.standard_normal((D, 2, D))
    nat, emb = nc.NativeInfiniteMPS([A], be=be), mk.InfiniteMPS.from_tensors([A], be=be)
    one = mk.VUMPS(tol=0.0, maxiter=1)
    rows = []
    nat, nenv, _ = mk.find_groundstate(nat, H, one)                                  # warm-up: tables, workspace, environments
    emb, eenv, _ = mk.find_groundstate(emb, H, one)
    tn, (nat, nenv, _) = _wall(be, lambda: mk.find_groundstate(nat, H, one, nenv))
    te, (emb, eenv, _) = _wall(be, lambda: mk.find_groundstate(emb, H, one, eenv))
    emb_bytes = 8 * sum(t.size for k in ("AL", "AR", "AC", "CR") for t in getattr(emb, k))
    emb_env = 8 * sum(t.size for lv in eenv.lw + eenv.rw for t in lv)
    rows.append({"what": "vumps_iteration", "D": D, "W": H.odim, "interleaved_ms": tn, "embedded_ms": te,
                 "embedded_over_interleaved": te / tn, "interleaved_state_bytes": nat.bytes(), "interleaved_env_bytes": nenv.bytes(),
                 "embedded_state_bytes": emb_bytes, "embedded_env_bytes": emb_env})
    alg = mk.TDVP()
    tn, (nat, nenv) = _wall(be, lambda: mk.timestep(nat, H, 0.0, 0.05, alg, nenv))
    te, (emb, eenv) = _wall(be, lambda: _embedded_step(emb, H, 0.05, alg, eenv))
    rows.append({"what": "tdvp_step", "D": D, "W": H.odim, "dt": 0.05, "interleaved_ms": tn, "embedded_ms": te,
                 "embedded_over_interleaved": te / tn})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--driver-D", type=int, nargs="*", default=[256])
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-drivers", action="store_true")
    a = ap.parse_args()
    be = mk.Backend(0)
    rows = []

    def save():
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
                f.write("\n")
    for D in a.D:
        for r in reg_timing(be, D):
            rows.append(r)
            print(json.dumps(r), flush=True)
        save()
    if not a.no_drivers:
        for D in a.driver_D:
            for r in driver_timing(be, D):
                rows.append(r)
                print(json.dumps(r), flush=True)
            save()
    be.close()


if __name__ == "__main__":
    main()
