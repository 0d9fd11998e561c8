"""Timings behind the statistical-mechanics quasiparticle table of the README (profiles/qp_statmech_timings.json): one site
of the effective operator and of the two environment updates by their two routes
  - fused:    mpsk_qp_apply (with the half buffer of mpsk_qp_half made once, outside the windows), mpsk_transfer_left_pair,
              mpsk_transfer_right_pair;
  - composed: three mpsk_dAC_proj and two axpby; two mpsk_transfer_left_ex / _right_ex and one axpby
on (a) a sparse W = 5 slice (Heisenberg) at D = 256 and D = 1024, (b) a dense chi = d = 2 slice at the same sizes, (c) a
dense chi = d = 16 slice at D = 256; and one full application of the effective operator (both real parts, the two GMRES
solves included) at D = 256 on the 4 x 4-cluster Ising tensor, with the share of its local term.  Windows of 20
asynchronous calls between two device events, the two routes alternating window by window, median of 9 windows after
warm-up (as tools/bench_window.py); the full application is timed with the host clock around a synchronised call (it reads
scalars back), median of 5 alternating calls.
Usage: python tools/bench_qp_statmech.py [--skip-full] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpskit_jl_amd as mk  # noqa: E402
from mpskit_jl_amd import quasiparticle as qpm  # noqa: E402
from bench_correlator import BATCH, alternate_ms  # noqa: E402


def site_timings(be, name, H, D):
    rng = np.random.default_rng(D)
    d, Wl, Wr = H.d, H.Wl, H.Wr
    env = lambda W: be.upload(rng.standard_normal(W * D * D)).reshape(W, D, D)
    ten = lambda: be.upload(rng.standard_normal((D, d, D)))
    GL, GR, lB, rB, B, AL, AR, Ab = env(Wl), env(Wr), env(Wl), env(Wr), ten(), ten(), ten(), ten()
    half = be.qp_half(H, GL, AL)
    y, y1, y2 = be.empty(D, d, D), be.empty(D, d, D), be.empty(D, d, D)
    ol, ol2, orr, or2 = be.empty(Wr, D, D), be.empty(Wr, D, D), be.empty(Wl, D, D), be.empty(Wl, D, D)

    def apply_fused():
        be.qp_apply(H, GL, GR, B, lB, AR, half, rB, out=y)

    def apply_composed():
        be.dAC_proj(H, GL, GR, B, out=y1)
        be.axpby(1.0, be.dAC_proj(H, lB, GR, AR, out=y2), 1.0, y1)
        be.axpby(1.0, be.dAC_proj(H, GL, rB, AL, out=y2), 1.0, y1)

    def left_fused():
        be.transfer_left_pair(H, lB, AR, GL, B, Ab, out=ol)

    def left_composed():
        be.transfer_left_ex(H, lB, AR, Ab, out=ol)
        be.axpby(1.0, be.transfer_left_ex(H, GL, B, Ab, out=ol2), 1.0, ol)

    def right_fused():
        be.transfer_right_pair(H, rB, AL, GR, B, Ab, out=orr)

    def right_composed():
        be.transfer_right_ex(H, rB, AL, Ab, out=orr)
        be.axpby(1.0, be.transfer_right_ex(H, GR, B, Ab, out=or2), 1.0, orr)

    rows = []
    for what, f, c, a, b in (("qp_apply", apply_fused, apply_composed, y, y1), ("transfer_left_pair", left_fused, left_composed, ol, ol),
                             ("transfer_right_pair", right_fused, right_composed, orr, orr)):
        f()
        ra = be.download(a.reshape(a.size)).copy()
        c()
        rb = be.download(b.reshape(b.size)).copy()
        t = alternate_ms(be, [f, c], BATCH)
        rows.append({"what": what, "slice": name, "Wl": Wl, "d": d, "D": D, "fused_ms": t[0], "composed_ms": t[1],
                     "composed_over_fused": t[1] / t[0], "max_rel_difference": float(np.abs(ra - rb).max() / np.abs(rb).max())})
        print(json.dumps(rows[-1]), flush=True)
    return rows


def full_application(be, D=256, cluster=4):
    O = mk.classical_ising(0.3, cluster=cluster)
    psi = mk.InfiniteMPS.random(O.d, D, np.random.default_rng(2), be=be)
    envs = mk.environments(psi, O, tol=1e-8)
    alg = mk.QuasiparticleAnsatz(solver_tol=1e-8)
    rng = np.random.default_rng(3)
    q = mk.LeftGaugedQP.random(psi, 0.7, rng)
    phi = qpm.MultilineQP([mk.LeftGaugedQP(psi, q.VLs, q.xshapes, 0.7, be.upload(rng.standard_normal(2 * q.N)), 2)], 0.7)
    ctxs = {r: qpm._StatmechContext(mk.MPSMultiline(psi), [envs], alg, r == "fused") for r in ("fused", "composed")}
    out = be.empty(2 * phi.N)
    res = {"what": "effective_operator_application", "tensor": f"classical_ising(0.3, cluster={cluster})", "chi": O[0].shape[0],
           "d": O.d, "D": D, "momentum": 0.7}
    Bs = [[phi.B(k, 0, 0) for k in range(2)]]
    lBs, rBs = ctxs["composed"].qp_envs(0, Bs, 0.7)
    full = {r: [] for r in ctxs}
    local = {r: [] for r in ctxs}
    for it in range(6):
        for r, ctx in ctxs.items():
            be.synchronize()
            t0 = time.perf_counter()
            qpm._statmech_heff(ctx, phi, phi.vec, out)
            be.synchronize()
            t1 = time.perf_counter()
            for k in range(2):
                ctx._local(0, 0, Bs[0][k], lBs[0][k], rBs[0][k])
            be.synchronize()
            t2 = time.perf_counter()
            if it:
                full[r].append((t1 - t0) * 1e3)
                local[r].append((t2 - t1) * 1e3)
    for r in ctxs:
        res[f"{r}_ms"] = statistics.median(full[r])
        res[f"{r}_local_term_ms"] = statistics.median(local[r])
        res[f"{r}_local_share"] = res[f"{r}_local_term_ms"] / res[f"{r}_ms"]
    res["composed_over_fused"] = res["composed_ms"] / res["fused_ms"]
    print(json.dumps(res), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-full", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    be = mk.Backend(0)
    rng = np.random.default_rng(0)
    rows = []
    for D in (256, 1024):
        rows += site_timings(be, "sparse W=5 (Heisenberg)", mk.heisenberg_XXX(0.5, be=be)[0], D)
    for D in (256, 1024):
        rows += site_timings(be, "dense chi=d=2", be.mposlice_dense(rng.random((2, 2, 2, 2))), D)
    rows += site_timings(be, "dense chi=d=16", be.mposlice_dense(rng.random((16, 16, 16, 16))), 256)
    if not a.skip_full:
        rows.append(full_application(be))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")
    be.close()


if __name__ == "__main__":
    main()
