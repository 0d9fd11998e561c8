"""Time one bond's expansion (optimalexpand.jl:22-32) on the device route (mpsk_dAC2_product + mpsk_complement_tsvd) and on
the composed route (mpsk_dAC2 on the formed product, null-space bases by QRpos / LQpos, full mpsk_tsvd) on identical inputs.

    python tools/bench_expand.py --kind ham --D 1024 --k 64 [--routes device,composed] [--reps 5]
    python tools/bench_expand.py --kind dense --chi 16 --D 256 --k 32 --routes device
    python tools/bench_expand.py --kind grow [--D 256] [--tol 1e-8]

One warm-up, then the median of --reps runs (synchronised wall time per run).  The composed route is skipped (and its
workspace reported) when the two-site mix would need more than --max-gib of workspace.
--kind grow: leading_boundary of the 4 x 4-cluster Ising tensor (beta = 0.3) to --tol at --D, once grown D/4 -> D/2 -> D by
OptimalExpand (each stage converged to 1e-4 first) and once from a random state at D: iterations and wall time of each."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import mpskit_jl_amd as mk  # noqa: E402
from mpskit_jl_amd.changebonds import _complement_directions, _tail_matrix  # noqa: E402


def grow(a):
    be = mk.Backend(0)
    mpo = mk.classical_ising(0.3, cluster=4)
    out = {"kind": "grow", "D": a.D, "tol": a.tol}

    def run(psi, tol, envs=None):
        t0 = time.perf_counter()
        psi, envs, eps = mk.leading_boundary(psi, mpo, mk.VUMPS(tol=tol, maxiter=100, verbosity=3), envs)
        be.synchronize()
        return psi, envs, eps, envs.history[-1][0], time.perf_counter() - t0

    psi = mk.InfiniteMPS.random(16, a.D // 4, np.random.default_rng(1), be=be)
    its, wall, t_exp = [], 0.0, 0.0
    psi, envs, eps, it, t = run(psi, 1e-4)
    its.append(it); wall += t
    for D in (a.D // 2, a.D):
        t0 = time.perf_counter()
        psi, envs = mk.changebonds(psi, mpo, mk.OptimalExpand(trunc_dim=D - psi.CR[0].shape[0]), envs)
        be.synchronize()
        t_exp += time.perf_counter() - t0
        psi, envs, eps, it, t = run(psi, a.tol if D == a.D else 1e-4, envs)
        its.append(it); wall += t
    out["grown"] = {"iterations": its, "vumps_s": round(wall, 3), "expand_s": round(t_exp, 3), "eps": eps,
                    "lambda": float(mk.statmech.expectation_value(psi, mpo, envs)[0])}
    psi = mk.InfiniteMPS.random(16, a.D, np.random.default_rng(1), be=be)
    psi, envs, eps, it, t = run(psi, a.tol)
    out["random_start"] = {"iterations": it, "vumps_s": round(t, 3), "eps": eps,
                           "lambda": float(mk.statmech.expectation_value(psi, mpo, envs)[0])}
    print(json.dumps(out))
    be.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", choices=["ham", "dense", "grow"], default="ham")
    ap.add_argument("--tol", type=float, default=1e-8)
    ap.add_argument("--D", type=int, default=1024)
    ap.add_argument("--chi", type=int, default=16)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--routes", default="device,composed")
    ap.add_argument("--max-gib", type=float, default=32.0)
    a = ap.parse_args()
    if a.kind == "grow":
        return grow(a)
    be = mk.Backend(0)
    rng = np.random.default_rng(0)
    D = a.D
    if a.kind == "ham":
        H = mk.heisenberg_XXX(0.5, be=be)
        o1, o2, d, W = H[0], H[1], 2, 5
    else:
        O = rng.standard_normal((a.chi,) * 4)
        o1 = o2 = be.mposlice_dense(O)
        d = W = a.chi
    q, _ = np.linalg.qr(rng.standard_normal((D * d, D)))
    al = be.upload(q.reshape(D, d, D, order="F"))
    ar = be.upload(np.ascontiguousarray(q.T).reshape(D, d, D))
    ac = be.gemm(al.reshape(D * d, D), be.upload(np.diag(2.0 ** (-np.arange(D) / 8.0)))).reshape(D, d, D)
    GL = be.upload(rng.standard_normal(W * D * D)).reshape(W, D, D)
    GR = be.upload(rng.standard_normal(W * D * D)).reshape(W, D, D)
    Bm = _tail_matrix(be, ar)
    m = D * d

    def device():
        Y = be.dAC2_product(o1, o2, GL, GR, ac, ar)
        return _complement_directions(be, Y.reshape(m, m), al.reshape(m, D), Bm, a.k, rng, "device")

    def composed():
        from mpskit_jl_amd.algorithms import _two_site_tensor
        Y = be.dAC2(o1, o2, GL, GR, _two_site_tensor(be, ac, ar))
        return _complement_directions(be, Y.reshape(m, m), al.reshape(m, D), Bm, a.k, rng, "composed")

    out = {"kind": a.kind, "D": D, "d": d, "W": W, "k": a.k}
    for name in a.routes.split(","):
        fn = {"device": device, "composed": composed}[name]
        if name == "composed":
            gib = 2.0 * W * d * d * D * D * 8 / 2 ** 30
            out["composed_mix_workspace_gib"] = round(gib, 2)
            if gib > a.max_gib:
                out["composed"] = "skipped: workspace above --max-gib"
                continue
        fn()
        be.synchronize()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            be.synchronize()
            ts.append(time.perf_counter() - t0)
        out[name + "_ms"] = round(1e3 * statistics.median(ts), 3)
    out["complement_stats"] = be.complement_stats()
    print(json.dumps(out))
    be.close()


if __name__ == "__main__":
    main()
