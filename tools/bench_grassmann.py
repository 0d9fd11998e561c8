"""Timings behind the GradientGrassmann paragraph of the README (profiles/grassmann_timings.json):
  - one line-search trial step of one site (Dl = Dr = D, d = 2) with the direction's SVD cached: coefficients, the two
    outputs W' and Z', and the complement projection of Z', three ways on the same inputs:
      device            mpsk_grassmann_coef + one mpsk_gemm_pair
      composed          what grassmann.py's composed route does: singular values read back, four diagonal matrices built
                        on the host and uploaded, plain mpsk_gemm calls
      composed_resident the same plain GEMMs with the four diagonal matrices already on the device (one fixed alpha): the
                        kernel-against-GEMM figure, without the copies
    The QRpos of W' is common to all and left out.  A window is BATCH back-to-back steps between two device events; the
    variants alternate window by window; the figure is the median over WINDOWS windows after warm-up, per step.
  - the split of one full evaluation of f and its gradient at a new point of an iTFI state (g = 2, one-site cell), the
    stages called one by one from here: SVD of the direction (+ P = W Vt^T), trial step (coefficients, gemm_pair, QRpos,
    projection), uniform gauge fix of the new AL (InfiniteMPS.from_AL), environments, the point (H_AC and projection, SVDs
    of the bond matrices, energy; the last two timed by wrappers installed here), preconditioned gradient.  Host clock
    around work that ends in a device synchronise; median over --evals evaluations after one warm-up.
Usage: python tools/bench_grassmann.py [--D 256 1024] [--evals 5] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mpskit_jl_amd as mk  # noqa: E402
from mpskit_jl_amd import algorithms, grassmann as gm  # noqa: E402

BATCH, WINDOWS = 10, 20


def alternate_ms(be, fns):
    for fn in fns:
        for _ in range(BATCH):
            fn()
    be.synchronize()
    ts = [[] for _ in fns]
    for _ in range(WINDOWS):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(be.torch_stream)
            for _ in range(BATCH):
                fn()
            e1.record(be.torch_stream)
            e1.synchronize()
            ts[i].append(e0.elapsed_time(e1) / BATCH)
    return [statistics.median(t) for t in ts]


def trial_step(be, D, d=2):
    rng = np.random.default_rng(D)
    m = D * d
    W, _ = np.linalg.qr(rng.standard_normal((m, D)))
    Z = rng.standard_normal((m, D))
    Z -= W @ (W.T @ Z)
    Z /= np.linalg.norm(Z)
    Wd, t = be.upload(W), gm.PrecGrad(be.upload(Z))
    U, S, Vt, P = gm._direction_svd(be, Wd, t)
    coef, Wn, Zn = be.empty(D, 4), be.empty(m, D), be.empty(m, D)
    alphas = iter(np.linspace(0.1, 0.9, 4 * BATCH * (WINDOWS + 1)))
    dg = [gm._diag(be, c) for c in gm._coef_host(np.asarray(be.download(S)).reshape(-1), 0.5, "retract")]

    def device():
        be.grassmann_coef(S, next(alphas), "retract", out=coef)
        be.gemm_pair(P, U, Vt, coef, out1=Wn, out2=Zn)
        gm._project_out(be, Wn, Zn)

    def composed():
        a1, b1, a2, b2 = gm._coef_host(np.asarray(be.download(S)).reshape(-1), next(alphas), "retract")
        be.gemm(P, be.gemm(gm._diag(be, a1), Vt), out=Wn)
        be.gemm(U, be.gemm(gm._diag(be, b1), Vt), beta=1.0, out=Wn)
        be.gemm(P, be.gemm(gm._diag(be, a2), Vt), out=Zn)
        be.gemm(U, be.gemm(gm._diag(be, b2), Vt), beta=1.0, out=Zn)
        gm._project_out(be, Wn, Zn)

    def composed_resident():
        be.gemm(P, be.gemm(dg[0], Vt), out=Wn)
        be.gemm(U, be.gemm(dg[1], Vt), beta=1.0, out=Wn)
        be.gemm(P, be.gemm(dg[2], Vt), out=Zn)
        be.gemm(U, be.gemm(dg[3], Vt), beta=1.0, out=Zn)
        gm._project_out(be, Wn, Zn)

    dev_ms, comp_ms, res_ms = alternate_ms(be, [device, composed, composed_resident])
    return {"what": "trial_step_one_site", "D": D, "d": d, "device_ms": dev_ms, "composed_ms": comp_ms,
            "composed_resident_ms": res_ms, "composed_over_device": comp_ms / dev_ms,
            "composed_resident_over_device": res_ms / dev_ms}


class Stopwatch:
    """seconds per bucket; `with sw("name")` synchronises the device on both sides"""

    def __init__(self, be):
        self.be, self.t = be, {}

    def __call__(self, name):
        self.name = name
        return self

    def __enter__(self):
        self.be.synchronize()
        self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        self.be.synchronize()
        self.t[self.name] = self.t.get(self.name, 0.0) + time.perf_counter() - self.t0

    def wrap(self, fn, name):
        """fn timed into its own bucket and taken OUT of the bucket that is open around it"""
        def timed(*a, **k):
            self.be.synchronize()
            t0 = time.perf_counter()
            r = fn(*a, **k)
            self.be.synchronize()
            dt = time.perf_counter() - t0
            self.t[name] = self.t.get(name, 0.0) + dt
            self.t[self.name] = self.t.get(self.name, 0.0) - dt
            return r
        return timed


def fg_split(be, D, evals, d=2):
    H = mk.transverse_field_ising(g=2.0, be=be)
    psi = mk.InfiniteMPS.random(d, D, np.random.default_rng(D + 1), be=be)
    envs = mk.environments(psi, H)
    x = gm.ManifoldPoint(psi, envs)
    _, g = gm.fg(x)
    eta = gm.scale(be, g, -1.0)
    W = gm._mat(psi.AL[0])
    runs = []
    rho_cls, expval = gm.Rhoreg, algorithms.expectation_value
    for k in range(evals + 1):
        sw = Stopwatch(be)
        eta[0]._svd = None                     # a new direction every time: its SVD belongs to the evaluation
        with sw("direction_svd"):
            gm._direction_svd(be, W, eta[0])
        with sw("trial_step"):
            Wn, _ = gm.retract_site(be, W, eta[0], 1e-3 * (k + 1), "device")
        with sw("gauge_fix"):
            nstate = mk.InfiniteMPS.from_AL([Wn.reshape(*psi.AL[0].shape)], psi.CR[0], be=be)
        with sw("environments"):
            envs.recalculate(nstate)
        gm.Rhoreg, algorithms.expectation_value = sw.wrap(rho_cls, "bond_svds"), sw.wrap(expval, "energy")
        try:
            with sw("H_AC_and_projection"):
                xp = gm.ManifoldPoint(nstate, envs, "device")
        finally:
            gm.Rhoreg, algorithms.expectation_value = rho_cls, expval
        with sw("preconditioned_gradient"):
            gm.fg(xp)
        runs.append(sw.t)
    runs = runs[1:]
    med = {k: statistics.median(r[k] for r in runs) for k in runs[0]}
    total = sum(med.values())
    return {"what": "fg_split_iTFI", "D": D, "d": d, "evals": evals, "seconds": med,
            "share": {k: v / total for k, v in med.items()}, "total_seconds": total}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--evals", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    be = mk.Backend(0)
    rows = []

    def record(row):
        rows.append(row)
        print(json.dumps(row), flush=True)
        if a.out:                                  # rewritten after every row: a long evaluation never costs the earlier ones
            with open(a.out, "w") as f:
                json.dump(rows, f, indent=1)
                f.write("\n")

    for D in a.D:
        record(trial_step(be, D))
    for D in a.D:
        record(fg_split(be, D, a.evals))
    be.close()


if __name__ == "__main__":
    main()
