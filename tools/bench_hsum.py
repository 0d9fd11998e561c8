#!/usr/bin/env python
"""Timing of the summed prepared operator (mpsk_hsum) against the composed sum, n = 3 Heisenberg (W = 5, d = 2) terms:
  folded       mpsk_hsum_apply on route 1 (canonical environments: identity corners)
  accumulated  mpsk_hsum_apply on route 2 (the same terms on generic environments)
  composed     n mpsk_hac_apply + n - 1 mpsk_vaxpby on the same terms (the operators mpsk_hac_create prepares)
and mpsk_hsum_set_coefs alone (bytes read and written / time).  Method of tools/bench_propagator.py: every variant is
timed in windows of REPS back-to-back calls between two events, the variants alternate window by window, the first
windows are warm-up and the figure is the median of the rest.

  python tools/bench_hsum.py [--out profiles/hsum_timings.json] [--D 256 1024] [--windows 12]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPS, WARM = 20, 3


def _window(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / REPS            # ms per call


def _case(be, mk, D, cplx, rng):
    n, d, W = 3, 2, 5
    Hs = [mk.heisenberg_XXX(0.5, J=J, be=be) for J in (1.0, 0.5, -0.25)]
    slices = [be.mposlice(H.odim, d, H[0].chil, H[0].chir, dict(H[0].blocks), cplx=True) if cplx else H[0] for H in Hs]

    def envs(canonical):
        out = []
        for _ in range(n):
            mkb = lambda: rng.standard_normal((D, 1, D)) + (1j * rng.standard_normal((D, 1, D)) if cplx else 0)
            gl, gr = [mkb() for _ in range(W)], [mkb() for _ in range(W)]
            if canonical:
                gl[0] = np.eye(D)[:, None, :] + (0j if cplx else 0)
                gr[-1] = np.eye(D)[:, None, :] + (0j if cplx else 0)
            up = be.upload_env_c if cplx else be.upload_env
            out.append((up(gl), up(gr)))
        return [e[0] for e in out], [e[1] for e in out]

    flag = {"canonical_c128": True} if cplx else {"canonical": True}
    GLc, GRc = envs(True)
    GLg, GRg = envs(False)
    x = rng.standard_normal((D, d, D)) + (1j * rng.standard_normal((D, d, D)) if cplx else 0)
    xd = (be.upload_c if cplx else be.upload)(x)
    m = 2 if cplx else 1
    y, tmp = be.empty(m * D, d, D), be.empty(m * D, d, D)
    coefs = [1.0, 0.7, -0.3]
    folded = be.hsum_create(slices, GLc, GRc, **flag).set_coefs(coefs)
    accum = be.hsum_create(slices, GLg, GRg).set_coefs(coefs)
    assert folded.info()["route"] == 1 and accum.info()["route"] == 2
    singles = [be.hac_create(s, gl, gr) for s, gl, gr in zip(slices, GLg, GRg)]

    def composed():
        singles[0].apply(xd, out=y)
        be.scal(coefs[0], y)
        for c, h in zip(coefs[1:], singles[1:]):
            h.apply(xd, out=tmp)
            be.axpby(c, tmp, 1.0, y)

    variants = {"folded": lambda: folded.apply(xd, out=y), "accumulated": lambda: accum.apply(xd, out=y),
                "composed": composed, "set_coefs": lambda: folded.set_coefs(coefs)}
    # bytes of one set_coefs: n source pairs read, one pair written; a fold pair is 2 d^2 D^2 elements
    pair = 2 * d * d * D * D * (16 if cplx else 8)
    return variants, (n + 1) * pair, {"folded": folded.info(), "accumulated": accum.info()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "hsum_timings.json"))
    ap.add_argument("--D", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--windows", type=int, default=12)
    args = ap.parse_args()
    import torch
    import mpskit_jl_amd as mk
    be = mk.Backend(0)
    rng = np.random.default_rng(0)
    rows = []
    for cplx in (False, True):
        for D in args.D:
            variants, nbytes, info = _case(be, mk, D, cplx, rng)
            times = {k: [] for k in variants}
            for w in range(WARM + args.windows):
                for k, fn in variants.items():                   # alternate the variants window by window
                    t = _window(torch, fn)
                    if w >= WARM:
                        times[k].append(t)
            med = {k: float(np.median(v)) for k, v in times.items()}
            row = {"dtype": "c128" if cplx else "f64", "D": D, "n": 3, "W": 5, "d": 2, "ms": med, "info": info,
                   "composed_over_folded": med["composed"] / med["folded"],
                   "composed_over_accumulated": med["composed"] / med["accumulated"],
                   "set_coefs_GBps": nbytes / (med["set_coefs"] * 1e-3) / 1e9,
                   "reps_per_window": REPS, "windows": args.windows, "warmup_windows": WARM}
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"tool": "tools/bench_hsum.py", "device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
    be.close()


if __name__ == "__main__":
    main()
