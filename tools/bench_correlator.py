"""Timings behind the measurement paragraph of the README (profiles/correlator_timings.json):
  - correlator(psi, Sz, Sz, 0, range(1, L)) over a whole chain of L = 100 sites at D = 256 and D = 1024, fused device route
    (one mpsk_transfer_left_gram per site, one download) against the composed route (two mpsk_transfer_left, a dot and a host
    round trip per site).  The state is a random FiniteMPS with those bond dimensions (the timings do not depend on the
    entries).  A window is one whole call between two device events; the routes alternate window by window and the figure
    is the median after warm-up.
  - mpsk_site_gram alone at D = 1024, d = 2, W = 1 and W = 3 (windows of BATCH asynchronous calls), with achieved GB/s over
    the (W + 1) D d D doubles it reads, next to mpsk_vdot on two vectors of the same total bytes in the same run.  mpsk_vdot
    returns a host scalar, so each of its calls ends in a stream synchronisation that the Gram calls do not have.
Usage: python tools/bench_correlator.py [--D 256 1024] [--L 100] [--gram-D 1024] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mpskit_jl_amd as mk  # noqa: E402

BATCH, WINDOWS, WARMUP = 20, 9, 2
SZ = np.diag([0.5, -0.5])


def alternate_ms(be, fns, batch):
    """per-call milliseconds of each fn: median over WINDOWS event-timed windows of `batch` calls, variants interleaved"""
    for _ in range(WARMUP):
        for fn in fns:
            fn()
    be.synchronize()
    ts = [[] for _ in fns]
    for _ in range(WINDOWS):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(be.torch_stream)
            for _ in range(batch):
                fn()
            e1.record(be.torch_stream)
            e1.synchronize()
            ts[i].append(e0.elapsed_time(e1) / batch)
    return [statistics.median(t) for t in ts]


def correlator_timing(be, L, D):
    psi = mk.FiniteMPS.random(L, 2, D, np.random.default_rng(D), be=be)
    psi.AC(0)
    for j in range(1, L):                                   # the gauge sweep happens once, outside the windows
        psi.AR(j)
    js = range(1, L)
    dev = mk.correlator(psi, SZ, SZ, 0, js, device=True)
    comp = mk.correlator(psi, SZ, SZ, 0, js, device=False)
    t = alternate_ms(be, [lambda: mk.correlator(psi, SZ, SZ, 0, js, device=True),
                          lambda: mk.correlator(psi, SZ, SZ, 0, js, device=False)], 1)
    return {"what": "correlator_full_chain", "L": L, "D": max(psi.bond_dims()), "device_ms": t[0], "composed_ms": t[1],
            "composed_over_device": t[1] / t[0], "max_abs_difference": float(np.abs(dev - comp).max())}


def gram_timing(be, D, W, d=2):
    rng = np.random.default_rng(W)
    ab = be.upload(rng.standard_normal((D, d, D)))
    x = be._upload_slabs([rng.standard_normal((D, d, D)) for _ in range(W)])
    out = be.empty(W, d, d)
    nbytes = 8 * (W + 1) * D * d * D
    n = nbytes // 16
    u, v = be.upload(rng.standard_normal(n)), be.upload(rng.standard_normal(n))
    t = alternate_ms(be, [lambda: be.site_gram(x, ab, out=out), lambda: be.dot(u, v)], BATCH)
    return {"what": "site_gram", "D": D, "d": d, "W": W, "bytes": nbytes, "site_gram_ms": t[0],
            "site_gram_GBps": nbytes / t[0] * 1e-6, "vdot_ms": t[1], "vdot_GBps": nbytes / t[1] * 1e-6,
            "vdot_synchronises": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--L", type=int, default=100)
    ap.add_argument("--gram-D", type=int, default=1024)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    be = mk.Backend(0)
    rows = [gram_timing(be, a.gram_D, W) for W in (1, 3)]
    rows += [correlator_timing(be, a.L, D) for D in a.D]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")
    be.close()


if __name__ == "__main__":
    main()
