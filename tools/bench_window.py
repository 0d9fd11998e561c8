"""Timings behind the window table of the README (profiles/window_timings.json): one site of window.transition at
D = 256 and D = 1024, d = 2, fp64 and complex128, by its two routes
  - fused:    mpsk_transfer_left_gram_env (stage 1, the closing product with its Gram epilogue, stage 2 of the transfer);
  - composed: the same three products from mpsk_gemm with X = T1 R written to memory, then mpsk_site_gram(X, Ab).
Both produce the site matrix M_j and the next left matrix L_{j+1}.  Windows of 20 asynchronous calls between two device
events, the two routes alternating window by window, median of 9 windows after warm-up (as tools/bench_correlator.py).
Usage: python tools/bench_window.py [--D 256 1024] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpskit_jl_amd as mk  # noqa: E402
from bench_correlator import BATCH, alternate_ms  # noqa: E402


def site_timing(be, D, cplx, d=2):
    rng = np.random.default_rng(D + cplx)
    c = 2 if cplx else 1
    gen = (lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)) if cplx else (lambda *s: rng.standard_normal(s))
    up = be.upload_c if cplx else be.upload
    mm = be.gemm_c if cplx else be.gemm
    kw = {"cplx": True} if cplx else {}
    Lin, A, Ab, R = up(gen(D, D)), up(gen(D, d, D)), up(gen(D, d, D)), up(gen(D, D))
    g1, g2 = be.empty(c * d, d), be.empty(1, c * d, d)
    lout = be.empty(1, c * D, D)
    t1, x, l2 = be.empty(c * D, d * D), be.empty(c * D * d, D), be.empty(c * D, D)

    def fused():
        be.transfer_left_gram_env(Lin, A, Ab, R, g1, out=lout, **kw)

    def composed():
        mm(Lin, A.reshape(c * D, d * D), out=t1)
        mm(t1.reshape(c * D * d, D), R, out=x)
        be.site_gram(x.reshape(c * D, d, D), Ab, out=g2, **kw)
        mm(Ab.reshape(c * D * d, D), t1.reshape(c * D * d, D), transA=True, out=l2)

    fused()
    composed()
    be.synchronize()
    a, b = be.download(g1).reshape(-1), be.download(g2).reshape(-1)
    t = alternate_ms(be, [fused, composed], BATCH)
    return {"what": "transition_site", "D": D, "d": d, "dtype": "c128" if cplx else "f64", "fused_ms": t[0],
            "composed_ms": t[1], "composed_over_fused": t[1] / t[0],
            "max_rel_difference": float(np.abs(a - b).max() / np.abs(b).max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    be = mk.Backend(0)
    rows = [site_timing(be, D, cplx) for D in a.D for cplx in (False, True)]
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")
    be.close()


if __name__ == "__main__":
    main()
