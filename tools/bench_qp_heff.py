"""Timings behind the Hamiltonian quasiparticle table of the README (profiles/qp_heff_timings.json): one site and one real
part of the effective excitation Hamiltonian by its two routes
  - fused:    mpsk_qp_heff_site (the half buffer of mpsk_qp_half made once, outside the windows);
  - composed: what _QPContext.heff runs without it -- one GEMM B = VL X, three mpsk_dAC (B in the centre, to the left, to
              the right), three axpby (-E B and the two sums), one projecting GEMM VL^T (.)
  - composed, B reused: the same without the GEMM B = VL X.  Inside one application of the operator the composed heff takes
              B from qp_envs, which forms it for the transfers on both routes, while mpsk_qp_heff_site forms it again: this
              is the ratio that decides the default.
on the sparse W = 5 Heisenberg slice, fp64, d = 2, at D = 256 and D = 1024 (VL [2 D, D], X [D, D]).  Windows of 20
asynchronous calls between two device events, the three variants alternating window by window, median of 9 windows after
warm-up (as tools/bench_qp_statmech.py).
Usage: python tools/bench_qp_heff.py [--sizes 256,1024] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpskit_jl_amd as mk  # noqa: E402
from bench_correlator import BATCH, WINDOWS, alternate_ms  # noqa: E402


def site_timing(be, name, H, D):
    rng = np.random.default_rng(D)
    d, Wl, Wr = H.d, H.Wl, H.Wr
    env = lambda W: be.upload(rng.standard_normal(W * D * D)).reshape(W, D, D)
    ten = lambda: be.upload(rng.standard_normal((D, d, D)))
    GL, GR, lB, rB, AR = env(Wl), env(Wr), env(Wl), env(Wr), ten()
    Q, _ = np.linalg.qr(rng.standard_normal((D * d, D * d)))
    AL, VL = be.upload(Q[:, :D].reshape(D, d, D, order="F")), be.upload(Q[:, D:])
    n = D * d - D
    X = be.upload(rng.standard_normal((n, D)))
    E = -0.4431
    half = be.qp_half(H, GL, AL)
    out_f, out_c = be.empty(n, D), be.empty(n, D)

    def fused():
        be.qp_heff_site(H, GL, GR, VL, X, E, lB, AR, half, rB, out=out_f)

    def composed():
        B = be.gemm(VL, X).reshape(D, d, D)
        Bn = be.dAC(H, GL, GR, B)
        be.axpby(-E, B, 1.0, Bn)
        be.axpby(1.0, be.dAC(H, lB, GR, AR), 1.0, Bn)
        be.axpby(1.0, be.dAC(H, GL, rB, AL), 1.0, Bn)
        be.gemm(VL, Bn.reshape(D * d, D), transA=True, out=out_c)

    B0 = be.gemm(VL, X).reshape(D, d, D)

    def composed_reusing_B():
        Bn = be.dAC(H, GL, GR, B0)
        be.axpby(-E, B0, 1.0, Bn)
        be.axpby(1.0, be.dAC(H, lB, GR, AR), 1.0, Bn)
        be.axpby(1.0, be.dAC(H, GL, rB, AL), 1.0, Bn)
        be.gemm(VL, Bn.reshape(D * d, D), transA=True, out=out_c)

    fused()
    composed()
    a, b = be.download(out_f), be.download(out_c)
    t = alternate_ms(be, [fused, composed, composed_reusing_B], BATCH)
    row = {"what": "qp_heff_site", "slice": name, "Wl": Wl, "d": d, "D": D, "complement": n, "calls_per_window": BATCH,
           "windows": WINDOWS, "fused_ms": t[0], "composed_ms": t[1], "composed_over_fused": t[1] / t[0],
           "composed_reusing_B_ms": t[2], "composed_reusing_B_over_fused": t[2] / t[0],
           "max_rel_difference": float(np.abs(a - b).max() / np.abs(b).max())}
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,1024")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    be = mk.Backend(0)
    rows = [site_timing(be, "sparse W=5 (Heisenberg)", mk.heisenberg_XXX(0.5, be=be)[0], int(D)) for D in a.sizes.split(",")]
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")
    be.close()


if __name__ == "__main__":
    main()
