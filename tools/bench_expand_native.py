"""Timings behind the bond-expansion paragraph of the README for interleaved complex states
(profiles/expand_native_timings.json): the expansion directions of ONE bond, d = 2, W = 3, on the device route
(mpsk_complement_tsvd under MPSK_C128) against the composed route (null-space bases from projected Gaussian blocks through
qrpos_c / lqpos_c, gemm_c, a full tsvd_c), at D = 256 and 1024 with k = 32 and 64.  Both routes read the same Y.  Two kinds of Y:
  graded      a planted complement spectrum s_j = 2^(-j / 4) plus Gaussian parts inside the ranges of AL and AR, which the
              projector removes: the spectrum of a state that lacks a few Schmidt values; the range finder is accepted;
  contracted  mpsk_dAC2_proj on Gaussian environments: a flat (Marchenko-Pastur) spectrum, the check of the range finder
              cannot pass, the entry answers with the full SVD and backs off -- the worst case of the device route.
A window is one whole call between two device events (both routes synchronise inside); the routes alternate window by
window; the figure is the median of 9 windows after 2 warm-up rounds.  mpsk_dAC2_proj itself is timed alone.
Usage: python tools/bench_expand_native.py [--D 256 1024] [--k 32 64] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpskit_jl_amd as mk  # noqa: E402
from mpskit_jl_amd import native_cplx as nc  # noqa: E402
from mpskit_jl_amd.changebonds import _tail_matrix  # noqa: E402
from bench_correlator import alternate_ms  # noqa: E402

Y_ = np.array([[0.0, -1.0j], [1.0j, 0.0]])
Z_ = np.diag([1.0, -1.0])


def gauss_c(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def one_size(be, D, ks):
    rng = np.random.default_rng(D)
    d, W = 2, 3
    m = D * d
    H = nc.ComplexMPOHamiltonian({(0, 0): 1, (0, 1): -Z_, (1, 2): Z_, (0, 2): -0.7 * Y_, (2, 2): 1}, be)
    q, _ = np.linalg.qr(gauss_c(rng, m, m))
    ql, nl = q[:, :D], q[:, D:]
    q2, _ = np.linalg.qr(gauss_c(rng, m, m))
    qr, nr = q2[:, :D].conj().T, q2[:, D:].conj().T                        # rows, (b, s) columns
    al = be.upload_c(ql.reshape(D, d, D, order="F"))
    ar = be.upload_c(np.transpose(qr.reshape(D, D, d, order="F"), (0, 2, 1)))
    ac = nc._mul_AC(be, al, be.upload_c(np.diag(2.0 ** (-np.arange(D) / 8.0)).astype(np.complex128)))
    GL = be.upload_env_c([gauss_c(rng, D, W, D)])
    GR = be.upload_env_c([gauss_c(rng, D, W, D)])
    QL, Bm = al.reshape(2 * m, D), _tail_matrix(be, ar)
    sig = 2.0 ** (-np.arange(D) / 4.0)
    Ys = {"graded": be.upload_c((nl * sig) @ nr + ql @ gauss_c(rng, D, m) + gauss_c(rng, m, D) @ qr),
          "contracted": be.dAC2_proj(H[0], H[0], GL, GR, ac, ar).reshape(2 * m, m)}
    out = {"D": D, "d": d, "W": W}
    out["dAC2_proj_ms"] = round(alternate_ms(be, [lambda: be.dAC2_proj(H[0], H[0], GL, GR, ac, ar)], 5)[0], 3)
    for kind, Y in Ys.items():
        for k in ks:
            before = be.complement_stats()
            dev, comp = alternate_ms(be, [lambda: nc._complement_directions_c(be, Y, QL, Bm, k, rng, True),
                                          lambda: nc._complement_directions_c(be, Y, QL, Bm, k, rng, False)], 1)
            after = be.complement_stats()
            Sd = nc._complement_directions_c(be, Y, QL, Bm, k, rng, True)[2]
            Sc = nc._complement_directions_c(be, Y, QL, Bm, k, rng, False)[2]
            out[f"{kind}_k{k}"] = {"device_ms": round(dev, 3), "composed_ms": round(comp, 3), "speedup": round(comp / dev, 2),
                                   "subspace_calls": after["subspace"] - before["subspace"],
                                   "full_calls": after["full"] - before["full"],
                                   "max_dS_over_S0": float(np.abs(Sd - Sc).max() / Sc[0])}
            print(json.dumps({"D": D, "kind": kind, "k": k, **out[f"{kind}_k{k}"]}), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--k", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "expand_native_timings.json"))
    a = ap.parse_args()
    res = {"protocol": "event-timed windows of one call, routes alternating, median of 9 after 2 warm-up rounds",
           "sizes": []}
    for D in a.D:                     # a context per size: one that backs off after the contracted kind would carry that over
        be = mk.Backend(0)
        res["sizes"].append(one_size(be, D, a.k))
        be.close()
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
