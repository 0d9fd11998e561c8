"""Timings behind the propagator paragraph of the README (profiles/propagator_timings.json):
  - mpsk_hac_apply against mpsk_hac_apply_axpby for the real Heisenberg S = 1/2 operator (modes 1 and 3) and for its complex
    twin without and with MPSK_HAC_CANONICAL_C128 (modes 2 and 3), at D = 256 and D = 1024.  A window is BATCH back-to-back
    calls between two device events; the variants alternate window by window, so drift hits them alike; the figure is the
    median over 20 windows after warm-up, per call.
  - one NaiveInvert site solve (the centre site of a random complex chain, z = E + 0.5 + 0.1i), flag off and on, each run
    once to warm up and then timed.  The GMRES is capped at --gmres-restarts cycles of 30, so on this (unconverged, random)
    state the number of applications is the cap's, not that of a converged solve; `converged` says which.
Usage: python tools/bench_propagator.py [--D 256 1024] [--solve-D 1024] [--solve-L 22] [--out FILE]"""
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
from mpskit_jl_amd import krylov  # noqa: E402
from mpskit_jl_amd.native_cplx import NativeFinEnv, NativeFiniteMPS  # noqa: E402

BATCH, WINDOWS = 20, 20


def alternate_ms(be, fns):
    """per-call milliseconds of each fn: median over WINDOWS event-timed windows of BATCH calls, variants interleaved"""
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


def apply_timings(be, D, d=2):
    rng = np.random.default_rng(D)
    H = mk.heisenberg_XXX(0.5, be=be)[0]
    W = H.Wl
    eye = np.eye(D)
    gl = [eye[:, None, :]] + [rng.standard_normal((D, 1, D)) for _ in range(W - 1)]
    gr = [rng.standard_normal((D, 1, D)) for _ in range(W - 1)] + [eye[:, None, :]]
    GL, GR = be.upload_env(gl), be.upload_env(gr)
    x, y = be.upload(rng.standard_normal((D, d, D))), be.empty(D, d, D)
    h1, h3 = be.hac_create(H, GL, GR), be.hac_create_ex(H, GL, GR, canonical=True)
    assert (h1.info()["mode"], h3.info()["mode"]) == (1, 3)
    t = alternate_ms(be, [lambda: h1.apply(x, out=y), lambda: h1.apply_axpby(-0.6, x, 1.7, out=y),
                          lambda: h3.apply(x, out=y), lambda: h3.apply_axpby(-0.6, x, 1.7, out=y)])
    out = [{"what": "apply", "dtype": "f64", "mode": m, "D": D, "d": d, "W": W, "apply_ms": a, "apply_axpby_ms": b,
            "overhead": b / a - 1.0} for m, a, b in ((1, t[0], t[1]), (3, t[2], t[3]))]
    h1.close(); h3.close()
    Hc = mk.cplx.HalfEmbeddedOp._cslice(be, H)
    GLc = be.upload_env_c([g.astype(complex) for g in gl])
    GRc = be.upload_env_c([g.astype(complex) for g in gr])
    xc = be.upload_c(rng.standard_normal((D, d, D)) + 1j * rng.standard_normal((D, d, D)))
    yc = be.empty(2 * D, d, D)
    c2, c3 = be.hac_create(Hc, GLc, GRc), be.hac_create_ex(Hc, GLc, GRc, canonical_c128=True)
    assert (c2.info()["mode"], c3.info()["mode"]) == (2, 3)
    z = -(0.5 + 0.1j)
    t = alternate_ms(be, [lambda: c2.apply(xc, out=yc), lambda: c2.apply_axpby(1.0, xc, z, out=yc),
                          lambda: c3.apply(xc, out=yc), lambda: c3.apply_axpby(1.0, xc, z, out=yc)])
    out += [{"what": "apply", "dtype": "c128", "flag": f, "mode": m, "D": D, "d": d, "W": W, "apply_ms": a, "apply_axpby_ms": b,
             "overhead": b / a - 1.0} for f, m, a, b in (("off", 2, t[0], t[1]), ("on", 3, t[2], t[3]))]
    out.append({"what": "flag_on_over_flag_off", "D": D, "apply_ratio": t[2] / t[0]})
    c2.close(); c3.close()
    return out


def solve_timing(be, L, D, restarts):
    from mpskit_jl_amd.propagator import _OverlapEnv, _ShiftedHAC
    rng = np.random.default_rng(5)
    dims = [min(2 ** i, 2 ** (L - i), D) for i in range(L + 1)]
    psi0 = NativeFiniteMPS([rng.standard_normal((dims[i], 2, dims[i + 1])) + 1j * rng.standard_normal((dims[i], 2, dims[i + 1]))
                            for i in range(L)], be)
    H = mk.heisenberg_XXX(0.5, be=be)
    init = psi0.copy()
    pos = L // 2
    init.move_center(pos)
    envs, mixed = NativeFinEnv(init, H), _OverlapEnv(init, psi0)
    vs, ws = krylov.ComplexVec(be), krylov.KrylovWorkspace(be)
    ac = init.A[pos]
    E = (vs.dot(ac, _ShiftedHAC(be, envs, pos, False)(ac)) / vs.dot(ac, ac)).real
    rhs = vs.axpby(-1.0, mixed.ac_proj(pos), 0.0, be.empty(*ac.shape))
    rows = []
    for flag in (False, True):
        for rep in range(2):                                  # the first run warms up (operator buffers, workspace, code objects)
            op = _ShiftedHAC(be, envs, pos, flag)
            be.synchronize()
            t0 = time.perf_counter()
            _, info = krylov.linsolve(be, op, rhs, ac, a0=-(E + 0.5 + 0.1j), a1=1.0, tol=1e-12, krylovdim=30, maxiter=restarts,
                                      ws=ws, cplx=True)
            be.synchronize()
            dt = time.perf_counter() - t0
        rows.append({"what": "naive_invert_site_solve", "flag": "on" if flag else "off", "mode": op.h.info()["mode"], "L": L,
                     "D": [ac.shape[0] // 2, ac.shape[2]], "seconds": dt, "applications": info.numops,
                     "gmres_restart_cap": restarts, "converged": info.converged, "normres": info.normres})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--D", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--solve-D", type=int, default=1024)
    ap.add_argument("--solve-L", type=int, default=22)
    ap.add_argument("--gmres-restarts", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    be = mk.Backend(0)
    rows = []
    for D in a.D:
        rows += apply_timings(be, D)
    rows += solve_timing(be, a.solve_L, a.solve_D, a.gmres_restarts)
    for r in rows:
        print(json.dumps(r), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")
    be.close()


if __name__ == "__main__":
    main()
