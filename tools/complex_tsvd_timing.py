"""Timing of the native complex128 truncated SVD (mpsk_tsvd under MPSK_C128) against what a complex SVD cost before it: the
fp64 mpsk_tsvd of the real 2n x 2n embedding.  Also one DMRG2() sweep (reference default truncerr(1e-6)) of a complex
Heisenberg chain on interleaved storage (native_cplx).

Every step runs once, in a fresh process of its own, under a time limit; each prints one JSON line.
usage: python tools/complex_tsvd_timing.py [--step NAME]      (no argument: all steps, one child process each)"""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {"c128_1024": 240, "c128_2048": 420, "f64_embed_2048": 240, "f64_embed_4096": 420, "dmrg2_L32": 420}


def _matrix(n):
    import numpy as np
    rng = np.random.default_rng(n)

    def unitary(k):
        q, r = np.linalg.qr(rng.standard_normal((k, k)) + 1j * rng.standard_normal((k, k)))
        return q * (np.diag(r) / np.abs(np.diag(r)))
    return (unitary(n) * np.logspace(0, -12, n)) @ unitary(n).conj().T   # graded spectrum, as a DMRG bond


def run_step(name):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import mpskit_jl_amd as mk
    be = mk.Backend(0)
    out = {"step": name}
    if name.startswith("c128_") or name.startswith("f64_embed_"):
        n = int(name.split("_")[-1])
        if name.startswith("c128_"):
            a = _matrix(n)
            be.tsvd_c(be.upload_c(a[:64, :64]))                         # load the kernels
            th = be.upload_c(a)
            call = lambda: be.tsvd_c(th)
        else:
            a = _matrix(n // 2)
            e = np.zeros((n, n))
            e[0::2, 0::2], e[1::2, 0::2], e[0::2, 1::2], e[1::2, 1::2] = a.real, a.imag, -a.imag, a.real
            be.tsvd(be.upload(e[:64, :64]))
            th = be.upload(e)
            call = lambda: be.tsvd(th)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        U, S, Vh, k, _ = call()
        torch.cuda.synchronize()
        out.update(ms=1e3 * (time.perf_counter() - t0), sweeps=be.svd_sweeps(), n=n)
        s = be.download(S)
        nc_ = n if name.startswith("c128_") else n // 2
        s = s if name.startswith("c128_") else s[::2]                 # the embedding doubles every value
        out["s_err"] = float(np.abs(s[:nc_] - np.logspace(0, -12, nc_)).max())
    else:
        from mpskit_jl_amd import native_cplx as nc
        L, d, D0 = 32, 2, 128
        rng = np.random.default_rng(3)
        dims = [min(d ** (i + 1), d ** (L - 1 - i), D0) for i in range(L)]
        As = [rng.standard_normal((1 if i == 0 else dims[i - 1], d, dims[i])) +
              1j * rng.standard_normal((1 if i == 0 else dims[i - 1], d, dims[i])) for i in range(L)]
        H = mk.heisenberg_XXX(0.5, be=be)
        psi = nc.NativeFiniteMPS(As, be)
        eig = mk.Arnoldi(fixed_matvecs=8, krylovdim=8)
        alg = mk.DMRG2(maxiter=1, eigalg=eig)                          # trunc_err = 1e-6, no trunc_dim
        psi, envs, _ = nc.find_groundstate(psi, H, alg)                  # warm-up sweep
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        psi, envs, _ = nc.find_groundstate(psi, H, alg, envs)
        torch.cuda.synchronize()
        out.update(ms=1e3 * (time.perf_counter() - t0), L=L, max_bond=max(psi.dims(i)[2] for i in range(L)),
                   energy=float(nc.energy(psi, envs)))
    be.close()
    print(json.dumps(out), flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--step":
        run_step(sys.argv[2])
        return
    for name, limit in STEPS.items():
        r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name],
                           cwd=ROOT, stdout=subprocess.PIPE, text=True)
        line = r.stdout.strip().splitlines()[-1] if r.stdout.strip() else json.dumps({"step": name, "error": r.returncode})
        print(line, flush=True)
        if r.returncode != 0:                     # a failed or timed-out GPU step ends the run
            sys.exit(r.returncode)


if __name__ == "__main__":
    main()
