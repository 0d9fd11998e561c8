"""A/B of the dense-MPO route (mpsk_mposlice_create_dense, stage 2 as an fp64 MFMA GEMM) against the slab-mix route of
the same O built through mpsk_mposlice_create: prepared matvec (mpsk_hac_apply) and the two transfers at (chi, d) in
{(2, 2), (2, 4), (4, 4), (9, 9), (16, 16)}, D in {128, 256, 512} (below the crossover also the forced GEMM route,
gemm_hac_ms); then one leading_boundary iteration of the 4 x 4-cluster Ising tensor (chi = d = 16) at D = 256.  TF/s are of the algorithmic flops 2 Dlo Dl d Dr Wl + 2 Dlo Dr (Wl d)(d Wr) + 2 Dlo d Dr^2 Wr.

    python tools/bench_dense_mpo.py             # full table + leading_boundary iteration
    python tools/bench_dense_mpo.py --trace     # dense route only, chi = d = 16, D = 256 (for a kernel trace)
"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import mpskit_jl_amd as mk  # noqa: E402


def flops(D, d, W):
    return 2 * D * D * d * D * W + 2 * D * D * (W * d) * (d * W) + 2 * D * d * D * D * W


def timeit(fn, n):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def rand(be, *shape):
    n = int(np.prod(shape))
    return mk.DTensor(torch.rand(n, dtype=torch.float64, device=be.device) - 0.5, shape)


def ab(be, chi, d, D, n):
    O = np.random.default_rng(chi).standard_normal((chi, d, d, chi))
    GL, GR, x, Ab = rand(be, chi, D, D), rand(be, chi, D, D), rand(be, D, d, D), rand(be, D, d, D)
    y = be.empty(D, d, D)
    row = {"chi": chi, "d": d, "D": D}
    res = {}
    for name, H in (("mix", be.mposlice(1, d, [chi], [chi], {(0, 0): O})), ("dense", be.mposlice_dense(O))):
        h = be.hac_create(H, GL, GR)
        res[name] = {
            "mode": h.info()["mode"],
            "hac_ms": timeit(lambda: h.apply(x, out=y), n),
            "tl_ms": timeit(lambda: be.transfer_left(H, GL, x, Ab), n),
            "tr_ms": timeit(lambda: be.transfer_right(H, GR, x, Ab), n),
        }
        res[name]["hac_tfs"] = flops(D, d, chi) / res[name]["hac_ms"] * 1e-9
        h.close()
        if name == "dense" and res[name]["mode"] != 4:      # below the crossover: what the GEMM route would cost
            os.environ["MPSK_DENSE_ROUTE"] = "1"
            h = be.hac_create(H, GL, GR)
            res["gemm"] = {"hac_ms": timeit(lambda: h.apply(x, out=y), n)}
            h.close()
            del os.environ["MPSK_DENSE_ROUTE"]
    row.update({f"{k}_{q}": v for k, r in res.items() for q, v in r.items()})
    row["speedup_hac"] = res["mix"]["hac_ms"] / res["dense"]["hac_ms"]
    return row


def lb_iteration(be, D):
    mpo = mk.classical_ising(0.3, cluster=4)
    psi = mk.InfiniteMPS.random(16, D, np.random.default_rng(1), be=be)
    torch.cuda.synchronize()
    t0 = time.time()
    envs = mk.statmech.environments(psi, mpo)
    torch.cuda.synchronize()
    t1 = time.time()
    psi, envs, eps = mk.leading_boundary(psi, mpo, mk.VUMPS(maxiter=1), envs=envs)
    torch.cuda.synchronize()
    t2 = time.time()
    return {"leading_boundary_D": D, "cluster": 4, "env_init_s": t1 - t0, "iteration_s": t2 - t1, "eps": eps,
            "hac_mode": envs.ddAC(0, psi)._prepare().info()["mode"]}


def main():
    be = mk.Backend(0)
    if "--trace" in sys.argv:
        O = np.random.default_rng(0).standard_normal((16, 16, 16, 16))
        H = be.mposlice_dense(O)
        D = 256
        GL, GR, x, Ab = rand(be, 16, D, D), rand(be, 16, D, D), rand(be, D, 16, D), rand(be, D, 16, D)
        h = be.hac_create(H, GL, GR)
        for _ in range(5):
            h.apply(x)
            be.transfer_left(H, GL, x, Ab)
            be.transfer_right(H, GR, x, Ab)
        torch.cuda.synchronize()
        print(json.dumps({"trace": "dense route chi = d = 16, D = 256", "mode": h.info()["mode"]}))
        return
    for chi, d in ((2, 2), (2, 4), (4, 4), (9, 9), (16, 16)):
        for D in (128, 256, 512):
            row = ab(be, chi, d, D, 10 if D < 512 else 5)
            print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items()}), flush=True)
    print(json.dumps(lb_iteration(be, 256)), flush=True)


if __name__ == "__main__":
    main()
