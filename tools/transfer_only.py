"""Environment transfers alone: the dense three-stage route against the canonical route (mpsk_transfer_left_ex /
mpsk_transfer_right_ex with MPSK_TRANSFER_CANONICAL; level by level and pair-Gram) of the same library in one process, on
canonical operands (identity level, isometric A).  Prints ms per call and TFLOP/s of the flops each route executes, and the largest difference.
usage: transfer_only.py [D ...] [--model heis|heis1] [--reps N]   (default: D = 256 512 1024, Heisenberg S=1/2)
Under rocprofv3 --kernel-trace --stats use --reps 5 --only dense|canonical."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import mpskit_jl_amd as mk

ap = argparse.ArgumentParser()
ap.add_argument("D", nargs="*", type=int, default=[256, 512, 1024])
ap.add_argument("--model", default="heis")
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--only", choices=["dense", "canonical", "pair"])
args = ap.parse_args()

be = mk.Backend(0)
H, d = {"heis": (lambda: mk.heisenberg_XXX(0.5, be=be), 2), "heis1": (lambda: mk.heisenberg_XXX(1.0, be=be), 3)}[args.model]
H = H()[0]
W = H.Wl


def dt(x, shape):
    return mk.DTensor(x.contiguous().flatten(), shape)


def timed(f, reps):
    for _ in range(5):
        f()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


for D in args.D:
    g = torch.Generator(device=be.device).manual_seed(D)
    rnd = lambda *s: torch.rand(*s, dtype=torch.float64, device=be.device, generator=g) - 0.5
    # Q: [D d, D] with orthonormal columns.  Left isometry A[(p,t), q] = Q: column-major flat index (p + D t) + D d q;
    # right isometry A[a, (t,b)] = Q^T: column-major flat index a + D (t + d b) = the row-major flattening of Q
    qr = lambda: torch.linalg.qr(rnd(D * d, D).cpu())[0].to(be.device)
    AL = dt(qr().t(), (D, d, D))
    AR = dt(qr(), (D, d, D))
    eye = torch.eye(D, dtype=torch.float64, device=be.device)
    GL = dt(torch.stack([eye] + [rnd(D, D) for _ in range(W - 1)]), (W, D, D))
    GR = dt(torch.stack([rnd(D, D) for _ in range(W - 1)] + [eye]), (W, D, D))
    outl, outr = be.empty(W, D, D), be.empty(W, D, D)
    dense_fl = 4.0 * d * W * D ** 3
    for side, f, G, A, out in (("left", be.transfer_left, GL, AL, outl), ("right", be.transfer_right, GR, AR, outr)):
        res = {}
        for route in ("dense", "canonical", "pair"):
            if args.only and route != args.only:
                continue
            # canonical: the level-by-level route (MPSK_TRANSFER_MODE=1); pair: the pair-Gram route forced (=2)
            os.environ["MPSK_TRANSFER_MODE"] = {"dense": "0", "canonical": "1", "pair": "2"}[route]
            ms = timed(lambda: f(H, G, A, A, out=out, canonical=(route != "dense")), args.reps)
            res[route] = (ms, out.buf[: out.size].clone())
        line = f"transfer_{side} {args.model} D={D} d={d} W={W}:"
        for route, (ms, _) in res.items():
            # canonical: fold application 2 d n D^3 (n = d slabs per t for these models) + stage 3 on W-1 levels
            fl = dense_fl if route == "dense" else 2.0 * d * d * D ** 3 + 2.0 * d * (W - 1) * D ** 3
            if route == "pair":         # fold application + finished level + the pair products at their nominal 2 D^3 each
                fl = 2.0 * d * d * D ** 3 + 2.0 * d * D ** 3 + 2.0 * (3 if d == 2 else 4) * D ** 3
            line += f"  {route} {ms:.4f} ms ({fl / ms / 1e9:.1f} TF/s of {fl / D ** 3:.0f} D^3)"
        if "dense" in res:
            for route in ("canonical", "pair"):
                if route in res:
                    a, b = res["dense"][1], res[route][1]
                    line += f"  {route}: {res['dense'][0] / res[route][0]:.3f}x of dense, max|diff|/max = {float((a - b).abs().max() / b.abs().max()):.2e}"
        print(line, flush=True)
be.close()
