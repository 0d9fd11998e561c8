"""Matvec timing of the prepared operator at the north-star site (Heisenberg S=1/2, D=1024, d=2, W=5): the Jordan form on
canonical environments (mode 3, 16 D^3) against the dense right-combined operator (mode 1, 40 D^3), HIP events over 50
applications after a 100-application warm-up.  Environments are uniform[0,1) with level 0 of GL and level W-1 of GR set
to the identity.  MPSK_HAC_LAUNCHES=2 / MPSK_SPLITK_F=f select the launch variants.

  python tools/bench_hac_jordan.py [D]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import mpskit_jl_amd as mk

D = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
d, W = 2, 5
be = mk.Backend(0)
H = mk.heisenberg_XXX(0.5, be=be)[1]
gl = torch.rand(W, D, D, dtype=torch.float64, device=be.device)
gr = torch.rand(W, D, D, dtype=torch.float64, device=be.device)
gl[0] = torch.eye(D, dtype=torch.float64, device=be.device)
gr[W - 1] = torch.eye(D, dtype=torch.float64, device=be.device)
GL = mk.DTensor(gl.flatten().contiguous(), (W, D, D))
GR = mk.DTensor(gr.flatten().contiguous(), (W, D, D))
x = mk.DTensor(torch.rand(D * d * D, dtype=torch.float64, device=be.device), (D, d, D))
y = be.empty(D, d, D)
for name, h, flops in [("mode 3", be.hac_create_ex(H, GL, GR, canonical=True), 16 * D ** 3),
                       ("mode 1", be.hac_create(H, GL, GR), 40 * D ** 3)]:
    for _ in range(100):
        h.apply(x, out=y)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 50
    e0.record()
    for _ in range(n):
        h.apply(x, out=y)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / n
    print(f"{name} (info {h.info()}): {ms:.4f} ms per matvec, {flops / ms * 1e-9:.1f} TFLOP/s at {flops // D ** 3} D^3",
          flush=True)
