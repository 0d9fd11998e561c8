"""Gauge-invariant A/B of the site operator: the bench workload (Heisenberg S=1/2, L, D, fixed budget of 8 matvecs per site,
seeded random start) swept N times with the dense prepared operator (MPSK_HAC_MODE=1) and with the default choice (mode 3,
Jordan form on canonical environments), in one process.  Prints one JSON line: the energy after every sweep of both runs,
their max relative difference, and the fidelity |<a|b>|^2 / (<a|a> <b|b>) of the two final states.

  python tools/hac_mode_ab.py [L] [D] [sweeps]"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import mpskit_jl_amd as mk
from mpskit_jl_amd import algorithms as alg, krylov
from mpskit_jl_amd import derivatives

L = int(sys.argv[1]) if len(sys.argv) > 1 else 100
D = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
N = int(sys.argv[3]) if len(sys.argv) > 3 else 25
be = mk.Backend(0)
H = mk.heisenberg_XXX(0.5, be=be)


def run(hac_mode):
    if hac_mode is None:
        os.environ.pop("MPSK_HAC_MODE", None)
    else:
        os.environ["MPSK_HAC_MODE"] = hac_mode
    modes = set()
    orig = derivatives.MPO_ddAC._prepare

    def spy(self):
        h = orig(self)
        modes.add(h.info()["mode"])
        return h
    derivatives.MPO_ddAC._prepare = spy
    try:
        psi = mk.FiniteMPS.random(L, 2, D, np.random.default_rng(20240213), normalize=True, be=be)
        envs = mk.FinEnv(psi, H)
        eig = mk.Arnoldi(fixed_matvecs=8, krylovdim=8)
        ws = krylov.KrylovWorkspace(be)
        energies = []
        for _ in range(N):
            alg.dmrg_sweep(psi, H, envs, eig, ws)
            energies.append(float(np.sum(alg.expectation_value(psi, H, envs))))
    finally:
        derivatives.MPO_ddAC._prepare = orig
        os.environ.pop("MPSK_HAC_MODE", None)
    # one consistent representation per state: AL on sites 0..L-2, AC on the last site
    tens = [psi.AL(i) for i in range(L - 1)] + [psi.AC(L - 1)]
    return energies, [t.buf[: t.size].view(t.shape[2], t.shape[1], t.shape[0]).permute(2, 1, 0) for t in tens], sorted(modes)


def overlap(a, b):
    E = torch.ones(1, 1, dtype=torch.float64, device=a[0].device)
    for A, B in zip(a, b):
        E = torch.einsum("ab,asr,bsq->rq", E, A, B)
    return float(E.reshape(-1)[0])


e1, s1, m1 = run("1")
e3, s3, m3 = run(None)
fid = overlap(s1, s3) ** 2 / (overlap(s1, s1) * overlap(s3, s3))
print(json.dumps({"L": L, "D": D, "sweeps": N, "modes_dense": m1, "modes_default": m3,
                  "energies_dense": e1, "energies_default": e3,
                  "max_rel_energy_diff": max(abs(x - y) / abs(x) for x, y in zip(e1, e3)),
                  "fidelity": fid, "one_minus_fidelity": 1.0 - fid}))
