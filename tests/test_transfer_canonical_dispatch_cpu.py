"""Host dispatch of the canonical transfers (FinEnv -> Backend.transfer_left/right(canonical=True)) on stand-in backends:
a backend without the `_ex` entries keeps working, a backend with them is asked for the canonical route exactly where ddAC
asks for mode 3 (plain FinEnv, real state), and ShardedFinEnv / the terms of a sum never ask for it."""
import numpy as np

import mpskit_oracle as mo
import mpskit_jl_amd as mk
from mpskit_jl_amd import algorithms as alg, krylov
from mpskit_jl_amd import dist as mdist
from cpu_backend import CpuBackend


class ExBackend(CpuBackend):
    """CpuBackend with the entries of the product Backend: records every `canonical` it is given, computes densely"""

    def __init__(self):
        super().__init__()
        self.asked = []

    def transfer_left(self, H, GLin, A, Ab, out=None, canonical=False):
        self.asked.append(("l", bool(canonical), A is Ab))
        return super().transfer_left(H, GLin, A, Ab, out=out)

    def transfer_right(self, H, GRin, A, Ab, out=None, canonical=False):
        self.asked.append(("r", bool(canonical), A is Ab))
        return super().transfer_right(H, GRin, A, Ab, out=out)

    def transfer_left_ex(self, H, GLin, A, Ab, canonical=False, out=None):
        return self.transfer_left(H, GLin, A, Ab, out=out, canonical=canonical)

    def transfer_right_ex(self, H, GRin, A, Ab, canonical=False, out=None):
        return self.transfer_right(H, GRin, A, Ab, out=out, canonical=canonical)


def _state(be, L=8, d=2, D=8, seed=3):
    rng = np.random.default_rng(seed)
    dims = mo.FiniteMPS.random(L, d, D, np.random.default_rng(0)).bond_dims()
    As = [rng.random((1 if i == 0 else dims[i - 1], d, dims[i])) for i in range(L)]
    return mk.FiniteMPS(As, normalize=True, be=be)


def _sweeps(be, envs_of, n=2):
    psi = _state(be)
    H = mk.heisenberg_XXX(0.5, be=be)
    envs = envs_of(psi, H)
    eig = mk.Arnoldi(fixed_matvecs=4, krylovdim=4)
    for _ in range(n):
        alg.dmrg_sweep(psi, H, envs, eig, krylov.KrylovWorkspace(be))
    return float(np.sum(mk.expectation_value(psi, H, envs))), envs


def test_backend_without_ex_entries_keeps_working():
    cb = CpuBackend()
    assert not hasattr(cb, "transfer_left_ex")
    E, envs = _sweeps(cb, mk.FinEnv)          # CpuBackend.transfer_left takes no `canonical`: a TypeError if it were passed
    assert np.isfinite(E) and envs.n_transfers > 0
    assert cb.calls["transfer_left"] + cb.calls["transfer_right"] == envs.n_transfers


def test_finenv_asks_for_the_canonical_route_and_sharded_never_does():
    xb = ExBackend()
    E1, envs = _sweeps(xb, mk.FinEnv)
    assert len(xb.asked) == envs.n_transfers > 0
    assert all(c and same for _, c, same in xb.asked), xb.asked
    assert {side for side, _, _ in xb.asked} == {"l", "r"}
    # same sweeps through a backend without the entries: same energy (the stand-in computes densely either way)
    E0, _ = _sweeps(CpuBackend(), mk.FinEnv)
    assert abs(E1 - E0) <= 1e-12 * abs(E0)
    # ShardedFinEnv (world 1, forced sharding of the bulk bonds) keeps the dense route on every update
    sb = ExBackend()
    _, senvs = _sweeps(sb, lambda p, H: mdist.ShardedFinEnv(p, H, mdist.Comm(1, 0), min_block=2, force=True))
    assert senvs.n_transfers > 0 and len(sb.asked) > 0
    assert not any(c for _, c, _ in sb.asked), sb.asked


def test_terms_of_a_sum_and_complex_states_keep_the_dense_route():
    xb = ExBackend()
    psi = _state(xb)
    H = mk.heisenberg_XXX(0.5, be=xb)
    e = mk.FinEnv(psi, H)
    from mpskit_jl_amd.environments import MultipleEnvironments
    MultipleEnvironments(None, [e])            # what environments(psi, LazySum) wraps its terms in
    e.leftenv(len(psi) - 1, psi)
    e.rightenv(0, psi)
    assert xb.asked and not any(c for _, c, _ in xb.asked)
    # a state flagged complex: dense
    xb2 = ExBackend()
    psi2 = _state(xb2)
    e2 = mk.FinEnv(psi2, mk.heisenberg_XXX(0.5, be=xb2))
    assert e2._canonical(psi2)
    psi2.cplx = True
    assert not e2._canonical(psi2)
