"""mpsk_dC_proj against numpy.einsum, its square case against mpsk_dC, its argument checks and host routes, and the uniform
approximate / leading_boundary (VOMPS) end to end on the device: the case bodies of tests/test_vomps_cpu.py."""
import numpy as np
import pytest
import torch

import mpskit_jl_amd as mk
from mpskit_jl_amd.statmech import dC_proj_composed

import exact_inputs as ei
import test_vomps_cpu as vc               # the shared NumPy restatements and case bodies (module attributes: not collected twice)

pytestmark = pytest.mark.gpu

RTOL = 2e-13                              # the bound and input convention of mpsk_dAC_proj (tests/test_gpu_approximate.py)
SEED = 20240213
PROJ_SHAPES = [(3, 5, 7, 2), (24, 40, 56, 20), (48, 20, 24, 40), (130, 200, 136, 72)]


def _slabs(be, arr):
    """host [D1, D2, W] (slab w = arr[:, :, w]) -> device environment (W, D1, D2)."""
    return be.upload(arr).reshape(arr.shape[2], arr.shape[0], arr.shape[1])


# ---- mpsk_dC_proj ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("W", [1, 3, 5])
def test_dc_proj_parity(be, W):
    rng = np.random.default_rng(SEED)
    for Dlo, Dl, Dr, Dro in PROJ_SHAPES:
        G, R, c = rng.random((Dlo, Dl, W)), rng.random((Dr, Dro, W)), rng.random((Dl, Dr))
        y = be.download(be.dC_proj(_slabs(be, G), _slabs(be, R), be.upload(c)))
        assert y.shape == (Dlo, Dro)
        ref = np.einsum("paw,ab,bqw->pq", G, c, R, optimize=True)
        e = np.abs(y - ref).max() / np.abs(ref).max()
        print("dC_proj", W, (Dlo, Dl, Dr, Dro), e)
        assert e < RTOL * max(Dlo, Dl, Dr, Dro), (W, Dlo, Dl, Dr, Dro, e)


@pytest.mark.parametrize("tile", [(0, 0)] + ei.TILES, ids=lambda t: f"{t[0]}x{t[1]}")
def test_dc_proj_square_is_dc_bitwise(be, tile):
    rng = np.random.default_rng(SEED)
    be.lib.mpsk_ctx_force_tile(be.ctx, *tile)
    try:
        for W, Dlo, Dl, Dr in ((3, 24, 40, 56), (5, 130, 72, 136)):
            G, R, c = (_slabs(be, rng.random((Dlo, Dl, W))), _slabs(be, rng.random((Dr, Dr, W))), be.upload(rng.random((Dl, Dr))))
            a, b = be.dC(G, R, c), be.dC_proj(G, R, c)
            assert a.shape == b.shape == (Dlo, Dr)
            assert torch.equal(a.buf[:a.size], b.buf[:b.size]), (tile, W, Dlo, Dl, Dr)
    finally:
        be.lib.mpsk_ctx_force_tile(be.ctx, 0, 0)            # process-wide knob: never leave a tile forced


def test_dc_proj_argument_checks(be):
    lib, ctx = be.lib, be.ctx
    p = be.zeros(4096).ptr

    def returns(code, rc):
        assert rc == code and len(lib.mpsk_last_error()) > 0, (rc, lib.mpsk_last_error())
    returns(1, lib.mpsk_dC_proj(ctx, 2, 2, 2, 2, 2, None, p, p, p))
    returns(1, lib.mpsk_dC_proj(ctx, 2, 2, 2, 2, 2, p, None, p, p))
    returns(1, lib.mpsk_dC_proj(ctx, 2, 2, 2, 2, 2, p, p, None, p))
    returns(1, lib.mpsk_dC_proj(ctx, 2, 2, 2, 2, 2, p, p, p, None))
    returns(1, lib.mpsk_dC_proj(None, 2, 2, 2, 2, 2, p, p, p, p))
    for dims in ((0, 2, 2, 2, 2), (2, 0, 2, 2, 2), (2, 2, 0, 2, 2), (2, 2, 2, 0, 2), (2, 2, 2, 2, 0), (2, 2, 2, 2, -3)):
        returns(1, lib.mpsk_dC_proj(ctx, *dims, p, p, p, p))
    be._set_dtype(True)
    try:
        returns(3, lib.mpsk_dC_proj(ctx, 2, 2, 2, 2, 2, p, p, p, p))          # MPSK_ERR_UNSUPPORTED under MPSK_C128
    finally:
        be._set_dtype(False)
    assert lib.mpsk_dC_proj(ctx, 2, 2, 2, 2, 2, p, p, p, p) == 0
    be.synchronize()


def test_dc_proj_host_routes(be):
    """Backend.dC_proj against the composed route (gemm products per slab + axpby) on the device, and c_proj reaching each
    through hasattr"""
    rng = np.random.default_rng(SEED)
    W, Dlo, Dl, Dr, Dro = 3, 24, 40, 56, 20
    G, R, c = _slabs(be, rng.random((Dlo, Dl, W))), _slabs(be, rng.random((Dr, Dro, W))), be.upload(rng.random((Dl, Dr)))
    a, b = be.download(be.dC_proj(G, R, c)), be.download(dC_proj_composed(be, G, R, c))
    assert a.shape == b.shape == (Dlo, Dro)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()
    out = be.empty(Dlo, Dro)
    assert be.dC_proj(G, R, c, out=out) is out and np.array_equal(be.download(out), a)
    above = mk.InfiniteMPS.random(2, 6, np.random.default_rng(1), be=be)
    below = mk.InfiniteMPS.random(2, 4, np.random.default_rng(2), be=be)
    O = mk.classical_ising()
    envs = mk.environments(below, (O, above))
    dev = be.download(mk.c_proj(0, below, envs))
    envs.be = Composed(be)
    comp = be.download(mk.c_proj(0, below, envs))
    assert dev.shape == (4, 4) and np.abs(dev - comp).max() <= 1e-12 * np.abs(dev).max()


# ---- the uniform algorithms on the device ----------------------------------------------------------------------------

class Composed:
    """The backend with the projection entry points hidden, so that c_proj takes its composed route."""

    def __init__(self, be):
        self._be = be

    def __getattr__(self, name):
        if name in ("dC_proj", "dAC_proj"):
            raise AttributeError(name)
        return getattr(self._be, name)


def test_mixed_environments(be):
    vc.case_mixed_environments(be)


def test_mixed_equals_plain(be):
    vc.case_mixed_equals_plain(be)


def test_exact_target(be):
    assert vc.case_exact_target(be) <= 200


def test_time_step_against_tdvp(be):
    vc.case_time_step(be)


def test_leading_boundary_vomps(be):
    vc.case_leading_boundary(be)


def test_compression(be):
    vc.case_compression(be)


def test_error_paths(be):
    vc.case_error_paths(be)


def test_vumps_is_converted(be):
    vc.case_vumps_is_converted(be)
