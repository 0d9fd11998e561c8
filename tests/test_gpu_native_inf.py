"""mpsk_dC_proj_c, mpsk_vsplit_c / mpsk_vjoin_c and the uniform states on interleaved complex storage, on the device.  The
operands and case bodies are those of tests/native_inf_cases.py (checked without a GPU in test_native_inf_cases_cpu.py);
the mpsk_dC_proj_c results must be bit-equal to the exact reference."""
import ctypes as C
import types

import numpy as np
import pytest

import native_inf_cases as cs
from mpskit_jl_amd import native_cplx as nc
from mpskit_jl_amd.backend import DTensor

pytestmark = pytest.mark.gpu
GUARD = 32            # doubles before and after the output (256 bytes: the output keeps its alignment)
GUARD_WORD = -4242.0


def _log(text):
    print("NATIVE-INF device " + text)


def _guarded(be, n):
    import torch
    buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float64, device=be.device)
    buf[:GUARD] = GUARD_WORD
    buf[GUARD + n:] = GUARD_WORD
    return buf


@pytest.mark.parametrize("shape", cs.DC_SHAPES, ids=str)
def test_dC_proj_c_is_exact_behind_guard_words(be, shape):
    W, Dlo, Dl, Dr, Dro = shape
    GL, GR, c = cs.dc_operands(shape)
    buf = _guarded(be, 2 * Dlo * Dro)
    y = DTensor(buf[GUARD:GUARD + 2 * Dlo * Dro], (2 * Dlo, Dro))
    be.dC_proj_c(cs.slabs_c(be, GL), cs.slabs_c(be, GR), be.upload_c(c), out=y)
    be.synchronize()
    assert np.array_equal(be.download_c(y), cs.dc_ref(GL, GR, c))
    host = buf.cpu().numpy()
    assert np.all(host[:GUARD] == GUARD_WORD) and np.all(host[-GUARD:] == GUARD_WORD)


@pytest.mark.parametrize("shape", [(3, 5, 3, 7, 7), (2, 4, 4, 4, 4), (3, 65, 17, 70, 70)], ids=str)
def test_square_right_environment_is_dC(be, shape):
    GL, GR, c = cs.dc_operands(shape, seed=7)
    gl, gr, cm = cs.slabs_c(be, GL), cs.slabs_c(be, GR), be.upload_c(c)
    a, b = be.dC_proj_c(gl, gr, cm), be.dC(gl, gr, cm, cplx=True)
    be.synchronize()
    assert np.array_equal(be.download_c(a), be.download_c(b))
    assert np.array_equal(be.download_c(a), cs.dc_ref(GL, GR, c))


def test_argument_checks(be):
    GL, GR, c = cs.dc_operands((2, 4, 4, 4, 4))
    gl, gr, cm, y = cs.slabs_c(be, GL), cs.slabs_c(be, GR), be.upload_c(c), be.empty(8, 4)
    call = lambda *a: be.lib.mpsk_dC_proj_c(be.ctx, *a)
    assert call(2, 4, 4, 4, 4, gl.ptr, gr.ptr, cm.ptr, y.ptr) == 3          # MPSK_F64 ctx: MPSK_ERR_UNSUPPORTED
    be._set_dtype(True)
    try:
        ptrs = [gl.ptr, gr.ptr, cm.ptr, y.ptr]
        for k in range(4):
            assert call(2, 4, 4, 4, 4, *[None if j == k else p for j, p in enumerate(ptrs)]) == 1
        assert be.lib.mpsk_dC_proj_c(None, 2, 4, 4, 4, 4, *ptrs) == 1
        for k in range(5):
            for bad in (0, -1):
                dims = [2, 4, 4, 4, 4]
                dims[k] = bad
                assert call(*dims, *ptrs) == 1
        assert call(2, 4, 4, 4, 4, *ptrs) == 0
        # mpsk_dC_proj itself stays real-only
        assert be.lib.mpsk_dC_proj(be.ctx, 2, 4, 4, 4, 4, *ptrs) == 3
    finally:
        be._set_dtype(False)
    be.synchronize()


def test_fused_against_composed_c_proj(be):
    W, Dlo, Dl, Dr, Dro = 3, 65, 17, 33, 70
    rng = np.random.default_rng(9)
    z = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    GL, GR, c = z(W, Dlo, Dl), z(W, Dr, Dro), z(Dl, Dr)
    gl, gr, cm = cs.slabs_c(be, GL), cs.slabs_c(be, GR), be.upload_c(c)
    fused, comp = be.download_c(be.dC_proj_c(gl, gr, cm)), be.download_c(nc.dC_proj_c_composed(be, gl, gr, cm))
    rel = np.linalg.norm(fused - comp) / np.linalg.norm(comp)
    ref = np.linalg.norm(fused - cs.dc_ref(GL, GR, c)) / np.linalg.norm(comp)
    _log(f"fused vs composed c_proj at (3; 65, 17, 33, 70): {rel:.3e}; fused vs NumPy: {ref:.3e}")
    assert rel <= 1e-13


@pytest.mark.parametrize("n", [1, 5, 1000, 70001])
def test_split_join_round_trip_is_exact(be, n):
    rng = np.random.default_rng(n)
    z = rng.standard_normal(n) + 1j * rng.standard_normal(n)
    zt = be.upload_c(z.reshape(n, 1))
    p = be.split_c(zt)
    back = be.join_c(p, zt.shape)
    be.synchronize()
    assert np.array_equal(be.download(p), np.concatenate([z.real, z.imag]))
    assert np.array_equal(be.download_c(back).ravel(), z)


@pytest.mark.parametrize("n", [1, 2])
def test_imaginary_time_parity_and_real_time(be, n):
    r = cs.case_imag_parity(be, n, log=_log)
    cs.case_real_time(be, n, r["b_dot"], log=_log)


def test_composed_route_on_the_device(be):
    r = cs.case_imag_parity(be, 1, device=False)
    cs.case_real_time(be, 1, r["b_dot"], device=False)


def test_gauge_contract_D16(be):
    _, worst = cs.case_gauge(be, 2, 16, seed=51)
    _log(f"gauge contract n = 2, D = 16: |AL CR - CR AR| / |AC| = {worst:.3e} at gauge tolerance 1e-12")
    cs.case_dot_self(be, 1, 16, seed=52)


def test_dC_proj_c_is_ordered_on_a_user_stream(be):
    """the delayed producer of tests/stream_order.py: mpsk_dC_proj_c on a non-blocking user stream must return while the
    producer of its operands is pending and still give the exact result"""
    import torch
    import mpskit_jl_amd as mk
    import stream_order as so
    shape = (3, 65, 17, 33, 70)
    W, Dlo, Dl, Dr, Dro = shape
    true, decoy = cs.dc_operands(shape, seed=1), cs.dc_operands(shape, seed=2)
    flat = lambda G: np.concatenate([np.ravel(g, order="F") for g in G]).view(np.float64)      # interleaved slabs
    fc = lambda m: np.ravel(m, order="F").view(np.float64)
    be2 = mk.Backend(0, stream=torch.cuda.Stream(0))
    try:
        def run(b, dev, _):
            view = lambda name, *s: DTensor(dev[name].buf, s)
            b.dC_proj_c(view("GL", W, 2 * Dlo, Dl), view("GR", W, 2 * Dr, Dro), view("c", 2 * Dl, Dr),
                        out=view("y", 2 * Dlo, Dro))
        case = types.SimpleNamespace(
            name="dC_proj_c", family="contraction", setup=None, run=run, sync=False,
            operands={"GL": (flat(true[0]), flat(decoy[0])), "GR": (flat(true[1]), flat(decoy[1])),
                      "c": (fc(true[2]), fc(decoy[2]))},
            outputs={"y": 2 * Dlo * Dro})
        got, info = so.Staged(be2, case).delayed(be2, so.Delay(be2.torch_stream))
        assert info["returned_before_produced"]
        y = got["y"].view(np.complex128).reshape((Dlo, Dro), order="F")
        assert np.array_equal(y, cs.dc_ref(*true))
        assert not np.array_equal(y, cs.dc_ref(*decoy))
    finally:
        be2.synchronize()
        be2.close()
