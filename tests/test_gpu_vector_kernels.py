"""Every Krylov vector kernel of mpsk_ops.hip against exact references (tests/exact_vector_inputs.py derives the inputs,
the guards and every bound used here; no tolerance in this file is a constant of its own).

Sizes come from the grid constants: 524 288 doubles per grid-stride trip of the d2 reductions, 262 144 of the long CGS2
kernels, 1 048 576 elements / 2 097 152 doubles of the capped elementwise kernels; one below, on and above a boundary,
odd tails included.  Which case reaches which kernel:

  test_dots[n]                 multidot_kernel<1..8> (k = 1..17: chunks 8 + 1..8 too), dot_final_kernel; two trips + odd
                               tail at 524 289 and 786 435
  test_gs_step_and_lincomb[n]  multidot_kernel, multiaxpy_kernel<1..8> (k = 1..17), through vgs_step / vlincomb /
                               vlincomb_dev; multiaxpy two trips at 2 097 155 (test_elementwise_two_trips, k = 11)
  test_orth_step[n]            k = 1..8: multiaxpy_dot_kernel<k, false> and <k, true>; k = 9..16 / 17..24 / 25..32:
                               multiaxpy_dot_long_kernel<16 | 24 | 32> + multiaxpy_norm_long_kernel; k = 33, 34: the
                               separate passes; scal_rsqrt_dev_kernel; host and device-slot entry points.  262 145 makes
                               two long trips, 786 435 three long trips / two d2 trips, both with an odd tail
  test_elementwise[n]          axpby_kernel (beta = 0 on NaN), scal_kernel, times_i_kernel, diff_nrm2_kernel (both ctx
                               dtypes), scal_rsqrt_dev(_oop)_kernel, zero vector
  test_elementwise_two_trips   the 4096-block cap: scal, scal_rsqrt*, multilincomb<8> at 1 048 833; axpby, multiaxpy<3, 8>,
                               times_i at 2 097 155 (2 097 156 for times_i)
  test_multilincomb[k]         multilincomb_kernel<8 | 16 | 24 | 32>
  test_complex_*               multidotc_kernel<1..8>, multiaxpy_c_kernel<1..8> (k = 1..32 through vorth_step_c, 1..17
                               through vlincomb_c), axpby_c_kernel; two trips at 262 145 (multidotc) and 1 048 577
                               complex (multiaxpy_c, axpby_c, k = 3)
  test_gaussian[...]           one Gaussian case per group inside the nested bound, each reducing call twice, same bits
  test_fused_sums_are_bit_identical_to_unfused   the claim in mpsk_ops.hip, k = 1..8 at 786 435
"""
import time

import numpy as np
import pytest

import exact_vector_inputs as ev

pytestmark = pytest.mark.gpu

BIG = 3 * ev.LONG_TRIP + 3
_dev = {}


def device(be, n, cplx=False, kmax=ev.KMAX):
    """the family's vectors on the GPU, uploaded once per n (the k sweeps use prefixes); one big family kept at a time"""
    key = (n, cplx, kmax)
    if key not in _dev:
        if n > 10 ** 5:
            for k_ in [k_ for k_ in _dev if k_[0] > 10 ** 5]:
                del _dev[k_]
        _dev[key] = ev.Device(be, ev.family(n, cplx, kmax))
    return _dev[key]


@pytest.mark.parametrize("n", ev.D2_SIZES)
def test_dots(be, n):
    out = ev.run_dots(device(be, n), range(1, 18))
    assert not out, out


@pytest.mark.parametrize("n", ev.D2_SIZES)
def test_gs_step_and_lincomb(be, n):
    out = ev.run_gs_lincomb(device(be, n), range(1, 18))
    assert not out, out


@pytest.mark.parametrize("n", sorted(set(ev.ORTH_SIZES + ev.LONG_SIZES)))
def test_orth_step(be, n):
    """mpsk_vorth_step and mpsk_vorth_step_dev (slot offset 3, h1 / h2 / n2 read back separately); every k = 1..34 at
    the sizes of the issue, one k per kernel variant at the other boundary sizes"""
    ks = range(1, ev.KMAX + 1) if n in ev.ORTH_SIZES else [1, 8, 9, 16, 17, 24, 25, 32, 33]
    out = ev.run_orth(device(be, n), ks)
    assert not out, out


@pytest.mark.parametrize("n", ev.D2_SIZES)
def test_elementwise(be, n):
    out = ev.run_elementwise(device(be, n))
    assert not out, out


def test_elementwise_two_trips(be):
    out = []
    dev = device(be, ev.EW_SIZE, kmax=3)
    ev.run_elementwise(dev, out)                                  # scal, scal_rsqrt*, ... past the 4096-block cap
    ev.run_multilincomb(dev, 3, 2, out)
    dev = device(be, ev.EW_D2_SIZE, kmax=11)
    ev.run_elementwise(dev, out)                                  # axpby
    ev.run_gs_lincomb(dev, [3, 11], out)                          # multiaxpy<3>, <8> + <3>
    dev = device(be, ev.EW_D2_SIZE + 1, kmax=1)
    p = dev.fam.y().reshape(-1, 2)
    ev.same(be.download(be.times_i(dev.y, out=dev.nan())), np.stack([-p[:, 1], p[:, 0]], axis=1).reshape(-1), "times_i", out)
    assert not out, out


@pytest.mark.parametrize("k,m", [(8, 5), (9, 32), (16, 3), (17, 2), (24, 7), (25, 1), (32, 32)])
def test_multilincomb(be, k, m):
    out = []
    for n in (3, 257, 4099):
        ev.run_multilincomb(device(be, n), k, m, out)
    assert not out, out


@pytest.mark.parametrize("n", ev.ORTH_C_SIZES)
def test_complex_orth_step(be, n):
    dev = device(be, n, cplx=True, kmax=32)
    out = ev.run_orth(dev, range(1, 33))
    ev.run_dots(dev, [1], out)
    ev.run_elementwise(dev, out)
    ev.run_gs_lincomb(dev, range(1, 18), out)
    assert not out, out


def test_complex_two_trips(be):
    dev = device(be, ev.EW_TRIP + 1, cplx=True, kmax=3)
    out = ev.run_orth(dev, [3])
    ev.run_gs_lincomb(dev, [3], out)
    ev.run_elementwise(dev, out)
    ev.run_dots(dev, [1], out)
    assert not out, out


@pytest.mark.parametrize("n,k,cplx", [(BIG, 8, False), (ev.LONG_TRIP + 1, 24, False), (4099, 34, False),
                                      (ev.D2_TRIP // 2 + 1, 5, True)])
def test_gaussian(be, n, k, cplx):
    out = ev.run_gauss(be, n, k, cplx)
    assert not out, out


def test_fused_sums_are_bit_identical_to_unfused(be):
    """mpsk_ops.hip: the fused CGS2 passes use the grid and per-thread element order of multidot_kernel, "so the sums are
    bit-identical to the unfused ones".  Gaussian data, k = 1..8, n = 786 435: the second-round dots mpsk_vorth_step_dev
    leaves in its slot against mpsk_vgs_step followed by mpsk_vmultidot of its result."""
    t = ev.gauss_case(BIG, 8)
    xs, y0 = [be.upload(x) for x in t["X"]], be.upload(t["y"])
    out = []
    for k in range(1, 9):
        y = be.copy(y0)
        h1 = be.gs_step(xs[:k], y)
        h2 = be.multidot(xs[:k], y)
        slot = be.upload(np.zeros(2 * k + 1))
        y = be.copy(y0)
        be.orth_step_dev(xs[:k], y, slot, 0)
        s = be.download(slot)
        ev.same(s[:k], h1, f"first-round dots k={k}", out)
        ev.same(s[k:2 * k], h2, f"second-round dots k={k}", out)
    assert not out, out
