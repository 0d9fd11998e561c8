"""CPU self-check of tests/exact_vector_inputs.py: the references of the GPU vector-kernel tests must pass their own
criteria.

Every exact case stays below the 2^50 guard and numpy's fp64 arithmetic reproduces the integer reference bit for bit;
numpy fp64 stays inside the derived bounds on every Gaussian case; numpy's eigh stays inside the measured constant the
Ritz tests multiply by 8; and the case runner itself is run on the host stand-in backend (tests/cpu_backend.py) for the
methods that backend has."""
import numpy as np
import pytest

import exact_vector_inputs as ev
from cpu_backend import CpuBackend

TABLE = [(3 * ev.LONG_TRIP + 3, 32), (4099, 32), (5, 3)]


def test_longdouble_is_wider_than_fp64():
    assert np.finfo(np.longdouble).nmant >= 63


def test_sizes_follow_the_grid_constants():
    assert ev.D2_TRIP == 524288 and ev.LONG_TRIP == 262144 and ev.EW_TRIP == 1048576 and ev.EW_D2_TRIP == 2097152
    assert 3 * ev.LONG_TRIP + 3 == 786435 and [ev.exponent(n) for n, _ in TABLE] == [9, 6, 1]
    # two trips of two elements + the odd tail, 9 levels, 4 partials per thread, 9 levels / three trips + one
    assert ev.depth(786435) == 2 * 2 + 1 + 9 + 4 + 9 and ev.depth(786435, long=True) == 4 + 9 + 4 + 9
    assert ev.depth(5) == 2 + 1 + 9 + 1 + 9


@pytest.mark.parametrize("n,k", TABLE)
@pytest.mark.parametrize("cplx", [False, True])
def test_numpy_fp64_reproduces_the_exact_reference(n, k, cplx):
    if cplx:
        n = (n + 1) // 2 if n > 5 else n
    fam = ev.family(n, cplx, k)
    X = np.stack([fam.x(j) for j in range(k)])
    (rec,) = ev.cgs2_sweep(fam, [k])
    assert rec["guard"] < ev.LIMIT, np.log2(rec["guard"])
    got = ev.numpy_cgs2(X, fam.y())
    for q in ("h1", "y1", "h2", "y2", "h"):
        assert np.array_equal(got[q], rec[q]), q
    dots, guard = ev.exact_dots(fam, k)
    assert guard < ev.LIMIT and np.array_equal(X.conj() @ fam.y(), dots)
    cf = ev.lincomb_coefs(k, cplx)
    ref, guard = ev.exact_lincomb(fam, cf)
    assert guard < ev.LIMIT and np.array_equal(cf @ X, ref)
    out = []
    nd = 2 * n if cplx else n
    ev.close_exact(got["n2"], ev.n2_fraction(rec), ev.n2_factor(nd), "n2", out)
    ev.within(got["beta"], ev.beta_ld(rec), ev.beta_factor(nd) * ev.beta_ld(rec), "beta", out)
    assert not out, out


@pytest.mark.parametrize("n", [5, 4099])
def test_every_prefix_of_a_sweep_is_guarded_and_matches_a_fresh_computation(n):
    fam = ev.family(n)
    for rec in ev.cgs2_sweep(fam, range(1, ev.KMAX + 1)):
        assert rec["guard"] < ev.LIMIT
        got = ev.numpy_cgs2(np.stack([fam.x(j) for j in range(rec["k"])]), fam.y())
        assert all(np.array_equal(got[q], rec[q]) for q in ("h1", "y1", "h2", "y2", "h")), rec["k"]


@pytest.mark.parametrize("n,k,cplx", [(4099, 34, False), (ev.LONG_TRIP + 1, 8, False), (4097, 5, True)])
def test_numpy_fp64_is_inside_the_gaussian_bounds(n, k, cplx):
    t = ev.gauss_case(n, k, cplx)
    got = ev.numpy_cgs2(t["X"], t["y"])
    out = []
    for q in ("h1", "h2", "h", "y1", "y2", "n2", "beta", "yn"):
        ev.within(got[q], t[q], t["E_" + q], q, out)
    assert not out, out


def test_case_runner_on_the_host_backend():
    be = CpuBackend()
    out = []
    for n in (3, 258, 4099):
        dev = ev.Device(be, ev.family(n))
        ev.run_dots(dev, range(1, 18), out)
        ev.run_gs_lincomb(dev, range(1, 18), out)
        ev.run_orth(dev, range(1, ev.KMAX + 1), out=out)
        ev.run_elementwise(dev, out)
    ev.run_gauss(be, 4099, 12, out=out)
    assert not out, out


def test_case_runner_reports_a_wrong_backend():
    class Wrong(CpuBackend):
        def multidot(self, xs, y):
            h = super().multidot(xs, y)
            h[-1] += 2.0 ** -20
            return h
    out = []
    dev = ev.Device(Wrong(), ev.family(258))
    ev.run_dots(dev, [3], out)
    ev.run_orth(dev, [3], out=out)
    assert any("multidot" in r for r in out) and any("orth_step h" in r for r in out), out


RITZ_CPU = ["m1", "m2", "m7", "m20", "m32-stride70", "cut0-zero", "cut1-tiny", "cut6-zero", "cut7-tiny", "degenerate", "sign",
            "zero", "scale+150", "scale-150", "overflow"]


@pytest.mark.parametrize("name", RITZ_CPU)
def test_numpy_eigh_is_inside_its_measured_constant_and_the_runner_works(name):
    """NUMPY_WORST is what the Ritz tests multiply by 8 (profiles/vector_kernel_bounds.log lists every case)"""
    ref = ev.ritz_ref(name)
    coef, info = ev.numpy_ritz(ref)
    r = ev.ritz_ratios(coef, info, ref, vector=ev.ritz_cases()[name]["kind"] == "plain")
    assert max(r.values()) <= ev.NUMPY_WORST, r
    got = ev.run_ritz(CpuBackend(), name)
    rec, _ = ev.check_ritz(name, *got, ev.RITZ_BOUND)
    assert not rec, rec
