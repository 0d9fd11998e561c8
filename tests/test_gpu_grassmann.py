"""GradientGrassmann on the device (mpskit.jl_amd/grassmann.py over mpsk_gemm_pair / mpsk_grassmann_coef): the geometry on
the forced device route, device route against composed route, the tie to calc_galerkin, and the ground-state runs of the
reference's default composite.  Shared checks: tests/grassmann_cases.py."""
import numpy as np
import pytest

import mpskit_jl_amd as mk
from mpskit_jl_amd import grassmann as gm
import grassmann_cases as gc

pytestmark = pytest.mark.gpu

SITES = [(65, 2, 65), (16, 3, 16)]


@pytest.mark.parametrize("dims", SITES, ids=str)
def test_geometry_device_route(be, dims):
    gc.check_geometry(be, *dims, route="device")


@pytest.mark.parametrize("route", ["device", "composed"])
def test_geometry_rank_deficient_direction_wide_bond(be, route):
    """a 100 x 80 site: every direction has rank <= 20 < 80, so the SVD of the direction has 60 zero singular values and
    80 > 64 columns take the wide Jacobi route; retract(alpha = 0) = W holds only with an orthogonal Vt behind them"""
    gc.check_geometry(be, 50, 2, 80, route=route)


def test_lazy_sum_gradient_is_the_galerkin_error(be):
    H = mk.LazySum([mk.transverse_field_ising(g=2.0, be=be), mk.transverse_field_ising(J=0.5, g=0.3, be=be)], [1.0, 0.7])
    gc.check_galerkin_tie(mk.InfiniteMPS.random(2, 12, np.random.default_rng(5), n=2, be=be), H)
    gc.check_galerkin_tie(mk.FiniteMPS.random(6, 2, 8, np.random.default_rng(6), be=be), H)


def _relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


@pytest.mark.parametrize("dims", SITES, ids=str)
def test_device_route_equals_composed_route(be, dims):
    """the two routes differ in summation order only: 1e-13 relative in max-norm"""
    Dl, d, Dr = dims
    Wd, Td, _, _ = gc.random_site(be, Dl, d, Dr, seed=7)
    z = gm.PrecGrad(Td[2])
    out = {}
    for route in ("device", "composed"):
        Wn, Zn = gm.retract_site(be, Wd, z, 0.3, route)
        Tn = gm.transport_site(be, Td[0], Wd, z, 0.3, Wn, route)
        out[route] = [be.download(t) for t in (Wn, Zn, Tn)]
    rng = np.random.default_rng(8)
    C = be.upload(rng.standard_normal((Dr, Dr)) / np.sqrt(Dr))
    rho = gm.Rhoreg(be, C, 0.05, True)
    pg_dev = be.download(rho.apply_inverse(Td[1]))
    rho.device = False
    out["device"].append(pg_dev)
    out["composed"].append(be.download(rho.apply_inverse(Td[1])))
    for name, a, b in zip(("W'", "Z'", "Theta'", "Pg"), out["device"], out["composed"]):
        assert _relmax(a, b) <= 1e-13, (name, _relmax(a, b))


def test_gradient_norm_is_the_galerkin_error(be):
    H = mk.transverse_field_ising(be=be)
    gc.check_galerkin_tie(mk.InfiniteMPS.random(2, 12, np.random.default_rng(5), n=2, be=be), H)
    gc.check_galerkin_tie(mk.FiniteMPS.random(6, 2, 8, np.random.default_rng(6), be=be), H)


@pytest.mark.parametrize("cell", [(1, 8), (2, 6)], ids=lambda c: f"n{c[0]}_D{c[1]}")
def test_default_uniform_groundstate(be, cell):
    """find_groundstate(psi, H, tol=1e-8): composite route, |g| <= 1e-8, energy within 1e-10 of VUMPS(tol=1e-10), and a
    non-increasing energy over the accepted steps (allowance 1e-13 |E|)"""
    gc.check_uniform_default(be, *cell)


def test_finite_chain(be):
    gc.check_finite_chain(be)


def test_finite_chain_forced_device_route(be):
    gc.check_finite_chain(be, route="device", L=6, D=4)
