"""The level solver of the infinite Hamiltonian environments and the uniform drivers make the backend calls recorded in
tests/golden/ham_inf_env_calls.json, in that order (tests/golden/make_ham_inf_env_calls.py records them: method name and
the shapes of the tensor arguments, with krylov.gmres / krylov.linsolve replaced by two applications of the operator).
environments.MPOHamInfEnv owns the control flow and native_cplx.NativeMPOHamInfEnv overrides its leaves; algorithms._vumps
and algorithms._timestep_inf are the loops of both state types.  A change to the shared flow shows here for both."""
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
import make_ham_inf_env_calls as gen  # noqa: E402
from cpu_backend_ham_inf import CpuHamInfBackend  # noqa: E402
from mpskit_jl_amd import krylov  # noqa: E402

SECTIONS = ["real_construct", "real_recalculate_changed_bonds", "native_composed_construct",
            "native_composed_recalculate_changed_bonds", "real_vumps_iteration", "native_vumps_iteration", "real_timestep",
            "native_timestep"]
NAMES = [f"{case}_n{n}/{sec}" for case in ("tfi", "diag") for n in gen.CELLS for sec in SECTIONS]


@pytest.fixture(scope="module")
def golden():
    return gen.load()


@pytest.fixture(scope="module")
def recorded():
    solvers = krylov.gmres, krylov.linsolve
    out = gen.record_host(CpuHamInfBackend())
    assert (krylov.gmres, krylov.linsolve) == solvers          # the stand-ins are gone again
    return out


def test_every_section_is_recorded(golden, recorded):
    assert set(recorded) == set(NAMES)
    assert set(golden) == set(NAMES) | {gen.DEVICE_SECTION}


@pytest.mark.parametrize("name", NAMES)
def test_same_calls_in_the_same_order(golden, recorded, name):
    diff = gen.first_difference(recorded[name], golden[name])
    assert diff is None, f"{name}: {diff}"


def test_the_plain_branch_and_the_regulariser_both_run(golden):
    """the cases reach what they are there for: the diagonal levels of `diag` solve through scaled and MPO-block transfers,
    identity levels regularise"""
    real, nat = golden["diag_n2/real_construct"], golden["diag_n2/native_composed_construct"]
    assert any(c.startswith("regularize(") for c in real) and any(c.startswith("scal(") for c in real)
    assert any(c.startswith("mposlice(") for c in real) and any(c.startswith("mposlice(") for c in nat)
    assert not any(c.startswith("scal(") for c in golden["tfi_n2/real_construct"])
