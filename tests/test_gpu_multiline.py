"""The multi-row leading_boundary / approximate and their environments end to end on the device: the case bodies of
tests/test_multiline_cpu.py.  Every column operator is a loop over mpsk_dAC_proj / mpsk_dC_proj; the stacked operator is
compared with per-row calls here."""
import numpy as np
import pytest

import mpskit_jl_amd as mk

import test_multiline_cpu as mc           # the shared NumPy restatements and case bodies (module attributes: not collected twice)

pytestmark = pytest.mark.gpu


def test_structure(be):
    mc.case_structure(be)


@pytest.mark.parametrize("above_too", [False, True])
def test_environments(be, above_too):
    mc.case_environments(be, above_too)


def test_stacked_operator_is_the_per_row_projection(be):
    """out[(r + shift) % R] of the stacked column operator is dAC_proj / dC_proj of row r, bit for bit (the same call, copied)"""
    mpo = mk.MPOMultiline([mk.classical_ising(0.3), mk.classical_ising(0.4)])
    for D in (8, [4, 6]):
        psi = mc.random_rows(be, D, 2)
        envs = mk.environments(psi, mpo)
        for shift in (0, 1):
            op = envs.ddAC(0, psi, shift=shift)
            out = op.split_out(op(op.stack_in([psi.AC[r, 0] for r in range(2)])))
            for r in range(2):
                one = be.dAC_proj(envs.O(r, 0), envs.leftenv(r, 0, psi), envs.rightenv(r, 0, psi), psi.AC[r, 0])
                assert np.array_equal(be.download(out[(r + shift) % 2]), be.download(one)), (D, shift, r)
            op = envs.ddC(0, psi, shift=shift)
            out = op.split_out(op(op.stack_in([psi.CR[r, 0] for r in range(2)])))
            for r in range(2):
                one = be.dC_proj(envs.leftenv(r, 1, psi), envs.rightenv(r, 0, psi), psi.CR[r, 0])
                assert np.array_equal(be.download(out[(r + shift) % 2]), be.download(one)), (D, shift, r)
    mc.case_mixed_D(be)


def test_identical_rows(be):
    mc.case_identical_rows(be, D=8)


def test_different_rows(be):
    mc.case_different_rows(be, D=8)


def test_vomps_same_eigenvalue(be):
    mc.case_vomps_same_eigenvalue(be)


def test_approximate(be):
    mc.case_approximate_identity(be)
    mc.case_approximate_ising(be)
