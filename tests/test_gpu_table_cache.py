"""Keying of the cached device offset tables (DevTables in mpsk_api_internal.h: jordan_tab, pair_tab, dense_tab on a slice,
product_tab on a ctx).  A table is built on the first call at a shape and found again by its key; a wrong key would hand a
later shape the offsets of an earlier one, silently.  So ONE slice and ONE ctx are asked for shape A, then B, then A again,
and every result must be, bit for bit, what the same call returns on a slice and a ctx created for that call alone.

Operands come from the helpers the exact tests use (tests/exact_canonical_inputs.py, exact_dense_inputs.py,
exact_proj_inputs.py); whether the results are RIGHT is checked there, against exact references.  The shapes are the
smallest with distinct keys: bonds 8 and 12."""
import numpy as np
import pytest
import torch

import exact_inputs as ei
import exact_canonical_inputs as eci
import exact_dense_inputs as ed
import exact_proj_inputs as epi
import mpskit_jl_amd as mk

pytestmark = pytest.mark.gpu

BONDS = [(8, 8), (8, 12), (12, 8), (8, 8)]                 # (Dl, Dr): jtabR is keyed by the pair, jtabL / ptab by Dl
DENSE_SLICE = (4, 4, 2)                                    # (Wl, Wr, d): min(Wl, Wr) d = 8, the GEMM route without forcing
DENSE_BONDS = [8, 12, 8]
PRODUCT_BONDS = [(8, 8, 8), (8, 12, 8), (8, 8, 8)]         # (Dl, Dm, Dr)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.buf[:a.size], b.buf[:b.size])


def _fresh(call):
    """call(backend) on a ctx of its own"""
    b2 = mk.Backend(0)
    try:
        return call(b2)
    finally:
        b2.close()


def _sparse(be, s):
    return be.mposlice(s.odim, s.d, s.chil, s.chir, dict(s.Os))


# ---- canonical transfers: jordan_tab (MPSK_TRANSFER_MODE=1 and 2) and pair_tab (2) -----------------------------------
def heisenberg_slice():
    import mpskit_oracle as mo
    s = mo.heisenberg_mpo(0.5)[0]
    assert (sum(s.chil), s.d) == (5, 2)
    return s


def transfer_operands(side, s, Dl, Dr):
    """the isometry and the input environment with its identity level, as eci.transfer_case builds them"""
    left = side == "l"
    chis = list(s.chil)
    A = (eci.left_isometry if left else eci.right_isometry)(Dl, s.d, Dr)
    G = eci.env(ei._rng(f"table-cache-{side}-{Dl}x{Dr}"), ei.int_array, Dl if left else Dr, chis, 0 if left else len(chis) - 1)
    return A, G


def _transfer(be, H, side, A, G):
    dA = be.upload(A)
    call = be.transfer_left if side == "l" else be.transfer_right
    out = call(H, be.upload_env(G), dA, dA, canonical=True)
    return out, be.transfer_stats()["pair"]


@pytest.mark.parametrize("mode", ["1", "2"])
@pytest.mark.parametrize("side", ["l", "r"])
def test_canonical_transfer_tables_follow_the_shape(be, monkeypatch, side, mode):
    monkeypatch.setenv("MPSK_TRANSFER_MODE", mode)         # read per call: 1 level by level, 2 pair-Gram
    s = heisenberg_slice()
    H = _sparse(be, s)
    n0 = be.transfer_stats()["pair"]
    for k, (Dl, Dr) in enumerate(BONDS):
        A, G = transfer_operands(side, s, Dl, Dr)
        got, n = _transfer(be, H, side, A, G)
        ref, n_ref = _fresh(lambda b2: _transfer(b2, _sparse(b2, s), side, A, G))
        # the route asked for did run, on both handles: every call under mode 2 is counted, none under mode 1
        assert (n - n0, n_ref) == ((k + 1, 1) if mode == "2" else (0, 0)), (k, n - n0, n_ref)
        assert _same(got, ref), f"visit {k}: {side} transfer at {Dl} x {Dr}, MPSK_TRANSFER_MODE={mode}"


# ---- dense slice: dense_tab --------------------------------------------------------------------------------------------
def _dense_calls(be, H, t):
    G, R, x = be.upload_env([t["G"]]), be.upload_env([t["R"]]), be.upload(t["x"])
    h = be.hac_create(H, G, R)
    try:
        assert h.info()["mode"] == 4, h.info()              # the GEMM route of a dense slice: dense_route holds
    finally:
        h.close()
    return be.dAC(H, G, R, x), be.transfer_left(H, be.upload_env([t["Gt"]]), x, be.upload(t["Ab"]))


def test_dense_tables_follow_the_bond(be, monkeypatch):
    monkeypatch.delenv("MPSK_DENSE_ROUTE", raising=False)
    O = ed.dense_O(DENSE_SLICE)
    H = be.mposlice_dense(O)
    for k, D in enumerate(DENSE_BONDS):
        t = ed.site(DENSE_SLICE, (D, D), "int", "", ed.square_aux((D, D)))
        got = _dense_calls(be, H, t)
        ref = _fresh(lambda b2: _dense_calls(b2, b2.mposlice_dense(O), t))
        for op, g, r in zip(("dAC", "transfer_left"), got, ref):
            assert _same(g, r), f"visit {k}: {op} at D = {D}"


# ---- product tables of the ctx: product_tab ----------------------------------------------------------------------------
def product_operands():
    rng = ei._rng("table-cache-product")
    chis, d = (1, 2, 1), 2
    W = sum(chis)
    s1, s2 = epi._slice(rng, chis, d, "int", False), epi._slice(rng, chis, d, "int", False)
    ops = {}
    for Dl, Dm, Dr in sorted(set(PRODUCT_BONDS)):
        ops[(Dl, Dm, Dr)] = dict(G=ei.int_array(rng, Dl, W, Dl), R=ei.int_array(rng, Dr, W, Dr),
                                 AC=ei.int_array(rng, Dl, d, Dm), AR=ei.int_array(rng, Dm, d, Dr))
    return s1, s2, list(chis), ops


def _product(be, H1, H2, chis, t):
    env = lambda k: be.upload_env(epi._unstack(t[k], chis))
    return be.dAC2_product(H1, H2, env("G"), env("R"), be.upload(t["AC"]), be.upload(t["AR"]))


def test_product_tables_follow_the_middle_bond(be):
    s1, s2, chis, ops = product_operands()
    H1, H2 = _sparse(be, s1), _sparse(be, s2)
    for k, shape in enumerate(PRODUCT_BONDS):
        got = _product(be, H1, H2, chis, ops[shape])
        ref = _fresh(lambda b2: _product(b2, _sparse(b2, s1), _sparse(b2, s2), chis, ops[shape]))
        assert _same(got, ref), f"visit {k}: dAC2_product at (Dl, Dm, Dr) = {shape}"
