"""Pair-Gram route of the canonical transfers (MPSK_TRANSFER_MODE=2 forces it, unset leaves the choice to the model)
against the level-by-level canonical route (=1) and the dense three-stage route (=0) on exactly representable operands
(tests/exact_canonical_inputs.py: integer environments and slices, dyadic isometries): all three routes and the oracle
are exact there, so the bar is np.array_equal.  Shapes: the smallest that reach each path -- one tile, ragged Dl != Dr,
odd dimensions (scalar loads, unaligned tables), Dl d == Dr, d = 3 with all six pairs over two tile rows, the Hubbard
slice (d = 4), the Ising slice (one interior level: never the pair route), a model-chosen bulk shape, a fresh ctx."""
import numpy as np
import pytest

import exact_inputs as ei
import exact_canonical_inputs as eci

pytestmark = pytest.mark.gpu

BAR = 1e-10                 # random operands against the oracle / sweep energies: the bar of test_gpu_transfer_canonical


def _int_slice(kind):
    """integer Jordan-form slices beyond the families of exact_canonical_inputs"""
    import mpskit_oracle as mo
    if kind == "hubbard":                                   # t = 1, U = 4: every entry an integer
        return mo.hubbard_mpo(1.0, 4.0)[0]
    if kind == "tfi":                                       # J = g = 1
        return mo.tfi_mpo(1.0, 1.0)[0]
    assert kind == "s1"                                     # S = 1 pattern (Sz, S+, S-) plus a dense D block: all six pairs
    rng = ei._rng("pairgram-s1")
    Sz = np.diag([1.0, 0.0, -1.0])
    Sp = np.diag([1.0, 2.0], 1)
    D = ei.int_array(rng, 3, 3)
    D = np.where(D == 0, 1.0, D)
    return mo.mpoham_from_chain({(0, 0): 1.0, (4, 4): 1.0, (0, 1): 2 * Sz, (1, 4): Sz, (0, 2): Sp, (2, 4): Sp.T,
                                 (0, 3): 3 * Sp.T, (3, 4): Sp, (0, 4): D}, 3)


_cache = {}


def case(side, slc, Dl, d, Dr):
    """a transfer case like eci.transfer_case; slc: a family of exact_canonical_inputs or a kind of _int_slice"""
    key = (side, slc, Dl, d, Dr)
    if key in _cache:
        return _cache[key]
    if slc in eci.FAMILIES:
        t = eci.transfer_case(side, slc, Dl, d, Dr)
    else:
        import mpskit_oracle as mo
        s = _int_slice(slc)
        assert s.d == d
        left = side == "l"
        O, chis = s.full(), list(s.chil)
        W, Dk = len(chis), (Dl if left else Dr)
        name = f"pairgram-{side}-{slc}-{Dl}x{d}x{Dr}"
        t = {"name": name, "op": "tl" if left else "tr", "s": s, "O": O, "chis": chis, "d": d, "cplx": False,
             "ident": 0 if left else W - 1, "n_out": Dr if left else Dl, "bound": None}
        t["A"] = (eci.left_isometry if left else eci.right_isometry)(Dl, d, Dr)
        G = eci.env(ei._rng(name), ei.int_array, Dk, chis, t["ident"])
        t["GL" if left else "GR"] = G
        u = eci.dyadic_unit(t["A"])
        eci._guard(t, [ei._stack(G), t["A"], t["A"], O], [Dk, W, d, Dk, d], unit=u * u)
        t["ref"] = ei._stack((mo.transfer_left if left else mo.transfer_right)(G, s, t["A"], t["A"]))
    _cache[key] = t
    return t


def run(be, monkeypatch, t, mode, H=None):
    """one transfer under MPSK_TRANSFER_MODE=mode (None: unset); returns (result, pair-route calls it made)"""
    with monkeypatch.context() as mp:
        if mode is None:
            mp.delenv("MPSK_TRANSFER_MODE", raising=False)
        else:
            mp.setenv("MPSK_TRANSFER_MODE", mode)
        n0 = be.transfer_stats()["pair"]
        got = eci.run_transfer(be, eci.make_slice(be, t) if H is None else H, t)
        return got, be.transfer_stats()["pair"] - n0


def mirror(side, shape):
    Dl, d, Dr = shape
    return shape if side == "l" else (Dr, d, Dl)


CASES = [("full", (64, 2, 64)), ("full", (40, 2, 72)), ("full", (33, 2, 65)), ("chi", (33, 2, 65)), ("full", (32, 2, 64)),
         ("sparse", (43, 3, 129)), ("s1", (130, 3, 192)), ("hubbard", (64, 4, 96))]


@pytest.mark.parametrize("slc,shape", CASES, ids=[f"{s}-{'x'.join(map(str, sh))}" for s, sh in CASES])
@pytest.mark.parametrize("side", ["l", "r"])
def test_pair_route_gives_the_bits_of_both_other_routes(be, monkeypatch, side, slc, shape):
    t = case(side, slc, *mirror(side, shape))
    H = eci.make_slice(be, t)
    pair, n2 = run(be, monkeypatch, t, "2", H)
    again, _ = run(be, monkeypatch, t, "2", H)              # cached offset tables, reused workspace
    lvl, n1 = run(be, monkeypatch, t, "1", H)
    dense, n0 = run(be, monkeypatch, t, "0", H)
    assert (n2, n1, n0) == (1, 0, 0), (n2, n1, n0)
    assert np.array_equal(pair[:, t["ident"], :], np.eye(t["n_out"]))
    for what, other in (("oracle", t["ref"]), ("second call", again), ("MPSK_TRANSFER_MODE=1", lvl), ("MPSK_TRANSFER_MODE=0", dense)):
        bad = ei.compare(pair, other, None, f"{t['name']} vs {what}")
        assert bad is None, bad


@pytest.mark.parametrize("side", ["l", "r"])
def test_ising_slice_and_small_shapes_keep_the_level_route(be, monkeypatch, side):
    """unset MPSK_TRANSFER_MODE: the model decides.  One interior level (Ising) is never sent to the pair route, and a
    launch-bound shape of a slice that has pairs is not either"""
    for slc in ("tfi", "full"):
        t = case(side, slc, 64, 2, 64)
        got, n = run(be, monkeypatch, t, None)
        assert n == 0, (slc, n)
        bad = ei.compare(got, t["ref"], None, t["name"])
        assert bad is None, bad
    t = case(side, "tfi", 64, 2, 64)                        # forced, the Ising slice (D block through the pairs) is exact too
    got, n = run(be, monkeypatch, t, "2")
    assert n == 1 and ei.compare(got, t["ref"], None, t["name"]) is None


@pytest.mark.parametrize("side", ["l", "r"])
def test_model_sends_a_bulk_shape_to_the_pair_route(be, monkeypatch, side):
    t = case(side, "full", 384, 2, 384)
    H = eci.make_slice(be, t)
    got, n = run(be, monkeypatch, t, None, H)
    lvl, n1 = run(be, monkeypatch, t, "1", H)
    assert (n, n1) == (1, 0)
    for other in (t["ref"], lvl):
        bad = ei.compare(got, other, None, t["name"])
        assert bad is None, bad


@pytest.mark.parametrize("side", ["l", "r"])
def test_fresh_ctx_first_call_is_the_largest_pair_transfer(be, monkeypatch, side):
    """workspace sizing: the first workspace user of a new ctx is the pair route at the largest shape of this file"""
    import mpskit_jl_amd as mk
    t = case(side, "s1", *mirror(side, (130, 3, 192)))
    b2 = mk.Backend(0)
    try:
        got, n = run(b2, monkeypatch, t, "2")
        assert n == 1
        bad = ei.compare(got, t["ref"], None, t["name"])
        assert bad is None, bad
        t4 = case(side, "hubbard", *mirror(side, (64, 4, 96)))      # more pairs afterwards
        got, _ = run(b2, monkeypatch, t4, "2")
        assert ei.compare(got, t4["ref"], None, t4["name"]) is None
    finally:
        b2.close()


@pytest.mark.parametrize("side", ["l", "r"])
def test_random_operands_against_the_oracle(be, monkeypatch, side):
    t = eci.transfer_case(side, "full", *mirror(side, (40, 2, 72)), "gauss")
    got, n = run(be, monkeypatch, t, "2")
    ref = t["oracle"]()
    e = np.abs(got - ref).max() / np.abs(ref).max()
    print(f"{t['name']}: pair route against the oracle, rel. max-norm error {e:.3e}")
    assert n == 1 and e <= BAR, e
    assert np.array_equal(got[:, t["ident"], :], np.eye(t["n_out"]))


def test_dmrg_sweeps_agree_between_the_routes(be, monkeypatch):
    """two fixed-budget sweeps at L = 12, D = 32: MPSK_TRANSFER_MODE=1, the default (the model) and the forced pair route"""
    import mpskit_jl_amd as mk
    from mpskit_jl_amd import algorithms as alg, krylov

    def sweeps(mode):
        with monkeypatch.context() as mp:
            if mode is None:
                mp.delenv("MPSK_TRANSFER_MODE", raising=False)
            else:
                mp.setenv("MPSK_TRANSFER_MODE", mode)
            H = mk.heisenberg_XXX(0.5, be=be)
            psi = mk.FiniteMPS.random(12, 2, 32, np.random.default_rng(9), normalize=True, be=be)
            envs = mk.FinEnv(psi, H)
            eig = mk.Arnoldi(fixed_matvecs=8, krylovdim=8)
            ws = krylov.KrylovWorkspace(be)
            n0 = be.transfer_stats()["pair"]
            for _ in range(2):
                alg.dmrg_sweep(psi, H, envs, eig, ws)
            E = float(np.sum(alg.expectation_value(psi, H, envs)))
            return E, be.transfer_stats()["pair"] - n0, envs.n_transfers

    e1, n1, nt = sweeps("1")
    ed, nd, _ = sweeps(None)
    e2, n2, _ = sweeps("2")
    print(f"energies: level route {e1:.15f}, default {ed:.15f}, pair route {e2:.15f}; pair-route transfers {n1} / {nd} / {n2} of {nt}")
    assert n1 == 0 and n2 == nt > 0
    assert abs(ed - e1) <= BAR * abs(e1) and abs(e2 - e1) <= BAR * abs(e1), (e1, ed, e2)
