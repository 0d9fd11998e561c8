"""Time-dependent operators on the host stand-in backend (tests/cpu_backend.py): MultipliedOperator / TimedOperator /
UntimedOperator algebra, timed LazySum evaluation and its misuse errors (reference: test/operators.jl:101-157), and the
derivatives of a timed sum at t against the sum of f_k(t) times the parts (test/operators.jl:251-278)."""
import numpy as np
import pytest

import mpskit_oracle as mo
import mpskit_jl_amd as mk
from mpskit_jl_amd import derivatives
from cpu_backend import CpuBackend


@pytest.fixture()
def cb():
    return CpuBackend()


def _state(cb, L=6, d=2, D=6, seed=0):
    rng = np.random.default_rng(seed)
    dims = mo.FiniteMPS.random(L, d, D, np.random.default_rng(0)).bond_dims()
    As = [rng.random((1 if i == 0 else dims[i - 1], d, dims[i])) for i in range(L)]
    return mk.FiniteMPS(As, normalize=True, be=cb)


f1 = lambda t: 1.0 + t
f2 = lambda t: np.cos(t)


def test_multiplied_operator_algebra(cb):
    H = mk.transverse_field_ising(1.0, 0.5, be=cb)
    ut, tm = mk.UntimedOperator(H, 3.0), mk.TimedOperator(H, f1)
    assert isinstance(ut, mk.MultipliedOperator) and isinstance(tm, mk.MultipliedOperator)
    assert not mk.istimed(ut) and mk.istimed(tm) and not mk.istimed(H)
    assert mk.istimed(mk.TimedOperator(H)) and mk.TimedOperator(H)(0.3).f == 1.0
    at = tm(2.0)                                            # x(t) on a timed operator: the untimed one
    assert not mk.istimed(at) and at.op is H and at.f == 3.0
    plain = ut()                                            # x() on an untimed one: f * op
    ref = H * 3.0
    for a, b in zip(plain.slices, ref.slices):
        assert a.blocks.keys() == b.blocks.keys()
        assert all(np.array_equal(np.asarray(a.blocks[k]), np.asarray(b.blocks[k])) for k in a.blocks)
    with pytest.raises(ValueError):
        tm()
    with pytest.raises(ValueError):
        ut(1.0)
    # op * callable, products of factors (multipliedoperator.jl:40-46)
    assert mk.istimed(H * f1) and (H * f1)(1.0).f == 2.0
    assert (2.0 * ut).f == 6.0 and (ut * 2.0).f == 6.0
    assert mk.istimed(tm * 2.0) and (tm * 2.0)(1.0).f == 4.0 and (tm * f2)(0.0).f == 1.0
    with pytest.raises(TypeError):
        mk.UntimedOperator(H, f1)
    # sums
    s = ut + tm
    assert isinstance(s, mk.LazySum) and len(s) == 2 and mk.istimed(s) and s(1.0).fs == [3.0, 2.0]
    s2 = H + tm
    assert isinstance(s2, mk.LazySum) and s2[0] is H and s2(0.5).fs == [1.0, 1.5]
    s3 = s2 + ut
    assert len(s3) == 3 and mk.istimed(s3) and s3(0.0).fs == [1.0, 1.0, 3.0]
    assert not mk.istimed(ut + ut) and (ut + ut).fs == [3.0, 3.0]


def test_lazysum_time_evaluation_and_misuse(cb):
    Ha, Hb = mk.transverse_field_ising(1.0, 0.0, be=cb), mk.transverse_field_ising(0.0, 1.0, be=cb)
    Ht = mk.LazySum([Ha, Hb], [f1, 0.5])
    assert mk.istimed(Ht)
    H1 = Ht(1.0)
    assert isinstance(H1, mk.LazySum) and not mk.istimed(H1) and H1.fs == [2.0, 0.5] and list(H1) == [Ha, Hb]
    with pytest.raises(ValueError, match="untimed"):
        H1(1.0)                                             # lazysum.jl:36-43
    with pytest.raises(ValueError, match="untimed"):
        Ht.fs
    # repeat and + keep the time dependence
    r = Ht.repeat(2)
    assert mk.istimed(r) and r(1.0).fs == [2.0, 0.5] and len(r[0]) == 2
    assert mk.istimed(Ht + Ha) and (Ht + Ha)(0.0).fs == [1.0, 0.5, 1.0]
    assert mk.istimed(Ht + mk.LazySum([Ha])) and mk.istimed(mk.LazySum([Ha]) + Ht)
    # an untimed sum keeps its attributes
    Hu = mk.LazySum([Ha, Hb], [0.25, 0.75])
    assert Hu.fs == [0.25, 0.75] and not mk.istimed(Hu) and (Hu + Hu).fs == [0.25, 0.75, 0.25, 0.75]
    assert mk.LazySum([Ha, Hb]).fs == [1.0, 1.0]
    with pytest.raises(ValueError):
        mk.LazySum([Ha, Hb], [1.0])


def test_environments_of_multiplied_and_timed(cb):
    psi = _state(cb)
    Ha, Hb = mk.transverse_field_ising(1.0, 0.0, be=cb), mk.transverse_field_ising(0.0, 1.0, be=cb)
    e = mk.environments(psi, mk.TimedOperator(Ha, f1))
    assert type(e) is mk.FinEnv and e.H is Ha               # multipliedoperator.jl:50-52
    et = mk.environments(psi, mk.LazySum([Ha, Hb], [f1, f2]))
    assert isinstance(et, mk.MultipleEnvironments) and len(et.envs) == 2
    eu = mk.environments(psi, mk.LazySum([Ha, Hb]))
    assert all(not x.canonical for x in eu.envs)            # the terms of an untimed sum keep the dense transfers
    Hfull = mk.transverse_field_ising(1.0, 1.0, be=cb)
    Ht = mk.LazySum([Ha, Hb], [f1, f2])
    E = mk.expectation_value(psi, Ht(0.0), et)              # f1(0) = f2(0) = 1
    assert np.abs(E - mk.expectation_value(psi, Hfull, mk.environments(psi, Hfull))).max() < 1e-12
    with pytest.raises(ValueError, match=r"H\(t\)"):
        mk.expectation_value(psi, Ht, et)
    with pytest.raises(ValueError, match=r"H\(t\)"):
        mk.find_groundstate(psi, Ht, mk.DMRG(maxiter=1))


@pytest.mark.parametrize("fn,tensor", [("ddAC", "AC"), ("ddC", "C"), ("ddAC2", "AC2")])
def test_timed_derivatives_are_the_weighted_sum_of_the_parts(cb, fn, tensor):
    from mpskit_jl_amd.algorithms import _two_site_tensor
    psi = _state(cb, seed=3)
    Hs = [mk.heisenberg_XXX(0.5, be=cb), mk.transverse_field_ising(1.0, 0.5, be=cb), mk.transverse_field_ising(0.0, 1.0, be=cb)]
    fs = [f1, f2, 0.75]
    Ht = mk.LazySum(Hs, fs)
    envs = mk.environments(psi, Ht)
    dd = getattr(mk, fn)
    pos = 2
    x = {"AC": lambda: psi.AC(pos), "C": lambda: psi.CR(pos),
         "AC2": lambda: _two_site_tensor(cb, psi.AC(pos), psi.AR(pos + 1))}[tensor]()
    h = dd(pos, psi, Ht, envs)
    parts = [cb.download(dd(pos, psi, Hk, ek)(x)) for Hk, ek in zip(Hs, envs.envs)]
    for t in (0.0, 0.7, 2.5):
        ref = sum((f(t) if callable(f) else f) * p for f, p in zip(fs, parts))
        y = cb.download(h(x, t))
        assert np.abs(y - ref).max() <= 1e-13 * np.abs(ref).max()
        out = cb.empty(*x.shape)
        assert h(x, t, out=out) is out and np.array_equal(cb.download(out), y)       # the sum passes `out` down
        assert np.array_equal(cb.download(h.at(t)(x)), y)
        yu = cb.download(dd(pos, psi, Ht(t), envs)(x))                                 # the evaluated sum: the old route
        assert np.abs(yu - ref).max() <= 1e-13 * np.abs(ref).max()
    with pytest.raises(ValueError, match="time"):
        h(x)                                                # a timed operator called without t
    # a MultipliedOperator: f times the derivative of op, callable without t when untimed
    e0 = envs.envs[0]
    hm = dd(pos, psi, mk.TimedOperator(Hs[0], f1), e0)
    assert np.abs(cb.download(hm(x, 1.0)) - 2.0 * parts[0]).max() <= 1e-13 * np.abs(parts[0]).max()
    hu = dd(pos, psi, mk.UntimedOperator(Hs[0], 3.0), e0)
    assert np.abs(cb.download(hu(x)) - 3.0 * parts[0]).max() <= 1e-13 * np.abs(parts[0]).max()
    with pytest.raises(ValueError, match="time"):
        hm(x)


def test_untimed_lazysum_is_bit_identical_to_the_composed_formula(cb):
    """the untimed sum keeps derivatives.LazyDerivativeSum and its dense terms: term 0 scaled in place, every further term
    added by one axpby -- reproduced here call by call on a fixed input."""
    psi = _state(cb, seed=5)
    Ha, Hb = mk.heisenberg_XXX(0.5, be=cb), mk.transverse_field_ising(1.0, 0.5, be=cb)
    Hu = mk.LazySum([Ha, Hb], [0.25, 0.75])
    envs = mk.environments(psi, Hu)
    pos, x = 3, psi.AC(3)
    h = mk.ddAC(pos, psi, Hu, envs)
    assert type(h) is derivatives.LazyDerivativeSum and h.fs == [0.25, 0.75]
    assert all(type(t) is derivatives.MPO_ddAC and not t.canonical for t in h.terms)
    y = cb.download(h(x))
    ta, tb = (mk.ddAC(pos, psi, H, e, canonical=False) for H, e in zip(Hu, envs.envs))
    ref = ta(x)
    cb.scal(0.25, ref)
    cb.axpby(0.75, tb(x), 1.0, ref)
    assert np.array_equal(y, cb.download(ref))
