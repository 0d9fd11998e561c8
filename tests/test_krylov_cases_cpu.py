"""tests/krylov_cases.py on the host stand-in: every case converges there within its maxiter, the inputs have the gaps,
condition numbers and structure the cases are named for, and the host run alone meets every bar that
tests/test_gpu_krylov_paths.py holds the device to.  The KRYLOV-BOUNDS lines (`pytest -s`) are the host figures kept in
profiles/krylov_paths_bounds.log."""
import numpy as np
import pytest

import krylov_cases as kc


@pytest.fixture(scope="module")
def hb():
    return kc.host_backend()


def _log(what, **figures):
    print("KRYLOV-BOUNDS host " + what + ": " + ", ".join(
        f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}" for k, v in figures.items()))


def test_hide_forwards_everything_but_the_named_attributes():
    class B:
        x = 3

        def f(self):
            return self.x

        def g(self):
            return 7
    b = B()
    h = kc.hide(b, "g")
    assert h.f() == 3 and h.x == 3 and hasattr(h, "f") and not hasattr(h, "g")
    with pytest.raises(AttributeError):
        h.g
    h.y = 5                                             # state set through the proxy lands on the backend
    assert b.y == 5 and h.y == 5
    with pytest.raises(AssertionError):
        kc.hide(b, "no_such_method")


@pytest.mark.parametrize("name", list(kc.EIG))
def test_eigsolve_cases(hb, name):
    c = kc.eig_case(name)
    n, m = c["n"], c["krylovdim"]
    assert c["gap"] > 100 * c["tol"]
    g = kc.run_eig(hb, name, first=True)
    f = kc.check_eig(name, g)                           # includes res <= tol: converged within maxiter
    assert g["nmv"] == g["applied"]
    keep = (3 * m) // 5
    if name[0] == "a":
        assert g["nmv"] <= m                            # inside the first cycle
    if name[0] == "b":
        assert m <= 32 and g["nmv"] >= m + 3 * (m - keep)   # at least three shrinks, through multilincomb on a device
    if name[0] == "c":
        assert m > 32 and g["nmv"] > m                  # at least one shrink, through the lincomb loop
    if name[0] == "d":
        assert g["nmv"] == 3 and g["res"] == 0.0        # beta_3 is exactly zero
        sub = np.zeros(n, dtype=bool)
        sub[list(kc.D_SUPPORT)] = True
        assert not g["v"][~sub].any()
        assert np.array_equal(g["first"], c["A"][:, kc.D_SUPPORT[0]])
    if name[0] == "e":
        assert g["nmv"] == n
    ref, bound = kc.first_image_bound(name)
    ferr = np.abs(g["first"].astype(kc.LD) - ref)
    assert bool((ferr <= bound).all())
    _log("eigsolve_sr " + name, nmv=g["nmv"], res=g["res"], r_true=f["r"], lam_err=f["lam_err"], sin=f["sin"], gap=f["gap"],
         r_ref=c["r_ref"], first_image=float((ferr[bound > 0] / bound[bound > 0]).max()))


@pytest.mark.parametrize("name", list(kc.GMRES))
def test_gmres_cases(hb, name):
    c = kc.gmres_case(name)
    assert c["cond"] <= 2.3 + 1e-12                     # (hi + skew) / lo of krylov_cases.nonsym
    g = kc.run_gmres(hb, name)
    f = kc.check_solve(c, g["x"])
    assert g["info"]["converged"] is True and g["info"]["normres"] <= c["tol"]
    if name.startswith("one"):
        assert 1 < g["applied"] <= c["krylovdim"] + 1   # one cycle
    if name.startswith("restart"):
        assert g["applied"] > 2 * (c["krylovdim"] + 1)
    if name == "zero_b":
        assert g["applied"] == 0 and not g["x"].any() and g["info"]["normres"] == 0.0
    if name == "exact_x0":
        assert g["applied"] == 1 and np.array_equal(g["x"], c["x0"])
    _log("gmres " + name, applied=g["applied"], normres=g["info"]["normres"], r_true=f["r"], err=f["err"], inv_norm=c["inv_norm"],
         r_ref=c["r_ref"])


def test_nested_solve(hb):
    c = kc.nest_case()
    assert kc.NEST_TOL_INNER <= 1e-3 * kc.NEST_TOL_OUTER and c["gap"] > 100 * kc.NEST_TOL_OUTER
    g = kc.run_nest(hb)
    f = kc.check_nest(g)
    assert g["unconverged"] == 0 and g["res"] <= kc.NEST_TOL_OUTER
    _log("nested", nmv=g["nmv"], inner=g["inner"], res=g["res"], rho=f["rho"], lam_err=f["lam_err"], sin=f["sin"])


@pytest.mark.parametrize("name", list(kc.EXPO) + list(kc.EXPO_GENERAL))
def test_exponentiate_cases(hb, name):
    c = kc.expo_case(name)
    g = kc.run_expo(hb, name)
    f = kc.check_expo(name, g)
    if name.startswith("cut"):
        assert g["nmv"] > 2 * c["krylovdim"]            # more than one sub-step
    elif name.startswith("zero"):
        assert g["nmv"] == 0 and not g["y"].any()
    elif name.startswith("eigvec"):
        assert g["nmv"] == 1
    else:
        assert g["nmv"] <= c["krylovdim"]
    if name.startswith("rot"):
        assert np.abs(c["A"] + c["A"].T).max() == 0.0   # antisymmetric generator: a rotation
        assert abs(kc.nrm(g["y"]) - 1.0) <= f["err"] + abs(kc.nrm(c["ref"]) - 1.0)     # it keeps the norm: triangle inequality
    _log("exponentiate " + name, nmv=g["nmv"], err=f["err"])


@pytest.mark.parametrize("n", [96, 257])
def test_perron_case(hb, n):
    c = kc.perron_case(n)
    assert c["A"].min() > 0 and abs(c["lam"] - 1.0) <= 1e-13 and c["second"] < 0.1
    assert np.abs(c["A"] - c["A"].T).max() > 1e-3       # not symmetric
    g = kc.run_perron(hb, n)
    f = kc.check_perron(n, g)                           # includes r_true <= tol: the solver returns no residual of its own
    assert g["applied"] <= 30                           # inside the first cycle
    _log(f"eigsolve_lm_real perron{n}", applied=g["applied"], r_true=f["r"], lam_err=f["lam_err"], kappa=c["kappa"], r_ref=c["r_ref"])


def test_pair_case(hb):
    c = kc.pair_case()
    lam = c["lam"]
    assert abs(lam[0] - 2.0) <= 1e-12 and abs(abs(lam[1]) - 1.5) <= 1e-12 and lam[1] == np.conj(lam[2]) and abs(lam[1].imag) > 1.0
    assert c["fourth"] <= 0.5 + 1e-12 and c["kappa"].max() < 2.0
    g = kc.run_arnoldi(hb)
    f = kc.check_arnoldi(g)
    _log("arnoldi_eigvals pair", applied=g["applied"], err=f["err"].tolist(), kappa=c["kappa"].tolist())
    g = kc.run_planar(hb)
    f = kc.check_planar(g)
    _log("eigsolve_lm_planar pair", applied=g["applied"], r_true=f["r"].tolist(), res=g["res"].tolist())


def test_linsolve_complex_case(hb):
    c = kc.linsolve_case()
    assert c["cond"] < 20
    g = kc.run_linsolve(hb)
    i = g["info"]
    f = kc.check_solve(c, g["x"])
    assert i.converged == 1 and i.normres <= c["tol"] and np.iscomplexobj(i.hessenberg)
    assert i.numops > 33                                # more steps than mpsk_vorth_step_c takes basis vectors
    _log("linsolve complex", numops=i.numops, numiter=i.numiter, normres=i.normres, r_true=f["r"], err=f["err"], inv_norm=c["inv_norm"])


def test_linsolve_apply_axpby_case(hb):
    c = kc.hac_case()
    assert c["cond"] < 3
    g = kc.run_hac(hb)
    i = g["info"]
    f = kc.check_solve(c, g["x"])
    assert g["mode"] == 3 and i.converged == 1 and i.normres <= c["tol"]
    _log("linsolve apply_axpby", numops=i.numops, normres=i.normres, r_true=f["r"], err=f["err"], inv_norm=c["inv_norm"])
