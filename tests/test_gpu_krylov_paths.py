"""mpskit_jl_amd/krylov.py driven by the real Backend, on the branches the host stand-in never takes: the one-step-ahead
expansion of eigsolve_sr and gmres (Backend.orth_step_async / _OrthHandle: pinned slot pairs, events, the free list, the
__del__ of a dropped handle), the multilincomb basis rotation of the thick restart and its lincomb fallback above 32
vectors, the native entry points behind ComplexVec, the apply_axpby route of linsolve, and the solvers that had no
device test of their own (gmres, eigsolve_lm_real, exponentiate_general, arnoldi_eigvals, eigsolve_lm_planar).

Cases, references and bars are those of tests/krylov_cases.py; tests/test_krylov_cases_cpu.py proves them on the host
stand-in, and the host figures (profiles/krylov_paths_bounds.log) are recomputed here in-process, since n <= 257.

Exact parity.  mpsk_vorth_step and mpsk_vorth_step_dev enqueue the same vec_cgs2 and vec_scal_rsqrt_dev launches and both
hosts form h1 + h2 and a correctly rounded square root, so `be` and hide(be, "orth_step_async") build bit-identical
projected matrices and take identical decisions: vectors are compared with np.array_equal, lam / res / info with ==,
and the speculative run applies the operator at most once more (the discarded step).  The same holds for a reused
against a fresh KrylovWorkspace and for the nested solve.  Matvec counts against the HOST run are printed, not asserted:
a decision at the 1e-12 threshold may flip between two correct roundings.

Slot ownership.  After every solve no _OrthHandle is alive and the free list has the length it had after the first of
two identical solves; the nested solve (an inner gmres inside the matvec of an outer eigsolve_sr that has a handle in
flight, as the quasiparticle effective Hamiltonian does it) does not grow it either.

Case (d), the exact breakdown: the third remainder is exactly zero, vec_scal_rsqrt_dev takes its n2 <= 0 branch and
writes a ZERO vector, so the speculative fourth step (operator applied to that vector) leaves zeros, not NaNs, in the
pool; the Ritz vector does not involve it.  The reuse test therefore also fills the whole pool with NaN before the next
solve: nothing may be read from a workspace before it is written.

Read while writing these (no GPU test drives them): between side_begin and side_end (algorithms.py, left-moving visits
of the DMRG sweep) only _galerkin runs -- one operator application, normalize_dev, two GEMMs and nrm2_dev / norm -- so no
Krylov solve, and no orth_step_async copy on torch_stream, is reachable while the ctx is on its second stream.  The
basis / spare rotation of the shrink keeps spare[:keep] out of basis[:m] at every restart: the new spare is the tail of
the old basis, which the new basis does not contain (mpsk_vmultilincomb also refuses aliased outputs; cases b run 6 to 8
shrinks over the 13 vectors of the pool).  These tests found no bug in krylov.py or backend.py."""
import functools
import gc

import numpy as np
import pytest

import krylov_cases as kc
from mpskit_jl_amd import krylov
from mpskit_jl_amd.backend import Backend

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def host(kind, name=None):
    """the same case through tests/cpu_backend.py, once per module run"""
    hb = kc.host_backend()
    run = {"eig": kc.run_eig, "gmres": kc.run_gmres, "expo": kc.run_expo, "perron": kc.run_perron}
    if kind in run:
        return run[kind](hb, name)
    return {"nest": kc.run_nest, "arnoldi": kc.run_arnoldi, "planar": kc.run_planar, "linsolve": kc.run_linsolve,
            "hac": kc.run_hac}[kind](hb)


def live_handles():
    gc.collect()
    return sum(type(o) is Backend._OrthHandle for o in gc.get_objects())


def free_slots(be):
    return len(getattr(be, "_orth_free", []))


def plain(be):
    return kc.hide(be, "orth_step_async")


def _log(what, **figures):
    print("KRYLOV-BOUNDS device " + what + ": " + ", ".join(
        f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}" for k, v in figures.items()))


# ---- eigsolve_sr, tolerance mode -------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", kc.SPEC_EIG)
def test_eigsolve_speculative_equals_plain_and_meets_the_dense_bars(be, name):
    c = kc.eig_case(name)
    gs = kc.run_eig(be, name, first=True)
    assert live_handles() == 0
    nfree = free_slots(be)
    gp = kc.run_eig(plain(be), name, first=True)
    assert free_slots(be) == nfree                                         # the plain run touches no slot
    again = kc.run_eig(be, name, first=True)
    assert live_handles() == 0 and free_slots(be) == nfree                 # every slot came back, none was added
    h = host("eig", name)
    fh = kc.eig_figures(name, h)
    f = kc.check_eig(name, gs, r_host=fh["r"])
    _log("eigsolve_sr " + name, nmv=gs["nmv"], nmv_plain=gp["nmv"], nmv_host=h["nmv"], res=gs["res"], r_true=f["r"], r_host=fh["r"],
         lam_err=f["lam_err"], sin=f["sin"], slots=nfree)
    for g in (gp, again):
        assert np.array_equal(g["v"], gs["v"]) and g["lam"] == gs["lam"] and g["res"] == gs["res"]
        assert np.array_equal(g["first"], gs["first"])
    assert again["nmv"] == gs["nmv"]
    assert gs["nmv"] - gp["nmv"] in (0, 1) and gs["applied"] == gs["nmv"] and gp["applied"] == gp["nmv"]
    # (f) first_image = A x0 / |x0|
    ref, bound = kc.first_image_bound(name)
    ferr = np.abs(gs["first"].astype(kc.LD) - ref)
    print(f"KRYLOV-BOUNDS device first_image {name}: err / bound {float((ferr[bound > 0] / bound[bound > 0]).max(initial=0.0)):.3f}")
    assert bool((ferr <= bound).all())
    if name[0] == "c":                                                     # m = 40: at least one shrink through the lincomb loop
        assert gp["nmv"] > c["krylovdim"]
    if name[0] == "d":                                                     # the exact breakdown, one discarded step
        assert gp["nmv"] == 3 and gs["nmv"] == 4 and gs["res"] == 0.0
        assert np.array_equal(gs["first"], c["A"][:, kc.D_SUPPORT[0]])
    if name[0] == "e":
        assert gp["nmv"] == c["n"]


@pytest.mark.parametrize("name", ["b96", "b257"])
def test_thick_restart_through_multilincomb_and_through_the_lincomb_loop(be, name):
    """two kernels with their own order of summation, so equal bits are not asked (at m = 8 an MI355X did return the same
    bits: mpsk_vlincomb adds its first eight vectors in one launch, in the order of the multilincomb accumulator); both
    meet the dense bars"""
    fh = kc.eig_figures(name, host("eig", name))
    g1 = kc.run_eig(be, name)
    g2 = kc.run_eig(kc.hide(be, "multilincomb"), name)
    f1, f2 = kc.check_eig(name, g1, r_host=fh["r"]), kc.check_eig(name, g2, r_host=fh["r"])
    m = kc.eig_case(name)["krylovdim"]
    assert g1["nmv"] > m + 3 * (m - (3 * m) // 5) and g2["nmv"] > m + 3 * (m - (3 * m) // 5)      # several shrinks each
    _log("shrink " + name, nmv_multilincomb=g1["nmv"], nmv_lincomb=g2["nmv"], r_multilincomb=f1["r"], r_lincomb=f2["r"], r_host=fh["r"],
         dv=float(np.abs(g1["v"] - g2["v"]).max()))


def test_workspace_after_a_discarded_speculative_step(be):
    """case (d) leaves its discarded fourth step in the pool; an ordinary solve on the same KrylovWorkspace returns the bits
    of the same solve on a fresh one -- also when every pooled buffer holds NaN"""
    ws = krylov.KrylovWorkspace(be)
    gd = kc.run_eig(be, "d96", ws=ws)
    kc.check_eig("d96", gd, r_host=kc.eig_figures("d96", host("eig", "d96"))["r"])
    assert gd["nmv"] == 4 and len(ws.pool[(None, (96, 1))]) == 32
    fresh = kc.run_eig(be, "a96", first=True)
    reused = kc.run_eig(be, "a96", ws=ws, first=True)
    for bufs in ws.pool.values():
        for t in bufs:
            t.buf.fill_(float("nan"))
    poisoned = kc.run_eig(be, "a96", ws=ws, first=True)
    for g in (reused, poisoned):
        assert np.array_equal(g["v"], fresh["v"]) and g["lam"] == fresh["lam"] and g["res"] == fresh["res"] and g["nmv"] == fresh["nmv"]
        assert np.array_equal(g["first"], fresh["first"])
    assert live_handles() == 0


# ---- gmres -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", kc.SPEC_GMRES)
def test_gmres_speculative_equals_plain_and_meets_the_dense_bars(be, name):
    c = kc.gmres_case(name)
    gs = kc.run_gmres(be, name)
    assert live_handles() == 0
    nfree = free_slots(be)
    gp = kc.run_gmres(plain(be), name)
    again = kc.run_gmres(be, name)
    assert live_handles() == 0 and free_slots(be) == nfree
    h = host("gmres", name)
    fh = kc.solve_figures(c, h["x"])
    f = kc.check_solve(c, gs["x"], r_host=fh["r"])
    _log("gmres " + name, applied=gs["applied"], applied_plain=gp["applied"], applied_host=h["applied"], normres=gs["info"]["normres"],
         r_true=f["r"], r_host=fh["r"], err=f["err"])
    for g in (gp, again):
        assert np.array_equal(g["x"], gs["x"]) and g["info"] == gs["info"]
    assert again["applied"] == gs["applied"] and gs["applied"] - gp["applied"] in (0, 1)
    assert set(gs["info"]) == {"converged", "normres"} and gs["info"]["converged"] is True and gs["info"]["normres"] <= c["tol"]
    if name == "zero_b":
        assert gs["applied"] == 0 and not gs["x"].any() and gs["info"]["normres"] == 0.0
    if name == "exact_x0":
        assert gs["applied"] == 1 and np.array_equal(gs["x"], c["x0"])
    if name.startswith("one"):
        assert gp["applied"] <= c["krylovdim"] + 1
    if name.startswith("restart"):
        assert gp["applied"] > 2 * (c["krylovdim"] + 1)


def test_nested_solve_keeps_its_slots_apart(be):
    g1 = kc.run_nest(be)
    assert live_handles() == 0
    nfree = free_slots(be)
    g2 = kc.run_nest(be)
    assert live_handles() == 0 and free_slots(be) == nfree
    gp = kc.run_nest(plain(be))
    h = kc.check_nest(host("nest"))
    f = kc.check_nest(g1, rho_host=h["rho"])
    _log("nested", nmv=g1["nmv"], nmv_plain=gp["nmv"], inner=g1["inner"], inner_plain=gp["inner"], res=g1["res"], rho=f["rho"],
         rho_host=h["rho"], lam_err=f["lam_err"], slots=nfree)
    assert g1["unconverged"] == 0 and g1["res"] <= kc.NEST_TOL_OUTER
    for g in (g2, gp):
        assert np.array_equal(g["v"], g1["v"]) and g["lam"] == g1["lam"] and g["res"] == g1["res"]
    assert g2["nmv"] == g1["nmv"] and g2["inner"] == g1["inner"]
    assert g1["nmv"] - gp["nmv"] in (0, 1)
    assert nfree >= 2                                   # the outer handle was in flight while the inner solves ran


# ---- exponentiate / exponentiate_general -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(kc.EXPO) + list(kc.EXPO_GENERAL))
def test_exponentiate_against_the_dense_exponential(be, name):
    g = kc.run_expo(be, name)
    h = host("expo", name)
    eh = kc.check_expo(name, h)["err"]
    f = kc.check_expo(name, g, err_host=eh)
    _log("exponentiate " + name, nmv=g["nmv"], nmv_host=h["nmv"], err=f["err"], err_host=eh)
    if name.startswith("zero"):
        assert g["nmv"] == 0 and not g["y"].any()
    if name.startswith("cut"):
        assert g["nmv"] > 2 * kc.expo_case(name)["krylovdim"]


# ---- non-symmetric eigenproblems -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [96, 257])
def test_eigsolve_lm_real_on_a_perron_matrix(be, n):
    g = kc.run_perron(be, n)
    h = host("perron", n)
    rh = kc.check_perron(n, h)["r"]
    f = kc.check_perron(n, g, r_host=rh)
    _log(f"eigsolve_lm_real perron{n}", applied=g["applied"], applied_host=h["applied"], r_true=f["r"], r_host=rh, lam_err=f["lam_err"])


def test_arnoldi_eigvals_with_a_conjugate_pair(be):
    g = kc.run_arnoldi(be)
    h = host("arnoldi")
    eh = kc.check_arnoldi(h)["err"]
    f = kc.check_arnoldi(g, err_host=eh)
    _log("arnoldi_eigvals pair", applied=g["applied"], applied_host=h["applied"], err=f["err"].tolist(), err_host=eh.tolist())


def test_eigsolve_lm_planar_with_a_conjugate_pair(be):
    g = kc.run_planar(be)
    h = host("planar")
    rh = kc.check_planar(h)["r"]
    f = kc.check_planar(g, r_host=rh)
    _log("eigsolve_lm_planar pair", applied=g["applied"], applied_host=h["applied"], r_true=f["r"].tolist(), r_host=rh.tolist())


# ---- linsolve, complex -----------------------------------------------------------------------------------------------
def test_linsolve_complex_caps_its_cycles_at_32_vectors(be):
    c = kc.linsolve_case()
    rh = kc.solve_figures(c, host("linsolve")["x"])["r"]
    g = kc.run_linsolve(be)
    i = g["info"]
    f = kc.check_solve(c, g["x"], r_host=rh)
    _log("linsolve complex", numops=i.numops, numiter=i.numiter, normres=i.normres, r_true=f["r"], r_host=rh, err=f["err"])
    assert i.converged == 1 and i.normres <= c["tol"] and np.iscomplexobj(i.hessenberg)
    assert i.hessenberg.shape == (33, 32) and i.numiter >= 2              # krylovdim 50, n = 40: cycles of 32
    # the same device without the complex entry points: ComplexVec composes them from the real kernels and times_i
    g2 = kc.run_linsolve(kc.hide(be, "dotc", "axpby_c", "orth_step_c", "lincomb_c"))
    i2 = g2["info"]
    f2 = kc.check_solve(c, g2["x"], r_host=rh)
    _log("linsolve complex, composed", numops=i2.numops, numiter=i2.numiter, normres=i2.normres, r_true=f2["r"], err=f2["err"])
    assert i2.converged == 1 and i2.hessenberg.shape == (41, 40)


def test_linsolve_through_apply_axpby_of_a_prepared_operator(be):
    c = kc.hac_case()
    rh = kc.solve_figures(c, host("hac")["x"])["r"]
    g = kc.run_hac(be)
    i = g["info"]
    f = kc.check_solve(c, g["x"], r_host=rh)
    _log("linsolve apply_axpby", mode=g["mode"], numops=i.numops, normres=i.normres, r_true=f["r"], r_host=rh, err=f["err"])
    assert g["mode"] == 3 and i.converged == 1 and i.normres <= c["tol"]
