"""Writes tests/golden/ham_inf_env_calls.json: the ORDER of backend calls (method name + shapes of the tensor arguments) that
the level solver of the infinite Hamiltonian environments and the uniform drivers make, for the real stack
(environments.MPOHamInfEnv, InfiniteMPS) and the interleaved one (native_cplx.NativeMPOHamInfEnv, NativeInfiniteMPS).
tests/test_ham_inf_env_calls_cpu.py and tests/test_gpu_native_ham_inf.py import `record_host` / `record_device` from here and
hold the package to the recorded sequences: the two classes share one control flow, and a change to it (which level is
zeroed, when a cycle runs, which bond's fixed point regularises which site) shows as a changed sequence.

While a section is recorded krylov.gmres and krylov.linsolve are replaced by `two_images`: the operator is applied to x0,
then to that image, and the second image is returned -- the sequence cannot depend on rounding or on iteration counts.  The
environments a driver starts from are built with the real solvers before its section begins.

Cases: transverse-field Ising (W = 3) and a four-level Hamiltonian with a scalar and a dense diagonal level that are not the
identity (the plain branch of the solver); unit cells of 1 and 2 sites, D = 4 (6 after the bond change), d = 2.
Host sections run on the NumPy stand-in (composed route of the regulariser); the fused route has no stand-in and is recorded
on the device:
    python tests/golden/make_ham_inf_env_calls.py            host sections
    python tests/golden/make_ham_inf_env_calls.py --device   the device section (keeps the host sections of the file)"""
import contextlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mpskit_jl_amd as mk  # noqa: E402
from mpskit_jl_amd import algorithms as al, krylov, native_cplx as nc  # noqa: E402
from mpskit_jl_amd.backend import DTensor  # noqa: E402

PATH = os.path.join(HERE, "ham_inf_env_calls.json")
X = np.array([[0.0, 1.0], [1.0, 0.0]])
Z = np.diag([1.0, -1.0])
D, D_CHANGED, CELLS = 4, 6, (1, 2)
DEVICE_SECTION = "diag_n2/native_fused_construct"


def hamiltonians(be):
    """tfi: levels 0 and 2 are the identity, level 1 has no diagonal block.  diag: level 1 carries the scalar 0.5, level 2 the
    dense block 0.3 Z -- both take the plain branch, one through the scaled pass-through transfer, one through an MPO block."""
    diag = {(0, 0): 1, (0, 1): -Z, (1, 1): 0.5, (1, 3): Z, (0, 2): X, (2, 2): 0.3 * Z, (2, 3): X, (0, 3): -0.7 * X, (3, 3): 1}
    return {"tfi": mk.transverse_field_ising(1.0, 0.7, be=be), "diag": mk.MPOHamiltonian(diag, be=be)}


def _shapes(v):
    if isinstance(v, DTensor):
        return "x".join(map(str, v.shape))
    if isinstance(v, (list, tuple)) and any(isinstance(t, DTensor) for t in v):
        return "[" + ",".join(_shapes(t) for t in v if isinstance(t, DTensor)) + "]"
    return None


class Recorder:
    """a backend that logs `name(shape, ..., key=shape)` of every public method called on it, then forwards the call"""

    def __init__(self, inner):
        self.__dict__.update(inner=inner, log=[])

    def __getattr__(self, name):
        v = getattr(self.inner, name)              # AttributeError for a missing entry: hasattr(be, ...) keeps its meaning
        if name.startswith("_") or not callable(v) or isinstance(v, type):
            return v

        def call(*args, **kw):
            parts = [s for s in map(_shapes, args) if s is not None]
            parts += [f"{k}={s}" for k, s in sorted((k, _shapes(t)) for k, t in kw.items()) if s is not None]
            self.log.append(f"{name}({', '.join(parts)})")
            return v(*args, **kw)
        return call

    def __setattr__(self, name, value):
        setattr(self.inner, name, value)


def two_images(be, op, x0):
    return op(op(x0, be.empty(*x0.shape)), be.empty(*x0.shape))


def _gmres(be, matvec, b, x0, **kw):
    return two_images(be, matvec, x0)


def _linsolve(be, op, b, x0, **kw):
    return two_images(be, op, x0), krylov.ConvergenceInfo(1, 0.0, 1, 2, None)


@contextlib.contextmanager
def recording(rec, out, name):
    """record the calls made inside the block as section `name`, with the two linear solvers replaced"""
    saved = krylov.gmres, krylov.linsolve
    krylov.gmres, krylov.linsolve = _gmres, _linsolve
    rec.log.clear()
    try:
        yield
    finally:
        krylov.gmres, krylov.linsolve = saved
    out[name] = list(rec.log)


def record_host(inner):
    """every host section: {"<case>_n<cell>/<section>": [call, ...]}"""
    rec, out = Recorder(inner), {}
    for case, H in hamiltonians(rec).items():
        for n in CELLS:
            tag = f"{case}_n{n}/"
            psi = mk.InfiniteMPS.random(2, D, np.random.default_rng(10 + n), n=n, be=rec)
            big = mk.InfiniteMPS.random(2, D_CHANGED, np.random.default_rng(20 + n), n=n, be=rec)
            nat = nc.NativeInfiniteMPS.random(2, D, np.random.default_rng(30 + n), n=n, be=rec)
            nbig = nc.NativeInfiniteMPS.random(2, D_CHANGED, np.random.default_rng(40 + n), n=n, be=rec)
            with recording(rec, out, tag + "real_construct"):
                env = mk.MPOHamInfEnv(psi, H)
            with recording(rec, out, tag + "real_recalculate_changed_bonds"):
                env.recalculate(big)
            with recording(rec, out, tag + "native_composed_construct"):
                nenv = nc.NativeMPOHamInfEnv(nat, H, device=False)
            with recording(rec, out, tag + "native_composed_recalculate_changed_bonds"):
                nenv.recalculate(nbig)
            one = mk.VUMPS(tol=0.0, maxiter=1)
            env, nenv = mk.MPOHamInfEnv(psi, H), nc.NativeMPOHamInfEnv(nat, H, device=False)      # the real solvers
            with recording(rec, out, tag + "real_vumps_iteration"):
                al._vumps(psi, H, one, env)
            with recording(rec, out, tag + "native_vumps_iteration"):
                mk.find_groundstate(nat, H, one, nenv)
            env, nenv = mk.MPOHamInfEnv(psi, H), nc.NativeMPOHamInfEnv(nat, H, device=False)
            with recording(rec, out, tag + "real_timestep"):
                mk.timestep(psi, H, 0.0, -0.05j, mk.TDVP(), env)
            with recording(rec, out, tag + "native_timestep"):
                mk.timestep(nat, H, 0.0, 0.05, mk.TDVP(), nenv)
    return out


def record_device(inner):
    """the fused route of the regulariser: one construction at n = 2, D = 4 on a backend that has mpsk_regularize_axpby"""
    rec, out = Recorder(inner), {}
    H = hamiltonians(rec)["diag"]
    nat = nc.NativeInfiniteMPS.random(2, D, np.random.default_rng(32), n=2, be=rec)
    with recording(rec, out, DEVICE_SECTION):
        nc.NativeMPOHamInfEnv(nat, H, device=True)
    return out


def pack(sections):
    """{"calls": the distinct call strings, "sections": {name: indices into them}}"""
    calls = sorted({c for seq in sections.values() for c in seq})
    idx = {c: k for k, c in enumerate(calls)}
    return {"calls": calls, "sections": {name: [idx[c] for c in seq] for name, seq in sorted(sections.items())}}


def unpack(packed):
    return {name: [packed["calls"][k] for k in seq] for name, seq in packed["sections"].items()}


def load():
    with open(PATH) as f:
        return unpack(json.load(f))


def first_difference(got, want):
    """None when the sequences agree, else a line that names the first call that differs and the two before it"""
    for k, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return f"call {k}: {g} where {w} was recorded (after {want[max(0, k - 2):k]})"
    if len(got) != len(want):
        return f"{len(got)} calls where {len(want)} were recorded"
    return None


if __name__ == "__main__":
    sections = load() if os.path.exists(PATH) else {}
    if "--device" in sys.argv[1:]:
        be = mk.Backend(0)
        sections.update(record_device(be))
        be.close()
    else:
        from cpu_backend_ham_inf import CpuHamInfBackend
        device = {k: v for k, v in sections.items() if k == DEVICE_SECTION}
        sections = dict(record_host(CpuHamInfBackend()), **device)
    with open(PATH, "w") as f:
        json.dump(pack(sections), f, separators=(",", ":"))
        f.write("\n")
    for name, seq in sorted(sections.items()):
        print(f"{name}: {len(seq)} calls")
