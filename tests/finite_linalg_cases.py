"""Shared by test_finite_linalg_cpu.py and test_gpu_finite_linalg.py: the chains, the dense references and the tolerance
rule of the FiniteMPS linear algebra (linalg.py).

States are contracted to dense vectors with mpskit_oracle.mps_to_vector on downloaded tensors.  Tolerance: e0 is the relative
distance between the vector of each ADDEND as the backend holds it (its canonical tensors, downloaded) and the dense
contraction of the host tensors it was built from -- the error the existing gauge code makes at this L and D.  Every vector
comparison allows 8 max(e0, L (D1 + D2) 2^-53): 2x because the sum's bonds are twice as wide, 2x because two half sweeps meet
at the centre, 2x slack for CholeskyQR against Householder rounding.  Vector errors are taken relative to max(|v1|, |v2|),
scalar ones (dot) relative to |v1| |v2|."""
import numpy as np

import mpskit_jl_amd as mk
import mpskit_oracle as mo
from mpskit_jl_amd import linalg
from mpskit_jl_amd.native_cplx import NativeFiniteMPS

U = 2.0 ** -53
# (L, d, cap of addend 1, cap of addend 2)
CHAINS = [(6, 2, 4, 3), (5, 3, 5, 2)]
CHAIN_IDS = ["L6d2", "L5d3"]
KINDS = ["real", "embedded", "native"]


class _Sites:
    """what mps_to_vector reads: site tensors whose product is the state"""

    def __init__(self, sites):
        self.sites = sites

    def __len__(self):
        return len(self.sites)

    def AL(self, i):
        return self.sites[i]

    AC = AL


def dims(L, d, D):
    """bonds right of sites 0 .. L-1 of FiniteMPS.random: min(d^(i+1), D, d^(L-1-i))"""
    return [min(d ** (i + 1), D, d ** (L - 1 - i)) for i in range(L)]


def host_tensors(L, d, D, rng, cplx):
    ds = [1] + dims(L, d, D)
    out = []
    for i in range(L):
        a = rng.standard_normal((ds[i], d, ds[i + 1]))
        out.append(a + 1j * rng.standard_normal(a.shape) if cplx else a)
    return out


def build(be, kind, As):
    if kind == "native":
        return NativeFiniteMPS(As, be, normalize=True)
    return mk.FiniteMPS(As, normalize=True, be=be)


def vec(psi):
    """dense vector of a state from its downloaded tensors"""
    if isinstance(psi, NativeFiniteMPS):
        return mo.mps_to_vector(_Sites(psi.to_host()))
    L = len(psi)
    h = L // 2
    sites = [psi.AL(i) for i in range(h)] + [psi.AC(h)] + [psi.AR(i) for i in range(h + 1, L)]
    return mo.mps_to_vector(_Sites([psi.download(t) for t in sites]))


def host_vec(As):
    v = mo.mps_to_vector(_Sites(As))
    return v / np.linalg.norm(v)


def sum_bond_dims(L, d, D1, D2):
    """(bond_dims() of psi1 + psi2, shape of its centre matrix) by the reference's min(rows, cols) chain: a QRpos sweep over
    sites < L//2 (r_i = min(r_{i-1} d, s_i)), an LQpos sweep over the others (l_i = min(s_{i-1}, d l_{i+1})), s the bonds of
    the direct sum.  Site i reports the right bond of the tensor that is stored for it: AL(i) below L//2, AR(i) from there."""
    s = [a + b for a, b in zip(dims(L, d, D1), dims(L, d, D2))]
    half = L // 2
    r, cur = [], 1
    for i in range(half):
        cur = min(cur * d, s[i])
        r.append(cur)
    l = {L: 1}
    for i in range(L - 1, half - 1, -1):
        l[i] = min(s[i - 1], d * l[i + 1])
    return r + [l[i + 1] for i in range(half, L)], (r[half - 1], l[half])


class Case:
    """two addends of one chain on one backend, their dense vectors (computed once, never modified) and the tolerance"""

    def __init__(self, be, kind, chain, seed=0):
        self.be, self.kind, (self.L, self.d, self.D1, self.D2) = be, kind, chain
        rng = np.random.default_rng(1000 * seed + 17 * self.L + self.d)
        cplx = kind != "real"
        self.A1 = host_tensors(self.L, self.d, self.D1, rng, cplx)
        self.A2 = host_tensors(self.L, self.d, self.D2, rng, cplx)
        self.psi1, self.psi2 = build(be, kind, self.A1), build(be, kind, self.A2)
        self.v1, self.v2 = vec(self.psi1), vec(self.psi2)
        self.e0 = max(np.linalg.norm(self.v1 - host_vec(self.A1)), np.linalg.norm(self.v2 - host_vec(self.A2)))
        self.floor = self.L * (self.D1 + self.D2) * U
        self.tol = 8.0 * max(self.e0, self.floor)
        self.worst = 0.0                                   # largest observed error in units of tol

    def close_vec(self, got, ref, what):
        scale = max(np.linalg.norm(self.v1), np.linalg.norm(self.v2))
        err = np.linalg.norm(got - ref) / scale
        self.worst = max(self.worst, err / self.tol)
        print(f"{self.kind} L={self.L} d={self.d} {what}: err {err:.3e} tol {self.tol:.3e} (e0 {self.e0:.3e})")
        assert err <= self.tol, (what, err, self.tol)

    def close_scalar(self, got, ref, what, scale=None):
        scale = np.linalg.norm(self.v1) * np.linalg.norm(self.v2) if scale is None else scale
        err = abs(got - ref) / scale
        self.worst = max(self.worst, err / self.tol)
        print(f"{self.kind} L={self.L} d={self.d} {what}: err {err:.3e} tol {self.tol:.3e} (e0 {self.e0:.3e})")
        assert err <= self.tol, (what, err, self.tol)


# ---- the public-level checks, one function per property (the two test files call them per backend / route) ---------------

def check_sum_and_difference(c, fused=None):
    kw = {} if c.kind == "native" else {"fused": fused}
    c.close_vec(vec(linalg.add(c.psi1, c.psi2, **kw)), c.v1 + c.v2, "psi1 + psi2")
    c.close_vec(vec(linalg.sub(c.psi1, c.psi2, **kw)), c.v1 - c.v2, "psi1 - psi2")
    if fused is None:
        c.close_vec(vec(c.psi1 + c.psi2), c.v1 + c.v2, "operator +")
        c.close_vec(vec(c.psi2 - c.psi1), c.v2 - c.v1, "operator -")


def check_scalars(c):
    a = 0.75 - 0.5j if c.kind != "real" else -1.5
    c.close_vec(vec(a * c.psi1), a * c.v1, "a * psi")
    c.close_vec(vec(c.psi1 * a), a * c.v1, "psi * a")
    c.close_vec(vec(-c.psi2), -c.v2, "-psi")
    c.close_vec(vec(c.psi1), c.v1, "psi unchanged by a * psi")
    big = 3.0 * c.psi1
    c.close_scalar(big.norm(), 3.0 * np.linalg.norm(c.v1), "norm(3 psi)", scale=3.0)
    c.close_vec(vec(mk.normalize(big)), c.v1 / np.linalg.norm(c.v1), "normalize(3 psi)")
    c.close_scalar(big.norm(), 3.0 * np.linalg.norm(c.v1), "normalize left its argument alone", scale=3.0)
    assert big.normalize() is big
    c.close_vec(vec(big), c.v1 / np.linalg.norm(c.v1), "psi.normalize()")
    s = (2.0 * c.psi1) + (a * c.psi2)
    c.close_vec(vec(s) / 3.0, (2.0 * c.v1 + a * c.v2) / 3.0, "2 psi1 + a psi2")


def isometry_defects(c, s):
    """max |AL^dag AL - 1| over sites < L//2 and max |AR AR^dag - 1| over sites >= L//2 of a sum"""
    half = c.L // 2
    if c.kind == "native":
        hs = s.to_host()
        AL, AR = hs[:half], {i: hs[i] for i in range(half + 1, c.L)}
    else:
        AL = [s.download(s.AL(i)) for i in range(half)]
        AR = {i: s.download(s.AR(i)) for i in range(half, c.L)}
    dl = max(np.abs(np.einsum("asb,asc->bc", np.conj(a), a) - np.eye(a.shape[2])).max() for a in AL)
    dr = max(np.abs(np.einsum("asb,csb->ac", a, np.conj(a)) - np.eye(a.shape[0])).max() for a in AR.values())
    return dl, dr


def check_canonical_form(c, fused=None):
    kw = {} if c.kind == "native" else {"fused": fused}
    s = linalg.add(c.psi1, c.psi2, **kw)
    dl, dr = isometry_defects(c, s)
    print(f"{c.kind} L={c.L} d={c.d}: isometry defects {dl:.3e} {dr:.3e}")
    assert dl <= c.tol and dr <= c.tol
    want, (left, right) = sum_bond_dims(c.L, c.d, c.D1, c.D2)
    half = c.L // 2
    if c.kind == "native":
        got = [s.dims(i)[2] for i in range(c.L)]
        assert s.center == half and s.dims(half)[0] == left
    else:
        got = s.bond_dims()
        cshape = s.CLs[half].shape
        assert (cshape[0], cshape[1]) == ((2 * left, 2 * right) if s.cplx else (left, right))
    assert got == want, (got, want)
    if c.kind != "native":                               # the lazy views of the result work on every site and bond
        for i in range(c.L):
            assert s.AC(i).shape[1] == c.d
        for i in range(-1, c.L):
            assert s.CR(i) is not None
        c.close_vec(vec(s), c.v1 + c.v2, "sum after every AC / CR was visited")
        c.close_scalar(s.norm(), np.linalg.norm(c.v1 + c.v2), "norm of the sum", scale=1.0)


def check_overlap(c):
    ref = np.vdot(c.v1, c.v2)
    got = linalg.dot(c.psi1, c.psi2)
    assert isinstance(got, float if c.kind == "real" else complex)
    c.close_scalar(got, ref, "dot(psi1, psi2)")
    c.close_scalar(linalg.dot(c.psi2, c.psi1), np.conj(ref), "dot(psi2, psi1) = conj")
    c.close_scalar(mk.dot(c.psi1, c.psi2), ref, "mk.dot")
    c.close_scalar(c.psi1.dot(c.psi2), ref, "psi1.dot(psi2)")
    if c.kind != "real":
        a = 0.5 + 2.0j
        c.close_scalar(linalg.dot(a * c.psi1, c.psi2) / abs(a), np.conj(a) * ref / abs(a), "conjugate-linear in the first")
        c.close_scalar(linalg.dot(c.psi1, a * c.psi2) / abs(a), a * ref / abs(a), "linear in the second")


def check_norms(c):
    n1 = c.psi1.norm()
    c.close_scalar(linalg.dot(c.psi1, c.psi1), n1 ** 2, "dot(psi, psi) = norm^2", scale=n1 ** 2)
    z = c.psi1 - c.psi1
    c.close_scalar(z.norm(), 0.0, "(psi - psi).norm()", scale=n1)
    s = c.psi1 + c.psi2
    c.close_scalar(linalg.dot(s, s).real, np.linalg.norm(c.v1 + c.v2) ** 2, "dot(sum, sum)", scale=4.0)


def check_mixed_overlap(be, chain):
    """a real state next to an embedded one"""
    cr, ce = Case(be, "real", chain, seed=1), Case(be, "embedded", chain, seed=2)
    ref = np.vdot(cr.v1, ce.v2)
    tol = max(cr.tol, ce.tol)
    got = linalg.dot(cr.psi1, ce.psi2)
    assert isinstance(got, complex) and abs(got - ref) <= tol, (got, ref)
    assert abs(linalg.dot(ce.psi2, cr.psi1) - np.conj(ref)) <= tol
