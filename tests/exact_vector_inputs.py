"""Inputs on which the Krylov vector kernels are exact, the bounds for what is not, and a case runner for any backend.

Exact family.  Basis vectors hold entries in {-1, 0, 1} * 2^-a, the vector y holds integers in [-4, 4] (Gaussian
integers, and basis entries with both parts in {-1, 0, 1} * 2^-a, for the complex forms); coefficients and scalars are
dyadic.  With a = floor(log4 n) (4^a ~ n/2 .. n) every intermediate of two classical Gram-Schmidt rounds is a dyadic
rational that fp64 holds exactly:

    h1 = X^T y          multiples of 2^-a       y1 = y - X h1       multiples of 2^-2a
    h2 = X^T y1         multiples of 2^-3a      y2 = y1 - X h2      multiples of 2^-4a       h1 + h2: multiples of 2^-3a

so ANY correct kernel -- whatever its grid, its chunking of the basis, its reduction order, fused or not, with or
without FMA -- returns the same bits, and the comparison is np.array_equal.  The Gram matrix of such a basis is about
(2/3) n 4^-a I, not I, so h2 is as large as h1 and the second round carries weight.  The reference is computed in
int64 arithmetic on the numerators (Python ints for the squared norm).  The condition is checked, not assumed: every
stage records the largest sum of absolute values any partial sum of it can reach, in units of its own quantum and taken
from the actual data (|X| <= 2^-a elementwise, so sum |y| bounds every dot's abs-sum), and `guard` of every record must
stay below 2^50 (`LIMIT`).

The squared norm of the remainder is NOT exact (its terms are multiples of 2^-8a).  All its terms are positive, so a
summation tree of depth `depth` errs by at most depth * u relative, plus one rounding for each product: it is held to
(depth + 2) u sum y2^2 around the exact rational sum, and needs no margin.  `depth(n, long)` counts the additions on the
longest path of the kernels of mpsk_ops.hip: a thread makes T = ceil(pairs / (256 grid)) trips of two elements (the long
kernels: T = ceil(n / (256 grid)) trips of one), thread 0 may add the odd tail, a wavefront adds 6 levels, the four
wavefronts 3 more; dot_final_kernel then adds ceil(grid / 256) partials per thread and the same 6 + 3 levels.
beta = sqrt(n2) and the normalised vector y2 / beta are held to half that bound (the square root halves a relative
error) plus three roundings (sqrt, reciprocal, multiply): ((depth + 2) / 2 + 3) u, plus 2^-63 for the longdouble
division that forms the reference.

Gaussian family.  Integers this small survive an fp32 path, so every kernel group gets a Gaussian case against
np.longdouble.  A dot is held to gamma_n |x|.|y| (Higham, Accuracy and Stability, 2nd ed., section 3.1), any order,
with or without FMA; gamma_m is taken as (m + 2) u here.  The CGS2 outputs nest.  Write A = |X|, ^ for computed values
and E_v for a bound on |v^ - v|, v the value of exact arithmetic on the same inputs.  Then, componentwise,

    E_h1 = gamma_n A^T |y|
    E_y1 = A E_h1 + gamma_{k+1} (|y| + A (|h1| + E_h1))                (the axpy sums k + 1 terms per element)
    E_h2 = A^T E_y1 + gamma_n A^T (|y1| + E_y1)
    E_y2 = E_y1 + A E_h2 + gamma_{k+1} (|y1| + E_y1 + A (|h2| + E_h2))
    E_n2 = sum (2 |y2| E_y2 + E_y2^2) + gamma_{n+1} sum (|y2| + E_y2)^2
    E_h  = E_h1 + E_h2 + u (|h1 + h2| + E_h1 + E_h2)                   (the host adds the two rounds)
    E_beta = E_n2 / (2 beta) * (1 + E_n2 / n2) + 2 u beta,   E_yn = E_y2 / beta + |y2| / beta (E_beta / beta + 3 u)

each line the standard forward bound of its operation applied to perturbed inputs.  Complex forms: a complex product
is four real products and two additions, a length-n complex dot a real one of length 2n per component; the moduli obey
the same lines with gamma_m replaced by 4 (m + 4) u (tests/exact_inputs.py derives that constant), and A = |X| the
moduli.  tests/test_exact_vector_inputs_cpu.py checks every guard, numpy fp64 == exact reference on the exact cases and
numpy fp64 inside the bounds on the Gaussian ones, and runs the case runner below on the host stand-in backend.
"""
from __future__ import annotations

import functools
import math
import zlib
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
LIMIT = 2 ** 50
LD = np.longdouble
CLD = np.clongdouble
KMAX = 34                       # 32 (fused / long kernels) + 2 on the separate-pass fallback of vec_cgs2
ALPHA, BETA = 0.5, -2.0
ALPHA_C, BETA_C = 0.5 - 0.25j, -2.0 + 0.5j

# grid constants of mpskit.jl_amd/csrc/mpsk_ops.hip
THREADS, DOT_BLOCKS, EW_BLOCKS, MD, ML = 256, 1024, 4096, 8, 32
D2_TRIP = 2 * THREADS * DOT_BLOCKS          # doubles per grid-stride trip of the d2 reductions
LONG_TRIP = THREADS * DOT_BLOCKS            # ... of the long CGS2 kernels (9 <= k <= 32)
EW_TRIP = THREADS * EW_BLOCKS               # elements per trip of the capped elementwise kernels
EW_D2_TRIP = 2 * THREADS * EW_BLOCKS        # doubles per trip of the capped d2 elementwise kernels

SMALL = [1, 2, 3, 255, 257, 511, 513]
D2_SIZES = SMALL + [D2_TRIP - 1, D2_TRIP, D2_TRIP + 1, 3 * LONG_TRIP + 3]
LONG_SIZES = SMALL + [LONG_TRIP - 1, LONG_TRIP + 1, 3 * LONG_TRIP + 3]
ORTH_SIZES = [5, 4099, LONG_TRIP + 1, 3 * LONG_TRIP + 3]
ORTH_C_SIZES = [1, 63, 4097, D2_TRIP // 2 + 1]
EW_SIZE = EW_TRIP + 257
EW_D2_SIZE = EW_D2_TRIP + 3


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def exponent(n):
    """a = floor(log4 n), at least 1"""
    return max(1, (int(n).bit_length() - 1) // 2)


def depth(n, long=False):
    """additions on the longest path of a reduction over n doubles (module docstring)"""
    if long:
        grid = min(max((n + THREADS - 1) // THREADS, 1), DOT_BLOCKS)
        per_thread = -(-n // (THREADS * grid))
    else:
        grid = min(max((n // 2 + THREADS - 1) // THREADS, 1), DOT_BLOCKS)
        per_thread = 2 * max(-(-(n // 2) // (THREADS * grid)), 1) + 1
    return per_thread + 9 + -(-grid // THREADS) + 9


def n2_factor(n, long=False):
    return (depth(n, long) + 2) * U


def beta_factor(n, long=False):
    return ((depth(n, long) + 2) / 2 + 3) * U + 2.0 ** -63


# ----------------------------------------------------------------------------------------------------------------------
# exact family
# ----------------------------------------------------------------------------------------------------------------------
class Family:
    """kmax basis vectors and one y of length n (complex: n complex elements); built once per (n, cplx) and read-only"""

    def __init__(self, n, cplx=False, kmax=KMAX):
        self.n, self.cplx, self.kmax, self.a = int(n), bool(cplx), int(kmax), exponent(n)
        rng = _rng(f"vector-family-{n}-{int(cplx)}-{kmax}")
        self.Xr = rng.integers(-1, 2, size=(kmax, n)).astype(np.int64)
        self.yr = rng.integers(-4, 5, size=n).astype(np.int64)
        self.zr = rng.integers(-4, 5, size=n).astype(np.int64)             # a second integer vector (axpby, diff_nrm2)
        if cplx:
            self.Xi = rng.integers(-1, 2, size=(kmax, n)).astype(np.int64)
            self.yi = rng.integers(-4, 5, size=n).astype(np.int64)
            self.zi = rng.integers(-4, 5, size=n).astype(np.int64)
        for v in vars(self).values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)

    @property
    def q(self):
        return 2.0 ** -self.a

    def x(self, j):
        """basis vector j as fp64 (complex128)"""
        if self.cplx:
            return (self.Xr[j] + 1j * self.Xi[j]) * self.q
        return self.Xr[j] * self.q

    def y(self):
        return (self.yr + 1j * self.yi) if self.cplx else self.yr.astype(np.float64)

    def z(self):
        return (self.zr + 1j * self.zi) if self.cplx else self.zr.astype(np.float64)


@functools.lru_cache(maxsize=2)
def family(n, cplx=False, kmax=KMAX):
    return Family(n, cplx, kmax)


def _f(num, e):
    """numerator array (int64 or Python ints) * 2^-e as fp64; exact because every |numerator| < 2^53 (guarded)"""
    return np.ldexp(np.asarray(num, dtype=np.float64), -e)


def _fc(re, im, e):
    return _f(re, e) + 1j * _f(im, e)


def _sumsq(v):
    """sum of squares of an int64 array with |v| < 2^50 as a Python int (three int64 sums of 25-bit halves)"""
    hi, lo = v >> 25, v & ((1 << 25) - 1)
    out = 0
    for s in range(0, v.size, 1 << 10):                                    # 2^10 terms below 2^52 each
        h, l_ = hi[s:s + (1 << 10)], lo[s:s + (1 << 10)]
        out += (int(np.sum(h * h)) << 50) + (int(np.sum(h * l_)) << 26) + int(np.sum(l_ * l_))
    return out


def exact_dots(fam, k):
    """(<xs[j], y>, j < k, as fp64 -- complex for the complex family: conj(xs[j]) . y --, guard)"""
    X, y = fam.Xr[:k], fam.yr
    if not fam.cplx:
        return _f(X @ y, fam.a), int(np.abs(y).sum())
    Xi, yi = fam.Xi[:k], fam.yi
    return _fc(X @ y + Xi @ yi, X @ yi - Xi @ y, fam.a), int(2 * (np.abs(y).sum() + np.abs(yi).sum()))


def cgs2_sweep(fam, ks, second=True):
    """Yields, for each k of the ascending list ks, the exact record of two classical Gram-Schmidt rounds of y against
    xs[:k]: dict(k, h1, h2, h (= h1 + h2), y1, y2 (fp64 / complex128, all exact), N2 (Python int) and e2 with
    |y2|^2 = N2 2^-e2, guard).  second=False stops after y1 (one round: mpsk_vgs_step).  The first-round state is
    carried from k to k + 1, so a sweep costs one pass per k and round."""
    a, n, c = fam.a, fam.n, fam.cplx
    s = 1 << (2 * a)                                                         # 4^a: one quantum step of a round
    Xr, yr = fam.Xr, fam.yr
    Xi, yi = (fam.Xi, fam.yi) if c else (None, None)
    g1r = Xr @ yr + (Xi @ yi if c else 0)                                    # h1 numerators (2^-a), all kmax at once
    g1i = (Xr @ yi - Xi @ yr) if c else None
    guard = int(np.abs(yr).sum() + (np.abs(yi).sum() if c else 0)) * (2 if c else 1)
    y1r, y1i = yr * s, (yi * s if c else None)                               # y1 numerators (2^-2a)
    done, acc1 = 0, 0                                                        # acc1: sum_j |h1_j| (|X| <= 1 quantum)
    for k in ks:
        for j in range(done, k):                                             # y1 -= xs[j] h1[j]
            if c:
                y1r = y1r - (Xr[j] * g1r[j] - Xi[j] * g1i[j])
                y1i = y1i - (Xr[j] * g1i[j] + Xi[j] * g1r[j])
                acc1 += 2 * (abs(int(g1r[j])) + abs(int(g1i[j])))
            else:
                y1r = y1r - Xr[j] * g1r[j]
                acc1 += abs(int(g1r[j]))
        done = k
        gd = max(guard, 4 * s * (2 if c else 1) + acc1)                      # elementwise abs-sum of the first axpy
        rec = {"k": k, "h1": _fc(g1r[:k], g1i[:k], a) if c else _f(g1r[:k], a),
               "y1": _fc(y1r, y1i, 2 * a) if c else _f(y1r, 2 * a)}
        if second:
            g2r = Xr[:k] @ y1r + (Xi[:k] @ y1i if c else 0)                  # h2 numerators (2^-3a)
            g2i = (Xr[:k] @ y1i - Xi[:k] @ y1r) if c else None
            gd = max(gd, int(np.abs(y1r).sum() + (np.abs(y1i).sum() if c else 0)) * (2 if c else 1))
            if c:
                y2r = y1r * s - (g2r @ Xr[:k] - g2i @ Xi[:k])                # y2 numerators (2^-4a)
                y2i = y1i * s - (g2i @ Xr[:k] + g2r @ Xi[:k])
                acc2 = 2 * int(np.abs(g2r).sum() + np.abs(g2i).sum())
                gd = max(gd, int(max(np.abs(y1r).max(), np.abs(y1i).max())) * 2 * s + acc2)
                hr, hi = g1r[:k] * s + g2r, g1i[:k] * s + g2i
                gd = max(gd, int(np.abs(hr).max()), int(np.abs(hi).max()))
                N2 = _sumsq(y2r) + _sumsq(y2i)
                rec.update(h2=_fc(g2r, g2i, 3 * a), h=_fc(hr, hi, 3 * a), y2=_fc(y2r, y2i, 4 * a))
            else:
                y2r = y1r * s - g2r @ Xr[:k]
                gd = max(gd, int(np.abs(y1r).max()) * s + int(np.abs(g2r).sum()))
                hr = g1r[:k] * s + g2r
                gd = max(gd, int(np.abs(hr).max()))
                N2 = _sumsq(y2r)
                rec.update(h2=_f(g2r, 3 * a), h=_f(hr, 3 * a), y2=_f(y2r, 4 * a))
            rec.update(N2=N2, e2=8 * a)
        rec["guard"] = gd
        yield rec


def n2_fraction(rec):
    return Fraction(rec["N2"], 1 << rec["e2"])


def beta_ld(rec):
    """sqrt(|y2|^2) as longdouble, relative error below 2^-63 (integer square root of the numerator scaled by 2^128)"""
    r = math.isqrt(rec["N2"] << 128)
    sh = max(r.bit_length() - 64, 0)
    r >>= sh
    return np.ldexp(LD(r >> 32) * LD(2.0 ** 32) + LD(r & 0xFFFFFFFF), sh - 64 - rec["e2"] // 2)


def lincomb_coefs(k, cplx=False):
    """dyadic coefficients in [-2, 2] with step 1/4, none zero"""
    rng = _rng(f"lincomb-{k}-{int(cplx)}")
    c = rng.choice(np.array([-8, -5, -3, -2, -1, 1, 2, 3, 6, 7]), size=k) / 4.0
    if cplx:
        c = c + 1j * rng.choice(np.array([-8, -5, -3, -2, -1, 1, 2, 3, 6, 7]), size=k) / 4.0
    return c


def exact_lincomb(fam, coefs):
    """(sum_j coefs[j] xs[j] exactly, guard): numerators in units of 2^-(a + 2)"""
    k = len(coefs)
    cr = np.round(4 * np.real(coefs)).astype(np.int64)
    guard = int(np.abs(cr).sum())
    if not fam.cplx:
        return _f(cr @ fam.Xr[:k], fam.a + 2), guard
    ci = np.round(4 * np.imag(coefs)).astype(np.int64)
    return (_fc(cr @ fam.Xr[:k] - ci @ fam.Xi[:k], cr @ fam.Xi[:k] + ci @ fam.Xr[:k], fam.a + 2),
            2 * (guard + int(np.abs(ci).sum())))


# ----------------------------------------------------------------------------------------------------------------------
# Gaussian family
# ----------------------------------------------------------------------------------------------------------------------
def _gam(m, cplx):
    return 4 * (m + 4) * U if cplx else (m + 2) * U


@functools.lru_cache(maxsize=2)
def gauss_case(n, k, cplx=False):
    """Gaussian basis (columns of norm ~1), y, and the longdouble reference of two CGS2 rounds with the nested bounds of
    the module docstring: dict(X, y, h1, h2, h, y1, y2, n2, beta, yn and E_* for each, dot_bound)."""
    rng = _rng(f"vector-gauss-{n}-{k}-{int(cplx)}")
    X = rng.standard_normal((k, n)) / np.sqrt(n)
    y = rng.standard_normal(n)
    if cplx:
        X = X + 1j * rng.standard_normal((k, n)) / np.sqrt(n)
        y = y + 1j * rng.standard_normal(n)
    hp = CLD if cplx else LD
    Xh, yh = X.astype(hp), y.astype(hp)
    A, ay = np.abs(Xh), np.abs(yh)
    gn, gk, gn1 = _gam(n, cplx), _gam(k + 1, cplx), _gam(n + 1, cplx)
    h1 = Xh.conj() @ yh
    y1 = yh - h1 @ Xh
    h2 = Xh.conj() @ y1
    y2 = y1 - h2 @ Xh
    n2 = (np.abs(y2) ** 2).sum()
    beta = np.sqrt(n2)
    E_h1 = gn * (A @ ay)
    E_y1 = E_h1 @ A + gk * (ay + (np.abs(h1) + E_h1) @ A)
    E_h2 = A @ E_y1 + gn * (A @ (np.abs(y1) + E_y1))
    E_y2 = E_y1 + E_h2 @ A + gk * (np.abs(y1) + E_y1 + (np.abs(h2) + E_h2) @ A)
    E_n2 = (2 * np.abs(y2) * E_y2 + E_y2 ** 2).sum() + gn1 * ((np.abs(y2) + E_y2) ** 2).sum()
    E_h = E_h1 + E_h2 + U * (np.abs(h1 + h2) + E_h1 + E_h2)
    E_beta = E_n2 / (2 * beta) * (1 + E_n2 / n2) + 2 * U * beta
    E_yn = E_y2 / beta + np.abs(y2) / beta * (E_beta / beta + 3 * U)
    t = dict(n=n, k=k, cplx=cplx, X=X, y=y, h1=h1, h2=h2, h=h1 + h2, y1=y1, y2=y2, n2=n2, beta=beta, yn=y2 / beta,
             E_h1=E_h1, E_h2=E_h2, E_h=E_h, E_y1=E_y1, E_y2=E_y2, E_n2=E_n2, E_beta=E_beta, E_yn=E_yn)
    for v in t.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return t


def numpy_cgs2(X, y):
    """the same two rounds in plain numpy fp64 / complex128 (what the CPU self-check holds to the bounds)"""
    h1 = X.conj() @ y
    y1 = y - h1 @ X
    h2 = X.conj() @ y1
    y2 = y1 - h2 @ X
    n2 = float((np.abs(y2) ** 2).sum())
    beta = np.sqrt(n2)
    return dict(h1=h1, h2=h2, h=h1 + h2, y1=y1, y2=y2, n2=n2, beta=beta, yn=y2 * (1.0 / beta))


def within(got, ref, bound, what, out):
    """appends a mismatch record to `out` unless |got - ref| <= bound everywhere (longdouble difference) and got is finite"""
    got = np.asarray(got)
    hp = CLD if np.iscomplexobj(got) or np.iscomplexobj(ref) else LD
    err = np.abs(got.astype(hp) - np.asarray(ref, dtype=hp))
    bound = np.broadcast_to(np.asarray(bound, dtype=LD), err.shape)
    bad = ~(err <= bound)
    ratio = np.where(err > 0, err / np.maximum(bound, np.finfo(LD).tiny), 0)
    if bad.any():
        i = int(np.argmax(np.where(bad, ratio, -1)))
        out.append(f"{what}: {int(bad.sum())} of {err.size} outside the bound; worst at {i}: err {float(err.flat[i]):.3e} "
                   f"bound {float(bound.flat[i]):.3e}")
    return float(np.nanmax(ratio, initial=0.0))


def same(got, ref, what, out):
    got, ref = np.asarray(got), np.asarray(ref)
    if got.shape != ref.shape or not np.array_equal(got, ref):
        d = np.flatnonzero(np.ravel(got) != np.ravel(ref)) if got.shape == ref.shape else []
        i = int(d[0]) if len(d) else -1
        out.append(f"{what}: {len(d)} of {ref.size} entries differ"
                   + (f"; first at {i}: got {np.ravel(got)[i]!r} expected {np.ravel(ref)[i]!r}" if i >= 0 else " (shape)"))


def close_exact(got, ref: Fraction, factor, what, out):
    """|got - ref| <= factor * ref in exact rational arithmetic (ref > 0, or got == ref == 0)"""
    if not np.isfinite(got) or abs(Fraction(float(got)) - ref) > Fraction(float(factor)) * ref:
        out.append(f"{what}: got {float(got)!r}, exact {float(ref)!r}, allowed relative {factor:.3e}")


# ----------------------------------------------------------------------------------------------------------------------
# case runner: any backend with the vector protocol of mpskit.jl_amd.backend.Backend (methods it lacks are skipped)
# ----------------------------------------------------------------------------------------------------------------------
class Device:
    """the family's vectors on a backend, uploaded once: xs[0..kmax), y, z"""

    def __init__(self, be, fam, kmax=None):
        self.be, self.fam = be, fam
        kmax = fam.kmax if kmax is None else kmax
        self.up = be.upload_c if fam.cplx else be.upload
        self.down = be.download_c if fam.cplx else be.download
        self.xs = [self.up(fam.x(j)) for j in range(kmax)]
        self.y, self.z = self.up(fam.y()), self.up(fam.z())

    def fresh_y(self):
        return self.be.copy(self.y)

    def nan(self):
        n = self.fam.n
        return self.up(np.full(n, np.nan + (1j * np.nan if self.fam.cplx else 0)))


def run_dots(dev, ks, out=None):
    """mpsk_vdot / vnrm2 / vmultidot (real) or mpsk_vdotc (complex, k = 1) on the exact family"""
    out = [] if out is None else out
    be, fam = dev.be, dev.fam
    tag = f"n={fam.n}"
    if fam.cplx:
        ref, _ = exact_dots(fam, 1)
        same(np.complex128(be.dotc(dev.xs[0], dev.y)), ref[0], f"dotc {tag}", out)
        return out
    ref, _ = exact_dots(fam, max(ks))
    same(be.dot(dev.xs[0], dev.y), ref[0], f"dot {tag}", out)
    same(be.norm(dev.y), np.sqrt(float(int((fam.yr * fam.yr).sum()))), f"nrm2 {tag}", out)
    for k in ks:
        same(be.multidot(dev.xs[:k], dev.y), ref[:k], f"multidot {tag} k={k}", out)
    return out


def run_gs_lincomb(dev, ks, out=None):
    """mpsk_vgs_step, mpsk_vlincomb and mpsk_vlincomb_dev (complex: mpsk_vlincomb_c) on the exact family"""
    out = [] if out is None else out
    be, fam = dev.be, dev.fam
    tag = f"n={fam.n}"
    if not fam.cplx:
        for rec in cgs2_sweep(fam, list(ks), second=False):
            k = rec["k"]
            y = dev.fresh_y()
            same(be.gs_step(dev.xs[:k], y), rec["h1"], f"gs_step h {tag} k={k}", out)
            same(dev.down(y), rec["y1"], f"gs_step y {tag} k={k}", out)
    for k in ks:
        cf = lincomb_coefs(k, fam.cplx)
        ref, _ = exact_lincomb(fam, cf)
        if fam.cplx:
            same(dev.down(be.lincomb_c(dev.xs[:k], cf, out=dev.nan())), ref, f"lincomb_c {tag} k={k}", out)
            continue
        same(dev.down(be.lincomb(dev.xs[:k], cf, out=dev.nan())), ref, f"lincomb {tag} k={k}", out)
        if hasattr(be, "lincomb_dev"):
            same(dev.down(be.lincomb_dev(dev.xs[:k], be.upload(cf), out=dev.nan())), ref, f"lincomb_dev {tag} k={k}", out)
    return out


def run_orth(dev, ks, slot_offset=3, out=None, ratios=None):
    """mpsk_vorth_step and mpsk_vorth_step_dev (complex: mpsk_vorth_step_c) for every k of ks on the exact family:
    coefficients bit for bit, |remainder|^2, beta and the normalised vector inside the derived bounds"""
    out = [] if out is None else out
    be, fam = dev.be, dev.fam
    nd = 2 * fam.n if fam.cplx else fam.n
    for rec in cgs2_sweep(fam, list(ks)):
        k = rec["k"]
        tag = f"n={fam.n} k={k}"
        long = (not fam.cplx) and MD < k <= ML
        fn2, fb = n2_factor(nd, long), beta_factor(nd, long)
        b_ref = beta_ld(rec)
        yn_ref = rec["y2"].astype(CLD if fam.cplx else LD) / b_ref if rec["N2"] else rec["y2"]
        y = dev.fresh_y()
        h, beta = (be.orth_step_c if fam.cplx else be.orth_step)(dev.xs[:k], y)
        same(h, rec["h"], f"orth_step h {tag}", out)
        r = within(beta, b_ref, fb * b_ref, f"orth_step beta {tag}", out)
        r = max(r, within(dev.down(y), yn_ref, fb * np.abs(yn_ref), f"orth_step y {tag}", out))
        if ratios is not None:
            ratios.append(r)
        if fam.cplx or not hasattr(be, "orth_step_dev"):
            continue
        slot = be.upload(np.full(slot_offset + 2 * k + 1 + 2, -7.0))
        y = dev.fresh_y()
        be.orth_step_dev(dev.xs[:k], y, slot, slot_offset)
        s = be.download(slot)
        same(s[:slot_offset], np.full(slot_offset, -7.0), f"orth_step_dev slot head {tag}", out)
        same(s[slot_offset + 2 * k + 1:], np.full(2, -7.0), f"orth_step_dev slot tail {tag}", out)
        same(s[slot_offset:slot_offset + k], rec["h1"], f"orth_step_dev h1 {tag}", out)
        same(s[slot_offset + k:slot_offset + 2 * k], rec["h2"], f"orth_step_dev h2 {tag}", out)
        close_exact(s[slot_offset + 2 * k], n2_fraction(rec), fn2, f"orth_step_dev n2 {tag}", out)
        within(dev.down(y), yn_ref, fb * np.abs(yn_ref), f"orth_step_dev y {tag}", out)
    return out


def run_elementwise(dev, out=None):
    """axpby (beta != 0, beta == 0 on NaN), scal, times_i, diff_nrm2, normalize_dev / nrm2_dev on the exact family"""
    out = [] if out is None else out
    be, fam = dev.be, dev.fam
    n, tag = fam.n, f"n={fam.n}"
    x0, yv, zv = fam.x(0), fam.y(), fam.z()
    if fam.cplx:
        same(dev.down(be.axpby_c(ALPHA_C, dev.xs[0], BETA_C, dev.fresh_y())), ALPHA_C * x0 + BETA_C * yv, f"axpby_c {tag}", out)
        same(dev.down(be.axpby_c(ALPHA_C, dev.xs[0], 0.0, dev.nan())), ALPHA_C * x0, f"axpby_c beta=0 {tag}", out)
        return out
    same(dev.down(be.axpby(ALPHA, dev.xs[0], BETA, dev.fresh_y())), ALPHA * x0 + BETA * yv, f"axpby {tag}", out)
    same(dev.down(be.axpby(ALPHA, dev.xs[0], 0.0, dev.nan())), ALPHA * x0, f"axpby beta=0 {tag}", out)
    same(dev.down(be.scal(-0.75, dev.fresh_y())), -0.75 * yv, f"scal {tag}", out)
    if n % 2 == 0:
        p = yv.reshape(-1, 2)
        same(dev.down(be.times_i(dev.y, out=dev.nan())), np.stack([-p[:, 1], p[:, 0]], axis=1).reshape(-1), f"times_i {tag}", out)
    if hasattr(be, "vdiff_nrm2"):
        ref = [float(int(((fam.yr - fam.zr) ** 2).sum())), float(int((fam.yr ** 2).sum()))]
        same(np.array(be.vdiff_nrm2(dev.y, dev.z)), np.array(ref), f"diff_nrm2 f64 {tag}", out)
        if n % 2 == 0 and hasattr(be, "_set_dtype") and hasattr(be, "lib"):
            be._set_dtype(True)
            try:
                got = np.array(_diff_c128(be, dev))
            finally:
                be._set_dtype(False)
            same(got, np.array(ref), f"diff_nrm2 c128 {tag}", out)
    # normalisation: |y|^2 is an exact integer; the scaling is held to beta_factor (sqrt, reciprocal, multiply)
    N2 = int((fam.yr ** 2).sum())
    rec = {"N2": N2, "e2": 0}
    fb = beta_factor(n)
    yn_ref = yv.astype(LD) / beta_ld(rec) if N2 else yv
    slot = be.upload(np.full(4, -7.0))
    be.nrm2_dev(dev.y, slot, 1)
    same(be.download(slot), np.array([-7.0, float(N2), -7.0, -7.0]), f"nrm2_dev {tag}", out)
    for inplace in (True, False):
        for with_slot in (True, False):
            x = dev.fresh_y()
            o = None if inplace else dev.nan()
            slot = be.upload(np.full(4, -7.0))
            r = be.normalize_dev(x, out=o, slot=slot if with_slot else None, offset=2)
            what = f"normalize_dev {'in place' if inplace else 'out of place'}{' +n2' if with_slot else ''} {tag}"
            within(dev.down(r), yn_ref, fb * np.abs(yn_ref), what, out)
            if not inplace:
                same(dev.down(x), yv, what + " (input kept)", out)
            same(be.download(slot), np.array([-7.0, -7.0, float(N2) if with_slot else -7.0, -7.0]), what + " slot", out)
    zero = be.upload(np.zeros(n))
    for o in (None, dev.nan()):
        same(dev.down(be.normalize_dev(zero, out=o)), np.zeros(n), f"normalize_dev of the zero vector {tag}", out)
    return out


def _diff_c128(be, dev):
    import ctypes as C
    res = (C.c_double * 2)()
    rc = be.lib.mpsk_vdiff_nrm2(be.ctx, dev.fam.n // 2, dev.y.ptr, dev.z.ptr, res)
    assert rc == 0, rc
    return [res[0], res[1]]


def multilincomb_coefs(k, m):
    rng = _rng(f"multilincomb-{k}-{m}")
    return rng.choice(np.array([-8, -5, -3, -2, -1, 0, 1, 2, 3, 6, 7]), size=(k, m)) / 4.0


def run_multilincomb(dev, k, m, out=None):
    out = [] if out is None else out
    be, fam = dev.be, dev.fam
    S = multilincomb_coefs(k, m)
    outs = [dev.nan() for _ in range(m)]
    be.multilincomb(dev.xs[:k], S, outs)
    for j in range(m):
        ref, _ = exact_lincomb(fam, S[:, j])
        same(dev.down(outs[j]), ref, f"multilincomb n={fam.n} k={k} m={m} output {j}", out)
    return out


def run_gauss(be, n, k, cplx=False, out=None, ratios=None):
    """one Gaussian case: dots, orth_step (and orth_step_dev) inside the nested bounds, every reducing call twice with
    identical bits"""
    out = [] if out is None else out
    t = gauss_case(n, k, cplx)
    tag = f"gauss n={n} k={k}{' c128' if cplx else ''}"
    up, down = (be.upload_c, be.download_c) if cplx else (be.upload, be.download)
    xs, y0 = [up(x) for x in t["X"]], up(t["y"])
    res = []
    for rep in range(2):
        y = be.copy(y0)
        if cplx:
            d = np.complex128(be.dotc(xs[0], y0))
            h, beta = be.orth_step_c(xs, y)
            res.append((d, h, beta, down(y)))
        else:
            d = be.multidot(xs, y0)
            h, beta = be.orth_step(xs, y)
            res.append((d, h, beta, down(y)))
    for a_, b_, nm in zip(res[0], res[1], ("dots", "h", "beta", "y")):
        same(b_, a_, f"{tag}: second run, {nm}", out)
    d, h, beta, yn = res[0]
    r = [within(d, t["h1"][0] if cplx else t["h1"], t["E_h1"][0] if cplx else t["E_h1"], f"{tag} dots", out),
         within(h, t["h"], t["E_h"], f"{tag} orth_step h", out),
         within(beta, t["beta"], t["E_beta"], f"{tag} orth_step beta", out),
         within(yn, t["yn"], t["E_yn"], f"{tag} orth_step y", out)]
    if not cplx and hasattr(be, "orth_step_dev"):
        slot = be.upload(np.zeros(2 * k + 1))
        y = be.copy(y0)
        be.orth_step_dev(xs, y, slot, 0)
        s = be.download(slot)
        r += [within(s[:k], t["h1"], t["E_h1"], f"{tag} orth_step_dev h1", out),
              within(s[k:2 * k], t["h2"], t["E_h2"], f"{tag} orth_step_dev h2", out),
              within(s[2 * k], t["n2"], t["E_n2"], f"{tag} orth_step_dev n2", out)]
        same(down(y), yn, f"{tag}: orth_step_dev y against orth_step y", out)
    if ratios is not None:
        ratios.append(max(r))
    return out


# ----------------------------------------------------------------------------------------------------------------------
# Ritz step (ritz_small_kernel through mpsk_vritz_dev): synthesised slots, mpmath reference, error ratios
# ----------------------------------------------------------------------------------------------------------------------
# numpy eigh's own worst error ratio against mpmath over every case of ritz_cases() (value and residual in units of
# u |A|_F, vector in u |A|_F / gap): 3.594 at m = 20 -- profiles/vector_kernel_bounds.log.  The kernel is allowed 8 times
# that, the rule of the factor-path tests: its Newton-refined rcp / rsq seeds are not correctly rounded.
NUMPY_WORST = 3.594
RITZ_BOUND = 8 * NUMPY_WORST
RITZ_N = 48                     # dimension of the dense symmetric matrix behind the Arnoldi slots (> 32 steps)


def arnoldi_slots(m, stride, scale=1.0, seed="ritz"):
    """The slot mpsk_vorth_step_dev would leave after m Arnoldi / CGS2 steps of a dense symmetric matrix, computed in
    np.longdouble and rounded to fp64; each h is split into h1 + h2 with h2 about 1e-3 of it.  Step k sits at k * stride:
    h1[0..k], h2[0..k], |remainder|^2.  scale multiplies the matrix (h by scale, the squared norms by scale^2)."""
    rng = _rng(f"{seed}-matrix")
    M = rng.standard_normal((RITZ_N, RITZ_N))
    M = ((M + M.T) / 2).astype(LD)
    v = rng.standard_normal(RITZ_N).astype(LD)
    V = [v / np.sqrt(v @ v)]
    slot = np.zeros(m * stride)
    for k in range(m):
        Vm = np.stack(V)
        w = M @ V[k]
        h = Vm @ w
        w = w - h @ Vm
        c = Vm @ w
        w, h = w - c @ Vm, h + c
        b2 = w @ w
        hf = (h * LD(scale)).astype(np.float64)
        h2 = hf * 1e-3 * rng.uniform(-1.0, 1.0, size=k + 1)
        kk = k + 1
        slot[k * stride:k * stride + kk] = hf - h2
        slot[k * stride + kk:k * stride + 2 * kk] = h2
        slot[k * stride + 2 * kk] = float(b2 * LD(scale) * LD(scale))
        V.append(w / np.sqrt(b2))
    return slot


def symmetric_slots(S, beta):
    """slot (stride 2m + 1, h2 = 0) whose symmetrised projected matrix is S up to one rounding: the kernel forms
    0.5 (h[i][j] + lower[j][i]) with lower = beta on the sub-diagonal and 0 elsewhere"""
    m = len(S)
    stride = 2 * m + 1
    slot = np.zeros(m * stride)
    for t in range(m):
        for j in range(t + 1):
            slot[t * stride + j] = S[j][t] if j == t else (2 * S[j][t] - beta[j] if j == t - 1 else 2 * S[j][t])
        slot[t * stride + 2 * (t + 1)] = beta[t] ** 2
    return slot


def ritz_reference(slot, m, stride, digits=40):
    """what the header comment of ritz_small_kernel describes, evaluated by mpmath at `digits` digits on the fp64 slot:
    h = h1 + h2, beta = sqrt of the last scalar, cut at the first beta <= 1e-13 max|H|, symmetrise, eigsy."""
    import mpmath
    mp = mpmath.mp
    old = mp.dps
    mp.dps = digits
    try:
        H = mpmath.zeros(m, m)
        beta = []
        scale = mpmath.mpf("1e-300")
        for t in range(m):
            kk = t + 1
            blk = slot[t * stride:t * stride + 2 * kk + 1]
            for j in range(kk):
                H[j, t] = mpmath.mpf(float(blk[j])) + mpmath.mpf(float(blk[kk + j]))
                scale = max(scale, abs(H[j, t]))
            beta.append(mpmath.sqrt(mpmath.mpf(float(blk[2 * kk]))) if blk[2 * kk] > 0 else mpmath.mpf(0))
        for k in range(m - 1):
            scale = max(scale, beta[k])
        me = m
        for k in range(m):
            if beta[k] <= mpmath.mpf("1e-13") * scale:
                me = k + 1
                break
        A = mpmath.zeros(me, me)
        for i in range(me):
            for j in range(i, me):
                lower = beta[i] if j == i + 1 else 0
                A[i, j] = H[i, j] if i == j else (H[i, j] + lower) / 2
                A[j, i] = A[i, j]
        E, Q = mpmath.eigsy(A)
        order = sorted(range(me), key=lambda i: E[i])
        lam = E[order[0]]
        v = [Q[i, order[0]] for i in range(me)]
        if v[0] < 0:
            v = [-x for x in v]
        gap = (E[order[1]] - lam) if me > 1 else None
        norm = mpmath.sqrt(sum(A[i, j] ** 2 for i in range(me) for j in range(me)))
        return dict(m=m, me=me, lam=lam, v=v, gap=gap, norm=norm, beta_last=beta[me - 1], A=A, digits=digits)
    finally:
        mp.dps = old


def ritz_ratios(coef, info, ref, vector=True):
    """error of (coef, info) against the reference in units of u times the natural scale of each quantity:
    value / |A|_F, residual |A c - lambda c|_inf / |A|_F, vector / (|A|_F / gap), estimate / (beta_last |A|_F / gap)"""
    import mpmath
    mp = mpmath.mp
    old = mp.dps
    mp.dps = ref["digits"]
    try:
        me, A, u = ref["me"], ref["A"], mpmath.mpf(U)
        norm = ref["norm"] if ref["norm"] > 0 else mpmath.mpf(1)
        c = [mpmath.mpf(float(x)) for x in coef[:me]]
        lam = mpmath.mpf(float(info[0]))
        r = {"value": abs(lam - ref["lam"]) / (u * norm),
             "residual": max(abs(sum(A[i, j] * c[j] for j in range(me)) - lam * c[i]) for i in range(me)) / (u * norm)}
        if vector:
            cond = norm / ref["gap"] if me > 1 and ref["gap"] > 0 else mpmath.mpf(1)
            cond = max(cond, 1)
            r["vector"] = max(abs(c[i] - ref["v"][i]) for i in range(me)) / (u * cond)
            est = abs(ref["beta_last"] * ref["v"][me - 1])
            den = u * (ref["beta_last"] * cond + est)
            r["estimate"] = abs(mpmath.mpf(float(info[1])) - est) / den if den > 0 else abs(mpmath.mpf(float(info[1])))
        return {k: float(v) for k, v in r.items()}
    finally:
        mp.dps = old


def numpy_ritz(ref):
    """numpy's eigh on the fp64 rounding of the reference matrix, in the kernel's output convention"""
    me = ref["me"]
    A = np.array([[float(ref["A"][i, j]) for j in range(me)] for i in range(me)])
    ev, S = np.linalg.eigh(A)
    v = S[:, 0] * (1.0 if S[0, 0] >= 0 else -1.0)
    coef = np.zeros(ref["m"])
    coef[:me] = v
    return coef, np.array([ev[0], abs(float(ref["beta_last"]) * v[-1]), float(me)])


@functools.lru_cache(maxsize=None)
def ritz_cases():
    """name -> dict(m, stride, slot, kind, cut): kind "plain" compares the vector, "values" (degenerate pair) only the
    eigenvalue, Rayleigh quotient and residual, "sign" the vector up to its sign; cut = the expected info[2] or None"""
    cases = {}

    def add(name, m, stride, slot, kind="plain", cut=None):
        slot.setflags(write=False)
        cases[name] = dict(m=m, stride=stride, slot=slot, kind=kind, cut=cut)

    for m in range(1, 33):
        add(f"m{m}", m, 2 * m + 1, arnoldi_slots(m, 2 * m + 1))
        add(f"m{m}-stride70", m, 70, arnoldi_slots(m, 70))
    m = 8
    base = arnoldi_slots(m, 2 * m + 1)
    hmax = max(np.abs(base).max(), 1.0)
    for j in (0, 1, m - 2, m - 1):
        for nm, b in (("zero", 0.0), ("tiny", 1e-14 * hmax)):
            s = base.copy()
            s[j * (2 * m + 1) + 2 * (j + 1)] = b * b
            add(f"cut{j}-{nm}", m, 2 * m + 1, s, cut=j + 1 if j + 1 < m else m)
    rng = _rng("ritz-special")
    m = 6
    Q = np.linalg.qr(rng.standard_normal((m, m)))[0]
    S = Q @ np.diag([-2.0, -2.0, -0.5, 0.25, 1.0, 3.0]) @ Q.T
    add("degenerate", m, 2 * m + 1, symmetric_slots((S + S.T) / 2, np.ones(m)), kind="values")
    q = rng.standard_normal(m)
    q[0] = 0.0
    Q = np.linalg.qr(np.column_stack([q, rng.standard_normal((m, m - 1))]))[0]
    S = Q @ np.diag([-2.0, -1.0, -0.5, 0.25, 1.0, 3.0]) @ Q.T
    add("sign", m, 2 * m + 1, symmetric_slots((S + S.T) / 2, np.ones(m)), kind="sign")
    add("zero", 5, 11, np.zeros(55), cut=1)
    add("scale+150", 8, 17, arnoldi_slots(8, 17, scale=1e150))
    add("scale-150", 8, 17, arnoldi_slots(8, 17, scale=1e-150))
    # a zero diagonal entry next to an off-diagonal of 1e-160 max|H|: pair (0, 3) is the first rotation of the first
    # round for m = 4 and sees the untouched entries; theta^2 = ((a33 - a00) / (2 a03))^2 overflows
    S = np.array([[0.0, 0.5, 0.25, 1e-160], [0.5, 1.0, -0.75, 0.5], [0.25, -0.75, -1.0, 0.5], [1e-160, 0.5, 0.5, 2.0]])
    add("overflow", 4, 9, symmetric_slots(S, np.ones(4)))
    return cases


@functools.lru_cache(maxsize=None)
def ritz_ref(name):
    c = ritz_cases()[name]
    return ritz_reference(c["slot"], c["m"], c["stride"])


def run_ritz(be, name):
    """(coef[m], info[3]) of mpsk_vritz_dev (any backend with ritz_dev) on a case's slot"""
    c = ritz_cases()[name]
    slot = be.upload(c["slot"])
    buf = be.upload(np.full(40, np.nan))
    be.ritz_dev(c["m"], c["stride"], slot, buf)
    out = be.download(buf)
    return out[:c["m"]].copy(), out[32:35].copy()


def check_ritz(name, coef, info, bound, out=None):
    """the assertions of the Ritz tests as mismatch records; returns (records, ratios)"""
    out = [] if out is None else out
    c, ref = ritz_cases()[name], ritz_ref(name)
    m, me = c["m"], ref["me"]
    if not (np.isfinite(coef).all() and np.isfinite(info).all()):
        out.append(f"{name}: non-finite output coef={coef} info={info}")
        return out, {}
    if c["cut"] is not None and me != c["cut"]:
        out.append(f"{name}: the reference cuts at {me}, the case expects {c['cut']}")
    if info[2] != me:
        out.append(f"{name}: info[2] = {info[2]}, expected {me}")
    if np.any(coef[me:] != 0.0):
        out.append(f"{name}: coefficients past the cut are not exactly zero: {coef[me:]}")
    if abs(np.sqrt(float(np.sum(coef.astype(LD) ** 2))) - 1.0) > 4 * U * m:
        out.append(f"{name}: |coef| - 1 = {np.linalg.norm(coef) - 1.0:.3e} exceeds 4 u m")
    if not coef[0] >= 0:
        out.append(f"{name}: coef[0] = {coef[0]} is negative")
    kind = c["kind"]
    r = ritz_ratios(coef, info, ref, vector=kind != "values")
    if kind == "sign":                                   # reference component on the start vector is ~0: either sign
        flipped = np.concatenate([[coef[0]], -coef[1:]])
        r2 = ritz_ratios(flipped, info, ref)
        if r2["vector"] < r["vector"]:
            r = r2
    for k, v in r.items():
        if not v <= bound:
            out.append(f"{name}: {k} error is {v:.2f} u-units, allowed {bound:.2f}")
    return out, r
