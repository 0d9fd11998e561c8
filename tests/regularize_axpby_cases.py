"""Operands and the exact reference for mpsk_regularize_axpby (include/mpsk.h):
    coef_w = sum_{p,q} lvec[q,p] y[w][p,q]              (bilinear: nothing is conjugated)
    out[w] = a0 x[w] + a1 (y[w] - coef_w rvec)
Integer-valued operands (entries in [-3, 3], Gaussian integers for the complex dtype) and a0, a1 from {1, -1, 2, 0.5}: every
partial sum of the dot is an integer far below 2^53 and the update is exact in fp64, so the result does not depend on the
summation order and the device must return the reference bit for bit.  tests/test_regularize_axpby_cases_cpu.py proves
both statements without a GPU; tests/test_gpu_regularize_axpby.py runs the entry."""
import numpy as np

# phase 2 of the entry: at most 1024 workgroups per slab, 2048 elements each below the cap, a grid-stride loop above it
# (RGA_MAX_BLOCKS / RGA_BLOCK_ELEMS of mpsk_gauge.hip)
PASS_ELEMENTS = 1024 * 2048
TILE = 32

# (W, D1, D2): one element; both edges of the 32-tile straddled; aligned; many ragged tiles, rectangular; more elements
# than one pass of phase 2's grid covers
SHAPES = [(1, 1, 1), (2, 33, 31), (3, 64, 64), (1, 257, 129), (1, 1500, 1400)]
BIG = (1, 1500, 1400)
SCALARS = [(1.0, -1.0), (-1.0, 2.0), (2.0, 0.5), (0.5, 1.0)]          # (a0, a1), one pair per shape in turn


def scalars(shape):
    return SCALARS[SHAPES.index(shape) % len(SCALARS)]


def ints(rng, shape, cplx):
    re = rng.integers(-3, 4, shape).astype(np.float64)
    return (re + 1j * rng.integers(-3, 4, shape)).astype(np.complex128) if cplx else re


def operands(shape, cplx, seed=0):
    """y, x [W, D1, D2]; lvec [D2, D1]; rvec [D1, D2]"""
    W, D1, D2 = shape
    rng = np.random.default_rng(7000 + 10 * seed + int(cplx))
    return dict(y=ints(rng, (W, D1, D2), cplx), x=ints(rng, (W, D1, D2), cplx), lvec=ints(rng, (D2, D1), cplx),
                rvec=ints(rng, (D1, D2), cplx))


def ref(y, lvec, rvec, a1, x=None, a0=0.0):
    coef = np.einsum("qp,wpq->w", lvec, y)
    out = a1 * (y - coef[:, None, None] * rvec[None])
    return out if x is None else a0 * x + out


def guard(y, lvec, rvec, a1, x=None, a0=0.0):
    """the same in longdouble, real and imaginary parts apart: (re, im, bound on every |partial sum| of the dot, bound on
    every |intermediate| of the update)"""
    ld = np.longdouble
    yr, yi, lr, li, rr, ri = (np.asarray(v).astype(ld) for v in (y.real, y.imag, lvec.real, lvec.imag, rvec.real, rvec.imag))
    cr = np.einsum("qp,wpq->w", lr, yr) - np.einsum("qp,wpq->w", li, yi)
    ci = np.einsum("qp,wpq->w", lr, yi) + np.einsum("qp,wpq->w", li, yr)
    our = ld(a1) * (yr - (cr[:, None, None] * rr[None] - ci[:, None, None] * ri[None]))
    oui = ld(a1) * (yi - (cr[:, None, None] * ri[None] + ci[:, None, None] * rr[None]))
    if x is not None:
        our = our + ld(a0) * x.real.astype(ld)
        oui = oui + ld(a0) * x.imag.astype(ld)
    dot_bound = float(np.einsum("qp,wpq->w", np.abs(lr) + np.abs(li), np.abs(yr) + np.abs(yi)).max())
    # every intermediate of the update is a multiple of 1/2 bounded by |a0| |x| + |a1| (|y| + 2 |coef| |rvec|_inf)
    upd_bound = 2.0 * 3 + 2.0 * (3 + 2 * dot_bound * 3)
    return our, oui, dot_bound, upd_bound


def _swap_layout(m):
    """the matrix read with its two dimensions swapped (same column-major memory), given back in the original shape"""
    r, c = m.shape
    return m.ravel(order="F").reshape((c, r), order="F").T


# wrong contractions a correct reference must tell apart; each takes the arguments of `ref`
WRONG = {
    "lvec not transposed": lambda y, l, r, a1, x, a0: ref(y, _swap_layout(l), r, a1, x, a0),
    "lvec conjugated": lambda y, l, r, a1, x, a0: ref(y, np.conj(l), r, a1, x, a0),
    "coefficient shared across slabs": lambda y, l, r, a1, x, a0: a0 * x + a1 * (
        y - np.einsum("qp,pq->", l, y[0]) * r[None]),
    "rvec transposed where square": lambda y, l, r, a1, x, a0: ref(y, l, r.T if r.shape[0] == r.shape[1] else r, a1, x, a0),
    "a0 and a1 swapped": lambda y, l, r, a1, x, a0: ref(y, l, r, a0, x, a1),
}


def applies(wrong, shape, cplx):
    """whether the wrong contraction can differ from the right one on this shape and dtype at all"""
    W, D1, D2 = shape
    if D1 * D2 == 1:                      # the trivial shape: y - lvec y rvec may vanish or coincide
        return False
    if wrong == "lvec conjugated":
        return cplx
    if wrong == "coefficient shared across slabs":
        return W > 1
    if wrong == "rvec transposed where square":
        return D1 == D2
    return True


def slabs(be, G, cplx):
    """[W, D1, D2] -> device slabs (W, D1, D2), interleaved (W, 2 D1, D2) for complex"""
    blocks = [np.transpose(G, (1, 0, 2))]
    return be.upload_env_c(blocks) if cplx else be.upload_env(blocks)


def flat(G, cplx):
    """the memory of the slabs / of one matrix as doubles"""
    G = np.asarray(G)
    parts = [np.ravel(g, order="F") for g in (G if G.ndim == 3 else [G])]
    v = np.concatenate(parts)
    return v.view(np.float64) if cplx else v.astype(np.float64)


def unflat(v, shape, cplx):
    W, D1, D2 = shape
    v = np.asarray(v)
    v = v.view(np.complex128) if cplx else v
    return np.stack([v[w * D1 * D2:(w + 1) * D1 * D2].reshape((D1, D2), order="F") for w in range(W)])
