"""mpsk_gemm_pair and mpsk_grassmann_coef (mpsk_gemm.hip: gemm_pair_f64_kernel, grassmann_coef_kernel) against exact references.

gemm_pair: small integer P, Q, B and coefficients make every partial sum exactly representable (|sum| <= 128 * 12 * 3), so
the comparison with NumPy integer arithmetic is bit for bit.  Per shape and forced tile: two outputs with Q, Q = NULL,
out2 = NULL, beta1 = 1 onto a non-zero output; leading dimensions larger than the row counts; padding rows below row M - 1 and
padding columns behind column N - 1 of both outputs (and, for beta = 0, the whole output) poisoned with NaN beforehand and
checked untouched afterwards.  A forced 128x128 tile runs the
two-output form as 128x64 (documented in gemm_pair_f64).  Kernels reached: <64|128, 64|128, ALIGNED = false> for the ragged
shapes, ALIGNED = true for (256, 128, 128) with even leading dimensions; TWO = true / false."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILES = [(64, 64), (128, 64), (64, 128), (128, 128)]
SHAPES = [(10, 5, 5), (48, 16, 16), (130, 65, 65), (256, 128, 128)]


def _padded(be, a, ld, fill=np.nan, cols=0):
    """device buffer of an (ld x (columns of a + cols)) column-major matrix holding `a` in its leading rows and columns,
    `fill` in the padding rows below and the padding columns behind"""
    buf = np.full((ld, a.shape[1] + cols), fill)
    buf[: a.shape[0], : a.shape[1]] = a
    return be.upload(buf), buf


def _run(be, M, K, N, pad, rng, with_q=True, two=True, beta1=0.0):
    P, Q, B = (rng.integers(-3, 4, s).astype(float) for s in ((M, K), (M, K), (K, N)))
    coef = rng.integers(-2, 3, (4, K)).astype(float)
    C0 = rng.integers(-5, 6, (M, N)).astype(float) if beta1 else np.full((M, N), np.nan)
    dP, _ = _padded(be, P, M + pad, 7.0)
    dQ, _ = _padded(be, Q, M + pad + 2, 7.0)
    dB, _ = _padded(be, B, K + pad, 7.0)
    dcoef, _ = _padded(be, coef.T, K + 1, 7.0)              # row r of coef = column r of a (K + 1)-row buffer: ldcoef = K + 1
    d1, h1 = _padded(be, C0, M + pad, cols=pad)              # pad padding columns behind column N - 1, NaN like the rows
    d2, h2 = _padded(be, np.full((M, N), np.nan), M + pad + 4, cols=pad)
    be.gemm_pair_raw(M, N, K, dP.ptr, M + pad, dQ.ptr if with_q else None, M + pad + 2, dB.ptr, K + pad, dcoef.ptr, K + 1,
                     beta1, d1.ptr, M + pad, 0.0, d2.ptr if two else None, M + pad + 4)
    Pi, Qi, Bi, ci = (x.astype(np.int64) for x in (P, Q if with_q else 0 * Q, B, coef))
    r1 = (Pi * ci[0] + Qi * ci[1]) @ Bi + (C0.astype(np.int64) if beta1 else 0)
    r2 = (Pi * ci[2] + Qi * ci[3]) @ Bi
    g1, g2 = be.download(d1), be.download(d2)
    bad = []
    if not np.array_equal(g1[:M, :N], r1.astype(float)):
        bad.append("out1")
    if not (np.isnan(g1[M:]).all() and np.isnan(g1[:, N:]).all()):
        bad.append("out1 padding rows / columns")
    if two and not np.array_equal(g2[:M, :N], r2.astype(float)):
        bad.append("out2")
    if not (np.isnan(g2[M:]).all() and np.isnan(g2[:, N:]).all() if two else np.isnan(g2).all()):
        bad.append("out2 padding rows / columns / unused out2")
    return bad, g1.tobytes() + g2.tobytes()


@pytest.mark.parametrize("tile", TILES, ids=lambda t: f"{t[0]}x{t[1]}")
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gemm_pair_exact(be, shape, tile):
    M, K, N = shape
    pad = 2 if shape == (256, 128, 128) else 3              # even leading dimensions keep the aligned loader
    bad = []
    try:
        be.lib.mpsk_ctx_force_tile(be.ctx, *tile)
        for name, kw in [("both", {}), ("Q=NULL", {"with_q": False}), ("out2=NULL", {"two": False}),
                         ("beta1=1", {"beta1": 1.0}), ("beta1=1, Q=NULL, out2=NULL", {"beta1": 1.0, "with_q": False, "two": False})]:
            b1, bytes1 = _run(be, M, K, N, pad, np.random.default_rng(11), **kw)
            b2, bytes2 = _run(be, M, K, N, pad, np.random.default_rng(11), **kw)
            bad += [(name, x) for x in b1 + b2]
            if bytes1 != bytes2:
                bad.append((name, "run-to-run bytes differ"))
    finally:
        be.lib.mpsk_ctx_force_tile(be.ctx, 0, 0)            # process-wide knob: never leave a tile forced
    assert not bad, bad


def test_gemm_pair_default_tile_and_refusals(be):
    for shape in SHAPES:
        bad, _ = _run(be, *shape, 3, np.random.default_rng(5))
        assert not bad, (shape, bad)
    x = be.zeros(4, 4)
    args = (4, 4, 4, x.ptr, 4, None, 4, x.ptr, 4, x.ptr, 4, 0.0, be.zeros(4, 4).ptr, 4, 0.0, None, 4)
    be._set_dtype(True)
    try:
        assert be.lib.mpsk_gemm_pair(be.ctx, *args) == 3                                        # MPSK_ERR_UNSUPPORTED
        assert be.lib.mpsk_grassmann_coef(be.ctx, 4, x.ptr, 0.0, 0, be.zeros(4, 4).ptr) == 3
    finally:
        be._set_dtype(False)
    short = list(args)
    short[4] = 3                                                                                # ldp < M
    assert be.lib.mpsk_gemm_pair(be.ctx, *short) == 1                                           # MPSK_ERR_INVALID


@pytest.mark.parametrize("K", [5, 65])
def test_grassmann_coef(be, K):
    """4 ulp of max(1, |value|): twice the documented 2 ulp bound of the device sin / cos (they are not correctly rounded);
    the other operations of a row are one rounding each.  Measured on an MI355X: at most 0.5 ulp, over all modes and scalars."""
    s = np.logspace(-12, np.log10(3.0), K)
    S = be.upload(s)
    worst = 0.0
    for scalar in (0.0, 0.37, -2.0):
        refs = {"retract": [np.cos(scalar * s), np.sin(scalar * s), -s * np.sin(scalar * s), s * np.cos(scalar * s)],
                "transport": [-np.sin(scalar * s), np.cos(scalar * s) - 1.0, 0 * s, 0 * s],
                "precondition": [s / (s ** 2 + (s.max() * scalar) ** 2), 0 * s, 0 * s, 0 * s]}
        for mode, ref in refs.items():
            got = be.download(be.grassmann_coef(S, scalar, mode)).T          # (K, 4) column-major -> rows a1, b1, a2, b2
            ref = np.array(ref)
            ulp = np.spacing(np.maximum(1.0, np.abs(ref)))
            err = np.abs(got - ref) / ulp
            worst = max(worst, err.max())
            print(f"grassmann_coef K={K} {mode} scalar={scalar}: max error {err.max():.2f} ulp")
            assert err.max() <= 4.0, (mode, scalar, err.max())
            if mode == "retract" and scalar == 0.0:
                assert np.array_equal(got[0], np.ones(K)) and np.array_equal(got[1], np.zeros(K))
