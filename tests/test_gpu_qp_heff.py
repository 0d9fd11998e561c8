"""mpsk_qp_heff_site against float64 numpy.einsum of its defining sum (include/mpsk.h):

    Xout = VL^T ( proj(GL, GR; VL X) + proj(lB, GR; AR) + proj(GL, rB; AL) ) - E X

on a sparse slice (Heisenberg, W = 5) and on dense slices forced down each of their two routes, with every combination of
the two optional pairs, E = 0 and E != 0.

Tolerance: the bound tests/test_gpu_qp_apply.py uses for mpsk_qp_apply -- RTOL = 2e-13 times the largest bond, relative to
the largest entry of the reference, once per summed term (3 with both pairs, 2 with one, 1 with none) -- plus one more term
of the same size for each of the two GEMMs the entry adds (B = VL X in front, the pull-back behind): every one of them is a
product of the same GEMM family whose rounding errors add."""
import numpy as np
import pytest

import mpskit_jl_amd as mk

pytestmark = pytest.mark.gpu

RTOL = 2e-13
SEED = 20250907
# (Dl, d, DrL, Dr), DrL the column count of AL: complements 8 (below one tile), 15 (one short of a tile), 35 (crosses a
# 16-wide and a 32-wide tile edge), 65
SHAPES = [(5, 3, 7, 9), (17, 2, 19, 23), (33, 2, 31, 33), (65, 2, 65, 65)]
KINDS = ["sparse", "dense1", "dense0"]
POISON = -7.25e77


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def slabs(be, arr):
    """host [w, i, j] -> device environment (W, D1, D2), every slab column-major"""
    return be.upload(np.transpose(arr, (1, 2, 0))).reshape(*arr.shape)


def full_O(H):
    ol, orr = np.concatenate([[0], np.cumsum(H.chil)]), np.concatenate([[0], np.cumsum(H.chir)])
    O = np.zeros((H.Wl, H.d, H.d, H.Wr))
    for (i, j), v in H.blocks.items():
        blk = v * np.einsum("wv,ts->wtsv", np.eye(H.chil[i], H.chir[j]), np.eye(H.d)) if np.isscalar(v) else np.asarray(v)
        O[ol[i]:ol[i + 1], :, :, orr[j]:orr[j + 1]] = blk
    return O


def make_slice(be, monkeypatch, kind, d, rng):
    if kind == "sparse":
        monkeypatch.delenv("MPSK_DENSE_ROUTE", raising=False)
        H = mk.heisenberg_XXX(0.5 if d == 2 else 1.0, be=be)[0]
        assert (H.Wl, H.Wr, H.d) == (5, 5, d)
        return H, full_O(H)
    monkeypatch.setenv("MPSK_DENSE_ROUTE", kind[-1])
    O = rng.random((3, d, d, 4))
    return be.mposlice_dense(O), O


def proj(G, x, O, R):
    """y[p,t,q] = sum G[w][p,a] x[a,s,b] O[w,t,s,v] R[v][b,q], pairwise"""
    T1 = np.einsum("wpa,asb->pwsb", G, x, optimize=True)
    T2 = np.einsum("pwsb,wtsv->pbtv", T1, O, optimize=True)
    return np.einsum("pbtv,vbq->ptq", T2, R, optimize=True)


def operands(be, H, shape, rng):
    """host and device operands of one site; AL | VL are the columns of one orthogonal matrix"""
    Dl, d, DrL, Dr = shape
    Wl, Wr = H.Wl, H.Wr
    n = Dl * d - DrL
    Dl2 = max(Dl - 2, 1)
    Q, _ = np.linalg.qr(rng.standard_normal((Dl * d, Dl * d)))
    h = dict(GL=rng.standard_normal((Wl, Dl, Dl)), GR=rng.standard_normal((Wr, Dr, Dr)),
             AL=Q[:, :DrL].reshape((Dl, d, DrL), order="F"), VL=Q[:, DrL:], X=rng.standard_normal((n, Dr)),
             lB=rng.standard_normal((Wl, Dl, Dl2)), AR=rng.standard_normal((Dl2, d, Dr)), rB=rng.standard_normal((Wr, DrL, Dr)))
    dev = {k: (slabs(be, v) if k in ("GL", "GR", "lB", "rB") else be.upload(v)) for k, v in h.items()}
    return h, dev


@pytest.mark.parametrize("shape", SHAPES, ids=["n8", "n15", "n35", "n65"])
@pytest.mark.parametrize("kind", KINDS)
def test_qp_heff_site(be, monkeypatch, kind, shape):
    rng = np.random.default_rng(SEED)
    Dl, d, DrL, Dr = shape
    H, O = make_slice(be, monkeypatch, kind, d, rng)
    h, dv = operands(be, H, shape, rng)
    n = Dl * d - DrL
    B = (h["VL"] @ h["X"]).reshape((Dl, d, Dr), order="F")          # rows of VL: (p, t) column-major, p fastest
    t1, t2, t3 = proj(h["GL"], B, O, h["GR"]), proj(h["lB"], h["AR"], O, h["GR"]), proj(h["GL"], h["AL"], O, h["rB"])
    pull = lambda y: h["VL"].T @ y.reshape((Dl * d, Dr), order="F")
    half = be.qp_half(H, dv["GL"], dv["AL"])
    half0, X0 = be.download(half), be.download(dv["X"])
    bound = RTOL * max(Dl, DrL, Dr)                    # Dl2 = Dl - 2 is never the largest
    call = lambda E, lB, AR, hf, rB: be.download(be.qp_heff_site(H, dv["GL"], dv["GR"], dv["VL"], dv["X"], E, lB, AR, hf, rB))
    for E in (0.0, -3.7):
        cases = {"all": (call(E, dv["lB"], dv["AR"], half, dv["rB"]), t1 + t2 + t3, 3),
                 "no_left": (call(E, None, None, half, dv["rB"]), t1 + t3, 2),
                 "no_right": (call(E, dv["lB"], dv["AR"], None, None), t1 + t2, 2),
                 "plain": (call(E, None, None, None, None), t1, 1)}
        for name, (got, y, terms) in cases.items():
            ref = pull(y) - E * h["X"]
            assert got.shape == (n, Dr)
            e = relerr(got, ref)
            print("qp_heff_site", kind, shape, "E", E, name, e, "bound", (terms + 2) * bound)
            assert e < (terms + 2) * bound, (name, E, e)
        # bit-identical from run to run
        assert np.array_equal(call(E, dv["lB"], dv["AR"], half, dv["rB"]), cases["all"][0])
        if E == 0.0:
            # both pairs NULL and E = 0: VL^T dAC_proj(VL X) from the existing entries
            Bd = be.gemm(dv["VL"], dv["X"]).reshape(Dl, d, Dr)
            yd = be.dAC_proj(H, dv["GL"], dv["GR"], Bd)
            comp = be.download(be.gemm(dv["VL"], yd.reshape(Dl * d, Dr), transA=True))
            e = relerr(cases["plain"][0], comp)
            print("qp_heff_site", kind, shape, "against composed", e, "bound", 3 * bound)
            assert e < 3 * bound
    # X and the half buffer are read, not consumed
    assert np.array_equal(be.download(dv["X"]), X0)
    assert np.array_equal(be.download(half), half0)


def test_split_k_pullback(be, monkeypatch):
    """The pull-back GEMM in its split-K form.  (Dl, d, DrL, Dr) = (512, 2, 512, 64) gives M = 512, N = 64, K = Dl d = 1024:
    8 tiles of 64 x 64 and 64 k-tiles of 16, the smallest K at which the GEMM core splits (64 x 64 tiles, at least 64
    k-tiles, at most 4096 tiles), and with 8 tiles on 256 CUs its cost model takes two shares or more.  The share that
    starts a tile adds gamma Z and writes C, the others write partial tiles, the fixup adds them onto C: E != 0 makes a Z
    added twice, dropped, or read at a wrong offset visible.  Same bound as above, for the shapes used here."""
    rng = np.random.default_rng(SEED + 2)
    shape = (512, 2, 512, 64)
    Dl, d, DrL, Dr = shape
    H, O = make_slice(be, monkeypatch, "sparse", d, rng)
    h, dv = operands(be, H, shape, rng)
    n = Dl * d - DrL
    B = (h["VL"] @ h["X"]).reshape((Dl, d, Dr), order="F")
    t1, t2, t3 = proj(h["GL"], B, O, h["GR"]), proj(h["lB"], h["AR"], O, h["GR"]), proj(h["GL"], h["AL"], O, h["rB"])
    half = be.qp_half(H, dv["GL"], dv["AL"])
    X0 = be.download(dv["X"])
    bound = RTOL * max(Dl, DrL, Dr)
    for E in (0.0, -3.7):
        got = be.download(be.qp_heff_site(H, dv["GL"], dv["GR"], dv["VL"], dv["X"], E, dv["lB"], dv["AR"], half, dv["rB"]))
        plain = be.download(be.qp_heff_site(H, dv["GL"], dv["GR"], dv["VL"], dv["X"], E))
        for name, res, y, terms in (("all", got, t1 + t2 + t3, 3), ("plain", plain, t1, 1)):
            ref = h["VL"].T @ y.reshape((Dl * d, Dr), order="F") - E * h["X"]
            e = relerr(res, ref)
            print("qp_heff_site split-K", shape, "E", E, name, e, "bound", (terms + 2) * bound)
            assert res.shape == (n, Dr) and e < (terms + 2) * bound, (name, E, e)
        again = be.download(be.qp_heff_site(H, dv["GL"], dv["GR"], dv["VL"], dv["X"], E, dv["lB"], dv["AR"], half, dv["rB"]))
        assert np.array_equal(again, got)
    # X is read, not consumed
    assert np.array_equal(be.download(dv["X"]), X0)


@pytest.mark.parametrize("kind", KINDS)
def test_empty_complement_writes_nothing(be, monkeypatch, kind):
    """Dl d == DrL: MPSK_OK and the output buffer keeps its poison."""
    rng = np.random.default_rng(SEED + 1)
    shape = (4, 2, 8, 8)
    Dl, d, DrL, Dr = shape
    H, _ = make_slice(be, monkeypatch, kind, d, rng)
    h, dv = operands(be, H, shape, rng)
    assert dv["VL"].shape == (8, 0) and dv["X"].shape == (0, 8)
    out = mk.DTensor(be.upload(np.full(64, POISON)).buf, (0, Dr))
    half = be.qp_half(H, dv["GL"], dv["AL"])
    got = be.qp_heff_site(H, dv["GL"], dv["GR"], dv["VL"], dv["X"], 1.5, dv["lB"], dv["AR"], half, dv["rB"], out=out)
    be.synchronize()
    assert got is out
    assert np.array_equal(out.buf.cpu().numpy(), np.full(64, POISON))


def test_refusals(be):
    """An MPSK_C128 slice or ctx gets MPSK_ERR_UNSUPPORTED (3); Xout aliasing X and half-given pairs get MPSK_ERR_INVALID (1)."""
    Hc = be.mposlice(2, 2, [1, 1], [1, 1], {(0, 0): 1.0, (0, 1): np.ones((1, 2, 2, 1)) * 1j, (1, 1): 1.0}, cplx=True)
    Hr = mk.heisenberg_XXX(0.5, be=be)[0]
    bufs = be.empty(256), be.empty(256)
    p, q = bufs[0].ptr, bufs[1].ptr
    lib, ctx = be.lib, be.ctx
    E = 0.5
    assert lib.mpsk_qp_heff_site(ctx, Hc.handle, 2, 2, 2, 0, 0, p, p, p, p, E, None, None, None, None, q) == 3
    assert b"MPSK_F64 only" in lib.mpsk_last_error()
    assert lib.mpsk_qp_heff_site(ctx, Hr.handle, 2, 2, 2, 0, 0, p, p, p, p, E, None, None, None, None, p) == 1
    assert b"alias" in lib.mpsk_last_error()
    assert lib.mpsk_qp_heff_site(ctx, Hr.handle, 2, 2, 2, 2, 0, p, p, p, p, E, p, None, None, None, q) == 1
    assert lib.mpsk_qp_heff_site(ctx, Hr.handle, 2, 2, 2, 0, 2, p, p, p, p, E, None, None, p, None, q) == 1
    assert be.has_qp_heff
    # an MPSK_C128 ctx with a real slice
    be._set_dtype(True)
    try:
        rc = lib.mpsk_qp_heff_site(ctx, Hr.handle, 2, 2, 2, 0, 0, p, p, p, p, E, None, None, None, None, q)
        msg = lib.mpsk_last_error()
    finally:
        be._set_dtype(False)
    assert rc == 3 and b"MPSK_F64 only" in msg, (rc, msg)
