"""mpsk_qp_half / mpsk_qp_apply / mpsk_transfer_left_pair / mpsk_transfer_right_pair against float64 numpy.einsum of their
defining sums (include/mpsk.h), on sparse slices (Heisenberg, W = 5) and on dense slices forced down each of their two
routes.

Tolerance: the bound of the mpsk_dAC_proj parity tests (tests/test_gpu_approximate.py: RTOL = 2e-13 times the largest bond,
relative to the largest entry of the reference), times the number of summed terms -- 3 for mpsk_qp_apply with both pairs, 2
with one pair and for the pair transfers, 1 for a single term: every term is one chain of the same three stages and their
rounding errors add."""
import numpy as np
import pytest

import mpskit_jl_amd as mk

pytestmark = pytest.mark.gpu

RTOL = 2e-13
SEED = 20250611
SHAPES = [(20, 24, 17, 33, 19, 28), (65, 65, 65, 65, 65, 65)]          # Dlo, Dl, Dl2, Dr, Dr2, Dro
KINDS = ["sparse", "dense1", "dense0"]


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def slabs(be, arr):
    """host [w, i, j] -> device environment (W, D1, D2), every slab column-major"""
    return be.upload(np.transpose(arr, (1, 2, 0))).reshape(*arr.shape)


def env_host(be, t):
    W, D1, D2 = t.shape
    return be.download(t.reshape(t.size)).reshape(W, D2, D1).transpose(0, 2, 1)


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


def tl(V, A, O, Ab):
    """out[v][q,b] = sum V[w][p,a] A[a,s,b] O[w,t,s,v] Ab[p,t,q], pairwise"""
    T1 = np.einsum("wpa,asb->pwsb", V, A, optimize=True)
    T2 = np.einsum("pwsb,wtsv->pbtv", T1, O, optimize=True)
    return np.einsum("pbtv,ptq->vqb", T2, Ab, optimize=True)


def tr(V, A, O, Ab):
    """out[w][a,p] = sum A[a,s,b] O[w,t,s,v] Ab[p,t,q] V[v][b,q], pairwise"""
    T1 = np.einsum("asb,vbq->asvq", A, V, optimize=True)
    T2 = np.einsum("asvq,wtsv->awtq", T1, O, optimize=True)
    return np.einsum("awtq,ptq->wap", T2, Ab, optimize=True)


@pytest.mark.parametrize("shape", SHAPES, ids=["odd", "b65"])
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_qp_apply(be, monkeypatch, kind, d, shape):
    rng = np.random.default_rng(SEED)
    H, O = make_slice(be, monkeypatch, kind, d, rng)
    Dlo, Dl, Dl2, Dr, Dr2, Dro = shape
    Wl, Wr = H.Wl, H.Wr
    GL, GR = rng.standard_normal((Wl, Dlo, Dl)), rng.standard_normal((Wr, Dr, Dro))
    B, lB, AR = rng.standard_normal((Dl, d, Dr)), rng.standard_normal((Wl, Dlo, Dl2)), rng.standard_normal((Dl2, d, Dr))
    AL, rB = rng.standard_normal((Dl, d, Dr2)), rng.standard_normal((Wr, Dr2, Dro))
    t1, t2, t3 = proj(GL, B, O, GR), proj(lB, AR, O, GR), proj(GL, AL, O, rB)
    dGL, dGR, dB, dlB, dAR, drB = slabs(be, GL), slabs(be, GR), be.upload(B), slabs(be, lB), be.upload(AR), slabs(be, rB)
    half = be.qp_half(H, dGL, be.upload(AL))
    half0 = be.download(half)
    bound = RTOL * max(shape)
    full = be.download(be.qp_apply(H, dGL, dGR, dB, dlB, dAR, half, drB))
    assert full.shape == (Dlo, d, Dro)
    cases = {"all": (full, t1 + t2 + t3, 3),
             "no_left": (be.download(be.qp_apply(H, dGL, dGR, dB, None, None, half, drB)), t1 + t3, 2),
             "no_right": (be.download(be.qp_apply(H, dGL, dGR, dB, dlB, dAR, None, None)), t1 + t2, 2)}
    plain = be.download(be.qp_apply(H, dGL, dGR, dB))
    cases["plain"] = (plain, t1, 1)
    for name, (got, ref, terms) in cases.items():
        e = relerr(got, ref)
        print("qp_apply", kind, d, shape, name, e, "bound", terms * bound)
        assert e < terms * bound, (name, e)
    # both pairs NULL: mpsk_dAC_proj bit for bit
    assert np.array_equal(plain, be.download(be.dAC_proj(H, dGL, dGR, dB)))
    # the half buffer is read, not consumed
    assert np.array_equal(be.download(half), half0)
    assert np.array_equal(be.download(be.qp_apply(H, dGL, dGR, dB, dlB, dAR, half, drB)), full)


@pytest.mark.parametrize("shape", SHAPES, ids=["odd", "b65"])
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_pair_transfers(be, monkeypatch, kind, d, shape):
    rng = np.random.default_rng(SEED + 1)
    H, O = make_slice(be, monkeypatch, kind, d, rng)
    Dlb, Dl1, Dl2, Dr, Dr2, Drb = shape
    Wl, Wr = H.Wl, H.Wr
    bound = RTOL * max(shape)
    Ab = rng.standard_normal((Dlb, d, Drb))
    dAb = be.upload(Ab)
    # left: kets [Dl1, d, Dr] and [Dl2, d, Dr]
    V1, A1 = rng.standard_normal((Wl, Dlb, Dl1)), rng.standard_normal((Dl1, d, Dr))
    V2, A2 = rng.standard_normal((Wl, Dlb, Dl2)), rng.standard_normal((Dl2, d, Dr))
    dV1, dA1, dA2 = slabs(be, V1), be.upload(A1), be.upload(A2)
    got = env_host(be, be.transfer_left_pair(H, dV1, dA1, slabs(be, V2), dA2, dAb))
    ref1 = tl(V1, A1, O, Ab)
    ref = ref1 + tl(V2, A2, O, Ab)
    assert got.shape == (Wr, Drb, Dr)
    e = relerr(got, ref)
    got0 = env_host(be, be.transfer_left_pair(H, dV1, dA1, slabs(be, np.zeros_like(V2)), dA2, dAb))
    one = env_host(be, be.transfer_left_ex(H, dV1, dA1, dAb))
    e0, e1 = relerr(got0, one), relerr(got0, ref1)
    print("left pair", kind, d, shape, e, e0, e1, "bound", 2 * bound)
    assert e < 2 * bound and e0 < 2 * bound and e1 < 2 * bound
    # right: kets [Dl1, d, Dr] and [Dl1, d, Dr2]
    V1, A1 = rng.standard_normal((Wr, Dr, Drb)), rng.standard_normal((Dl1, d, Dr))
    V2, A2 = rng.standard_normal((Wr, Dr2, Drb)), rng.standard_normal((Dl1, d, Dr2))
    dV1, dA1, dA2 = slabs(be, V1), be.upload(A1), be.upload(A2)
    got = env_host(be, be.transfer_right_pair(H, dV1, dA1, slabs(be, V2), dA2, dAb))
    ref1 = tr(V1, A1, O, Ab)
    ref = ref1 + tr(V2, A2, O, Ab)
    assert got.shape == (Wl, Dl1, Dlb)
    e = relerr(got, ref)
    got0 = env_host(be, be.transfer_right_pair(H, dV1, dA1, slabs(be, np.zeros_like(V2)), dA2, dAb))
    one = env_host(be, be.transfer_right_ex(H, dV1, dA1, dAb))
    e0, e1 = relerr(got0, one), relerr(got0, ref1)
    print("right pair", kind, d, shape, e, e0, e1, "bound", 2 * bound)
    assert e < 2 * bound and e0 < 2 * bound and e1 < 2 * bound


def test_complex_is_unsupported(be):
    """MPSK_C128 slices are refused by all four entries with MPSK_ERR_UNSUPPORTED (3)."""
    Hc = be.mposlice(2, 2, [1, 1], [1, 1], {(0, 0): 1.0, (0, 1): np.ones((1, 2, 2, 1)) * 1j, (1, 1): 1.0}, cplx=True)
    p = be.empty(64).ptr
    lib, ctx = be.lib, be.ctx
    rcs = [lib.mpsk_qp_half(ctx, Hc.handle, 2, 2, 2, p, p, p),
           lib.mpsk_qp_apply(ctx, Hc.handle, 2, 2, 0, 2, 0, 2, p, p, p, None, None, None, None, p),
           lib.mpsk_transfer_left_pair(ctx, Hc.handle, 2, 2, 2, 2, 2, p, p, p, p, p, p),
           lib.mpsk_transfer_right_pair(ctx, Hc.handle, 2, 2, 2, 2, 2, p, p, p, p, p, p)]
    assert rcs == [3, 3, 3, 3], rcs
    assert b"MPSK_F64 only" in lib.mpsk_last_error()
