"""mpsk_dsum_site through the backend: the site step of FiniteMPS + FiniteMPS as one grouped-GEMM launch.

Exact cases: integer inputs with |x| <= 4, so every partial sum is an exact double whatever the order; the expected value is
a NumPy int64 einsum and the assertion is equality of bits.  out is allocated with 8 sentinel words behind it.  Gaussian
cases: the entrywise any-order summation bound K 2^-53 sum |G| |A| with K the contracted extent of that block, reference in
long double; the same call twice returns the same bits."""
import numpy as np
import pytest
import torch

import mpskit_jl_amd as mk
from mpskit_jl_amd.backend import DTensor

pytestmark = pytest.mark.gpu

GUARD = 8
SENTINEL = -7.25
U = 2.0 ** -53
SIDES = ["left", "right"]
# (Dn, D1, D2, E1, E2, d)
CASES = {
    "boundary": (1, 1, 1, 2, 3, 2),                 # G = [1 1]
    "mixed_edges": (17, 5, 12, 16, 1, 2),           # one block of one column, K not a multiple of 4, tile edge + 1
    "three_slices": (33, 16, 17, 15, 18, 3),        # blocks straddling a tile boundary
    "full_tiles": (64, 32, 32, 32, 32, 2),
}
TILES = [(64, 64), (64, 128), (128, 64), (128, 128)]


def _shapes(side, dims):
    """(shape of G, shape of out)"""
    Dn, D1, D2, E1, E2, d = dims
    return ((Dn, D1 + D2), (Dn, d, E1 + E2)) if side == "left" else ((E1 + E2, Dn), (D1 + D2, d, Dn))


def _inputs(rng, side, dims, gauss=False, boundary=False):
    Dn, D1, D2, E1, E2, d = dims
    draw = (lambda s: rng.standard_normal(s)) if gauss else (lambda s: rng.integers(-4, 5, size=s).astype(np.float64))
    G = np.ones(_shapes(side, dims)[0]) if boundary else draw(_shapes(side, dims)[0])
    return G, draw((D1, d, E1)), draw((D2, d, E2))


def _ref(side, dims, G, A1, A2, dtype):
    D1, E1 = dims[1], dims[3]
    G, A1, A2 = G.astype(dtype), A1.astype(dtype), A2.astype(dtype)
    if side == "left":
        return np.concatenate([np.einsum("na,ase->nse", G[:, :D1], A1), np.einsum("na,ase->nse", G[:, D1:], A2)], axis=2)
    return np.concatenate([np.einsum("ase,en->asn", A1, G[:E1]), np.einsum("ase,en->asn", A2, G[E1:])], axis=0)


def _bound(side, dims, G, A1, A2):
    """K 2^-53 sum |G| |A| per entry, K the contracted extent of the block the entry belongs to"""
    _, D1, D2, E1, E2, _ = dims
    K1, K2 = (D1, D2) if side == "left" else (E1, E2)
    a = _ref(side, dims, np.abs(G), np.abs(A1), np.zeros_like(A2), np.longdouble)
    b = _ref(side, dims, np.abs(G), np.zeros_like(A1), np.abs(A2), np.longdouble)
    return U * (K1 * a + K2 * b)


def _guarded(be, shape):
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENTINEL, dtype=torch.float64, device=be.device)
    return DTensor(buf[:n], shape), buf


def _run(be, side, dims, G, A1, A2, ldg=None):
    gshape, oshape = _shapes(side, dims)
    if ldg is None:
        g = be.upload(G)
    else:                                                     # G as the leading rows of a taller, poisoned matrix
        tall = np.full((ldg, gshape[1]), np.nan)
        tall[:gshape[0]] = G
        g = DTensor(be.upload(tall).buf, gshape)
    out, buf = _guarded(be, oshape)
    assert be.dsum_site(side, g, be.upload(A1), be.upload(A2), out=out, ldg=ldg) is out
    h = buf.cpu().numpy()
    assert np.all(h[out.size:] == SENTINEL), "guard words behind out were written"
    return h[:out.size].reshape(oshape, order="F").copy()


def _same_bits(got, ref):
    got, ref = np.ascontiguousarray(got) + 0.0, np.ascontiguousarray(ref, dtype=np.float64) + 0.0
    return np.array_equal(got.view(np.uint64), ref.view(np.uint64))


def _mirror(dims):
    Dn, D1, D2, E1, E2, d = dims
    return (Dn, E1, E2, D1, D2, d)


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("name", list(CASES))
def test_exact(be, name, side):
    rng = np.random.default_rng(len(name) + (side == "right"))
    for dims in {CASES[name], _mirror(CASES[name])}:          # the mirrored case: the boundary site of the other side
        boundary = name == "boundary" and (dims[1] == dims[2] == 1) == (side == "left")
        G, A1, A2 = _inputs(rng, side, dims, boundary=boundary)
        got = _run(be, side, dims, G, A1, A2)
        assert _same_bits(got, _ref(side, dims, G, A1, A2, np.int64)), (side, dims)
        if boundary and side == "left":                       # G = [1 1]: the result is the direct sum itself
            assert np.array_equal(got[:, :, :dims[3]], A1) and np.array_equal(got[:, :, dims[3]:], A2)
        if boundary and side == "right":
            assert np.array_equal(got[:dims[1], :, :], A1) and np.array_equal(got[dims[1]:, :, :], A2)


@pytest.mark.parametrize("side", SIDES)
def test_exact_with_a_leading_dimension(be, side):
    dims = CASES["three_slices"]
    rng = np.random.default_rng(41)
    G, A1, A2 = _inputs(rng, side, dims)
    got = _run(be, side, dims, G, A1, A2, ldg=G.shape[0] + 7)
    assert _same_bits(got, _ref(side, dims, G, A1, A2, np.int64))


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("tile", TILES, ids=[f"{a}x{b}" for a, b in TILES])
def test_exact_on_every_forced_tile(be, tile, side):
    """partial tiles, one full tile of the forced shape on each family, and more than one tile along both directions"""
    rng = np.random.default_rng(tile[0] + 2 * tile[1])
    mk.backend.check(be.lib.mpsk_ctx_force_tile(be.ctx, *tile), "mpsk_ctx_force_tile")
    try:
        for dims in (CASES["three_slices"], (128, 64, 64, 64, 64, 2), (130, 70, 3, 2, 67, 2)):
            G, A1, A2 = _inputs(rng, side, dims)
            assert _same_bits(_run(be, side, dims, G, A1, A2), _ref(side, dims, G, A1, A2, np.int64)), (tile, dims)
    finally:
        mk.backend.check(be.lib.mpsk_ctx_force_tile(be.ctx, 0, 0), "mpsk_ctx_force_tile")


@pytest.mark.parametrize("side", SIDES)
@pytest.mark.parametrize("dims", [CASES["three_slices"], CASES["full_tiles"], (70, 40, 37, 33, 50, 2)],
                         ids=["three_slices", "full_tiles", "several_k_tiles"])
def test_gaussian_and_determinism(be, dims, side):
    rng = np.random.default_rng(sum(dims))
    G, A1, A2 = _inputs(rng, side, dims, gauss=True)
    g1, g2 = _run(be, side, dims, G, A1, A2), _run(be, side, dims, G, A1, A2)
    assert _same_bits(g1, g2), "two runs of the same call differ"
    ref = _ref(side, dims, G, A1, A2, np.longdouble)
    bound = _bound(side, dims, G, A1, A2)
    err = np.abs(g1 - ref)
    print("max err / bound:", float(np.max(err / bound)))
    assert np.all(err <= bound)


@pytest.mark.parametrize("side", SIDES)
def test_error_paths_launch_nothing(be, side):
    dims = CASES["mixed_edges"]
    Dn, D1, D2, E1, E2, d = dims
    rng = np.random.default_rng(9)
    G, A1, A2 = _inputs(rng, side, dims)
    g, a1, a2 = be.upload(G), be.upload(A1), be.upload(A2)
    out, buf = _guarded(be, _shapes(side, dims)[1])
    code = {"left": 0, "right": 1}[side]

    def raw(**kw):
        p = dict(d=d, Dn=Dn, D1=D1, D2=D2, E1=E1, E2=E2, ldg=G.shape[0], A1=a1.ptr, out=out.ptr)
        p.update(kw)
        return be.lib.mpsk_dsum_site(be.ctx, code, p["d"], p["Dn"], p["D1"], p["D2"], p["E1"], p["E2"], g.ptr, p["ldg"],
                                     p["A1"], a2.ptr, p["out"])

    be._set_dtype(True)
    try:
        assert raw() == 3                                     # MPSK_ERR_UNSUPPORTED
        with pytest.raises(mk.MpskError, match="code 3"):
            be.dsum_site(side, g, a1, a2, out=out)
    finally:
        be._set_dtype(False)
    for name in ("d", "Dn", "D1", "D2", "E1", "E2"):
        assert raw(**{name: 0}) == 1, name                    # MPSK_ERR_INVALID
    assert raw(ldg=G.shape[0] - 1) == 1
    assert raw(out=a1.ptr) == 1                               # out aliases an operand
    assert be.lib.mpsk_dsum_site(be.ctx, 2, d, Dn, D1, D2, E1, E2, g.ptr, G.shape[0], a1.ptr, a2.ptr, out.ptr) == 1
    with pytest.raises(mk.MpskError):
        be.dsum_site(side, g, a1, be.upload(rng.standard_normal((D2, d + 1, E2))), out=out)
    be.synchronize()
    assert bool(torch.all(buf == SENTINEL)), "a refused call wrote to out"
    assert np.array_equal(be.download(a1), A1)
    assert raw() == 0                                         # and the same arguments, unchanged, are accepted
    be.synchronize()
    assert _same_bits(buf.cpu().numpy()[:out.size].reshape(out.shape, order="F"), _ref(side, dims, G, A1, A2, np.int64))
