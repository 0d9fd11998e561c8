"""Shared by the WindowMPS tests: uniform ground states to cut windows out of, and a NumPy restatement of the window
contractions that assumes nothing about the gauge of the tensors it is given."""
import numpy as np

import mpskit_jl_amd as mk

SZ = np.array([[0.5, 0.0], [0.0, -0.5]])
SP = np.array([[0.0, 1.0], [0.0, 0.0]])


def itfi_groundstate(be, D, n, g=1.5, tol=1e-11, maxiter=200):
    """(H, psi, envs, eps) of the transverse-field Ising chain in its gapped phase by VUMPS, unit cell n"""
    H = mk.transverse_field_ising(1.0, g, be=be)
    psi0 = mk.InfiniteMPS.random(2, D, np.random.default_rng(7), n=n, be=be)
    psi, envs, eps = mk.find_groundstate(psi0, H, mk.VUMPS(tol=tol, maxiter=maxiter))
    return H, psi, envs, eps


def heisenberg_groundstate(be, D, tol=1e-10, maxiter=300):
    """(H, psi, envs, eps) of the S = 1/2 Heisenberg chain by VUMPS on a two-site unit cell"""
    H = mk.heisenberg_XXX(0.5, be=be)
    psi0 = mk.InfiniteMPS.random(2, D, np.random.default_rng(3), n=2, be=be)
    psi, envs, eps = mk.find_groundstate(psi0, H, mk.VUMPS(tol=tol, maxiter=maxiter))
    return H, psi, envs, eps


def left_canonical_host(w):
    """host tensors whose product is the window's state (complex for a complex window)"""
    return [np.asarray(t) for t in w.to_host()]


def dense_site_matrices(bra, ket):
    """M_j[t,s] = <bra| (|t><s|)_j |ket> for two lists of host tensors [Dl, d, Dr] on the same (identity) edges: the whole
    network contracted around the open site, no canonical form assumed."""
    L = len(ket)
    lefts = [np.eye(bra[0].shape[0], ket[0].shape[0])]
    for j in range(L - 1):
        lefts.append(np.einsum("pa,asb,psq->qb", lefts[-1], ket[j], np.conj(bra[j])))
    rights = [None] * L
    rights[L - 1] = np.eye(ket[-1].shape[2], bra[-1].shape[2])
    for j in range(L - 1, 0, -1):
        rights[j - 1] = np.einsum("asb,bq,psq->ap", ket[j], rights[j], np.conj(bra[j]))
    return [np.einsum("ptq,pa,asb,bq->ts", np.conj(bra[j]), lefts[j], ket[j], rights[j]) for j in range(L)]


def apply_onsite(w, O, site):
    """the window with O applied at `site` (not normalised): host tensors -> a new window of the same kind or complex"""
    ts = left_canonical_host(w)
    ts[site] = np.einsum("ts,asb->atb", O, ts[site])
    return ts


def quench(be, D=16, L=8, site=4, steps=5, dt=0.05, gs_be=None):
    """S^+ applied at `site` of a window of the Heisenberg ground state, then real-time TDVP on an interleaved complex
    window.  Returns (|<w0|w(t)>| after every step, energy `tot` before the first and after every step).
    gs_be: a second host backend for the uniform ground state (the complex stand-in prepares complex operators only); its
    tensors are host buffers either way and are handed to `be` as they are."""
    from mpskit_jl_amd import window
    H, psi, envs, eps = heisenberg_groundstate(be if gs_be is None else gs_be, D)
    if gs_be is not None:
        psi = mk.InfiniteMPS(psi.AL, psi.AR, psi.CR, psi.AC, be)
        psi.cplx = False
        envs.be = be
        envs.dependency = psi
        H = mk.heisenberg_XXX(0.5, be=be)
    w = mk.WindowMPS(psi, L)
    w0 = mk.WindowMPS(psi, [t.astype(np.complex128) for t in apply_onsite(w, SP, site)]).normalize()
    wenvs = mk.environments(w0, H, envs, envs)
    tots = [mk.expectation_value(w0, H, wenvs)[1]]
    wt, overlaps = w0, []
    for n in range(steps):
        wt, wenvs = mk.timestep(wt, H, n * dt, dt, mk.TDVP(), wenvs)
        overlaps.append(abs(window.dot(w0, wt)))
        tots.append(mk.expectation_value(wt, H, wenvs)[1])
    return overlaps, tots


def dense_hac(be, sl, GL, GR):
    """the matrix of H_AC on vec(x[a,s,b]) (C order) from a host MPO slice and the device environments of its site:
    y[p,t,q] = sum GL_i[p,w,a] x[a,s,b] O_ij[w,t,s,v] GR_j[b,v,q] over the blocks (i, j) of the slice"""
    gl, gr = be._env(GL, sl.chil), be._env(GR, sl.chir)
    d = sl.d
    Dl, Dr = gl[0].shape[2], gr[0].shape[0]
    M = np.zeros((gl[0].shape[0], d, gr[0].shape[2], Dl, d, Dr))
    for (i, j), v in sl.blocks.items():
        O = v * np.eye(d)[None, :, :, None] if np.isscalar(v) else np.asarray(v)
        if O.ndim == 2:
            O = O[None, :, :, None]
        M += np.einsum("pwa,wtsv,bvq->ptqasb", gl[i], O, gr[j])
    n = Dl * d * Dr
    return M.reshape(-1, n)
