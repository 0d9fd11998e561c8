"""Dense restatement of one finite TDVP step with a time-dependent Hamiltonian H(t) = sum_k f_k(t) H_k (tdvp.jl:61-91),
written for the tests of the timed drivers and independent of the package's MPO / environment code: every effective
Hamiltonian is the explicit matrix P^+ H(t) P of the dense 2^L x 2^L Hamiltonian with the tangent-space isometry P built
from the state's own AL / AR tensors, and every local step is scipy.linalg.expm of that matrix.  Site 0 is the most
significant index of the state vector (the ordering of the oracle's mps_to_vector / dense_hamiltonian)."""
import numpy as np
import scipy.linalg as sla

# evaluation times in units of dt: AC and C on the way right, AC and C on the way back (integrators.jl:20-25: a sub-step
# from t0 by h evaluates its generator at t0 + h / 2)
OFFSETS = (0.25, -0.25, 0.75, 0.25)


def _left_iso(ALs, d):
    v = np.ones((1, 1), dtype=complex)
    for A in ALs:
        v = np.tensordot(v, A, axes=([1], [0])).reshape(-1, A.shape[2])
    return v                                   # (d^n, D)


def _right_iso(ARs):
    v = np.ones((1, 1), dtype=complex)
    for A in reversed(ARs):
        v = np.tensordot(A, v, axes=([2], [0])).reshape(A.shape[0], -1)
    return v                                   # (D, d^n)


def mps_vector(As):
    v = np.ones((1, 1), dtype=complex)
    for A in As:
        v = np.tensordot(v, np.asarray(A, dtype=complex), axes=([1], [0])).reshape(-1, A.shape[2])
    return v.reshape(-1)


def _ham(Hs, fs, te):
    return sum((f(te) if callable(f) else f) * np.asarray(H, dtype=complex) for f, H in zip(fs, Hs))


def tdvp_step_dense(As, Hs, fs, t, dt, offsets=OFFSETS, normalize=True):
    """One TDVP step of the MPS with site tensors As ([Dl, d, Dr], any gauge) under H(t) = sum_k fs[k](t) Hs[k] (dense
    matrices); dt may be complex (dt = -1j tau: imaginary time).  Returns the state vector after the step."""
    A = [np.asarray(a, dtype=complex) for a in As]
    L, d = len(A), A[0].shape[1]
    for i in range(L - 1, 0, -1):              # right-canonical form, centre on site 0
        Dl, _, Dr = A[i].shape
        Q, R = np.linalg.qr(A[i].reshape(Dl, d * Dr).conj().T)
        A[i] = Q.conj().T.reshape(-1, d, Dr)
        A[i - 1] = np.tensordot(A[i - 1], R.conj().T, axes=([2], [0]))
    if normalize:
        A[0] = A[0] / np.linalg.norm(A[0])
    a1, c1, a2, c2 = (t + o * dt for o in offsets)

    def hac(i, te):
        Lm, Rm = _left_iso(A[:i], d), _right_iso(A[i + 1:])
        P = np.einsum("al,st,rb->asbltr", Lm, np.eye(d), Rm)
        P = P.reshape(Lm.shape[0] * d * Rm.shape[1], Lm.shape[1] * d * Rm.shape[0])
        return P.conj().T @ _ham(Hs, fs, te) @ P

    def hc(i, te):                             # bond right of site i
        Lm, Rm = _left_iso(A[:i + 1], d), _right_iso(A[i + 1:])
        P = np.einsum("al,rb->ablr", Lm, Rm).reshape(Lm.shape[0] * Rm.shape[1], Lm.shape[1] * Rm.shape[0])
        return P.conj().T @ _ham(Hs, fs, te) @ P

    def evolve(M, x, z):
        return (sla.expm(z * M) @ x.reshape(-1)).reshape(x.shape)

    for i in range(L - 1):
        A[i] = evolve(hac(i, a1), A[i], -1j * dt / 2)
        Dl, _, Dr = A[i].shape
        Q, R = np.linalg.qr(A[i].reshape(Dl * d, Dr))
        A[i] = Q.reshape(Dl, d, -1)
        C = evolve(hc(i, c1), R, 1j * dt / 2)
        A[i + 1] = np.tensordot(C, A[i + 1], axes=([1], [0]))
    A[L - 1] = evolve(hac(L - 1, a1), A[L - 1], -1j * dt / 2)
    for i in range(L - 1, 0, -1):
        A[i] = evolve(hac(i, a2), A[i], -1j * dt / 2)
        Dl, _, Dr = A[i].shape
        Q, R = np.linalg.qr(A[i].reshape(Dl, d * Dr).conj().T)
        A[i] = Q.conj().T.reshape(-1, d, Dr)
        C = evolve(hc(i - 1, c2), R.conj().T, 1j * dt / 2)
        A[i - 1] = np.tensordot(A[i - 1], C, axes=([2], [0]))
    A[0] = evolve(hac(0, a2), A[0], -1j * dt / 2)
    return mps_vector(A)


def tdvp2_step_dense(As, Hs, fs, t, dt, offsets=OFFSETS, normalize=True):
    """One two-site TDVP step (tdvp.jl:113-146) without truncation: the two-site tensor is evolved forward by dt / 2 with the
    explicit P2^+ H(t) P2, split by an SVD that keeps everything, and the new centre is evolved backward with P^+ H(t) P.
    offsets: AC2 and AC on the way right, AC2 and AC on the way back, in units of dt.  Returns the state vector."""
    A = [np.asarray(a, dtype=complex) for a in As]
    L, d = len(A), A[0].shape[1]
    for i in range(L - 1, 0, -1):
        Dl, _, Dr = A[i].shape
        Q, R = np.linalg.qr(A[i].reshape(Dl, d * Dr).conj().T)
        A[i] = Q.conj().T.reshape(-1, d, Dr)
        A[i - 1] = np.tensordot(A[i - 1], R.conj().T, axes=([2], [0]))
    if normalize:
        A[0] = A[0] / np.linalg.norm(A[0])
    f2, f1, b2, b1 = (t + o * dt for o in offsets)

    def proj(nl, nr):                          # isometry of the block of sites [nl, nr) embedded in the chain
        Lm, Rm = _left_iso(A[:nl], d), _right_iso(A[nr:])
        k = d ** (nr - nl)
        P = np.einsum("al,st,rb->asbltr", Lm, np.eye(k), Rm)
        return P.reshape(Lm.shape[0] * k * Rm.shape[1], Lm.shape[1] * k * Rm.shape[0])

    def evolve(nl, nr, te, x, z):
        P = proj(nl, nr)
        M = P.conj().T @ _ham(Hs, fs, te) @ P
        return (sla.expm(z * M) @ x.reshape(-1)).reshape(x.shape)

    def split(theta):                          # theta [Dl, d, d, Dr] -> (u [Dl, d, k], s [k], vh [k, d, Dr])
        Dl, _, _, Dr = theta.shape
        u, s, vh = np.linalg.svd(theta.reshape(Dl * d, d * Dr), full_matrices=False)
        return u.reshape(Dl, d, -1), s, vh.reshape(-1, d, Dr)

    for i in range(L - 1):
        theta = np.tensordot(A[i], A[i + 1], axes=([2], [0]))
        u, s, vh = split(evolve(i, i + 2, f2, theta, -1j * dt / 2))
        A[i], A[i + 1] = u, s[:, None, None] * vh
        if i != L - 2:
            A[i + 1] = evolve(i + 1, i + 2, f1, A[i + 1], 1j * dt / 2)
    for i in range(L - 1, 0, -1):
        theta = np.tensordot(A[i - 1], A[i], axes=([2], [0]))
        u, s, vh = split(evolve(i - 1, i + 1, b2, theta, -1j * dt / 2))
        A[i - 1], A[i] = u * s[None, None, :], vh
        if i != 1:
            A[i - 1] = evolve(i - 1, i, b1, A[i - 1], 1j * dt / 2)
    return mps_vector(A)


def local_expm_step(apply, x, z):
    """exp(z M) x for the linear map `apply` on tensors of x's shape, with M assembled column by column (explicit matrix)."""
    n = x.size
    M = np.zeros((n, n), dtype=complex)
    for j in range(n):
        e = np.zeros(n)
        e[j] = 1.0
        M[:, j] = np.asarray(apply(e.reshape(x.shape))).reshape(-1)
    return (sla.expm(z * M) @ x.reshape(-1)).reshape(x.shape)
