"""Dense NumPy references for the local measurements (test_gpu_measure.py, test_measure_cpu.py): the state vector is
contracted from host tensors inside the tests; nothing here touches the package's routes."""
import numpy as np

SZ2 = np.diag([0.5, -0.5])
SP2 = np.array([[0.0, 1.0], [0.0, 0.0]])
SM2 = SP2.T.copy()
SX2 = 0.5 * (SP2 + SM2)
SY2 = -0.5j * (SP2 - SM2)

_r2 = np.sqrt(2.0)
SZ3 = np.diag([1.0, 0.0, -1.0])
SP3 = _r2 * np.array([[0.0, 1, 0], [0, 0, 1], [0, 0, 0]])
SM3 = SP3.T.copy()
SX3 = 0.5 * (SP3 + SM3)
SY3 = -0.5j * (SP3 - SM3)


def state_vector(tensors):
    """[A_1 .. A_L] with trivial outer bonds -> psi[s_1 .. s_L]"""
    v = np.asarray(tensors[0])
    for a in tensors[1:]:
        v = np.tensordot(v, np.asarray(a), axes=(v.ndim - 1, 0))
    return v.reshape(v.shape[1:-1])


def apply(v, O, i):
    """O[t,s] on site i"""
    return np.moveaxis(np.tensordot(O, v, axes=(1, i)), 0, i)


def ev1(v, O, i):
    return np.vdot(v, apply(v, O, i))


def ev2(v, A, i, B, j):
    return np.vdot(v, apply(apply(v, B, j), A, i))


def ev12(v, O12, i, j):
    """two-site operator O12[t1,t2,s1,s2] on sites i < j"""
    w = np.tensordot(O12, v, axes=((2, 3), (i, j)))
    return np.vdot(v, np.moveaxis(w, (0, 1), (i, j)))


def twosite(terms):
    """sum of A (x) B as O12[t1,t2,s1,s2]"""
    return sum(np.einsum("ab,cd->acbd", A, B) for A, B in terms)


def heisenberg_bond(d=2):
    sp, sm, sz = (SP2, SM2, SZ2) if d == 2 else (SP3, SM3, SZ3)
    return twosite([(0.5 * sp, sm), (0.5 * sm, sp), (sz, sz)])


def infinite_correlator(AC, AR, O1, O2, i, js):
    """<O1_i O2_j> of a uniform state from its own tensors (lists over the unit cell): plain transfer matrices"""
    n = len(AC)
    ac = AC[i % n]
    V = np.einsum("asb,ts,atq->qb", ac, O1, np.conj(ac))
    out, ctr = [], i + 1
    for j in js:
        for k in range(ctr, j):
            a = AR[k % n]
            V = np.einsum("pa,asb,psq->qb", V, a, np.conj(a))
        ctr = j
        a = AR[j % n]
        out.append(np.einsum("pa,asb,ts,ptb->", V, a, O2, np.conj(a)))
    return np.array(out)
