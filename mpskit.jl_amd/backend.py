"""Device plumbing above the C ABI: a context bound to a torch CUDA(HIP) device/stream, device
tensors (torch is used ONLY as the allocator / stream / collective provider -- all arithmetic is
libmpsk's hand-written HIP) and thin typed wrappers over the mpsk_* entry points.

Layout: every tensor is a flat fp64 torch tensor holding the column-major (TensorKit) data;
`DTensor.shape` carries the logical index order, e.g. (Dl, d, Dr).  Environments are stored as
(W, Dbra, Dket) = W column-major slabs (include/mpsk.h).
"""
from __future__ import annotations

import ctypes as C
import numpy as np

from . import _lib
from ._lib import MpskError, check


def _torch():
    import torch
    return torch


class DTensor:
    """Flat device buffer + logical column-major shape."""
    __slots__ = ("buf", "shape")

    def __init__(self, buf, shape):
        self.buf = buf
        self.shape = tuple(int(s) for s in shape)

    @property
    def ptr(self):
        return self.buf.data_ptr()

    @property
    def size(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    def reshape(self, *shape):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list)):
            shape = tuple(shape[0])
        t = DTensor(self.buf, shape)
        assert t.size == self.size, (self.shape, shape)
        return t


class Backend:
    """One mpsk_ctx on one GPU.  Raises MpskError when the HIP library or a GPU is missing."""

    def __init__(self, device=0, stream=None):
        """stream: a torch.cuda.Stream to bind (default: the calling thread's current torch stream).  Two Backends on
        two streams may be driven from two host threads at the same time (include/mpsk.h, thread-safety note)."""
        torch = _torch()
        if not torch.cuda.is_available():
            raise MpskError("no HIP device visible: the mpskit.jl_amd product path has no CPU fallback")
        self.lib = _lib.load()
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        h = C.c_void_p()
        check(self.lib.mpsk_ctx_create(device, C.byref(h)), "mpsk_ctx_create")
        self.ctx = h
        self.bind_stream(stream)

    def bind_stream(self, stream=None):
        torch = _torch()
        self.torch_stream = torch.cuda.current_stream(self.device) if stream is None else stream
        check(self.lib.mpsk_ctx_set_stream(self.ctx, C.c_void_p(self.torch_stream.cuda_stream)), "mpsk_ctx_set_stream")

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.mpsk_ctx_destroy(self.ctx)
            self.ctx = None

    def synchronize(self):
        check(self.lib.mpsk_ctx_synchronize(self.ctx), "mpsk_ctx_synchronize")

    def set_qr_mode(self, mode):
        check(self.lib.mpsk_ctx_set_qr_mode(self.ctx, int(mode)), "mpsk_ctx_set_qr_mode")

    def qr_retries(self) -> int:
        """CholeskyQR3 factorizations repeated with the published shift after a breakdown of the rounding-level one."""
        r = C.c_long(0)
        check(self.lib.mpsk_ctx_qr_retries(self.ctx, C.byref(r)), "mpsk_ctx_qr_retries")
        return r.value

    def qr_stats(self):
        a, b, f, r = C.c_long(), C.c_long(), C.c_long(), C.c_long()
        check(self.lib.mpsk_ctx_qr_stats(self.ctx, C.byref(a), C.byref(b), C.byref(f), C.byref(r)), "mpsk_ctx_qr_stats")
        return {"cholqr3": a.value, "householder": b.value, "fallback": f.value, "robust": r.value}

    def set_svd_mode(self, precondition=True):
        """0 / False: Jacobi on theta itself; 1 / True: QR-preconditioned; 2: QR + QR of R^T; 3: 2 + truncation-aware
        mpsk_tsplit (subspace iteration, checked; include/mpsk.h)."""
        check(self.lib.mpsk_ctx_set_svd_mode(self.ctx, int(precondition)), "mpsk_ctx_set_svd_mode")

    def svd_sweeps(self):
        n = C.c_int()
        check(self.lib.mpsk_ctx_svd_stats(self.ctx, C.byref(n)), "mpsk_ctx_svd_stats")
        return n.value

    def split_stats(self):
        """last mpsk_tsplit: {"path": 0 full iteration / 1 subspace stage accepted / 2 stage gave up, "iterations", "residual"}"""
        p, it, r = C.c_int(), C.c_int(), C.c_double()
        check(self.lib.mpsk_ctx_split_stats(self.ctx, C.byref(p), C.byref(it), C.byref(r)), "mpsk_ctx_split_stats")
        return {"path": p.value, "iterations": it.value, "residual": r.value}

    def prof_enable(self, on=True):
        check(self.lib.mpsk_prof_enable(self.ctx, int(on)), "mpsk_prof_enable")

    def prof_summary(self):
        import json
        buf = C.create_string_buffer(1 << 16)
        check(self.lib.mpsk_prof_summary(self.ctx, buf, len(buf)), "mpsk_prof_summary")
        return json.loads(buf.value.decode())

    # ---- memory ---------------------------------------------------------------------------
    def empty(self, *shape):
        torch = _torch()
        if len(shape) == 1 and isinstance(shape[0], (tuple, list)):
            shape = tuple(shape[0])
        n = 1
        for s in shape:
            n *= int(s)
        return DTensor(torch.empty(max(n, 1), dtype=torch.float64, device=self.device), shape)

    def zeros(self, *shape):
        t = self.empty(*shape)
        t.buf.zero_()
        return t

    def upload(self, a, shape=None):
        """host ndarray (logical index order) -> device column-major."""
        torch = _torch()
        a = np.asarray(a)
        if np.iscomplexobj(a):
            if np.abs(a.imag).max(initial=0.0) > 0:
                raise MpskError("complex128 tensors are not supported by the fp64 device path (MPSK_C128 reserved)")
            a = a.real
        a = np.ascontiguousarray(a, dtype=np.float64)
        flat = np.ravel(a, order="F")
        buf = torch.from_numpy(np.ascontiguousarray(flat)).to(self.device)
        if buf.numel() == 0:
            buf = torch.empty(1, dtype=torch.float64, device=self.device)
        return DTensor(buf, a.shape if shape is None else shape)

    def download(self, t: DTensor):
        flat = t.buf[: t.size].cpu().numpy()
        return flat.reshape(t.shape, order="F").copy()

    # ---- complex128 tensors: interleaved (re, im) = a REAL tensor whose first dimension is doubled ("half-embedded"
    # view, include/mpsk.h); the complex operator paths take such DTensors (flag cplx / a complex MPO slice)
    def upload_c(self, a):
        """complex ndarray (logical index order) -> device, interleaved complex128 column-major; shape (2 n0, n1, ...)."""
        torch = _torch()
        a = np.asarray(a, dtype=np.complex128)
        flat = np.ravel(a, order="F").view(np.float64)
        buf = torch.from_numpy(np.ascontiguousarray(flat)).to(self.device)
        return DTensor(buf, (2 * a.shape[0],) + tuple(a.shape[1:]))

    def download_c(self, t: DTensor):
        flat = t.buf[: t.size].cpu().numpy().view(np.complex128)
        return flat.reshape((t.shape[0] // 2,) + tuple(t.shape[1:]), order="F").copy()

    def upload_env_c(self, blocks):
        """complex env = list of [Dbra, chi_i, Dket] arrays -> device (W, 2 Dbra, Dket) interleaved slabs."""
        torch = _torch()
        slabs = [np.asarray(b, dtype=np.complex128)[:, k, :] for b in blocks for k in range(np.asarray(b).shape[1])]
        flat = np.concatenate([np.ravel(s_, order="F") for s_ in slabs]).view(np.float64)
        buf = torch.from_numpy(np.ascontiguousarray(flat)).to(self.device)
        return DTensor(buf, (len(slabs), 2 * slabs[0].shape[0], slabs[0].shape[1]))

    def download_env_c(self, t: DTensor, chis):
        W, Db2, Dk = t.shape
        flat = t.buf[: t.size].cpu().numpy().view(np.complex128)
        Db = Db2 // 2
        slabs = [flat[w * Db * Dk:(w + 1) * Db * Dk].reshape((Db, Dk), order="F") for w in range(W)]
        out, o = [], 0
        for chi in chis:
            out.append(np.stack(slabs[o:o + chi], axis=1))
            o += chi
        return out

    def _set_dtype(self, cplx):
        check(self.lib.mpsk_ctx_set_dtype(self.ctx, 1 if cplx else 0), "mpsk_ctx_set_dtype")

    def upload_env(self, blocks):
        """reference env = list of [Dbra, chi_i, Dket] arrays -> device (W, Dbra, Dket) slabs."""
        slabs = []
        for b in blocks:
            b = np.asarray(b)
            for k in range(b.shape[1]):
                slabs.append(b[:, k, :])
        return self._upload_slabs(slabs)

    def _upload_slabs(self, slabs):
        torch = _torch()
        flat = np.concatenate([np.ravel(np.asarray(s, dtype=np.float64), order="F") for s in slabs])
        buf = torch.from_numpy(flat).to(self.device)
        return DTensor(buf, (len(slabs),) + tuple(slabs[0].shape))

    def download_env(self, t: DTensor, chis):
        W, Db, Dk = t.shape
        flat = t.buf[: t.size].cpu().numpy()
        slabs = [flat[w * Db * Dk:(w + 1) * Db * Dk].reshape((Db, Dk), order="F") for w in range(W)]
        out, o = [], 0
        for chi in chis:
            out.append(np.stack(slabs[o:o + chi], axis=1))
            o += chi
        return out

    def copy(self, t: DTensor):
        return DTensor(t.buf.clone(), t.shape)

    # ---- MPO slices -----------------------------------------------------------------------
    def mposlice(self, odim, d, chil, chir, blocks, cplx=False):
        """blocks: {(i, j): scalar | ndarray [chi_i, d, d, chi_j]} (0-based levels).  cplx: an MPSK_C128 slice (complex
        entries allowed; every operand of a call that takes it is an interleaved complex128 tensor)."""
        return DeviceMPOSlice(self, odim, d, chil, chir, blocks, cplx=cplx)

    def mposlice_dense(self, O):
        """mpsk_mposlice_create_dense: one real DenseMPO tensor O[w, t(out), s(in), v] (densempo.jl:4-17) as a slice whose
        middle contraction runs as an fp64 MFMA GEMM (mpsk_hac_info mode 4 above the crossover)."""
        return DeviceDenseSlice(self, O)

    # ---- hot-path operators ----------------------------------------------------------------
    def dAC(self, H, GL: DTensor, GR: DTensor, x: DTensor, out: DTensor = None):
        if getattr(H, "cplx", False):          # interleaved complex128 operands: first dimensions are doubled
            Dl2x, d, Dr = x.shape
            Wl, Dlo2, Dl = GL.shape
            assert Dl2x == 2 * Dl and GR.shape == (H.Wr, 2 * Dr, Dr) and Wl == H.Wl and d == H.d, (GL.shape, GR.shape, x.shape)
            y = self.empty(Dlo2, d, Dr) if out is None else out
            check(self.lib.mpsk_dAC(self.ctx, H.handle, Dlo2 // 2, Dl, Dr, GL.ptr, GR.ptr, x.ptr, y.ptr), "mpsk_dAC")
            return y
        Dl, d, Dr = x.shape
        Wl, Dlo, Dl2 = GL.shape
        assert Dl2 == Dl and GR.shape == (H.Wr, Dr, Dr) and Wl == H.Wl and d == H.d, (GL.shape, GR.shape, x.shape)
        y = self.empty(Dlo, d, Dr) if out is None else out
        check(self.lib.mpsk_dAC(self.ctx, H.handle, Dlo, Dl, Dr, GL.ptr, GR.ptr, x.ptr, y.ptr), "mpsk_dAC")
        return y

    def dAC_blocked(self, H, GLrows: DTensor, GR: DTensor, xb: DTensor, nblk, out: DTensor = None):
        """mpsk_dAC_blocked: x in `nblk` row blocks (dist.to_blocked), GLrows = this rank's rows (W, Dlo, Dl);
        returns / fills y[Dlo, d, Dr] (the caller usually points `out` into the blocked destination vector)."""
        Dl, d, Dr = xb.shape
        Wl, Dlo, Dl2 = GLrows.shape
        assert Dl2 == Dl and GR.shape == (H.Wr, Dr, Dr) and Wl == H.Wl and d == H.d and Dl % nblk == 0
        y = self.empty(Dlo, d, Dr) if out is None else out
        check(self.lib.mpsk_dAC_blocked(self.ctx, H.handle, int(nblk), Dlo, Dl, Dr, GLrows.ptr, GR.ptr, xb.ptr, y.ptr),
              "mpsk_dAC_blocked")
        return y

    def hac_create(self, H, GL: DTensor, GR: DTensor):
        """mpsk_hac_create: the prepared effective Hamiltonian of one site (MPO_ddAC).  Returns a PreparedHAC that
        keeps GL / GR alive and releases the device-side object when it is garbage collected."""
        return PreparedHAC(self, H, GL, GR)

    def hac_create_ex(self, H, GL: DTensor, GR: DTensor, canonical: bool = False, canonical_c128: bool = False):
        """mpsk_hac_create_ex: as hac_create; canonical=True promises that level 0 of GL and level W-1 of GR are
        identities (MPSK_HAC_CANONICAL), which lets a real Jordan-form slice take the 16 D^3 operator (mode 3).
        canonical_c128=True (MPSK_HAC_CANONICAL_C128) asks for the same operator on a complex slice; the library checks
        the identities itself and keeps mode 2 when they do not hold."""
        return PreparedHAC(self, H, GL, GR, flags=(1 if canonical else 0) | (2 if canonical_c128 else 0))

    def hsum_create(self, Hs, GLs, GRs, canonical: bool = False, canonical_c128: bool = False):
        """mpsk_hsum_create: the prepared sum of n effective Hamiltonians of one site, y = sum_k coefs[k] H_k x.  Hs: the
        terms' slices, GLs / GRs their environments; the flags are those of hac_create_ex.  Returns a PreparedHSum."""
        return PreparedHSum(self, Hs, GLs, GRs, flags=(1 if canonical else 0) | (2 if canonical_c128 else 0))

    def dC(self, GL: DTensor, GR: DTensor, c: DTensor, out: DTensor = None, cplx=False):
        if cplx:
            Dl2, Dr = c.shape
            W, Dlo2, Dl = GL.shape
            assert Dl2 == 2 * Dl and GR.shape == (W, 2 * Dr, Dr)
            y = self.empty(Dlo2, Dr) if out is None else out
            self._set_dtype(True)
            try:
                check(self.lib.mpsk_dC(self.ctx, W, Dlo2 // 2, Dl, Dr, GL.ptr, GR.ptr, c.ptr, y.ptr), "mpsk_dC")
            finally:
                self._set_dtype(False)
            return y
        Dl, Dr = c.shape
        W, Dlo, _ = GL.shape
        assert GR.shape == (W, Dr, Dr)
        y = self.empty(Dlo, Dr) if out is None else out
        check(self.lib.mpsk_dC(self.ctx, W, Dlo, Dl, Dr, GL.ptr, GR.ptr, c.ptr, y.ptr), "mpsk_dC")
        return y

    def dAC2(self, H1, H2, GL: DTensor, GR: DTensor, x2: DTensor, out: DTensor = None):
        if getattr(H1, "cplx", False):
            Dl2, d1, Dr, d2 = x2.shape
            Wl, Dlo2, Dl = GL.shape
            assert Dl2 == 2 * Dl and GR.shape == (H2.Wr, 2 * Dr, Dr) and Wl == H1.Wl
            y = self.empty(Dlo2, d1, Dr, d2) if out is None else out
            check(self.lib.mpsk_dAC2(self.ctx, H1.handle, H2.handle, Dlo2 // 2, Dl, Dr, GL.ptr, GR.ptr, x2.ptr, y.ptr),
                  "mpsk_dAC2")
            return y
        Dl, d1, Dr, d2 = x2.shape
        Wl, Dlo, _ = GL.shape
        assert GR.shape == (H2.Wr, Dr, Dr) and Wl == H1.Wl
        y = self.empty(Dlo, d1, Dr, d2) if out is None else out
        check(self.lib.mpsk_dAC2(self.ctx, H1.handle, H2.handle, Dlo, Dl, Dr, GL.ptr, GR.ptr, x2.ptr, y.ptr),
              "mpsk_dAC2")
        return y

    def dAC2_product(self, H1, H2, GL: DTensor, GR: DTensor, AC: DTensor, AR: DTensor, out: DTensor = None):
        """mpsk_dAC2_product: H_AC2 applied to the product AC[a,s1,m] AR[m,s2,b], factorised through the middle bond
        (the two-site tensor is never formed).  Returns Y[Dl, d1, Dr, d2]."""
        Dl, d1, Dm = AC.shape
        Dm2, d2, Dr = AR.shape
        assert Dm2 == Dm and GL.shape == (H1.Wl, Dl, Dl) and GR.shape == (H2.Wr, Dr, Dr) and d1 == H1.d and d2 == H2.d, \
            (GL.shape, GR.shape, AC.shape, AR.shape)
        y = self.empty(Dl, d1, Dr, d2) if out is None else out
        check(self.lib.mpsk_dAC2_product(self.ctx, H1.handle, H2.handle, Dl, Dm, Dr, GL.ptr, GR.ptr, AC.ptr, AR.ptr, y.ptr),
              "mpsk_dAC2_product")
        return y

    def dAC_proj(self, H, GL: DTensor, GR: DTensor, x: DTensor, out: DTensor = None):
        """mpsk_dAC_proj (ac_proj): the matvec with rectangular environments, GL (Wl, Dlo, Dl) and GR (Wr, Dr, Dro); x is
        [Dl, d, Dr], the result [Dlo, d, Dro].  A complex slice takes interleaved operands (doubled first dimensions)."""
        m = 2 if getattr(H, "cplx", False) else 1
        Dlx, d, Dr = x.shape
        Wl, Dlo, Dl = GL.shape
        Wr, Dr2, Dro = GR.shape
        assert Dlx == m * Dl and Dr2 == m * Dr and Wl == H.Wl and Wr == H.Wr and d == H.d, (GL.shape, GR.shape, x.shape)
        y = self.empty(Dlo, d, Dro) if out is None else out
        check(self.lib.mpsk_dAC_proj(self.ctx, H.handle, Dlo // m, Dl, Dr, Dro, GL.ptr, GR.ptr, x.ptr, y.ptr), "mpsk_dAC_proj")
        return y

    # ---- quasiparticle excitations of a transfer matrix (qp_statmech.py).  The presence of these methods tells the host code
    # that the backend has the fused route; qp_calls counts the calls of each entry.
    def _qp_count(self, name):
        calls = self.__dict__.setdefault("qp_calls", {})
        calls[name] = calls.get(name, 0) + 1

    def qp_half(self, H, GL: DTensor, A: DTensor):
        """mpsk_qp_half: stages 1 and 2 of (GL, A) as an opaque device buffer for qp_apply (the B-independent third term)."""
        Wl, Dlo, Dl = GL.shape
        Dla, d, Dr2 = A.shape
        assert Dla == Dl and Wl == H.Wl and d == H.d, (GL.shape, A.shape)
        n = C.c_size_t()
        check(self.lib.mpsk_qp_half_size(H.handle, Dlo, Dr2, C.byref(n)), "mpsk_qp_half_size")
        half = self.empty(n.value)
        check(self.lib.mpsk_qp_half(self.ctx, H.handle, Dlo, Dl, Dr2, GL.ptr, A.ptr, half.ptr), "mpsk_qp_half")
        self._qp_count("qp_half")
        return half

    def qp_apply(self, H, GL: DTensor, GR: DTensor, B: DTensor, lB: DTensor = None, AR: DTensor = None, half: DTensor = None,
                 rB: DTensor = None, out: DTensor = None):
        """mpsk_qp_apply: proj(GL, GR; B) + proj(lB, GR; AR) + half rB, with GL (Wl, Dlo, Dl), GR (Wr, Dr, Dro), B [Dl, d, Dr],
        lB (Wl, Dlo, Dl2), AR [Dl2, d, Dr], half from qp_half(H, GL, AL [Dl, d, Dr2]), rB (Wr, Dr2, Dro).  Either pair may be
        None."""
        Wl, Dlo, Dl = GL.shape
        Wr, Dr, Dro = GR.shape
        assert B.shape == (Dl, H.d, Dr) and Wl == H.Wl and Wr == H.Wr, (GL.shape, GR.shape, B.shape)
        assert (lB is None) == (AR is None) and (half is None) == (rB is None)
        Dl2 = Dr2 = 0
        if lB is not None:
            Dl2 = lB.shape[2]
            assert lB.shape == (Wl, Dlo, Dl2) and AR.shape == (Dl2, H.d, Dr), (lB.shape, AR.shape)
        if rB is not None:
            Dr2 = rB.shape[1]
            assert rB.shape == (Wr, Dr2, Dro) and half.size == Wr * H.d * Dlo * Dr2, (rB.shape, half.shape)
        y = self.empty(Dlo, H.d, Dro) if out is None else out
        nul = lambda t: None if t is None else t.ptr
        check(self.lib.mpsk_qp_apply(self.ctx, H.handle, Dlo, Dl, Dl2, Dr, Dr2, Dro, GL.ptr, GR.ptr, B.ptr, nul(lB), nul(AR),
                                     nul(half), nul(rB), y.ptr), "mpsk_qp_apply")
        self._qp_count("qp_apply")
        return y

    def transfer_left_pair(self, H, V1: DTensor, A1: DTensor, V2: DTensor, A2: DTensor, Ab: DTensor, out: DTensor = None):
        """mpsk_transfer_left_pair: transfer_left(H, V1, A1, Ab) + transfer_left(H, V2, A2, Ab), stages 2 and 3 once."""
        Dl1, d, Dr = A1.shape
        Dl2 = A2.shape[0]
        Dlb, _, Drb = Ab.shape
        assert V1.shape == (H.Wl, Dlb, Dl1) and V2.shape == (H.Wl, Dlb, Dl2) and A2.shape == (Dl2, d, Dr) and d == H.d, \
            (V1.shape, A1.shape, V2.shape, A2.shape, Ab.shape)
        y = self.empty(H.Wr, Drb, Dr) if out is None else out
        check(self.lib.mpsk_transfer_left_pair(self.ctx, H.handle, Dl1, Dl2, Dr, Dlb, Drb, V1.ptr, A1.ptr, V2.ptr, A2.ptr, Ab.ptr,
                                               y.ptr), "mpsk_transfer_left_pair")
        self._qp_count("transfer_left_pair")
        return y

    def transfer_right_pair(self, H, V1: DTensor, A1: DTensor, V2: DTensor, A2: DTensor, Ab: DTensor, out: DTensor = None):
        """mpsk_transfer_right_pair: transfer_right(H, V1, A1, Ab) + transfer_right(H, V2, A2, Ab), stages 2 and 3 once."""
        Dl, d, Dr1 = A1.shape
        Dr2 = A2.shape[2]
        Dlb, _, Drb = Ab.shape
        assert V1.shape == (H.Wr, Dr1, Drb) and V2.shape == (H.Wr, Dr2, Drb) and A2.shape == (Dl, d, Dr2) and d == H.d, \
            (V1.shape, A1.shape, V2.shape, A2.shape, Ab.shape)
        y = self.empty(H.Wl, Dl, Dlb) if out is None else out
        check(self.lib.mpsk_transfer_right_pair(self.ctx, H.handle, Dl, Dr1, Dr2, Dlb, Drb, A1.ptr, V1.ptr, A2.ptr, V2.ptr, Ab.ptr,
                                                y.ptr), "mpsk_transfer_right_pair")
        self._qp_count("transfer_right_pair")
        return y

    # ---- quasiparticle excitations of a Hamiltonian (quasiparticle.py, susceptibility.py)
    @property
    def has_qp_heff(self):
        """True when the loaded library exports mpsk_qp_heff_site; the host code takes the composed route otherwise."""
        return hasattr(self.lib, "mpsk_qp_heff_site")

    def qp_heff_site(self, H, GL: DTensor, GR: DTensor, VL: DTensor, X: DTensor, E, lB: DTensor = None, AR: DTensor = None,
                     half: DTensor = None, rB: DTensor = None, out: DTensor = None):
        """mpsk_qp_heff_site: VL^T qp_apply(GL, GR, VL X, lB, AR, half, rB) - E X for one site and one real part, with GL
        (Wl, Dl, Dl), GR (Wr, Dr, Dr), VL [Dl d, n], X [n, Dr]; lB (Wl, Dl, Dl2), AR [Dl2, d, Dr], half from
        qp_half(H, GL, AL), rB (Wr, Dr2, Dr).  Either pair may be None.  out must not alias X; an empty complement (n = 0)
        returns out untouched."""
        if not self.has_qp_heff:
            raise MpskError("this libmpsk has no mpsk_qp_heff_site: rebuild it")
        Wl, Dl, Dl_ = GL.shape
        Wr, Dr, Dr_ = GR.shape
        rows, n = VL.shape
        d = H.d
        assert Dl_ == Dl and Dr_ == Dr and rows == Dl * d and X.shape == (n, Dr) and Wl == H.Wl and Wr == H.Wr, \
            (GL.shape, GR.shape, VL.shape, X.shape)
        assert (lB is None) == (AR is None) and (half is None) == (rB is None)
        Dl2 = Dr2 = 0
        if lB is not None:
            Dl2 = lB.shape[2]
            assert lB.shape == (Wl, Dl, Dl2) and AR.shape == (Dl2, d, Dr), (lB.shape, AR.shape)
        if rB is not None:
            Dr2 = rB.shape[1]
            assert rB.shape == (Wr, Dr2, Dr) and half.size == Wr * d * Dl * Dr2, (rB.shape, half.shape)
        y = self.empty(n, Dr) if out is None else out
        assert y.shape == (n, Dr) and (n == 0 or y.ptr != X.ptr), "out must be [n, Dr] and must not alias X"
        nul = lambda t: None if t is None else t.ptr
        check(self.lib.mpsk_qp_heff_site(self.ctx, H.handle, Dl, rows - n, Dr, Dl2, Dr2, GL.ptr, GR.ptr, VL.ptr, X.ptr, float(E),
                                         nul(lB), nul(AR), nul(half), nul(rB), y.ptr), "mpsk_qp_heff_site")
        self._qp_count("qp_heff_site")
        return y

    def dC_proj(self, GL: DTensor, GR: DTensor, c: DTensor, out: DTensor = None):
        """mpsk_dC_proj (c_proj): the zero-site map with rectangular environments, GL (W, Dlo, Dl) and GR (W, Dr, Dro); c is
        [Dl, Dr], the result [Dlo, Dro].  Real fp64 only."""
        Dl, Dr = c.shape
        W, Dlo, Dl2 = GL.shape
        W2, Dr2, Dro = GR.shape
        assert W2 == W and Dl2 == Dl and Dr2 == Dr, (GL.shape, GR.shape, c.shape)
        y = self.empty(Dlo, Dro) if out is None else out
        check(self.lib.mpsk_dC_proj(self.ctx, W, Dlo, Dl, Dr, Dro, GL.ptr, GR.ptr, c.ptr, y.ptr), "mpsk_dC_proj")
        return y

    def dC_proj_c(self, GL: DTensor, GR: DTensor, c: DTensor, out: DTensor = None):
        """mpsk_dC_proj_c (c_proj on interleaved complex128): GL (W, 2 Dlo, Dl), GR (W, 2 Dr, Dro), c (2 Dl, Dr); the result is
        (2 Dlo, Dro).  Nothing is conjugated; asynchronous."""
        Dl2, Dr = c.shape
        W, Dlo2, Dl = GL.shape
        W2, Dr2, Dro = GR.shape
        assert W2 == W and Dl2 == 2 * Dl and Dr2 == 2 * Dr, (GL.shape, GR.shape, c.shape)
        y = self.empty(Dlo2, Dro) if out is None else out
        self._set_dtype(True)
        try:
            check(self.lib.mpsk_dC_proj_c(self.ctx, W, Dlo2 // 2, Dl, Dr, Dro, GL.ptr, GR.ptr, c.ptr, y.ptr), "mpsk_dC_proj_c")
        finally:
            self._set_dtype(False)
        return y

    def split_c(self, z: DTensor, out: DTensor = None):
        """mpsk_vsplit_c: interleaved complex tensor (z.size doubles) -> planar vector [Re | Im] of the same length."""
        p = self.empty(z.size) if out is None else out
        check(self.lib.mpsk_vsplit_c(self.ctx, z.size // 2, z.ptr, p.ptr), "mpsk_vsplit_c")
        return p

    def join_c(self, p: DTensor, shape, out: DTensor = None):
        """mpsk_vjoin_c: planar vector [Re | Im] -> interleaved complex tensor of `shape` (first dimension doubled)."""
        z = self.empty(*shape) if out is None else out
        check(self.lib.mpsk_vjoin_c(self.ctx, p.size // 2, p.ptr, z.ptr), "mpsk_vjoin_c")
        return z

    def dAC2_proj(self, H1, H2, GL: DTensor, GR: DTensor, AC: DTensor, AR: DTensor, out: DTensor = None):
        """mpsk_dAC2_proj (ac2_proj) on the two factors of the state above, AC [Dl, d1, Dm] and AR [Dm, d2, Dr], with
        GL (Wl, Dlo, Dl) and GR (Wr, Dr, Dro).  Returns Y[Dlo, d1, Dro, d2]; the two-site tensor is not formed (fp64)."""
        m = 2 if getattr(H1, "cplx", False) else 1
        Dlx, d1, Dm = AC.shape
        Dmx, d2, Dr = AR.shape
        Wl, Dlo, Dl = GL.shape
        Wr, Dr2, Dro = GR.shape
        assert (Dlx == m * Dl and Dmx == m * Dm and Dr2 == m * Dr and Wl == H1.Wl and Wr == H2.Wr and d1 == H1.d
                and d2 == H2.d), (GL.shape, GR.shape, AC.shape, AR.shape)
        y = self.empty(Dlo, d1, Dro, d2) if out is None else out
        check(self.lib.mpsk_dAC2_proj(self.ctx, H1.handle, H2.handle, Dlo // m, Dl, Dm, Dr, Dro, GL.ptr, GR.ptr, AC.ptr,
                                      AR.ptr, y.ptr), "mpsk_dAC2_proj")
        return y

    def complement_tsvd(self, Y: DTensor, QL: DTensor, QR: DTensor, k: int):
        """mpsk_complement_tsvd: the k leading singular triplets of (1 - QL QL^T) Y (1 - QR^T QR); Y (m, n), QL (m, pl)
        with orthonormal columns or None, QR (pr, n) with orthonormal rows or None.  Returns (U (m, kept), S (kept,),
        Vt (kept, n), kept); kept = 0: (None, None, None, 0)."""
        m, n = Y.shape
        pl = 0 if QL is None else QL.shape[1]
        pr = 0 if QR is None else QR.shape[0]
        kk = max(0, min(int(k), m - pl, n - pr))
        U, S, Vt = self.empty(m, kk), self.empty(kk), self.empty(kk, n)
        kept = C.c_int(-1)
        check(self.lib.mpsk_complement_tsvd(self.ctx, m, n, Y.ptr, m, None if QL is None else QL.ptr, m, pl,
                                            None if QR is None else QR.ptr, max(pr, 1), pr, int(k), U.ptr, m, S.ptr, Vt.ptr,
                                            max(kk, 1), C.byref(kept)), "mpsk_complement_tsvd")
        assert kept.value == kk, (kept.value, kk)
        if kk == 0:
            return None, None, None, 0
        return U, S, Vt, kk

    def complement_tsvd_c(self, Y: DTensor, QL: DTensor, QR: DTensor, k: int):
        """mpsk_complement_tsvd under MPSK_C128: the k leading singular triplets of (1 - QL QL^H) Y (1 - QR^H QR) on interleaved
        complex128 matrices; Y (2 m, n), QL (2 m, pl) with orthonormal columns or None, QR (2 pr, n) with orthonormal rows or
        None.  Returns (U (2 m, kept), S (kept,) real, Vt (2 kept, n), kept); kept = 0: (None, None, None, 0)."""
        m2, n = Y.shape
        m = m2 // 2
        assert m2 == 2 * m
        pl = 0 if QL is None else QL.shape[1]
        pr = 0 if QR is None else QR.shape[0] // 2
        kk = max(0, min(int(k), m - pl, n - pr))
        U, S, Vt = self.empty(m2, kk), self.empty(kk), self.empty(2 * kk, n)
        kept = C.c_int(-1)
        self._set_dtype(True)
        try:
            check(self.lib.mpsk_complement_tsvd(self.ctx, m, n, Y.ptr, m, None if QL is None else QL.ptr, m, pl,
                                                None if QR is None else QR.ptr, max(pr, 1), pr, int(k), U.ptr, m, S.ptr,
                                                Vt.ptr, max(kk, 1), C.byref(kept)), "mpsk_complement_tsvd (C128)")
        finally:
            self._set_dtype(False)
        assert kept.value == kk, (kept.value, kk)
        if kk == 0:
            return None, None, None, 0
        return U, S, Vt, kk

    def complement_stats(self):
        """mpsk_complement_tsvd calls: {"calls", "subspace" (answered by the accepted subspace stage), "full" (all others: full
        iteration of the split, mpsk_tsvd of a small X, X = 0)}"""
        a, b, c = C.c_long(), C.c_long(), C.c_long()
        check(self.lib.mpsk_ctx_complement_stats(self.ctx, C.byref(a), C.byref(b), C.byref(c)), "mpsk_ctx_complement_stats")
        return {"calls": a.value, "subspace": b.value, "full": c.value}

    def transfer_stats(self):
        """{"pair": canonical transfers of this ctx that took the pair-Gram route} (mpsk_ctx_transfer_stats)"""
        a = C.c_long()
        check(self.lib.mpsk_ctx_transfer_stats(self.ctx, C.byref(a)), "mpsk_ctx_transfer_stats")
        return {"pair": a.value}

    def transfer_left(self, H, GLin: DTensor, A: DTensor, Ab: DTensor, out: DTensor = None, cplx=False, canonical=False):
        """mpsk_transfer_left; canonical=True promises that level 0 of GLin is the identity and that A (== Ab) is a left
        isometry (MPSK_TRANSFER_CANONICAL): a real Jordan-form slice then takes the 24 D^3 route of mpsk_transfer_left_ex."""
        if cplx or getattr(H, "cplx", False):
            Dl, d, Dr = A.shape[0] // 2, A.shape[1], A.shape[2]
            Dlb, Drb = Ab.shape[0] // 2, Ab.shape[2]
            W = GLin.shape[0]
            Wout = H.Wr if H is not None else W
            y = self.empty(Wout, 2 * Drb, Dr) if out is None else out
            if H is None:
                self._set_dtype(True)
            try:
                check(self.lib.mpsk_transfer_left(self.ctx, H.handle if H is not None else None, W, d, Dl, Dr, Dlb, Drb,
                                                  GLin.ptr, A.ptr, Ab.ptr, y.ptr), "mpsk_transfer_left")
            finally:
                if H is None:
                    self._set_dtype(False)
            return y
        Dl, d, Dr = A.shape
        Dlb, _, Drb = Ab.shape
        W = GLin.shape[0]
        Wout = H.Wr if H is not None else W
        y = self.empty(Wout, Drb, Dr) if out is None else out
        if canonical and H is not None:
            check(self.lib.mpsk_transfer_left_ex(self.ctx, H.handle, W, d, Dl, Dr, Dlb, Drb, GLin.ptr, A.ptr, Ab.ptr, 1, y.ptr),
                  "mpsk_transfer_left_ex")
            return y
        check(self.lib.mpsk_transfer_left(self.ctx, H.handle if H is not None else None, W, d, Dl, Dr, Dlb, Drb,
                                          GLin.ptr, A.ptr, Ab.ptr, y.ptr), "mpsk_transfer_left")
        return y

    # ---- local measurements (measure.py): the presence of these two methods tells the host code that the backend has the
    # fused device route.  Gram results are slabs like an environment: W column-major d x d matrices (t fastest), shape
    # (W, d, d), or (W, 2 d, d) interleaved for complex tensors; they stay on the device.
    def site_gram(self, X: DTensor, Ab: DTensor, out: DTensor = None, cplx=False):
        """mpsk_site_gram: out[w][t,s] = sum_{p,b} conj(Ab[p,t,b]) X[w][p,s,b].  X: [Dl,d,Dr] or W of them as
        (W, Dl, d, Dr) slabs; asynchronous."""
        c = 2 if cplx else 1
        Dl, d, Dr = Ab.shape[0] // c, Ab.shape[1], Ab.shape[2]
        W = X.size // Ab.size
        if W < 1 or W * Ab.size != X.size:
            raise MpskError(f"site_gram: X {X.shape} is not a whole number of tensors of the shape of Ab {Ab.shape}")
        g = self.empty(W, c * d, d) if out is None else out
        if g.size != W * c * d * d:
            raise MpskError(f"site_gram: out {g.shape} does not hold {W} matrices {c * d} x {d}")
        self._set_dtype(cplx)
        try:
            check(self.lib.mpsk_site_gram(self.ctx, W, d, Dl, Dr, X.ptr, Ab.ptr, g.ptr), "mpsk_site_gram")
        finally:
            self._set_dtype(False)
        return g

    def transfer_left_gram(self, Vin: DTensor, A: DTensor, Ab: DTensor, gram_out: DTensor, out: DTensor = None, last=False,
                           cplx=False):
        """mpsk_transfer_left_gram: the pass-through transfer_left(None, Vin, A, Ab) plus gram_out[w][t,s] =
        sum Vin[w][p,a] A[a,s,b] conj(Ab[p,t,b]) from its intermediate.  gram_out: a view into a caller-owned buffer (a whole
        range is downloaded once).  last=True: last site of a range, nothing is transferred and None is returned."""
        c = 2 if cplx else 1
        Dl, d, Dr = A.shape[0] // c, A.shape[1], A.shape[2]
        Dlb, Drb = Ab.shape[0] // c, Ab.shape[2]
        W = Vin.shape[0]
        if gram_out.size != W * c * d * d:
            raise MpskError(f"transfer_left_gram: gram_out {gram_out.shape} does not hold {W} matrices {c * d} x {d}")
        y = None if last else (self.empty(W, c * Drb, Dr) if out is None else out)
        self._set_dtype(cplx)
        try:
            check(self.lib.mpsk_transfer_left_gram(self.ctx, W, d, Dl, Dr, Dlb, Drb, Vin.ptr, A.ptr, Ab.ptr,
                                                   None if last else y.ptr, gram_out.ptr), "mpsk_transfer_left_gram")
        finally:
            self._set_dtype(False)
        return y

    def transfer_left_gram_env(self, Lin: DTensor, A: DTensor, Ab: DTensor, R: DTensor, gram_out: DTensor,
                               out: DTensor = None, last=False, cplx=False):
        """mpsk_transfer_left_gram_env: the pass-through transfer_left(None, Lin, A, Ab) of one slab plus gram_out[t,s] =
        sum conj(Ab[p,t,q]) Lin[p,a] A[a,s,b] R[b,q], closed on the right with R [Dr, Drb].  gram_out: a view into a
        caller-owned buffer.  last=True: nothing is transferred and None is returned."""
        c = 2 if cplx else 1
        Dl, d, Dr = A.shape[0] // c, A.shape[1], A.shape[2]
        Dlb, Drb = Ab.shape[0] // c, Ab.shape[2]
        if Lin.size != c * Dlb * Dl or R.size != c * Dr * Drb or Ab.shape[1] != d:
            raise MpskError(f"transfer_left_gram_env: Lin {Lin.shape} / R {R.shape} do not fit A {A.shape}, Ab {Ab.shape}")
        if gram_out.size != c * d * d:
            raise MpskError(f"transfer_left_gram_env: gram_out {gram_out.shape} does not hold a matrix {c * d} x {d}")
        y = None if last else (self.empty(1, c * Drb, Dr) if out is None else out)
        self._set_dtype(cplx)
        try:
            check(self.lib.mpsk_transfer_left_gram_env(self.ctx, d, Dl, Dr, Dlb, Drb, Lin.ptr, A.ptr, Ab.ptr, R.ptr,
                                                       None if last else y.ptr, gram_out.ptr), "mpsk_transfer_left_gram_env")
        finally:
            self._set_dtype(False)
        return y

    def transfer_left_ex(self, H, GLin: DTensor, A: DTensor, Ab: DTensor, canonical: bool = False, out: DTensor = None):
        """mpsk_transfer_left_ex (real tensors); its presence tells FinEnv that the backend has the canonical route."""
        return self.transfer_left(H, GLin, A, Ab, out=out, canonical=canonical)

    def transfer_right_ex(self, H, GRin: DTensor, A: DTensor, Ab: DTensor, canonical: bool = False, out: DTensor = None):
        return self.transfer_right(H, GRin, A, Ab, out=out, canonical=canonical)

    def transfer_right(self, H, GRin: DTensor, A: DTensor, Ab: DTensor, out: DTensor = None, cplx=False, canonical=False):
        """mpsk_transfer_right; canonical=True: level W-1 of GRin is the identity and A (== Ab) is a right isometry."""
        if cplx or getattr(H, "cplx", False):
            Dl, d, Dr = A.shape[0] // 2, A.shape[1], A.shape[2]
            Dlb, Drb = Ab.shape[0] // 2, Ab.shape[2]
            W = GRin.shape[0]
            Wout = H.Wl if H is not None else W
            y = self.empty(Wout, 2 * Dl, Dlb) if out is None else out
            if H is None:
                self._set_dtype(True)
            try:
                check(self.lib.mpsk_transfer_right(self.ctx, H.handle if H is not None else None, W, d, Dl, Dr, Dlb, Drb,
                                                   A.ptr, Ab.ptr, GRin.ptr, y.ptr), "mpsk_transfer_right")
            finally:
                if H is None:
                    self._set_dtype(False)
            return y
        Dl, d, Dr = A.shape
        Dlb, _, Drb = Ab.shape
        W = GRin.shape[0]
        Wout = H.Wl if H is not None else W
        y = self.empty(Wout, Dl, Dlb) if out is None else out
        if canonical and H is not None:
            check(self.lib.mpsk_transfer_right_ex(self.ctx, H.handle, W, d, Dl, Dr, Dlb, Drb, A.ptr, Ab.ptr, GRin.ptr, 1, y.ptr),
                  "mpsk_transfer_right_ex")
            return y
        check(self.lib.mpsk_transfer_right(self.ctx, H.handle if H is not None else None, W, d, Dl, Dr, Dlb, Drb,
                                           A.ptr, Ab.ptr, GRin.ptr, y.ptr), "mpsk_transfer_right")
        return y

    def regularize(self, v: DTensor, lvec: DTensor, rvec: DTensor):
        W, D1, D2 = v.shape
        check(self.lib.mpsk_regularize(self.ctx, W, D1, D2, v.ptr, lvec.ptr, rvec.ptr), "mpsk_regularize")
        return v

    def regularize_axpby(self, y: DTensor, lvec: DTensor, rvec: DTensor, a1=1.0, x: DTensor = None, a0=0.0,
                         out: DTensor = None, cplx=False):
        """mpsk_regularize_axpby: out[w] = a0 x[w] + a1 (y[w] - <lvec^T, y[w]> rvec), bilinear, W slabs (W, D1, D2) -- cplx:
        interleaved (W, 2 D1, D2).  x=None drops the a0 term; out may be y or x (default: a new tensor); asynchronous."""
        m = 2 if cplx else 1
        W, D1, D2 = y.shape[0], y.shape[1] // m, y.shape[2]
        if lvec.size != m * D1 * D2 or rvec.size != m * D1 * D2 or (x is not None and x.size != y.size):
            raise MpskError(f"regularize_axpby: lvec {lvec.shape} / rvec {rvec.shape} / x do not fit y {y.shape}")
        o = self.empty(*y.shape) if out is None else out
        if o.size != y.size:
            raise MpskError(f"regularize_axpby: out {o.shape} does not fit y {y.shape}")
        self._set_dtype(cplx)
        try:
            check(self.lib.mpsk_regularize_axpby(self.ctx, W, D1, D2, y.ptr, lvec.ptr, rvec.ptr, float(a1),
                                                 None if x is None else x.ptr, float(a0), o.ptr), "mpsk_regularize_axpby")
        finally:
            self._set_dtype(False)
        return o

    def gemm(self, A: DTensor, B: DTensor, transA=False, transB=False, alpha=1.0, beta=0.0, out: DTensor = None,
             m=None, n=None, k=None, lda=None, ldb=None, ldc=None):
        """C = alpha op(A) op(B) + beta C on 2-D column-major views (leading dims default to rows)."""
        ar, ac = A.shape
        br, bc = B.shape
        M = (ac if transA else ar) if m is None else m
        K = (ar if transA else ac) if k is None else k
        N = (br if transB else bc) if n is None else n
        c = self.empty(M, N) if out is None else out
        check(self.lib.mpsk_gemm(self.ctx, int(transA), int(transB), M, N, K, float(alpha), A.ptr,
                                 ar if lda is None else lda, B.ptr, br if ldb is None else ldb, float(beta),
                                 c.ptr, M if ldc is None else ldc), "mpsk_gemm")
        return c

    def gemm_raw(self, transA, transB, M, N, K, alpha, a_ptr, lda, b_ptr, ldb, beta, c_ptr, ldc):
        check(self.lib.mpsk_gemm(self.ctx, int(transA), int(transB), M, N, K, float(alpha), a_ptr, lda, b_ptr,
                                 ldb, float(beta), c_ptr, ldc), "mpsk_gemm")

    def gemm_pair(self, P: DTensor, Q, B: DTensor, coef: DTensor, out1: DTensor = None, out2: DTensor = None, beta1=0.0,
                  beta2=0.0, two=True):
        """mpsk_gemm_pair: out1 = beta1 out1 + (P diag(a1) + Q diag(b1)) B and, with two=True, out2 likewise from rows
        a2 / b2 of coef (grassmann_coef: (K, 4) column-major, column r = row r of the ABI).  P, Q: (M, K), B: (K, N); Q may be None.  Returns (out1, out2 | None)."""
        M, K = P.shape
        K2, N = B.shape
        assert K2 == K and coef.shape == (K, 4) and (Q is None or Q.shape == (M, K)), (P.shape, B.shape, coef.shape)
        o1 = self.empty(M, N) if out1 is None else out1
        o2 = (self.empty(M, N) if out2 is None else out2) if two else None
        check(self.lib.mpsk_gemm_pair(self.ctx, M, N, K, P.ptr, M, None if Q is None else Q.ptr, M, B.ptr, K, coef.ptr, K,
                                      float(beta1), o1.ptr, M, float(beta2), None if o2 is None else o2.ptr, M),
              "mpsk_gemm_pair")
        return o1, o2

    def gemm_pair_raw(self, M, N, K, p_ptr, ldp, q_ptr, ldq, b_ptr, ldb, coef_ptr, ldcoef, beta1, o1_ptr, ld1, beta2, o2_ptr,
                      ld2):
        check(self.lib.mpsk_gemm_pair(self.ctx, M, N, K, p_ptr, ldp, q_ptr, ldq, b_ptr, ldb, coef_ptr, ldcoef, float(beta1),
                                      o1_ptr, ld1, float(beta2), o2_ptr, ld2), "mpsk_gemm_pair")

    DSUM_SIDES = {"left": 0, "right": 1}

    def dsum_site(self, side, G: DTensor, A1: DTensor, A2: DTensor, out: DTensor = None, ldg=None):
        """mpsk_dsum_site: the site step of FiniteMPS + FiniteMPS in one launch.  A1: (D1, d, E1), A2: (D2, d, E2).
        side "left":  G (Dn, D1 + D2) -> out (Dn, d, E1 + E2), out[:, :, :E1] = G[:, :D1] A1, out[:, :, E1:] = G[:, D1:] A2;
        side "right": G (E1 + E2, Dn) -> out (D1 + D2, d, Dn), out[:D1, s, :] = A1[:, s, :] G[:E1, :] and
        out[D1:, s, :] = A2[:, s, :] G[E1:, :].  ldg: leading dimension of G when it is a view of a taller matrix."""
        D1, d, E1 = A1.shape
        D2, d2, E2 = A2.shape
        gr, gc = G.shape
        left = self.DSUM_SIDES[side] == 0
        Dn = gr if left else gc
        if d2 != d or (gc if left else gr) != (D1 + D2 if left else E1 + E2):
            raise MpskError(f"dsum_site ({side}): G {G.shape} does not match the site tensors {A1.shape}, {A2.shape}")
        shape = (Dn, d, E1 + E2) if left else (D1 + D2, d, Dn)
        o = self.empty(*shape) if out is None else out
        if o.shape != shape:
            raise MpskError(f"dsum_site ({side}): out {o.shape} is not {shape}")
        check(self.lib.mpsk_dsum_site(self.ctx, self.DSUM_SIDES[side], d, Dn, D1, D2, E1, E2, G.ptr, gr if ldg is None else ldg,
                                      A1.ptr, A2.ptr, o.ptr), "mpsk_dsum_site")
        return o

    GRASSMANN_MODES = {"retract": 0, "transport": 1, "precondition": 2}

    def grassmann_coef(self, S: DTensor, scalar, mode, out: DTensor = None):
        """mpsk_grassmann_coef: the coefficient rows a1, b1, a2, b2 of gemm_pair (the columns of a (K, 4) tensor) from the
        device vector S and one host scalar (alpha, or delta for "precondition"); no device-to-host copy."""
        K = S.size
        coef = self.empty(K, 4) if out is None else out
        check(self.lib.mpsk_grassmann_coef(self.ctx, K, S.ptr, float(scalar), self.GRASSMANN_MODES[mode], coef.ptr),
              "mpsk_grassmann_coef")
        return coef

    def triu_(self, M: DTensor):
        """zero the strictly lower triangle of a column-major matrix in place (torch view of the buffer: a fill, no arithmetic)."""
        torch = _torch()
        r, c = M.shape
        v = torch.as_strided(M.buf, (r, c), (1, r))
        v.copy_(torch.triu(v))
        return M

    def tril_(self, M: DTensor):
        torch = _torch()
        r, c = M.shape
        v = torch.as_strided(M.buf, (r, c), (1, r))
        v.copy_(torch.tril(v))
        return M

    def copy2d(self, rows, cols, src_ptr, lds, dst_ptr, ldd):
        check(self.lib.mpsk_copy2d(self.ctx, rows, cols, src_ptr, lds, dst_ptr, ldd), "mpsk_copy2d")

    # ---- gauge -------------------------------------------------------------------------------
    def qrpos(self, A: DTensor):
        m, n = A.shape
        k = min(m, n)
        Q, R = self.empty(m, k), self.empty(k, n)
        check(self.lib.mpsk_qrpos(self.ctx, m, n, A.ptr, m, Q.ptr, m, R.ptr, k), "mpsk_qrpos")
        return Q, R

    def cx_embed_raw(self, m, n, h_ptr, ldh, e_ptr, lde):
        """embedded (2m x 2n) <- interleaved complex (2m x n), one launch (mpsk_cx_embed; leading dimensions in doubles)"""
        check(self.lib.mpsk_cx_embed(self.ctx, m, n, h_ptr, ldh, e_ptr, lde), "mpsk_cx_embed")

    def cx_half_raw(self, m, n, e_ptr, lde, h_ptr, ldh):
        """interleaved complex (2m x n) <- structured part of the embedded (2m x 2n), one launch (mpsk_cx_half)"""
        check(self.lib.mpsk_cx_half(self.ctx, m, n, e_ptr, lde, h_ptr, ldh), "mpsk_cx_half")

    def gemm_c(self, A: DTensor, B: DTensor, transA=False, transB=False, alpha=1.0, beta=0.0, out: DTensor = None):
        """C = alpha op(A) op(B) + beta C on interleaved complex128 matrices (shape (2 rows, cols); op = conjugate transpose;
        mpsk_gemm under MPSK_C128: the small gauge products AC = AL*C, AL = Q_AC*Q_C' of a complex host)."""
        ar, ac = A.shape[0] // 2, A.shape[1]
        br, bc = B.shape[0] // 2, B.shape[1]
        M, K = (ac, ar) if transA else (ar, ac)
        K2, N = (bc, br) if transB else (br, bc)
        assert K == K2
        out = self.empty(2 * M, N) if out is None else out
        self._set_dtype(True)
        try:
            check(self.lib.mpsk_gemm(self.ctx, int(transA), int(transB), M, N, K, float(alpha), A.ptr, ar, B.ptr, br,
                                     float(beta), out.ptr, M), "mpsk_gemm (C128)")
        finally:
            self._set_dtype(False)
        return out

    def qrpos_c(self, A: DTensor):
        """QRpos of an interleaved complex128 matrix (upload_c layout: shape (2 m, n) = complex m x n): returns Q (2 m, n) and
        R (2 n, n), complex upper triangular with a real positive diagonal (mpsk_qrpos under MPSK_C128)."""
        m2, n = A.shape
        m = m2 // 2
        assert m2 == 2 * m and m >= n
        Q, R = self.empty(m2, n), self.empty(2 * n, n)
        self._set_dtype(True)
        try:
            check(self.lib.mpsk_qrpos(self.ctx, m, n, A.ptr, m, Q.ptr, m, R.ptr, n), "mpsk_qrpos (C128)")
        finally:
            self._set_dtype(False)
        return Q, R

    def lqpos_c(self, A: DTensor):
        """LQpos of an interleaved complex128 matrix (shape (2 m, n), m <= n): L (2 m, m) lower triangular with a real positive
        diagonal, Q (2 m, n) with orthonormal rows (mpsk_lqpos under MPSK_C128)."""
        m2, n = A.shape
        m = m2 // 2
        assert m2 == 2 * m and m <= n
        L, Q = self.empty(m2, m), self.empty(m2, n)
        self._set_dtype(True)
        try:
            check(self.lib.mpsk_lqpos(self.ctx, m, n, A.ptr, m, L.ptr, m, Q.ptr, m), "mpsk_lqpos (C128)")
        finally:
            self._set_dtype(False)
        return L, Q

    def tsvd_c(self, theta: DTensor, max_keep=0, trunc_err=0.0):
        """Truncated SVD of an interleaved complex128 matrix (upload_c layout: shape (2 m, n) = complex m x n; mpsk_tsvd under
        MPSK_C128): U (2 m, kmax), S (kmax,) real descending, Vh (2 kmax, n), kept, discarded norm -- as tsvd."""
        m2, n = theta.shape
        m = m2 // 2
        assert m2 == 2 * m
        kmax = min(m, n)
        U, S, Vh = self.empty(m2, kmax), self.empty(kmax), self.empty(2 * kmax, n)
        kept, disc = C.c_int(0), C.c_double(0.0)
        self._set_dtype(True)
        try:
            check(self.lib.mpsk_tsvd(self.ctx, m, n, theta.ptr, m, U.ptr, m, S.ptr, Vh.ptr, kmax, int(max_keep),
                                     float(trunc_err), C.byref(kept), C.byref(disc)), "mpsk_tsvd (C128)")
        finally:
            self._set_dtype(False)
        return U, S, Vh, kept.value, disc.value

    def tsplit_c(self, theta: DTensor, max_keep=0, trunc_err=0.0):
        """Two-site split of an interleaved complex128 tensor (shape (2 m, n) = complex m x n; mpsk_tsplit under MPSK_C128):
        al (2 m, k), c (2 k, k) lower triangular, ar (2 k, n), the k kept singular values, discarded norm.  trunc_err = 0:
        truncdim scheme (max_keep); trunc_err > 0: k from the native complex SVD (the smaller of the two schemes)."""
        m2, n = theta.shape
        m = m2 // 2
        kf = min(m, n)
        AL, Cm, AR, S = self.empty(m2, kf), self.empty(2 * kf, kf), self.empty(2 * kf, n), self.empty(kf)
        kept, disc = C.c_int(0), C.c_double(0.0)
        self._set_dtype(True)
        try:
            check(self.lib.mpsk_tsplit(self.ctx, m, n, theta.ptr, m, int(max_keep), float(trunc_err), AL.ptr, m, Cm.ptr, kf,
                                       AR.ptr, kf, S.ptr, C.byref(kept), C.byref(disc)), "mpsk_tsplit (C128)")
        finally:
            self._set_dtype(False)
        k = kept.value
        c, ar = self.empty(2 * k, k), self.empty(2 * k, n)
        self.copy2d(2 * k, k, Cm.ptr, 2 * kf, c.ptr, 2 * k)
        self.copy2d(2 * k, n, AR.ptr, 2 * kf, ar.ptr, 2 * k)
        return DTensor(AL.buf, (m2, k)), c, ar, self.download(DTensor(S.buf, (k,))), disc.value

    def qrpos2(self, A1: DTensor, A2: DTensor):
        """two QRpos of equal shape in flight together (two streams inside the ctx)."""
        m, n = A1.shape
        assert A2.shape == (m, n) and m >= n
        Q1, R1, Q2, R2 = self.empty(m, n), self.empty(n, n), self.empty(m, n), self.empty(n, n)
        check(self.lib.mpsk_qrpos2(self.ctx, m, n, A1.ptr, m, Q1.ptr, m, R1.ptr, n, A2.ptr, m, Q2.ptr, m, R2.ptr, n),
              "mpsk_qrpos2")
        return Q1, R1, Q2, R2

    def qr_defer(self):
        """the next qrpos2 / lqpos returns once enqueued; finish it with qr_commit (include/mpsk.h)."""
        check(self.lib.mpsk_ctx_qr_defer(self.ctx), "mpsk_ctx_qr_defer")

    def side_mark(self):
        check(self.lib.mpsk_ctx_side_mark(self.ctx), "mpsk_ctx_side_mark")

    def side_begin(self):
        """route the following calls to the ctx's second stream, ordered after side_mark() only (include/mpsk.h)."""
        check(self.lib.mpsk_ctx_side_begin(self.ctx), "mpsk_ctx_side_begin")

    def side_end(self):
        check(self.lib.mpsk_ctx_side_end(self.ctx), "mpsk_ctx_side_end")

    def qr_commit(self) -> int:
        r = C.c_int(0)
        check(self.lib.mpsk_qr_commit(self.ctx, C.byref(r)), "mpsk_qr_commit")
        return r.value

    def qrlq_pair(self, A1: DTensor, A2: DTensor):
        """QRpos of A1 (m x n) and LQpos of A2 (n x m) in flight together -> (Q1, R1, L2, Q2)."""
        m, n = A1.shape
        assert A2.shape == (n, m) and m >= n
        Q1, R1, L2, Q2 = self.empty(m, n), self.empty(n, n), self.empty(n, n), self.empty(n, m)
        check(self.lib.mpsk_qrlq_pair(self.ctx, m, n, A1.ptr, m, Q1.ptr, m, R1.ptr, n, A2.ptr, n, L2.ptr, n, Q2.ptr, n),
              "mpsk_qrlq_pair")
        return Q1, R1, L2, Q2

    def lqpos(self, A: DTensor):
        m, n = A.shape
        k = min(m, n)
        L, Q = self.empty(m, k), self.empty(k, n)
        check(self.lib.mpsk_lqpos(self.ctx, m, n, A.ptr, m, L.ptr, m, Q.ptr, k), "mpsk_lqpos")
        return L, Q

    def tsvd(self, theta: DTensor, max_keep=0, trunc_err=0.0):
        m, n = theta.shape
        kmax = min(m, n)
        U, S, Vh = self.empty(m, kmax), self.empty(kmax), self.empty(kmax, n)
        kept, disc = C.c_int(0), C.c_double(0.0)
        check(self.lib.mpsk_tsvd(self.ctx, m, n, theta.ptr, m, U.ptr, m, S.ptr, Vh.ptr, kmax, int(max_keep),
                                 float(trunc_err), C.byref(kept), C.byref(disc)), "mpsk_tsvd")
        return U, S, Vh, kept.value, disc.value

    def tsplit(self, theta: DTensor, max_keep=0, trunc_err=0.0):
        """Truncated two-site split theta (m x n) ~ al (m x k) . c (k x k) . ar (k x n)  (mpsk_tsplit: V-free Jacobi;
        small tensors go through mpsk_tsvd with c = diag(S)).  Returns (al, c, ar, S[:k] on the host, disc)."""
        m, n = theta.shape
        kmax = min(m, n)
        if kmax <= 64:
            U, S, Vh, k, disc = self.tsvd(theta, max_keep=max_keep, trunc_err=trunc_err)
            s = self.download(DTensor(S.buf, (k,)))
            al = self.empty(m, k)
            self.copy2d(m, k, U.ptr, m, al.ptr, m)
            ar = self.empty(k, n)
            self.copy2d(k, n, Vh.ptr, kmax, ar.ptr, k)
            if k > 0 and s[k - 1] <= 1e-14 * s[0]:
                # kept singular values at the rounding floor (rank-deficient theta with truncdim > rank): the one-sided
                # Jacobi leaves (numerically) zero vectors there, LAPACK returns an orthonormal completion.  QRpos /
                # LQpos (Householder for <= 64 columns) reproduce the well-defined columns and complete the rest,
                # so al / ar stay isometries, which the lazy gauge and FinEnv assume.
                al, _ = self.qrpos(al)
                _, ar = self.lqpos(ar)
            return al, self.upload(np.diag(s)), ar, s, disc
        AL, Cm, AR, S = self.empty(m, kmax), self.empty(kmax, kmax), self.empty(kmax, n), self.empty(kmax)
        kept, disc = C.c_int(0), C.c_double(0.0)
        check(self.lib.mpsk_tsplit(self.ctx, m, n, theta.ptr, m, int(max_keep), float(trunc_err), AL.ptr, m, Cm.ptr, kmax,
                                   AR.ptr, kmax, S.ptr, C.byref(kept), C.byref(disc)), "mpsk_tsplit")
        k = kept.value
        al = DTensor(AL.buf, (m, k))                       # leading k columns, ld = m
        c = self.empty(k, k)
        self.copy2d(k, k, Cm.ptr, kmax, c.ptr, k)
        ar = self.empty(k, n)
        self.copy2d(k, n, AR.ptr, kmax, ar.ptr, k)
        return al, c, ar, self.download(DTensor(S.buf, (k,))), disc.value

    # ---- vectors -----------------------------------------------------------------------------
    def _ptrs(self, xs):
        arr = (C.c_void_p * len(xs))(*[x.ptr for x in xs])
        return arr

    def dot(self, x: DTensor, y: DTensor):
        out = C.c_double()
        check(self.lib.mpsk_vdot(self.ctx, x.size, x.ptr, y.ptr, C.byref(out)), "mpsk_vdot")
        return out.value

    def norm(self, x: DTensor):
        out = C.c_double()
        check(self.lib.mpsk_vnrm2(self.ctx, x.size, x.ptr, C.byref(out)), "mpsk_vnrm2")
        return out.value

    def vdiff_nrm2(self, x: DTensor, y: DTensor):
        """mpsk_vdiff_nrm2: (|x - y|^2, |x|^2) from one pass over both vectors (interleaved complex tensors: the same sums
        over their doubles)."""
        assert x.size == y.size, (x.shape, y.shape)
        out = (C.c_double * 2)()
        check(self.lib.mpsk_vdiff_nrm2(self.ctx, x.size, x.ptr, y.ptr, out), "mpsk_vdiff_nrm2")
        return out[0], out[1]

    def axpby(self, alpha, x: DTensor, beta, y: DTensor):
        check(self.lib.mpsk_vaxpby(self.ctx, x.size, float(alpha), x.ptr, float(beta), y.ptr), "mpsk_vaxpby")
        return y

    def times_i(self, x: DTensor, out: DTensor = None):
        """embedded complex tensors (cplx.py): out = i * x  (first dimension = interleaved re/im rows)."""
        y = self.empty(*x.shape) if out is None else out
        check(self.lib.mpsk_vtimes_i(self.ctx, x.size, x.ptr, y.ptr), "mpsk_vtimes_i")
        return y

    def scal(self, alpha, x: DTensor):
        check(self.lib.mpsk_vscal(self.ctx, x.size, float(alpha), x.ptr), "mpsk_vscal")
        return x

    def multidot(self, xs, y: DTensor):
        out = (C.c_double * len(xs))()
        check(self.lib.mpsk_vmultidot(self.ctx, y.size, len(xs), self._ptrs(xs), y.ptr, out), "mpsk_vmultidot")
        return np.array(out[:])

    def gs_step(self, xs, y: DTensor):
        out = (C.c_double * len(xs))()
        check(self.lib.mpsk_vgs_step(self.ctx, y.size, len(xs), self._ptrs(xs), y.ptr, out), "mpsk_vgs_step")
        return np.array(out[:])

    def orth_step(self, xs, y: DTensor):
        """CGS2 of y against xs, then y <- y/||y||; ONE host sync.  Returns (h[k], beta)."""
        out = (C.c_double * len(xs))()
        beta = C.c_double()
        check(self.lib.mpsk_vorth_step(self.ctx, y.size, len(xs), self._ptrs(xs), y.ptr, out, C.byref(beta)),
              "mpsk_vorth_step")
        return np.array(out[:]), beta.value

    class _OrthHandle:
        """result of orth_step_async: .result() waits for the step's scalars only (an event), not for the stream, and
        hands the (device, pinned host) buffer pair back to the backend's free list"""
        __slots__ = ("be", "slot", "event", "k")

        def __init__(self, be, slot, event, k):
            self.be, self.slot, self.event, self.k = be, slot, event, k

        def result(self):
            self.event.synchronize()
            k = self.k
            t = self.slot[1].numpy()
            h = (t[:k] + t[k:2 * k]).copy()
            beta = float(np.sqrt(max(t[2 * k], 0.0)))
            self.be._orth_free.append(self.slot)
            self.slot = None
            return h, beta

        def __del__(self):                      # a speculative step that was dropped: the buffers go back as well
            if self.slot is not None:           # (stream order: the dropped copy completes before any later use of them)
                self.be._orth_free.append(self.slot)

    ORTH_SLOT = 544                             # 2 * 271 + 2 doubles

    def orth_step_async(self, xs, y: DTensor):
        """orth_step whose scalars travel to the host asynchronously: the call returns once the CGS2 / normalisation
        kernels and the device-to-host copy of the 2k+1 scalars are enqueued.  A tolerance-mode Krylov loop enqueues the
        NEXT matvec before it reads the handle, so the GPU works while the host takes its per-step decision (the stream used
        to drain at every step: 36 % idle in the VUMPS run of BASELINE config 3, profiles/r03_small_D_kernel_stats.log).
        Every handle owns its buffers until it is read or dropped: solvers nest (the quasiparticle effective Hamiltonian
        runs GMRES solves inside the matvec of an outer eigensolver that has a handle in flight)."""
        torch = _torch()
        k = len(xs)
        n = 2 * k + 1
        if n > self.ORTH_SLOT:
            raise MpskError("orth_step_async: more than 271 basis vectors")
        free = getattr(self, "_orth_free", None)
        if free is None:
            free = self._orth_free = []
        slot = free.pop() if free else (torch.empty(self.ORTH_SLOT, dtype=torch.float64, device=self.device),
                                        torch.empty(self.ORTH_SLOT, dtype=torch.float64).pin_memory())
        check(self.lib.mpsk_vorth_step_dev(self.ctx, y.size, k, self._ptrs(xs), y.ptr, slot[0].data_ptr()), "mpsk_vorth_step_dev")
        with torch.cuda.stream(self.torch_stream):
            slot[1][:n].copy_(slot[0][:n], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.torch_stream)
        return Backend._OrthHandle(self, slot, ev, k)

    def orth_step_dev(self, xs, y: DTensor, slot: DTensor, offset: int):
        """orth_step without the host sync: the 2k+1 scalars go to slot[offset : offset + 2k + 1] on the device."""
        check(self.lib.mpsk_vorth_step_dev(self.ctx, y.size, len(xs), self._ptrs(xs), y.ptr, slot.ptr + 8 * offset),
              "mpsk_vorth_step_dev")

    def normalize_dev(self, x: DTensor, out: DTensor = None, slot: DTensor = None, offset: int = 0):
        """out = x / |x| (default in place) with no host sync; |x|^2 goes to slot[offset] (device) when given."""
        y = x if out is None else out
        check(self.lib.mpsk_vnormalize_dev(self.ctx, x.size, x.ptr, y.ptr, None if slot is None else slot.ptr + 8 * offset),
              "mpsk_vnormalize_dev")
        return y

    def nrm2_dev(self, x: DTensor, slot: DTensor, offset: int = 0):
        """slot[offset] = |x|^2 on the device, no host sync."""
        check(self.lib.mpsk_vnrm2_dev(self.ctx, x.size, x.ptr, slot.ptr + 8 * offset), "mpsk_vnrm2_dev")

    RITZ_BUF = 40   # doubles: coefficients [0:32], info (lambda, residual estimate, effective m) [32:35]

    def ritz_dev(self, m: int, stride: int, slot: DTensor, buf: DTensor):
        """Ritz coefficients of a fixed-budget solve on the device (mpsk_vritz_dev): buf[0:m], buf[32:35] = info."""
        check(self.lib.mpsk_vritz_dev(self.ctx, int(m), int(stride), slot.ptr, buf.ptr, buf.ptr + 8 * 32), "mpsk_vritz_dev")

    def lincomb_dev(self, xs, coef: DTensor, out: DTensor = None):
        y = self.empty(xs[0].shape) if out is None else out
        check(self.lib.mpsk_vlincomb_dev(self.ctx, y.size, len(xs), self._ptrs(xs), coef.ptr, y.ptr), "mpsk_vlincomb_dev")
        return y

    def multilincomb(self, xs, S, outs):
        """outs[j] = sum_i S[i, j] xs[i] in one pass over the vectors (mpsk_vmultilincomb: the basis rotation of a thick
        restart); len(xs), len(outs) <= 32, outs disjoint from xs."""
        S = np.asarray(S, dtype=float)
        k, m = len(xs), len(outs)
        assert S.shape == (k, m)
        cf = (C.c_double * (k * m))(*S.T.reshape(-1))                # column j of S contiguous: coefs[i + k j]
        check(self.lib.mpsk_vmultilincomb(self.ctx, xs[0].size, k, self._ptrs(xs), m, self._ptrs(outs), cf),
              "mpsk_vmultilincomb")
        return outs

    def lincomb(self, xs, coefs, out: DTensor = None):
        y = self.empty(xs[0].shape) if out is None else out
        cf = (C.c_double * len(xs))(*[float(c) for c in coefs])
        check(self.lib.mpsk_vlincomb(self.ctx, y.size, len(xs), self._ptrs(xs), cf, y.ptr), "mpsk_vlincomb")
        return y

    # ---- complex forms on interleaved vectors (mpsk_v*_c; sizes in complex elements = half the doubles) ------------
    @staticmethod
    def _c2(z):
        z = complex(z)
        return (C.c_double * 2)(z.real, z.imag)

    def dotc(self, x: DTensor, y: DTensor):
        """conj(x) . y of two interleaved complex tensors (mpsk_vdotc)."""
        assert x.size == y.size and x.size % 2 == 0, (x.shape, y.shape)
        out = (C.c_double * 2)()
        check(self.lib.mpsk_vdotc(self.ctx, x.size // 2, x.ptr, y.ptr, out), "mpsk_vdotc")
        return complex(out[0], out[1])

    def axpby_c(self, alpha, x: DTensor, beta, y: DTensor):
        """y = alpha x + beta y with complex scalars (mpsk_vaxpby_c)."""
        assert x.size == y.size and x.size % 2 == 0, (x.shape, y.shape)
        check(self.lib.mpsk_vaxpby_c(self.ctx, x.size // 2, self._c2(alpha), x.ptr, self._c2(beta), y.ptr), "mpsk_vaxpby_c")
        return y

    def orth_step_c(self, xs, y: DTensor):
        """orth_step in complex arithmetic (mpsk_vorth_step_c): returns (h[k] complex = X^H y, beta)."""
        k = len(xs)
        out = (C.c_double * (2 * k))()
        beta = C.c_double()
        check(self.lib.mpsk_vorth_step_c(self.ctx, y.size // 2, k, self._ptrs(xs), y.ptr, out, C.byref(beta)),
              "mpsk_vorth_step_c")
        return np.array(out[:]).view(np.complex128).copy(), beta.value

    def lincomb_c(self, xs, coefs, out: DTensor = None):
        """out = sum_j coefs[j] xs[j] with complex coefficients (mpsk_vlincomb_c)."""
        y = self.empty(xs[0].shape) if out is None else out
        flat = np.ascontiguousarray(np.asarray(coefs, dtype=np.complex128)[:len(xs)]).view(np.float64)
        cf = (C.c_double * (2 * len(xs)))(*flat)
        check(self.lib.mpsk_vlincomb_c(self.ctx, y.size // 2, len(xs), self._ptrs(xs), cf, y.ptr), "mpsk_vlincomb_c")
        return y


class PreparedHAC:
    """Owner of an mpsk_hac handle (include/mpsk.h): `apply(x, out, nblk)` is one matvec."""

    def __init__(self, be: Backend, H, GL: DTensor, GR: DTensor, flags: int = 0):
        Wl, Dlo, Dl = GL.shape
        Wr, Dr2, Dr = GR.shape
        self.cplx = bool(getattr(H, "cplx", False))
        m = 2 if self.cplx else 1                                   # interleaved complex: doubled first dimensions
        Dlo //= m
        assert Wl == H.Wl and Wr == H.Wr and Dr2 == m * Dr, (GL.shape, GR.shape)
        self.be, self.H, self.GL, self.GR = be, H, GL, GR           # references keep the operands alive
        self.Dlo, self.Dl, self.Dr, self.d = Dlo, Dl, Dr, H.d
        h = C.c_void_p()
        if flags:
            check(be.lib.mpsk_hac_create_ex(be.ctx, H.handle, Dlo, Dl, Dr, GL.ptr, GR.ptr, int(flags), C.byref(h)),
                  "mpsk_hac_create_ex")
        else:
            check(be.lib.mpsk_hac_create(be.ctx, H.handle, Dlo, Dl, Dr, GL.ptr, GR.ptr, C.byref(h)), "mpsk_hac_create")
        self.handle = h

    def info(self):
        mode, ns = C.c_int(), C.c_int()
        check(self.be.lib.mpsk_hac_info(self.handle, C.byref(mode), C.byref(ns)), "mpsk_hac_info")
        return {"mode": mode.value, "combined_slabs": ns.value}

    def apply(self, x: DTensor, out: DTensor = None, nblk=1):
        m = 2 if self.cplx else 1
        assert x.shape == (m * self.Dl, self.d, self.Dr), (x.shape, (m * self.Dl, self.d, self.Dr))
        y = self.be.empty(m * self.Dlo, self.d, self.Dr) if out is None else out
        check(self.be.lib.mpsk_hac_apply(self.handle, x.ptr, int(nblk), y.ptr), "mpsk_hac_apply")
        return y

    def apply_axpby(self, a1, x: DTensor, a0, out: DTensor = None, nblk=1):
        """out = a0 x + a1 (H x) (mpsk_hac_apply_axpby): the shifted operator of a linear solve.  Complex scalars for a
        complex operator; a real operator takes their real parts."""
        m = 2 if self.cplx else 1
        assert x.shape == (m * self.Dl, self.d, self.Dr), (x.shape, (m * self.Dl, self.d, self.Dr))
        y = self.be.empty(m * self.Dlo, self.d, self.Dr) if out is None else out
        check(self.be.lib.mpsk_hac_apply_axpby(self.handle, Backend._c2(a1), x.ptr, int(nblk), Backend._c2(a0), y.ptr),
              "mpsk_hac_apply_axpby")
        return y

    def eigsolve_fixed(self, x0: DTensor, m: int, vecs, scal: DTensor, out: DTensor, first_image: DTensor = None):
        """mpsk_hac_eigsolve_fixed: the whole fixed-budget solve (m steps) in one call; vecs = m + 2 work vectors."""
        assert not self.cplx and len(vecs) >= m + 2 and scal.size >= m * (2 * m + 1) + 40
        ptrs = self.be._ptrs(vecs[:m + 2])
        check(self.be.lib.mpsk_hac_eigsolve_fixed(self.handle, x0.ptr, int(m), ptrs, scal.ptr, out.ptr,
                                                  None if first_image is None else first_image.ptr), "mpsk_hac_eigsolve_fixed")
        return out

    def close(self):
        if getattr(self, "handle", None) and self.be.ctx:
            self.be.lib.mpsk_hac_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PreparedHSum:
    """Owner of an mpsk_hsum handle (include/mpsk.h): set_coefs(c) then apply(x, out) is y = sum_k c[k] H_k x."""

    def __init__(self, be: Backend, Hs, GLs, GRs, flags: int = 0):
        n = len(Hs)
        assert n == len(GLs) == len(GRs) and n >= 1
        self.cplx = bool(getattr(Hs[0], "cplx", False))
        m = 2 if self.cplx else 1
        _, Dlo, Dl = GLs[0].shape
        _, _, Dr = GRs[0].shape
        self.be, self.Hs, self.GLs, self.GRs = be, list(Hs), list(GLs), list(GRs)      # keep the operands alive
        self.n, self.Dlo, self.Dl, self.Dr, self.d = n, Dlo // m, Dl, Dr, Hs[0].d
        arr = lambda ps: (C.c_void_p * n)(*ps)
        h = C.c_void_p()
        check(be.lib.mpsk_hsum_create(be.ctx, n, arr([H.handle.value for H in Hs]), self.Dlo, Dl, Dr,
                                      arr([g.ptr for g in GLs]), arr([g.ptr for g in GRs]), int(flags), C.byref(h)),
              "mpsk_hsum_create")
        self.handle = h

    def info(self):
        route, ln = C.c_int(), C.c_int()
        check(self.be.lib.mpsk_hsum_info(self.handle, C.byref(route), C.byref(ln)), "mpsk_hsum_info")
        return {"route": route.value, "launches": ln.value}

    def set_coefs(self, coefs):
        assert len(coefs) == self.n
        check(self.be.lib.mpsk_hsum_set_coefs(self.handle, (C.c_double * self.n)(*[float(c) for c in coefs])),
              "mpsk_hsum_set_coefs")
        return self

    def apply(self, x: DTensor, out: DTensor = None):
        m = 2 if self.cplx else 1
        assert x.shape == (m * self.Dl, self.d, self.Dr), (x.shape, (m * self.Dl, self.d, self.Dr))
        y = self.be.empty(m * self.Dlo, self.d, self.Dr) if out is None else out
        check(self.be.lib.mpsk_hsum_apply(self.handle, x.ptr, y.ptr), "mpsk_hsum_apply")
        return y

    def apply_axpby(self, a1, x: DTensor, a0, out: DTensor = None):
        m = 2 if self.cplx else 1
        assert x.shape == (m * self.Dl, self.d, self.Dr), (x.shape, (m * self.Dl, self.d, self.Dr))
        y = self.be.empty(m * self.Dlo, self.d, self.Dr) if out is None else out
        check(self.be.lib.mpsk_hsum_apply_axpby(self.handle, Backend._c2(a1), x.ptr, Backend._c2(a0), y.ptr),
              "mpsk_hsum_apply_axpby")
        return y

    def close(self):
        if getattr(self, "handle", None) and self.be.ctx:
            self.be.lib.mpsk_hsum_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceMPOSlice:
    """Device-side SparseMPOSlice (sparseslice.jl:13-27): keeps the host block table for the
    host-side logic (keys / isscal / contains) and an mpsk_mposlice handle for the kernels."""

    def __init__(self, be: Backend, odim, d, chil, chir, blocks, cplx=False):
        self.be = be
        self.cplx = bool(cplx)
        self.odim, self.d = int(odim), int(d)
        self.chil, self.chir = [int(c) for c in chil], [int(c) for c in chir]
        self.Wl, self.Wr = sum(self.chil), sum(self.chir)
        self.blocks = dict(blocks)
        n = self.odim
        kind = (C.c_int32 * (n * n))()
        scal = (C.c_double * ((2 if self.cplx else 1) * n * n))()
        ptrs = (C.c_void_p * (n * n))()
        keep = []
        for (i, j), v in self.blocks.items():
            if np.isscalar(v):
                if not self.cplx and np.iscomplexobj(v) and complex(v).imag != 0:
                    raise MpskError("complex MPO entries need an MPSK_C128 slice (mposlice(..., cplx=True))")
                if v == 0:
                    continue
                kind[i + n * j] = 1
                if self.cplx:
                    scal[2 * (i + n * j)], scal[2 * (i + n * j) + 1] = float(np.real(v)), float(np.imag(v))
                else:
                    scal[i + n * j] = float(np.real(v))
            else:
                a = np.asarray(v)
                if np.iscomplexobj(a) and not self.cplx:
                    if np.abs(a.imag).max() > 0:
                        raise MpskError("complex MPO entries need an MPSK_C128 slice (mposlice(..., cplx=True))")
                    a = a.real
                assert a.shape == (self.chil[i], d, d, self.chir[j]), (a.shape, i, j)
                if self.cplx:
                    flat = np.ravel(np.asarray(a, dtype=np.complex128), order="F").view(np.float64).copy()
                else:
                    flat = np.ravel(np.asfortranarray(a, dtype=np.float64), order="F").copy()
                keep.append(flat)
                kind[i + n * j] = 2
                ptrs[i + n * j] = flat.ctypes.data
        h = C.c_void_p()
        cl = (C.c_int32 * n)(*self.chil)
        cr = (C.c_int32 * n)(*self.chir)
        check(be.lib.mpsk_mposlice_create(be.ctx, 1 if self.cplx else 0, n, cl, cr, self.d, kind, scal, ptrs, C.byref(h)),
              "mpsk_mposlice_create")
        self.handle = h

    def __del__(self):
        try:
            if self.handle and self.be.ctx:
                self.be.lib.mpsk_mposlice_destroy(self.handle)
        except Exception:
            pass
        self.handle = None

    # host-side helpers mirroring sparseslice.jl:74-106
    def keys(self):
        return sorted(self.blocks.keys(), key=lambda t: (t[1], t[0]))

    def contains(self, i, j):
        return (i, j) in self.blocks and not (np.isscalar(self.blocks[(i, j)]) and self.blocks[(i, j)] == 0)

    def isscal(self, i, j):
        return self.contains(i, j) and np.isscalar(self.blocks[(i, j)])


class DeviceDenseSlice:
    """Device-side DenseMPO tensor: one dense level [Wl, d, d, Wr] behind an mpsk_mposlice handle marked dense."""

    cplx = False

    def __init__(self, be: Backend, O):
        a = np.asarray(O)
        if np.iscomplexobj(a):
            if np.abs(a.imag).max(initial=0.0) > 0:
                raise MpskError("DenseMPO: complex tensors are not supported (MPSK_F64 only)")
            a = a.real
        if a.ndim != 4 or a.shape[1] != a.shape[2]:
            raise MpskError(f"DenseMPO tensor must be [Wl, d, d, Wr], got {a.shape}")
        self.be = be
        self.Wl, self.d, _, self.Wr = (int(n) for n in a.shape)
        self.odim, self.chil, self.chir = 1, [self.Wl], [self.Wr]
        self.blocks = {(0, 0): a}
        flat = np.ravel(np.asarray(a, dtype=np.float64), order="F").copy()
        h = C.c_void_p()
        check(be.lib.mpsk_mposlice_create_dense(be.ctx, 0, self.Wl, self.Wr, self.d, flat.ctypes.data, C.byref(h)),
              "mpsk_mposlice_create_dense")
        self.handle = h

    def __del__(self):
        try:
            if self.handle and self.be.ctx:
                self.be.lib.mpsk_mposlice_destroy(self.handle)
        except Exception:
            pass
        self.handle = None


_default = {}


def default_backend(device=None):
    torch = _torch()
    if device is None:
        device = torch.cuda.current_device() if torch.cuda.is_available() else 0
    if device not in _default:
        _default[device] = Backend(device)
    return _default[device]
