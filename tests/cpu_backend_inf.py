"""TEST INFRASTRUCTURE: CpuComplexBackend + the entry points the uniform states on interleaved storage use
(mpskit_jl_amd.native_cplx.NativeInfiniteMPS / NativePerMPOInfEnv): pass-through complex transfers, mpsk_dAC_proj on a complex
slice, mpsk_dC_proj_c, mpsk_vsplit_c / mpsk_vjoin_c and the complex mpsk_site_gram, all by NumPy and the oracle."""
import numpy as np
import torch

import mpskit_oracle as mo
from cpu_backend import CpuComplexBackend


class CpuInfBackend(CpuComplexBackend):
    def transfer_left(self, H, GLin, A, Ab, out=None, cplx=False, canonical=False):
        if H is None and cplx:
            self._count("transfer_left_c")
            a, ab = self.download_c(A), self.download_c(Ab)
            res = [mo.transfer_left_block(v, None, a, ab) for v in self._env_c(GLin, [1] * GLin.shape[0])]
            return self._put_env_c(res, out)
        return super().transfer_left(H, GLin, A, Ab, out, cplx, canonical)

    def transfer_right(self, H, GRin, A, Ab, out=None, cplx=False, canonical=False):
        if H is None and cplx:
            self._count("transfer_right_c")
            a, ab = self.download_c(A), self.download_c(Ab)
            res = [mo.transfer_right_block(v, None, a, ab) for v in self._env_c(GRin, [1] * GRin.shape[0])]
            return self._put_env_c(res, out)
        return super().transfer_right(H, GRin, A, Ab, out, cplx, canonical)

    def dAC_proj(self, H, GL, GR, x, out=None):
        o = self.empty(GL.shape[1], x.shape[1], GR.shape[2]) if out is None else out
        if not getattr(H, "cplx", False):
            self._count("dAC_proj")
            return self._set(o, mo.dAC(self.download(x), H.oracle, self._env(GL, H.chil), self._env(GR, H.chir)))
        self._count("dAC_proj_c")
        return self._set_c(o, mo.dAC(self.download_c(x), H.oracle, self._env_c(GL, H.chil), self._env_c(GR, H.chir)))

    def dC_proj_c(self, GL, GR, c, out=None):
        self._count("dC_proj_c")
        W = GL.shape[0]
        y = mo.dC(self.download_c(c), self._env_c(GL, [1] * W), self._env_c(GR, [1] * W))
        o = self.empty(GL.shape[1], GR.shape[2]) if out is None else out
        return self._set_c(o, y)

    def split_c(self, z, out=None):
        v = z.buf[: z.size].numpy().reshape(-1, 2)
        p = self.empty(z.size) if out is None else out
        p.buf[: z.size] = torch.from_numpy(np.concatenate([v[:, 0], v[:, 1]]))
        return p

    def join_c(self, p, shape, out=None):
        n = p.size // 2
        v = p.buf[: p.size].numpy()
        z = self.empty(*shape) if out is None else out
        z.buf[: p.size] = torch.from_numpy(np.stack([v[:n], v[n:]], axis=1).reshape(-1))
        return z

    def site_gram(self, X, Ab, out=None, cplx=False):
        assert cplx and X.shape == Ab.shape, "the stand-in computes the one-site complex Gram matrix only"
        x, ab = self.download_c(X), self.download_c(Ab)
        g = np.einsum("ptb,psb->ts", np.conj(ab), x)
        return self.upload_c(g).reshape(1, 2 * g.shape[0], g.shape[1])
