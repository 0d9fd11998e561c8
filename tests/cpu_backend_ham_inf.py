"""TEST INFRASTRUCTURE: CpuInfBackend for the cases of tests/native_ham_inf_cases.py, which run the project's real VUMPS / TDVP
and the interleaved drivers (mpskit_jl_amd.native_cplx.NativeMPOHamInfEnv, VUMPS, TDVP on a NativeInfiniteMPS) on ONE
backend: the prepared site operator is served for real slices as well.  It has no regularize_axpby, so the environments
take the composed route of the regulariser (dotc / axpby_c, composed in turn from the real vector methods)."""
from cpu_backend import CpuComplexBackend
from cpu_backend_inf import CpuInfBackend


class CpuHamInfBackend(CpuInfBackend):
    def hac_create(self, H, GL, GR):
        return CpuComplexBackend._Hac(self, H, GL, GR)
