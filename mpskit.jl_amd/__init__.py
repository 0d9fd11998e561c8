"""mpskit.jl_amd -- MI355X-native (gfx950) DMRG / VUMPS hot path with the API of MPSKit.jl.

Import as ``import mpskit_jl_amd`` (the directory name contains a dot; the top-level module
``mpskit_jl_amd.py`` registers this package under that name).
"""
from ._lib import MpskError, LIB_PATH  # noqa: F401
from .backend import Backend, DTensor, DeviceMPOSlice, default_backend  # noqa: F401
from .operators import (MPOHamiltonian, SparseMPO, LazySum, MultipliedOperator, TimedOperator, UntimedOperator, istimed,
                        heisenberg_XXX, transverse_field_ising, hubbard, from_twosite,  # noqa: F401,E402
                        periodic_boundary_conditions)
from .states import FiniteMPS, InfiniteMPS  # noqa: F401,E402
from .environments import FinEnv, FinEnvPair, MPOHamInfEnv, MultipleEnvironments, environments  # noqa: F401,E402
from .derivatives import ddAC, ddAC2, ddC, MPO_ddAC, MPO_ddAC2, MPO_ddC  # noqa: F401,E402
from .algorithms import (DMRG, DMRG2, VUMPS, VOMPS, IDMRG1, IDMRG2, GradientGrassmann, UnionAlg, TDVP, TDVP2, Arnoldi,  # noqa: F401,E402
                         find_groundstate, calc_galerkin, expectation_value, timestep, time_evolve)
from . import grassmann  # noqa: F401,E402
from .changebonds import changebonds, OptimalExpand, RandExpand, SvdCut  # noqa: F401,E402
from .approximate import approximate, ac_proj, c_proj, make_time_mpo, WI, WII, TaylorCluster  # noqa: F401,E402
from .excitations import excitations, FiniteExcited, ProjectionOperator  # noqa: F401,E402
from .quasiparticle import QuasiparticleAnsatz, LeftGaugedQP, MultilineQP  # noqa: F401,E402
from .toolbox import (variance, entropy, entanglement_spectrum, transfer_spectrum, marek_gap, correlation_length,  # noqa: F401,E402
                      exact_diagonalization)
from .statmech import DenseMPO, PerMPOInfEnv, leading_boundary, classical_ising, sixvertex, dot  # noqa: F401,E402
from .multiline import MPSMultiline, MPOMultiline, MultilineEnv  # noqa: F401,E402
from . import native_cplx  # noqa: F401,E402   (complex128 states on interleaved storage: NativeFiniteMPS, dmrg, tdvp_step)
from .measure import correlator, decompose_localmpo  # noqa: F401,E402   (local expectation values: expectation_value above)
from . import window  # noqa: F401,E402
from .window import WindowMPS, WindowEnv, transition  # noqa: F401,E402   (window.dot: overlaps of two windows)
from .propagator import propagator, DynamicalDMRG, NaiveInvert, Jeckelmann, GMRES, LinearCombination  # noqa: F401,E402
from .susceptibility import fidelity_susceptibility, effective_excitation_hamiltonian, qp_dot  # noqa: F401,E402
from . import linalg  # noqa: F401,E402
from .linalg import normalize  # noqa: F401,E402   (psi1 + psi2, a * psi, dot(psi1, psi2) of finite states: linalg.py)
