/* libmpsk -- C ABI of the MI355X-native (gfx950) DMRG / VUMPS hot path.
 *
 * This is the drop-in boundary for the per-site inner loop of stecrotti/MPSKit.jl v0.10.2: every
 * entry point replaces one Julia method of the reference (cited as file:line relative to the
 * reference root) and is what a `ccall((:mpsk_xxx, libmpsk), Cint, ...)` shim binds.  The
 * reference itself has no FFI: the seams are the multiple-dispatch methods listed below
 * (SURVEY.md section 8b); INTEGRATION.md shows the Julia-side overloads.
 *
 * Conventions
 *  - every function returns 0 on success, non-zero on error; mpsk_last_error() gives the
 *    thread-local message.  No exceptions or longjmp cross the boundary.
 *  - all tensor arguments are DEVICE pointers to fp64, column-major ("Fortran", TensorKit's
 *    trivial-sector storage) in TensorKit index order:
 *        MPS tensor      x [Dl, d, Dr]             (V_l (x) P <- V_r)        src/states/abstractmps.jl:30-33
 *        two-site tensor x2[Dl, d, Dr, d]          (V_l (x) P <- V_r (x) P)  src/algorithms/groundstate/dmrg.jl:92
 *        bond matrix     c [Dl, Dr]
 *        environment     G [W][Dbra, Dket]  = W column-major slabs, slab (off_i + k) holding
 *                        GL[i][:, k, :] of the reference's Vector of [D, chi_i, D] tensors
 *                        (src/environments/FinEnv.jl:49-59, mpohaminfenv.jl:25-30); W = sum_i chi_i.
 *    The host owns all device memory (any allocator: hipMalloc, torch, AMDGPU.jl ROCArray);
 *    mpsk_malloc & co. are provided for hosts that have none.
 *  - one mpsk_ctx = one device + one HIP stream + a private workspace.  Calls on a ctx are
 *    asynchronous on its stream; functions that return a host scalar synchronise.  Distinct
 *    ctxs may be driven concurrently from distinct host threads (the reference applies its
 *    operators from several Julia tasks: vumps.jl:39-49,78-86); give each its own stream
 *    (mpsk_ctx_set_stream) if the work is to overlap.  ONE ctx must not be used from two threads
 *    at once.  The only process-wide state of the library (per-device kernel attributes, the
 *    split-K workspace table keyed by (device, stream), the event profile) is atomic /
 *    mutex-protected; tests/test_gpu_threads.py drives two ctxs from two threads and compares
 *    bit-for-bit with the serial run.  mpsk_ctx_force_tile and mpsk_prof_* are process-wide
 *    diagnostics.
 *  - dtype: MPSK_F64 (real fp64) everywhere; MPSK_C128 (complex128, the reference's default scalar type,
 *    defaults.jl:18) for the matvec / transfer family: mpsk_dAC, mpsk_dC, mpsk_dAC2, mpsk_hac_*, mpsk_transfer_left,
 *    mpsk_transfer_right.  A slice created with MPSK_C128 makes every tensor argument of a call that takes it complex;
 *    the slice-less calls (mpsk_dC, pass-through transfers) follow mpsk_ctx_set_dtype.  Complex tensors are
 *    INTERLEAVED complex128 in the same column-major index order (TensorKit / Julia Array{ComplexF64} storage); a
 *    complex MPO slice takes interleaved scalars[2 odim^2] and dense blocks.  Internally a complex product runs on
 *    the real fp64 MFMA core as two K-segments (re / im of the second operand, the first one through a loader that
 *    multiplies by i): 4x the real flops, the complex optimum.
 *    The gauge entry points follow mpsk_ctx_set_dtype too: mpsk_qrpos, mpsk_lqpos, mpsk_tsvd, mpsk_tsplit and mpsk_gemm.
 *    With MPSK_C128 their matrix operands are interleaved complex, leading dimensions count COMPLEX elements, and
 *    singular values (S) stay real doubles.
 *     - mpsk_qrpos / mpsk_lqpos: Q / R / L complex with a real positive diagonal on the triangular factor (TensorKit
 *       leftorth! / rightorth! with QRpos() / LQpos()).  They run on the real 2m x 2n embedding inside the library and
 *       keep the complex structure also for ill-conditioned / rank-deficient input (structured part + one more
 *       factorization, R = triu(Q^H A)).
 *     - mpsk_tsvd: a NATIVE complex one-sided block Jacobi (complex rotations, Hermitian Gram matrices) on the R^H of a
 *       complex QRpos of the tall orientation; each complex singular value appears once.  Same truncation rule as fp64.
 *     - mpsk_tsplit: trunc_err = 0 (truncdim): the real split of the embedding supplies the kept subspace (every value
 *       twice, arbitrary basis inside each pair), made an embedding again by projecting structured random vectors on it,
 *       with a J-invariant choice inside a cluster that straddles the cut.  trunc_err > 0 (truncerr, optionally with
 *       max_keep): the complex mpsk_tsvd chooses k, AL = U[:, :k] and (C, AR) = LQpos(AL^H theta).  Both return complex
 *       isometries AL / AR and C lower triangular with a real positive diagonal.
 *     - mpsk_gemm: interleaved complex matrices (trans = conjugate transpose, alpha / beta real) as ONE real GEMM on the
 *       embedded A and the interleaved B: 8 M N K flops, the complex optimum.
 *    The remaining entry points (mpsk_qrpos2, mpsk_qrlq_pair, Krylov vector helpers, mpsk_regularize) are fp64 only and
 *    ignore the ctx dtype: a complex host runs its vector arithmetic on the 2n doubles of an interleaved vector (real
 *    inner products suffice for the Hermitian Lanczos solvers).  Solvers that need a Krylov space over the complex
 *    numbers (GMRES with a complex shift) use the mpsk_v*_c forms at the end of this header.  mpsk_regularize_axpby, the
 *    regulariser of those solves on a uniform state, follows mpsk_ctx_set_dtype.
 */
#ifndef MPSK_H
#define MPSK_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mpsk_ctx mpsk_ctx;
typedef struct mpsk_mposlice mpsk_mposlice;

enum { MPSK_F64 = 0, MPSK_C128 = 1 };
enum { MPSK_OK = 0, MPSK_ERR_INVALID = 1, MPSK_ERR_HIP = 2, MPSK_ERR_UNSUPPORTED = 3, MPSK_ERR_NOMEM = 4 };
/* MPO block kinds, src/operators/sparsempo/sparseslice.jl:74-106 (contains / isscal) */
enum { MPSK_BLOCK_ZERO = 0, MPSK_BLOCK_SCALAR = 1, MPSK_BLOCK_DENSE = 2 };

int mpsk_version(void);
const char* mpsk_last_error(void);

/* ---- context ---------------------------------------------------------------------------- */
int mpsk_ctx_create(int device, mpsk_ctx** out);
int mpsk_ctx_destroy(mpsk_ctx* ctx);
int mpsk_ctx_set_stream(mpsk_ctx* ctx, void* hip_stream);      /* hipStream_t; NULL = default */
int mpsk_ctx_set_dtype(mpsk_ctx* ctx, int dtype);              /* scalar type of the slice-less calls (mpsk_dC, pass-through
                                                                 * transfers, mpsk_qrpos, mpsk_lqpos, mpsk_tsplit, mpsk_gemm) */
int mpsk_ctx_get_stream(mpsk_ctx* ctx, void** hip_stream);
int mpsk_ctx_get_device(mpsk_ctx* ctx, int* device);
int mpsk_ctx_synchronize(mpsk_ctx* ctx);
int mpsk_ctx_workspace_reserve(mpsk_ctx* ctx, size_t bytes);   /* pre-size the private workspace */
/* QRpos algorithm: 0 auto (shifted CholeskyQR3 on the GEMM core; when the device flags an ill-conditioned /
 * rank-deficient input: perturbed, repeatedly shifted CholeskyQR, then blocked Householder as the last resort),
 * 1 Householder only, 2 CholeskyQR3 only (error on flag).
 * Counters: factorizations finished by CholeskyQR3 / by Householder / CholeskyQR3 attempts that were flagged /
 * flagged inputs finished by the robust CholeskyQR variant (any pointer may be NULL). */
int mpsk_ctx_set_qr_mode(mpsk_ctx* ctx, int mode);
int mpsk_ctx_qr_stats(mpsk_ctx* ctx, long* n_chol, long* n_house, long* n_fallback, long* n_robust);
/* CholeskyQR3 factorizations whose first attempt (shift at the rounding level of the Gram matrix) broke down and that were
 * repeated with the shift of Fukaya et al. (s = 11 (mn + n(n+1)) u ||A||_F^2); counted in n_chol when the repeat succeeds */
int mpsk_ctx_qr_retries(mpsk_ctx* ctx, long* n_retry);
/* tsvd algorithm switch: 0 = Jacobi on theta directly; 1 = the tall orientation of theta is factored with QRpos first and
 * the block-Jacobi iteration runs on R^T (Drmac-Veselic preconditioning; far fewer sweeps on graded spectra); 2
 * = additionally R^T = Q1 R1 and the iteration runs on R1^T (V-free in mpsk_tsplit, with accumulated rotations in
 * mpsk_tsvd: 15 -> 10 sweeps on graded 4096^2 tensors for one more n x n QRpos).  mpsk_ctx_svd_stats returns the number of
 * Jacobi sweeps of the last mpsk_tsvd / mpsk_tsplit.
 * 3 (default) = mode 2, and mpsk_tsplit becomes TRUNCATION-AWARE when max_keep > 0 and r = max_keep + max(64, max_keep / 2) (rounded
 * up to 64; max_keep / 4 if that is too wide) is at most 5/8 of min(m, n): a randomized subspace iteration on the GEMM core finds the dominant r-dimensional
 * subspace, the Jacobi split runs on r columns instead of min(m, n), and the result is accepted only after a CHECK -- the
 * part of the kept triplets outside the iterated subspace, || U_k^T theta (I - W W^T) ||_F <= 1e-12 ||theta||_F
 * (MPSK_SPLIT_TOL) -- otherwise the iteration continues or the call falls through to mode 2 (flat spectra).  Same AL / C / AR
 * contract; S then holds the r leading values and NaN behind them.  mpsk_ctx_split_stats: path of the last mpsk_tsplit
 * (0 full iteration, 1 subspace stage accepted, 2 stage gave up -> full iteration), subspace iterations, check value.
 * Mode 0 has no relative accuracy on matrices whose COLUMNS are nearly parallel (condition number of the column-scaled
 * matrix >= 1/u, e.g. U diag(logspace(0,-14)) V^T behind random orthogonal factors): every rotation against an O(1) column
 * injects rounding noise u |a_big| into columns whose norm is of that order, so their mutual cosines stay O(1) and the
 * scale-invariant convergence test cannot be met; the call then returns MPSK_ERR_HIP "did not converge" instead of
 * non-isometric factors.  (Demmel-Veselic: one-sided Jacobi is accurate for A = B D with B well conditioned -- which is
 * what the QR preconditioning of modes 1 / 2 produces.) */
int mpsk_ctx_set_svd_mode(mpsk_ctx* ctx, int precondition);
int mpsk_ctx_svd_stats(mpsk_ctx* ctx, int* last_sweeps);
int mpsk_ctx_split_stats(mpsk_ctx* ctx, int* path, int* iterations, double* residual);   /* any pointer may be NULL */
/* tile override for benchmarking the GEMM core (0,0 restores the heuristic) */
int mpsk_ctx_force_tile(mpsk_ctx* ctx, int bm, int bn);

/* HIP-event profile of the matvec-stage GEMM launches (the dominant kernel, dac_gemm_f64_kernel):
 * enable, run, then read a JSON summary [{kernel, launches, total_ms, avg_ms, flops}] (synchronises). */
int mpsk_prof_enable(mpsk_ctx* ctx, int on);
int mpsk_prof_summary(mpsk_ctx* ctx, char* buf, size_t buflen);

/* ---- memory helpers (optional) ------------------------------------------------------------ */
int mpsk_malloc(mpsk_ctx* ctx, size_t bytes, void** dptr);
int mpsk_free(mpsk_ctx* ctx, void* dptr);
int mpsk_memcpy_h2d(mpsk_ctx* ctx, void* dst, const void* src, size_t bytes);
int mpsk_memcpy_d2h(mpsk_ctx* ctx, void* dst, const void* src, size_t bytes);
int mpsk_memcpy_d2d(mpsk_ctx* ctx, void* dst, const void* src, size_t bytes);

/* ---- MPO slice: SparseMPOSlice, src/operators/sparsempo/sparseslice.jl:13-27 ----------------
 * odim x odim blocks (column-major tables: entry (i,j) at i + odim*j).  chi_l[i] / chi_r[j] are
 * the MPO bond dimensions of level i (left) / j (right).  kind: MPSK_BLOCK_*.  scalars[i,j]: value of a
 * scalar block (c * identity, needs chi_l[i] == chi_r[j]).  blocks[i,j]: HOST pointer to a dense
 * block O[chi_l[i], d, d, chi_r[j]] column-major, index order [w, t(out), s(in), v]
 * (docs/src/man/intro.md:78-83, derivatives.jl:97), or NULL. */
int mpsk_mposlice_create(mpsk_ctx* ctx, int dtype, int odim, const int32_t* chi_l, const int32_t* chi_r,
                         int d, const int32_t* kind, const double* scalars, const void* const* blocks,
                         mpsk_mposlice** out);
/* Dense MPO slice: DenseMPO tensor of src/operators/densempo.jl:4-17 (the transfer tensor of a 2D partition function or
 * boundary-MPS contraction), O = HOST pointer to a [Wl, d, d, Wr] column-major tensor in the index order [w, t(out),
 * s(in), v] above: O(w,t,s,v) at w + Wl (t + d (s + d v)).  MPSK_F64 only (MPSK_C128: MPSK_ERR_INVALID).  The result is an
 * ordinary slice handle, accepted by every entry point that takes one; it is marked dense: mpsk_dAC, mpsk_hac_* (plain
 * vector layout), mpsk_transfer_left and mpsk_transfer_right run the middle contraction (w,s) -> (v,t) as ONE fp64 MFMA
 * GEMM [(row, col) x (s,w)] x [(s,w) x (t,v)] on intermediates laid out for it (workspace Dlo d Dr (Wl + Wr) doubles)
 * instead of the slab mix, once min(Wl, Wr) d >= 8 (below that the mix route is kept; environment MPSK_DENSE_ROUTE=1 / 0
 * forces the GEMM / mix route).  mpsk_dAC2, mpsk_dAC_blocked and blocked mpsk_hac_apply keep the mix route.  mpsk_hac_info:
 * mode 4 = dense GEMM route; below the crossover the slice is prepared exactly like the mpsk_mposlice_create slice of the
 * same O (mode 0 or 1); above it the right-combined fold (mode 1, Wl d^2 slabs) is never built. */
int mpsk_mposlice_create_dense(mpsk_ctx* ctx, int dtype, int Wl, int Wr, int d, const void* O, mpsk_mposlice** out);
int mpsk_mposlice_destroy(mpsk_mposlice* s);
int mpsk_mposlice_dims(const mpsk_mposlice* s, int* Wl, int* Wr, int* d);

/* ---- effective-Hamiltonian matvecs: src/algorithms/derivatives.jl ---------------------------
 * mpsk_dAC  == dAC(x, H::SparseMPOSlice, leftenv, rightenv)   derivatives.jl:77-104
 *   y[p,t,q] = sum GL[w][p,a] x[a,s,b] O[w,t,s,v] GR[v][b,q]
 *   GL: Wl slabs [Dlo, Dl]   (Dlo = number of output rows held by this rank; == Dl unsharded)
 *   GR: Wr slabs [Dr, Dr];  x: [Dl, d, Dr];  y: [Dlo, d, Dr]. */
int mpsk_dAC(mpsk_ctx* ctx, const mpsk_mposlice* H, int Dlo, int Dl, int Dr, const void* GL,
             const void* GR, const void* x, void* y);
/* The same matvec with x in the bond-sharded ("blocked") vector layout of the multi-GPU path: x is given
 * as nblk row blocks, block q = x[q Dl/nblk : (q+1) Dl/nblk, :, :] stored as a contiguous [Dl/nblk, d, Dr] tensor at
 * offset q (Dl/nblk) d Dr -- exactly what an all-gather of the ranks' output row blocks produces, so the Krylov vectors
 * of a sharded eigensolve never have to be re-interleaved.  y: [Dlo, d, Dr] (this rank's row block; the caller points
 * it INTO the blocked destination vector and all-gathers in place).  nblk == 1 is mpsk_dAC. */
int mpsk_dAC_blocked(mpsk_ctx* ctx, const mpsk_mposlice* H, int nblk, int Dlo, int Dl, int Dr, const void* GL,
                     const void* GR, const void* xblk, void* y);
/* Prepared effective Hamiltonian == the reference's MPO_ddAC object (derivatives.jl:11-15, 44-46): `ddAC(pos, psi, H, envs)`
 * builds it ONCE per site visit from (H[pos], leftenv, rightenv) and the Krylov solver applies it many times.
 * mpsk_hac_create folds the MPO tensor into the right environment (GRc[(w,s,t)] = sum_v O[w,t,s,v] GR[v], one
 * elementwise pass) whenever that does not cost extra GEMM work (Heisenberg / TFI-type MPOs): the application is then
 * TWO GEMM launches with no slab mix and one intermediate instead of two; otherwise it applies exactly what mpsk_dAC
 * does.  GL / GR must stay valid and unchanged while the object lives.  x may be in the blocked layout (nblk row
 * blocks, see mpsk_dAC_blocked; nblk = 1: plain).  mpsk_hac_info: mode 1 = combined environment (nslabs of them);
 * mode 4 = dense-slice GEMM route (mpsk_mposlice_create_dense).
 * The blocked layout (nblk > 1) is taken by MPSK_F64 operators in modes 0, 1 and 4; nblk must divide Dl and be at most 32
 * (MPSK_ERR_INVALID otherwise).  MPSK_C128 operators (mode 2, complex mode 3) and the real mode 3 take the plain layout only:
 * nblk > 1 returns MPSK_ERR_UNSUPPORTED and launches nothing. */
typedef struct mpsk_hac mpsk_hac;
int mpsk_hac_create(mpsk_ctx* ctx, const mpsk_mposlice* H, int Dlo, int Dl, int Dr, const void* GL, const void* GR,
                    mpsk_hac** out);
/* mpsk_hac_create with flags.  MPSK_HAC_CANONICAL: the caller guarantees that level 0 of GL and level W-1 of GR are
 * identities -- true for the environments of a finite chain in canonical form (FinEnv starts them as identities and
 * every update with an isometric AL / AR keeps them so, to the isometry error of the gauge step).  For a real slice in
 * Jordan form (levels 0 and W-1 of chi 1, O[0,0] = O[W-1,W-1] = 1, O[w,v] = 0 for w > 0, v < W-1: nothing enters level
 * 0, nothing leaves level W-1, no A blocks) and Dlo == Dl the operator is then prepared in mode 3:
 *   y[:,t,:] = sum_s x[:,s,:] GRc0[(s,t)] + sum_s GLc[(s,t)] x[:,s,:],
 *   GRc0[(s,t)] = sum_v O[0,t,s,v] GR[v]  (start level, C blocks, D block),  GLc[(s,t)] = sum_{w>0} O[w,t,s,W-1] GL[w],
 * both folded once at create time; an application is ONE GEMM launch (two when Dl != Dr) with no intermediate:
 * 2 d n D^3 flops (n = non-zero (s,t) slabs per t and family; Heisenberg: 16 D^3 against the 40 D^3 of mode 1).
 * Slices with A blocks (longer-range MPOs), complex slices and every other case keep the mode mpsk_hac_create picks.
 * Environment MPSK_HAC_CHECK=1 (debug, synchronises): a mode-3 candidate whose max|GL[0] - I| or max|GR[W-1] - I|
 * exceeds 1e-10 fails with MPSK_ERR_INVALID.  mpsk_hac_info: mode 3, nslabs = folded slabs (2 d^2). */
enum { MPSK_HAC_CANONICAL = 1, MPSK_HAC_CANONICAL_C128 = 2 };
/* MPSK_HAC_CANONICAL_C128: the same operator for a COMPLEX slice (MPSK_HAC_CANONICAL keeps its meaning and is still ignored
 * for complex slices).  Conditions: the slice is in Jordan form with exactly real identity corners (the complex twin of a
 * real Jordan-form slice, or one with complex B / C / D blocks), Dlo == Dl, and GL[0], GR[W-1] are identities -- checked on
 * the device at create time (one synchronisation; tolerance 1e-10).  The folds GRc0 / GLc are then built once, in complex
 * arithmetic, and an application is two launches on the complex GEMM family, 16 d^2 D^3 real flops (Heisenberg: 64 D^3
 * against the 160 D^3 of mode 2); mpsk_hac_info reports mode 3.  If a condition fails the operator is what
 * mpsk_hac_create prepares (mode 2), except under MPSK_HAC_CHECK=1, where non-canonical environments fail with
 * MPSK_ERR_INVALID as for the real mode.  The environments of the correction vector of a propagator sweep are its case
 * (src/algorithms/propagator/corvector.jl:52,66). */
int mpsk_hac_create_ex(mpsk_ctx* ctx, const mpsk_mposlice* H, int Dlo, int Dl, int Dr, const void* GL, const void* GR,
                       int flags, mpsk_hac** out);
int mpsk_hac_apply(mpsk_hac* h, const void* x, int nblk, void* y);
/* y = a0 x + a1 (H_AC x): the shifted operator KrylovKit's linsolve(H_AC, b, x0, alg, a0, a1) applies, as the dynamical-DMRG
 * site solves call it (src/algorithms/propagator/corvector.jl:68 with a0 = -z, :123 with a0 = |z|^2).  a0, a1: (re, im)
 * pairs; the imaginary parts are ignored for MPSK_F64 operators.  Every mode of mpsk_hac_apply, through mpsk_hac_apply
 * itself (same launches, same bits) followed by ONE fused vector pass over x and y; a0 = 0, a1 = 1 is mpsk_hac_apply bit
 * for bit.  x and y must not alias; a0 != 0 needs Dlo == Dl and nblk == 1. */
int mpsk_hac_apply_axpby(mpsk_hac* h, const double* a1, const void* x, int nblk, const double* a0, void* y);
/* Fixed-budget smallest-real eigensolve with the prepared operator in ONE call: V[0] = x0 / |x0|, m Krylov steps (apply,
 * CGS2 + normalise), Ritz step of the projected matrix on the device, y = normalised Ritz vector -- fixedpoint(H_AC, AC, :SR,
 * Arnoldi(; krylovdim = m, maxiter = 1)) of dmrg.jl:36 without a convergence test and without a host synchronisation.
 * V: HOST array of m + 2 device vectors of the operator's size; scal: device scratch, >= m (2m + 1) + 40 doubles;
 * first_image (optional): H (x0 / |x0|) as the first step produced it (what calc_galerkin of the old tensor needs,
 * toolbox.jl:18).  1 <= m <= 32, MPSK_F64 operators, unblocked vectors. */
int mpsk_hac_eigsolve_fixed(mpsk_hac* hac, const void* x0, int m, void* const* V, void* scal, void* y, void* first_image);
int mpsk_hac_destroy(mpsk_hac* h);
int mpsk_hac_info(const mpsk_hac* h, int* mode, int* nslabs);
/* Summed prepared operator: y = sum_k coefs[k] H_k x for n effective Hamiltonians of ONE site, 1 <= n <= 8 -- the
 * derivative of a LazySum of MultipliedOperators (derivatives.jl:283-323), whose coefficients change with the evaluation
 * time while the operators do not.  H, GL, GR: HOST arrays of n slices / left / right environments; the slices may differ
 * in W and in their block pattern and share d and dtype (else MPSK_ERR_INVALID).  `flags` are those of
 * mpsk_hac_create_ex, applied to every term.  The coefficients are REAL for both dtypes and start as 1.
 *   Route 1 (folded): every term is prepared in mode 3 under the flag (MPSK_HAC_CANONICAL for MPSK_F64,
 *   MPSK_HAC_CANONICAL_C128 with its device-side identity check for MPSK_C128; Jordan-form slice, Dlo == Dl).  Mode 3 is
 *   linear in its two folds, so the sum is ONE mode-3 operator with GRc0 = sum_k coefs[k] GRc0_k and GLc likewise:
 *   mpsk_hsum_set_coefs combines both fold buffers in one memory-bound launch (terms added in the order k = 0 .. n-1,
 *   bit-reproducible; the coefficients travel by value: no upload, no synchronisation), and an application is exactly the
 *   launches of one mode-3 mpsk_hac_apply of that dtype and shape, whatever n is.  The segment tables cover the union of
 *   the terms' non-zero (s,t) slabs; a term without a slab at some (s,t) contributes nothing there.  The per-term folds
 *   are KEPT, not recomputed from the environments (n 2 d^2 D^2 elements, folded once at create time), and the combined
 *   pair takes another 2 d^2 D^2; an application needs no workspace (complex: the planar copy of x, as mode 3 does).
 *   Route 2 (accumulated): everything else (non-canonical environments, slices with A blocks, infinite-MPS environments,
 *   Dlo != Dl).  The terms are applied one after another on their own preparation, term k with alpha = coefs[k] and, for
 *   k > 0, beta = 1 in its last GEMM stage: no vector pass and no temporary beyond the stage workspace the terms share.
 *   Every mode accumulates in its last stage, so no term falls back to mpsk_vaxpby.
 * mpsk_hsum_set_coefs: n host reals, copied before it returns; stream-ordered, so it may be called between applications;
 * a coefficient 0 is legal.  n == 1 with coefs = {1} is mpsk_hac_apply (nblk = 1) bit for bit on both routes.
 * mpsk_hsum_apply_axpby: y = a0 x + a1 (sum x), the application followed by the one fused pass of mpsk_hac_apply_axpby.
 * mpsk_hsum_info: route (1 / 2) and the GEMM launches of one application (route 2: summed over the terms).
 * GL / GR must stay valid and unchanged while the object lives; x and y must not alias. */
typedef struct mpsk_hsum mpsk_hsum;
int mpsk_hsum_create(mpsk_ctx* ctx, int n, const mpsk_mposlice* const* H, int Dlo, int Dl, int Dr,
                     const void* const* GL, const void* const* GR, int flags, mpsk_hsum** out);
int mpsk_hsum_set_coefs(mpsk_hsum* h, const double* coefs);
int mpsk_hsum_apply(mpsk_hsum* h, const void* x, void* y);
int mpsk_hsum_apply_axpby(mpsk_hsum* h, const double* a1, const void* x, const double* a0, void* y);
int mpsk_hsum_info(const mpsk_hsum* h, int* route, int* launches_per_apply);
int mpsk_hsum_destroy(mpsk_hsum* h);
/* mpsk_dC == dC(x, leftenv::Vector, rightenv::Vector)   derivatives.jl:171-193
 *   y[p,q] = sum_w GL[w][p,a] c[a,b] GR[w][b,q] */
int mpsk_dC(mpsk_ctx* ctx, int W, int Dlo, int Dl, int Dr, const void* GL, const void* GR,
            const void* c, void* y);
/* mpsk_dAC2 == dAC2(x, h1, h2, leftenv, rightenv)   derivatives.jl:119-158
 *   x2, y2: [Dl, d1, Dr, d2] with (d1, d2) the physical dims of H1 / H2 */
int mpsk_dAC2(mpsk_ctx* ctx, const mpsk_mposlice* H1, const mpsk_mposlice* H2, int Dlo, int Dl, int Dr,
              const void* GL, const void* GR, const void* x2, void* y2);

/* ---- projections on the tangent space of ANOTHER state: derivatives.jl:210-226 (ac_proj / ac2_proj), the site step of
 * approximate (src/algorithms/approximate/fvomps.jl).  The tensors of the state ABOVE are contracted with environments whose
 * bra legs belong to the state BELOW, so both environments are rectangular:
 *   GL: Wl slabs [Dlo, Dl]  (Dlo = left bond of the state below, Dl = of the state above)
 *   GR: Wr slabs [Dr, Dro]  column-major, slab stride Dr Dro  (Dr = right bond of the state above, Dro = of the state below)
 * mpsk_dAC_proj == ac_proj:  y[p,t,q] = sum GL[w][p,a] x[a,s,b] O[w,t,s,v] GR[v][b,q],  x: [Dl, d, Dr], y: [Dlo, d, Dro].
 *   Every route of mpsk_dAC: sparse slices (slab mix), dense slices above the crossover of mpsk_mposlice_create_dense
 *   (stage 2 as one MFMA GEMM; MPSK_DENSE_ROUTE honoured), MPSK_C128 slices (interleaved complex operands, planar copy of GR
 *   in the workspace).  The order of contraction is fixed, left first: 2 Wl d Dlo Dl Dr + 2 Wr d Dlo Dr Dro flops; workspace
 *   Dlo d Dr (Wl + Wr) doubles (twice that, plus the planes of x and GR, for complex).  Dro == Dr is mpsk_dAC bit for bit. */
int mpsk_dAC_proj(mpsk_ctx* ctx, const mpsk_mposlice* H, int Dlo, int Dl, int Dr, int Dro, const void* GL, const void* GR,
                  const void* x, void* y);
/* mpsk_dC_proj == c_proj (derivatives.jl:204-207), the zero-site map on the same rectangular environments:
 *   y[p,q] = sum_w GL[w][p,a] c[a,b] GR[w][b,q],  GL: W slabs [Dlo, Dl], GR: W slabs [Dr, Dro], c: [Dl, Dr], y: [Dlo, Dro].
 *   The order of contraction is fixed, left first: one batched fp64 MFMA GEMM T[w] = GL[w] c, then the segmented-K GEMM over
 *   (w, b) as mpsk_dC runs it: 2 W (Dlo Dl Dr + Dlo Dr Dro) flops; workspace W Dlo Dr doubles.  MPSK_F64 only: a ctx set to
 *   MPSK_C128 (mpsk_ctx_set_dtype) gets MPSK_ERR_UNSUPPORTED.  Dro == Dr is mpsk_dC bit for bit (same launches, same tiles). */
int mpsk_dC_proj(mpsk_ctx* ctx, int W, int Dlo, int Dl, int Dr, int Dro, const void* GL, const void* GR, const void* c,
                 void* y);
/* mpsk_dC_proj_c == c_proj on interleaved complex128 operands (the zero-site step of approximate on a complex uniform state):
 *   y[p,q] = sum_w GL[w][p,a] c[a,b] GR[w][b,q],  nothing conjugated;  GL: W slabs [Dlo, Dl], GR: W slabs [Dr, Dro] (slab
 *   stride Dr Dro complex elements), c: [Dl, Dr], y: [Dlo, Dro], all interleaved ComplexF64, 16-byte aligned.
 *   The rectangular form of the complex mpsk_dC: planes of c and GR in the workspace, one batched GEMM T[w] = GL[w] c on
 *   2 Dlo rows, then one segmented-K complex GEMM over (w, b) with N = Dro:  8 W (Dlo Dl Dr + Dlo Dr Dro) flops; workspace
 *   2 (Dl Dr + W Dr Dro) + 2 W Dlo Dr doubles (each plane rounded up to an even count).  Asynchronous on the ctx stream.
 *   The ctx must be set to MPSK_C128 (mpsk_ctx_set_dtype); an MPSK_F64 ctx gets MPSK_ERR_UNSUPPORTED.  Dro == Dr is mpsk_dC
 *   under MPSK_C128 bit for bit (same launches, same tiles). */
int mpsk_dC_proj_c(mpsk_ctx* ctx, int W, int Dlo, int Dl, int Dr, int Dro, const void* GL, const void* GR, const void* c,
                   void* y);
/* mpsk_dAC2_proj == ac2_proj applied to the two factors of the state above, AC [Dl, d1, Dm] and AR [Dm, d2, Dr] (as
 * mpsk_dAC2_product takes them); Y: [Dlo, d1, Dro, d2] (the layout of mpsk_dAC2's result).
 *   MPSK_F64: factorised through the middle bond, Y = sum_u Lhalf[u] Rhalf[u] with Lhalf[u] [Dlo, d1, Dm] and Rhalf[u]
 *   [Dm, d2, Dro] (the half contractions of mpsk_dAC2_product, shared with it), the product ONE GEMM launch with K = Wm Dm.
 *   The two-site tensor of the state above is never formed:
 *     flops ~ 2 Wl d1 Dlo Dl Dm + 2 Wr d2 Dm Dr Dro + 2 Wm d1 d2 Dlo Dro Dm   -- no D_above^3 d^2 term.
 *   Both slice kinds; workspace (Wl + Wm) d1 Dlo Dm + (Wr + Wm) d2 Dm Dro doubles.
 *   MPSK_C128: theta = AC AR (2 Dl d1 Dr d2 doubles) is built with d2 complex GEMMs in the ctx's expansion scratch -- the
 *   buffer mpsk_complement_tsvd uses for its operands, grown on demand, separate from the workspace -- and the rectangular
 *   form of the complex mpsk_dAC2 route runs on it (sparse slices; interleaved complex operands): workspace
 *   2 (Dl d1 Dr d2 + Wr Dr Dro) + 2 Dlo d1 Dr d2 (Wl + Wr) doubles, plus 4 Dl d1 Dm doubles of GEMM scratch. */
int mpsk_dAC2_proj(mpsk_ctx* ctx, const mpsk_mposlice* H1, const mpsk_mposlice* H2, int Dlo, int Dl, int Dm, int Dr, int Dro,
                   const void* GL, const void* GR, const void* AC, const void* AR, void* Y);

/* ---- bond expansion of a uniform state: src/algorithms/changebonds/optimalexpand.jl:16-67 --------------------------
 * mpsk_dAC2_product == dd-AC2(i, psi, H, envs) * (AC[i] * AR[i+1])   optimalexpand.jl:22-23 (MPOHamiltonian) and :51-52
 * (DenseMPO), derivatives.jl:119-158, WITHOUT forming the two-site tensor:
 *   Y[(a,t1), (b,t2)] = sum GL[w][a,a'] AC[a',s1,m] O1[w,t1,s1,u] O2[u,t2,s2,v] AR[m,s2,b'] GR[v][b',b]
 * factorised through the middle bond, Y = sum_u Lhalf[u] Rhalf[u] (each half = the first two stages of a one-site matvec
 * with the inner MPO leg u open; the product is one GEMM launch with K = Wm Dm).  GL: Wl slabs [Dl, Dl]; GR: Wr slabs
 * [Dr, Dr]; AC: [Dl, d1, Dm]; AR: [Dm, d2, Dr]; Y: [Dl, d1, Dr, d2] (the layout of mpsk_dAC2's result).  Both slice
 * kinds; a dense slice above the crossover of mpsk_mposlice_create_dense contracts its MPO tensor as an fp64 MFMA GEMM,
 * never as a slab mix.  Workspace: (Wl + Wm) d1 Dl Dm + (Wr + Wm) d2 Dm Dr doubles, no single intermediate above
 * max(Wl, Wm, Wr) d Dmax^2.  MPSK_F64 only: the complex Y of a bond expansion is mpsk_dAC2_proj under MPSK_C128 with
 * Dlo = Dl, Dro = Dr, which mpsk_complement_tsvd takes under MPSK_C128. */
int mpsk_dAC2_product(mpsk_ctx* ctx, const mpsk_mposlice* H1, const mpsk_mposlice* H2, int Dl, int Dm, int Dr,
                      const void* GL, const void* GR, const void* AC, const void* AR, void* Y);
/* mpsk_complement_tsvd == VL = leftnull(AL); VR = rightnull(AR); U, S, V = tsvd(VL' * Y * VR'; trunc = truncdim(k));
 * (VL * U, S, V * VR)   optimalexpand.jl:25-32, randexpand.jl:24-31 -- without the null-space bases, because
 * VL VL' = 1 - QL QL^T and VR' VR = 1 - QR^T QR.  Y: m x n (ldy); QL: m x pl, orthonormal columns; QR: pr x n,
 * orthonormal rows (pl = 0 / pr = 0: no projector on that side, the pointer may be NULL).  Returns the
 * *kept = min(k, m - pl, n - pr) leading singular triplets of X = (1 - QL QL^T) Y (1 - QR^T QR): U m x kept (ldu),
 * S kept doubles, descending, Vt kept x n (ldvt >= kept).  kept = 0 is a valid answer (nothing is written).
 *   S[j] = sigma_j(X) to 1e-10 S[0];  U^T U = 1, Vt Vt^T = 1, QL^T U = 0, Vt QR^T = 0 to 1e-12 BY CONSTRUCTION: after the
 *   SVD both factors are projected on the complement and re-orthonormalised (QRpos / LQpos), twice; directions the SVD
 *   cannot deliver (X = 0, rank(X) < kept) are completed inside the complement with S = 0.
 * Method: min(m, n) <= 64: mpsk_tsvd of X.  Otherwise the truncated split of mpsk_tsplit followed by the SVD of the
 * kept x kept core.  The split takes its checked subspace iteration only in svd mode 3 (mpsk_ctx_set_svd_mode), with
 * r = k + max(64, k / 2) within 5/8 of min(m, n), and not while the ctx backs off after a stage that gave up; in every
 * other case, and when the check fails, its full iteration runs on X (not mpsk_tsvd: the split needs the vectors of one
 * side only).  mpsk_ctx_split_stats describes that split.  mpsk_ctx_complement_stats: calls with a non-empty complement /
 * calls answered by the accepted subspace stage / all other calls (full iteration of the split, mpsk_tsvd of a small X,
 * X = 0); any pointer may be NULL.  Synchronises.
 *   MPSK_C128 (mpsk_ctx_set_dtype): Y, QL, QR, U, Vt interleaved complex128, column-major, leading dimensions in complex
 *   elements; S stays kept real doubles, descending.  Adjoint replaces transpose: X = (1 - QL QL^H) Y (1 - QR^H QR), and the
 *   contract reads U^H U = 1, Vt Vt^H = 1, QL^H U = 0, Vt QR^H = 0.  Everything else above carries over (kept, NULL sides,
 *   completion, refusals, synchronisation, the counters, non-finite Y).  Method: min(m, n) <= 64: the complex mpsk_tsvd of X.
 *   Otherwise, in svd mode 3 and while the ctx is not backing off, a truncated range finder on the interleaved tensors:
 *   r = min(k + max(64, k / 2), m - pl, n - pr) rows (rank(X) cannot exceed the complement, so the 5/8 cap of the fp64 split
 *   does not apply), structured random start, 4 rounds of  Z = W X^H, LQpos, B = Z X, LQpos,  the complex mpsk_tsvd of
 *   B = Z X (r x n), U = Z^H U_B.  X and X^H are the SECOND operands of the complex GEMM and are read as stored: only the
 *   r-row block is embedded, no 2m x 2n real copy of X or Y exists, a product costs 8 r m n flops (16 (pl + pr) m n for the
 *   projection, 64 r m n for the iteration).  The kept triplets are checked against X itself:
 *   |(1 - Z^H Z) X Vt^H|_F <= 1e-12 |X|_F (MPSK_SPLIT_TOL) -> counted under n_subspace; a failed check, a lower svd mode or
 *   a ctx that backs off (after a failed check: 4, 8, ... 64 calls) -> the complex mpsk_tsvd of X, counted under n_full.
 *   Singular values at or below 32 eps sqrt(m + n) max|Y_ij|, the rounding level of the projection, are returned as exactly
 *   0 and their directions completed inside the complement.  Scratch (the ctx's expansion scratch, in doubles, interleaved
 *   operands): 4 m n (X, X^H) + 2 min(m, n) n + 6 r max(m, n) + 2 r n + 4 r^2 + 2 k (2 m + n + r + k)
 *   + 2 max(pl n, pr m, pl k, k pr), plus what the complex GEMM, QRpos / LQpos and SVD take for themselves.
 *   The complex Y comes from mpsk_dAC2_proj (Dlo = Dl, Dro = Dr): mpsk_dAC2_product stays MPSK_F64 only. */
int mpsk_complement_tsvd(mpsk_ctx* ctx, int m, int n, const void* Y, int ldy, const void* QL, int ldql, int pl,
                         const void* QR, int ldqr, int pr, int k, void* U, int ldu, void* S, void* Vt, int ldvt, int* kept);
int mpsk_ctx_complement_stats(mpsk_ctx* ctx, long* n_calls, long* n_subspace, long* n_full);

/* ---- transfer matrices / environment updates: src/transfermatrix/transfer.jl ---------------
 * mpsk_transfer_left == transfer_left(vec, ham::SparseMPOSlice, A, Ab)   transfer.jl:166-211
 *   GLout[v][q,b] = sum GLin[w][p,a] A[a,s,b] O[w,t,s,v] conj(Ab[p,t,q])
 *   GLin: Wl slabs [Dlb, Dl]; A: [Dl,d,Dr]; Ab: [Dlb,d,Drb]; GLout: Wr slabs [Drb, Dr]
 * mpsk_transfer_right == transfer_right(vec, ham, A, Ab)                  transfer.jl:212-259
 *   GRout[w][a,p] = sum A[a,s,b] O[w,t,s,v] conj(Ab[p,t,q]) GRin[v][b,q]
 *   GRin: Wr slabs [Dr, Drb]; GRout: Wl slabs [Dl, Dlb]
 * H == NULL: pass-through legs, W independent slabs (transfer.jl:18-25,38-45,66-75). */
int mpsk_transfer_left(mpsk_ctx* ctx, const mpsk_mposlice* H, int W, int d, int Dl, int Dr, int Dlb,
                       int Drb, const void* GLin, const void* A, const void* Ab, void* GLout);
int mpsk_transfer_right(mpsk_ctx* ctx, const mpsk_mposlice* H, int W, int d, int Dl, int Dr, int Dlb,
                        int Drb, const void* A, const void* Ab, const void* GRin, void* GRout);
/* ---- local measurements: src/algorithms/expval.jl:23-37, src/algorithms/correlators.jl:10-43 ----
 * mpsk_site_gram: the Gram matrix over the physical index of two site tensors,
 *   dev_out[w][t,s] = sum_{p,b} conj(Ab[p,t,b]) X[w][p,s,b]
 *   X: W tensors [Dl,d,Dr], contiguous; Ab: [Dl,d,Dr]; dev_out: W column-major d x d matrices (t fastest) in DEVICE memory.
 *   X = Ab = AC, W = 1 is the one-site reduced density matrix: <O> = sum_{t,s} O[t,s] dev_out[t,s] for every one-site
 *   operator of that site (expval.jl:23-37).  One pass over X and Ab for d <= 4 (ceil(d/4) passes above), O(d^2 Dl Dr)
 *   flops.  Asynchronous on the ctx stream, nothing is copied to the host.  Follows mpsk_ctx_set_dtype: under MPSK_C128
 *   all three arrays are interleaved complex; under MPSK_F64 the conj does nothing.  The reduction takes a fixed order
 *   (per-thread partial sums, wavefront reduction, one final reduction launch, no atomics): bit-identical from run to run.
 *   Workspace: W d^2 1024 doubles (twice that for MPSK_C128).
 * mpsk_transfer_left_gram: one site of correlator(psi, O1, O2, i, js) (correlators.jl:25-38): the pass-through
 *   (H == NULL) mpsk_transfer_left together with the site Gram of its stage-1 product T1[w][p,s,b] = sum_a Vin[w][p,a] A[a,s,b],
 *   dev_gram[w][t,s] = sum Vin[w][p,a] A[a,s,b] conj(Ab[p,t,b])       (= mpsk_site_gram(T1, Ab); needs Dr == Drb)
 *   so that the closing contraction with O2, sum_{w,t,s} O2[w,t,s] dev_gram[w][t,s], costs no second pair of GEMMs.
 *   Vin: W slabs [Dlb, Dl]; A: [Dl,d,Dr]; Ab: [Dlb,d,Drb]; Vout: W slabs [Drb, Dr], bit for bit what
 *   mpsk_transfer_left(ctx, NULL, W, ...) writes (the same GEMM calls), or NULL for the last site of a range: stage 2 is
 *   then skipped.  dev_gram: W column-major d x d matrices in DEVICE memory.  Asynchronous; follows the ctx dtype.
 *   Dr != Drb: MPSK_ERR_INVALID. */
int mpsk_site_gram(mpsk_ctx* ctx, int W, int d, int Dl, int Dr, const void* X, const void* Ab, void* dev_out);
int mpsk_transfer_left_gram(mpsk_ctx* ctx, int W, int d, int Dl, int Dr, int Dlb, int Drb, const void* Vin, const void* A,
                            const void* Ab, void* Vout, void* dev_gram);
/* mpsk_transfer_left_gram_env: one site of the matrix elements <bra| O_j |ket> between two DIFFERENT states that share their
 * environments (WindowMPS, window.transition): everything to the right of the site does not close to an identity but to
 * a matrix R[b,q] ([Dr, Drb], ket index first), carried from the right by pass-through transfers.
 *   dev_gram[t,s] = sum conj(Ab[p,t,q]) Lin[p,a] A[a,s,b] R[b,q]          <bra| O_j |ket> = sum O[t,s] dev_gram[t,s]
 *   Lin: [Dlb, Dl]; A: [Dl,d,Dr] (the ket's tensor at j); Ab: [Dlb,d,Drb] (the bra's); dev_gram: one column-major d x d
 *   matrix in DEVICE memory, t fastest (interleaved under MPSK_C128).
 *   Lout: [Drb, Dr], bit for bit what mpsk_transfer_left(ctx, NULL, 1, ...) writes on (Lin, A, Ab) (the same stage calls),
 *   or NULL on the last site: stage 2 is then skipped; dev_gram does not depend on it.
 * The stage-1 product T1 = Lin A is computed once and shared by the transfer and the Gram.  The closing product T1 R is a
 * GEMM over the Dr index whose MFMA accumulator tiles are contracted in the epilogue with the matching tiles of conj(Ab)
 * over (p, q): wavefront reduction, per-workgroup partials, one fixed-order final reduction, no atomics -- the product
 * itself is never written to memory, and results are bit-identical from run to run.  Asynchronous; follows the ctx dtype
 * (MPSK_F64, MPSK_C128).  d <= 64 (MPSK_ERR_INVALID above).  Workspace: that of mpsk_transfer_left plus d^2 1024 doubles
 * (MPSK_C128: twice that, and 2 Dr Drb for the planes of R). */
int mpsk_transfer_left_gram_env(mpsk_ctx* ctx, int d, int Dl, int Dr, int Dlb, int Drb, const void* Lin, const void* A,
                                const void* Ab, const void* R, void* Lout, void* dev_gram);
/* The transfers with flags.  MPSK_TRANSFER_CANONICAL: the caller guarantees that level 0 of GLin (mpsk_transfer_left_ex) /
 * level W-1 of GRin (mpsk_transfer_right_ex) is the identity and that A == Ab is an isometry on the contracted side
 * (sum_{p,t} A[p,t,q] A[p,t,b] = delta_qb, resp. sum_{t,b} A[a,t,b] A[p,t,b] = delta_ap) -- the environment update of a finite
 * chain in canonical form (FinEnv).  For a real slice in Jordan form (see mpsk_hac_create_ex) given with A and Ab the same
 * pointer, the identity level of the result is then WRITTEN (exactly the identity, Dr x Dr resp. Dl x Dl), the interior
 * levels come from the C (resp. B) blocks applied to A in one elementwise pass, and the finished level from the fold of
 * mpsk_hac mode 3 applied to A: no stage-1 GEMM on any level, 2 d n D^3 + 2 d (W-1) D^3 flops instead of 4 d W D^3
 * (Heisenberg: 24 D^3 instead of 40 D^3).  Everything else -- flag not set, slices with A blocks, dense-MPO slices,
 * MPSK_C128, H == NULL, A != Ab -- is mpsk_transfer_left / mpsk_transfer_right bit for bit; so is every call under
 * environment MPSK_TRANSFER_MODE=0.  Workspace: d^2 D^2 + (W-1) d Dl Dr doubles.  MPSK_HAC_CHECK=1 (debug, synchronises):
 * a canonical-route call whose input identity level or Gram matrix of A is off by more than 1e-10 fails with
 * MPSK_ERR_INVALID. */
enum { MPSK_TRANSFER_CANONICAL = 1 };
int mpsk_transfer_left_ex(mpsk_ctx* ctx, const mpsk_mposlice* H, int W, int d, int Dl, int Dr, int Dlb, int Drb,
                          const void* GLin, const void* A, const void* Ab, int flags, void* GLout);
int mpsk_transfer_right_ex(mpsk_ctx* ctx, const mpsk_mposlice* H, int W, int d, int Dl, int Dr, int Dlb, int Drb,
                           const void* A, const void* Ab, const void* GRin, int flags, void* GRout);
/* Pair-Gram route of the canonical transfers.  The levels that receive from the identity level alone are combinations of
 * a few products of the site tensor with itself, GLout[v] = sum_{t,s} O[0,t,s,v] P_ts with P_ts = A[:,t,:]^T A[:,s,:] and
 * P_st = P_ts^T (right: GRout[w] = sum O[w,t,s,W-1] Q_st, Q_st = A[:,s,:] A[:,t,:]^T).  Where a flop-and-launch model says
 * it pays (Heisenberg S = 1/2: from D ~ 350), a canonical-route call computes the unordered pairs {t,s} that carry a
 * coefficient in ONE batched launch (symmetric products P_tt: upper block triangle only), one elementwise kernel writes the
 * interior levels (and the D-block term of the finished level) from them, and the finished level is a single GEMM of the
 * fold application: Heisenberg 24 -> ~16 D^3.  Workspace d^2 D^2 + d Dl Dr + pairs n^2 doubles (n = Dr left, Dl right).
 * Environment MPSK_TRANSFER_MODE, read per call: 0 dense route, 1 the level-by-level canonical route, 2 the pair-Gram
 * route wherever the slice has pairs, unset: the model.
 * mpsk_ctx_transfer_stats: canonical transfers of this ctx that took the pair-Gram route.
 * mpsk_transfer_pair_model: host only (no ctx, no device) -- what mpsk_mposlice_create records for a Jordan-form slice
 * given as the dense tensor O[Wl, d, d, Wr] (column-major, index (w,t,s,v)) and what the model chooses at (Dl, Dr); every
 * output is an int[2] = {transfer_left, transfer_right} or NULL: pairs, the symmetric ones among them, output levels of the
 * combination kernel, route (1 pair-Gram, 0 level by level). */
int mpsk_ctx_transfer_stats(mpsk_ctx* ctx, long* n_pair);
int mpsk_transfer_pair_model(int Wl, int Wr, int d, const double* O, int Dl, int Dr, int* pairs, int* diagonal, int* levels,
                             int* route);
/* ---- quasiparticle excitations of a transfer matrix: quasiparticleexcitation.jl:258-293 (the local term of the effective
 * operator) and qpenv.jl:238-251 (the updates of lB / rB).  MPSK_F64 only: a MPSK_C128 slice or ctx gets
 * MPSK_ERR_UNSUPPORTED.  Both slice kinds: sparse slices (slab mix) and dense slices on both sides of the crossover of
 * mpsk_mposlice_create_dense (MPSK_DENSE_ROUTE honoured).  All entries are built from the stages of mpsk_dAC_proj and of
 * the transfers; no new kernel.
 * mpsk_qp_apply:   y[p,t,q] = sum GL[w][p,a] B[a,s,b]  O[w,t,s,v] GR[v][b,q]        B in the centre      :273-276
 *                           + sum lB[w][p,c] AR[c,s,b] O[w,t,s,v] GR[v][b,q]        B further left       :278-281
 *                           + sum GL[w][p,a] AL[a,s,e] O[w,t,s,v] rB[v][e,q]        B further right      :283-286
 *   GL: Wl slabs [Dlo, Dl]; GR: Wr slabs [Dr, Dro]; B: [Dl, d, Dr]; lB: Wl slabs [Dlo, Dl2]; AR: [Dl2, d, Dr];
 *   rB: Wr slabs [Dr2, Dro]; y: [Dlo, d, Dro].  The third term enters through `half`, stages 1 and 2 of (GL, AL [Dl, d, Dr2]):
 *   it does not depend on B, so mpsk_qp_half computes it once per site into a caller-owned device buffer of
 *   mpsk_qp_half_size doubles (= Wr d Dlo Dr2; its layout is that of the stage-2 result of the route the slice takes, so a
 *   buffer is valid for the slice and the setting of MPSK_DENSE_ROUTE it was made with).  mpsk_qp_apply only reads it.
 *   The pair (lB, AR) and the pair (half, rB) may each be NULL (both members).  With both NULL the call is mpsk_dAC_proj
 *   bit for bit (same launches, same tiles).  Stage 1 of the second term is a GEMM that accumulates (beta = 1) into the
 *   stage-1 buffer of the first; the third term is a second segmented-K GEMM that accumulates into y.
 *   flops: 2 Wl d Dlo (Dl + Dl2) Dr + 2 Wr d Dlo (Dr + Dr2) Dro (+ the MPO stage, once) against three times
 *   2 Wl d Dlo Dl Dr + 2 Wr d Dlo Dr Dro (+ three MPO stages) composed; mpsk_qp_half: 2 Wl d Dlo Dl Dr2 + the MPO stage.
 *   Workspace: Dlo d Dr (Wl + Wr) doubles (mpsk_qp_half: Dlo d Dr2 Wl). */
int mpsk_qp_half_size(const mpsk_mposlice* H, int Dlo, int Dr2, size_t* doubles);
int mpsk_qp_half(mpsk_ctx* ctx, const mpsk_mposlice* H, int Dlo, int Dl, int Dr2, const void* GL, const void* A, void* half);
int mpsk_qp_apply(mpsk_ctx* ctx, const mpsk_mposlice* H, int Dlo, int Dl, int Dl2, int Dr, int Dr2, int Dro, const void* GL,
                  const void* GR, const void* B, const void* lB, const void* AR, const void* half, const void* rB, void* y);
/* The pair transfers (qpenv.jl:238-251): out = T(V1; A1, O, Ab) + T(V2; A2, O, Ab), two transfers through the same O and the
 * same bra Ab whose kets and environments differ.  Stage 1 runs twice, the second product accumulating into the first
 * one's buffer; stages 2 and 3 run once.  Layouts as mpsk_transfer_left_ex / mpsk_transfer_right_ex without flags:
 *   left:  V1: Wl slabs [Dlb, Dl1], A1: [Dl1, d, Dr]; V2: Wl slabs [Dlb, Dl2], A2: [Dl2, d, Dr]; Ab: [Dlb, d, Drb];
 *          out: Wr slabs [Drb, Dr].   flops 2 Wl d Dlb (Dl1 + Dl2) Dr + 2 Wr d Dlb Dr Drb; workspace Dlb d Dr (Wl + Wr).
 *   right: A1: [Dl, d, Dr1], V1: Wr slabs [Dr1, Drb]; A2: [Dl, d, Dr2], V2: Wr slabs [Dr2, Drb]; Ab: [Dlb, d, Drb];
 *          out: Wl slabs [Dl, Dlb].   The ket is contracted first (the order of the right half of mpsk_dAC2_product), so
 *          that both terms meet in one intermediate [Dl, d, Drb]: flops 2 Wr d Dl (Dr1 + Dr2) Drb + 2 Wl d Dl Drb Dlb;
 *          workspace Dl d Drb (Wl + Wr).  (mpsk_transfer_right contracts the bra first: with V2 = 0 the results agree to
 *          rounding, not bit for bit.)
 * H is required. */
int mpsk_transfer_left_pair(mpsk_ctx* ctx, const mpsk_mposlice* H, int Dl1, int Dl2, int Dr, int Dlb, int Drb, const void* V1,
                            const void* A1, const void* V2, const void* A2, const void* Ab, void* out);
int mpsk_transfer_right_pair(mpsk_ctx* ctx, const mpsk_mposlice* H, int Dl, int Dr1, int Dr2, int Dlb, int Drb, const void* A1,
                             const void* V1, const void* A2, const void* V2, const void* Ab, void* out);
/* ---- quasiparticle excitations of a Hamiltonian: one site and one real part of effective_excitation_hamiltonian in the left
 * gauge (quasiparticleexcitation.jl:254-328, quasiparticle_state.jl:95-104).  MPSK_F64 only (MPSK_ERR_UNSUPPORTED otherwise).
 * mpsk_qp_heff_site:   Xout[n,q] = sum_{p,t} VL[(p,t),n] y[p,t,q] - E X[n,q],
 *                      y = mpsk_qp_apply(GL, GR, B = VL X, lB, AR, half, rB)  with Dlo = Dl and Dro = Dr.
 *   VL: [Dl d, Dl d - DrL], orthonormal columns (the complement of AL [Dl, d, DrL]); X, Xout: [Dl d - DrL, Dr]; GL: Wl slabs
 *   [Dl, Dl]; GR: Wr slabs [Dr, Dr]; lB: Wl slabs [Dl, Dl2]; AR: [Dl2, d, Dr]; half: mpsk_qp_half(H, Dl, Dl, Dr2, GL, AL);
 *   rB: Wr slabs [Dr2, Dr].  The pairs (lB, AR) and (half, rB) may each be NULL (both members).  -E X stands for -E B pulled
 *   back (VL^T B = X), so B is never scaled: B = VL X is one GEMM into the workspace, the three terms run through the stages
 *   of mpsk_qp_apply into the workspace, and the pull-back is one GEMM C = A^T Y + gamma Z whose store path reads X and
 *   writes Xout -- no pass over the result, no copy of X.  Xout must not alias X; X and half are only read.  An empty
 *   complement (Dl d == DrL) returns MPSK_OK and writes nothing.  Fixed summation order: bit-reproducible.
 *   flops: those of mpsk_qp_apply + 4 (Dl d)(Dl d - DrL) Dr.  Workspace: Dl d Dr (Wl + Wr + 2) doubles. */
int mpsk_qp_heff_site(mpsk_ctx* ctx, const mpsk_mposlice* H, int Dl, int DrL, int Dr, int Dl2, int Dr2, const void* GL,
                      const void* GR, const void* VL, const void* X, double E, const void* lB, const void* AR, const void* half,
                      const void* rB, void* Xout);
/* regularize!(v, lvec, rvec)   src/transfermatrix/transfermatrix.jl:70-76
 *   v[w] -= <lvec^T, v[w]> * rvec  for each of the W slabs [D1, D2]; lvec: [D2, D1]; rvec: [D1, D2] */
int mpsk_regularize(mpsk_ctx* ctx, int W, int D1, int D2, void* v, const void* lvec, const void* rvec);
/* The regulariser fused with the sum a GMRES step on (1 - T_reg) needs (mpohaminfenv.jl:95, :146), for both dtypes:
 *   coef_w = sum_{p,q} lvec[q,p] y[w][p,q]             (bilinear: NO conjugate, transfermatrix.jl:70-76)
 *   out[w] = a0 x[w] + a1 (y[w] - coef_w rvec)          w = 0 .. W-1
 * y, x, out: W slabs [D1, D2]; lvec: [D2, D1]; rvec: [D1, D2]; column-major.  Follows mpsk_ctx_set_dtype: under MPSK_C128
 * every array is interleaved complex and coef_w is a complex number; a0 and a1 stay real doubles (the solve needs 1 and -1).
 * x == NULL drops the a0 x term (a0 is not read).  out may alias y or x.  With x == NULL, a1 = 1 and out == y this is
 * regularize! in place: the complex twin of mpsk_regularize.
 * Two launches on the ctx stream, asynchronous, no atomics, nothing written to the host: a tiled dot (the lvec tile is
 * transposed through LDS so that both reads coalesce) whose per-tile partials go to the ctx workspace, one (re, im) pair per
 * tile for complex operands; then one pass in which every workgroup sums the partials of its slab in the same fixed order
 * and writes its part of out.  Bit-identical from run to run.  Workspace: W ceil(D1 / 32) ceil(D2 / 32) doubles, twice that
 * for MPSK_C128.  MPSK_ERR_INVALID: a dimension < 1, W > 65535, NULL y / lvec / rvec / out. */
int mpsk_regularize_axpby(mpsk_ctx* ctx, int W, int D1, int D2, const void* y, const void* lvec, const void* rvec, double a1,
                          const void* x, double a0, void* out);

/* ---- gauge steps: TensorKit leftorth!(QRpos) / rightorth!(LQpos) / tsvd! ----------------------
 * call sites: src/states/orthoview.jl:52,56 ; finitemps.jl:149 ; ortho.jl:128-136 ; dmrg.jl:96 */
/* A (m x n, m >= n, lda) = Q (m x n, ldq) * R (n x n upper, ldr), diag(R) > 0.  A is not modified.
 * Row limit: a call that takes the blocked Householder route -- every call with n <= 64 (complex: n <= 32), qr mode 1, and
 * the last fallback of the CholeskyQR ladder -- needs m <= 19712 (complex: m <= 9856, the embedding doubles the rows): one
 * panel column has to fit the LDS.  Above it the call fails with MPSK_ERR_INVALID.  The limit reaches
 * mpsk_qrpos2, mpsk_qrlq_pair and mpsk_lqpos (there: n <= 19712 columns) through the same route. */
int mpsk_qrpos(mpsk_ctx* ctx, int m, int n, const void* A, int lda, void* Q, int ldq, void* R, int ldr);
/* two independent QRpos of equal shape issued together (two streams inside the ctx): the sweep needs
 * leftorth of the old AC (toolbox.jl:17-22) and of the new AC (orthoview.jl:56) at the same moment */
int mpsk_qrpos2(mpsk_ctx* ctx, int m, int n, const void* A1, int lda1, void* Q1, int ldq1, void* R1, int ldr1,
                const void* A2, int lda2, void* Q2, int ldq2, void* R2, int ldr2);
/* QRpos of A1 (m x n) and LQpos of A2 (n x m: A2 = L2 Q2, L2 n x n lower, Q2 n x m) issued together: the
 * left-moving site update needs leftorth of the old AC (toolbox.jl:17-22) and rightorth of the new AC
 * (orthoview.jl:52) at the same moment */
int mpsk_qrlq_pair(mpsk_ctx* ctx, int m, int n, const void* A1, int lda1, void* Q1, int ldq1, void* R1, int ldr1,
                   const void* A2, int lda2, void* L2, int ldl2, void* Q2, int ldq2);
/* A (m x n, m <= n) = L (m x m lower) * Q (m x n), diag(L) > 0 */
int mpsk_lqpos(mpsk_ctx* ctx, int m, int n, const void* A, int lda, void* L, int ldl, void* Q, int ldq);
/* Deferred completion of a gauge step.  After mpsk_ctx_qr_defer the NEXT mpsk_qrpos2 / mpsk_lqpos call on the ctx that
 * takes the CholeskyQR3 path returns as soon as its launches are enqueued: Q / R of mpsk_qrpos2 are speculative, L / Q of
 * mpsk_lqpos not yet written, until mpsk_qr_commit has read the device's success flag (and run the repeated third pass /
 * the fallbacks where it asks for them).  *redone: bit 0 / bit 1 = the first / second factorization of the pair was
 * corrected after its enqueue -- whatever was computed from the speculative factor has to be recomputed.  Between the
 * two calls only entry points that do not use the ctx workspace are accepted (mpsk_gemm, mpsk_v*): the DMRG sweep
 * enqueues the galerkin evaluation of the site there (toolbox.jl:17-22), so the stream has work while the host waits.
 * A deferral armed before a call that does NOT take the CholeskyQR3 path -- the sequential branch of mpsk_qrpos2 (qr mode 1
 * or n <= 64), mpsk_lqpos with qr mode 1 or m <= 64, mpsk_qrpos, mpsk_qrlq_pair -- is consumed by that call, which
 * completes at once: its outputs are final when it returns, nothing is pending, and mpsk_qr_commit returns *redone = 0. */
int mpsk_ctx_qr_defer(mpsk_ctx* ctx);
/* Side stream: mpsk_ctx_side_mark records "now" on the ctx stream; after mpsk_ctx_side_begin every mpsk_* call of the ctx
 * runs on its second stream, ordered after the mark only; mpsk_ctx_side_end switches back and makes the main stream wait
 * for the side work.  Workspace users and the calls that use the second stream themselves (mpsk_qrpos2, mpsk_qrlq_pair,
 * mpsk_tsplit) are refused in between.  The sweep runs the galerkin evaluation of a left-moving visit there, under the
 * latency-bound CholeskyQR chain of the LQ step it has just enqueued on the main stream. */
int mpsk_ctx_side_mark(mpsk_ctx* ctx);
int mpsk_ctx_side_begin(mpsk_ctx* ctx);
int mpsk_ctx_side_end(mpsk_ctx* ctx);
int mpsk_qr_commit(mpsk_ctx* ctx, int* redone);
/* thin SVD of theta (m x n): theta = U diag(S) Vh, S descending.  U: m x kmax, S: kmax, Vh: kmax x n
 * buffers with kmax = min(m, n).  Truncation (TensorKit truncdim & truncerr, dmrg.jl:75,96):
 * keep at most max_keep (<= 0: no limit) values and drop the tail while ||S_dropped||_2 <= trunc_err -- an ABSOLUTE
 * bound, as TensorKit 0.12's truncerr(eps) (p = 2) applies it [restated from the published TensorKit source, which the
 * reference does not vendor: parity unpinned; equal to the relative rule for the normalised theta of DMRG2 / IDMRG2 /
 * real-time TDVP2].  *kept / *disc_norm are written on the host (sync).
 * Returns MPSK_ERR_HIP with "did not converge" if the Jacobi iteration is not orthogonal to 1e-9 after 40 sweeps;
 * trunc_err < 0 is MPSK_ERR_INVALID.
 * MPSK_C128 (mpsk_ctx_set_dtype): theta, U, Vh interleaved complex (ldt / ldu / ldv in complex elements), S kmax real
 * doubles, descending; theta = U diag(S) Vh with Vh = V^H.  The truncation counts every complex value once.
 * Rank-deficient input (MPSK_C128): a zero singular value gets a ZERO vector on one side (the side the Jacobi normalises
 * by 1 / sigma) and a vector of an orthonormal completion on the other.  The zero is the column of U when m >= n and
 * min(m, n) <= 64, or m < n and min(m, n) > 64; otherwise it is the row of Vh. */
int mpsk_tsvd(mpsk_ctx* ctx, int m, int n, const void* theta, int ldt, void* U, int ldu, void* S, void* Vh,
              int ldv, int max_keep, double trunc_err, int* kept, double* disc_norm);
/* Truncated two-site split theta (m x n, min(m, n) > 64) ~ AL (m x k) . C (k x k) . AR (k x n): what dmrg.jl:96-104 /
 * tdvp.jl:124-126 build from tsvd! (al, c, ar), with the same truncation arguments as mpsk_tsvd, but computed without
 * accumulating the Jacobi rotations (a third less memory traffic per round): AL, AR are isometries to rounding,
 * AL C AR = theta projected on the kept singular subspace, C is TRIANGULAR instead of diag(S) -- lower or upper depending on
 * the orientation and on the svd mode (mode 2 delivers the left vectors of the tall orientation, the other factor comes from
 * an LQpos); S (min(m, n) doubles) receives all singular values (svd mode 3: see mpsk_ctx_set_svd_mode), *kept = k.
 * Buffers: AL m x min(m,n), C min(m,n)^2, AR min(m,n) x n (only the leading k columns / rows are written).
 * Any scale: a theta whose largest entry is outside [1e-100, 1e100] is split as theta / max|theta_ij| (C, S, disc_norm scaled
 * back); theta = 0 returns C = 0 with identity isometries.
 * MPSK_C128: interleaved complex operands (leading dimensions in complex elements), C lower triangular with a real positive
 * diagonal.  trunc_err = 0: truncdim only, S receives the k kept values (the rest NaN).  trunc_err > 0: k = the smaller of
 * the max_keep and truncerr results of the complex mpsk_tsvd, S receives all min(m, n) values, *disc_norm = the 2-norm of
 * the discarded complex values; any min(m, n) >= 1.  trunc_err < 0: MPSK_ERR_INVALID. */
int mpsk_tsplit(mpsk_ctx* ctx, int m, int n, const void* theta, int ldt, int max_keep, double trunc_err,
                void* AL, int ldal, void* C, int ldc, void* AR, int ldar, void* S, int* kept, double* disc_norm);
/* Interleaved complex matrix (m x n complex: 2m x n doubles, ldh in doubles) <-> its real 2m x 2n embedding
 * E[:, 2b] = h_b, E[:, 2b+1] = J h_b, one launch each.  mpsk_cx_half takes the STRUCTURED PART of a nearly embedded matrix
 * (re = (E00 + E11) / 2, im = (E10 - E01) / 2 per 2 x 2 block).  For hosts that keep complex tensors bond-embedded
 * (mpskit.jl_amd/cplx.py) and iterate their Krylov solvers on interleaved vectors. */
int mpsk_cx_embed(mpsk_ctx* ctx, int m, int n, const void* H, int64_t ldh, void* E, int64_t lde);
int mpsk_cx_half(mpsk_ctx* ctx, int m, int n, const void* E, int64_t lde, void* H, int64_t ldh);
/* general column-major product C = alpha op(A) op(B) + beta C for the small gauge products
 * AC = AL*C, AC = C*AR, theta = AC*AR, AL = Q_AC*Q_C'  (orthoview.jl:99,103; dmrg.jl:92; ortho.jl:130) */
int mpsk_gemm(mpsk_ctx* ctx, int transA, int transB, int M, int N, int K, double alpha, const void* A,
              int64_t lda, const void* B, int64_t ldb, double beta, void* C, int64_t ldc);

/* Paired column-scaled product: the retraction, transport and preconditioner of the Grassmann gradient optimiser
 * (src/algorithms/grassmann.jl:154-205 retract / transport!, :227-235 the regularised rho^-1), which the reference takes
 * from TensorKitManifolds' Grassmann.retract / Grassmann.transport! on the SVD Z = U S Vt of the direction at base W:
 *   out1 = beta1 out1 + (P diag(a1) + Q diag(b1)) B
 *   out2 = beta2 out2 + (P diag(a2) + Q diag(b2)) B          (out2 == NULL: not computed)
 * P, Q: M x K (ldp, ldq), B: K x N (ldb), out1 / out2: M x N (ld1, ld2), all column-major and not transposed; leading
 * dimensions are independent of the row counts.  coef: device matrix of four rows a1, b1, a2, b2 of length K, row r at
 * coef + r ldcoef (what mpsk_grassmann_coef writes with ldcoef = K).  Q == NULL drops the Q terms (rows b1 / b2 are
 * not read); without out2 rows a2 / b2 are not read.  beta == 0 never reads the output.  The column scaling and the
 * P / Q combination happen while the A tile is staged into LDS in front of v_mfma_f64_16x16x4_f64; P and Q are read once
 * for both outputs.  One launch, no workspace, ascending k inside one workgroup per output tile: results are bit-identical
 * from run to run.  Outputs must not alias the operands.  mpsk_ctx_force_tile applies.  MPSK_F64 only: a ctx set to
 * MPSK_C128 gets MPSK_ERR_UNSUPPORTED. */
int mpsk_gemm_pair(mpsk_ctx* ctx, int M, int N, int K, const void* P, int64_t ldp, const void* Q, int64_t ldq,
                   const void* B, int64_t ldb, const void* coef, int64_t ldcoef, double beta1, void* out1, int64_t ld1,
                   double beta2, void* out2, int64_t ld2);
/* Site step of the sum of two finite MPS (src/states/finitemps.jl:397-408 the left half, :423-435 the right half): the
 * carried gauge factor times the direct sum of the two states' site tensors, written as the direct-sum tensor itself.  The
 * isometries F1 / F2 of the reference are never formed: they are the block offsets below.  A1: [D1, d, E1], A2: [D2, d, E2],
 * column-major with the first index fastest, contiguous.
 *   MPSK_DSUM_LEFT   G: [Dn, D1 + D2] (ldg), out: [Dn, d, E1 + E2]
 *                    out[:, :, :E1] = G[:, :D1] A1,  out[:, :, E1:] = G[:, D1:] A2     (two contiguous halves of out)
 *   MPSK_DSUM_RIGHT  G: [E1 + E2, Dn] (ldg), out: [D1 + D2, d, Dn]
 *                    out[:D1, s, :] = A1[:, s, :] G[:E1, :],  out[D1:, s, :] = A2[:, s, :] G[E1:, :]
 *                    (the two blocks interleave along the fastest index of out: no mpsk_gemm call writes that layout)
 * The boundary sites are D1 = D2 = Dn = 1 with G = [1 1] on the left, and E1 = E2 = Dn = 1 with G = [1; 1] on the right.
 * One launch: the tile list holds both block products (a grouped GEMM on v_mfma_f64_16x16x4_f64, operands staged through
 * LDS as in mpsk_gemm), one workgroup per output tile, ascending k, no atomics and no workspace: results are bit-identical
 * from run to run.  Partial tiles are guarded on every edge; nothing outside out is written.  2 d Dn (D1 E1 + D2 E2) flops.
 * out must not overlap an operand.  mpsk_ctx_force_tile applies.  All of d, Dn, D1, D2, E1, E2 >= 1 and ldg >= the rows of
 * G, else MPSK_ERR_INVALID.  MPSK_F64 only: a ctx set to MPSK_C128 gets MPSK_ERR_UNSUPPORTED (bond-embedded complex
 * tensors run on it unchanged: concatenating embedded bond indices keeps their (re, im) pairing). */
enum { MPSK_DSUM_LEFT = 0, MPSK_DSUM_RIGHT = 1 };
int mpsk_dsum_site(mpsk_ctx* ctx, int side, int d, int Dn, int D1, int D2, int E1, int E2, const void* G, int64_t ldg,
                   const void* A1, const void* A2, void* out);

/* The four coefficient rows of mpsk_gemm_pair from the K singular values S (device) and one host scalar, on the device:
 * a line-search trial step at a new alpha costs no device-to-host copy.  coef: 4 K doubles, row r at coef + r K; rows a
 * mode does not use are zeroed.
 *   MPSK_GRASSMANN_RETRACT      (scalar alpha):  cos(alpha s), sin(alpha s), -s sin(alpha s), s cos(alpha s)
 *                                                -> out1 = W', out2 = transported direction, with P = W Vt^T, Q = U, B = Vt
 *   MPSK_GRASSMANN_TRANSPORT    (scalar alpha):  -sin(alpha s), cos(alpha s) - 1      -> B = U^T Theta, beta1 = 1
 *   MPSK_GRASSMANN_PRECONDITION (scalar delta):  s / (s^2 + (max(s) delta)^2)         grassmann.jl:231
 * MPSK_F64 only (MPSK_C128: MPSK_ERR_UNSUPPORTED). */
enum { MPSK_GRASSMANN_RETRACT = 0, MPSK_GRASSMANN_TRANSPORT = 1, MPSK_GRASSMANN_PRECONDITION = 2 };
int mpsk_grassmann_coef(mpsk_ctx* ctx, int K, const void* S, double scalar, int mode, void* coef);

/* strided column-major matrix copy dst[r, c] = src[r, c] (index permutations of small tensors, e.g.
 * AR[k, s, b] <- Vh[k, b, s] after tsvd!: dmrg.jl:104 `_transpose_front(ar)`) */
int mpsk_copy2d(mpsk_ctx* ctx, int rows, int cols, const void* src, int64_t lds, void* dst, int64_t ldd);

/* ---- Krylov vector protocol (VectorInterface: inner / add!! / scale!! / zerovector) -----------
 * KrylovKit needs these of the iterate type (quasiparticle_state.jl:357-411 is the in-repo example). */
int mpsk_vdot(mpsk_ctx* ctx, int64_t n, const void* x, const void* y, double* host_out);
int mpsk_vnrm2(mpsk_ctx* ctx, int64_t n, const void* x, double* host_out);
/* host_out[0] = |x - y|^2, host_out[1] = |x|^2 in ONE pass over both vectors (one launch + the final reduction of
 * mpsk_vdot; synchronises like it): norm(AC' - AC) / norm(AC') of fvomps.jl:66, taken on every site visit of approximate.
 * Follows mpsk_ctx_set_dtype: under MPSK_C128 n counts complex elements.  x == y gives exactly 0. */
int mpsk_vdiff_nrm2(mpsk_ctx* ctx, int64_t n, const void* x, const void* y, double* host_out);
int mpsk_vaxpby(mpsk_ctx* ctx, int64_t n, double alpha, const void* x, double beta, void* y);
int mpsk_vscal(mpsk_ctx* ctx, int64_t n, double alpha, void* x);
/* y = (I (x) J) x, J = [[0,-1],[1,0]], on interleaved row pairs of a tensor whose first dimension is even: the
 * multiplication by i of a complex tensor carried as 2x2 real blocks on its bond indices (integrators.jl:21
 * `-1im * dt` on the embedded representation, mpskit.jl_amd/cplx.py) */
int mpsk_vtimes_i(mpsk_ctx* ctx, int64_t n, const void* x, void* y);
/* interleaved complex z (n COMPLEX elements, 16-byte aligned) <-> planar p = [Re: n doubles | Im: n doubles], the vector
 * layout of the complex Arnoldi of the host (krylov.eigsolve_lm_planar); out of place, one memory-bound launch each way
 * (16 n bytes read, 16 n written), asynchronous, exact. */
int mpsk_vsplit_c(mpsk_ctx* ctx, int64_t n, const void* z, void* p);
int mpsk_vjoin_c(mpsk_ctx* ctx, int64_t n, const void* p, void* z);
int mpsk_vcopy(mpsk_ctx* ctx, int64_t n, const void* x, void* y);
int mpsk_vzero(mpsk_ctx* ctx, int64_t n, void* x);
/* fused Gram-Schmidt helpers: xs = HOST array of k device pointers.
 *   mpsk_vmultidot : host_out[j] = <xs[j], y>                       (one sync for k dots)
 *   mpsk_vgs_step  : h = [<xs[j], y>]_j ; y -= sum_j h[j] xs[j] ; host_out[j] = h[j]
 *                    (coefficients stay on the device between the two kernels) */
int mpsk_vmultidot(mpsk_ctx* ctx, int64_t n, int k, const void* const* xs, const void* y, double* host_out);
int mpsk_vgs_step(mpsk_ctx* ctx, int64_t n, int k, const void* const* xs, void* y, double* host_out);
/*   mpsk_vorth_step: one full Krylov orthogonalisation step with a single host sync: CGS2 of y against
 *                    xs[0..k), then y <- y / ||y||; host_h[j] = coefficient on xs[j], *host_beta = ||y|| */
int mpsk_vorth_step(mpsk_ctx* ctx, int64_t n, int k, const void* const* xs, void* y, double* host_h,
                    double* host_beta);
/* the same step without a host synchronisation: the 2k+1 scalars (h1[k], h2[k], |remainder|^2; h = h1 + h2,
 * beta = sqrt of the last) stay in dev_out (device memory, >= 2k+1 doubles) */
int mpsk_vorth_step_dev(mpsk_ctx* ctx, int64_t n, int k, const void* const* xs, void* y, void* dev_out);
/* y = sum_j coefs[j] xs[j]   (Ritz vector assembly); asynchronous (host_coefs is copied before the call returns) */
int mpsk_vlincomb(mpsk_ctx* ctx, int64_t n, int k, const void* const* xs, const double* host_coefs, void* y);
/* ys[j] = sum_i host_coefs[i + k j] xs[i] for j < m, all in ONE pass over the vectors (k + m instead of ~m (k + 6) vector
 * passes): the basis rotation of KrylovKit's thick restart (shrink step of eigsolve / schursolve at krylovdim 30, which
 * fixedpoint.jl:19-30 runs with maxiter = 100).  k, m <= 32; outputs must not alias inputs; asynchronous like mpsk_vlincomb. */
int mpsk_vmultilincomb(mpsk_ctx* ctx, int64_t n, int k, const void* const* xs, int m, void* const* ys, const double* host_coefs);
/* y = x / |x| (y may be x) and dev_out[0] = |x|^2, both without a host synchronisation: the start / Ritz-vector
 * normalisations of a fixed-budget Krylov solve and the per-site galerkin norms of a sweep are read back once per
 * solve / sweep instead of stalling the stream at every use (normalize! in toolbox.jl:18, fixedpoint.jl:19-30).
 * dev_n2 (optional, device memory, one double) receives |x|^2. */
int mpsk_vnormalize_dev(mpsk_ctx* ctx, int64_t n, const void* x, void* y, void* dev_n2);
/* Ritz step of a fixed-budget solve without leaving the device: dev_slot holds, for step k at offset k * stride, the
 * 2 (k + 1) + 1 scalars of mpsk_vorth_step_dev; dev_coef[0..m) receives the eigenvector of the smallest eigenvalue of
 * the projected (m <= 32) matrix (positive component on the start vector; zeros beyond an invariant-subspace cut) and
 * dev_info (optional, 3 doubles) {eigenvalue, residual estimate, effective m}.  mpsk_vlincomb_dev assembles
 * y = sum_j dev_coefs[j] xs[j] from device-resident coefficients.  (KrylovKit's eigsolve does this step on the host;
 * fixedpoint.jl:19-30 only uses the vector.) */
int mpsk_vritz_dev(mpsk_ctx* ctx, int m, int stride, const void* dev_slot, void* dev_coef, void* dev_info);
int mpsk_vlincomb_dev(mpsk_ctx* ctx, int64_t n, int k, const void* const* xs, const void* dev_coefs, void* y);
int mpsk_vnrm2_dev(mpsk_ctx* ctx, int64_t n, const void* x, void* dev_out);
/* Complex forms of the protocol, for Krylov spaces over the complex numbers: the GMRES of a correction-vector site solve
 * with complex z (corvector.jl:68: KrylovKit's linsolve on a ComplexF64 tensor, inner = conj(x) . y).  Vectors are
 * interleaved complex128, 16-byte aligned, n counts COMPLEX elements, complex scalars are (re, im) pairs.
 *   mpsk_vdotc       : host_out[0..2) = conj(x) . y
 *   mpsk_vaxpby_c    : y = alpha x + beta y   (beta = 0: y is not read)
 *   mpsk_vorth_step_c: mpsk_vorth_step with complex coefficients: CGS2 of y against xs[0..k), k <= 32, then y <- y / ||y||;
 *                      host_h[2j], host_h[2j + 1] = coefficient on xs[j] (conj(xs[j]) . y, both rounds), *host_beta = ||y||;
 *                      one host sync
 *   mpsk_vlincomb_c  : y = sum_j coefs[j] xs[j], host_coefs = 2k doubles; asynchronous like mpsk_vlincomb
 * Reductions take a fixed order (per-thread partial sums, wavefront reduction, one final reduction launch, no atomics):
 * results are bit-identical from run to run. */
int mpsk_vdotc(mpsk_ctx* ctx, int64_t n, const void* x, const void* y, double* host_out);
int mpsk_vaxpby_c(mpsk_ctx* ctx, int64_t n, const double* alpha, const void* x, const double* beta, void* y);
int mpsk_vorth_step_c(mpsk_ctx* ctx, int64_t n, int k, const void* const* xs, void* y, double* host_h, double* host_beta);
int mpsk_vlincomb_c(mpsk_ctx* ctx, int64_t n, int k, const void* const* xs, const double* host_coefs, void* y);

#ifdef __cplusplus
}
#endif
#endif /* MPSK_H */
