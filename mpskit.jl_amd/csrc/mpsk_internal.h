// Internal declarations shared by the HIP translation units of libmpsk (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <atomic>
#include <vector>
#include <string>

namespace mpsk {

// Once-per-device hipFuncSetAttribute(MaxDynamicSharedMemorySize).  `done` is a static bit mask owned by the call site
// (one bit per device ordinal); distinct ctxs may be driven from distinct host threads, so the flag is atomic -- a race
// only repeats the idempotent call.
inline hipError_t ensure_dyn_smem(std::atomic<uint64_t>& done, const void* kernel, size_t bytes) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const uint64_t bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
  e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return e;
  done.fetch_or(bit, std::memory_order_release);
  return hipSuccess;
}

constexpr int MAXSEG = 32;

struct GemmArgs {
  const double* A;
  const double* B;
  double* C;
  int M, N, K;               // K = length of ONE segment
  int64_t lda, ldb, ldc;
  int64_t bsA, bsB, bsC;     // batch strides (elements)
  int batch;
  int nseg;
  int64_t segA[MAXSEG], segB[MAXSEG];  // element offsets of each K-segment
  double alpha, beta;
  int transA, transB;        // 0: col-major as given; 1: operand is the transpose of a col-major matrix
  // optional per-batch element offsets (device arrays of length batch); override bsA/bsB/bsC when set
  const int64_t* tabA;
  const int64_t* tabB;
  const int64_t* tabC;
  // optional column split of C: columns n >= splitN of batch z go to C + tabC2[z] + (n - splitN)*ldc
  const int64_t* tabC2;
  int splitN;
  // stream-K (set by gemm_f64 itself): units of k-tiles per workgroup and the partial-tile workspace
  int sk_units;
  int sk_split_major;   // split-K launches: share index = split * (tiles * batch) + tile (see gemm_sk_body)
  double* sk_ws;
  // XCD grid (set by gemm_f64): the 8 XCDs' tile chunks are xcd_gx x xcd_gy rectangles of the tile grid (0: linear)
  int xcd_gx, xcd_gy;
  int xcd_interleave;   // triangular work (upper_only / a_upper / b_upper): tiles round-robin over the XCDs instead of chunks
  // optional per-batch K-segment offsets (device arrays [batch][nseg], element offsets): batch z reads segment i at
  // A + tabA/bsA offset + zsegA[z * nseg + i] (override segA / segB when set; nseg is uniform over the batches)
  const int64_t* zsegA;
  const int64_t* zsegB;
  // second operand family of a per-batch-table launch: segments i >= nseg1 read A2 / B2 (plus the batch offset of A / B)
  // instead of A / B, with the same lda / ldb / K.  The Jordan-form matvec (mpsk_hac mode 3) sums x GRc0 and GLc x in
  // one launch this way while its tables stay relative to their own bases (x changes every Krylov step, they do not).
  // A2 / B2 null: one family (gemm_f64 sets A2 = A, B2 = B, nseg1 = nseg).
  const double* A2;
  const double* B2;
  int nseg1;
  // complex128 operands carried as REAL matrices with (re, im) interleaved along the first (row) index of the A operand
  // and of C ("half-embedded" real view of TensorKit's interleaved complex storage), B planar (separate re / im planes):
  //   C_half = A_half Br + (J A_half) Bi,   J (re, im) = (-im, re)  -- the multiplication by i on a row pair.
  // segJ[i]: what the A loader applies to K-segment i: 0 nothing, 1 J, 2 -J.  cplx selects the kernel family with that
  // loader (the real kernels do not carry the test).  c_rs: row stride of C (1, or 2 to write one plane of an interleaved
  // complex result: transfer_left's Ab^H T2).
  signed char segJ[MAXSEG];
  int b_upper, a_upper;      // operand is upper triangular (single K segment, K index aligned with N resp. M): k-tiles that
                             // only meet structural zeros are skipped -- B upper: k < n0 + BN ; A upper: k >= m0
  int upper_only;            // C is symmetric (Gram matrix) and only its upper triangle is consumed: tiles strictly below the
                             // block diagonal are skipped (M == N, square tiles)
  int upper_nb;              // upper_only on a batch whose first upper_nb results are symmetric and the others are not: only
                             // batches z < upper_nb skip their lower tiles (0: every batch)
  int cplx;
  int c_rs;
  int tag;                   // 1: matvec-stage launch (own kernel symbol + event profile)
  int tabs_even;             // caller guarantees every tabA/tabB entry is even (16-B aligned operands)
  // optional second epilogue: C = alpha A^T B + gamma Z with Z [M, N] (column stride ldz) another matrix than C, which is
  // then only written (beta must be 0).  transA, !transB, batch 1, real operands; null: the alpha / beta epilogue.
  const double* Z;
  int64_t ldz;
  double gamma;
};

hipError_t gemm_f64(const GemmArgs& g, hipStream_t s);
void gemm_force_tile(int bm, int bn);
// reference count of the ctxs bound to (current device, stream); the split-K partial-tile workspace attached to the pair is
// freed when the last of them releases it (ctx destroyed or bound to another stream)
void gemm_retain_stream(hipStream_t s);
void gemm_release_stream(hipStream_t s);
void gemm_enable_streamk(bool on);
void gemm_prof_enable(bool on);
std::string gemm_prof_summary();

// ---- paired column-scaled product (mpsk_gemm_pair; mpsk_gemm.hip) ------------------------------
//   C1 = beta1 C1 + (P diag(a1) + Q diag(b1)) B,   C2 = beta2 C2 + (P diag(a2) + Q diag(b2)) B
// P, Q: M x K, B: K x N, column-major, not transposed; a* / b*: device vectors of length K.  Q == nullptr drops the Q
// terms (b* are not read), C2 == nullptr the second output (a2 / b2 are not read).  One launch, no workspace, one
// workgroup per output tile walking k in ascending order: the summation order is fixed.
struct GemmPairArgs {
  const double* P;
  const double* Q;
  const double* B;
  double* C1;
  double* C2;
  int M, N, K;
  int64_t ldp, ldq, ldb, ld1, ld2;
  const double* a1;
  const double* b1;
  const double* a2;
  const double* b2;
  double beta1, beta2;
};
hipError_t gemm_pair_f64(const GemmPairArgs& g, hipStream_t s);
// ---- direct-sum site step (mpsk_dsum_site; mpsk_gemm.hip) -------------------------------------
// Two products C_f = A_f B_f in one launch (a grouped GEMM: the tile list of family 0, then that of family 1).  Of each
// GemmArgs only A, B, C, M, N, K, lda, ldb, ldc and K-segment 0 (nseg = 1, segA[0] = segB[0] = 0) are read; neither
// operand is transposed.  Row m of family f is written at C_f + (m % rmod[f]) + (m / rmod[f]) * rstride + n * ldc.
// One workgroup per output tile, k ascending, no workspace; ntiles0 is filled by dsum_f64.
struct DsumArgs {
  GemmArgs f[2];
  int rmod[2];
  int64_t rstride;
  int ntiles0;
};
static_assert(sizeof(DsumArgs) <= 4096, "DsumArgs is passed by value as a kernel argument");
hipError_t dsum_f64(const DsumArgs& a, hipStream_t s);
// coefficient rows of the Grassmann retraction / transport / preconditioner (mpsk_grassmann_coef): coef[r * K + k],
// r = a1, b1, a2, b2; mode 0 retract, 1 transport, 2 precondition
hipError_t grassmann_coef(int K, const double* S, double scalar, int mode, double* coef, hipStream_t s);

// ---- slab mixing:  out_slab[o][r,c] = sum_t coef[t] * in_slab[src[t]][r,c]  --------------------
// A "slab" is an R x C column-major matrix view (ld, base offset) inside a larger tensor.  This
// is the (w,s) -> (v,t) application of the small MPO tensor between the two big GEMMs.
struct MixTerm { int32_t out, in; double coef; double coef_im = 0.0; };

struct MixPlan {          // device-resident CSR: terms grouped by output slab
  int n_out = 0, n_in = 0;
  int32_t* d_rowptr = nullptr;   // [n_out+1]
  int32_t* d_src = nullptr;      // [nnz]
  double* d_coef = nullptr;      // [nnz]
  double* d_coef_im = nullptr;   // [nnz] imaginary parts (complex plans: slabs hold (re, im) row pairs), else null
  int nnz = 0;
  int max_terms = 0;
};

hipError_t mix_plan_create(const std::vector<MixTerm>& terms, int n_out, int n_in, MixPlan* plan);
void mix_plan_destroy(MixPlan* plan);

// slab j = j0 + n0*(j1 + n1*j2) lives at element offset j0*s0 + j1*s1 + j2*s2; rows contiguous,
// column stride ld.
struct SlabIndex { int n0, n1; int64_t s0, s1, s2; int64_t ld; };
hipError_t mix_apply(const MixPlan& plan, const double* in, SlabIndex iin, double* out, SlabIndex iout,
                     int R, int C, hipStream_t s);
// dst[r * drs + c * dcs] = src[r * srs + c * scs]   (R x C elements, arbitrary strides): interleaved <-> planar complex,
// extraction of the real / imaginary planes of an embedded tensor
hipError_t deinterleave(const double* z, int64_t n, double* re, double* im, hipStream_t s);   // z 16-byte aligned
hipError_t interleave(const double* re, const double* im, int64_t n, double* z, hipStream_t s);     // z 16-byte aligned
hipError_t copy_strided(const double* src, int64_t srs, int64_t scs, double* dst, int64_t drs, int64_t dcs, int64_t R,
                        int64_t C, hipStream_t s);
hipError_t identity_slab(double* G, int n, hipStream_t s);   // G[n, n] (contiguous) = identity
// out[l] = sum_p cd[l,p] P[p] + ct[l,p] P[p]^T for l < nl: P np contiguous n x n matrices, out[l] at out + l * out_stride
// (n x n, contiguous), d_coef device [nl][np][2] = (cd, ct).  The first ndiag matrices are symmetric with only their upper
// triangle valid (the Gram products P_tt of the pair-Gram transfers): element (r, c) with r > c is read at (c, r), and their
// ct is not used.  Terms with both coefficients zero are skipped; the others are added in the order p = 0 .. np-1, direct
// before transposed: bit-reproducible.
hipError_t pair_combine(const double* P, int np, int ndiag, int n, const double* d_coef, int nl, double* out,
                        int64_t out_stride, hipStream_t s);

// ---- vector kernels ---------------------------------------------------------------------------
// xs: HOST array of k device pointers; d_out / d_coefs: device [k]; d_partial: device scratch
// [MPSK_DOT_SCRATCH doubles].  Vectors must be 16-B aligned.
constexpr int MPSK_DOT_SCRATCH = 32 * 1024;     // up to 32 dots x DOT_BLOCKS partial sums (the long fused Gram-Schmidt passes)
hipError_t vec_multidot(const double* const* xs, int k, const double* y, int64_t n, double* d_out,
                        double* d_partial, hipStream_t s);
// d_out = {|x - y|^2, |x|^2}: one pass over both vectors + the final reduction of vec_multidot
hipError_t vec_diff_nrm2(const double* x, const double* y, int64_t n, double* d_out, double* d_partial, hipStream_t s);
hipError_t vec_axpby(double a, const double* x, double b, double* y, int64_t n, hipStream_t s);
hipError_t vec_times_i(const double* x, double* y, int64_t n, hipStream_t s);
hipError_t vec_scal(double a, double* x, int64_t n, hipStream_t s);
hipError_t vec_scal_rsqrt_dev(const double* d_n2, double* x, int64_t n, hipStream_t s);
hipError_t vec_scal_rsqrt_dev_oop(const double* d_n2, const double* x, double* y, int64_t n, hipStream_t s);
// CGS2 of y against xs[0..k) + squared norm of the remainder, fused passes (mpsk_ops.hip); d_out = {h1[k], h2[k], |y|^2}
hipError_t vec_cgs2(const double* const* xs, int k, double* y, int64_t n, double* d_out, double* d_partial, hipStream_t s);
// Ritz step of a fixed-budget Krylov solve on the device (mpsk_ops.hip: ritz_small_kernel); m <= 32
hipError_t vec_ritz_small(const double* d_slot, int m, int stride, double* d_coef, double* d_info, hipStream_t s);
hipError_t vec_multilincomb(const double* const* xs, int k, double* const* ys, int m, const double* d_coefs, int64_t n,
                            hipStream_t s);   // ys[j] = sum_i d_coefs[i + k j] xs[i]; k, m <= 32
hipError_t vec_multiaxpy(const double* const* xs, const double* d_coefs, int k, double sign, double* y,
                         int64_t n, hipStream_t s);
// complex128 forms (interleaved vectors, n = complex elements, complex scalars as (re, im) pairs); d_out of vec_multidotc:
// [2k], of vec_cgs2_c: {h1[2k], h2[2k], |y|^2}; vec_axpby_c: y = a x + b y, x == nullptr: y = b y
hipError_t vec_multidotc(const double* const* xs, int k, const double* y, int64_t n, double* d_out, double* d_partial,
                         hipStream_t s);
hipError_t vec_multiaxpy_c(const double* const* xs, const double* d_coefs, int k, double sign, double* y, int64_t n,
                           hipStream_t s);
hipError_t vec_cgs2_c(const double* const* xs, int k, double* y, int64_t n, double* d_out, double* d_partial, hipStream_t s);
hipError_t vec_axpby_c(const double a[2], const double* x, const double b[2], double* y, int64_t n, hipStream_t s);
hipError_t identity_dev_c(const double* G, int n, double* d_out, int nblocks, hipStream_t s);   // d_out[b]: per-block max|G - I|
// dstR = sum_k coef[k] srcR[k] (nR doubles) and dstL = sum_k coef[k] srcL[k] (nL doubles) in ONE launch, terms in the order
// k = 0 .. n-1 (bit-reproducible); everything is passed by value.  All pointers 16-byte aligned.  The fold pair of a summed
// mode-3 operator (mpsk_hsum_set_coefs).
constexpr int MPSK_HSUM_MAX = 8;
struct FoldLincombArgs {
  const double* srcR[MPSK_HSUM_MAX];
  const double* srcL[MPSK_HSUM_MAX];
  double coef[MPSK_HSUM_MAX];
  double *dstR, *dstL;
  int64_t nR, nL;
  int n;
};
hipError_t fold_lincomb(const FoldLincombArgs& a, hipStream_t s);
// d_out[w][t,s] = sum_{p,b} conj(Ab[p,t,b]) X[w][p,s,b]: X W tensors [Dl,d,Dr], Ab [Dl,d,Dr] (interleaved when cplx), d_out
// W column-major d x d matrices; d_partial: site_gram_partial_doubles(W, d, cplx) doubles of scratch.  Asynchronous,
// deterministic (fixed-order partial sums + dot_final_kernel).
size_t site_gram_partial_doubles(int W, int d, bool cplx);
hipError_t site_gram(int W, int d, int Dl, int Dr, const double* X, const double* Ab, bool cplx, double* d_out,
                     double* d_partial, hipStream_t s);
// per-block partial sums of the dot / Gram kernels: row j of a partial buffer is DOT_BLOCKS doubles, one per workgroup
constexpr int DOT_BLOCKS = 1024;
// d_out[j] = sum_{b < nblocks} d_partial[j * DOT_BLOCKS + b], j < nrows, in a fixed order (the closing launch of every dot
// and Gram reduction)
hipError_t dot_final(const double* d_partial, int nblocks, int nrows, double* d_out, hipStream_t s);
// d_out[t,s] = sum_{p,q} conj(Ab[p,t,q]) sum_b T1[p,s,b] R[b,q]: the closing product of mpsk_transfer_left_gram_env on
// the stage-1 product T1 [Dlb, d, Dr], fused with the Gram reduction (mpsk_gemm.hip: the product T1 R only exists as MFMA
// accumulator tiles).  R: [Dr, Drb], for complex operands planar with r_plane doubles between the planes; T1 / Ab
// interleaved.  d <= gram_env_max_d(); d_partial: site_gram_partial_doubles(1, d, cplx) doubles.  Asynchronous,
// deterministic.
int gram_env_max_d();
hipError_t gram_env(int d, int Dlb, int Dr, int Drb, const double* T1, const double* R, int64_t r_plane, const double* Ab,
                    bool cplx, double* d_out, double* d_partial, hipStream_t s);

// ---- gauge kernels ----------------------------------------------------------------------------
size_t regularize_workspace_doubles(int W, int D1, int D2);
hipError_t regularize(int W, int D1, int D2, double* v, const double* lvec, const double* rvec, double* partial, hipStream_t s);
// out[w] = a0 x[w] + a1 (y[w] - <lvec^T, y[w]> rvec) (bilinear), two launches; x may be NULL (a0 unused); out may be y or x.
// cplx: interleaved complex operands, `partial` then holds 2 * regularize_workspace_doubles(W, D1, D2) doubles.
hipError_t regularize_axpby(bool cplx, int W, int D1, int D2, const double* y, const double* lvec, const double* rvec, double a1,
                            const double* x, double a0, double* out, double* partial, hipStream_t s);
hipError_t transpose(const double* in, int ldi, int rows, int cols, double* out, int ldo, hipStream_t s);
size_t qrpos_workspace_doubles(int m, int n);
int qrpos_max_rows();   // row limit of the blocked Householder route (one panel column in the LDS)
hipError_t qrpos(int m, int n, const double* A, int lda, double* Q, int ldq, double* R, int ldr, double* ws,
                 hipStream_t s, std::string* err);

size_t cholqr_workspace_doubles(int m, int n);
hipError_t cholqr3(int m, int n, const double* A, int lda, double* Q, int ldq, double* R, int ldr, double* ws,
                   int* d_flag, int* flag_out, hipStream_t s, double shift_scale = 1.0);
hipError_t cholqr_robust(int m, int n, const double* A, int lda, double* Q, int ldq, double* R, int ldr, double* ws,
                         int* d_flag, int* flag_out, hipStream_t s);
hipError_t cholqr1_orth(int m, int n, const double* X, int ldx, double* Q, int ldq, double* ws, int* d_flag, hipStream_t s,
                        double shift_scale);
hipError_t cholqr3_enqueue(int m, int n, const double* A, int lda, double* Q, int ldq, double* R, int ldr, double* ws,
                           int* d_flag, int* flag_out, hipStream_t s, double shift_scale = 1.0);
hipError_t cholqr3_finalize(int m, int n, double* Q, int ldq, double* R, int ldr, double* ws, int* d_flag,
                            int* flag_out, hipStream_t s);
size_t tsvd_workspace_bytes(int m, int n);
hipError_t tsvd(int m, int n, const double* theta, int ldt, double* U, int ldu, double* S, double* Vh, int ldv,
                int max_keep, double trunc_err, int* kept, double* disc_norm, void* ws, hipStream_t s,
                std::string* err, int* sweeps_out, const double* Qpre = nullptr, int ldq = 0, int q_rows = 0,
                int outer_transposed = 0, const hipStream_t* xs = nullptr, int nxs = 0, int vfree = 0);
// complex128 counterpart (interleaved operands, leading dimensions in complex elements; mpsk_svd.hip).  q_rows: rows of
// Qpre in the QR-preconditioned mode (0 otherwise); the workspace depends on it.
size_t tsvd_c128_workspace_bytes(int m, int n, int q_rows);
hipError_t tsvd_c128(int m, int n, const double* theta, int ldt, double* U, int ldu, double* S, double* Vh, int ldv,
                     int max_keep, double trunc_err, int* kept, double* disc_norm, void* ws, hipStream_t s,
                     std::string* err, int* sweeps_out, const double* Qpre, int ldq, int q_rows, int outer_transposed);

}  // namespace mpsk
