// Slice-less entries of the C ABI (see include/mpsk.h): the GEMM wrappers and the vector protocol of the Krylov solvers.
#include <cstdio>
#include <cmath>
#include <algorithm>
#include "mpsk_api_internal.h"

// complex128 (ctx dtype MPSK_C128): C = alpha op(A) op(B) + beta C on interleaved complex matrices, op = conjugate transpose,
// alpha / beta real.  An interleaved complex matrix IS the even-column half of its real embedding, and only those columns
// of the result are wanted:  C_half = op(E_A) . (op(B))_half  -- ONE real GEMM with A embedded (2M x 2K) and B (or its
// conjugate transpose, materialised) as is: 8 M N K real flops, the complex optimum.
int gemm_c128(mpsk_ctx* c, int transA, int transB, int M, int N, int K, double alpha, const void* A, int64_t lda,
                     const void* B, int64_t ldb, double beta, void* C, int64_t ldc) {
  HIPCHK(hipSetDevice(c->device));
  const int ar = transA ? K : M, ac = transA ? M : K;                  // A as stored: ar x ac complex
  const size_t ea = (size_t)4 * ar * ac, bt = transB ? (size_t)2 * K * N : 0;
  double* buf = nullptr;
  if (int rc = cx_scratch(c, 1, sizeof(double) * (ea + bt), &buf)) return rc;
  double* EA = buf;
  hipLaunchKernelGGL(cx_embed_kernel, dim3(1024), dim3(256), 0, c->stream, (const double*)A, 2 * lda, ar, ac, EA, (int64_t)2 * ar);
  const double* Bh = (const double*)B;
  int64_t ldbh = 2 * ldb;
  if (transB) {                                                        // B stored N x K complex -> B^H (K x N)
    double* Bt = buf + ea;
    hipLaunchKernelGGL(cx_ctranspose_kernel, dim3(1024), dim3(256), 0, c->stream, (const double*)B, 2 * ldb, N, K, Bt, (int64_t)2 * K);
    Bh = Bt; ldbh = (int64_t)2 * K;
  }
  GemmArgs g = mk(EA, Bh, (double*)C, 2 * M, N, 2 * K, (int64_t)2 * ar, ldbh, 2 * ldc, transA ? 1 : 0, 0);
  g.alpha = alpha; g.beta = beta;
  HIPCHK(gemm_f64(g, c->stream));
  return MPSK_OK;
}

extern "C" {

int mpsk_gemm(mpsk_ctx* c, int transA, int transB, int M, int N, int K, double alpha, const void* A, int64_t lda,
              const void* B, int64_t ldb, double beta, void* C, int64_t ldc) {
  REQUIRE(c && A && B && C, "NULL argument");
  REQUIRE(M > 0 && N > 0 && K > 0, "dimensions must be positive");
  if (c->dtype == MPSK_C128) return gemm_c128(c, transA, transB, M, N, K, alpha, A, lda, B, ldb, beta, C, ldc);
  HIPCHK(hipSetDevice(c->device));
  GemmArgs g = mk((const double*)A, (const double*)B, (double*)C, M, N, K, lda, ldb, ldc, transA ? 1 : 0, transB ? 1 : 0);
  g.alpha = alpha; g.beta = beta;
  HIPCHK(gemm_f64(g, c->stream));
  return MPSK_OK;
}

// fp64 only; no workspace (the kernel keeps both outputs' accumulators in registers and writes C directly)
int mpsk_gemm_pair(mpsk_ctx* c, int M, int N, int K, const void* P, int64_t ldp, const void* Q, int64_t ldq, const void* B,
                   int64_t ldb, const void* coef, int64_t ldcoef, double beta1, void* out1, int64_t ld1, double beta2,
                   void* out2, int64_t ld2) {
  REQUIRE(c && P && B && coef && out1, "NULL argument");
  if (c->dtype == MPSK_C128) return fail(MPSK_ERR_UNSUPPORTED, "mpsk_gemm_pair: fp64 only");
  REQUIRE(M > 0 && N > 0 && K > 0, "dimensions must be positive");
  REQUIRE(ldp >= M && ldb >= K && ld1 >= M && ldcoef >= K, "leading dimension below the row count");
  REQUIRE(!Q || ldq >= M, "ldq below the row count");
  REQUIRE(!out2 || ld2 >= M, "ld2 below the row count");
  REQUIRE(out1 != out2 && out1 != P && out1 != Q && out1 != B && (!out2 || (out2 != P && out2 != Q && out2 != B)),
          "outputs must not alias the operands or each other");
  HIPCHK(hipSetDevice(c->device));
  const double* cf = (const double*)coef;
  GemmPairArgs g{};
  g.P = (const double*)P; g.Q = (const double*)Q; g.B = (const double*)B;
  g.C1 = (double*)out1; g.C2 = (double*)out2;
  g.M = M; g.N = N; g.K = K;
  g.ldp = ldp; g.ldq = Q ? ldq : 0; g.ldb = ldb; g.ld1 = ld1; g.ld2 = out2 ? ld2 : 0;
  g.a1 = cf; g.b1 = cf + ldcoef; g.a2 = cf + 2 * ldcoef; g.b2 = cf + 3 * ldcoef;
  g.beta1 = beta1; g.beta2 = beta2;
  HIPCHK(gemm_pair_f64(g, c->stream));
  return MPSK_OK;
}

// fp64 only; one launch, no workspace: the two block products are the two tile families of dsum_f64
int mpsk_dsum_site(mpsk_ctx* c, int side, int d, int Dn, int D1, int D2, int E1, int E2, const void* G, int64_t ldg,
                   const void* A1, const void* A2, void* out) {
  REQUIRE(c && G && A1 && A2 && out, "NULL argument");
  if (c->dtype == MPSK_C128) return fail(MPSK_ERR_UNSUPPORTED, "mpsk_dsum_site: fp64 only");
  REQUIRE(side == MPSK_DSUM_LEFT || side == MPSK_DSUM_RIGHT, "side must be MPSK_DSUM_LEFT or MPSK_DSUM_RIGHT");
  REQUIRE(d > 0 && Dn > 0 && D1 > 0 && D2 > 0 && E1 > 0 && E2 > 0, "dimensions must be positive");
  const bool left = side == MPSK_DSUM_LEFT;
  const int64_t Dt = (int64_t)D1 + D2, Et = (int64_t)E1 + E2;
  const int64_t g_rows = left ? Dn : Et, g_cols = left ? Dt : Dn;
  REQUIRE(ldg >= g_rows, "ldg below the row count of G");
  REQUIRE((int64_t)D1 * d <= 0x7fffffff && (int64_t)D2 * d <= 0x7fffffff && (int64_t)E1 * d <= 0x7fffffff &&
              (int64_t)E2 * d <= 0x7fffffff && Dt <= 0x7fffffff && Et <= 0x7fffffff,
          "a matrix extent exceeds 2^31 - 1");
  const double* Gp = (const double*)G;
  const double* a1 = (const double*)A1;
  const double* a2 = (const double*)A2;
  double* o = (double*)out;
  const int64_t n_out = (left ? (int64_t)Dn * Et : Dt * Dn) * d;
  auto overlaps = [&](const double* p, int64_t n) { return p < o + n_out && o < p + n; };
  REQUIRE(!overlaps(a1, (int64_t)D1 * d * E1) && !overlaps(a2, (int64_t)D2 * d * E2) &&
              !overlaps(Gp, ldg * (g_cols - 1) + g_rows),
          "out must not alias an operand");
  HIPCHK(hipSetDevice(c->device));
  DsumArgs a;
  std::memset(&a, 0, sizeof(a));
  if (left) {
    // out[:, :, :E1] = G[:, :D1] A1 and out[:, :, E1:] = G[:, D1:] A2: two contiguous matrices Dn x (d E)
    a.f[0] = mk(Gp, a1, o, Dn, d * E1, D1, ldg, D1, Dn);
    a.f[1] = mk(Gp + (int64_t)D1 * ldg, a2, o + (int64_t)Dn * d * E1, Dn, d * E2, D2, ldg, D2, Dn);
    a.rmod[0] = a.rmod[1] = Dn;
    a.rstride = 0;
  } else {
    // out[:D1, s, :] = A1[:, s, :] G[:E1, :] and out[D1:, s, :] = A2[:, s, :] G[E1:, :]: the products (D d) x Dn with
    // row (a, s) of block f written at a + s (D1 + D2)
    a.f[0] = mk(a1, Gp, o, D1 * d, Dn, E1, (int64_t)D1 * d, ldg, Dt * d);
    a.f[1] = mk(a2, Gp + E1, o + D1, D2 * d, Dn, E2, (int64_t)D2 * d, ldg, Dt * d);
    a.rmod[0] = D1; a.rmod[1] = D2;
    a.rstride = Dt;
  }
  HIPCHK(dsum_f64(a, c->stream));
  return MPSK_OK;
}

int mpsk_grassmann_coef(mpsk_ctx* c, int K, const void* S, double scalar, int mode, void* coef) {
  REQUIRE(c && S && coef, "NULL argument");
  if (c->dtype == MPSK_C128) return fail(MPSK_ERR_UNSUPPORTED, "mpsk_grassmann_coef: fp64 only");
  REQUIRE(K > 0, "K must be positive");
  REQUIRE(mode >= MPSK_GRASSMANN_RETRACT && mode <= MPSK_GRASSMANN_PRECONDITION, "mode must be 0 (retract), 1 (transport) or 2 (precondition)");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(grassmann_coef(K, (const double*)S, scalar, mode, (double*)coef, c->stream));
  return MPSK_OK;
}

int mpsk_copy2d(mpsk_ctx* c, int rows, int cols, const void* src, int64_t lds, void* dst, int64_t ldd) {
  REQUIRE(c && src && dst, "NULL argument");
  REQUIRE(rows > 0 && cols > 0 && lds >= rows && ldd >= rows, "bad dimensions");
  HIPCHK(hipMemcpy2DAsync(dst, sizeof(double) * ldd, src, sizeof(double) * lds, sizeof(double) * rows, cols,
                          hipMemcpyDeviceToDevice, c->stream));
  return MPSK_OK;
}

// --------------------------------------------------------------------------------------------
// vectors
// --------------------------------------------------------------------------------------------
static int fetch_scalars(mpsk_ctx* c, int k, double* host_out) {
  HIPCHK(hipMemcpyAsync(c->h_scal, c->d_scal, sizeof(double) * k, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  std::memcpy(host_out, c->h_scal, sizeof(double) * k);
  return MPSK_OK;
}

int mpsk_vmultidot(mpsk_ctx* c, int64_t n, int k, const void* const* xs, const void* y, double* host_out) {
  REQUIRE(c && xs && y && host_out, "NULL argument");
  REQUIRE(k > 0 && k <= MAXK && n > 0, "bad k or n");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(vec_multidot((const double* const*)xs, k, (const double*)y, n, c->d_scal, c->d_partial, c->stream));
  return fetch_scalars(c, k, host_out);
}

int mpsk_vdot(mpsk_ctx* c, int64_t n, const void* x, const void* y, double* host_out) {
  const void* xs[1] = {x};
  return mpsk_vmultidot(c, n, 1, xs, y, host_out);
}

int mpsk_vnrm2(mpsk_ctx* c, int64_t n, const void* x, double* host_out) {
  double v = 0.0;
  if (int rc = mpsk_vdot(c, n, x, x, &v)) return rc;
  *host_out = std::sqrt(v);
  return MPSK_OK;
}

// host_out = {|x - y|^2, |x|^2} in one pass over both vectors: the convergence measure norm(AC' - AC) / norm(AC') of a
// variational-approximation site visit (fvomps.jl:66).  MPSK_C128 (ctx dtype): n counts complex elements.
int mpsk_vdiff_nrm2(mpsk_ctx* c, int64_t n, const void* x, const void* y, double* host_out) {
  REQUIRE(c && x && y && host_out, "NULL argument");
  REQUIRE(n > 0, "bad n");
  REQUIRE(((uintptr_t)x % 16 == 0) && ((uintptr_t)y % 16 == 0), "operands must be 16-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(vec_diff_nrm2((const double*)x, (const double*)y, c->dtype == MPSK_C128 ? 2 * n : n, c->d_scal, c->d_partial,
                       c->stream));
  return fetch_scalars(c, 2, host_out);
}

int mpsk_vgs_step(mpsk_ctx* c, int64_t n, int k, const void* const* xs, void* y, double* host_out) {
  REQUIRE(c && xs && y && host_out, "NULL argument");
  REQUIRE(k > 0 && k <= MAXK && n > 0, "bad k or n");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(vec_multidot((const double* const*)xs, k, (const double*)y, n, c->d_scal, c->d_partial, c->stream));
  HIPCHK(vec_multiaxpy((const double* const*)xs, c->d_scal, k, -1.0, (double*)y, n, c->stream));
  return fetch_scalars(c, k, host_out);
}

// One Krylov orthogonalisation step with ONE host sync: twice-iterated classical Gram-Schmidt of y
// against xs[0..k), then y <- y / ||y||.  host_h[j] = total coefficient on xs[j], *host_beta = ||y||
// before normalisation.  (KrylovKit's ModifiedGramSchmidt2 + normalize, 4 calls / 3 syncs fused.)
int mpsk_vorth_step(mpsk_ctx* c, int64_t n, int k, const void* const* xs, void* y, double* host_h, double* host_beta) {
  REQUIRE(c && xs && y && host_h && host_beta, "NULL argument");
  REQUIRE(k > 0 && 2 * k + 1 <= MAXK && n > 0, "bad k or n");
  HIPCHK(hipSetDevice(c->device));
  const double* const* X = (const double* const*)xs;
  double* yy = (double*)y;
  HIPCHK(vec_cgs2(X, k, yy, n, c->d_scal, c->d_partial, c->stream));
  HIPCHK(vec_scal_rsqrt_dev(c->d_scal + 2 * k, yy, n, c->stream));
  double tmp[MAXK];
  if (int rc = fetch_scalars(c, 2 * k + 1, tmp)) return rc;
  for (int j = 0; j < k; ++j) host_h[j] = tmp[j] + tmp[k + j];
  *host_beta = tmp[2 * k] > 0.0 ? std::sqrt(tmp[2 * k]) : 0.0;
  return MPSK_OK;
}

// Same fused step with the 2k+1 scalars left on the DEVICE (dev_out: first-pass dots [k], second-pass dots [k],
// squared norm of the remainder): no host synchronisation, so a fixed-length Krylov recurrence can be enqueued
// back to back and its small projected matrix is read once at the end.
int mpsk_vorth_step_dev(mpsk_ctx* c, int64_t n, int k, const void* const* xs, void* y, void* dev_out) {
  REQUIRE(c && xs && y && dev_out, "NULL argument");
  REQUIRE(k > 0 && 2 * k + 1 <= MAXK && n > 0, "bad k or n");
  HIPCHK(hipSetDevice(c->device));
  const double* const* X = (const double* const*)xs;
  double* yy = (double*)y;
  double* out = (double*)dev_out;
  HIPCHK(vec_cgs2(X, k, yy, n, out, c->d_partial, c->stream));
  HIPCHK(vec_scal_rsqrt_dev(out + 2 * k, yy, n, c->stream));
  return MPSK_OK;
}

int mpsk_vlincomb(mpsk_ctx* c, int64_t n, int k, const void* const* xs, const double* host_coefs, void* y) {
  REQUIRE(c && xs && y && host_coefs, "NULL argument");
  REQUIRE(k > 0 && k <= MAXK && n > 0, "bad k or n");
  HIPCHK(hipSetDevice(c->device));
  // asynchronous: the coefficients travel through their own pinned buffer, which is only rewritten once the upload that
  // last read it has completed (an event wait, normally already satisfied) -- no stream synchronisation on either side
  if (c->coef_pending) { HIPCHK(hipEventSynchronize(c->ev_coef)); c->coef_pending = false; }
  std::memcpy(c->h_coef, host_coefs, sizeof(double) * k);
  HIPCHK(hipMemcpyAsync(c->d_coef, c->h_coef, sizeof(double) * k, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipEventRecord(c->ev_coef, c->stream));
  c->coef_pending = true;
  HIPCHK(hipMemsetAsync(y, 0, sizeof(double) * n, c->stream));
  HIPCHK(vec_multiaxpy((const double* const*)xs, c->d_coef, k, 1.0, (double*)y, n, c->stream));
  return MPSK_OK;
}

// ys[j] = sum_i host_coefs[i + k j] xs[i], j < m: the basis rotation of a thick restart in one pass over the vectors
int mpsk_vmultilincomb(mpsk_ctx* c, int64_t n, int k, const void* const* xs, int m, void* const* ys, const double* host_coefs) {
  REQUIRE(c && xs && ys && host_coefs, "NULL argument");
  REQUIRE(k > 0 && k <= 32 && m > 0 && m <= 32 && n > 0, "needs 0 < k, m <= 32 and n > 0");
  for (int j = 0; j < m; ++j)
    for (int i = 0; i < k; ++i) REQUIRE(ys[j] != xs[i], "outputs must not alias inputs");
  HIPCHK(hipSetDevice(c->device));
  if (c->coef_pending) { HIPCHK(hipEventSynchronize(c->ev_coef)); c->coef_pending = false; }
  std::memcpy(c->h_coef, host_coefs, sizeof(double) * (size_t)k * m);
  HIPCHK(hipMemcpyAsync(c->d_coef, c->h_coef, sizeof(double) * (size_t)k * m, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipEventRecord(c->ev_coef, c->stream));
  c->coef_pending = true;
  HIPCHK(vec_multilincomb((const double* const*)xs, k, (double* const*)ys, m, c->d_coef, n, c->stream));
  return MPSK_OK;
}

// Ritz coefficients of a fixed-budget solve from the scalars mpsk_vorth_step_dev collected (see ritz_small_kernel)
int mpsk_vritz_dev(mpsk_ctx* c, int m, int stride, const void* dev_slot, void* dev_coef, void* dev_info) {
  REQUIRE(c && dev_slot && dev_coef, "NULL argument");
  REQUIRE(m > 0 && m <= 32 && stride >= 2 * m + 1, "needs 0 < m <= 32 and stride >= 2 m + 1");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(vec_ritz_small((const double*)dev_slot, m, stride, (double*)dev_coef, (double*)dev_info, c->stream));
  return MPSK_OK;
}

// y = sum_j dev_coefs[j] xs[j] with the coefficients already on the device
int mpsk_vlincomb_dev(mpsk_ctx* c, int64_t n, int k, const void* const* xs, const void* dev_coefs, void* y) {
  REQUIRE(c && xs && y && dev_coefs, "NULL argument");
  REQUIRE(k > 0 && k <= MAXK && n > 0, "bad k or n");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipMemsetAsync(y, 0, sizeof(double) * n, c->stream));
  HIPCHK(vec_multiaxpy((const double* const*)xs, (const double*)dev_coefs, k, 1.0, (double*)y, n, c->stream));
  return MPSK_OK;
}

// y = x / |x| without a host synchronisation; |x|^2 is left in dev_n2 (device memory, one double) when given
int mpsk_vnormalize_dev(mpsk_ctx* c, int64_t n, const void* x, void* y, void* dev_n2) {
  REQUIRE(c && x && y, "NULL argument");
  REQUIRE(n > 0, "bad n");
  HIPCHK(hipSetDevice(c->device));
  double* n2 = dev_n2 ? (double*)dev_n2 : c->d_scal + (MAXK - 1);
  const double* xs[1] = {(const double*)x};
  HIPCHK(vec_multidot(xs, 1, (const double*)x, n, n2, c->d_partial, c->stream));
  if (y != x) HIPCHK(vec_scal_rsqrt_dev_oop(n2, (const double*)x, (double*)y, n, c->stream));
  else HIPCHK(vec_scal_rsqrt_dev(n2, (double*)y, n, c->stream));
  return MPSK_OK;
}

// dev_out[0] = |x|^2 (device memory), no host synchronisation
int mpsk_vnrm2_dev(mpsk_ctx* c, int64_t n, const void* x, void* dev_out) {
  REQUIRE(c && x && dev_out, "NULL argument");
  REQUIRE(n > 0, "bad n");
  HIPCHK(hipSetDevice(c->device));
  const double* xs[1] = {(const double*)x};
  HIPCHK(vec_multidot(xs, 1, (const double*)x, n, (double*)dev_out, c->d_partial, c->stream));
  return MPSK_OK;
}

int mpsk_vaxpby(mpsk_ctx* c, int64_t n, double alpha, const void* x, double beta, void* y) {
  REQUIRE(c && x && y, "NULL argument");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(vec_axpby(alpha, (const double*)x, beta, (double*)y, n, c->stream));
  return MPSK_OK;
}
// ---- complex forms of the vector protocol: interleaved complex128 vectors, n = complex elements ----------------------
static bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

int mpsk_vdotc(mpsk_ctx* c, int64_t n, const void* x, const void* y, double* host_out) {
  REQUIRE(c && x && y && host_out, "NULL argument");
  REQUIRE(n > 0, "bad n");
  REQUIRE(aligned16(x) && aligned16(y), "operands must be 16-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  const double* xs[1] = {(const double*)x};
  HIPCHK(vec_multidotc(xs, 1, (const double*)y, n, c->d_scal, c->d_partial, c->stream));
  return fetch_scalars(c, 2, host_out);
}

int mpsk_vaxpby_c(mpsk_ctx* c, int64_t n, const double* alpha, const void* x, const double* beta, void* y) {
  REQUIRE(c && x && y && alpha && beta, "NULL argument");
  REQUIRE(n > 0, "bad n");
  REQUIRE(aligned16(x) && aligned16(y), "operands must be 16-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(vec_axpby_c(alpha, (const double*)x, beta, (double*)y, n, c->stream));
  return MPSK_OK;
}

// mpsk_vorth_step in complex arithmetic: CGS2 of y against xs[0..k), y <- y / ||y||, ONE host sync.  host_h: k complex
// coefficients (h = X^H y, both rounds summed), *host_beta = ||y|| before the normalisation.
int mpsk_vorth_step_c(mpsk_ctx* c, int64_t n, int k, const void* const* xs, void* y, double* host_h, double* host_beta) {
  REQUIRE(c && xs && y && host_h && host_beta, "NULL argument");
  REQUIRE(k > 0 && k <= 32 && n > 0, "needs 0 < k <= 32 and n > 0");
  REQUIRE(aligned16(y), "operands must be 16-byte aligned");
  for (int j = 0; j < k; ++j) REQUIRE(xs[j] && aligned16(xs[j]) && xs[j] != y, "basis vectors must be 16-byte aligned and distinct from y");
  HIPCHK(hipSetDevice(c->device));
  double* yy = (double*)y;
  HIPCHK(vec_cgs2_c((const double* const*)xs, k, yy, n, c->d_scal, c->d_partial, c->stream));
  HIPCHK(vec_scal_rsqrt_dev(c->d_scal + 4 * k, yy, 2 * n, c->stream));
  double tmp[MAXK];
  if (int rc = fetch_scalars(c, 4 * k + 1, tmp)) return rc;
  for (int j = 0; j < 2 * k; ++j) host_h[j] = tmp[j] + tmp[2 * k + j];
  *host_beta = tmp[4 * k] > 0.0 ? std::sqrt(tmp[4 * k]) : 0.0;
  return MPSK_OK;
}

// y = sum_j coefs[j] xs[j] with complex coefficients (host_coefs: 2k doubles); asynchronous like mpsk_vlincomb
int mpsk_vlincomb_c(mpsk_ctx* c, int64_t n, int k, const void* const* xs, const double* host_coefs, void* y) {
  REQUIRE(c && xs && y && host_coefs, "NULL argument");
  REQUIRE(k > 0 && 2 * k <= MAXK && n > 0, "bad k or n");
  REQUIRE(aligned16(y), "operands must be 16-byte aligned");
  for (int j = 0; j < k; ++j) REQUIRE(xs[j] && aligned16(xs[j]) && xs[j] != y, "inputs must be 16-byte aligned and distinct from y");
  HIPCHK(hipSetDevice(c->device));
  if (c->coef_pending) { HIPCHK(hipEventSynchronize(c->ev_coef)); c->coef_pending = false; }
  std::memcpy(c->h_coef, host_coefs, sizeof(double) * 2 * k);
  HIPCHK(hipMemcpyAsync(c->d_coef, c->h_coef, sizeof(double) * 2 * k, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipEventRecord(c->ev_coef, c->stream));
  c->coef_pending = true;
  HIPCHK(hipMemsetAsync(y, 0, sizeof(double) * 2 * n, c->stream));
  HIPCHK(vec_multiaxpy_c((const double* const*)xs, c->d_coef, k, 1.0, (double*)y, n, c->stream));
  return MPSK_OK;
}

int mpsk_vscal(mpsk_ctx* c, int64_t n, double alpha, void* x) {
  REQUIRE(c && x, "NULL argument");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(vec_scal(alpha, (double*)x, n, c->stream));
  return MPSK_OK;
}
int mpsk_vtimes_i(mpsk_ctx* c, int64_t n, const void* x, void* y) {
  REQUIRE(c && x && y, "NULL argument");
  REQUIRE(n % 2 == 0 && x != y, "needs an even length (interleaved re/im row pairs) and out-of-place operands");
  REQUIRE(((uintptr_t)x % 16 == 0) && ((uintptr_t)y % 16 == 0), "operands must be 16-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(vec_times_i((const double*)x, (double*)y, n, c->stream));
  return MPSK_OK;
}
// interleaved complex z[n] <-> planar p = [Re (n doubles) | Im (n doubles)], one memory-bound launch each way
int mpsk_vsplit_c(mpsk_ctx* c, int64_t n, const void* z, void* p) {
  REQUIRE(c && z && p, "NULL argument");
  REQUIRE(n > 0 && z != p, "needs n > 0 and out-of-place operands");
  REQUIRE(aligned16(z), "the interleaved operand must be 16-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(deinterleave((const double*)z, n, (double*)p, (double*)p + n, c->stream));
  return MPSK_OK;
}
int mpsk_vjoin_c(mpsk_ctx* c, int64_t n, const void* p, void* z) {
  REQUIRE(c && z && p, "NULL argument");
  REQUIRE(n > 0 && z != p, "needs n > 0 and out-of-place operands");
  REQUIRE(aligned16(z), "the interleaved operand must be 16-byte aligned");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(interleave((const double*)p, (const double*)p + n, n, (double*)z, c->stream));
  return MPSK_OK;
}
int mpsk_vcopy(mpsk_ctx* c, int64_t n, const void* x, void* y) {
  REQUIRE(c && x && y, "NULL argument");
  HIPCHK(hipMemcpyAsync(y, x, sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
  return MPSK_OK;
}
int mpsk_vzero(mpsk_ctx* c, int64_t n, void* x) {
  REQUIRE(c && x, "NULL argument");
  HIPCHK(hipMemsetAsync(x, 0, sizeof(double) * n, c->stream));
  return MPSK_OK;
}

}  // extern "C"
