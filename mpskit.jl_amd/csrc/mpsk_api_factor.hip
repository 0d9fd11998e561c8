// Factorization entries of the C ABI (see include/mpsk.h): QRpos / LQpos with their deferred and side-stream forms, the complex
// gauge steps on the real embedding, the truncated SVD, the two-site split and the complement SVD of the bond expansion.
#include <cstdio>
#include <cmath>
#include <algorithm>
#include "mpsk_api_internal.h"

extern "C" {

// QRpos dispatcher: CholeskyQR3 (GEMM-rich) for n > 64; when the device flag reports a non-positive pivot / a
// Gram matrix far from the identity (ill-conditioned or rank-deficient input) the perturbed, repeatedly shifted
// variant (cholqr_robust) runs, and only if that fails too the blocked Householder kernel.
static int qrpos_dispatch(mpsk_ctx* c, int m, int n, const double* A, int lda, double* Q, int ldq, double* R, int ldr,
                          double* ws) {
  std::string err;
  if (c->qr_mode != 1 && n > 64) {
    int flag = 0;
    hipError_t e = cholqr3(m, n, A, lda, Q, ldq, R, ldr, ws, c->d_flag, &flag, c->stream, c->qr_shift_fast);
    if (e != hipSuccess) return fail(MPSK_ERR_HIP, std::string("cholqr3: ") + hipGetErrorString(e));
    if (flag == 0) { c->n_qr_chol++; return MPSK_OK; }
    if (c->qr_shift_fast < 1.0) {          // breakdown with the rounding-level shift: the published shift next
      c->n_qr_retry++;
      e = cholqr3(m, n, A, lda, Q, ldq, R, ldr, ws, c->d_flag, &flag, c->stream, 1.0);
      if (e != hipSuccess) return fail(MPSK_ERR_HIP, std::string("cholqr3 (retry): ") + hipGetErrorString(e));
      if (flag == 0) { c->n_qr_chol++; return MPSK_OK; }
    }
    if (c->qr_mode == 2) return fail(MPSK_ERR_INVALID, "cholqr3: matrix too ill-conditioned / rank deficient");
    c->n_qr_fallback++;
    // second line of defence, still on the GEMM core: perturbed, repeatedly shifted CholeskyQR
    e = cholqr_robust(m, n, A, lda, Q, ldq, R, ldr, ws, c->d_flag, &flag, c->stream);
    if (e != hipSuccess) return fail(MPSK_ERR_HIP, std::string("cholqr_robust: ") + hipGetErrorString(e));
    if (flag == 0) { c->n_qr_robust++; return MPSK_OK; }
  }
  c->n_qr_house++;
  hipError_t e = qrpos(m, n, A, lda, Q, ldq, R, ldr, ws, c->stream, &err);
  if (e != hipSuccess) return fail(err.empty() ? MPSK_ERR_HIP : MPSK_ERR_INVALID, "qrpos: " + (err.empty() ? std::string(hipGetErrorString(e)) : err));
  return MPSK_OK;
}

static size_t qr_ws_doubles(int m, int n) {
  size_t a = qrpos_workspace_doubles(m, n), b = cholqr_workspace_doubles(m, n);
  return a > b ? a : b;
}

int mpsk_ctx_set_qr_mode(mpsk_ctx* c, int mode) {
  REQUIRE(c, "ctx is NULL");
  REQUIRE(mode >= 0 && mode <= 2, "mode must be 0 (auto), 1 (Householder) or 2 (CholeskyQR3 only)");
  c->qr_mode = mode;
  return MPSK_OK;
}
int mpsk_ctx_qr_stats(mpsk_ctx* c, long* n_chol, long* n_house, long* n_fallback, long* n_robust) {
  REQUIRE(c, "ctx is NULL");
  if (n_chol) *n_chol = c->n_qr_chol;
  if (n_house) *n_house = c->n_qr_house;
  if (n_fallback) *n_fallback = c->n_qr_fallback;
  if (n_robust) *n_robust = c->n_qr_robust;
  return MPSK_OK;
}

int mpsk_ctx_qr_retries(mpsk_ctx* c, long* n_retry) {
  REQUIRE(c && n_retry, "NULL argument");
  *n_retry = c->n_qr_retry;
  return MPSK_OK;
}

static int qrpos_f64(mpsk_ctx* c, int m, int n, const void* A, int lda, void* Q, int ldq, void* R, int ldr) {
  REQUIRE(c && A && Q && R, "NULL argument");
  REQUIRE(m >= n && n > 0, "needs m >= n > 0");
  REQUIRE(lda >= m && ldq >= m && ldr >= n, "leading dimension too small");
  HIPCHK(hipSetDevice(c->device));
  c->defer_next = false;                       // (single factorizations complete at once)
  if (int rc = ensure_ws(c, sizeof(double) * qr_ws_doubles(m, n))) return rc;
  return qrpos_dispatch(c, m, n, (const double*)A, lda, (double*)Q, ldq, (double*)R, ldr, c->ws.d());
}

// ---- complex128 gauge steps (ctx dtype MPSK_C128) ---------------------------------------------------------------------
// Operands are interleaved complex128 in column-major order (Julia Array{ComplexF64}): a complex m x n matrix is a real
// 2m x n matrix H whose row pairs hold (re, im); leading dimensions count COMPLEX elements.  The factorization runs on the
// real 2m x 2n embedding E = [h_0 | J h_0 | h_1 | J h_1 ...] (J (re, im) = (-im, re)): the real QRpos of an embedding is the
// embedding of the complex QRpos (R_E upper triangular with a positive diagonal, and the factorization is unique), so the
// whole CholeskyQR3 / fallback ladder is reused; the price is 2x the flops of a native complex kernel in the GEMM parts and a
// Cholesky chain of 2n instead of n columns.  Numerically the columns of Q_E along weakly determined directions are not
// embeddings (perturbed CholeskyQR, Householder completion of rank-deficient input); then Q := the structured part of Q_E,
// re-orthonormalised by a factorization that is now well conditioned, and R = triu(Q^H A) -- backward stable because those
// directions carry weight sigma_j (cplx.py: qrpos_structured, the same remedy on the host side).
__global__ __launch_bounds__(256) void cx_embed_kernel(const double* __restrict__ H, int64_t ldh, int m, int n,
                                                       double* __restrict__ E, int64_t lde) {
  const int64_t tot = (int64_t)m * n;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < tot; t += (int64_t)gridDim.x * blockDim.x) {
    const int a = (int)(t % m), b = (int)(t / m);
    const double re = H[2 * a + ldh * b], im = H[2 * a + 1 + ldh * b];
    double* e0 = E + 2 * a + lde * (2 * (int64_t)b);
    double* e1 = e0 + lde;
    e0[0] = re; e0[1] = im; e1[0] = -im; e1[1] = re;
  }
}
// H = structured part of the (nearly) embedded E: re = (E00 + E11) / 2, im = (E10 - E01) / 2; D (optional) = E - embed(H);
// upper != 0: complex entries below the diagonal are zeroed and the diagonal is made real (triangular factors); upper == 2:
// and non-negative (R = triu(Q^H A): the diagonal entry of a dependent column is a rounding error of either sign)
__global__ __launch_bounds__(256) void cx_half_kernel(const double* __restrict__ E, int64_t lde, int m, int n,
                                                      double* __restrict__ H, int64_t ldh, double* __restrict__ D, int64_t ldd,
                                                      int upper) {
  const int64_t tot = (int64_t)m * n;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < tot; t += (int64_t)gridDim.x * blockDim.x) {
    const int a = (int)(t % m), b = (int)(t / m);
    const double* e0 = E + 2 * a + lde * (2 * (int64_t)b);
    const double* e1 = e0 + lde;
    double re = 0.5 * (e0[0] + e1[1]), im = 0.5 * (e0[1] - e1[0]);
    if (upper) { if (a > b) re = im = 0.0; else if (a == b) { im = 0.0; if (upper == 2) re = fabs(re); } }
    H[2 * a + ldh * b] = re; H[2 * a + 1 + ldh * b] = im;
    if (D) {
      double* d0 = D + 2 * a + ldd * (2 * (int64_t)b);
      double* d1 = d0 + ldd;
      d0[0] = e0[0] - re; d0[1] = e0[1] - im; d1[0] = e1[0] + im; d1[1] = e1[1] - re;
    }
  }
}
// E2 (embedded 2m x 2n) = embed(H) with the dependent complex columns replaced by fixed pseudo-random ones: column b is
// dependent when a diagonal entry of its pair in the Householder factor RE is at most thresh
__global__ __launch_bounds__(256) void cx_embed_independent_kernel(const double* __restrict__ H, int64_t ldh, int m, int n,
                                                                   const double* __restrict__ RE, int64_t ldr, double thresh,
                                                                   double amp, double* __restrict__ E, int64_t lde) {
  const int64_t tot = (int64_t)m * n;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < tot; t += (int64_t)gridDim.x * blockDim.x) {
    const int a = (int)(t % m), b = (int)(t / m);
    double re = H[2 * a + ldh * b], im = H[2 * a + 1 + ldh * b];
    const double d0 = fabs(RE[2 * b + ldr * (2 * (int64_t)b)]), d1 = fabs(RE[2 * b + 1 + ldr * (2 * (int64_t)b + 1)]);
    if (d0 <= thresh || d1 <= thresh) {
      uint32_t x = (uint32_t)a * 2654435761u ^ ((uint32_t)b * 40503u + 0x9e3779b9u);
      x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
      re = amp * ((double)(x & 0xffffu) - 32767.5) / 32768.0;
      im = amp * ((double)(x >> 16) - 32767.5) / 32768.0;
    }
    double* e0 = E + 2 * a + lde * (2 * (int64_t)b);
    double* e1 = e0 + lde;
    e0[0] = re; e0[1] = im; e1[0] = -im; e1[1] = re;
  }
}
// out (n x m complex) = conjugate transpose of in (m x n complex)
__global__ __launch_bounds__(256) void cx_ctranspose_kernel(const double* __restrict__ in, int64_t ldi, int m, int n,
                                                            double* __restrict__ out, int64_t ldo) {
  const int64_t tot = (int64_t)m * n;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < tot; t += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(t % m), j = (int)(t / m);
    out[2 * j + ldo * i] = in[2 * i + ldi * j];
    out[2 * j + 1 + ldo * i] = -in[2 * i + 1 + ldi * j];
  }
}
static int qrpos_c128(mpsk_ctx* c, int m, int n, const void* A, int lda, void* Q, int ldq, void* R, int ldr) {
  REQUIRE(c && A && Q && R, "NULL argument");
  REQUIRE(m >= n && n > 0, "needs m >= n > 0");
  REQUIRE(lda >= m && ldq >= m && ldr >= n, "leading dimension too small");
  HIPCHK(hipSetDevice(c->device));
  const int m2 = 2 * m, n2 = 2 * n;
  const size_t en = (size_t)m2 * n2, rn = (size_t)n2 * n2;
  double* buf = nullptr;
  if (int rc = cx_scratch(c, 0, sizeof(double) * (3 * en + rn), &buf)) return rc;
  double *E = buf, *QE = E + en, *E2 = QE + en, *RE = E2 + en;
  const int grid = 1024;
  hipLaunchKernelGGL(cx_embed_kernel, dim3(grid), dim3(256), 0, c->stream, (const double*)A, (int64_t)2 * lda, m, n, E, (int64_t)m2);
  if (int rc = qrpos_f64(c, m2, n2, E, m2, QE, m2, RE, n2)) return rc;
  hipLaunchKernelGGL(cx_half_kernel, dim3(grid), dim3(256), 0, c->stream, QE, (int64_t)m2, m, n, (double*)Q, (int64_t)2 * ldq, E2,
                     (int64_t)m2, 0);
  double defect = 0.0;
  if (int rc = mpsk_vnrm2(c, (int64_t)en, E2, &defect)) return rc;
  if (defect <= 1.0e-13 * std::sqrt((double)n2)) {
    hipLaunchKernelGGL(cx_half_kernel, dim3(grid), dim3(256), 0, c->stream, RE, (int64_t)n2, n, n, (double*)R, (int64_t)2 * ldr,
                       (double*)nullptr, (int64_t)0, 1);
    return MPSK_OK;
  }
  // Exactly dependent columns (a zero column, a multiple of an earlier one) in front of other columns: the real kernels
  // complete Q_E by directions whose plane is not invariant under J, every later column is orthogonalised against them and
  // is no embedding either, and the spans of the structured part are no longer those of A: triu(Q^H A) would drop weight
  // below the diagonal.  The Householder factor shows such columns (a diagonal entry at rounding level); they are replaced
  // by fixed independent columns, whose QRpos is unique and so an embedding, with the same spans at every other column.
  int ndep = 0;
  double thresh = 0.0, amp = 1.0;
  if (m2 <= qrpos_max_rows()) {
    if (c->qr_mode != 1 && n2 > 64) {              // (the ladder's R does not show the rank: factor once more by Householder)
      const int keep = c->qr_mode;
      c->qr_mode = 1;
      const int rc = qrpos_f64(c, m2, n2, E, m2, QE, m2, RE, n2);
      c->qr_mode = keep;
      if (rc) return rc;
    }
    std::vector<double> dg((size_t)n2);
    HIPCHK(hipMemcpy2DAsync(dg.data(), sizeof(double), RE, sizeof(double) * (n2 + 1), sizeof(double), n2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    double dmax = 0.0;
    for (double v : dg) dmax = std::fabs(v) > dmax ? std::fabs(v) : dmax;
    thresh = 1.0e-13 * dmax;
    amp = dmax > 0.0 ? dmax : 1.0;
    for (int j = 0; j < n; ++j) ndep += (std::fabs(dg[2 * j]) <= thresh || std::fabs(dg[2 * j + 1]) <= thresh) ? 1 : 0;
  }
  if (ndep > 0) {
    hipLaunchKernelGGL(cx_embed_independent_kernel, dim3(grid), dim3(256), 0, c->stream, (const double*)A, (int64_t)2 * lda, m, n,
                       RE, (int64_t)n2, thresh, amp, E2, (int64_t)m2);
  } else {
    // structured part -> re-orthonormalise (well conditioned: structure preserving to rounding) -> R = triu(Q^H A)
    hipLaunchKernelGGL(cx_embed_kernel, dim3(grid), dim3(256), 0, c->stream, (const double*)Q, (int64_t)2 * ldq, m, n, E2, (int64_t)m2);
  }
  if (int rc = qrpos_f64(c, m2, n2, E2, m2, QE, m2, RE, n2)) return rc;
  hipLaunchKernelGGL(cx_half_kernel, dim3(grid), dim3(256), 0, c->stream, QE, (int64_t)m2, m, n, (double*)Q, (int64_t)2 * ldq,
                     (double*)nullptr, (int64_t)0, 0);
  hipLaunchKernelGGL(cx_embed_kernel, dim3(grid), dim3(256), 0, c->stream, (const double*)Q, (int64_t)2 * ldq, m, n, QE, (int64_t)m2);
  GemmArgs g = mk(QE, E, RE, n2, n2, m2, m2, m2, n2, 1, 0);
  HIPCHK(gemm_f64(g, c->stream));
  hipLaunchKernelGGL(cx_half_kernel, dim3(grid), dim3(256), 0, c->stream, RE, (int64_t)n2, n, n, (double*)R, (int64_t)2 * ldr,
                     (double*)nullptr, (int64_t)0, ndep > 0 ? 2 : 1);
  return MPSK_OK;
}
// A (m x n complex, m <= n) = L Q: the QRpos of A^H, conjugate-transposed back
static int lqpos_c128(mpsk_ctx* c, int m, int n, const void* A, int lda, void* L, int ldl, void* Q, int ldq) {
  REQUIRE(c && A && Q && L, "NULL argument");
  REQUIRE(m <= n && m > 0, "needs 0 < m <= n");
  REQUIRE(lda >= m && ldq >= m && ldl >= m, "leading dimension too small");
  HIPCHK(hipSetDevice(c->device));
  const size_t an = (size_t)2 * n * m, ln = (size_t)2 * m * m;
  double* buf = nullptr;
  if (int rc = cx_scratch(c, 1, sizeof(double) * (2 * an + ln), &buf)) return rc;
  double *At = buf, *Qt = At + an, *Rt = Qt + an;
  hipLaunchKernelGGL(cx_ctranspose_kernel, dim3(1024), dim3(256), 0, c->stream, (const double*)A, (int64_t)2 * lda, m, n, At, (int64_t)2 * n);
  if (int rc = qrpos_c128(c, n, m, At, n, Qt, n, Rt, m)) return rc;
  hipLaunchKernelGGL(cx_ctranspose_kernel, dim3(1024), dim3(256), 0, c->stream, Qt, (int64_t)2 * n, n, m, (double*)Q, (int64_t)2 * ldq);
  hipLaunchKernelGGL(cx_ctranspose_kernel, dim3(1024), dim3(256), 0, c->stream, Rt, (int64_t)2 * m, m, m, (double*)L, (int64_t)2 * ldl);
  return MPSK_OK;
}
// the ABI entry: fp64, or complex128 when the ctx dtype says so (mpsk_ctx_set_dtype; interleaved complex operands)
int mpsk_qrpos(mpsk_ctx* c, int m, int n, const void* A, int lda, void* Q, int ldq, void* R, int ldr) {
  REQUIRE(c, "ctx is NULL");
  return c->dtype == MPSK_C128 ? qrpos_c128(c, m, n, A, lda, Q, ldq, R, ldr) : qrpos_f64(c, m, n, A, lda, Q, ldq, R, ldr);
}

// completion of ONE CholeskyQR3 factorization whose launches are already on `s`: wait, read the device flag, repeat the
// third pass / run the fallbacks (robust CholeskyQR, Householder) if it asks for them.  *redone: the outputs changed
// after the enqueue (anything a caller computed from them speculatively has to be recomputed).
static int qr_complete_one(mpsk_ctx* c, int m, int n, const double* A, int lda, double* Q, int ldq, double* R, int ldr,
                           double* ws, int* d_flag, int* h_flag, hipStream_t s, bool* redone) {
  HIPCHK(hipStreamSynchronize(s));
  const int pre = *h_flag;
  hipError_t e = cholqr3_finalize(m, n, Q, ldq, R, ldr, ws, d_flag, h_flag, s);
  if (e != hipSuccess) return fail(MPSK_ERR_HIP, std::string("cholqr3 finalize: ") + hipGetErrorString(e));
  if (redone) *redone = (pre != 0);
  if (*h_flag == 0) { c->n_qr_chol++; return MPSK_OK; }
  int flag = 0;
  if (c->qr_shift_fast < 1.0) {            // breakdown with the rounding-level shift: the published shift next
    c->n_qr_retry++;
    e = cholqr3(m, n, A, lda, Q, ldq, R, ldr, ws, c->d_flag, &flag, c->stream, 1.0);
    if (e != hipSuccess) return fail(MPSK_ERR_HIP, std::string("cholqr3 (retry): ") + hipGetErrorString(e));
    if (flag == 0) { c->n_qr_chol++; return MPSK_OK; }
  }
  if (c->qr_mode == 2) return fail(MPSK_ERR_INVALID, "cholqr3: matrix too ill-conditioned / rank deficient");
  c->n_qr_fallback++;
  e = cholqr_robust(m, n, A, lda, Q, ldq, R, ldr, ws, c->d_flag, &flag, c->stream);
  if (e != hipSuccess) return fail(MPSK_ERR_HIP, std::string("cholqr_robust: ") + hipGetErrorString(e));
  if (flag == 0) { c->n_qr_robust++; return MPSK_OK; }
  c->n_qr_house++;
  std::string err;
  e = qrpos(m, n, A, lda, Q, ldq, R, ldr, ws, c->stream, &err);
  if (e != hipSuccess) return fail(err.empty() ? MPSK_ERR_HIP : MPSK_ERR_INVALID, "qrpos: " + (err.empty() ? std::string(hipGetErrorString(e)) : err));
  return MPSK_OK;
}

static int qrpos2_complete(mpsk_ctx* c, int* redone) {
  mpsk_ctx::PendingQR P = c->pend;
  c->pend.active = 0;
  bool r1 = false, r2 = false;
  // (the first factorization's fallbacks use c->ws / the main stream: both free once its own stream is drained; the
  //  second one's are run after the join, on the main stream as well)
  if (int rc = qr_complete_one(c, P.m, P.n, (const double*)P.A1, P.lda1, (double*)P.Q1, P.ldq1, (double*)P.R1, P.ldr1,
                               c->ws.d(), c->d_flag, &c->h_flags[0], c->stream, &r1)) return rc;
  HIPCHK(hipStreamSynchronize(c->stream2));
  const int pre2 = c->h_flags[1];
  hipError_t e = cholqr3_finalize(P.m, P.n, (double*)P.Q2, P.ldq2, (double*)P.R2, P.ldr2, c->ws2.d(), c->d_flag + 8,
                                  &c->h_flags[1], c->stream2);
  if (e != hipSuccess) return fail(MPSK_ERR_HIP, std::string("cholqr3 finalize (2): ") + hipGetErrorString(e));
  // join: later work on the main stream is ordered after stream2 (already drained by finalize)
  HIPCHK(hipEventRecord(c->ev_join, c->stream2));
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
  r2 = (pre2 != 0);
  bool ok2 = (c->h_flags[1] == 0);
  if (!ok2 && c->qr_shift_fast < 1.0) {    // (main stream, c->ws: the first factorization is complete)
    c->n_qr_retry++;
    int flag = 0;
    hipError_t e3 = cholqr3(P.m, P.n, (const double*)P.A2, P.lda2, (double*)P.Q2, P.ldq2, (double*)P.R2, P.ldr2,
                            c->ws.d(), c->d_flag, &flag, c->stream, 1.0);
    if (e3 != hipSuccess) return fail(MPSK_ERR_HIP, "cholqr3 (pair retry) failed");
    ok2 = (flag == 0);
  }
  if (ok2) c->n_qr_chol++;
  else {
    if (c->qr_mode == 2) return fail(MPSK_ERR_INVALID, "cholqr3: matrix too ill-conditioned / rank deficient");
    c->n_qr_fallback++;
    int flag = 0;
    hipError_t e2 = cholqr_robust(P.m, P.n, (const double*)P.A2, P.lda2, (double*)P.Q2, P.ldq2, (double*)P.R2, P.ldr2,
                                  c->ws.d(), c->d_flag, &flag, c->stream);
    if (e2 != hipSuccess) return fail(MPSK_ERR_HIP, "cholqr_robust (pair) failed");
    if (flag == 0) c->n_qr_robust++;
    else {
      c->n_qr_house++;
      std::string err;
      e2 = qrpos(P.m, P.n, (const double*)P.A2, P.lda2, (double*)P.Q2, P.ldq2, (double*)P.R2, P.ldr2, c->ws.d(), c->stream, &err);
      if (e2 != hipSuccess) return fail(MPSK_ERR_HIP, "qrpos fallback (pair) failed");
    }
  }
  if (redone) *redone = (r1 ? 1 : 0) | (r2 ? 2 : 0);
  return MPSK_OK;
}

// Two independent QRpos factorizations of equal shape, in flight together on two streams (the
// CholeskyQR3 launch chain is latency-bound, so the two chains interleave on the GPU): the DMRG sweep
// needs leftorth of the OLD AC (galerkin projector, toolbox.jl:17-22) and of the NEW AC (next site's
// AL, orthoview.jl:56) at the same moment.
int mpsk_qrpos2(mpsk_ctx* c, int m, int n, const void* A1, int lda1, void* Q1, int ldq1, void* R1, int ldr1,
                const void* A2, int lda2, void* Q2, int ldq2, void* R2, int ldr2) {
  REQUIRE(c && A1 && Q1 && R1 && A2 && Q2 && R2, "NULL argument");
  REQUIRE(m >= n && n > 0, "needs m >= n > 0");
  REQUIRE(lda1 >= m && ldq1 >= m && ldr1 >= n && lda2 >= m && ldq2 >= m && ldr2 >= n, "leading dimension too small");
  HIPCHK(hipSetDevice(c->device));
  const bool defer = c->defer_next;
  c->defer_next = false;
  const size_t wsd = qr_ws_doubles(m, n);
  if (int rc = ensure_ws(c, sizeof(double) * wsd)) return rc;
  if (c->qr_mode == 1 || n <= 64) {
    if (int rc = qrpos_dispatch(c, m, n, (const double*)A1, lda1, (double*)Q1, ldq1, (double*)R1, ldr1, c->ws.d())) return rc;
    return qrpos_dispatch(c, m, n, (const double*)A2, lda2, (double*)Q2, ldq2, (double*)R2, ldr2, c->ws.d());
  }
  if (int rc = c->ws2.reserve(sizeof(double) * wsd, "mpsk_qrpos2: workspace hipMalloc failed", c->stream2)) return rc;
  // fork: stream2 sees everything enqueued on the main stream so far (A2 / Q2 / R2 allocations and producers)
  HIPCHK(hipEventRecord(c->ev_fork, c->stream));
  HIPCHK(hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
  c->h_flags[0] = c->h_flags[1] = 0;
  hipError_t e = cholqr3_enqueue(m, n, (const double*)A1, lda1, (double*)Q1, ldq1, (double*)R1, ldr1, c->ws.d(),
                                 c->d_flag, &c->h_flags[0], c->stream, c->qr_shift_fast);
  if (e != hipSuccess) return fail(MPSK_ERR_HIP, std::string("cholqr3 (1): ") + hipGetErrorString(e));
  e = cholqr3_enqueue(m, n, (const double*)A2, lda2, (double*)Q2, ldq2, (double*)R2, ldr2, c->ws2.d(),
                      c->d_flag + 8, &c->h_flags[1], c->stream2, c->qr_shift_fast);
  if (e != hipSuccess) return fail(MPSK_ERR_HIP, std::string("cholqr3 (2): ") + hipGetErrorString(e));
  mpsk_ctx::PendingQR& P = c->pend;
  P.active = 1; P.m = m; P.n = n;
  P.A1 = A1; P.lda1 = lda1; P.Q1 = Q1; P.ldq1 = ldq1; P.R1 = R1; P.ldr1 = ldr1;
  P.A2 = A2; P.lda2 = lda2; P.Q2 = Q2; P.ldq2 = ldq2; P.R2 = R2; P.ldr2 = ldr2;
  if (defer) return MPSK_OK;                   // outputs are speculative until mpsk_qr_commit
  return qrpos2_complete(c, nullptr);
}

static int lqpos_complete(mpsk_ctx* c, int* redone) {
  mpsk_ctx::PendingQR P = c->pend;
  c->pend.active = 0;
  bool r1 = false;
  // the transposed problem: At (n x m) = Qt Rt; fallbacks write the same Qt / Rt
  if (int rc = qr_complete_one(c, P.n, P.m, P.At, P.n, P.Qt, P.n, P.Rt, P.m, P.ws, c->d_flag, &c->h_flags[0], c->stream, &r1)) return rc;
  HIPCHK(transpose(P.Qt, P.n, P.n, P.m, (double*)P.Qo, P.ldqo, c->stream));
  HIPCHK(transpose(P.Rt, P.m, P.m, P.m, (double*)P.L, P.ldl, c->stream));
  if (redone) *redone = 0;                     // L / Q are only written here: nothing speculative to redo
  (void)r1;
  return MPSK_OK;
}

// Side stream.  mpsk_ctx_side_mark records "now" on the ctx stream; mpsk_ctx_side_begin makes the ctx's second stream wait
// for that mark and routes every following mpsk_* call to it; mpsk_ctx_side_end routes calls back to the main stream, which
// waits for the side work.  The sweep marks, enqueues the (latency-bound, mostly idle) CholeskyQR chain of the next gauge
// step on the main stream, and runs the site's galerkin evaluation on the side stream underneath it.  Calls that use the
// second stream themselves (mpsk_qrpos2, mpsk_qrlq_pair, mpsk_tsplit) or the ctx workspace are refused in between.
int mpsk_ctx_side_mark(mpsk_ctx* c) {
  REQUIRE(c, "ctx is NULL");
  REQUIRE(!c->on_side, "already on the side stream");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipEventRecord(c->ev_fork, c->stream));
  return MPSK_OK;
}
int mpsk_ctx_side_begin(mpsk_ctx* c) {
  REQUIRE(c, "ctx is NULL");
  REQUIRE(!c->on_side, "already on the side stream");
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
  std::swap(c->stream, c->stream2);
  c->on_side = true;
  return MPSK_OK;
}
int mpsk_ctx_side_end(mpsk_ctx* c) {
  REQUIRE(c, "ctx is NULL");
  if (!c->on_side) return MPSK_OK;
  HIPCHK(hipSetDevice(c->device));
  HIPCHK(hipEventRecord(c->ev_join, c->stream));          // (the side stream)
  std::swap(c->stream, c->stream2);
  c->on_side = false;
  HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
  return MPSK_OK;
}

// The NEXT mpsk_qrpos2 / mpsk_lqpos call on this ctx that takes the CholeskyQR3 path returns as soon as its launches
// are enqueued; its outputs are speculative (qrpos2) / not yet written (lqpos) until mpsk_qr_commit.  Between the two
// calls only entry points that do not use the ctx workspace are accepted (mpsk_gemm, the mpsk_v* family): the sweep
// enqueues the galerkin evaluation there, so the GPU is not idle while the host waits for the success flag.
int mpsk_ctx_qr_defer(mpsk_ctx* c) {
  REQUIRE(c, "ctx is NULL");
  REQUIRE(!c->pend.active, "a deferred factorization is already pending");
  c->defer_next = true;
  return MPSK_OK;
}

// *redone: bit 0 / bit 1 = the first / second factorization of a deferred mpsk_qrpos2 was corrected after its enqueue
// (third pass repeated or a fallback ran): results computed from the speculative Q / R must be recomputed.
int mpsk_qr_commit(mpsk_ctx* c, int* redone) {
  REQUIRE(c, "ctx is NULL");
  HIPCHK(hipSetDevice(c->device));
  c->defer_next = false;
  if (redone) *redone = 0;
  if (c->pend.active == 1) return qrpos2_complete(c, redone);
  if (c->pend.active == 2) return lqpos_complete(c, redone);
  return MPSK_OK;
}

// QRpos of A1 (m x n) and LQpos of A2 (n x m) in flight together: the left-moving DMRG site update needs
// leftorth of the OLD AC (galerkin projector) and rightorth of the NEW AC (next site's AR / C) at the same moment;
// for Dl == Dr the transposed tail of the new AC has the shape of the old AC's front matrix.
int mpsk_qrlq_pair(mpsk_ctx* c, int m, int n, const void* A1, int lda1, void* Q1, int ldq1, void* R1, int ldr1,
                   const void* A2, int lda2, void* L2, int ldl2, void* Q2, int ldq2) {
  REQUIRE(c && A1 && Q1 && R1 && A2 && L2 && Q2, "NULL argument");
  REQUIRE(m >= n && n > 0, "needs m >= n > 0");
  REQUIRE(lda1 >= m && ldq1 >= m && ldr1 >= n && lda2 >= n && ldl2 >= n && ldq2 >= n, "leading dimension too small");
  REQUIRE(!c->pend.active, "a deferred factorization is pending (mpsk_qr_commit first)");
  c->defer_next = false;                       // deferral is defined for mpsk_qrpos2 / mpsk_lqpos only: this call completes at once
  HIPCHK(hipSetDevice(c->device));
  const size_t need = sizeof(double) * ((size_t)2 * m * n + (size_t)n * n + 8);
  if (int rc = c->ws3.reserve(need, "mpsk_qrlq_pair: workspace hipMalloc failed", c->stream, c->stream2)) return rc;
  double* At = c->ws3.d();                                 // m x n  (= A2^T)
  double* Qt = At + (((size_t)m * n + 1) & ~(size_t)1);         // m x n
  double* Rt = Qt + (((size_t)m * n + 1) & ~(size_t)1);         // n x n
  HIPCHK(transpose((const double*)A2, lda2, n, m, At, m, c->stream));
  if (int rc = mpsk_qrpos2(c, m, n, A1, lda1, Q1, ldq1, R1, ldr1, At, m, Qt, m, Rt, n)) return rc;
  HIPCHK(transpose(Qt, m, m, n, (double*)Q2, ldq2, c->stream));
  HIPCHK(transpose(Rt, n, n, n, (double*)L2, ldl2, c->stream));
  return MPSK_OK;
}

// LQ of A (m x n, m <= n) through the QR of A^T:  A^T = Qt Rt  ->  L = Rt^T, Q = Qt^T
static int lqpos_f64(mpsk_ctx* c, int m, int n, const void* A, int lda, void* L, int ldl, void* Q, int ldq) {
  REQUIRE(c && A && Q && L, "NULL argument");
  REQUIRE(m <= n && m > 0, "needs 0 < m <= n");
  REQUIRE(lda >= m && ldq >= m && ldl >= m, "leading dimension too small");
  HIPCHK(hipSetDevice(c->device));
  const bool defer = c->defer_next;
  c->defer_next = false;
  const size_t qws = qr_ws_doubles(n, m);
  const size_t extra = (size_t)2 * n * m + (size_t)m * m;
  if (int rc = ensure_ws(c, sizeof(double) * (qws + extra))) return rc;
  double* At = c->ws.d();            // n x m
  double* Qt = At + (size_t)n * m;        // n x m
  double* Rt = Qt + (size_t)n * m;        // m x m
  double* ws2 = Rt + (size_t)m * m;
  HIPCHK(transpose((const double*)A, lda, m, n, At, n, c->stream));
  if (defer && c->qr_mode != 1 && m > 64) {
    c->h_flags[0] = 0;
    hipError_t e = cholqr3_enqueue(n, m, At, n, Qt, n, Rt, m, ws2, c->d_flag, &c->h_flags[0], c->stream, c->qr_shift_fast);
    if (e != hipSuccess) return fail(MPSK_ERR_HIP, std::string("cholqr3: ") + hipGetErrorString(e));
    mpsk_ctx::PendingQR& P = c->pend;
    P.active = 2; P.m = m; P.n = n; P.At = At; P.Qt = Qt; P.Rt = Rt; P.ws = ws2;
    P.L = L; P.ldl = ldl; P.Qo = Q; P.ldqo = ldq;
    return MPSK_OK;
  }
  if (int rc = qrpos_dispatch(c, n, m, At, n, Qt, n, Rt, m, ws2)) return rc;
  HIPCHK(transpose(Qt, n, n, m, (double*)Q, ldq, c->stream));
  HIPCHK(transpose(Rt, m, m, m, (double*)L, ldl, c->stream));
  return MPSK_OK;
}
int mpsk_lqpos(mpsk_ctx* c, int m, int n, const void* A, int lda, void* L, int ldl, void* Q, int ldq) {
  REQUIRE(c, "ctx is NULL");
  return c->dtype == MPSK_C128 ? lqpos_c128(c, m, n, A, lda, L, ldl, Q, ldq) : lqpos_f64(c, m, n, A, lda, L, ldl, Q, ldq);
}
static int tsvd_f64(mpsk_ctx* c, int m, int n, const void* theta, int ldt, void* U, int ldu, void* S, void* Vh,
                    int ldv, int max_keep, double trunc_err, int* kept, double* disc_norm) {
  REQUIRE(c && theta && U && S && Vh && kept && disc_norm, "NULL argument");
  REQUIRE(m > 0 && n > 0, "dimensions must be positive");
  const int kmax = m < n ? m : n;
  REQUIRE(ldt >= m && ldu >= m && ldv >= kmax, "leading dimension too small");
  REQUIRE(trunc_err >= 0.0, "trunc_err must be >= 0");
  REQUIRE(!c->pend.active, "a deferred factorization is pending (mpsk_qr_commit first)");
  c->defer_next = false;
  HIPCHK(hipSetDevice(c->device));
  std::string err;
  const int mm = m < n ? n : m, nn = m < n ? m : n, transposed = m < n ? 1 : 0;
  if (c->svd_precondition && nn > 64) {
    // QR-preconditioned one-sided Jacobi: A' = theta or theta^T (tall) = Qb Rb, Jacobi on Rb^T
    const auto ev = [](size_t v) { return (v + 1) & ~(size_t)1; };   // keep every sub-buffer 16-byte aligned
    const bool dbl = c->svd_precondition >= 2;
    const size_t a_d = transposed ? ev((size_t)mm * nn) : 0, q_d = ev((size_t)mm * nn), r_d = ev((size_t)nn * nn);
    const size_t x_d = dbl ? 3 * r_d : 0;                              // Q1 / R^T, U'', Vh'' of the double preconditioning
    // (the workspace of a factorization is NOT monotone in its shape: the in-step solve / Gram of the small regime adds
    //  CQ_GS npad^2 doubles, so the square second QR can need more than the tall first one)
    const size_t qws = sizeof(double) * std::max(qr_ws_doubles(mm, nn), qr_ws_doubles(nn, nn)), sws = tsvd_workspace_bytes(nn, nn);
    if (int rc = ensure_ws(c, sizeof(double) * (a_d + q_d + r_d + x_d) + (qws > sws ? qws : sws) + 256)) return rc;
    double* At = c->ws.d();
    double* Qb = At + a_d;
    double* Rb = Qb + q_d;
    double* X0 = Rb + r_d;
    double* rest = X0 + x_d;
    const double* Ap = (const double*)theta;
    int lda = ldt;
    if (transposed) {
      HIPCHK(transpose((const double*)theta, ldt, m, n, At, mm, c->stream));
      Ap = At; lda = mm;
    }
    if (int rc = qrpos_dispatch(c, mm, nn, Ap, lda, Qb, mm, Rb, nn, rest)) return rc;
    if (dbl) {
      // Double preconditioning (Drmac-Veselic "QR of R^T", as mpsk_tsplit): R^T = Q1 R1, Jacobi on the columns of R1^T with
      // the rotations accumulated:  R^T = U2 S V2^T  (U2 = Q1 W, V2 = G S^-1)  =>  A' = Qb R = (Qb V2) S U2^T.
      // 3-4 sweeps fewer on graded spectra (each with the V update: 36 ms at 4096^2) for one n x n QRpos and one GEMM.
      double* Q1 = X0;                       // first R^T, then Q1
      double* U2 = X0 + r_d;                 // nn x kmax
      double* V2h = U2 + r_d;                // kmax x nn
      HIPCHK(transpose(Rb, nn, nn, nn, U2, nn, c->stream));
      if (int rc = qrpos_dispatch(c, nn, nn, U2, nn, Q1, nn, Rb, nn, rest)) return rc;      // Rb <- R1
      hipError_t e = tsvd(nn, nn, Rb, nn, U2, nn, (double*)S, V2h, nn, max_keep, trunc_err, kept, disc_norm, rest, c->stream,
                          &err, &c->last_svd_sweeps, Q1, nn, nn, 0, c->xstreams, 3);
      if (e != hipSuccess) return fail(MPSK_ERR_HIP, std::string("mpsk_tsvd: ") + (err.empty() ? hipGetErrorString(e) : err.c_str()));
      const int k = *kept;
      if (!transposed) {                     // theta = A':  U = Qb V2,  Vh = U2^T
        GemmArgs g = mk(Qb, V2h, (double*)U, mm, k, nn, mm, nn, ldu, 0, 1);
        HIPCHK(gemm_f64(g, c->stream));
        HIPCHK(transpose(U2, nn, nn, k, (double*)Vh, ldv, c->stream));
      } else {                               // theta^T = A':  theta = U2 S (Qb V2)^T :  U = U2,  Vh = V2^T Qb^T
        HIPCHK(hipMemcpy2DAsync(U, sizeof(double) * ldu, U2, sizeof(double) * nn, sizeof(double) * nn, k,
                                hipMemcpyDeviceToDevice, c->stream));
        GemmArgs g = mk(V2h, Qb, (double*)Vh, k, mm, nn, nn, mm, ldv, 0, 1);
        HIPCHK(gemm_f64(g, c->stream));
      }
      HIPCHK(hipStreamSynchronize(c->stream));
      return MPSK_OK;
    }
    hipError_t e = tsvd(nn, nn, Rb, nn, (double*)U, ldu, (double*)S, (double*)Vh, ldv, max_keep, trunc_err, kept,
                        disc_norm, rest, c->stream, &err, &c->last_svd_sweeps, Qb, mm, mm, transposed, c->xstreams, 3);
    if (e != hipSuccess) return fail(MPSK_ERR_HIP, std::string("mpsk_tsvd: ") + (err.empty() ? hipGetErrorString(e) : err.c_str()));
    return MPSK_OK;
  }
  if (int rc = ensure_ws(c, tsvd_workspace_bytes(m, n))) return rc;
  hipError_t e = tsvd(m, n, (const double*)theta, ldt, (double*)U, ldu, (double*)S, (double*)Vh, ldv, max_keep,
                      trunc_err, kept, disc_norm, c->ws.p, c->stream, &err, &c->last_svd_sweeps, nullptr, 0, 0, 0, c->xstreams, 3);
  if (e != hipSuccess) return fail(MPSK_ERR_HIP, std::string("mpsk_tsvd: ") + (err.empty() ? hipGetErrorString(e) : err.c_str()));
  return MPSK_OK;
}

// complex128 (ctx dtype MPSK_C128): interleaved theta / U / Vh, leading dimensions in complex elements, S real.  As the fp64
// entry, the tall orientation A' (theta or theta^H) is factored first, A' = Qb Rb (qrpos_c128), and the Jacobi runs on
// Rb^H.  ONE workspace plan covers the whole call, reserved before anything runs:
//   c->ws = [ region 0 | A^H (wide input only) | Qb | Rb ]
//   region 0 = max(the real workspace of the embedded QRpos inside qrpos_c128 (qrpos_f64 on 2 mm x 2 nn, at c->ws + 0),
//                  the Jacobi workspace (tsvd_c128_workspace_bytes)) -- the QR is finished before the Jacobi starts.
// qrpos_c128's own ensure_ws then finds the workspace large enough and never moves it under Qb / Rb.
static int tsvd_c128_entry(mpsk_ctx* c, int m, int n, const void* theta, int ldt, void* U, int ldu, void* S, void* Vh,
                           int ldv, int max_keep, double trunc_err, int* kept, double* disc_norm) {
  REQUIRE(c && theta && U && S && Vh && kept && disc_norm, "NULL argument");
  REQUIRE(m > 0 && n > 0, "dimensions must be positive");
  const int kmax = m < n ? m : n;
  REQUIRE(ldt >= m && ldu >= m && ldv >= kmax, "leading dimension too small");
  REQUIRE(trunc_err >= 0.0, "trunc_err must be >= 0");
  REQUIRE(!c->pend.active, "a deferred factorization is pending (mpsk_qr_commit first)");
  c->defer_next = false;
  HIPCHK(hipSetDevice(c->device));
  std::string err;
  const int mm = m < n ? n : m, nn = m < n ? m : n, transposed = m < n ? 1 : 0;
  hipError_t e = hipSuccess;
  if (c->svd_precondition && nn > 64) {
    const size_t a_d = transposed ? 2 * ev2((size_t)mm * nn) : 0, q_d = 2 * ev2((size_t)mm * nn), r_d = 2 * ev2((size_t)nn * nn);
    size_t r0 = sizeof(double) * qr_ws_doubles(2 * mm, 2 * nn);
    r0 = std::max(r0, tsvd_c128_workspace_bytes(nn, nn, mm));
    r0 = (r0 + 255) & ~(size_t)255;
    if (int rc = ensure_ws(c, r0 + sizeof(double) * (a_d + q_d + r_d))) return rc;
    double* At = (double*)((char*)c->ws.p + r0);
    double* Qb = At + a_d;
    double* Rb = Qb + q_d;
    const void* Ap = theta;
    int lda = ldt;
    if (transposed) {
      hipLaunchKernelGGL(cx_ctranspose_kernel, dim3(1024), dim3(256), 0, c->stream, (const double*)theta, (int64_t)2 * ldt, m, n,
                         At, (int64_t)2 * mm);
      Ap = At; lda = mm;
    }
    if (int rc = qrpos_c128(c, mm, nn, Ap, lda, Qb, mm, Rb, nn)) return rc;
    e = tsvd_c128(nn, nn, Rb, nn, (double*)U, ldu, (double*)S, (double*)Vh, ldv, max_keep, trunc_err, kept, disc_norm, c->ws.p,
                  c->stream, &err, &c->last_svd_sweeps, Qb, mm, mm, transposed);
  } else {
    if (int rc = ensure_ws(c, tsvd_c128_workspace_bytes(m, n, 0))) return rc;
    e = tsvd_c128(m, n, (const double*)theta, ldt, (double*)U, ldu, (double*)S, (double*)Vh, ldv, max_keep, trunc_err, kept,
                  disc_norm, c->ws.p, c->stream, &err, &c->last_svd_sweeps, nullptr, 0, 0, 0);
  }
  if (e != hipSuccess) return fail(MPSK_ERR_HIP, std::string("mpsk_tsvd (C128): ") + (err.empty() ? hipGetErrorString(e) : err.c_str()));
  return MPSK_OK;
}

// the ABI entry: fp64, or complex128 when the ctx dtype says so (mpsk_ctx_set_dtype)
int mpsk_tsvd(mpsk_ctx* c, int m, int n, const void* theta, int ldt, void* U, int ldu, void* S, void* Vh,
              int ldv, int max_keep, double trunc_err, int* kept, double* disc_norm) {
  REQUIRE(c, "ctx is NULL");
  return c->dtype == MPSK_C128 ? tsvd_c128_entry(c, m, n, theta, ldt, U, ldu, S, Vh, ldv, max_keep, trunc_err, kept, disc_norm)
                               : tsvd_f64(c, m, n, theta, ldt, U, ldu, S, Vh, ldv, max_keep, trunc_err, kept, disc_norm);
}

// Truncated two-site split  theta ~ AL . C . AR  (tsvd!(theta; trunc) followed by al, c, ar of dmrg.jl:96-104 /
// tdvp.jl:124-126) WITHOUT accumulating the Jacobi rotations: QRpos of the tall orientation, V-free block Jacobi on
// R^T -> singular values and the singular vectors of ONE side (exact, orthonormal); the other factor is rebuilt from
// theta itself and re-orthonormalised by QRpos / LQpos, so AL, AR are isometries to rounding and
// AL C AR = theta projected on the kept singular subspace; C is triangular instead of diag(S) (S is returned too).
// ---- truncation-aware stage of mpsk_tsplit (svd mode 3) ---------------------------------------------------------------
// When only k = max_keep << n singular triplets are kept, the block-Jacobi iteration on all n columns (127 rounds a sweep at
// n = 4096, ~10 sweeps) is replaced by
//   1. a randomized subspace iteration for the dominant right subspace of the tall orientation A' (mm x nn):
//        Y <- orth(A'^T orth(A' Y)),   Y: nn x r,  r = k + max(64, k / 2) rounded up to 64
//      -- two GEMMs on the MFMA core and two ONE-pass shifted CholeskyQR re-conditionings per iteration (only the span
//      matters; the error of the i-th direction shrinks by (sigma_{r+1} / sigma_i)^2 per iteration);
//   2. W = QRpos(Y) (working accuracy), B' = A' W (mm x r), and the usual preconditioned V-free Jacobi split on B': r
//      columns instead of nn (r = 1536 of 4096: 47 rounds a sweep instead of 127, 24 pairs a round instead of 64);
//   3. a CHECK, not an estimate: with U_k the kept left vectors and M = U_k^T A' (formed anyway for the LQpos / QRpos that
//      delivers the other factor),  rho = || M (I - W W^T) ||_F / ||theta||_F  is the part of the kept triplets that lies
//      outside the iterated subspace.  rho <= MPSK_SPLIT_TOL (1e-12): done.  Otherwise the iteration continues from the r
//      left Ritz vectors for the number of iterations the measured Ritz ratio predicts, or -- if that would cost more than
//      the full iteration -- the call falls through to mode 2.  Nothing is returned that has not passed the check.
// M is computed with the full theta, so C . AR = U_k^T theta exactly as in mode 2; S holds the r leading values (Ritz values
// of a converged subspace: errors O(rho^2)), the remaining entries are NaN.
__global__ __launch_bounds__(256) void split_fill_kernel(double* __restrict__ y, int64_t n, unsigned seed) {
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < n; e += (int64_t)gridDim.x * blockDim.x) {
    unsigned h = (unsigned)(e & 0xffffffffu) * 0x9E3779B1u ^ ((unsigned)(e >> 32) + seed) * 0x85EBCA77u;
    h ^= h >> 15; h *= 0x2C1B3C6Du; h ^= h >> 12; h *= 0x297A2D39u; h ^= h >> 15;
    y[e] = ((double)h + 0.5) * (2.0 / 4294967296.0) - 1.0;       // uniform in (-1, 1)
  }
}
__global__ __launch_bounds__(256) void split_fill_nan_kernel(double* __restrict__ y, int n) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n) y[e] = __longlong_as_double(0x7ff8000000000000LL);
}

// X (rows x cols, ld) = alpha * A (lda)   /   leading rows x cols of the identity
__global__ __launch_bounds__(256) void split_scale_copy_kernel(const double* __restrict__ A, int64_t lda, int rows, int cols,
                                                               double alpha, double* __restrict__ X, int64_t ldx) {
  const int64_t tot = (int64_t)rows * cols;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < tot; t += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(t % rows), c = (int)(t / rows);
    X[r + ldx * c] = A ? alpha * A[r + lda * c] : (r == c ? 1.0 : 0.0);
  }
}

// *out = max |A[r, c]| as the bit pattern of a non-negative double (order preserving under unsigned compare); NaN -> +inf bits
__global__ __launch_bounds__(256) void split_absmax_kernel(const double* __restrict__ A, int64_t lda, int rows, int cols,
                                                           unsigned long long* __restrict__ out) {
  const int64_t tot = (int64_t)rows * cols;
  double mx = 0.0;
  for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < tot; t += (int64_t)gridDim.x * blockDim.x) {
    const double v = fabs(A[(t % rows) + lda * (t / rows)]);
    mx = (v > mx || v != v) ? (v != v ? INFINITY : v) : mx;
  }
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(out, (unsigned long long)__double_as_longlong(mx));
}

struct SplitSub {             // state of the subspace stage across refinements
  int r = 0;
  double *Yb = nullptr, *Zb = nullptr, *Wb = nullptr, *Bp = nullptr;   // nn x r, mm x r, nn x r, mm x r
};

// one re-conditioning pass X -> Q (span preserved): rounding-level shift first, the published shift if a pivot broke down
static int split_orth1(mpsk_ctx* c, int m, int r, const double* X, double* Q) {
  HIPCHK(cholqr1_orth(m, r, X, m, Q, m, c->ws.d(), c->d_flag, c->stream, c->qr_shift_fast));
  int flag = 0;
  HIPCHK(hipMemcpyAsync(&flag, c->d_flag, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (flag) HIPCHK(cholqr1_orth(m, r, X, m, Q, m, c->ws.d(), c->d_flag, c->stream, 1.0));
  return MPSK_OK;
}
// q iterations  Y <- orth1(A'^T orth1(A' Y))  starting from Yb (nn x r); result in Yb.  Zb / Wb / Bp are scratch.
static int split_iterate(mpsk_ctx* c, int mm, int nn, const double* Ap, int lda, const SplitSub& sb, int q) {
  const int r = sb.r;
  const bool trace = getenv("MPSK_SPLIT_TRACE") != nullptr;
  auto stage = [&](const char* name, int i) {
    if (!trace) return;
    hipError_t e_ = hipStreamSynchronize(c->stream);
    fprintf(stderr, "[mpsk_tsplit]   iteration %d %-12s %s\n", i, name, hipGetErrorString(e_)); fflush(stderr);
  };
  for (int i = 0; i < q; ++i) {
    GemmArgs g = mk(Ap, sb.Yb, sb.Zb, mm, r, nn, lda, nn, mm);
    HIPCHK(gemm_f64(g, c->stream));
    stage("Z = A' Y", i);
    if (int rc = split_orth1(c, mm, r, sb.Zb, sb.Bp)) return rc;
    stage("orth1(Z)", i);
    GemmArgs g2 = mk(Ap, sb.Bp, sb.Wb, nn, r, mm, lda, mm, nn, 1, 0);
    HIPCHK(gemm_f64(g2, c->stream));
    stage("Y = A'^T Z", i);
    if (int rc = split_orth1(c, nn, r, sb.Wb, sb.Yb)) return rc;
    stage("orth1(Y)", i);
  }
  return MPSK_OK;
}

static int tsplit_core(mpsk_ctx* c, int m, int n, const void* theta, int ldt, int max_keep, double trunc_err,
                       void* AL, int ldal, void* Cm, int ldc, void* AR, int ldar, void* S, int* kept, double* disc_norm) {
  REQUIRE(c && theta && AL && Cm && AR && S && kept && disc_norm, "NULL argument");
  REQUIRE(m > 0 && n > 0, "dimensions must be positive");
  const int mm = m < n ? n : m, nn = m < n ? m : n, transposed = m < n ? 1 : 0;
  REQUIRE(nn > 64, "mpsk_tsplit needs min(m, n) > 64 (use mpsk_tsvd for small tensors)");
  REQUIRE(ldt >= m && ldal >= m && ldc >= 1 && ldar >= 1, "leading dimension too small");
  REQUIRE(trunc_err >= 0.0, "trunc_err must be >= 0");
  REQUIRE(!c->pend.active, "a deferred factorization is pending (mpsk_qr_commit first)");
  c->defer_next = false;                       // (the inner mpsk_qrpos / mpsk_lqpos calls complete at once)
  HIPCHK(hipSetDevice(c->device));
  // truncation-aware stage: worth it while r columns are well below nn (the Jacobi part scales ~ r^2, the iteration ~ q r)
  static const double sub_over = getenv("MPSK_SPLIT_OVERSAMPLE") ? atof(getenv("MPSK_SPLIT_OVERSAMPLE")) : 0.5;
  static const double sub_tol = getenv("MPSK_SPLIT_TOL") ? atof(getenv("MPSK_SPLIT_TOL")) : 1.0e-12;
  int r_sub = 0;
  if (c->split_skip > 0) --c->split_skip;          // (backing off after the stage gave up: see below)
  else if (c->svd_precondition == 3 && max_keep > 0 && ldt == m) {
    // r = k + max(64, k / 2) while that stays within 5/8 of the columns (d >= 3 chains: k = n / d), else k + max(64, k / 4)
    // (d = 2: k = n / 2, r = 5n / 8: 2048^2 -> 1024 50 ms against 68, 4096^2 -> 2048 180 against 255; more iterations but
    // the Jacobi stage, ~ r^2, is what counts), else no stage
    static const double sub_frac = getenv("MPSK_SPLIT_MAXFRAC") ? atof(getenv("MPSK_SPLIT_MAXFRAC")) : 0.625;
    for (double ov : {sub_over, 0.5 * sub_over}) {
      int over = (int)std::ceil(ov * max_keep);
      if (over < 64) over = 64;
      r_sub = (max_keep + over + 63) / 64 * 64;
      if (r_sub <= (int)(nn * sub_frac) && r_sub > 64) break;
      r_sub = 0;
    }
  }
  const size_t a_d = transposed ? ev2((size_t)mm * nn) : 0, q_d = ev2((size_t)mm * nn), r_d = ev2((size_t)nn * nn);
  const size_t t_d = ev2((size_t)mm * nn);
  const size_t s_d = r_sub ? 2 * ev2((size_t)nn * r_sub) + 2 * ev2((size_t)mm * r_sub) : 0;
  const size_t need = sizeof(double) * (a_d + q_d + 2 * r_d + t_d + s_d + 8);
  if (int rc = c->ws3.reserve(need, "mpsk_tsplit: workspace hipMalloc failed", c->stream, c->stream2)) return rc;
  double* At = c->ws3.d();            // theta^T when m < n
  double* Qb = At + a_d;                   // Q of the preconditioning QR of the tall orientation A' (mm x nn)
  double* Rb = Qb + q_d;                   // R (nn x nn); R1 of the second pass
  double* Y = Rb + r_d;                    // sorted, normalised singular vectors from the Jacobi iteration (nn x nn)
  double* T = Y + r_d;                     // scratch: R^T, then theta V_k / U_k^T theta
  SplitSub sb;
  sb.r = r_sub;
  sb.Yb = T + t_d; sb.Zb = sb.Yb + ev2((size_t)nn * r_sub); sb.Wb = sb.Zb + ev2((size_t)mm * r_sub);
  sb.Bp = sb.Wb + ev2((size_t)nn * r_sub);
  const double* Ap = (const double*)theta;
  int lda = ldt;
  if (transposed) {
    HIPCHK(transpose((const double*)theta, ldt, m, n, At, mm, c->stream));
    Ap = At; lda = mm;
  }
  // every factorization below runs in c->ws.  Its size is NOT monotone in the shape (the in-step solve / Gram of the small
  // regime adds CQ_GS npad^2 doubles: a 1280 x 1280 QRpos needs 3x the workspace of a 2048 x 2048 one), so take the maximum
  // over all shapes this call can factor: A' (mm x nn), R^T (nn x nn) and, with the subspace stage, Y (nn x r), A'Y / B'
  // (mm x r), R_B^T (r x r)
  size_t qwd = std::max(qr_ws_doubles(mm, nn), qr_ws_doubles(nn, nn));
  if (r_sub) qwd = std::max(std::max(qwd, qr_ws_doubles(nn, r_sub)), std::max(qr_ws_doubles(mm, r_sub), qr_ws_doubles(r_sub, r_sub)));
  const size_t qws = sizeof(double) * qwd, sws = tsvd_workspace_bytes(nn, nn);
  if (int rc = ensure_ws(c, (qws > sws ? qws : sws) + 256)) return rc;
  const bool dbl = c->svd_precondition >= 2;
  c->last_split_iters = 0; c->last_split_resid = 0.0; c->last_split_path = 0;

  // attempt 0: the truncation-aware stage (when configured); attempt 1 (or the only one): the full iteration
  // test hook (tests/test_gpu_ops.py): one iteration and the residual check waved through, so that the dominance probe is
  // the only line of defence -- it must then send the call to the full iteration
  const bool dbg_skip_check = getenv("MPSK_SPLIT_DEBUG_SKIP_CHECK") != nullptr;
  const bool dbg_trace = getenv("MPSK_SPLIT_TRACE") != nullptr;      // sync + one stderr line per stage (fault localisation)
#define SPLIT_STAGE(name) do { if (dbg_trace) { hipError_t e_ = hipStreamSynchronize(c->stream); \
    fprintf(stderr, "[mpsk_tsplit] stage %-28s %s\n", name, hipGetErrorString(e_)); fflush(stderr); } } while (0)
  double theta_nrm = 0.0, rho_prev = 0.0;
  int q_total = 0, q_prev = 0, n_checks = 0;
  bool sub_ready = false;                  // sb.Yb holds a basis to continue from
  for (int attempt = 0; attempt < 8; ++attempt) {
    const bool sub = r_sub > 0 && c->last_split_path != 2;
    const int nc = sub ? r_sub : nn;       // columns of the matrix the Jacobi split runs on
    const double* Bsrc = Ap;
    int ldb = lda;
    double te = trunc_err;
    if (sub) {
      if (!sub_ready) {
        if (int rc = mpsk_vnrm2(c, (int64_t)m * n, theta, &theta_nrm)) return rc;
        hipLaunchKernelGGL(split_fill_kernel, dim3(1024), dim3(256), 0, c->stream, sb.Yb, (int64_t)nn * r_sub, 0x5eedu);
        const auto hit = c->split_q_hint.find(std::make_pair(nn, r_sub));
        int q0 = hit == c->split_q_hint.end() ? 8 : hit->second;
        if (q0 < 2) q0 = 2;
        if (dbg_skip_check) q0 = 1;
        if (int rc = split_iterate(c, mm, nn, Ap, lda, sb, q0)) return rc;
        SPLIT_STAGE("iterate");
        q_total += q0;
        sub_ready = true;
      }
      // W = QRpos(Y) to working accuracy (R is not needed: Rb is scratch here), B' = A' W
      if (int rc = qrpos_dispatch(c, nn, r_sub, sb.Yb, nn, sb.Wb, nn, Rb, r_sub, c->ws.d())) return rc;
      SPLIT_STAGE("QRpos(Y)");
      GemmArgs gb = mk(Ap, sb.Wb, sb.Bp, mm, r_sub, nn, lda, nn, mm);
      HIPCHK(gemm_f64(gb, c->stream));
      Bsrc = sb.Bp; ldb = mm;
      SPLIT_STAGE("B' = A' W");
      if (trunc_err > 0.0) {               // weight outside the subspace counts as discarded in the truncerr rule
        double bn = 0.0;
        if (int rc = mpsk_vnrm2(c, (int64_t)mm * r_sub, sb.Bp, &bn)) return rc;
        const double out2 = std::max(theta_nrm * theta_nrm - bn * bn, 0.0);
        te = std::sqrt(std::max(trunc_err * trunc_err - out2, 0.0));
        if (te == 0.0) te = 1.0e-300;
      }
    }
    if (int rc = qrpos_dispatch(c, mm, nc, Bsrc, ldb, Qb, mm, Rb, nc, c->ws.d())) return rc;
    SPLIT_STAGE("QRpos(B')");
    // Double preconditioning (svd mode 2, Drmac-Veselic: "QR of R^T"): R^T = Q1 R1, Jacobi on the columns of R1^T.
    // A' = Qb R = Qb R1^T Q1^T, and R1^T W = G = Y Sigma at convergence, so  A' = (Qb Y) Sigma (Q1 W)^T : the V-free
    // iteration now yields the LEFT singular vectors Qb Y of the tall orientation (orthonormal to rounding as a product of
    // orthonormal factors) and costs fewer sweeps (9 -> 6 at n = 512, 10 -> 7 at n = 1024 in the block-Jacobi model with
    // exact inner solves; measured sweep counts: profiles/r02_svd_modes.log) for one extra n x n QRpos.
    if (dbl) {
      HIPCHK(transpose(Rb, nc, nc, nc, T, nc, c->stream));
      if (int rc = qrpos_dispatch(c, nc, nc, T, nc, Y, nc, Rb, nc, c->ws.d())) return rc;     // Y = Q1 (not needed), Rb = R1
      SPLIT_STAGE("QRpos(R^T)");
    }
    std::string err;
    hipError_t e = tsvd(nc, nc, Rb, nc, Y, nc, (double*)S, nullptr, 1, max_keep, te, kept, disc_norm, c->ws.p, c->stream,
                        &err, &c->last_svd_sweeps, nullptr, 0, 0, 0, c->xstreams, 3, /*vfree=*/1);
    if (e == hipErrorNotReady && sub) {      // the Jacobi stage on B' did not converge: nothing is lost, take the full iteration
      c->last_split_path = 2;
      continue;
    }
    if (e != hipSuccess) return fail(MPSK_ERR_HIP, std::string("mpsk_tsplit: ") + (err.empty() ? hipGetErrorString(e) : err.c_str()));
    const int k = *kept;
    REQUIRE(ldc >= k && ldar >= k, "leading dimension of C / AR smaller than the kept rank");
    SPLIT_STAGE("jacobi");
    // the factor that carries theta: M' = U_k'^T A' (k x nn) as T (k x n) when A' = theta, as T^T (m x k) when A' = theta^T
    double* Vk = At;                       // (transposed) theta^T is no longer needed once the iteration is over: see below
    if (!dbl) {
      if (!transposed) {
        // theta (m x n): Y_k = right singular vectors.  B = theta Y_k = U_k S_k ; AL C = QRpos(B) ; AR = Y_k^T
        GemmArgs g = mk((const double*)theta, Y, T, m, k, n, ldt, nn, m);
        HIPCHK(gemm_f64(g, c->stream));
        if (int rc = qrpos_f64(c, m, k, T, m, AL, ldal, Cm, ldc)) return rc;
        HIPCHK(transpose(Y, nn, n, k, (double*)AR, ldar, c->stream));
      } else {
        // theta (m x n), m < n: Y_k = left singular vectors = AL.  M = Y_k^T theta = S_k V_k^T ; C AR = LQpos(M)
        HIPCHK(hipMemcpy2DAsync(AL, sizeof(double) * ldal, Y, sizeof(double) * nn, sizeof(double) * m, k,
                                hipMemcpyDeviceToDevice, c->stream));
        GemmArgs g = mk(Y, (const double*)theta, T, k, n, m, nn, ldt, k, 1, 0);
        HIPCHK(gemm_f64(g, c->stream));
        if (int rc = lqpos_f64(c, k, n, T, k, Cm, ldc, AR, ldar)) return rc;
      }
      return MPSK_OK;
    }
    if (!transposed) {
      // A' = theta: AL = Qb Y_k (left singular vectors).  M = AL^T theta = S_k V_k^T ; C AR = LQpos(M)
      GemmArgs g = mk(Qb, Y, (double*)AL, m, k, nc, mm, nc, ldal);
      HIPCHK(gemm_f64(g, c->stream));
      GemmArgs g2 = mk((const double*)AL, (const double*)theta, T, k, n, m, ldal, ldt, k, 1, 0);
      HIPCHK(gemm_f64(g2, c->stream));
    } else {
      // A' = theta^T (n x m): V_k = Qb Y_k = right singular vectors of theta.  B = theta V_k = U_k S_k ; AL C = QRpos(B) ; AR = V_k^T
      if (sub) Vk = sb.Zb;                 // At (theta^T) is still needed if the check sends us back into the iteration
      GemmArgs g = mk(Qb, Y, Vk, n, k, nc, mm, nc, n);
      HIPCHK(gemm_f64(g, c->stream));
      GemmArgs g2 = mk((const double*)theta, Vk, T, m, k, n, ldt, n, m);
      HIPCHK(gemm_f64(g2, c->stream));
    }
    if (sub) {
      // the check: rho = || M' (I - W W^T) ||_F / ||theta||_F  (M' = T, k x nn, or T^T = B, nn x k)
      double* P1 = sb.Yb;                  // r x k (or k x r) scratch: Yb is rebuilt below if the iteration continues
      double* Rs = transposed ? sb.Bp : sb.Zb;     // residual, k x nn / nn x k  (Bp / Zb are free now; Vk may live in Zb)
      double rho = 0.0;
      if (!transposed) {
        GemmArgs p = mk(T, sb.Wb, P1, k, r_sub, nn, k, nn, k);                    // P1 = M' W            (k x r)
        HIPCHK(gemm_f64(p, c->stream));
        HIPCHK(hipMemcpyAsync(Rs, T, sizeof(double) * (size_t)k * nn, hipMemcpyDeviceToDevice, c->stream));
        GemmArgs p2 = mk(P1, sb.Wb, Rs, k, nn, r_sub, k, nn, k, 0, 1);            // Rs = M' - P1 W^T
        p2.alpha = -1.0; p2.beta = 1.0;
        HIPCHK(gemm_f64(p2, c->stream));
      } else {
        GemmArgs p = mk(sb.Wb, T, P1, r_sub, k, nn, nn, nn, r_sub, 1, 0);         // P1 = W^T B           (r x k)
        HIPCHK(gemm_f64(p, c->stream));
        HIPCHK(hipMemcpyAsync(Rs, T, sizeof(double) * (size_t)k * nn, hipMemcpyDeviceToDevice, c->stream));
        GemmArgs p2 = mk(sb.Wb, P1, Rs, nn, k, r_sub, nn, r_sub, nn);             // Rs = B - W P1
        p2.alpha = -1.0; p2.beta = 1.0;
        HIPCHK(gemm_f64(p2, c->stream));
      }
      if (int rc = mpsk_vnrm2(c, (int64_t)k * nn, Rs, &rho)) return rc;
      SPLIT_STAGE("check");
      rho = theta_nrm > 0.0 ? rho / theta_nrm : rho;
      if (dbg_skip_check) rho = 0.0;
      c->last_split_iters = q_total; c->last_split_resid = rho;
      ++n_checks;
      // Ritz ratio sigma~_r / sigma~_k: an upper bound of the convergence factor sigma_{r+1} / sigma_k per half iteration
      std::vector<double> hs(r_sub);
      HIPCHK(hipMemcpyAsync(hs.data(), S, sizeof(double) * r_sub, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      const double ratio = (hs[k - 1] > 0.0 && std::isfinite(rho)) ? hs[r_sub - 1] / hs[k - 1] : 1.0;
      if (getenv("MPSK_SVD_DEBUG"))
        fprintf(stderr, "[mpsk_tsplit] subspace stage: r = %d of %d, %d iterations, residual %.3e (tol %.1e), Ritz ratio s_r / s_k = %.3f, %d Jacobi sweeps\n",
                r_sub, nn, q_total, rho, sub_tol, ratio, c->last_svd_sweeps);
      // (the check is blind to a collapsed basis -- U_k = 0 has residual 0 -- so the kept left vectors must also be an isometry)
      {
        double un = 0.0;
        if (!transposed) { if (int rc = mpsk_vnrm2(c, (int64_t)m * k, AL, &un)) return rc; }
        else { if (int rc = mpsk_vnrm2(c, (int64_t)n * k, Vk, &un)) return rc; }
        if (!(std::fabs(un * un - (double)k) <= 1.0e-8 * k) && !(ldal != m && !transposed)) rho = INFINITY;
      }
      if (!(rho <= sub_tol)) {
        // not there: iterations still needed from the measured check value
        // (a Ritz ratio taken before convergence UNDERestimates sigma_{r+1} / sigma_k -- sigma~_r is still far below
        // sigma_r --, so from the second check on the OBSERVED decay of the check value per iteration is used instead)
        int q_more = 1 << 20;
        double fac = ratio < 0.97 ? ratio * ratio : 1.0;              // error factor per iteration
        if (rho_prev > 0.0 && rho < rho_prev && q_total > q_prev) fac = std::pow(rho / rho_prev, 1.0 / (q_total - q_prev));
        else fac = std::sqrt(fac);                                    // first check: assume half the predicted rate
        if (fac < 0.95 && std::isfinite(rho)) q_more = (int)std::ceil(std::log(0.1 * sub_tol / rho) / std::log(fac));
        if (q_more < 2) q_more = 2;
        rho_prev = rho; q_prev = q_total;
        // budget: one iteration ~ 4 n^2 r flops + two Cholesky chains; the full Jacobi iteration ~ 10 sweeps of 6 n^3 / ... :
        // in measured terms (4096^2, r = 1536) 3.7 ms against ~200 ms, i.e. ~50 iterations; scaled by r / nn it stays ~40
        const int q_cap = 40;
        if (attempt >= 3 || q_total + q_more > q_cap) {
          c->last_split_path = 2;          // fall through to the full iteration; flat spectra come in runs (the early
          c->split_q_hint.erase(std::make_pair(nn, r_sub));   // sweeps of a chain), so the next calls skip the stage: 4, 8, ... 64 of them
          c->split_backoff = c->split_backoff ? std::min(2 * c->split_backoff, 64) : 4;
          c->split_skip = c->split_backoff;
          continue;
        }
        // continue from the r left Ritz vectors: Z = Qb Y (mm x r), Y <- orth1(A'^T Z), then q_more iterations
        GemmArgs gz = mk(Qb, Y, sb.Zb, mm, r_sub, r_sub, mm, r_sub, mm);
        HIPCHK(gemm_f64(gz, c->stream));
        GemmArgs gy = mk(Ap, sb.Zb, sb.Wb, nn, r_sub, mm, lda, mm, nn, 1, 0);
        HIPCHK(gemm_f64(gy, c->stream));
        if (int rc = split_orth1(c, nn, r_sub, sb.Wb, sb.Yb)) return rc;
        if (int rc = split_iterate(c, mm, nn, Ap, lda, sb, q_more)) return rc;
        q_total += q_more + 1;
        continue;
      }
      c->last_split_path = 1;
      c->split_backoff = 0;
      // next call's first guess (neighbouring bonds of a chain have similar spectra): what this one took, one less when
      // the first check already passed with two digits to spare (a failed check costs a second Jacobi stage, ~15 iterations'
      // worth; an iteration too many costs one)
      c->split_q_hint[std::make_pair(nn, r_sub)] = (n_checks == 1 && rho <= 1.0e-2 * sub_tol && q_total > 3) ? q_total - 1 : q_total;
      // S: the r leading values are Ritz values of the converged subspace; the rest is not computed
      if (nn > r_sub)
        hipLaunchKernelGGL(split_fill_nan_kernel, dim3((nn - r_sub + 255) / 256), dim3(256), 0, c->stream, (double*)S + r_sub, nn - r_sub);
      // discarded weight: || theta - AL M ||_F formed directly (theta_nrm^2 - |M|^2 cancels when little is discarded);
      // Qb (mm x nn) is free once AL / V_k exist
      double* Dm = Qb;
      HIPCHK(hipMemcpy2DAsync(Dm, sizeof(double) * m, theta, sizeof(double) * ldt, sizeof(double) * m, n, hipMemcpyDeviceToDevice, c->stream));
      if (!transposed) {
        GemmArgs gd = mk((const double*)AL, T, Dm, m, n, k, ldal, k, m);
        gd.alpha = -1.0; gd.beta = 1.0;
        HIPCHK(gemm_f64(gd, c->stream));
      } else {
        GemmArgs gd = mk(T, Vk, Dm, m, n, k, m, n, m, 0, 1);                      // theta - (theta V_k) V_k^T
        gd.alpha = -1.0; gd.beta = 1.0;
        HIPCHK(gemm_f64(gd, c->stream));
      }
      if (int rc = mpsk_vnrm2(c, (int64_t)m * n, Dm, disc_norm)) return rc;
      SPLIT_STAGE("remainder");
      // dominance probe.  The check above certifies that span(AL) is INVARIANT (a singular subspace of theta); that it is
      // the DOMINANT one rests on the random start having a component along every leading direction (probability one, and
      // r - k >= 64 spare columns).  Cheap insurance against the measure-zero case: a few power iterations on the
      // remainder D = theta - AL M, whose largest singular value must be sigma_{k+1} <= S[k-1]; a left-out direction well
      // above the cut would dominate D and show after 6 steps ((2/3)^12 < 1e-2 for sigma_miss = 1.5 S[k-1]).
      {
        double* xv = sb.Bp;                // n, then m doubles (Bp, mm x r, is free by now)
        double* yv = sb.Bp + ev2((size_t)n);
        hipLaunchKernelGGL(split_fill_kernel, dim3(64), dim3(256), 0, c->stream, xv, (int64_t)n, 0xd0a1u);
        double est = 0.0;
        for (int it = 0; it < 6; ++it) {
          double nx = 0.0;
          if (int rc = mpsk_vnrm2(c, n, xv, &nx)) return rc;
          if (!(nx > 0.0)) break;
          HIPCHK(vec_scal(1.0 / nx, xv, n, c->stream));
          GemmArgs gy = mk(Dm, xv, yv, m, 1, n, m, n, m);
          HIPCHK(gemm_f64(gy, c->stream));
          if (int rc = mpsk_vnrm2(c, m, yv, &est)) return rc;
          GemmArgs gx = mk(Dm, yv, xv, n, 1, m, m, m, n, 1, 0);
          HIPCHK(gemm_f64(gx, c->stream));
        }
        SPLIT_STAGE("probe");
        if (est > 1.02 * hs[k - 1] + 1.0e-13 * theta_nrm) {
          if (getenv("MPSK_SVD_DEBUG"))
            fprintf(stderr, "[mpsk_tsplit] dominance probe: |D x| = %.6e above S[k-1] = %.6e -> full iteration\n", est, hs[k - 1]);
          c->last_split_path = 2;
          continue;
        }
      }
    }
    SPLIT_STAGE("before LQpos / QRpos");
    if (!transposed) {
      if (int rc = lqpos_f64(c, k, n, T, k, Cm, ldc, AR, ldar)) return rc;
    } else {
      if (int rc = qrpos_f64(c, m, k, T, m, AL, ldal, Cm, ldc)) return rc;
      HIPCHK(transpose(Vk, n, n, k, (double*)AR, ldar, c->stream));
    }
    SPLIT_STAGE("done");
    return MPSK_OK;
  }
  return fail(MPSK_ERR_HIP, "mpsk_tsplit: internal error (no path finished)");
#undef SPLIT_STAGE
}

// Front end of the fp64 split: every factorization inside squares the scale of theta (Gram matrices), so tensors whose norm
// is outside [1e-100, 1e100] are split as theta / |theta|_F and the values scaled back (the split is homogeneous of degree
// one: AL, AR unchanged, C, S, the discarded norm and trunc_err scale); theta = 0 gets the trivial answer (C = 0, any
// isometries) instead of a factorization of nothing.
static int tsplit_f64(mpsk_ctx* c, int m, int n, const void* theta, int ldt, int max_keep, double trunc_err,
                      void* AL, int ldal, void* Cm, int ldc, void* AR, int ldar, void* S, int* kept, double* disc_norm) {
  REQUIRE(c && theta && AL && Cm && AR && S && kept && disc_norm, "NULL argument");
  REQUIRE(m > 0 && n > 0 && ldt >= m, "dimensions must be positive");
  HIPCHK(hipSetDevice(c->device));
  // scale = max |theta_ij| (a norm would square the entries: 1e-200 underflows there already)
  double nrm = 1.0;
  {
    unsigned long long* d_mx = (unsigned long long*)c->d_partial;
    unsigned long long h_mx = 0;
    HIPCHK(hipMemsetAsync(d_mx, 0, sizeof(unsigned long long), c->stream));
    hipLaunchKernelGGL(split_absmax_kernel, dim3(1024), dim3(256), 0, c->stream, (const double*)theta, (int64_t)ldt, m, n, d_mx);
    HIPCHK(hipMemcpyAsync(&h_mx, d_mx, sizeof(h_mx), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::memcpy(&nrm, &h_mx, sizeof(double));
  }
  const int kfull = m < n ? m : n;
  if (nrm == 0.0) {
    const int k = (max_keep > 0 && max_keep < kfull) ? max_keep : kfull;
    REQUIRE(ldal >= m && ldc >= k && ldar >= k, "leading dimension too small");
    hipLaunchKernelGGL(split_scale_copy_kernel, dim3(256), dim3(256), 0, c->stream, (const double*)nullptr, (int64_t)0, m, k, 0.0, (double*)AL, (int64_t)ldal);
    hipLaunchKernelGGL(split_scale_copy_kernel, dim3(256), dim3(256), 0, c->stream, (const double*)nullptr, (int64_t)0, k, n, 0.0, (double*)AR, (int64_t)ldar);
    HIPCHK(hipMemset2DAsync(Cm, sizeof(double) * ldc, 0, sizeof(double) * k, k, c->stream));
    HIPCHK(hipMemsetAsync(S, 0, sizeof(double) * kfull, c->stream));
    *kept = k; *disc_norm = 0.0;
    c->last_split_path = 0; c->last_split_iters = 0; c->last_split_resid = 0.0; c->last_svd_sweeps = 0;
    return MPSK_OK;
  }
  if (std::isfinite(nrm) && (nrm < 1.0e-100 || nrm > 1.0e100)) {
    double* Ts = nullptr;
    if (int rc = cx_scratch(c, 3, sizeof(double) * (size_t)m * n, &Ts)) return rc;
    hipLaunchKernelGGL(split_scale_copy_kernel, dim3(1024), dim3(256), 0, c->stream, (const double*)theta, (int64_t)ldt, m, n, 1.0 / nrm, Ts, (int64_t)m);
    if (int rc = tsplit_core(c, m, n, Ts, m, max_keep, trunc_err / nrm, AL, ldal, Cm, ldc, AR, ldar, S, kept, disc_norm)) return rc;
    const int k = *kept;
    hipLaunchKernelGGL(split_scale_copy_kernel, dim3(256), dim3(256), 0, c->stream, (const double*)Cm, (int64_t)ldc, k, k, nrm, (double*)Cm, (int64_t)ldc);
    HIPCHK(vec_scal(nrm, (double*)S, kfull, c->stream));
    *disc_norm *= nrm;
    return MPSK_OK;
  }
  return tsplit_core(c, m, n, theta, ldt, max_keep, trunc_err, AL, ldal, Cm, ldc, AR, ldar, S, kept, disc_norm);
}

// ---- complex128 two-site split (ctx dtype MPSK_C128) -------------------------------------------------------------------
// trunc_err > 0: the native complex SVD chooses k (the smaller of the max_keep and truncerr results, every complex value
// counted once), AL = U[:, :k], M = AL^H theta and (C, AR) = LQpos(M): the contract of the truncdim path.  S receives all
// min(m, n) values.  U / Vh / M live in complex scratch 2; the SVD, the GEMM and the LQpos use c->ws and scratches 0 / 1.
static int tsplit_c128_truncerr(mpsk_ctx* c, int m, int n, const void* theta, int ldt, int max_keep, double trunc_err,
                                void* AL, int ldal, void* Cm, int ldc, void* AR, int ldar, void* S, int* kept, double* disc_norm) {
  REQUIRE(ldt >= m, "leading dimension too small");
  HIPCHK(hipSetDevice(c->device));
  const int kfull = m < n ? m : n;
  const size_t u_d = 2 * ev2((size_t)m * kfull), v_d = 2 * ev2((size_t)kfull * n), s_d = ev2((size_t)kfull);
  double* buf = nullptr;
  if (int rc = cx_scratch(c, 2, sizeof(double) * (u_d + 2 * v_d + s_d), &buf)) return rc;
  double *Ub = buf, *Vb = Ub + u_d, *Mh = Vb + v_d, *Sb = Mh + v_d;
  int k = 0;
  double dn = 0.0;
  if (int rc = tsvd_c128_entry(c, m, n, theta, ldt, Ub, m, Sb, Vb, kfull, max_keep, trunc_err, &k, &dn)) return rc;
  REQUIRE(ldal >= m && ldc >= k && ldar >= k, "leading dimension too small");
  HIPCHK(hipMemcpy2DAsync(AL, sizeof(double) * 2 * ldal, Ub, sizeof(double) * 2 * m, sizeof(double) * 2 * m, k,
                          hipMemcpyDeviceToDevice, c->stream));
  if (int rc = gemm_c128(c, 1, 0, k, n, m, 1.0, Ub, m, theta, ldt, 0.0, Mh, k)) return rc;
  if (int rc = lqpos_c128(c, k, n, Mh, k, Cm, ldc, AR, ldar)) return rc;
  HIPCHK(hipMemcpyAsync(S, Sb, sizeof(double) * kfull, hipMemcpyDeviceToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  *kept = k;
  *disc_norm = dn;
  return MPSK_OK;
}

// theta (m x n complex, interleaved) ~ AL (m x k) C (k x k) AR (k x n), all complex, AL / AR isometries, C lower triangular
// with a real positive diagonal, S the k kept COMPLEX singular values.  Runs on the real embedding E (2m x 2n), whose
// singular values are those of theta, each twice: the real split of E returns an arbitrary basis inside every doubled
// value, so what is taken from it is the kept SUBSPACE (2k + 16 leading left vectors through the truncation-aware
// real split), made an embedding again by projecting structured random vectors on it -- the construction of
// cplx.split_two_site (mpskit.jl_amd/cplx.py), including a J-invariant choice inside a cluster that straddles the cut.
// This path truncates by max_keep only (truncdim); trunc_err > 0 takes tsplit_c128_truncerr instead.
static int tsplit_c128(mpsk_ctx* c, int m, int n, const void* theta, int ldt, int max_keep, double trunc_err,
                       void* AL, int ldal, void* Cm, int ldc, void* AR, int ldar, void* S, int* kept, double* disc_norm) {
  REQUIRE(c && theta && AL && Cm && AR && S && kept && disc_norm, "NULL argument");
  REQUIRE(m > 0 && n > 0, "dimensions must be positive");
  if (trunc_err > 0.0)
    return tsplit_c128_truncerr(c, m, n, theta, ldt, max_keep, trunc_err, AL, ldal, Cm, ldc, AR, ldar, S, kept, disc_norm);
  REQUIRE(trunc_err == 0.0, "complex mpsk_tsplit truncates by max_keep only (trunc_err must be 0)");
  const int kfull = m < n ? m : n;
  const int k = (max_keep > 0 && max_keep < kfull) ? max_keep : kfull;
  REQUIRE(ldt >= m && ldal >= m && ldc >= k && ldar >= k, "leading dimension too small");
  HIPCHK(hipSetDevice(c->device));
  const int m2 = 2 * m, n2 = 2 * n, kE = 2 * kfull, K2 = 2 * k;
  const size_t e_d = ev2((size_t)m2 * n2), al_d = ev2((size_t)m2 * kE), c_d = ev2((size_t)kE * kE), ar_d = ev2((size_t)kE * n2);
  const size_t b_d = ev2((size_t)m2 * K2), x_d = ev2((size_t)m2 * K2), g_d = ev2((size_t)kE * K2), me_d = ev2((size_t)K2 * n2);
  const size_t mh_d = ev2((size_t)2 * k * n), r_d = ev2((size_t)K2 * K2);
  double* buf = nullptr;
  if (int rc = cx_scratch(c, 2, sizeof(double) * (e_d + al_d + c_d + ar_d + ev2((size_t)kE) + 2 * b_d + 2 * x_d + g_d + me_d + mh_d + r_d), &buf))
    return rc;
  double *E = buf, *ALe = E + e_d, *Ce = ALe + al_d, *ARe = Ce + c_d, *Se = ARe + ar_d, *B = Se + ev2((size_t)kE), *W = B + b_d;
  double *Xh = W + b_d, *Xe = Xh + x_d, *G = Xe + x_d, *Me = G + g_d, *Mh = Me + me_d, *Rs = Mh + mh_d;
  hipLaunchKernelGGL(cx_embed_kernel, dim3(1024), dim3(256), 0, c->stream, (const double*)theta, (int64_t)2 * ldt, m, n, E, (int64_t)m2);
  std::vector<double> hs;
  int lo = K2, hi = K2, have = 0;
  for (int pad = 16;; pad *= 4) {
    int req = K2 + pad;
    if (req > kE) req = kE;
    int kk = 0;
    double dn = 0.0;
    if (kE > 64) {
      if (int rc = tsplit_f64(c, m2, n2, E, m2, req, 0.0, ALe, m2, Ce, kE, ARe, kE, Se, &kk, &dn)) return rc;
    } else {        // small tensors: the full decomposition (mpsk_tsvd has no size floor); only its left vectors are used
      if (int rc = tsvd_f64(c, m2, n2, E, m2, ALe, m2, Se, ARe, kE, req, 0.0, &kk, &dn)) return rc;
    }
    have = kk;
    hs.resize(have);
    HIPCHK(hipMemcpyAsync(hs.data(), Se, sizeof(double) * have, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    // [lo, hi): the even-aligned run of singular values equal to hs[K2 - 1] to 1e-8 -- the cluster the cut may split
    const double sk = hs[K2 - 1], tolc = 1.0e-8 * sk + 1.0e-14 * hs[0];
    lo = K2; while (lo > 0 && std::fabs(hs[lo - 1] - sk) <= tolc) --lo;
    hi = K2; while (hi < have && std::fabs(hs[hi] - sk) <= tolc) ++hi;
    lo -= lo & 1; hi += hi & 1;
    if (hi > have) hi = have;
    if (hi < have || have >= kE || pad > 4096) break;     // the cluster ends inside what was computed (or nothing is left)
  }
  // B: orthonormal basis of the kept, J-invariant subspace
  if (hi == K2) {
    HIPCHK(hipMemcpy2DAsync(B, sizeof(double) * m2, ALe, sizeof(double) * m2, sizeof(double) * m2, K2, hipMemcpyDeviceToDevice, c->stream));
  } else {
    if (lo > 0) HIPCHK(hipMemcpy2DAsync(B, sizeof(double) * m2, ALe, sizeof(double) * m2, sizeof(double) * m2, lo, hipMemcpyDeviceToDevice, c->stream));
    const int r2 = K2 - lo, nc = hi - lo;
    const double* Uc = ALe + (size_t)m2 * lo;
    hipLaunchKernelGGL(split_fill_kernel, dim3(1024), dim3(256), 0, c->stream, Xh, (int64_t)m2 * (r2 / 2), 0xc1u);
    hipLaunchKernelGGL(cx_embed_kernel, dim3(1024), dim3(256), 0, c->stream, Xh, (int64_t)m2, m, r2 / 2, Xe, (int64_t)m2);
    GemmArgs g1 = mk(Uc, Xe, G, nc, r2, m2, m2, m2, nc, 1, 0);            // Uc^T Xc
    HIPCHK(gemm_f64(g1, c->stream));
    GemmArgs g2 = mk(Uc, G, W, m2, r2, nc, m2, nc, m2);                   // Uc (Uc^T Xc)
    HIPCHK(gemm_f64(g2, c->stream));
    if (int rc = qrpos_f64(c, m2, r2, W, m2, B + (size_t)m2 * lo, m2, Rs, r2)) return rc;
  }
  // embedded orthonormal basis of that subspace: structured random vectors projected on it, QRpos
  hipLaunchKernelGGL(split_fill_kernel, dim3(1024), dim3(256), 0, c->stream, Xh, (int64_t)m2 * k, 0xc2u);
  hipLaunchKernelGGL(cx_embed_kernel, dim3(1024), dim3(256), 0, c->stream, Xh, (int64_t)m2, m, k, Xe, (int64_t)m2);
  GemmArgs g3 = mk(B, Xe, G, K2, K2, m2, m2, m2, K2, 1, 0);
  HIPCHK(gemm_f64(g3, c->stream));
  GemmArgs g4 = mk(B, G, W, m2, K2, K2, m2, K2, m2);
  HIPCHK(gemm_f64(g4, c->stream));
  if (int rc = qrpos_f64(c, m2, K2, W, m2, B, m2, Rs, K2)) return rc;          // B <- al_E (embedded, m2 x K2)
  hipLaunchKernelGGL(cx_half_kernel, dim3(1024), dim3(256), 0, c->stream, B, (int64_t)m2, m, k, (double*)AL, (int64_t)2 * ldal,
                     (double*)nullptr, (int64_t)0, 0);
  // M = AL^H theta (k x n complex) through the embedded product, then C AR = LQpos(M)
  GemmArgs g5 = mk(B, E, Me, K2, n2, m2, m2, m2, K2, 1, 0);
  HIPCHK(gemm_f64(g5, c->stream));
  hipLaunchKernelGGL(cx_half_kernel, dim3(1024), dim3(256), 0, c->stream, Me, (int64_t)K2, k, n, Mh, (int64_t)2 * k,
                     (double*)nullptr, (int64_t)0, 0);
  double tn = 0.0, mn = 0.0;
  if (int rc = mpsk_vnrm2(c, (int64_t)m2 * n2, E, &tn)) return rc;           // |E|^2 = 2 |theta|^2
  if (int rc = mpsk_vnrm2(c, (int64_t)2 * k * n, Mh, &mn)) return rc;
  if (int rc = lqpos_c128(c, k, n, Mh, k, Cm, ldc, AR, ldar)) return rc;
  std::vector<double> sc(kfull, std::nan(""));
  for (int j = 0; j < k; ++j) sc[j] = hs[2 * j];
  HIPCHK(hipMemcpyAsync(S, sc.data(), sizeof(double) * kfull, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));                                    // sc is a host temporary
  *kept = k;
  *disc_norm = std::sqrt(std::max(0.5 * tn * tn - mn * mn, 0.0));
  return MPSK_OK;
}

// conversions between an interleaved complex matrix (m x n complex = 2m x n doubles, ldh in DOUBLES) and its real embedding
// (2m x 2n doubles): one launch each.  mpsk_cx_half returns the STRUCTURED PART of a nearly embedded matrix
// (re = (E00 + E11) / 2, im = (E10 - E01) / 2 on every 2 x 2 block), which is the complex matrix whose embedding is closest.
int mpsk_cx_embed(mpsk_ctx* c, int m, int n, const void* H, int64_t ldh, void* E, int64_t lde) {
  REQUIRE(c && H && E, "NULL argument");
  REQUIRE(m > 0 && n > 0 && ldh >= 2 * (int64_t)m && lde >= 2 * (int64_t)m, "bad dimensions");
  HIPCHK(hipSetDevice(c->device));
  hipLaunchKernelGGL(cx_embed_kernel, dim3(1024), dim3(256), 0, c->stream, (const double*)H, ldh, m, n, (double*)E, lde);
  return MPSK_OK;
}
int mpsk_cx_half(mpsk_ctx* c, int m, int n, const void* E, int64_t lde, void* H, int64_t ldh) {
  REQUIRE(c && H && E, "NULL argument");
  REQUIRE(m > 0 && n > 0 && ldh >= 2 * (int64_t)m && lde >= 2 * (int64_t)m, "bad dimensions");
  HIPCHK(hipSetDevice(c->device));
  hipLaunchKernelGGL(cx_half_kernel, dim3(1024), dim3(256), 0, c->stream, (const double*)E, lde, m, n, (double*)H, ldh,
                     (double*)nullptr, (int64_t)0, 0);
  return MPSK_OK;
}

// the ABI entry: fp64, or complex128 when the ctx dtype says so (mpsk_ctx_set_dtype)
int mpsk_tsplit(mpsk_ctx* c, int m, int n, const void* theta, int ldt, int max_keep, double trunc_err,
                void* AL, int ldal, void* Cm, int ldc, void* AR, int ldar, void* S, int* kept, double* disc_norm) {
  REQUIRE(c, "ctx is NULL");
  return c->dtype == MPSK_C128 ? tsplit_c128(c, m, n, theta, ldt, max_keep, trunc_err, AL, ldal, Cm, ldc, AR, ldar, S, kept, disc_norm)
                               : tsplit_f64(c, m, n, theta, ldt, max_keep, trunc_err, AL, ldal, Cm, ldc, AR, ldar, S, kept, disc_norm);
}

int mpsk_ctx_set_svd_mode(mpsk_ctx* c, int precondition) {
  REQUIRE(c, "ctx is NULL");
  REQUIRE(precondition >= 0 && precondition <= 3, "svd mode must be 0 (none), 1 (QR), 2 (QR + QR of R^T), 3 (2 + truncation-aware mpsk_tsplit)");
  c->svd_precondition = precondition;
  return MPSK_OK;
}
int mpsk_ctx_svd_stats(mpsk_ctx* c, int* last_sweeps) {
  REQUIRE(c && last_sweeps, "NULL argument");
  *last_sweeps = c->last_svd_sweeps;
  return MPSK_OK;
}
int mpsk_ctx_split_stats(mpsk_ctx* c, int* path, int* iterations, double* residual) {
  REQUIRE(c, "ctx is NULL");
  if (path) *path = c->last_split_path;
  if (iterations) *iterations = c->last_split_iters;
  if (residual) *residual = c->last_split_resid;
  return MPSK_OK;
}

// ---- complex128 complement SVD (ctx dtype MPSK_C128) -------------------------------------------------------------------
// The k leading singular triplets of X = (1 - QL QL^H) Y (1 - QR^H QR) on interleaved complex operands (leading dimensions
// in complex elements, S real).  Every product is gemm_c128 with X -- or its conjugate transpose XH, kept beside it -- as
// the SECOND operand: that operand is read as stored, and only the thin first operand (QL, QR, a block of r rows) is
// embedded, so no 2m x 2n real copy of X or Y ever exists and a product of a p-row block with X costs 8 p m n real flops, the
// complex optimum (the two-K-segment form of dAC_c128 has the same count and needs the planes of its second operand, i.e. a
// planar copy of X per product; gemm_c128 needs nothing but the thin embedding).
//   projection   X <- X - QL (QL^H X);  XH = X^H;  XH <- XH - QR^H (QR XH);  X = XH^H       four thin products, 16 (pl + pr) m n
//   min(m, n) <= 64: tsvd_c128_entry on X.
//   otherwise, in svd mode 3 and not while the ctx backs off: a truncated range finder on r = min(k + max(64, k / 2), m - pl,
//   n - pr) rows (rank(X) cannot exceed the dimension of the complement, so more rows add nothing and the fp64 cap of 5/8 of
//   the matrix does not apply):  W (r x n) structured random;  CX_RANGE_ITERS times  Z = W XH, Z <- rows of LQpos(Z),
//   B = Z X, W <- rows of LQpos(B)  (2 CX_RANGE_ITERS products of 8 r m n flops, lqpos_c128 in between; the last LQpos is
//   not taken);  B = Z X = U_B S V_B (tsvd_c128_entry, r x n);  U = Z^H U_B, Vt = V_B.
//   the check, not an estimate: U^H X = S Vt holds by construction, so the triplets are singular triplets of X exactly when
//   X Vt^H = U S, and X Vt^H - U S = (1 - Z^H Z) X Vt^H:  rho = |(Vt XH)(1 - Z^H Z)|_F / |X|_F <= 1e-12 (MPSK_SPLIT_TOL) and
//   |U|_F^2 = kept (a collapsed basis has rho = 0 too) -> accepted, counted under n_subspace.  Otherwise, and in every other
//   case above 64, tsvd_c128_entry on X itself (n_full); a failed check makes the ctx back off as the fp64 split does.
// Singular values at or below 32 eps sqrt(m + n) max|Y_ij| -- the rounding level of the projection -- are returned as
// exactly 0 (X = 0, rank(X) < kept, Y inside the range of QL): their directions are completed inside the complement.
// Then, as in the fp64 entry, two rounds of projection and QRpos / LQpos impose the complement condition and the isometry.
static const int CX_RANGE_ITERS = 4;

static int cx_copy2d(mpsk_ctx* c, void* dst, int lddst, const void* src, int ldsrc, int rows, int cols) {
  HIPCHK(hipMemcpy2DAsync(dst, sizeof(double) * 2 * lddst, src, sizeof(double) * 2 * ldsrc, sizeof(double) * 2 * rows, cols,
                          hipMemcpyDeviceToDevice, c->stream));
  return MPSK_OK;
}
static int cx_absmax(mpsk_ctx* c, const double* A, int64_t ld_doubles, int rows_doubles, int cols, double* out) {
  unsigned long long* d_mx = (unsigned long long*)c->d_partial;
  unsigned long long h_mx = 0;
  HIPCHK(hipMemsetAsync(d_mx, 0, sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(split_absmax_kernel, dim3(1024), dim3(256), 0, c->stream, A, ld_doubles, rows_doubles, cols, d_mx);
  HIPCHK(hipMemcpyAsync(&h_mx, d_mx, sizeof(h_mx), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  std::memcpy(out, &h_mx, sizeof(double));
  return MPSK_OK;
}

// (arguments checked by mpsk_complement_tsvd; kk = the number of triplets to deliver, > 0)
static int complement_tsvd_c128(mpsk_ctx* c, int m, int n, const void* Y, int ldy, const void* QL, int ldql, int pl,
                                const void* QR, int ldqr, int pr, int kk, void* U, int ldu, void* S, void* Vt, int ldvt) {
  static const double sub_tol = getenv("MPSK_SPLIT_TOL") ? atof(getenv("MPSK_SPLIT_TOL")) : 1.0e-12;
  const int nn = std::min(m, n), mx_dim = std::max(m, n);
  const bool small = nn <= 64;
  int r = 0;                                            // rows of the range finder (0: not taken)
  if (!small) {
    if (c->split_skip > 0) --c->split_skip;             // (backing off after a failed check)
    else if (c->svd_precondition == 3) r = std::min(kk + std::max(64, kk / 2), std::min(m - pl, n - pr));
  }
  // scratch, in doubles (every part an even count: 16-byte aligned complex elements)
  const size_t x_d = (size_t)2 * m * n, bf_d = (size_t)2 * nn * n, s_d = ev2((size_t)nn);
  const size_t tp_d = 2 * std::max(std::max((size_t)pl * n, (size_t)pr * m), std::max(std::max((size_t)pl * kk, (size_t)kk * pr), (size_t)1));
  const size_t g_d = (size_t)2 * r * mx_dim, l_d = (size_t)2 * r * r, vb_d = (size_t)2 * r * n, sb_d = ev2((size_t)r);
  const size_t th_d = (size_t)2 * kk * m, p1_d = (size_t)2 * kk * r;
  const size_t ut_d = (size_t)2 * m * kk, vtt_d = (size_t)2 * kk * n, rt_d = (size_t)2 * kk * kk;
  double* base = nullptr;
  if (int rc = ex_scratch(c, sizeof(double) * (2 * x_d + bf_d + s_d + tp_d + 3 * g_d + 2 * l_d + vb_d + sb_d + th_d + p1_d + ut_d +
                                                vtt_d + rt_d), &base))
    return rc;
  double* X = base;                  // m x n
  double* XH = X + x_d;              // n x m = X^H; U of the full SVD once the range finder is over (m x nn)
  double* Bf = XH + x_d;             // Vh of the full SVD (nn x n)
  double* Ss = Bf + bf_d;
  double* TP = Ss + s_d;
  double* GW = TP + tp_d;            // r x n   right block W
  double* GZ = GW + g_d;             // r x m   left block Z (orthonormal rows)
  double* GT = GZ + g_d;             // product before its LQpos; B = Z X at the end
  double* Lr = GT + g_d;             // triangular factors (discarded)
  double* UB = Lr + l_d;             // r x r
  double* VB = UB + l_d;             // r x n
  double* SB = VB + vb_d;
  double* Th = SB + sb_d;            // kk x m
  double* P1 = Th + th_d;            // kk x r
  double* Ut = P1 + p1_d;            // QRpos output
  double* Vtt = Ut + ut_d;           // LQpos output
  double* Rt = Vtt + vtt_d;
  hipStream_t st = c->stream;
  ++c->n_compl;
  c->last_split_iters = 0; c->last_split_resid = 0.0; c->last_split_path = 0;
  double my = 0.0, mx = 0.0;
  if (int rc = cx_absmax(c, (const double*)Y, (int64_t)2 * ldy, 2 * m, n, &my)) return rc;
  if (!std::isfinite(my)) return fail(MPSK_ERR_INVALID, "mpsk_complement_tsvd: Y is not finite");
  const double thr = 32.0 * 2.220446049250313e-16 * std::sqrt((double)m + (double)n) * my;
  int have = 0;                      // triplets delivered by the SVD; the rest is completed below
  if (my > 0.0) {
    // X = (1 - QL QL^H) Y (1 - QR^H QR)
    if (int rc = cx_copy2d(c, X, m, Y, ldy, m, n)) return rc;
    if (pl > 0) {
      if (int rc = gemm_c128(c, 1, 0, pl, n, m, 1.0, QL, ldql, X, m, 0.0, TP, pl)) return rc;
      if (int rc = gemm_c128(c, 0, 0, m, n, pl, -1.0, QL, ldql, TP, pl, 1.0, X, m)) return rc;
    }
    hipLaunchKernelGGL(cx_ctranspose_kernel, dim3(1024), dim3(256), 0, st, X, (int64_t)2 * m, m, n, XH, (int64_t)2 * n);
    if (pr > 0) {
      if (int rc = gemm_c128(c, 0, 0, pr, m, n, 1.0, QR, ldqr, XH, n, 0.0, TP, pr)) return rc;
      if (int rc = gemm_c128(c, 1, 0, n, m, pr, -1.0, QR, ldqr, TP, pr, 1.0, XH, n)) return rc;
      hipLaunchKernelGGL(cx_ctranspose_kernel, dim3(1024), dim3(256), 0, st, XH, (int64_t)2 * n, n, m, X, (int64_t)2 * m);
    }
    if (int rc = cx_absmax(c, X, (int64_t)2 * m, 2 * m, n, &mx)) return rc;
    if (!std::isfinite(mx)) return fail(MPSK_ERR_INVALID, "mpsk_complement_tsvd: Y is not finite");
  }
  const double* Usrc = nullptr; const double* Vsrc = nullptr; const double* Ssrc = nullptr;
  int ldus = 0, ldvs = 0, ns = 0;    // where the accepted SVD left its factors, and how many values it has
  bool done = false;
  if (!(mx > thr)) {
    ++c->n_compl_full;               // X = 0 to the rounding level of the projection: nothing to decompose
    done = true;
  } else if (r > 0) {
    // the range finder; a factorization that refuses its input sends the call to the full SVD like a failed check
    bool ok = true;
    double xn = 0.0, rho = INFINITY;
    if (int rc = mpsk_vnrm2(c, (int64_t)2 * m * n, X, &xn)) return rc;
    hipLaunchKernelGGL(split_fill_kernel, dim3(1024), dim3(256), 0, st, GW, (int64_t)2 * r * n, 0x5eedu);
    for (int it = 0; it < CX_RANGE_ITERS && ok; ++it) {
      if (int rc = gemm_c128(c, 0, 0, r, m, n, 1.0, GW, r, XH, n, 0.0, GT, r)) return rc;       // Z = W XH
      if (int rc = lqpos_c128(c, r, m, GT, r, Lr, r, GZ, r)) { if (rc != MPSK_ERR_INVALID) return rc; ok = false; break; }
      if (int rc = gemm_c128(c, 0, 0, r, n, m, 1.0, GZ, r, X, m, 0.0, GT, r)) return rc;        // B = Z X
      if (it + 1 < CX_RANGE_ITERS)
        if (int rc = lqpos_c128(c, r, n, GT, r, Lr, r, GW, r)) { if (rc != MPSK_ERR_INVALID) return rc; ok = false; }
    }
    int kb = 0; double dn = 0.0;
    if (ok) {
      if (int rc = tsvd_c128_entry(c, r, n, GT, r, UB, r, SB, VB, r, 0, 0.0, &kb, &dn)) { if (rc != MPSK_ERR_INVALID) return rc; ok = false; }
    }
    if (ok) {
      const int kc = std::min(kk, kb);
      // Th = Vt XH (= (X Vt^H)^H, kc x m);  Th <- Th - (Th Z^H) Z;  rho = |Th| / |X|
      if (int rc = gemm_c128(c, 0, 0, kc, m, n, 1.0, VB, r, XH, n, 0.0, Th, kc)) return rc;
      if (int rc = gemm_c128(c, 0, 1, kc, r, m, 1.0, Th, kc, GZ, r, 0.0, P1, kc)) return rc;
      if (int rc = gemm_c128(c, 0, 0, kc, m, r, -1.0, P1, kc, GZ, r, 1.0, Th, kc)) return rc;
      if (int rc = mpsk_vnrm2(c, (int64_t)2 * kc * m, Th, &rho)) return rc;
      rho = xn > 0.0 ? rho / xn : rho;
      // U = Z^H U_B into Ut (m x kc): nothing is written to the caller's buffers before the check has passed
      if (int rc = gemm_c128(c, 1, 0, m, kc, r, 1.0, GZ, r, UB, r, 0.0, Ut, m)) return rc;
      double un = 0.0;
      if (int rc = mpsk_vnrm2(c, (int64_t)2 * m * kc, Ut, &un)) return rc;
      if (!(std::fabs(un * un - (double)kc) <= 1.0e-8 * kc)) rho = INFINITY;
      c->last_split_iters = CX_RANGE_ITERS; c->last_split_resid = rho;
      if (getenv("MPSK_SVD_DEBUG"))
        fprintf(stderr, "[mpsk_complement_tsvd C128] range finder: r = %d of %d x %d, %d iterations, residual %.3e (tol %.1e)\n",
                r, m, n, CX_RANGE_ITERS, rho, sub_tol);
      if (rho <= sub_tol) {
        ++c->n_compl_sub;
        c->last_split_path = 1; c->split_backoff = 0;
        Usrc = Ut; ldus = m; Vsrc = VB; ldvs = r; Ssrc = SB; ns = kc;
        done = true;
      }
    }
    if (!done) {                     // flat spectra come in runs: the next calls skip the range finder, 4, 8, ... 64 of them
      c->last_split_path = 2;
      c->split_backoff = c->split_backoff ? std::min(2 * c->split_backoff, 64) : 4;
      c->split_skip = c->split_backoff;
    }
  }
  if (!done) {                       // small X, svd mode below 3, backing off, failed check: the full SVD of X
    int kf = 0; double dn = 0.0;
    double* Af = XH;                 // (X^H is no longer needed; m x nn fits in n x m)
    if (int rc = tsvd_c128_entry(c, m, n, X, m, Af, m, Ss, Bf, nn, 0, 0.0, &kf, &dn)) return rc;
    ++c->n_compl_full;
    Usrc = Af; ldus = m; Vsrc = Bf; ldvs = nn; Ssrc = Ss; ns = std::min(kk, kf);
  }
  if (ns > 0) {                      // values above the rounding level of the projection count; S is descending
    std::vector<double> hs((size_t)ns);
    HIPCHK(hipMemcpyAsync(hs.data(), Ssrc, sizeof(double) * ns, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    while (have < ns && hs[have] > thr) ++have;
  }
  if (have > 0) {
    if (int rc = cx_copy2d(c, U, ldu, Usrc, ldus, m, have)) return rc;
    if (int rc = cx_copy2d(c, Vt, ldvt, Vsrc, ldvs, have, n)) return rc;
    HIPCHK(hipMemcpyAsync(S, Ssrc, sizeof(double) * have, hipMemcpyDeviceToDevice, st));
  }
  if (have < kk) {                   // directions the SVD did not deliver: random, singular value 0
    const int rr = kk - have;
    hipLaunchKernelGGL(split_fill_kernel, dim3(256), dim3(256), 0, st, Vtt, (int64_t)2 * rr * n, 0xfeedu);
    if (int rc = cx_copy2d(c, (double*)Vt + (size_t)2 * have, ldvt, Vtt, rr, rr, n)) return rc;
    hipLaunchKernelGGL(split_fill_kernel, dim3(256), dim3(256), 0, st, Ut, (int64_t)2 * m * rr, 0x5eedu);    // (Ut is copied out by now)
    if (int rc = cx_copy2d(c, (double*)U + (size_t)2 * have * ldu, ldu, Ut, m, m, rr)) return rc;
    HIPCHK(hipMemsetAsync((double*)S + have, 0, sizeof(double) * rr, st));
  }
  // the complement condition and the isometry, by construction
  for (int round = 0; round < 2; ++round) {
    if (pl > 0) {
      if (int rc = gemm_c128(c, 1, 0, pl, kk, m, 1.0, QL, ldql, U, ldu, 0.0, TP, pl)) return rc;
      if (int rc = gemm_c128(c, 0, 0, m, kk, pl, -1.0, QL, ldql, TP, pl, 1.0, U, ldu)) return rc;
    }
    if (int rc = qrpos_c128(c, m, kk, U, ldu, Ut, m, Rt, kk)) return rc;
    if (int rc = cx_copy2d(c, U, ldu, Ut, m, m, kk)) return rc;
    if (pr > 0) {
      if (int rc = gemm_c128(c, 0, 1, kk, pr, n, 1.0, Vt, ldvt, QR, ldqr, 0.0, TP, kk)) return rc;
      if (int rc = gemm_c128(c, 0, 0, kk, n, pr, -1.0, TP, kk, QR, ldqr, 1.0, Vt, ldvt)) return rc;
    }
    if (int rc = lqpos_c128(c, kk, n, Vt, ldvt, Rt, kk, Vtt, kk)) return rc;
    if (int rc = cx_copy2d(c, Vt, ldvt, Vtt, kk, kk, n)) return rc;
  }
  HIPCHK(hipStreamSynchronize(st));
  return MPSK_OK;
}

// mpsk_complement_tsvd: the k leading singular triplets of X = (1 - QL QL^T) Y (1 - QR^T QR) without null-space bases
// (NL NL' = 1 - AL AL', NR' NR = 1 - AR' AR in optimalexpand.jl:22-29).  X is formed with four thin GEMMs; the triplets come
// from the checked subspace iteration of the truncated split (tsplit_f64: X ~ A C B, kept subspace verified against X
// itself or the full iteration taken) followed by the small SVD C = Uc S Vc, U = A Uc, Vt = Vc B.  min(m, n) <= 64: the
// full SVD of X.  The complement condition is then imposed, not inherited: U <- QRpos((1 - QL QL^T) U), twice, and the
// same with LQpos from the right, which also completes directions the SVD left empty (X of rank < kept, X = 0).
int mpsk_complement_tsvd(mpsk_ctx* c, int m, int n, const void* Y, int ldy, const void* QL, int ldql, int pl, const void* QR,
                         int ldqr, int pr, int k, void* U, int ldu, void* S, void* Vt, int ldvt, int* kept) {
  REQUIRE(c && Y && kept, "NULL argument");
  REQUIRE(m > 0 && n > 0 && ldy >= m && k >= 0, "bad dimensions");
  REQUIRE(pl >= 0 && pl <= m && pr >= 0 && pr <= n, "pl / pr out of range");
  REQUIRE((pl == 0 || (QL && ldql >= m)) && (pr == 0 || (QR && ldqr >= pr)), "QL / QR missing or leading dimension too small");
  const int kk = std::min(k, std::min(m - pl, n - pr));
  *kept = kk;
  if (kk <= 0) { *kept = 0; return MPSK_OK; }
  REQUIRE(U && S && Vt && ldu >= m && ldvt >= kk, "U / S / Vt missing or leading dimension too small");
  REQUIRE(!c->pend.active && !c->on_side, "not accepted inside a side-stream section / with a deferred factorization pending");
  HIPCHK(hipSetDevice(c->device));
  if (c->dtype == MPSK_C128) return complement_tsvd_c128(c, m, n, Y, ldy, QL, ldql, pl, QR, ldqr, pr, kk, U, ldu, S, Vt, ldvt);
  const auto ev = [](size_t v) { return (v + 1) & ~(size_t)1; };
  const int nn = std::min(m, n);
  const bool small = nn <= 64;
  const int kf = small ? nn : kk;                       // columns of the factor buffers
  const size_t x_d = ev((size_t)m * n);
  const size_t tp_d = ev(std::max(std::max((size_t)pl * n, (size_t)m * pr), std::max((size_t)pl * kk, (size_t)kk * pr)) + 2);
  const size_t a_d = ev((size_t)m * kf), b_d = ev((size_t)kf * n), c_d = ev((size_t)kf * kf), s_d = ev((size_t)nn);
  double* base = nullptr;
  if (int rc = ex_scratch(c, sizeof(double) * (x_d + tp_d + 2 * a_d + 2 * b_d + 4 * c_d + 2 * s_d), &base)) return rc;
  double* X = base;
  double* TP = X + x_d;
  double* Af = TP + tp_d;            // left factor of the split / U of the small SVD
  double* Ut = Af + a_d;             // QRpos output
  double* Bf = Ut + a_d;             // right factor / Vt of the small SVD
  double* Vtt = Bf + b_d;            // LQpos output
  double* Cc = Vtt + b_d;            // core of the split
  double* Uc = Cc + c_d;
  double* Vc = Uc + c_d;
  double* Rt = Vc + c_d;             // triangular factors of the re-orthonormalisations (discarded)
  double* Ss = Rt + c_d;
  double* S2 = Ss + s_d;
  hipStream_t st = c->stream;
  ++c->n_compl;
  // X = (1 - QL QL^T) Y (1 - QR^T QR)
  HIPCHK(hipMemcpy2DAsync(X, sizeof(double) * m, Y, sizeof(double) * ldy, sizeof(double) * m, n, hipMemcpyDeviceToDevice, st));
  if (pl > 0) {
    GemmArgs g1 = mk((const double*)QL, X, TP, pl, n, m, ldql, m, pl, 1, 0);
    HIPCHK(gemm_f64(g1, st));
    GemmArgs g2 = mk((const double*)QL, TP, X, m, n, pl, ldql, pl, m);
    g2.alpha = -1.0; g2.beta = 1.0;
    HIPCHK(gemm_f64(g2, st));
  }
  if (pr > 0) {
    GemmArgs g1 = mk(X, (const double*)QR, TP, m, pr, n, m, ldqr, m, 0, 1);
    HIPCHK(gemm_f64(g1, st));
    GemmArgs g2 = mk(TP, (const double*)QR, X, m, n, pr, m, ldqr, m);
    g2.alpha = -1.0; g2.beta = 1.0;
    HIPCHK(gemm_f64(g2, st));
  }
  double mx = 0.0;
  {
    unsigned long long* d_mx = (unsigned long long*)c->d_partial;
    unsigned long long h_mx = 0;
    HIPCHK(hipMemsetAsync(d_mx, 0, sizeof(unsigned long long), st));
    hipLaunchKernelGGL(split_absmax_kernel, dim3(1024), dim3(256), 0, st, (const double*)X, (int64_t)m, m, n, d_mx);
    HIPCHK(hipMemcpyAsync(&h_mx, d_mx, sizeof(h_mx), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::memcpy(&mx, &h_mx, sizeof(double));
  }
  int have = 0;                      // triplets delivered by the SVD; the rest is completed below
  if (mx == 0.0 || !std::isfinite(mx)) {
    REQUIRE(mx == 0.0, "Y is not finite");
    ++c->n_compl_full;
  } else if (small) {
    int kf2 = 0; double dn = 0.0;
    if (int rc = tsvd_f64(c, m, n, X, m, Af, m, Ss, Bf, nn, 0, 0.0, &kf2, &dn)) return rc;
    have = std::min(kk, kf2);
    ++c->n_compl_full;
    HIPCHK(hipMemcpy2DAsync(U, sizeof(double) * ldu, Af, sizeof(double) * m, sizeof(double) * m, have, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpy2DAsync(Vt, sizeof(double) * ldvt, Bf, sizeof(double) * nn, sizeof(double) * have, n, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(S, Ss, sizeof(double) * have, hipMemcpyDeviceToDevice, st));
  } else {
    int ks = 0, k2 = 0; double dn = 0.0;
    if (int rc = tsplit_f64(c, m, n, X, m, kk, 0.0, Af, m, Cc, kk, Bf, kk, Ss, &ks, &dn)) return rc;
    if (c->last_split_path == 1) ++c->n_compl_sub; else ++c->n_compl_full;
    REQUIRE(ks >= 1 && ks <= kk, "split returned an unexpected rank");
    if (int rc = tsvd_f64(c, ks, ks, Cc, kk, Uc, ks, S2, Vc, ks, 0, 0.0, &k2, &dn)) return rc;
    have = std::min(ks, k2);
    GemmArgs gu = mk(Af, Uc, (double*)U, m, have, ks, m, ks, ldu);
    HIPCHK(gemm_f64(gu, st));
    GemmArgs gv = mk(Vc, Bf, (double*)Vt, have, n, ks, ks, kk, ldvt);
    HIPCHK(gemm_f64(gv, st));
    HIPCHK(hipMemcpyAsync(S, S2, sizeof(double) * have, hipMemcpyDeviceToDevice, st));
  }
  if (have < kk) {                   // directions the SVD did not deliver: random, singular value 0
    const int r = kk - have;
    hipLaunchKernelGGL(split_fill_kernel, dim3(256), dim3(256), 0, st, Ut, (int64_t)m * r, 0x5eedu);
    HIPCHK(hipMemcpy2DAsync((double*)U + (size_t)have * ldu, sizeof(double) * ldu, Ut, sizeof(double) * m, sizeof(double) * m, r,
                            hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(split_fill_kernel, dim3(256), dim3(256), 0, st, Vtt, (int64_t)r * n, 0xfeedu);
    HIPCHK(hipMemcpy2DAsync((double*)Vt + have, sizeof(double) * ldvt, Vtt, sizeof(double) * r, sizeof(double) * r, n,
                            hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemsetAsync((double*)S + have, 0, sizeof(double) * r, st));
  }
  // the complement condition and the isometry, by construction
  for (int round = 0; round < 2; ++round) {
    if (pl > 0) {
      GemmArgs g1 = mk((const double*)QL, (const double*)U, TP, pl, kk, m, ldql, ldu, pl, 1, 0);
      HIPCHK(gemm_f64(g1, st));
      GemmArgs g2 = mk((const double*)QL, TP, (double*)U, m, kk, pl, ldql, pl, ldu);
      g2.alpha = -1.0; g2.beta = 1.0;
      HIPCHK(gemm_f64(g2, st));
    }
    if (int rc = qrpos_f64(c, m, kk, U, ldu, Ut, m, Rt, kk)) return rc;
    HIPCHK(hipMemcpy2DAsync(U, sizeof(double) * ldu, Ut, sizeof(double) * m, sizeof(double) * m, kk, hipMemcpyDeviceToDevice, st));
    if (pr > 0) {
      GemmArgs g1 = mk((const double*)Vt, (const double*)QR, TP, kk, pr, n, ldvt, ldqr, kk, 0, 1);
      HIPCHK(gemm_f64(g1, st));
      GemmArgs g2 = mk(TP, (const double*)QR, (double*)Vt, kk, n, pr, kk, ldqr, ldvt);
      g2.alpha = -1.0; g2.beta = 1.0;
      HIPCHK(gemm_f64(g2, st));
    }
    if (int rc = lqpos_f64(c, kk, n, Vt, ldvt, Rt, kk, Vtt, kk)) return rc;
    HIPCHK(hipMemcpy2DAsync(Vt, sizeof(double) * ldvt, Vtt, sizeof(double) * kk, sizeof(double) * kk, n, hipMemcpyDeviceToDevice, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  return MPSK_OK;
}

int mpsk_ctx_complement_stats(mpsk_ctx* c, long* n_calls, long* n_subspace, long* n_full) {
  REQUIRE(c, "ctx is NULL");
  if (n_calls) *n_calls = c->n_compl;
  if (n_subspace) *n_subspace = c->n_compl_sub;
  if (n_full) *n_full = c->n_compl_full;
  return MPSK_OK;
}

}  // extern "C"
