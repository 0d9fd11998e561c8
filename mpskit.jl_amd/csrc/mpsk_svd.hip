// Truncated SVD for the two-site update (tsvd!(theta; trunc, alg = SVD()) at dmrg.jl:96,112 and
// tdvp.jl:124,140 of the reference): one-sided BLOCK JACOBI (Hestenes) on the MFMA GEMM core.
//
//   G <- theta (m x n, m >= n, columns padded to a multiple of 64), V <- I.
//   The n/32 column blocks are paired by a round-robin tournament.  Per round, for every pair p
//   (64 adjacent columns X_p of G):
//     1. Gram   M_p = X_p^T X_p             -- batched TN GEMM, K split over Q workgroups
//     2. eig    M_p = W_p L W_p^T           -- cyclic two-sided Jacobi in LDS, one workgroup / pair
//     3. update X_p <- X_p W_p, V_p <- V_p W_p, written straight to next round's slots
//        (ping-pong buffers; the tournament permutation is folded into the GEMM's C offsets)
//   until every off-diagonal Gram entry satisfies |g_ij| <= tol sqrt(g_ii g_jj).
//   Then sigma_j = ||G_j||, U = G diag(1/sigma), sorted descending on the host.
// Jacobi keeps high RELATIVE accuracy of small singular values (they decide truncerr/truncdim),
// which a Gram-matrix eigensolve of the whole theta would not.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <string>
#include <utility>
#include <vector>
#include "mpsk_internal.h"

namespace mpsk {

constexpr int JB = 32;
constexpr int J2 = 64;

typedef double sv_d4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ double sv_readlane(double v, int lane) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_readlane(lo, lane);
  hi = __builtin_amdgcn_readlane(hi, lane);
  return __hiloint2double(hi, lo);
}

// 1/sqrt(x) and sqrt(x) for a pivot on the serial critical path of the 64-step elimination: v_rsq_f64 seed (~2^-26)
// + two Newton steps (full fp64) instead of the IEEE sqrt + division sequences (~50 dependent instructions a pivot).
__device__ __forceinline__ void sv_piv_rsqrt(double x, double* rs_out, double* sq_out) {
  double r = __builtin_amdgcn_rsq(x);
  r = r * (1.5 - 0.5 * x * r * r);
  r = r * (1.5 - 0.5 * x * r * r);
  double s = x * r;
  s = s + 0.5 * r * (x - s * s);            // one correction: s = sqrt(x) to the last bit or two
  *rs_out = r;
  *sq_out = s;
}

__global__ __launch_bounds__(256) void jacobi_eig_kernel(const double* __restrict__ Mpart, int Q,
                                                         double* __restrict__ Wout, double tol,
                                                         unsigned long long* __restrict__ flag, int inner_sweeps) {
  __shared__ double Ms[J2][J2 + 1];
  __shared__ double Ws[J2][J2 + 1];
  __shared__ double red[4];
  __shared__ int any_rot;
  const int tid = threadIdx.x;
  const int p = blockIdx.x;
  const double* Mp = Mpart + (size_t)p * Q * J2 * J2;
  {
    double accv[16];                   // 16 independent running sums per thread: loads stay in flight
#pragma unroll
    for (int i = 0; i < 16; ++i) accv[i] = 0.0;
#pragma unroll 4
    for (int q = 0; q < Q; ++q) {
      const double* mq = Mp + (size_t)q * J2 * J2 + tid;
#pragma unroll
      for (int i = 0; i < 16; ++i) accv[i] += mq[256 * i];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int e = tid + 256 * i;
      Ms[e % J2][e / J2] = accv[i];    // Ms[i][j], column-major source
      Ws[e % J2][e / J2] = (e % J2 == e / J2) ? 1.0 : 0.0;
    }
  }
  __syncthreads();
  // symmetrise + convergence measure of this pair
  double mx = 0.0;
  for (int e = tid; e < J2 * J2; e += 256) {
    int i = e % J2, j = e / J2;
    if (i < j) {
      double a = 0.5 * (Ms[i][j] + Ms[j][i]);
      double dd = Ms[i][i] * Ms[j][j];
      double r = (a == 0.0) ? 0.0 : (dd > 0.0 ? fabs(a) / sqrt(dd) : 1.0);
      mx = fmax(mx, r);
    }
  }
  for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  if (tid == 0) atomicMax(flag, (unsigned long long)__double_as_longlong(mx));
  double* Wp = Wout + (size_t)p * J2 * J2;
  if (mx <= tol) {
    for (int e = tid; e < J2 * J2; e += 256) Wp[e] = (e % J2 == e / J2) ? 1.0 : 0.0;
    return;
  }
  __syncthreads();
  for (int e = tid; e < J2 * J2; e += 256) {
    int i = e % J2, j = e / J2;
    if (i < j) { double a = 0.5 * (Ms[i][j] + Ms[j][i]); Ms[i][j] = a; }
  }
  __syncthreads();
  for (int e = tid; e < J2 * J2; e += 256) {
    int i = e % J2, j = e / J2;
    if (i > j) Ms[i][j] = Ms[j][i];
  }
  __syncthreads();

  // ---- inner solve: M = R^T R (Cholesky on the matrix cores, semi-definite safe), then ONE-SIDED
  // Jacobi on the columns of R (R W has orthogonal columns  <=>  W^T M W diagonal).  One barrier per
  // step and no serial parameter phase: every pair (p, q) of a step is owned by 8 lanes that form the
  // three dot products with two shuffles and rotate their 8 rows of R and W.  (The earlier two-sided
  // LDS version cost ~2.5 us per step = 315 us per call, 85 % of the SVD; profiles/r01_other_configs.)
  {
    // (1) Cholesky, rows four at a time, rank-4 MFMA updates (same scheme as cq_step_kernel in mpsk_cholqr.hip)
    __shared__ double P[2][4][J2];
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, lr = lane >> 4, lc = lane & 15;
    // symmetric scaling to unit diagonal: the column norms of X can span many orders of magnitude
    // (graded singular values); chol(D^-1 M D^-1) is then well behaved and R = R~ D has Gram M.
    __shared__ double dsc[J2], dinv[J2];
    if (tid < J2) {
      const double dd = Ms[tid][tid];
      dsc[tid] = dd > 0.0 ? sqrt(dd) : 0.0;
      dinv[tid] = dd > 0.0 ? 1.0 / sqrt(dd) : 0.0;
    }
    __syncthreads();
    sv_d4 acc[2][2];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const int rr = 32 * wr + 16 * ti + lr + 4 * rg, cc = 32 * wc + 16 * tj + lc;
          acc[ti][tj][rg] = (rr == cc) ? (dinv[rr] > 0.0 ? 1.0 : 0.0) : Ms[rr][cc] * dinv[rr] * dinv[cc];
        }
    const double ptol = 1.0e-14;
    __syncthreads();                       // everyone has read Ms before it is overwritten with R
    for (int c = 0; c < J2 / 4; ++c) {
      const int j0 = 4 * c;
      double (*Pb)[J2] = P[c & 1];
      if (wr == (j0 >> 5)) {
        const int ti = (j0 >> 4) & 1, q = (j0 >> 2) & 3;
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) {
          const sv_d4 v = ti ? acc[1][tj] : acc[0][tj];
          Pb[lr][32 * wc + 16 * tj + lc] = (q == 0) ? v[0] : (q == 1) ? v[1] : (q == 2) ? v[2] : v[3];
        }
      }
      __syncthreads();
      if (wave == 0) {
        double pr[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) pr[t] = Pb[t][lane];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const double piv = sv_readlane(pr[t], j0 + t);
          const bool ok = (piv > ptol) && (piv < 1.0e300);     // semi-definite: a vanishing pivot zeroes the row
          double rs_, sq_;
          sv_piv_rsqrt(ok ? piv : 1.0, &rs_, &sq_);
          const double sq = ok ? sq_ : 0.0;
          const double rs = ok ? rs_ : 0.0;
          pr[t] = (lane > j0 + t) ? pr[t] * rs : (lane == j0 + t ? sq : 0.0);
#pragma unroll
          for (int u = t + 1; u < 4; ++u) pr[u] -= sv_readlane(pr[t], j0 + u) * pr[t];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) { Pb[t][lane] = pr[t]; Ms[j0 + t][lane] = pr[t] * dsc[lane]; }   // row j0+t of R = R~ D
      }
      __syncthreads();
      double af[2], bf[2];
#pragma unroll
      for (int ti = 0; ti < 2; ++ti) af[ti] = -Pb[lr][32 * wr + 16 * ti + lc];
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) bf[tj] = Pb[lr][32 * wc + 16 * tj + lc];
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
          acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[ti], bf[tj], acc[ti][tj], 0, 0, 0);
    }
    __syncthreads();
  }
  // (2) one-sided Jacobi on R = Ms (upper triangular), W = Ws
  // Pair index of this 8-lane team.  Teams that share a 32-lane LDS read group (16-lane write group) get
  // pair indices 8 apart: their columns pp = (st + pk) % 63 then sit 8 apart too, so the four 8-row
  // segments {col + pj} tile the 32 bank pairs instead of piling onto the same ones (consecutive pk:
  // ~4-way conflicts on all 64 LDS accesses of a step, 3000 cycles/step).
  const int team = tid >> 3, pj = tid & 7;
  const int pk = ((team & 3) << 3) | (team >> 2);
  for (int sweep = 0; sweep < inner_sweeps; ++sweep) {
    if (tid == 0) any_rot = 0;
    __syncthreads();
    int rotated = 0;
    for (int st = 0; st < J2 - 1; ++st) {
      int pp, qq;
      if (pk == 0) { pp = J2 - 1; qq = st; }
      else { pp = (st + pk) % (J2 - 1); qq = (st + (J2 - 1) - pk) % (J2 - 1); }
      if (pp > qq) { const int t = pp; pp = qq; qq = t; }
      double rp[8], rq[8], wp[8], wq[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int r = pj + 8 * i;
        rp[i] = Ms[r][pp]; rq[i] = Ms[r][qq]; wp[i] = Ws[r][pp]; wq[i] = Ws[r][qq];
      }
      double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
      for (int i = 0; i < 8; ++i) { al += rp[i] * rp[i]; be += rq[i] * rq[i]; ga += rp[i] * rq[i]; }
#pragma unroll
      for (int off = 1; off < 8; off <<= 1) {
        al += __shfl_xor(al, off, 64); be += __shfl_xor(be, off, 64); ga += __shfl_xor(ga, off, 64);
      }
      // Rotation parameters without fp64 division / square root (each is a ~30-instruction
      // software sequence and 6 of them per step dominated this kernel): the ANGLE only has to be
      // approximately right for Jacobi to converge, so t = tan(theta) comes from fp32 hardware
      // rcp / sqrt; (c, s) must be orthogonal to fp64 accuracy, so c = (1 + t^2)^(-1/2) is an fp32
      // rsqrt seed polished by two fp64 Newton steps (error ~1e-7 -> 1e-14 -> 1e-28).
      double c = 1.0, sn = 0.0;
      const double ab = al * be, gg = ga * ga;
      if (gg > 1.0e-34 * ab) {
        const double num = (be - al) * 0.5;
        int ex;
        (void)frexp(fmax(fabs(num), fabs(ga)), &ex);       // common power-of-two scale: no fp32 over/underflow
        const float zf = (float)ldexp(num, -ex) * __frcp_rn((float)ldexp(ga, -ex));
        // |zeta| > 1e4: sqrt(1 + zeta^2) == |zeta| in fp32 and zeta^2 would overflow for graded column pairs
        // (norm ratio x cosine < 1e-19) -- those rotations were silently dropped (t = 1/inf) and the sweep
        // count ran to the cap; t = 1 / (2 zeta) there.
        const float az = fabsf(zf);
        const float tf = copysignf(1.0f, zf) * (az > 1.0e4f ? 0.5f * __frcp_rn(az) : __frcp_rn(az + __fsqrt_rn(1.0f + zf * zf)));
        const double t = (double)tf;
        const double x = 1.0 + t * t;
        double r = (double)__frsqrt_rn((float)x);
        r = r * (1.5 - 0.5 * x * r * r);
        r = r * (1.5 - 0.5 * x * r * r);
        c = r;
        sn = r * t;
        if (gg > 1.0e-20 * ab) rotated = 1;   // |cos| > 1e-10: another inner sweep is worth it (quadratic
      }                                        // convergence; the OUTER loop re-measures every pair anyway)
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        const int r = pj + 8 * i;
        Ms[r][pp] = c * rp[i] - sn * rq[i];
        Ms[r][qq] = sn * rp[i] + c * rq[i];
        Ws[r][pp] = c * wp[i] - sn * wq[i];
        Ws[r][qq] = sn * wp[i] + c * wq[i];
      }
      __syncthreads();
    }
    if (rotated) any_rot = 1;
    __syncthreads();
    if (!any_rot) break;
    __syncthreads();
  }
  // One Newton-Schulz step  W <- W (3 I - W^T W) / 2  removes the O(#rotations * eps) drift of
  // W's orthogonality, so the accumulated V (and G = theta V) stay orthogonal over ~10^3 rounds.
  // Both 64^3 products run on the matrix cores (4 waves x 2x2 tiles of 16x16).
  __syncthreads();
  {
    const int lane = tid & 63, wave = tid >> 6;
    const int wr = wave >> 1, wc = wave & 1, fq = lane >> 4, fr = lane & 15;
    sv_d4 acc[2][2];
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = sv_d4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < J2; k0 += 4) {       // T = W^T W
      double af[2], bf[2];
#pragma unroll
      for (int ti = 0; ti < 2; ++ti) af[ti] = Ws[k0 + fq][32 * wr + 16 * ti + fr];
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) bf[tj] = Ws[k0 + fq][32 * wc + 16 * tj + fr];
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
          acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[ti], bf[tj], acc[ti][tj], 0, 0, 0);
    }
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) Ms[32 * wr + 16 * ti + fq + 4 * rg][32 * wc + 16 * tj + fr] = acc[ti][tj][rg];
    __syncthreads();
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = sv_d4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < J2; k0 += 4) {       // P = W T
      double af[2], bf[2];
#pragma unroll
      for (int ti = 0; ti < 2; ++ti) af[ti] = Ws[32 * wr + 16 * ti + fr][k0 + fq];
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) bf[tj] = Ms[k0 + fq][32 * wc + 16 * tj + fr];
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
          acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[ti], bf[tj], acc[ti][tj], 0, 0, 0);
    }
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const int i = 32 * wr + 16 * ti + fq + 4 * rg, j = 32 * wc + 16 * tj + fr;
          Wp[i + J2 * j] = 1.5 * Ws[i][j] - 0.5 * acc[ti][tj][rg];
        }
  }
}

// ---- rotation kernel, second generation (MPSK_SVD_EIG=1 selects the first) -------------------------------------------
// Same mathematics as jacobi_eig_kernel (scaled Cholesky of the pair's Gram matrix, one-sided cyclic Jacobi on the factor R,
// accumulated rotations W, one Newton-Schulz step), different data placement.  The first kernel keeps R AND W in LDS and every
// one of the 63 steps reads and writes both (128 KB of LDS traffic per step, ~770 cycles of ds_write alone): 70 of its
// ~100 us.  Here W never touches LDS during the iteration:
//   * waves 0-3 rotate R in LDS exactly as before (8 lanes per column pair) and publish each pair's (c, s);
//   * wave 4 holds W in REGISTERS, lane = row, 64 columns = 64 register pairs.  The round-robin order is known at compile
//     time, so with the 63 steps fully unrolled every rotation addresses its two columns statically; the wave applies the
//     rotations of step t while the other four work on step t + 1 (one barrier per step, (c, s) double-buffered).
// LDS traffic per step halves and W's rotations leave the critical path.
constexpr int EIG2_THREADS = 320;
#ifndef MPSK_EIG2_DIAG
#define MPSK_EIG2_DIAG 0      // timing diagnostics only (wrong results): 1 = wave 4 idles, 2 = waves 0-3 idle
#endif

template <int CTRL>
__device__ __forceinline__ double sv_dpp(double x) {
  int lo = __double2loint(x), hi = __double2hiint(x);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, false);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, false);
  return __hiloint2double(hi, lo);
}

// Order of the 63 steps of one inner sweep over the 64 columns of a pair (block A = columns 0-31, block B = 32-63):
//   steps 0-30   INTRA: two independent 32-column round robins side by side (16 + 16 pairs per step; B runs its round robin
//                16 steps ahead of A's, which keeps the four teams of a 32-lane LDS access group 8 columns apart);
//   steps 31-62  CROSS: pair k = (k, 32 + (k + t) mod 32): every column of A against every column of B.
// A block leaves a pair with its 32 columns mutually orthogonal, so on its next visit the intra rotations are second-order
// small: the kernel skips steps 0-30 outright when the measured intra cosines are far below the cross ones (see `intra_ratio`).
constexpr int EIG2_NI = J2 / 2 - 1;          // 31 intra steps
__host__ __device__ constexpr int eig2_pair(int t, int pk, bool hi) {
  int a = 0, b = 0;
  if (t < EIG2_NI) {
    const int k = pk & 15, off = (pk & 16) ? J2 / 2 : 0;
    const int tt = (pk & 16) ? (t + 16) % EIG2_NI : t;
    a = off + ((k == 0) ? EIG2_NI : (tt + k) % EIG2_NI);
    b = off + ((k == 0) ? tt : (tt + EIG2_NI - k) % EIG2_NI);
  } else {
    a = pk;
    b = J2 / 2 + (pk + (t - EIG2_NI)) % (J2 / 2);
  }
  return hi ? (a < b ? b : a) : (a < b ? a : b);
}
__host__ __device__ constexpr int eig2_lo(int t, int pk) { return eig2_pair(t, pk, false); }
__host__ __device__ constexpr int eig2_hi(int t, int pk) { return eig2_pair(t, pk, true); }
// wave 4: the 32 rotations of step T on the register-resident rows of W (every index a compile-time constant).  The
// (c, s) pairs are broadcast LDS reads (all lanes, one address), fetched in groups of 8 one group ahead of their use;
// scheduling barriers keep the compiler from clustering all 32 reads up front (128 more live registers: it spilled W).
typedef double sv_d2 __attribute__((ext_vector_type(2)));
template <int T, int G, int... K>
__device__ __forceinline__ void eig2_w_group(double (&w)[J2], const sv_d2 (&cb)[8], std::integer_sequence<int, K...>) {
  ((void)([&] {
     constexpr int pp = eig2_lo(T, 8 * G + K), qq = eig2_hi(T, 8 * G + K);
     const double c = cb[K].x, sn = cb[K].y;
     const double a = w[pp], b = w[qq];
     w[pp] = c * a - sn * b;
     w[qq] = sn * a + c * b;
     // pins the rotation HERE: pure arithmetic is not ordered against s_barrier, and without this the compiler sank all
     // 2016 rotations behind the last barrier and spilled every (c, s) it had to read in place (32 KB of scratch per lane)
     asm volatile("" : "+v"(w[pp]), "+v"(w[qq]));
   }()),
   ...);
}
template <int G>
__device__ __forceinline__ void eig2_w_fetch(sv_d2 (&cb)[8], const double* __restrict__ csb) {
#pragma unroll
  for (int k = 0; k < 8; ++k) cb[k] = *reinterpret_cast<const sv_d2*>(csb + 2 * (8 * G + k));
}
template <int T>
__device__ __forceinline__ void eig2_w_apply(double (&w)[J2], const double* __restrict__ csb) {
  sv_d2 c0[8], c1[8];
  constexpr auto seq = std::make_integer_sequence<int, 8>{};
  eig2_w_fetch<0>(c0, csb);
  eig2_w_fetch<1>(c1, csb);
  __builtin_amdgcn_sched_barrier(0);
  eig2_w_group<T, 0>(w, c0, seq);
  __builtin_amdgcn_sched_barrier(0);
  eig2_w_fetch<2>(c0, csb);
  __builtin_amdgcn_sched_barrier(0);
  eig2_w_group<T, 1>(w, c1, seq);
  __builtin_amdgcn_sched_barrier(0);
  eig2_w_fetch<3>(c1, csb);
  __builtin_amdgcn_sched_barrier(0);
  eig2_w_group<T, 2>(w, c0, seq);
  __builtin_amdgcn_sched_barrier(0);
  eig2_w_group<T, 3>(w, c1, seq);
  __builtin_amdgcn_sched_barrier(0);
}

// waves 0-3: step `st` of the one-sided Jacobi sweep on R (LDS) for the pair of this 8-lane team; publishes (c, s)
__device__ __forceinline__ void eig2_r_step(double (*Ms)[J2 + 1], double* __restrict__ csw, int st, int pk, int pj, int* rotated) {
  const int pp = eig2_lo(st, pk), qq = eig2_hi(st, pk);
  double rp[8], rq[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = pj + 8 * i;
    rp[i] = Ms[r][pp]; rq[i] = Ms[r][qq];
  }
  double al = 0.0, be = 0.0, ga = 0.0;
#pragma unroll
  for (int i = 0; i < 8; ++i) { al += rp[i] * rp[i]; be += rq[i] * rq[i]; ga += rp[i] * rq[i]; }
  // 8-lane sums by DPP (quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror): VALU moves with a few cycles of
  // latency; __shfl_xor compiles to ds_bpermute_b32, an LDS-crossbar round trip per stage on the serial path of the step
  al += sv_dpp<0xB1>(al); be += sv_dpp<0xB1>(be); ga += sv_dpp<0xB1>(ga);
  al += sv_dpp<0x4E>(al); be += sv_dpp<0x4E>(be); ga += sv_dpp<0x4E>(ga);
  al += sv_dpp<0x141>(al); be += sv_dpp<0x141>(be); ga += sv_dpp<0x141>(ga);
  // Rotation parameters in ~20 fp64 operations (the first kernel's fp32 detour with frexp / ldexp / conversions is ~45):
  // the ANGLE only needs to be approximately right, so zeta, sqrt(1 + zeta^2) and t come from the hardware reciprocal /
  // rsqrt approximations (v_rcp_f64 / v_rsq_f64, ~1e-8 relative); (c, s) must be orthonormal to fp64 accuracy, so
  // c = (1 + t^2)^(-1/2) is polished by two Newton steps and s = c t.  No overflow: a rotation is only formed when
  // gamma^2 > 1e-34 alpha beta, i.e. |zeta| < ~1e17 |beta - alpha| / sqrt(alpha beta) stays far inside the fp64 range.
  double c = 1.0, sn = 0.0;
  const double ab = al * be, gg = ga * ga;
  if (gg > 1.0e-34 * ab) {
    const double zeta = 0.5 * (be - al) * __builtin_amdgcn_rcp(ga);
    const double az = fabs(zeta);
    const double w = fma(zeta, zeta, 1.0);
    const double den = az + w * __builtin_amdgcn_rsq(w);          // |zeta| + sqrt(1 + zeta^2)
    const double t = copysign(__builtin_amdgcn_rcp(den), zeta);
    const double x = fma(t, t, 1.0);
    double r = __builtin_amdgcn_rsq(x);
    r = r * (1.5 - 0.5 * x * r * r);
    r = r * (1.5 - 0.5 * x * r * r);
    c = r;
    sn = r * t;
    if (gg > 1.0e-20 * ab) *rotated = 1;
  }
  if (pj == 0) { csw[2 * pk] = c; csw[2 * pk + 1] = sn; }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int r = pj + 8 * i;
    Ms[r][pp] = c * rp[i] - sn * rq[i];
    Ms[r][qq] = sn * rp[i] + c * rq[i];
  }
}

// wave 4's side of one inner sweep: phase ST applies the rotations of step ST - 1 (published by waves 0-3 during phase
// ST - 1) and joins the phase's barrier.  Waves 0-3 run their own, rolled loop with the SAME number of barriers
// (s_barrier counts arrivals, not program locations).
template <int ST, int END>
__device__ __forceinline__ void eig2_w_phases(double (*cs)[2 * 32], double (&w)[J2]) {
  if constexpr (ST < END) {
    if constexpr (ST >= 1 && MPSK_EIG2_DIAG != 1) eig2_w_apply<ST - 1>(w, cs[(ST - 1) & 1]);
    __syncthreads();
    eig2_w_phases<ST + 1, END>(cs, w);
  }
}

__global__ __launch_bounds__(EIG2_THREADS) void jacobi_eig2_kernel(const double* __restrict__ Mpart, int Q,
                                                                   double* __restrict__ Wout, double tol,
                                                                   unsigned long long* __restrict__ flag, int inner_sweeps,
                                                                   double intra_ratio,
                                                                   unsigned long long* __restrict__ dbg) {
  __shared__ double Ms[J2][J2 + 1];
  __shared__ double Ws[J2][J2 + 1];
  __shared__ double P[2][4][J2];
  __shared__ double dsc[J2], dinv[J2];
  __shared__ __attribute__((aligned(16))) double cs[2][2 * 32];     // (c, s) of pair k of a step at [buf][2k], [2k + 1]
  __shared__ double red[2][4];
  __shared__ int any_rot;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const bool rw = tid < 256;                 // waves 0-3: everything the first kernel's 256 threads did, except W
  const int p = blockIdx.x;
  const double* Mp = Mpart + (size_t)p * Q * J2 * J2;
  // diagnostic stamps (dbg != nullptr only in profiling runs: MPSK_SVD_STAMPS=1), 100 MHz real-time counter
#define EIG2_STAMP(i) do { if (dbg && tid == 0 && p == 0) dbg[i] = __builtin_amdgcn_s_memrealtime(); } while (0)
  EIG2_STAMP(0);
  if (rw) {
    double accv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) accv[i] = 0.0;
#pragma unroll 4
    for (int q = 0; q < Q; ++q) {
      const double* mq = Mp + (size_t)q * J2 * J2 + tid;
#pragma unroll
      for (int i = 0; i < 16; ++i) accv[i] += mq[256 * i];
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int e = tid + 256 * i;
      Ms[e % J2][e / J2] = accv[i];
    }
  }
  __syncthreads();
  EIG2_STAMP(1);
  // symmetrise and measure in ONE pass: the thread that owns (i, j), i < j, also owns (j, i); max |cos|^2 through the
  // hardware reciprocal (the convergence decision has 1e-8 of slack), one square root per workgroup at the end
  // (separately for column pairs inside one block and across the two blocks: see eig2_pair)
  double mx = 0.0, mxi = 0.0;
  if (rw) {
    for (int e = tid; e < J2 * J2; e += 256) {
      const int i = e % J2, j = e / J2;
      if (i < j) {
        const double a = 0.5 * (Ms[i][j] + Ms[j][i]);
        const double dd = Ms[i][i] * Ms[j][j];
        const double r2 = (a == 0.0) ? 0.0 : (dd > 0.0 ? a * a * __builtin_amdgcn_rcp(dd) : 1.0);
        if ((i < J2 / 2) == (j < J2 / 2)) mxi = fmax(mxi, r2); else mx = fmax(mx, r2);
        Ms[i][j] = a;
        Ms[j][i] = a;
      }
    }
    for (int off = 32; off > 0; off >>= 1) {
      mx = fmax(mx, __shfl_xor(mx, off, 64));
      mxi = fmax(mxi, __shfl_xor(mxi, off, 64));
    }
    if (lane == 0) { red[0][wave] = mx; red[1][wave] = mxi; }
  }
  __syncthreads();
  mx = fmax(fmax(red[0][0], red[0][1]), fmax(red[0][2], red[0][3]));
  mxi = fmax(fmax(red[1][0], red[1][1]), fmax(red[1][2], red[1][3]));
  // intra steps skipped on the first inner sweep when the blocks are still orthogonal inside relative to the coupling
  // between them (cos^2 ratio; uniform over the workgroup).  Whatever is skipped here is measured again on the next visit.
  const bool skip_intra = mxi <= intra_ratio * mx;
  mx = sqrt(fmax(mx, mxi));
  if (tid == 0) atomicMax(flag, (unsigned long long)__double_as_longlong(mx));
  double* Wp = Wout + (size_t)p * J2 * J2;
  if (mx <= tol) {                           // (uniform over the workgroup)
    for (int e = tid; e < J2 * J2; e += EIG2_THREADS) Wp[e] = (e % J2 == e / J2) ? 1.0 : 0.0;
    return;
  }
  EIG2_STAMP(2);
  // ---- (1) Cholesky of the unit-diagonal scaled Gram matrix, rows four at a time (see jacobi_eig_kernel)
  const int wr = (wave >> 1) & 1, wc = wave & 1, lr = lane >> 4, lc = lane & 15;
  if (tid < J2) {
    const double dd = Ms[tid][tid];
    dsc[tid] = dd > 0.0 ? sqrt(dd) : 0.0;
    dinv[tid] = dd > 0.0 ? 1.0 / sqrt(dd) : 0.0;
  }
  __syncthreads();
  sv_d4 acc[2][2];
#pragma unroll
  for (int ti = 0; ti < 2; ++ti)
#pragma unroll
    for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = sv_d4{0.0, 0.0, 0.0, 0.0};
  if (rw) {
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj)
#pragma unroll
        for (int rg = 0; rg < 4; ++rg) {
          const int rr = 32 * wr + 16 * ti + lr + 4 * rg, cc = 32 * wc + 16 * tj + lc;
          acc[ti][tj][rg] = (rr == cc) ? (dinv[rr] > 0.0 ? 1.0 : 0.0) : Ms[rr][cc] * dinv[rr] * dinv[cc];
        }
  }
  const double ptol = 1.0e-14;
  __syncthreads();                           // everyone has read Ms before it is overwritten with R
  for (int c = 0; c < J2 / 4; ++c) {
    const int j0 = 4 * c;
    double (*Pb)[J2] = P[c & 1];
    if (rw && wr == (j0 >> 5)) {
      const int ti = (j0 >> 4) & 1, q = (j0 >> 2) & 3;
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) {
        const sv_d4 v = ti ? acc[1][tj] : acc[0][tj];
        Pb[lr][32 * wc + 16 * tj + lc] = (q == 0) ? v[0] : (q == 1) ? v[1] : (q == 2) ? v[2] : v[3];
      }
    }
    __syncthreads();
    if (wave == 0) {
      double pr[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) pr[t] = Pb[t][lane];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const double piv = sv_readlane(pr[t], j0 + t);
        const bool ok = (piv > ptol) && (piv < 1.0e300);     // semi-definite: a vanishing pivot zeroes the row
        double rs_, sq_;
        sv_piv_rsqrt(ok ? piv : 1.0, &rs_, &sq_);
        const double sq = ok ? sq_ : 0.0;
        const double rs = ok ? rs_ : 0.0;
        pr[t] = (lane > j0 + t) ? pr[t] * rs : (lane == j0 + t ? sq : 0.0);
#pragma unroll
        for (int u = t + 1; u < 4; ++u) pr[u] -= sv_readlane(pr[t], j0 + u) * pr[t];
      }
#pragma unroll
      for (int t = 0; t < 4; ++t) { Pb[t][lane] = pr[t]; Ms[j0 + t][lane] = pr[t] * dsc[lane]; }   // row j0+t of R = R~ D
    }
    __syncthreads();
    if (rw) {
      double af[2], bf[2];
#pragma unroll
      for (int ti = 0; ti < 2; ++ti) af[ti] = -Pb[lr][32 * wr + 16 * ti + lc];
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) bf[tj] = Pb[lr][32 * wc + 16 * tj + lc];
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
          acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[ti], bf[tj], acc[ti][tj], 0, 0, 0);
    }
  }
  __syncthreads();
  EIG2_STAMP(3);
  // ---- (2) one-sided Jacobi on R (LDS, waves 0-3); W in the registers of wave 4.  The two sides run DIFFERENT code with
  // the same barrier count per inner sweep: 1 + 64 + 1 (+ 1 when another sweep follows), then one before step (3).
  if (rw) {
    const int team = tid >> 3, pj = tid & 7;
    const int pk = ((team & 3) << 3) | (team >> 2);
    for (int sweep = 0; sweep < inner_sweeps; ++sweep) {
      if (tid == 0) any_rot = 0;
      __syncthreads();
      int rotated = 0;
      const int st0 = (sweep == 0 && skip_intra) ? EIG2_NI : 0;
      for (int st = st0; st < J2; ++st) {    // phase st: step st (< 63); wave 4 applies step st - 1 meanwhile
        if (st < J2 - 1 && MPSK_EIG2_DIAG != 2) eig2_r_step(Ms, cs[st & 1], st, pk, pj, &rotated);
        __syncthreads();
      }
      if (rotated) any_rot = 1;
      __syncthreads();
      if (!any_rot) break;
      __syncthreads();
    }
    __syncthreads();
  } else {
    double w[J2];
#pragma unroll
    for (int c = 0; c < J2; ++c) w[c] = (c == lane) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < inner_sweeps; ++sweep) {
      __syncthreads();
      if (!(sweep == 0 && skip_intra)) {
        eig2_w_phases<0, EIG2_NI>(cs, w);
        if (MPSK_EIG2_DIAG != 1) eig2_w_apply<EIG2_NI - 1>(w, cs[(EIG2_NI - 1) & 1]);
      }
      __syncthreads();                       // phase 31
      eig2_w_phases<EIG2_NI + 1, J2>(cs, w);
      __syncthreads();
      if (!any_rot) break;
      __syncthreads();
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < J2; ++c) Ws[lane][c] = w[c];
  }
  // ---- (3) Newton-Schulz step  W <- W (3 I - W^T W) / 2  on the matrix cores (waves 0-3)
  __syncthreads();
  EIG2_STAMP(4);
  {
    const int fq = lane >> 4, fr = lane & 15;
#pragma unroll
    for (int ti = 0; ti < 2; ++ti)
#pragma unroll
      for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = sv_d4{0.0, 0.0, 0.0, 0.0};
    if (rw) {
      for (int k0 = 0; k0 < J2; k0 += 4) {       // T = W^T W
        double af[2], bf[2];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) af[ti] = Ws[k0 + fq][32 * wr + 16 * ti + fr];
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) bf[tj] = Ws[k0 + fq][32 * wc + 16 * tj + fr];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
          for (int tj = 0; tj < 2; ++tj)
            acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[ti], bf[tj], acc[ti][tj], 0, 0, 0);
      }
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) Ms[32 * wr + 16 * ti + fq + 4 * rg][32 * wc + 16 * tj + fr] = acc[ti][tj][rg];
    }
    __syncthreads();
    if (rw) {
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) acc[ti][tj] = sv_d4{0.0, 0.0, 0.0, 0.0};
      for (int k0 = 0; k0 < J2; k0 += 4) {       // P = W T
        double af[2], bf[2];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti) af[ti] = Ws[32 * wr + 16 * ti + fr][k0 + fq];
#pragma unroll
        for (int tj = 0; tj < 2; ++tj) bf[tj] = Ms[k0 + fq][32 * wc + 16 * tj + fr];
#pragma unroll
        for (int ti = 0; ti < 2; ++ti)
#pragma unroll
          for (int tj = 0; tj < 2; ++tj)
            acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[ti], bf[tj], acc[ti][tj], 0, 0, 0);
      }
#pragma unroll
      for (int ti = 0; ti < 2; ++ti)
#pragma unroll
        for (int tj = 0; tj < 2; ++tj)
#pragma unroll
          for (int rg = 0; rg < 4; ++rg) {
            const int i = 32 * wr + 16 * ti + fq + 4 * rg, j = 32 * wc + 16 * tj + fr;
            Wp[i + J2 * j] = 1.5 * Ws[i][j] - 0.5 * acc[ti][tj][rg];
          }
    }
  }
  EIG2_STAMP(5);
#undef EIG2_STAMP
}

// MPSK_SVD_STAMPS=1: pair 0 of every launch leaves six real-time stamps (100 MHz) here; printed with MPSK_SVD_DEBUG
static unsigned long long* g_eig2_dbg = nullptr;
static const int g_svd_eig = getenv("MPSK_SVD_EIG") ? atoi(getenv("MPSK_SVD_EIG")) : 2;
// intra-block steps are skipped when max intra cos^2 <= this * max cross cos^2 (0 = never skip)
static const double g_svd_intra = getenv("MPSK_SVD_INTRA") ? atof(getenv("MPSK_SVD_INTRA")) : 1.0e-2;
static inline void launch_eig(int npairs, hipStream_t s, const double* Mpart, int Q, double* Wb, double tol,
                              unsigned long long* flag, int inner_sweeps) {
  if (g_svd_eig == 1)
    hipLaunchKernelGGL(jacobi_eig_kernel, dim3(npairs), dim3(256), 0, s, Mpart, Q, Wb, tol, flag, inner_sweeps);
  else
    hipLaunchKernelGGL(jacobi_eig2_kernel, dim3(npairs), dim3(EIG2_THREADS), 0, s, Mpart, Q, Wb, tol, flag, inner_sweeps,
                       npairs > 1 ? g_svd_intra : 0.0, g_eig2_dbg);
}

// sigma2[j] = sum_r G[r, j]^2   (one workgroup per column)
__global__ __launch_bounds__(256) void colnorm2_kernel(const double* __restrict__ G, int ldg, int m,
                                                       double* __restrict__ sigma2) {
  __shared__ double red[4];
  const double* g = G + (size_t)blockIdx.x * ldg;
  double acc = 0.0;
  for (int r = threadIdx.x; r < m; r += 256) acc += g[r] * g[r];
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) sigma2[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// out(r, i) [+transposed store] = src[r, perm[i]] * scale[i]
__global__ __launch_bounds__(256) void gather_cols_kernel(const double* __restrict__ src, int lds_, int rows,
                                                          const int* __restrict__ perm, const double* __restrict__ scale,
                                                          int k, double* __restrict__ out, int ldo, int transposed) {
  const int64_t total = (int64_t)rows * k;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    int r = (int)(e % rows), i = (int)(e / rows);
    double v = src[r + (size_t)perm[i] * lds_];
    if (scale) v *= scale[i];
    if (transposed) out[i + (size_t)r * ldo] = v;
    else out[r + (size_t)i * ldo] = v;
  }
}

__global__ __launch_bounds__(256) void svd_init_kernel(const double* __restrict__ theta, int ldt, int m, int n,
                                                       int transposed, double* __restrict__ G, int mm, int npad,
                                                       double* __restrict__ V, int nn) {
  // G (mm x npad) = theta or theta^T, zero padded ; V (nn x npad) = [I 0]
  const int64_t tg = (int64_t)mm * npad, tv = (int64_t)nn * npad;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < tg + tv; e += (int64_t)gridDim.x * blockDim.x) {
    if (e < tg) {
      int r = (int)(e % mm), c = (int)(e / mm);
      double v = 0.0;
      if (c < nn) v = transposed ? theta[c + (size_t)r * ldt] : theta[r + (size_t)c * ldt];
      G[e] = v;
    } else {
      int64_t f = e - tg;
      int r = (int)(f % nn), c = (int)(f / nn);
      V[f] = (r == c) ? 1.0 : 0.0;
    }
  }
}

constexpr double SVD_EXIT_COS = 1.0e-12;   // sweeps end without a verification sweep from this max |cos| on (see tsvd())

struct SvdPlan {
  int mm, nn, npad, P, Q, transposed;
  size_t bytes;
};

// ---- chained tournament ---------------------------------------------------------------------------------------------
// The rotation kernel is latency-bound (one workgroup per pair, ~100 us) and leaves most of the chip idle, while the Gram
// and update GEMMs of a round are bandwidth-bound full-chip launches.  A plain round-robin round is three DEPENDENT
// launches, so the two kinds of work never overlap.  The sweep is therefore re-ordered into NC independent CHAINS
// (sub-tournaments over disjoint block sets, each on its own stream, no events inside a stage):
//   the 2P column blocks form 2 NC groups of pc = P / NC blocks;
//   stage A : chain c runs a full round-robin on the union of two groups                   (2 pc - 1 rounds, pc pairs each)
//   stage B : the remaining group pairs follow a 1-factorisation of K_{2NC} (circle method) whose first matching is the
//             set of unions of stage A; per matching every chain runs the bipartite tournament of one group pair
//                                                                                         (2 NC - 2 matchings x pc rounds)
// = 2P - 1 rounds and every pair of blocks exactly once per sweep, as in the plain order.  The rotations of one chain run
// under the GEMMs of the others.  The block -> slot permutation between rounds is only a table of C offsets of the update
// GEMM (one table per round); the LAST round of a stage writes blocks into other chains' slot ranges and is bracketed by
// two all-stream barriers (2 (2 NC - 1) per sweep).  NC = 2 is the "phased" schedule of round 2.
struct ChainSched {
  int NC = 1, pc = 0, rounds = 0;
  std::vector<int> blk;           // [rounds][P][2]: logical block in (pair slot p, half h); block ids = round-0 slots
  std::vector<char> stage_first, stage_last;
};

static bool build_chain_schedule(int P, int NC, ChainSched* sc) {
  if (NC < 2 || P % NC != 0 || P / NC < 2) return false;
  const int pc = P / NC, NG = 2 * NC, M = NG - 1, T = NG - 1;
  sc->NC = NC; sc->pc = pc; sc->rounds = 2 * P - 1;
  sc->blk.assign((size_t)sc->rounds * P * 2, -1);
  sc->stage_first.assign(sc->rounds, 0);
  sc->stage_last.assign(sc->rounds, 0);
  auto matching = [&](int r, std::vector<std::pair<int, int>>* out) {
    out->clear();
    out->push_back({T, r % M});
    for (int k = 1; k < NC; ++k) out->push_back({(r + k) % M, ((r - k) % M + M) % M});
  };
  std::vector<std::pair<int, int>> mt;
  int r = 0;
  // stage A
  matching(0, &mt);
  sc->stage_first[0] = 1;
  const int n2 = 2 * pc;
  for (int t = 0; t < n2 - 1; ++t, ++r) {
    for (int c = 0; c < NC; ++c) {
      std::vector<int> B(n2), arr(n2);
      for (int i = 0; i < pc; ++i) { B[i] = mt[c].first * pc + i; B[pc + i] = mt[c].second * pc + i; }
      for (int i = 0; i < n2 - 1; ++i) arr[i] = B[(i + t) % (n2 - 1)];
      arr[n2 - 1] = B[n2 - 1];
      for (int i = 0; i < pc; ++i) {
        int* e = &sc->blk[((size_t)r * P + c * pc + i) * 2];
        e[0] = arr[i]; e[1] = arr[n2 - 1 - i];
      }
    }
  }
  sc->stage_last[r - 1] = 1;
  // stage B
  for (int sm = 1; sm <= NG - 2; ++sm) {
    matching(sm, &mt);
    sc->stage_first[r] = 1;
    for (int t = 0; t < pc; ++t, ++r)
      for (int c = 0; c < NC; ++c)
        for (int i = 0; i < pc; ++i) {
          int* e = &sc->blk[((size_t)r * P + c * pc + i) * 2];
          e[0] = mt[c].first * pc + i; e[1] = mt[c].second * pc + (i + t) % pc;
        }
    sc->stage_last[r - 1] = 1;
  }
  if (r != sc->rounds) return false;
  // relabel: block id = its slot in round 0 (the initial column order of G)
  std::vector<int> slot0(2 * P, -1);
  for (int p = 0; p < P; ++p) for (int h = 0; h < 2; ++h) slot0[sc->blk[((size_t)p) * 2 + h]] = 2 * p + h;
  for (int b = 0; b < 2 * P; ++b) if (slot0[b] < 0) return false;
  for (auto& v : sc->blk) v = slot0[v];
  // every unordered pair of blocks exactly once
  std::vector<char> seen((size_t)4 * P * P, 0);
  for (int rr = 0; rr < sc->rounds; ++rr)
    for (int p = 0; p < P; ++p) {
      const int a = sc->blk[((size_t)rr * P + p) * 2], b = sc->blk[((size_t)rr * P + p) * 2 + 1];
      if (a == b || seen[(size_t)a * 2 * P + b]) return false;
      seen[(size_t)a * 2 * P + b] = seen[(size_t)b * 2 * P + a] = 1;
    }
  return true;
}

static int svd_default_chains(int P) {
  // measured (MI355X, mode 2, graded6; profiles/r03_svd_chains.log): n = 1024 (P = 16): 27.3 ms unchained, 34.0 with 2 chains
  // (the stage barriers cost more than the overlap returns on launches this small); n = 2048: 86 / 84 / 92 ms with 1 / 2 / 4;
  // n = 4096: 290 / - / 252 ms
  int nc = (P >= 64 && P % 4 == 0) ? 4 : ((P >= 32 && P % 2 == 0) ? 2 : 1);
  if (const char* ev = getenv("MPSK_SVD_CHAINS")) { const int v = atoi(ev); if (v >= 1 && v <= 8) nc = v; }
  if (nc > 1 && (P % nc != 0 || P / nc < 2)) nc = 1;
  return nc;
}

static SvdPlan svd_plan(int m, int n) {
  SvdPlan p;
  p.transposed = (m < n);
  p.mm = p.transposed ? n : m;
  p.nn = p.transposed ? m : n;
  p.npad = ((p.nn + J2 - 1) / J2) * J2;
  p.P = p.npad / J2;
  int target = 1024 / p.P;           // aim at ~1024 Gram tiles per round (and k-tiles too short for split-K)
  if (target < 1) target = 1;
  if (target > 16) target = 16;
  if (const char* ev = getenv("MPSK_SVD_Q")) { int t = atoi(ev); if (t >= 1 && t <= 16) target = t; }
  int q = 1;                         // largest divisor of mm <= target with >= 128 (even) rows per split
  for (int c = target; c >= 2; --c)
    if (p.mm % c == 0 && (p.mm / c) % 2 == 0 && p.mm / c >= 128) { q = c; break; }
  p.Q = q;
  size_t d = (size_t)2 * p.mm * p.npad + (size_t)2 * p.nn * p.npad + (size_t)p.P * p.Q * J2 * J2 +
             (size_t)2 * p.P * J2 * J2 + (size_t)p.npad * 2 + 64;
  // tables: five fixed 2P-entry tables, the Gram tables, and (chained schedule) two destination tables per round
  size_t tabs = (size_t)8 * (2 * p.P) * sizeof(int64_t) + (size_t)p.P * p.Q * 2 * sizeof(int64_t) +
                (size_t)2 * (2 * p.P) * (2 * p.P) * sizeof(int64_t) + 256;
  p.bytes = d * sizeof(double) + tabs + (size_t)p.npad * sizeof(int);
  return p;
}

size_t tsvd_workspace_bytes(int m, int n) { return svd_plan(m, n).bytes; }

// Host-synchronising truncated SVD; see include/mpsk.h (mpsk_tsvd) for the contract.
//
// QR-preconditioned mode (Qpre != nullptr; Drmac-Veselic): the caller factored the tall orientation
// A' (q_rows x n, = theta or theta^T) as A' = Qpre R and passes theta := R (n x n, m == n).  Jacobi then runs
// on the columns of R^T, which are far closer to orthogonal than those of A' (graded spectra -- the DMRG
// case -- stagnate for tens of sweeps without it):  R^T = G W^T  =>  A' = (Qpre W) Sigma (G Sigma^-1)^T.
// outer_transposed says whether A' was theta^T, i.e. which factor is U and which is Vh.
// xs[0 .. nxs): extra streams of the calling ctx for the chained schedule (xs[0] also serves the V accumulation of the
// unchained order); the main stream s is chain 0.
hipError_t tsvd(int m, int n, const double* theta, int ldt, double* U, int ldu, double* S, double* Vh, int ldv,
                int max_keep, double trunc_err, int* kept, double* disc_norm, void* ws, hipStream_t s,
                std::string* err, int* sweeps_out, const double* Qpre, int ldq, int q_rows, int outer_transposed,
                const hipStream_t* xs, int nxs, int vfree) {
  // vfree: theta := R (n x n) of a QR-preconditioned problem, Jacobi on R^T WITHOUT accumulating the rotations
  // (a third of the per-round traffic): returns S and, in U (n x kmax, ldu), the normalised sorted columns of the
  // converged G = R^T W, i.e. the RIGHT singular vectors of R (and of the matrix R came from).  The caller rebuilds the
  // other factor from the original matrix (mpsk_tsplit).
  SvdPlan pl = svd_plan(m, n);
  hipStream_t s2 = (nxs > 0 && xs) ? xs[0] : nullptr;
  if (vfree) {
    if (m != n) return hipErrorInvalidValue;
    pl.transposed = 1;
  }
  if (Qpre) {
    if (m != n) return hipErrorInvalidValue;
    pl.transposed = 1;                    // G <- R^T
  }
  const int mm = pl.mm, nn = pl.nn, npad = pl.npad, P = pl.P, Q = pl.Q;
  const int kmax = std::min(m, n);
  double* G[2]; double* V[2];
  double* base = (double*)ws;
  G[0] = base; G[1] = G[0] + (size_t)mm * npad;
  V[0] = G[1] + (size_t)mm * npad; V[1] = V[0] + (size_t)nn * npad;
  double* Mpart = V[1] + (size_t)nn * npad;
  double* Wm = Mpart + (size_t)P * Q * J2 * J2;
  double* sigma2 = Wm + (size_t)2 * P * J2 * J2;      // Wm is double-buffered (see the round loop)
  double* scale = sigma2 + npad;
  unsigned long long* flag = (unsigned long long*)(scale + npad);
  int64_t* tabs = (int64_t*)(flag + 8);
  // tables (device): gram: A/B offsets per (p,q) and C offsets; update: A (pair), B (W half), C (dest slot)
  int64_t* t_gramA = tabs;                 // P*Q
  int64_t* t_gramC = t_gramA + (size_t)P * Q;  // P*Q
  int64_t* t_updA_G = t_gramC + (size_t)P * Q; // 2P
  int64_t* t_updA_V = t_updA_G + 2 * P;
  int64_t* t_updB = t_updA_V + 2 * P;
  int64_t* t_updC_G = t_updB + 2 * P;
  int64_t* t_updC_V = t_updC_G + 2 * P;
  int64_t* t_destG = t_updC_V + 2 * P;                 // chained schedule: [rounds][2][P] destination offsets (G)
  int64_t* t_destV = t_destG + (size_t)(2 * P) * (2 * P);   //                                                     (V)
  int* d_perm = (int*)(t_destV + (size_t)(2 * P) * (2 * P));

  // round-robin tournament on 2P blocks: slot 2p = top[p], 2p+1 = bottom[p]
  auto dest_slot = [&](int p, int half) -> int {
    if (P == 1) return half;
    if (half == 0) {                       // top[p]
      if (p == 0) return 0;
      if (p + 1 <= P - 1) return 2 * (p + 1);
      return 2 * (P - 1) + 1;              // top[P-1] -> bottom[P-1]
    }
    if (p == 0) return 2 * 1;              // bottom[0] -> top[1]
    return 2 * (p - 1) + 1;                // bottom[p] -> bottom[p-1]
  };
  const int kq = mm / Q;                   // rows per K-split (Q divides mm by construction)
  ChainSched csch;
  int NC = svd_default_chains(P);
  if (NC > 1 + nxs) NC = (1 + nxs >= 4) ? 4 : ((1 + nxs >= 2) ? 2 : 1);
  if (NC > 1 && (P % NC != 0 || P / NC < 2 || !build_chain_schedule(P, NC, &csch))) NC = 1;
  // host mirror of the device tables (one upload): Gram tables, five 2P-entry update tables, then -- chained schedule --
  // the per-round destination tables of G and V at a fixed distance of (2P)^2 entries (rounds = 2P - 1 < 2P)
  std::vector<int64_t> h((size_t)2 * P * Q + 10 * P + (NC > 1 ? 2 * (size_t)(2 * P) * (2 * P) : 0), 0);
  int64_t* hgA = h.data(); int64_t* hgC = hgA + (size_t)P * Q;
  int64_t* huAG = hgC + (size_t)P * Q; int64_t* huAV = huAG + 2 * P; int64_t* huB = huAV + 2 * P;
  int64_t* huCG = huB + 2 * P; int64_t* huCV = huCG + 2 * P;
  int64_t* hdG = huCV + 2 * P; int64_t* hdV = hdG + (size_t)(2 * P) * (2 * P);
  for (int p = 0; p < P; ++p) {
    for (int q = 0; q < Q; ++q) {
      hgA[p * Q + q] = (int64_t)p * J2 * mm + (int64_t)q * kq;
      hgC[p * Q + q] = ((int64_t)p * Q + q) * J2 * J2;
    }
    // update tables, one entry per pair: entries [0, P) = first half's destination, [P, 2P) = second half's
    huAG[p] = (int64_t)p * J2 * mm;
    huAV[p] = (int64_t)p * J2 * nn;
    huB[p] = (int64_t)p * J2 * J2;
    huCG[p] = (int64_t)dest_slot(p, 0) * JB * mm;
    huCG[P + p] = (int64_t)dest_slot(p, 1) * JB * mm;
    huCV[p] = (int64_t)dest_slot(p, 0) * JB * nn;
    huCV[P + p] = (int64_t)dest_slot(p, 1) * JB * nn;
  }
  if (NC > 1) {
    std::vector<int> slot_next(2 * P);
    for (int r = 0; r < csch.rounds; ++r) {
      const int rn = (r + 1) % csch.rounds;
      for (int p = 0; p < P; ++p)
        for (int hh = 0; hh < 2; ++hh) slot_next[csch.blk[((size_t)rn * P + p) * 2 + hh]] = 2 * p + hh;
      for (int p = 0; p < P; ++p)
        for (int hh = 0; hh < 2; ++hh) {
          const int dst = slot_next[csch.blk[((size_t)r * P + p) * 2 + hh]];
          hdG[((size_t)r * 2 + hh) * P + p] = (int64_t)dst * JB * mm;
          hdV[((size_t)r * 2 + hh) * P + p] = (int64_t)dst * JB * nn;
        }
    }
  }
  hipError_t e;
  if (!g_eig2_dbg && getenv("MPSK_SVD_STAMPS")) { if (hipMalloc(&g_eig2_dbg, 64) != hipSuccess) g_eig2_dbg = nullptr; }
  if ((e = hipMemcpyAsync(tabs, h.data(), h.size() * sizeof(int64_t), hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(svd_init_kernel, dim3(2048), dim3(256), 0, s, theta, ldt, m, n, pl.transposed, G[0], mm, npad,
                     V[0], nn);
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;   // h goes out of scope later; keep it simple

  const bool kq_even = (kq % 2 == 0) && (mm % 2 == 0) && (nn % 2 == 0);
  const double tol = std::sqrt((double)mm) * 2.220446049250313e-16;
  int cur = 0, sweeps = 0;
  // One cyclic inner sweep per visit of a pair is enough: measured on MI355X the outer sweep count does not
  // change (4096^2: 14-15 sweeps with 1, 2 or 3 inner sweeps) while the eig kernel time drops 2.5x.  A single
  // pair (n <= 64) has no outer tournament, so it keeps the full inner iteration.
  int inner_sweeps = (P == 1) ? 3 : 1;
  if (const char* ev = getenv("MPSK_SVD_INNER")) { inner_sweeps = atoi(ev); if (inner_sweeps < 1) inner_sweeps = 1; }
  const int rounds = (P == 1) ? 1 : 2 * P - 1;
  unsigned long long hflag = 0;
  double mx_last = 0.0;
  // Unchained order (NC == 1), two streams: the V accumulation of round r (bandwidth-bound, needs only W_r) runs on s2
  // while the main stream already forms the Gram matrices / rotations of round r+1 (latency-bound, 1 workgroup per pair).
  // W is double-buffered; evW[b]: W_b written (s -> s2), evV[b]: W_b consumed by the V update (s2 -> s).
  if (!s2 || vfree || NC > 1) s2 = s;
  hipStream_t st[8] = {s, s, s, s, s, s, s, s};
  for (int c = 1; c < NC; ++c) st[c] = xs[c - 1];
  hipEvent_t evW[2], evV[2], evB[8], evLag[8];
  std::vector<hipEvent_t> all_ev;
  auto new_event = [&](hipEvent_t* ev) -> hipError_t {
    hipError_t e2 = hipEventCreateWithFlags(ev, hipEventDisableTiming | hipEventDisableSystemFence);
    if (e2 == hipSuccess) all_ev.push_back(*ev);
    return e2;
  };
  auto drop_events = [&]() { for (hipEvent_t ev : all_ev) (void)hipEventDestroy(ev); all_ev.clear(); };
  for (int b = 0; b < 2; ++b) {
    if ((e = new_event(&evW[b])) != hipSuccess) { drop_events(); return e; }
    if ((e = new_event(&evV[b])) != hipSuccess) { drop_events(); return e; }
  }
  for (int c = 0; c < NC && NC > 1; ++c) {
    if ((e = new_event(&evB[c])) != hipSuccess) { drop_events(); return e; }
    if ((e = new_event(&evLag[c])) != hipSuccess) { drop_events(); return e; }
  }
  static const bool lag_on = !(getenv("MPSK_SVD_LAG") && atoi(getenv("MPSK_SVD_LAG")) == 0);
  long rc = 0;                              // global round counter
  int vcur = 0;
  auto barrier_all = [&]() -> hipError_t {  // every chain has finished everything enqueued so far
    hipError_t e2;
    for (int c = 0; c < NC; ++c) if ((e2 = hipEventRecord(evB[c], st[c])) != hipSuccess) return e2;
    for (int c = 0; c < NC; ++c)
      for (int c2 = 0; c2 < NC; ++c2)
        if (c2 != c && (e2 = hipStreamWaitEvent(st[c], evB[c2], 0)) != hipSuccess) return e2;
    return hipSuccess;
  };
  auto sync_chains = [&]() -> hipError_t {
    for (int c = NC - 1; c >= 1; --c) { hipError_t e2 = hipStreamSynchronize(st[c]); if (e2 != hipSuccess) return e2; }
    return hipSuccess;
  };
  for (int sweep = 0; sweep < 40; ++sweep) {
    const auto t_sweep0 = std::chrono::steady_clock::now();
    if ((e = hipMemsetAsync(flag, 0, sizeof(unsigned long long), s)) != hipSuccess) { drop_events(); return e; }
    if (NC > 1) {
      const int pc = csch.pc;
      if ((e = barrier_all()) != hipSuccess) { drop_events(); return e; }      // (flag memset; the previous sweep's last round)
      for (int r = 0; r < csch.rounds; ++r, ++rc) {
        const bool last = csch.stage_last[r] != 0, first = csch.stage_first[r] != 0;
        double* Wb = Wm + (size_t)(rc & 1) * P * J2 * J2;
        const int64_t* dG = t_destG + (size_t)r * 2 * P;
        const int64_t* dV = t_destV + (size_t)r * 2 * P;
        if (last && (e = barrier_all()) != hipSuccess) { drop_events(); return e; }
        // identical chains would march in lockstep (same durations, same start): at the start of a stage chain c starts
        // only when chain c-1 has finished its first Gram product, so that from then on the GEMMs of one chain fall into
        // the rotation windows of the others
        const bool lag = lag_on && first && !last;
        for (int c = 0; c < NC; ++c) {
          hipStream_t sg = st[c];
          const int p0 = c * pc;
          if (lag && c > 0 && (e = hipStreamWaitEvent(sg, evLag[c - 1], 0)) != hipSuccess) { drop_events(); return e; }
          GemmArgs g;
          std::memset(&g, 0, sizeof(g));
          g.A = G[cur]; g.B = G[cur]; g.C = Mpart; g.M = J2; g.N = J2; g.lda = mm; g.ldb = mm; g.ldc = J2;
          g.batch = pc * Q; g.nseg = 1; g.alpha = 1.0; g.beta = 0.0; g.transA = 1; g.transB = 0;
          g.tabA = t_gramA + (size_t)p0 * Q; g.tabB = g.tabA; g.tabC = t_gramC + (size_t)p0 * Q; g.tabs_even = kq_even;
          g.K = kq;
          if ((e = gemm_f64(g, sg)) != hipSuccess) { drop_events(); return e; }
          if (lag && c + 1 < NC && (e = hipEventRecord(evLag[c], sg)) != hipSuccess) { drop_events(); return e; }
          launch_eig(pc, sg, Mpart + (size_t)p0 * Q * J2 * J2, Q, Wb + (size_t)p0 * J2 * J2, tol, flag, inner_sweeps);
          GemmArgs u;
          std::memset(&u, 0, sizeof(u));
          u.B = Wb; u.N = J2; u.K = J2; u.ldb = J2; u.batch = pc; u.nseg = 1; u.alpha = 1.0; u.beta = 0.0;
          u.tabB = t_updB + p0; u.tabs_even = kq_even; u.splitN = JB;
          u.A = G[cur]; u.C = G[cur ^ 1]; u.M = mm; u.lda = mm; u.ldc = mm; u.tabA = t_updA_G + p0;
          u.tabC = dG + p0; u.tabC2 = dG + P + p0;
          if ((e = gemm_f64(u, sg)) != hipSuccess) { drop_events(); return e; }
          if (!vfree) {
            u.A = V[vcur]; u.C = V[vcur ^ 1]; u.M = nn; u.lda = nn; u.ldc = nn; u.tabA = t_updA_V + p0;
            u.tabC = dV + p0; u.tabC2 = dV + P + p0;
            if ((e = gemm_f64(u, sg)) != hipSuccess) { drop_events(); return e; }
          }
        }
        if (last && (e = barrier_all()) != hipSuccess) { drop_events(); return e; }
        cur ^= 1;
        vcur ^= 1;
      }
    }
    for (int r = 0; r < (NC > 1 ? 0 : rounds); ++r, ++rc) {
      const int wb = (int)(rc & 1);
      double* Wb = Wm + (size_t)wb * P * J2 * J2;
      // 1. Gram (TN): M[p][q] = X_p[rows of split q]^T X_p[rows of split q]
      GemmArgs g;
      std::memset(&g, 0, sizeof(g));
      g.A = G[cur]; g.B = G[cur]; g.C = Mpart; g.M = J2; g.N = J2; g.lda = mm; g.ldb = mm; g.ldc = J2;
      g.batch = P * Q; g.nseg = 1; g.alpha = 1.0; g.beta = 0.0; g.transA = 1; g.transB = 0;
      g.tabA = t_gramA; g.tabB = t_gramA; g.tabC = t_gramC; g.tabs_even = kq_even;
      g.K = kq;
      if ((e = gemm_f64(g, s)) != hipSuccess) { drop_events(); return e; }
      // 2. rotations of each 64-column pair (W_b may still be read by the V update of round rc - 2)
      if (rc >= 2 && s2 != s) (void)hipStreamWaitEvent(s, evV[wb], 0);
      launch_eig(P, s, Mpart, Q, Wb, tol, flag, inner_sweeps);
      if (s2 != s) (void)hipEventRecord(evW[wb], s);
      // 3. updates into next round's slots: G on the main stream, V on s2
      GemmArgs u;
      std::memset(&u, 0, sizeof(u));
      u.B = Wb; u.N = J2; u.K = J2; u.ldb = J2; u.batch = P; u.nseg = 1; u.alpha = 1.0; u.beta = 0.0;
      u.tabB = t_updB; u.tabs_even = kq_even; u.splitN = JB;
      u.A = G[cur]; u.C = G[cur ^ 1]; u.M = mm; u.lda = mm; u.ldc = mm; u.tabA = t_updA_G; u.tabC = t_updC_G;
      u.tabC2 = t_updC_G + P;
      if ((e = gemm_f64(u, s)) != hipSuccess) { drop_events(); return e; }
      if (!vfree) {
        if (s2 != s) (void)hipStreamWaitEvent(s2, evW[wb], 0);
        u.A = V[vcur]; u.C = V[vcur ^ 1]; u.M = nn; u.lda = nn; u.ldc = nn; u.tabA = t_updA_V; u.tabC = t_updC_V;
        u.tabC2 = t_updC_V + P;
        if ((e = gemm_f64(u, s2)) != hipSuccess) { drop_events(); return e; }
        if (s2 != s) (void)hipEventRecord(evV[wb], s2);
      }
      cur ^= 1;
      vcur ^= 1;
    }
    ++sweeps;
    const auto t_enq = std::chrono::steady_clock::now();
    if ((e = sync_chains()) != hipSuccess) { drop_events(); return e; }
    if ((e = hipMemcpyAsync(&hflag, flag, sizeof(hflag), hipMemcpyDeviceToHost, s)) != hipSuccess) { drop_events(); return e; }
    if ((e = hipStreamSynchronize(s)) != hipSuccess) { drop_events(); return e; }
    double mx;
    std::memcpy(&mx, &hflag, sizeof(double));
    if (getenv("MPSK_SVD_DEBUG")) {
      const auto t_done = std::chrono::steady_clock::now();
      fprintf(stderr, "[mpsk_tsvd] sweep %d: max |cos| = %.3e (tol %.1e)  host enqueue %.2f ms, sweep %.2f ms\n", sweeps, mx, tol,
              std::chrono::duration<double, std::milli>(t_enq - t_sweep0).count(),
              std::chrono::duration<double, std::milli>(t_done - t_sweep0).count());
      unsigned long long hs[6];
      if (g_eig2_dbg && sweeps <= 2 && hipMemcpy(hs, g_eig2_dbg, sizeof(hs), hipMemcpyDeviceToHost) == hipSuccess)
        fprintf(stderr, "[mpsk_tsvd] eig2 stamps, pair 0 of the sweep's last launch (us): load %.2f  measure+symm %.2f  cholesky %.2f  jacobi %.2f  newton-schulz %.2f\n",
                (hs[1] - hs[0]) * 0.01, (hs[2] - hs[1]) * 0.01, (hs[3] - hs[2]) * 0.01, (hs[4] - hs[3]) * 0.01, (hs[5] - hs[4]) * 0.01);
    }
    mx_last = mx;
    if (mx <= tol) break;
    // Quadratic convergence: a sweep that STARTED with every |cos| <= eps leaves eps^2 -- but only between columns whose
    // singular values are separated.  Inside a cluster of three or more (nearly) equal singular values the rotations are
    // 45 degrees whatever the cosine, each one mixes the cosines to the rest of the cluster instead of squaring them, and a
    // sweep only shrinks them by a constant (measured, exact multiplicities up to 4 at 512^2: start 9.6e-11, left 1.5e-11;
    // complex 256^2: 1.4e-10 -> 1.8e-12).  The verification sweep is therefore skipped only from 1e-12 on, which leaves
    // <= 2e-13 either way (separated spectra arrive there from ~1e-6 in one sweep: 7e-13, 1e-13, 3e-14 measured).
    if (mx <= SVD_EXIT_COS) break;
  }
  if (s2 != s) {                            // join: everything below runs on s and reads V
    if ((e = hipStreamSynchronize(s2)) != hipSuccess) { drop_events(); return e; }
  }
  drop_events();
  if (sweeps_out) *sweeps_out = sweeps;
  if (!(mx_last <= 1.0e-9)) {               // 40 sweeps without reaching the quadratic regime: the factors would not be isometries
    if (err) {
      char buf[160];
      snprintf(buf, sizeof(buf), "block-Jacobi SVD did not converge: max |cos| = %.3e after %d sweeps", mx_last, sweeps);
      *err = buf;
    }
    return hipErrorNotReady;
  }
  if (getenv("MPSK_SVD_DEBUG")) fprintf(stderr, "[mpsk_tsvd] %d x %d: P=%d Q=%d rounds/sweep=%d sweeps=%d chains=%d inner=%d\n", mm, nn, P, Q, rounds, sweeps, NC, inner_sweeps);
  // singular values, sorting, truncation (host)
  hipLaunchKernelGGL(colnorm2_kernel, dim3(npad), dim3(256), 0, s, G[cur], mm, mm, sigma2);
  std::vector<double> hs(npad);
  if ((e = hipMemcpyAsync(hs.data(), sigma2, sizeof(double) * npad, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
  std::vector<int> perm(npad);
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return hs[a] > hs[b]; });
  std::vector<double> sv(kmax), sc(kmax);
  double tot2 = 0.0;
  for (int i = 0; i < kmax; ++i) { sv[i] = std::sqrt(std::max(hs[perm[i]], 0.0)); tot2 += sv[i] * sv[i]; }
  int k = kmax;
  if (max_keep > 0 && max_keep < k) k = max_keep;
  if (trunc_err > 0.0) {
    // drop the tail while ||dropped||_2 <= trunc_err, an ABSOLUTE bound (TensorKit 0.12 `truncerr(eps)`, p = 2: its
    // _truncate! compares the p-norm of the discarded values with eps itself.  TensorKit is not vendored in the reference
    // tree, so this is restated from the published source: "parity unpinned", include/mpsk.h).  The two-site drivers
    // normalise theta before the split (eigenvectors; unitary real-time steps), where absolute == relative.
    double tail2 = 0.0;
    for (int i = k; i < kmax; ++i) tail2 += sv[i] * sv[i];
    while (k > 1 && tail2 + sv[k - 1] * sv[k - 1] <= trunc_err * trunc_err) { tail2 += sv[k - 1] * sv[k - 1]; --k; }
    (void)tot2;
  }
  double disc2 = 0.0;
  for (int i = k; i < kmax; ++i) disc2 += sv[i] * sv[i];
  *kept = k;
  *disc_norm = std::sqrt(disc2);
  for (int i = 0; i < kmax; ++i) sc[i] = sv[i] > 0.0 ? 1.0 / sv[i] : 0.0;
  if ((e = hipMemcpyAsync(d_perm, perm.data(), sizeof(int) * kmax, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(scale, sc.data(), sizeof(double) * kmax, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(S, sv.data(), sizeof(double) * kmax, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  if (vfree) {
    hipLaunchKernelGGL(gather_cols_kernel, dim3(1024), dim3(256), 0, s, G[cur], mm, nn, d_perm, scale, kmax, U, ldu, 0);
  } else if (Qpre) {
    double* Vp = G[cur ^ 1];              // the idle ping-pong buffer holds W[:, perm]  (n x kmax)
    hipLaunchKernelGGL(gather_cols_kernel, dim3(1024), dim3(256), 0, s, V[cur], nn, nn, d_perm, (const double*)nullptr,
                       kmax, Vp, nn, 0);
    GemmArgs g;
    std::memset(&g, 0, sizeof(g));
    g.batch = 1; g.nseg = 1; g.alpha = 1.0; g.beta = 0.0; g.K = nn;
    if (!outer_transposed) {              // U = Qpre W_p ; Vh = (G_p Sigma^-1)^T
      g.A = Qpre; g.lda = ldq; g.B = Vp; g.ldb = nn; g.C = U; g.ldc = ldu; g.M = q_rows; g.N = kmax;
      if ((e = gemm_f64(g, s)) != hipSuccess) return e;
      hipLaunchKernelGGL(gather_cols_kernel, dim3(1024), dim3(256), 0, s, G[cur], mm, nn, d_perm, scale, kmax, Vh, ldv, 1);
    } else {                              // U = G_p Sigma^-1 ; Vh = (Qpre W_p)^T = W_p^T Qpre^T
      hipLaunchKernelGGL(gather_cols_kernel, dim3(1024), dim3(256), 0, s, G[cur], mm, nn, d_perm, scale, kmax, U, ldu, 0);
      g.A = Vp; g.lda = nn; g.transA = 1; g.B = Qpre; g.ldb = ldq; g.transB = 1; g.C = Vh; g.ldc = ldv;
      g.M = kmax; g.N = q_rows;
      if ((e = gemm_f64(g, s)) != hipSuccess) return e;
    }
  } else if (!pl.transposed) {
    hipLaunchKernelGGL(gather_cols_kernel, dim3(1024), dim3(256), 0, s, G[cur], mm, m, d_perm, scale, kmax, U, ldu, 0);
    hipLaunchKernelGGL(gather_cols_kernel, dim3(1024), dim3(256), 0, s, V[cur], nn, n, d_perm, (const double*)nullptr,
                       kmax, Vh, ldv, 1);
  } else {   // theta^T = G V^T  ->  theta = V (G)^T :  U = V-part, Vh = (G diag(1/sigma))^T
    hipLaunchKernelGGL(gather_cols_kernel, dim3(1024), dim3(256), 0, s, V[cur], nn, m, d_perm, (const double*)nullptr,
                       kmax, U, ldu, 0);
    hipLaunchKernelGGL(gather_cols_kernel, dim3(1024), dim3(256), 0, s, G[cur], mm, n, d_perm, scale, kmax, Vh, ldv, 1);
  }
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;   // perm/sc/sv are host temporaries
  return hipGetLastError();
}

// ==== complex128 (mpsk_tsvd under MPSK_C128) ============================================================================
// The same one-sided block Jacobi on interleaved complex storage, with J2 = 64 COMPLEX columns per pair.  A complex m x n
// matrix is the real 2m x n matrix whose row pairs hold (re, im) (the "half-embedded" view of mpsk_internal.h), so with
// X_p the 2m x 64 half view of pair p:
//   Gram    Re(X_p^H X_p) = X_p^T X_p,   Im(X_p^H X_p) = (J X_p)^T X_p   -- two batched TN launches of the complex GEMM
//           family (segJ = 0 / 1), each writing one plane of the interleaved Gram matrix (c_rs = 2)
//   eig     M_p = W_p L W_p^H   -- cyclic two-sided Jacobi with complex rotations, M and W in LDS (cjacobi_eig_kernel)
//   update  X_p <- X_p W_p = X_p Wr + (J X_p) Wi   -- one launch, two K-segments, W planar
// The tournament, tables, tolerance and sweep logic are those of the real solver with 2m real rows; only the unchained,
// single-stream order exists here.
//
// Rotation of the column pair (p, q), g = M_pq = |g| e^{i phi}:  the real Hestenes rotation (c, s) of the 2 x 2 problem
// [[a, |g|], [|g|, b]] and sigma = s e^{i phi};  J = [[c, sigma], [-conj(sigma), c]], X <- X J, M <- J^H M J.
// LDS: M and W, two planes each, rows padded to 65: 4 x 64 x 65 x 8 B = 130 KB -> one workgroup per CU.  A call has
// P = n / 64 <= 256 pairs for n <= 16384, never more workgroups than CUs, so the occupancy costs nothing.
__global__ __launch_bounds__(256) void cjacobi_eig_kernel(const double* __restrict__ Mpart, int Q, double* __restrict__ Wout,
                                                          double tol, unsigned long long* __restrict__ flag, int inner_sweeps) {
  __shared__ double Mr[J2][J2 + 1], Mi[J2][J2 + 1];    // M[i][j] = X_i^H X_j
  __shared__ double Wr[J2][J2 + 1], Wi[J2][J2 + 1];
  __shared__ double red[4];
  __shared__ int any_rot;
  const int tid = threadIdx.x;
  const int p = blockIdx.x;
  const size_t psz = (size_t)2 * J2 * J2;              // one interleaved (Gram) or planar (W) complex 64 x 64 matrix
  const double* Mp = Mpart + (size_t)p * Q * psz;
  for (int e = tid; e < 2 * J2 * J2; e += 256) {       // sum of the Q K-split partial Gram matrices (interleaved)
    double acc = 0.0;
    for (int q = 0; q < Q; ++q) acc += Mp[(size_t)q * psz + e];
    const int ij = e >> 1, i = ij % J2, j = ij / J2;
    if (e & 1) Mi[i][j] = acc; else Mr[i][j] = acc;
  }
  __syncthreads();
  // Hermitian part + convergence measure max |g_ij|^2 / (g_ii g_jj); the thread that owns (i, j), i < j, also owns (j, i)
  double mx = 0.0;
  for (int e = tid; e < J2 * J2; e += 256) {
    const int i = e % J2, j = e / J2;
    if (i < j) {
      const double ar = 0.5 * (Mr[i][j] + Mr[j][i]), ai = 0.5 * (Mi[i][j] - Mi[j][i]);
      const double dd = Mr[i][i] * Mr[j][j], g2 = ar * ar + ai * ai;
      mx = fmax(mx, g2 == 0.0 ? 0.0 : (dd > 0.0 ? g2 / dd : 1.0));
      Mr[i][j] = ar; Mi[i][j] = ai;
      Mr[j][i] = ar; Mi[j][i] = -ai;
    } else if (i == j) {
      Mi[i][i] = 0.0;
    }
  }
  for (int off = 32; off > 0; off >>= 1) mx = fmax(mx, __shfl_xor(mx, off, 64));
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  mx = sqrt(fmax(fmax(red[0], red[1]), fmax(red[2], red[3])));
  if (tid == 0) atomicMax(flag, (unsigned long long)__double_as_longlong(mx));
  double* Wp = Wout + (size_t)p * psz;                 // planar: re plane [0, J2^2), im plane [J2^2, 2 J2^2)
  if (mx <= tol) {                                     // (uniform over the workgroup)
    for (int e = tid; e < J2 * J2; e += 256) {
      Wp[e] = (e % J2 == e / J2) ? 1.0 : 0.0;
      Wp[J2 * J2 + e] = 0.0;
    }
    return;
  }
  for (int e = tid; e < J2 * J2; e += 256) {
    const int i = e % J2, j = e / J2;
    Wr[i][j] = (i == j) ? 1.0 : 0.0;
    Wi[i][j] = 0.0;
  }
  __syncthreads();
  // 32 disjoint pairs per step (round robin over 64 indices, the pairing of jacobi_eig_kernel), 8 lanes per pair, two phases:
  //   A: rotation parameters from (M_pp, M_qq, M_pq), then columns p, q of M and W   (a team only touches its own columns)
  //   B: rows p, q of M                                                              (a team only touches its own rows)
  const int team = tid >> 3, pj = tid & 7;
  const int pk = ((team & 3) << 3) | (team >> 2);
  for (int sweep = 0; sweep < inner_sweeps; ++sweep) {
    if (tid == 0) any_rot = 0;
    __syncthreads();
    int rotated = 0;
    for (int st = 0; st < J2 - 1; ++st) {
      int pp, qq;
      if (pk == 0) { pp = J2 - 1; qq = st; }
      else { pp = (st + pk) % (J2 - 1); qq = (st + (J2 - 1) - pk) % (J2 - 1); }
      if (pp > qq) { const int t = pp; pp = qq; qq = t; }
      const double a = Mr[pp][pp], b = Mr[qq][qq], gr = Mr[pp][qq], gi = Mi[pp][qq];
      const double g2 = gr * gr + gi * gi;
      double c = 1.0, sr = 0.0, si = 0.0;              // sigma = sr + i si
      if (g2 > 1.0e-34 * a * b) {
        const double ag = sqrt(g2);
        const double zeta = (b - a) / (2.0 * ag);
        const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        c = 1.0 / sqrt(1.0 + t * t);
        const double sg = c * t / ag;
        sr = sg * gr;
        si = sg * gi;
        if (g2 > 1.0e-20 * a * b) rotated = 1;         // |cos| > 1e-10: another inner sweep is worth it
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {                    // x_p <- c x_p - conj(sigma) x_q ,  x_q <- sigma x_p + c x_q
        const int r = pj + 8 * i;
        const double mpr = Mr[r][pp], mpi = Mi[r][pp], mqr = Mr[r][qq], mqi = Mi[r][qq];
        const double wpr = Wr[r][pp], wpi = Wi[r][pp], wqr = Wr[r][qq], wqi = Wi[r][qq];
        Mr[r][pp] = c * mpr - (sr * mqr + si * mqi);
        Mi[r][pp] = c * mpi - (sr * mqi - si * mqr);
        Mr[r][qq] = (sr * mpr - si * mpi) + c * mqr;
        Mi[r][qq] = (sr * mpi + si * mpr) + c * mqi;
        Wr[r][pp] = c * wpr - (sr * wqr + si * wqi);
        Wi[r][pp] = c * wpi - (sr * wqi - si * wqr);
        Wr[r][qq] = (sr * wpr - si * wpi) + c * wqr;
        Wi[r][qq] = (sr * wpi + si * wpr) + c * wqi;
      }
      __syncthreads();
#pragma unroll
      for (int i = 0; i < 8; ++i) {                    // y_p <- c y_p - sigma y_q ,  y_q <- conj(sigma) y_p + c y_q
        const int j = pj + 8 * i;
        const double ypr = Mr[pp][j], ypi = Mi[pp][j], yqr = Mr[qq][j], yqi = Mi[qq][j];
        Mr[pp][j] = c * ypr - (sr * yqr - si * yqi);
        Mi[pp][j] = c * ypi - (sr * yqi + si * yqr);
        Mr[qq][j] = (sr * ypr + si * ypi) + c * yqr;
        Mi[qq][j] = (sr * ypi - si * ypr) + c * yqi;
      }
      __syncthreads();
    }
    if (rotated) any_rot = 1;
    __syncthreads();
    if (!any_rot) break;
    __syncthreads();
  }
  // one Newton-Schulz step  W <- W (3 I - W^H W) / 2  (unitarity drift of the accumulated rotations, see jacobi_eig_kernel);
  // T = W^H W goes to the M planes, which are no longer needed
  for (int e = tid; e < J2 * J2; e += 256) {
    const int i = e % J2, j = e / J2;
    double tr = 0.0, ti = 0.0;
    for (int k = 0; k < J2; ++k) {
      const double ar = Wr[k][i], ai = Wi[k][i], br = Wr[k][j], bi = Wi[k][j];
      tr += ar * br + ai * bi;
      ti += ar * bi - ai * br;
    }
    Mr[i][j] = tr; Mi[i][j] = ti;
  }
  __syncthreads();
  for (int e = tid; e < J2 * J2; e += 256) {
    const int i = e % J2, j = e / J2;
    double pr = 0.0, pi = 0.0;
    for (int k = 0; k < J2; ++k) {
      const double ar = Wr[i][k], ai = Wi[i][k], br = Mr[k][j], bi = Mi[k][j];
      pr += ar * br - ai * bi;
      pi += ar * bi + ai * br;
    }
    Wp[i + J2 * j] = 1.5 * Wr[i][j] - 0.5 * pr;
    Wp[J2 * J2 + i + J2 * j] = 1.5 * Wi[i][j] - 0.5 * pi;
  }
}

// G (mm x npad complex, interleaved) = theta or theta^H (ctrans), zero padded ; V (nn x npad complex) = [I 0].  ldt2: the
// leading dimension of theta in DOUBLES
__global__ __launch_bounds__(256) void csvd_init_kernel(const double* __restrict__ theta, int64_t ldt2, int mm, int nn, int ctrans,
                                                        double* __restrict__ G, int npad, double* __restrict__ V) {
  const int64_t tg = (int64_t)mm * npad, tv = (int64_t)nn * npad;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < tg + tv; e += (int64_t)gridDim.x * blockDim.x) {
    if (e < tg) {
      const int r = (int)(e % mm), c = (int)(e / mm);
      double re = 0.0, im = 0.0;
      if (c < nn) {
        if (ctrans) { re = theta[2 * c + ldt2 * r]; im = -theta[2 * c + 1 + ldt2 * r]; }
        else { re = theta[2 * r + ldt2 * c]; im = theta[2 * r + 1 + ldt2 * c]; }
      }
      G[2 * e] = re; G[2 * e + 1] = im;
    } else {
      const int64_t f = e - tg;
      const int r = (int)(f % nn), c = (int)(f / nn);
      V[2 * f] = (r == c) ? 1.0 : 0.0; V[2 * f + 1] = 0.0;
    }
  }
}

// column i of the result = column perm[i] (i when perm is null) of the complex src (rows x ., lds complex) times scale[i]:
//   mode 0  out (rows x k) interleaved, ldo complex       mode 1  out (k x rows) = its conjugate transpose, ldo complex
//   mode 2  out (rows x k) planar: re plane at out, im plane at out + plane, ldo real
__global__ __launch_bounds__(256) void cgather_kernel(const double* __restrict__ src, int64_t lds, int rows,
                                                      const int* __restrict__ perm, const double* __restrict__ scale, int k,
                                                      double* __restrict__ out, int64_t ldo, int mode, int64_t plane) {
  const int64_t total = (int64_t)rows * k;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(e % rows), i = (int)(e / rows);
    const double* sp = src + 2 * (r + lds * (perm ? perm[i] : i));
    double re = sp[0], im = sp[1];
    if (scale) { re *= scale[i]; im *= scale[i]; }
    if (mode == 0) { out[2 * (r + ldo * i)] = re; out[2 * (r + ldo * i) + 1] = im; }
    else if (mode == 1) { out[2 * (i + ldo * r)] = re; out[2 * (i + ldo * r) + 1] = -im; }
    else { out[r + ldo * i] = re; out[plane + r + ldo * i] = im; }
  }
}

struct CSvdPlan {
  int mm, nn, npad, P, Q, kq, transposed;    // kq: REAL rows (2 mm / Q) per K-split of the Gram product
  size_t y_doubles, bytes;
};

static CSvdPlan csvd_plan(int m, int n, int q_rows) {
  CSvdPlan p;
  p.transposed = (m < n);
  p.mm = p.transposed ? n : m;
  p.nn = p.transposed ? m : n;
  p.npad = ((p.nn + J2 - 1) / J2) * J2;
  p.P = p.npad / J2;
  const int mr = 2 * p.mm;
  int target = 1024 / p.P;
  if (target < 1) target = 1;
  if (target > 16) target = 16;
  int q = 1;                                 // largest divisor of 2 mm <= target with >= 128 (even) real rows per split
  for (int c = target; c >= 2; --c)
    if (mr % c == 0 && (mr / c) % 2 == 0 && mr / c >= 128) { q = c; break; }
  p.Q = q;
  p.kq = mr / q;
  const size_t w = (size_t)2 * J2 * J2;
  p.y_doubles = (size_t)2 * q_rows * p.nn;   // QR-preconditioned, wide: Qpre W before its conjugate transpose
  const size_t d = (size_t)2 * (2 * (size_t)p.mm * p.npad) + (size_t)2 * (2 * (size_t)p.nn * p.npad) + (size_t)p.P * p.Q * w +
                   (size_t)p.P * w + (size_t)2 * p.npad + p.y_doubles + 64;
  const size_t tabs = (size_t)(2 * (size_t)p.P * p.Q + 10 * (size_t)p.P) * sizeof(int64_t) + 256;
  p.bytes = d * sizeof(double) + tabs + (size_t)p.npad * sizeof(int);
  return p;
}

size_t tsvd_c128_workspace_bytes(int m, int n, int q_rows) { return csvd_plan(m, n, q_rows).bytes; }

// Host-synchronising complex truncated SVD (include/mpsk.h, mpsk_tsvd under MPSK_C128).  Every matrix is interleaved complex,
// leading dimensions in complex elements; S real.  Qpre != nullptr: QR-preconditioned mode as in tsvd(): the caller factored
// the tall orientation A' (q_rows x n) = Qpre R and passes theta := R (n x n); Jacobi runs on R^H:
//   R^H V = G  =>  A' = (Qpre V) Sigma (G Sigma^-1)^H ;  outer_transposed: A' = theta^H.
hipError_t tsvd_c128(int m, int n, const double* theta, int ldt, double* U, int ldu, double* S, double* Vh, int ldv,
                     int max_keep, double trunc_err, int* kept, double* disc_norm, void* ws, hipStream_t s,
                     std::string* err, int* sweeps_out, const double* Qpre, int ldq, int q_rows, int outer_transposed) {
  const CSvdPlan pl = csvd_plan(m, n, Qpre ? q_rows : 0);
  int ctrans = pl.transposed;
  if (Qpre) {
    if (m != n) return hipErrorInvalidValue;
    ctrans = 1;                                // G <- R^H
  }
  const int mm = pl.mm, nn = pl.nn, npad = pl.npad, P = pl.P, Q = pl.Q, kq = pl.kq;
  const int mr = 2 * mm, nr = 2 * nn;          // real rows of G and V
  const int kmax = std::min(m, n);
  const size_t wsz = (size_t)2 * J2 * J2;
  double* G[2]; double* V[2];
  double* base = (double*)ws;
  G[0] = base; G[1] = G[0] + (size_t)mr * npad;
  V[0] = G[1] + (size_t)mr * npad; V[1] = V[0] + (size_t)nr * npad;
  double* Mpart = V[1] + (size_t)nr * npad;
  double* Wb = Mpart + (size_t)P * Q * wsz;    // one stream: round r's update has read W before round r + 1's eig writes it
  double* sigma2 = Wb + (size_t)P * wsz;
  double* scale = sigma2 + npad;
  double* Y = scale + npad;
  unsigned long long* flag = (unsigned long long*)(Y + pl.y_doubles);
  int64_t* tabs = (int64_t*)(flag + 8);
  int64_t* t_gramA = tabs;
  int64_t* t_gramC = t_gramA + (size_t)P * Q;
  int64_t* t_updA_G = t_gramC + (size_t)P * Q;
  int64_t* t_updA_V = t_updA_G + 2 * P;
  int64_t* t_updB = t_updA_V + 2 * P;
  int64_t* t_updC_G = t_updB + 2 * P;
  int64_t* t_updC_V = t_updC_G + 2 * P;
  int* d_perm = (int*)(t_updC_V + 2 * P);
  auto dest_slot = [&](int p, int half) -> int {   // the round robin of tsvd()
    if (P == 1) return half;
    if (half == 0) {
      if (p == 0) return 0;
      if (p + 1 <= P - 1) return 2 * (p + 1);
      return 2 * (P - 1) + 1;
    }
    if (p == 0) return 2 * 1;
    return 2 * (p - 1) + 1;
  };
  std::vector<int64_t> h((size_t)2 * P * Q + 10 * P, 0);
  int64_t* hgA = h.data(); int64_t* hgC = hgA + (size_t)P * Q;
  int64_t* huAG = hgC + (size_t)P * Q; int64_t* huAV = huAG + 2 * P; int64_t* huB = huAV + 2 * P;
  int64_t* huCG = huB + 2 * P; int64_t* huCV = huCG + 2 * P;
  for (int p = 0; p < P; ++p) {
    for (int q = 0; q < Q; ++q) {
      hgA[p * Q + q] = (int64_t)p * J2 * mr + (int64_t)q * kq;
      hgC[p * Q + q] = ((int64_t)p * Q + q) * (int64_t)wsz;
    }
    huAG[p] = (int64_t)p * J2 * mr;
    huAV[p] = (int64_t)p * J2 * nr;
    huB[p] = (int64_t)p * (int64_t)wsz;
    huCG[p] = (int64_t)dest_slot(p, 0) * JB * mr;
    huCG[P + p] = (int64_t)dest_slot(p, 1) * JB * mr;
    huCV[p] = (int64_t)dest_slot(p, 0) * JB * nr;
    huCV[P + p] = (int64_t)dest_slot(p, 1) * JB * nr;
  }
  hipError_t e;
  if ((e = hipMemcpyAsync(tabs, h.data(), h.size() * sizeof(int64_t), hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  hipLaunchKernelGGL(csvd_init_kernel, dim3(2048), dim3(256), 0, s, theta, (int64_t)2 * ldt, mm, nn, ctrans, G[0], npad, V[0]);
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;   // h is a host temporary

  const double tol = std::sqrt((double)mm) * 2.220446049250313e-16;
  const int inner_sweeps = (P == 1) ? 15 : 1;     // a single pair has no tournament: the full inner iteration
  const int rounds = (P == 1) ? 1 : 2 * P - 1;
  int cur = 0, sweeps = 0;
  unsigned long long hflag = 0;
  double mx_last = 0.0;
  for (int sweep = 0; sweep < 40; ++sweep) {
    if ((e = hipMemsetAsync(flag, 0, sizeof(unsigned long long), s)) != hipSuccess) return e;
    for (int r = 0; r < rounds; ++r) {
      for (int al = 0; al < 2; ++al) {             // 1. Gram planes: Re = X^T X, Im = (J X)^T X, K split over Q
        GemmArgs g;
        std::memset(&g, 0, sizeof(g));
        g.A = G[cur]; g.B = G[cur]; g.C = Mpart + al; g.M = J2; g.N = J2; g.K = kq; g.lda = mr; g.ldb = mr; g.ldc = 2 * J2;
        g.batch = P * Q; g.nseg = 1; g.alpha = 1.0; g.beta = 0.0; g.transA = 1; g.transB = 0;
        g.tabA = t_gramA; g.tabB = t_gramA; g.tabC = t_gramC; g.tabs_even = 1;
        g.cplx = 1; g.c_rs = 2; g.segJ[0] = (signed char)al;
        if ((e = gemm_f64(g, s)) != hipSuccess) return e;
      }
      hipLaunchKernelGGL(cjacobi_eig_kernel, dim3(P), dim3(256), 0, s, Mpart, Q, Wb, tol, flag, inner_sweeps);   // 2.
      GemmArgs u;                                  // 3. X <- X Wr + (J X) Wi into next round's slots, G then V
      std::memset(&u, 0, sizeof(u));
      u.B = Wb; u.N = J2; u.K = J2; u.ldb = J2; u.batch = P; u.nseg = 2; u.segB[1] = (int64_t)J2 * J2; u.segJ[1] = 1;
      u.alpha = 1.0; u.beta = 0.0; u.tabB = t_updB; u.tabs_even = 1; u.splitN = JB; u.cplx = 1;
      u.A = G[cur]; u.C = G[cur ^ 1]; u.M = mr; u.lda = mr; u.ldc = mr; u.tabA = t_updA_G; u.tabC = t_updC_G; u.tabC2 = t_updC_G + P;
      if ((e = gemm_f64(u, s)) != hipSuccess) return e;
      u.A = V[cur]; u.C = V[cur ^ 1]; u.M = nr; u.lda = nr; u.ldc = nr; u.tabA = t_updA_V; u.tabC = t_updC_V; u.tabC2 = t_updC_V + P;
      if ((e = gemm_f64(u, s)) != hipSuccess) return e;
      cur ^= 1;
    }
    ++sweeps;
    if ((e = hipMemcpyAsync(&hflag, flag, sizeof(hflag), hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
    double mx;
    std::memcpy(&mx, &hflag, sizeof(double));
    if (getenv("MPSK_SVD_DEBUG")) fprintf(stderr, "[mpsk_tsvd c128] sweep %d: max |cos| = %.3e (tol %.1e)\n", sweeps, mx, tol);
    mx_last = mx;
    if (mx <= tol || mx <= SVD_EXIT_COS) break;    // (quadratic convergence and its limit inside clusters: see tsvd())
  }
  if (sweeps_out) *sweeps_out = sweeps;
  if (!(mx_last <= 1.0e-9)) {
    if (err) {
      char buf[160];
      snprintf(buf, sizeof(buf), "complex block-Jacobi SVD did not converge: max |cos| = %.3e after %d sweeps", mx_last, sweeps);
      *err = buf;
    }
    return hipErrorNotReady;
  }
  if (getenv("MPSK_SVD_DEBUG")) fprintf(stderr, "[mpsk_tsvd c128] %d x %d: P=%d Q=%d rounds/sweep=%d sweeps=%d\n", mm, nn, P, Q, rounds, sweeps);
  hipLaunchKernelGGL(colnorm2_kernel, dim3(npad), dim3(256), 0, s, G[cur], mr, mr, sigma2);
  std::vector<double> hs(npad);
  if ((e = hipMemcpyAsync(hs.data(), sigma2, sizeof(double) * npad, hipMemcpyDeviceToHost, s)) != hipSuccess) return e;
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;
  std::vector<int> perm(npad);
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return hs[a] > hs[b]; });
  std::vector<double> sv(kmax), sc(kmax);
  for (int i = 0; i < kmax; ++i) sv[i] = std::sqrt(std::max(hs[perm[i]], 0.0));
  int k = kmax;                                    // truncation: exactly the fp64 rule (tsvd()), every value counted once
  if (max_keep > 0 && max_keep < k) k = max_keep;
  if (trunc_err > 0.0) {
    double tail2 = 0.0;
    for (int i = k; i < kmax; ++i) tail2 += sv[i] * sv[i];
    while (k > 1 && tail2 + sv[k - 1] * sv[k - 1] <= trunc_err * trunc_err) { tail2 += sv[k - 1] * sv[k - 1]; --k; }
  }
  double disc2 = 0.0;
  for (int i = k; i < kmax; ++i) disc2 += sv[i] * sv[i];
  *kept = k;
  *disc_norm = std::sqrt(disc2);
  for (int i = 0; i < kmax; ++i) sc[i] = sv[i] > 0.0 ? 1.0 / sv[i] : 0.0;
  if ((e = hipMemcpyAsync(d_perm, perm.data(), sizeof(int) * kmax, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(scale, sc.data(), sizeof(double) * kmax, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  if ((e = hipMemcpyAsync(S, sv.data(), sizeof(double) * kmax, hipMemcpyHostToDevice, s)) != hipSuccess) return e;
  const dim3 gg(1024), gb(256);
  if (Qpre) {
    double* Vp = G[cur ^ 1];                       // the idle ping-pong buffer: V[:, perm] planar (nn x kmax, two planes)
    const int64_t plane = (int64_t)nn * kmax;
    hipLaunchKernelGGL(cgather_kernel, gg, gb, 0, s, V[cur], (int64_t)nn, nn, d_perm, (const double*)nullptr, kmax, Vp,
                       (int64_t)nn, 2, plane);
    GemmArgs g;                                    // Qpre V_p: interleaved A, planar B
    std::memset(&g, 0, sizeof(g));
    g.A = Qpre; g.lda = (int64_t)2 * ldq; g.B = Vp; g.ldb = nn; g.M = 2 * q_rows; g.N = kmax; g.K = nn;
    g.batch = 1; g.nseg = 2; g.segB[1] = plane; g.segJ[1] = 1; g.alpha = 1.0; g.beta = 0.0; g.cplx = 1;
    if (!outer_transposed) {                       // U = Qpre V_p ;  Vh = (G_p Sigma^-1)^H
      g.C = U; g.ldc = (int64_t)2 * ldu;
      if ((e = gemm_f64(g, s)) != hipSuccess) return e;
      hipLaunchKernelGGL(cgather_kernel, gg, gb, 0, s, G[cur], (int64_t)mm, nn, d_perm, scale, kmax, Vh, (int64_t)ldv, 1, (int64_t)0);
    } else {                                       // U = G_p Sigma^-1 ;  Vh = (Qpre V_p)^H
      g.C = Y; g.ldc = (int64_t)2 * q_rows;
      if ((e = gemm_f64(g, s)) != hipSuccess) return e;
      hipLaunchKernelGGL(cgather_kernel, gg, gb, 0, s, G[cur], (int64_t)mm, nn, d_perm, scale, kmax, U, (int64_t)ldu, 0, (int64_t)0);
      hipLaunchKernelGGL(cgather_kernel, gg, gb, 0, s, (const double*)Y, (int64_t)q_rows, q_rows, (const int*)nullptr,
                         (const double*)nullptr, kmax, Vh, (int64_t)ldv, 1, (int64_t)0);
    }
  } else if (!pl.transposed) {                     // theta = G V^H:  U = G_p Sigma^-1, Vh = V_p^H
    hipLaunchKernelGGL(cgather_kernel, gg, gb, 0, s, G[cur], (int64_t)mm, m, d_perm, scale, kmax, U, (int64_t)ldu, 0, (int64_t)0);
    hipLaunchKernelGGL(cgather_kernel, gg, gb, 0, s, V[cur], (int64_t)nn, n, d_perm, (const double*)nullptr, kmax, Vh, (int64_t)ldv, 1,
                       (int64_t)0);
  } else {                                         // theta^H = G V^H:  U = V_p, Vh = (G_p Sigma^-1)^H
    hipLaunchKernelGGL(cgather_kernel, gg, gb, 0, s, V[cur], (int64_t)nn, m, d_perm, (const double*)nullptr, kmax, U, (int64_t)ldu, 0,
                       (int64_t)0);
    hipLaunchKernelGGL(cgather_kernel, gg, gb, 0, s, G[cur], (int64_t)mm, n, d_perm, scale, kmax, Vh, (int64_t)ldv, 1, (int64_t)0);
  }
  if ((e = hipStreamSynchronize(s)) != hipSuccess) return e;   // perm / sc / sv are host temporaries
  return hipGetLastError();
}

}  // namespace mpsk
