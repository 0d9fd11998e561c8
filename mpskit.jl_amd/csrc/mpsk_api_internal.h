// Private declarations shared by the units of the C ABI (not part of it, not seen by the kernel units):
//   mpsk_api.hip         context, slices, every contraction entry point
//   mpsk_api_factor.hip  QR / LQ, SVD and two-site split entries, complement SVD
//   mpsk_api_vec.hip     GEMM wrappers and the vector protocol
// The handle types behind include/mpsk.h, the two owner types of their device resources, and the few helpers that cross
// a unit boundary.  Helpers and owner types sit in hidden-visibility blocks: they are no exports of libmpsk.so.
#pragma once
#include <hip/hip_runtime.h>
#include <array>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>
#include "mpsk.h"
#include "mpsk_internal.h"

using namespace mpsk;

// kernels of mpsk_api_factor.hip that mpsk_api_vec.hip launches too (gemm_c128)
extern "C" {
__global__ __launch_bounds__(256) void cx_embed_kernel(const double* __restrict__ H, int64_t ldh, int m, int n,
                                                       double* __restrict__ E, int64_t lde);
__global__ __launch_bounds__(256) void cx_ctranspose_kernel(const double* __restrict__ in, int64_t ldi, int m, int n,
                                                            double* __restrict__ out, int64_t ldo);
}

#pragma GCC visibility push(hidden)

int fail(int code, const std::string& msg);      // records the text mpsk_last_error returns (mpsk_api.hip); returns code
#define HIPCHK(expr)                                                                        \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(MPSK_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));         \
  } while (0)
#define REQUIRE(cond, msg)                                                  \
  do {                                                                      \
    if (!(cond)) return fail(MPSK_ERR_INVALID, std::string(__func__) + ": " + (msg)); \
  } while (0)

// Growable device buffer.  reserve() is the only place that grows one and the destructor the only one that frees it.
struct DevScratch {
  void* p = nullptr;
  size_t bytes = 0;
  DevScratch() = default;
  DevScratch(const DevScratch&) = delete;
  ~DevScratch() { if (p) (void)hipFree(p); }
  double* d() const { return (double*)p; }
  // At least `want` bytes.  Growing drops the contents: `streams` are the streams whose enqueued work may still use the old
  // buffer, drained before it is freed.  `nomem` is the MPSK_ERR_NOMEM text (callers match on it).
  template <class... Streams> int reserve(size_t want, const char* nomem, Streams... streams) {
    if (want <= bytes) return MPSK_OK;
    for (hipStream_t s : {streams...}) HIPCHK(hipStreamSynchronize(s));
    if (p) HIPCHK(hipFree(p));
    p = nullptr; bytes = 0;
    if (hipMalloc(&p, want) != hipSuccess) return fail(MPSK_ERR_NOMEM, nomem);
    bytes = want;
    return MPSK_OK;
  }
};

// device copy of a host offset / segment table (mpsk_api.hip); DevTables::get is its only caller
int upload_table(const std::vector<int64_t>& h, const char* what, int64_t** out);

// Cache of device int64 tables, one per key of N shape numbers; the destructor frees every table.
template <size_t N> struct DevTables {
  std::map<std::array<int64_t, N>, int64_t*> tabs;
  DevTables() = default;
  DevTables(const DevTables&) = delete;
  ~DevTables() { for (auto& kv : tabs) (void)hipFree(kv.second); }
  // the table of `key`; on a miss build(h) fills the host vector, which is uploaded and kept
  template <class Build> int get(const std::array<int64_t, N>& key, Build build, const char* what, const int64_t** out) {
    auto it = tabs.find(key);
    if (it == tabs.end()) {
      std::vector<int64_t> h;
      build(h);
      int64_t* p = nullptr;
      if (int rc = upload_table(h, what, &p)) return rc;
      it = tabs.emplace(key, p).first;
    }
    *out = it->second;
    return MPSK_OK;
  }
};

#pragma GCC visibility pop

// Pair-Gram form of the interior levels of a canonical transfer (Jordan-form slice, dense O[Wl, d, d, Wr]).  The levels
// that receive from the identity level alone are combinations of a few D x D products of the site tensor with itself:
//   left   GLout[v] = sum_{t,s} O[0,t,s,v] P_ts,      P_ts = A[:,t,:]^T A[:,s,:],   P_st = P_ts^T,   v = 1 .. Wr-2, and the
//          D-block term of level Wr-1
//   right  GRout[w] = sum_{t,s} O[w,t,s,Wr-1] Q_st,   Q_st = A[:,s,:] A[:,t,:]^T,   Q_ts = Q_st^T,   w = 1 .. Wl-2
// Pair p = {i, j}, i <= j, stands for M_p = op(A_i) op(A_j) (left: P_ij, right: Q_ij); only pairs with a non-zero
// coefficient on some level are listed, the diagonal ones (symmetric M_p) first.  coef[l][p] = (direct, transposed):
//   left   level v = 1 + l:  (O[0,i,j,v], O[0,j,i,v])          right  level w = 1 + l:  (O[w,j,i,Wr-1], O[w,i,j,Wr-1])
// with the transposed coefficient of a diagonal pair zero.  Host data only; d_coef is the slice's device copy.
struct PairPlan {
  int np = 0, ndiag = 0, nl = 0;
  std::vector<int> i, j;
  std::vector<double> coef;        // [nl][np][2]
  double* d_coef = nullptr;
};

struct mpsk_mposlice {
  mpsk_ctx* ctx;
  int Wl, Wr, d;
  int dtype = MPSK_F64;       // MPSK_C128: complex entries (Ofull_im), every operand of a call with this slice is complex128
  std::vector<double> Ofull;  // [Wl, d, d, Wr] column-major, index (w,t,s,v)
  std::vector<double> Ofull_im;
  MixPlan fwd;                // (w,s) -> (v,t)   in = s + d*w, out = t + d*v
  MixPlan bwd;                // (v,t) -> (w,s)   in = t + d*v, out = s + d*w
  MixPlan rgt;                // (v,s) -> (w,t)   in = s + d*v, out = t + d*w   (complex transfer_right: A GR first, then Ab^H)
  double Oi(int w, int t, int s, int v) const {
    return Ofull_im.empty() ? 0.0 : Ofull_im[w + (size_t)Wl * (t + d * (s + (size_t)d * v))];
  }
  std::vector<char> row_used, col_used;
  // "right-combined" form of the matvec (mpsk_hac): the MPO tensor is folded into the right environment once per
  // site visit,  GRc[c] = sum_v O[w_c, t_c, s_c, v] GR[v]  for every (w, s, t) with a non-zero entry, so that
  //   y[:, t, :] = sum_{c : t_c = t} T1[w_c][:, s_c, :] GRc[c]   needs no slab mix between the two GEMM stages.
  MixPlan rc;                      // out slab c <- in slab v
  std::vector<int> rc_w, rc_s, rc_t;
  int rc_nseg = 0;                 // max over t of the number of c with t_c = t (lists are padded to this length)
  // Jordan form (mpsk_hac mode 3, real slices): levels 0 and W-1 have chi = 1, O[0,0] = O[W-1,W-1] = 1 and
  // O[w,v] = 0 for every w > 0, v < W-1 (nothing enters level 0, nothing leaves level W-1, no A blocks).  With level 0
  // of GL and level W-1 of GR identities (canonical environments) the matvec is then
  //   y[:,t,:] = sum_s x[:,s,:] GRc0[(s,t)] + sum_s GLc[(s,t)] x[:,s,:],
  //   GRc0[(s,t)] = sum_v O[0,t,s,v] GR[v]   (start level + C blocks + D block),
  //   GLc[(s,t)]  = sum_{w>0} O[w,t,s,W-1] GL[w]   (B blocks + finished level).
  // Slab p = s + d t of both folds; jr_p / jl_p [d][nseg]: per t the slabs p with terms, padded to jr_nseg / jl_nseg
  // with an empty slab of the same family (the fold writes zeros there).
  bool jordan = false;
  MixPlan jr, jl;                  // out slab p <- in slab v of GR / w of GL
  std::vector<int> jr_p, jl_p;
  int jr_nseg = 0, jl_nseg = 0;
  // canonical transfers (mpsk_transfer_left_ex / mpsk_transfer_right_ex on a Jordan-form slice): elementwise plans whose
  // only input is the site tensor, in slab s = A[:, s, :]
  //   tl: out slab t + d (v - 1) <- O[0,t,s,v]      v = 1 .. Wr-2 (C blocks), and v = Wr-1 (D block) when tl_dblock
  //   tr: out slab t + d (w - 1) <- O[w,t,s,Wr-1]   w = 1 .. Wl-2 (B blocks)
  // jtabL / jtabR: device segment tables [2][d][nseg] of the fold application (A offsets, B offsets), one per shape seen
  MixPlan tl, tr;
  bool tl_dblock = false;
  mutable DevTables<1> jtabL;      // key Dl
  mutable DevTables<2> jtabR;      // key (Dl, Dr)
  // pair-Gram route of the canonical transfers (PairPlan below): pl for transfer_left, pr for transfer_right; ptabL /
  // ptabR: device offset tables [2][np] of the pair batch (first operand i Dl, second operand j Dl), key Dl
  PairPlan pl, pr;
  mutable DevTables<1> ptabL, ptabR;
  double O(int w, int t, int s, int v) const { return Ofull[w + (size_t)Wl * (t + d * (s + (size_t)d * v))]; }
  // dense slice (mpsk_mposlice_create_dense): stage 2 of dAC / the transfers is the fp64 GEMM
  //   T2[:, (t,v)] = T1[:, (s,w)] Od[(s,w), (t,v)]  on intermediates whose K index (s,w) has ONE stride;
  // Od = O as a column-major [d Wl, d Wr] matrix, device-resident.  dtab: per-batch offset tables of the (s,w)-batched
  // stage 1 ([2][Wl d]: A offset w P, B offset s Q), one per (P, Q) seen, built on first use.
  bool dense = false;
  double* d_Od = nullptr;
  mutable DevTables<2> dtab;       // key (P, Q)
  // right half of mpsk_dAC2_product: OdR = O as a column-major [d Wr, d Wl] matrix, rows (s,v), columns (t,w) (the physical
  // input and the RIGHT MPO leg are contracted, the left leg stays open); dtabR: stage-1 offset tables [2][Wr d] for
  // z = s + d v (A offset s P into the site tensor, B offset v Q into the right environment)
  double* d_OdR = nullptr;
  mutable DevTables<2> dtabR;
};

struct PoolBuf { void* p; size_t bytes; bool used; hipStream_t last = nullptr; hipEvent_t ev = nullptr; bool ev_set = false; };

struct mpsk_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  // workspace of the entry points (Ws below).  mpsk_ctx_workspace_reserve / ensure_ws refuse to grow it inside a side-stream
  // section or under a deferred factorization, and every other user enqueues on `stream` or on chains that have joined
  // it again: draining `stream` is enough
  DevScratch ws;
  double* d_scal = nullptr;     // [MAXK] device scalars
  double* d_partial = nullptr;  // dot scratch
  double* h_scal = nullptr;     // pinned host mirror
  double* d_coef = nullptr;     // [MAXK] coefficients of mpsk_vlincomb + their pinned source + the event that frees it
  double* h_coef = nullptr;
  hipEvent_t ev_coef = nullptr;
  bool coef_pending = false;
  int dtype = MPSK_F64;         // scalar type of the slice-less entry points (mpsk_ctx_set_dtype)
  int last_svd_sweeps = 0;
  int split_skip = 0, split_backoff = 0;           // calls that skip the stage after it gave up
  // subspace iterations the next truncation-aware mpsk_tsplit of the same (min(m, n), r) starts with: what the last one needed
  // (the bonds near the ends of a chain have other shapes and other spectra than the bulk; 8 for a shape not seen yet)
  std::map<std::pair<int, int>, int> split_q_hint;
  int last_split_iters = 0, last_split_path = 0;   // path: 0 full iteration (mode <= 2 / not applicable), 1 subspace stage, 2 stage gave up -> full
  double last_split_resid = 0.0;
  int svd_precondition = 3;     // mpsk_ctx_set_svd_mode: 0 plain, 1 QR-preconditioned, 2 QR + QR of R^T (mpsk_tsplit V-free, mpsk_tsvd with accumulated rotations), 3 = 2 + truncation-aware mpsk_tsplit
  int qr_mode = 0;              // 0 auto (CholeskyQR3 + Householder fallback), 1 Householder, 2 CholeskyQR3 only
  int* d_flag = nullptr;
  long n_qr_chol = 0, n_qr_house = 0, n_qr_fallback = 0, n_qr_robust = 0, n_qr_retry = 0;
  // first attempt of CholeskyQR3 with shift = qr_shift_fast * (bound of Fukaya et al.); a flagged breakdown repeats it with the bound
  double qr_shift_fast = getenv("MPSK_CQ_SHIFT_SCALE") ? atof(getenv("MPSK_CQ_SHIFT_SCALE")) : 1.0e-8;
  // second stream + workspace for two concurrent factorizations (mpsk_qrpos2)
  hipStream_t stream2 = nullptr;
  hipStream_t xstreams[3] = {nullptr, nullptr, nullptr};   // {stream2, two more}: chains of the block-Jacobi schedule (mpsk_svd.hip)
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  DevScratch ws2;               // workspace of the second factorization of mpsk_qrpos2: only stream2 ever works in it
  // transposed operands of mpsk_qrlq_pair, operands of mpsk_tsplit: written on `stream`; the second stream of mpsk_qrpos2
  // reads the transposed operand and writes its factors here, so both streams are drained before it grows
  DevScratch ws3;
  // scratch: complex gauge steps (embedded operands; conjugate transposes; split), rescaled theta.  Filled and read by
  // launches on `stream` alone (cx_scratch)
  DevScratch cxws[4];
  int* h_flags = nullptr;       // pinned [2]
  // deferred completion of a CholeskyQR gauge step (mpsk_ctx_qr_defer / mpsk_qr_commit): the launches are enqueued, the
  // success flag is read (and a fallback run) only at commit -- the caller fills the gap with work that does not need c->ws
  struct PendingQR {
    int active = 0;               // 0 none, 1 qrpos2, 2 lqpos
    int m = 0, n = 0;
    const void *A1 = nullptr, *A2 = nullptr; void *Q1 = nullptr, *R1 = nullptr, *Q2 = nullptr, *R2 = nullptr;
    int lda1 = 0, ldq1 = 0, ldr1 = 0, lda2 = 0, ldq2 = 0, ldr2 = 0;
    double *At = nullptr, *Qt = nullptr, *Rt = nullptr, *ws = nullptr;   // lqpos: transposed problem in c->ws
    void *L = nullptr, *Qo = nullptr; int ldl = 0, ldqo = 0;
  } pend;
  bool defer_next = false;
  bool on_side = false;         // mpsk_ctx_side_begin .. mpsk_ctx_side_end: `stream` and `stream2` are swapped
  std::map<std::pair<const mpsk_mposlice*, const mpsk_mposlice*>, MixPlan> pair_plans;
  std::vector<PoolBuf> pool;    // device buffers of prepared operators (mpsk_hac), reused across site visits
  // bond expansion (mpsk_dAC2_product / mpsk_complement_tsvd): batch offset tables of the K = Wm Dm product keyed by their
  // strides; operands of the complement SVD in a buffer of their own (the factorizations inside size and use c->ws
  // themselves); calls / calls answered by the accepted subspace stage / all other calls (full iteration, small X, X = 0)
  DevTables<6> prod_tabs;
  DevScratch exws;              // used on `stream` alone (ex_scratch)
  long n_compl = 0, n_compl_sub = 0, n_compl_full = 0;
  long n_transfer_pair = 0;     // canonical transfers that took the pair-Gram route (mpsk_ctx_transfer_stats)
  __attribute__((visibility("hidden"))) ~mpsk_ctx() = default;      // (frees the owners above; out of line, and no export)
};

// prepared effective Hamiltonian of one site (MPO_ddAC of derivatives.jl:11-15: built once, applied by every Krylov step)
struct mpsk_hac {
  mpsk_ctx* ctx;
  const mpsk_mposlice* H;
  int Dlo, Dl, Dr;
  const double* GL;
  const double* GR;
  int mode;                     // 0: GEMM -> slab mix -> GEMM (mpsk_dAC);  1: right-combined environment, no mix;
                                // 2: complex128;  3: Jordan form on canonical environments (one GEMM, no intermediate)
  double* GRc = nullptr;        // mode 1: [nc + 1][Dr, Dr] (last slab: zeros, pads the shorter segment lists)
                                // mode 3: GRc0, per t a [Dr, d, Dr] tensor (slab (s, t) = its plane s)
  double* GLc = nullptr;        // mode 3: per t a [Dlo, d, Dl] tensor (slab (s, t) = its plane s)
  int launches = 1;             // mode 3: 1 = both families in one launch (Dl == Dr), 2 = x GRc0, then GLc x with beta = 1
  int64_t* zseg = nullptr;      // device [2][d][nseg]: A offsets (into T1), B offsets (into GRc); mode 3: see hac_jordan_prepare
  std::vector<int64_t> zseg_host;   // source of the asynchronous upload of zseg: lives as long as the handle (no sync)
  hipEvent_t ev_up = nullptr;       // completion of that upload (waited for before the handle is freed)
  int pool_idx = -1;
  // mode 3, MPSK_F64: segments per batch of the two families and their per-t slab lists [d][jn1] / [d][jn2] -- the slice's
  // own (jr_p / jl_p), or the union over the terms of a summed operator (mpsk_hsum)
  int jn1 = 0, jn2 = 0;
  const std::vector<int>* jp1 = nullptr;
  const std::vector<int>* jp2 = nullptr;
};
constexpr int MAXK = 256;
constexpr int MAXCOEF = 1024;   // coefficient staging: MAXK for mpsk_vlincomb, 32 x 32 for mpsk_vmultilincomb

#pragma GCC visibility push(hidden)

// helpers that cross a unit boundary
int ensure_ws(mpsk_ctx* c, size_t bytes);      // mpsk_api.hip
int gemm_c128(mpsk_ctx* c, int transA, int transB, int M, int N, int K, double alpha, const void* A, int64_t lda,
              const void* B, int64_t ldb, double beta, void* C, int64_t ldc);      // mpsk_api_vec.hip

inline GemmArgs mk(const double* A, const double* B, double* C, int M, int N, int K, int64_t lda, int64_t ldb,
                   int64_t ldc, int tA = 0, int tB = 0) {
  GemmArgs g;
  std::memset(&g, 0, sizeof(g));
  g.A = A; g.B = B; g.C = C; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb; g.ldc = ldc;
  g.batch = 1; g.nseg = 1; g.alpha = 1.0; g.beta = 0.0; g.transA = tA; g.transB = tB;
  return g;
}

inline size_t ev2(size_t v) { return (v + 1) & ~(size_t)1; }
inline size_t up32(size_t n) { return (n + 31) & ~(size_t)31; }      // 256-B aligned parts of the workspace

// Workspace cursor: the regions of c->ws in the order they are taken, in doubles.  take() returns the offset of a region
// and advances by its size rounded up to a multiple of `round` (2: ev2, 32: up32 -- the caller's choice); ensure() asks for
// exactly what was taken, and only then at() is a valid pointer.
struct Ws {
  size_t n = 0;
  size_t take(size_t doubles, size_t round = 1) { const size_t o = n; n += (doubles + round - 1) / round * round; return o; }
  int ensure(mpsk_ctx* c) const { return ensure_ws(c, sizeof(double) * n); }
  static double* at(mpsk_ctx* c, size_t off) { return c->ws.d() + off; }
};
// K-segment lists: element offsets into A / B; j: plane of a complex B operand (the J-aware loader), empty for a real one
struct Segs { std::vector<int64_t> a, b; std::vector<int> j; };

// complex scratch `which` / the bond-expansion scratch, at least `bytes` large (null with the error code)
inline int cx_scratch(mpsk_ctx* c, int which, size_t bytes, double** out) {
  const int rc = c->cxws[which].reserve(bytes, "complex gauge step: workspace hipMalloc failed", c->stream);
  *out = c->cxws[which].d();
  return rc;
}
inline int ex_scratch(mpsk_ctx* c, size_t bytes, double** out) {
  const int rc = c->exws.reserve(bytes, "bond expansion / two-site projection: scratch hipMalloc failed", c->stream);
  *out = c->exws.d();
  return rc;
}

#pragma GCC visibility pop
