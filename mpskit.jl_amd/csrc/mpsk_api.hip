// C ABI of libmpsk (see include/mpsk.h): argument checking, workspace management and the
// decomposition of every hot-path operator into  MFMA-GEMM -> slab-mix -> MFMA-GEMM  launches.
#include <cstdio>
#include <cmath>
#include <algorithm>
#include "mpsk_api_internal.h"

static thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }

// dense slices (mpsk_mposlice_create_dense) with min(Wl, Wr) d below this keep the slab-mix route (see dense_route)
static constexpr int MPSK_DENSE_MIN_CHID = 8;

static void pair_plan_build(int Wl, int Wr, int d, const double* O, bool left, PairPlan* pp) {
  auto at = [&](int w, int t, int s, int v) { return O[w + (size_t)Wl * (t + d * (s + (size_t)d * v))]; };
  *pp = PairPlan();
  if (Wl < 2 || Wr < 2) return;
  int nl = left ? Wr - 2 : Wl - 2;
  if (left)
    for (int t = 0; t < d && nl == Wr - 2; ++t)
      for (int s = 0; s < d; ++s) if (at(0, t, s, Wr - 1) != 0.0) { nl = Wr - 1; break; }
  if (nl <= 0) return;
  auto direct = [&](int l, int i, int j) { return left ? at(0, i, j, 1 + l) : at(1 + l, j, i, Wr - 1); };
  for (int pass = 0; pass < 2; ++pass)          // diagonal pairs, then the others
    for (int i = 0; i < d; ++i)
      for (int j = i; j < d; ++j) {
        if ((pass == 0) != (i == j)) continue;
        bool used = false;
        for (int l = 0; l < nl && !used; ++l) used = direct(l, i, j) != 0.0 || direct(l, j, i) != 0.0;
        if (!used) continue;
        pp->i.push_back(i); pp->j.push_back(j);
        if (i == j) pp->ndiag++;
      }
  pp->np = (int)pp->i.size();
  pp->nl = pp->np ? nl : 0;
  pp->coef.assign((size_t)pp->nl * pp->np * 2, 0.0);
  for (int l = 0; l < pp->nl; ++l)
    for (int p = 0; p < pp->np; ++p) {
      const int i = pp->i[p], j = pp->j[p];
      pp->coef[((size_t)l * pp->np + p) * 2] = direct(l, i, j);
      pp->coef[((size_t)l * pp->np + p) * 2 + 1] = i == j ? 0.0 : direct(l, j, i);
    }
}

// Route choice of a canonical transfer, in seconds at the rate the batched transfer GEMMs reach (~50 TFLOP/s): the pair
// products -- 2 K n^2 flops each, a symmetric one ~0.55 of that with its lower tiles skipped -- plus the one launch the
// route adds (~6 us with its gap, the price mpsk_hac_create_ex uses) against `interior` levels of 2 d K n^2.  The
// elementwise passes of the two routes (slab mix / combination) move about the same bytes and are left out.  With a
// single interior level the batch of two levels would fall apart into two launches of n^2 / 64^2 tiles each for less than
// 2 K n^2 saved: not taken.  K, n: contracted and result bond (left: Dl, Dr; right: Dr, Dl).
static bool pair_route_pays(const PairPlan& pp, int interior, int d, int K, int n) {
  if (pp.np == 0 || interior < 2) return false;
  const double unit = 2.0 * K * (double)n * n / 50e12;
  return (0.55 * pp.ndiag + (pp.np - pp.ndiag)) * unit + 6e-6 < (double)interior * d * unit;
}

extern "C" {

int mpsk_version(void) { return 100; }
const char* mpsk_last_error(void) { return g_err.c_str(); }

int mpsk_ctx_create(int device, mpsk_ctx** out) {
  REQUIRE(out != nullptr, "out is NULL");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  REQUIRE(device >= 0 && device < ndev, "no such HIP device (is a GPU visible?)");
  HIPCHK(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(MPSK_ERR_UNSUPPORTED, std::string("libmpsk is built for gfx950 only, device is ") + prop.gcnArchName);
  mpsk_ctx* c = new mpsk_ctx();
  c->device = device;
  HIPCHK(hipMalloc(&c->d_scal, sizeof(double) * MAXK));
  HIPCHK(hipMalloc(&c->d_partial, sizeof(double) * MPSK_DOT_SCRATCH));
  HIPCHK(hipHostMalloc(&c->h_scal, sizeof(double) * MAXK, hipHostMallocDefault));
  HIPCHK(hipMalloc(&c->d_coef, sizeof(double) * MAXCOEF));
  HIPCHK(hipHostMalloc(&c->h_coef, sizeof(double) * MAXCOEF, hipHostMallocDefault));
  HIPCHK(hipEventCreateWithFlags(&c->ev_coef, hipEventDisableTiming | hipEventDisableSystemFence));
  HIPCHK(hipMalloc(&c->d_flag, 64));
  HIPCHK(hipHostMalloc(&c->h_flags, 64, hipHostMallocDefault));
  HIPCHK(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
  c->xstreams[0] = c->stream2;
  HIPCHK(hipStreamCreateWithFlags(&c->xstreams[1], hipStreamNonBlocking));
  HIPCHK(hipStreamCreateWithFlags(&c->xstreams[2], hipStreamNonBlocking));
  HIPCHK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming | hipEventDisableSystemFence));
  HIPCHK(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming | hipEventDisableSystemFence));
  gemm_retain_stream(c->stream);
  gemm_retain_stream(c->stream2);
  gemm_retain_stream(c->xstreams[1]);
  gemm_retain_stream(c->xstreams[2]);
  *out = c;
  return MPSK_OK;
}

int mpsk_ctx_destroy(mpsk_ctx* c) {
  if (!c) return MPSK_OK;
  (void)hipSetDevice(c->device);
  // a ctx destroyed inside a side-stream section or with a deferred factorization pending: route back to the main stream
  // (otherwise the caller's stream would be destroyed below and the private one leaked) and complete the factorization
  if (c->on_side) (void)mpsk_ctx_side_end(c);
  if (c->pend.active) (void)mpsk_qr_commit(c, nullptr);
  (void)hipStreamSynchronize(c->stream);
  if (c->stream2) (void)hipStreamSynchronize(c->stream2);
  gemm_release_stream(c->stream);     // split-K partial-tile workspaces attached to this ctx's streams
  gemm_release_stream(c->stream2);
  for (auto& kv : c->pair_plans) mix_plan_destroy(&kv.second);
  for (auto& b : c->pool) { if (b.p) (void)hipFree(b.p); if (b.ev) (void)hipEventDestroy(b.ev); }
  if (c->d_scal) (void)hipFree(c->d_scal);
  if (c->d_partial) (void)hipFree(c->d_partial);
  if (c->h_scal) (void)hipHostFree(c->h_scal);
  if (c->d_coef) (void)hipFree(c->d_coef);
  if (c->h_coef) (void)hipHostFree(c->h_coef);
  if (c->ev_coef) (void)hipEventDestroy(c->ev_coef);
  if (c->d_flag) (void)hipFree(c->d_flag);
  if (c->h_flags) (void)hipHostFree(c->h_flags);
  for (int i = 1; i < 3; ++i)
    if (c->xstreams[i]) { (void)hipStreamSynchronize(c->xstreams[i]); gemm_release_stream(c->xstreams[i]); (void)hipStreamDestroy(c->xstreams[i]); }
  if (c->stream2) { (void)hipStreamSynchronize(c->stream2); (void)hipStreamDestroy(c->stream2); }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  delete c;
  return MPSK_OK;
}

int mpsk_ctx_set_stream(mpsk_ctx* c, void* s) {
  REQUIRE(c, "ctx is NULL");
  REQUIRE(!c->on_side, "not inside a side-stream section (mpsk_ctx_side_end first)");
  REQUIRE(!c->pend.active, "a deferred factorization is pending (mpsk_qr_commit first)");
  if (c->stream != (hipStream_t)s) {
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    gemm_release_stream(c->stream);
    gemm_retain_stream((hipStream_t)s);
  }
  c->stream = (hipStream_t)s;
  return MPSK_OK;
}

int mpsk_ctx_set_dtype(mpsk_ctx* c, int dtype) {
  REQUIRE(c, "ctx is NULL");
  REQUIRE(dtype == MPSK_F64 || dtype == MPSK_C128, "dtype must be MPSK_F64 or MPSK_C128");
  c->dtype = dtype;
  return MPSK_OK;
}
int mpsk_ctx_get_stream(mpsk_ctx* c, void** s) {
  REQUIRE(c && s, "NULL argument");
  *s = (void*)c->stream;
  return MPSK_OK;
}
int mpsk_ctx_get_device(mpsk_ctx* c, int* device) {
  REQUIRE(c && device, "NULL argument");
  *device = c->device;
  return MPSK_OK;
}

int mpsk_ctx_synchronize(mpsk_ctx* c) {
  REQUIRE(c, "ctx is NULL");
  HIPCHK(hipStreamSynchronize(c->stream));
  return MPSK_OK;
}

int mpsk_ctx_workspace_reserve(mpsk_ctx* c, size_t bytes) {
  REQUIRE(c, "ctx is NULL");
  if (bytes <= c->ws.bytes) return MPSK_OK;
  REQUIRE(!c->on_side && !c->pend.active, "the workspace is in use (side-stream section / deferred factorization)");
  HIPCHK(hipSetDevice(c->device));
  size_t want = (bytes + (size_t(1) << 20) - 1) & ~((size_t(1) << 20) - 1);
  return c->ws.reserve(want, "workspace hipMalloc failed", c->stream);
}

int mpsk_ctx_force_tile(mpsk_ctx* c, int bm, int bn) {
  REQUIRE(c, "ctx is NULL");
  REQUIRE((bm == 0 && bn == 0) || ((bm == 64 || bm == 128) && (bn == 64 || bn == 128)), "tile must be 64/128");
  gemm_force_tile(bm, bn);
  return MPSK_OK;
}

// Event profile of the matvec-stage GEMM launches (kernel dac_gemm_f64_kernel): enable, run, then
// read a JSON summary [{kernel, launches, total_ms, avg_ms, flops}] (device-synchronising).
int mpsk_prof_enable(mpsk_ctx* c, int on) {
  REQUIRE(c, "ctx is NULL");
  gemm_prof_enable(on != 0);
  return MPSK_OK;
}
int mpsk_prof_summary(mpsk_ctx* c, char* buf, size_t buflen) {
  REQUIRE(c && buf && buflen > 0, "NULL argument");
  std::string s = gemm_prof_summary();
  if (s.size() + 1 > buflen) return fail(MPSK_ERR_INVALID, "mpsk_prof_summary: buffer too small");
  std::memcpy(buf, s.c_str(), s.size() + 1);
  return MPSK_OK;
}

int mpsk_malloc(mpsk_ctx* c, size_t bytes, void** dptr) {
  REQUIRE(c && dptr, "NULL argument");
  HIPCHK(hipSetDevice(c->device));
  hipError_t e = hipMalloc(dptr, bytes ? bytes : 16);
  if (e != hipSuccess) return fail(MPSK_ERR_NOMEM, "hipMalloc failed");
  return MPSK_OK;
}
int mpsk_free(mpsk_ctx* c, void* dptr) {
  REQUIRE(c, "ctx is NULL");
  if (dptr) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(dptr)); }
  return MPSK_OK;
}
int mpsk_memcpy_h2d(mpsk_ctx* c, void* dst, const void* src, size_t bytes) {
  REQUIRE(c, "ctx is NULL");
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return MPSK_OK;
}
int mpsk_memcpy_d2h(mpsk_ctx* c, void* dst, const void* src, size_t bytes) {
  REQUIRE(c, "ctx is NULL");
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  return MPSK_OK;
}
int mpsk_memcpy_d2d(mpsk_ctx* c, void* dst, const void* src, size_t bytes) {
  REQUIRE(c, "ctx is NULL");
  HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, c->stream));
  return MPSK_OK;
}

// --------------------------------------------------------------------------------------------
// MPO slices
// --------------------------------------------------------------------------------------------
// dense = true: the slice of mpsk_mposlice_create_dense.  Above the crossover it has no right-combined fold (mpsk_hac never
// takes mode 1 for it: at chi = d = 16 the fold would hold 4096 slabs); below, it is prepared exactly like the slice
// mpsk_mposlice_create builds from the same O.
static int mposlice_build(mpsk_ctx* c, int dtype, int odim, const int32_t* chi_l, const int32_t* chi_r, int d,
                          const int32_t* kind, const double* scalars, const void* const* blocks, bool dense,
                          mpsk_mposlice** out) {
  REQUIRE(c && out && chi_l && chi_r && kind, "NULL argument");
  REQUIRE(dtype == MPSK_F64 || dtype == MPSK_C128, "dtype must be MPSK_F64 or MPSK_C128");
  const bool cx = dtype == MPSK_C128;     // scalars / dense blocks are then interleaved complex128 (re, im)
  REQUIRE(odim > 0 && d > 0, "odim and d must be positive");
  HIPCHK(hipSetDevice(c->device));
  std::vector<int> offl(odim + 1, 0), offr(odim + 1, 0);
  for (int i = 0; i < odim; ++i) {
    REQUIRE(chi_l[i] > 0 && chi_r[i] > 0, "chi must be positive");
    offl[i + 1] = offl[i] + chi_l[i];
    offr[i + 1] = offr[i] + chi_r[i];
  }
  auto* s = new mpsk_mposlice();
  s->ctx = c; s->Wl = offl[odim]; s->Wr = offr[odim]; s->d = d; s->dtype = dtype;
  s->Ofull.assign((size_t)s->Wl * d * d * s->Wr, 0.0);
  if (cx) s->Ofull_im.assign(s->Ofull.size(), 0.0);
  auto at = [&](int w, int t, int si, int v) -> double& {
    return s->Ofull[w + (size_t)s->Wl * (t + d * (si + (size_t)d * v))];
  };
  auto ati = [&](int w, int t, int si, int v) -> double& {
    return s->Ofull_im[w + (size_t)s->Wl * (t + d * (si + (size_t)d * v))];
  };
  for (int j = 0; j < odim; ++j)
    for (int i = 0; i < odim; ++i) {
      int k = kind[i + odim * j];
      if (k == MPSK_BLOCK_ZERO) continue;
      if (k == MPSK_BLOCK_SCALAR) {
        if (!scalars || chi_l[i] != chi_r[j]) { delete s; return fail(MPSK_ERR_INVALID, "scalar block needs scalars[] and chi_l[i] == chi_r[j]"); }
        const size_t e = (size_t)i + (size_t)odim * j;
        const double cv = cx ? scalars[2 * e] : scalars[e], ci = cx ? scalars[2 * e + 1] : 0.0;
        for (int a = 0; a < chi_l[i]; ++a)
          for (int t = 0; t < d; ++t) {
            at(offl[i] + a, t, t, offr[j] + a) = cv;
            if (cx) ati(offl[i] + a, t, t, offr[j] + a) = ci;
          }
      } else if (k == MPSK_BLOCK_DENSE) {
        if (!blocks || !blocks[i + odim * j]) { delete s; return fail(MPSK_ERR_INVALID, "dense block pointer is NULL"); }
        const double* b = (const double*)blocks[i + odim * j];
        const int cl = chi_l[i], cr = chi_r[j];
        for (int v = 0; v < cr; ++v)
          for (int si = 0; si < d; ++si)
            for (int t = 0; t < d; ++t)
              for (int w = 0; w < cl; ++w) {
                const size_t e = w + (size_t)cl * (t + d * (si + (size_t)d * v));
                at(offl[i] + w, t, si, offr[j] + v) = cx ? b[2 * e] : b[e];
                if (cx) ati(offl[i] + w, t, si, offr[j] + v) = b[2 * e + 1];
              }
      } else { delete s; return fail(MPSK_ERR_INVALID, "bad block kind"); }
    }
  std::vector<MixTerm> fwd, bwd, rgt;
  s->row_used.assign(s->Wl, 0); s->col_used.assign(s->Wr, 0);
  for (int v = 0; v < s->Wr; ++v)
    for (int si = 0; si < d; ++si)
      for (int t = 0; t < d; ++t)
        for (int w = 0; w < s->Wl; ++w) {
          const double cv = s->O(w, t, si, v), ci = s->Oi(w, t, si, v);
          if (cv == 0.0 && ci == 0.0) continue;
          fwd.push_back({t + d * v, si + d * w, cv, ci});
          bwd.push_back({si + d * w, t + d * v, cv, ci});
          rgt.push_back({t + d * w, si + d * v, cv, ci});
          s->row_used[w] = 1; s->col_used[v] = 1;
        }
  HIPCHK(mix_plan_create(fwd, d * s->Wr, d * s->Wl, &s->fwd));
  HIPCHK(mix_plan_create(bwd, d * s->Wl, d * s->Wr, &s->bwd));
  HIPCHK(mix_plan_create(rgt, d * s->Wl, d * s->Wr, &s->rgt));
  const bool fold = !dense || std::min(s->Wl, s->Wr) * d < MPSK_DENSE_MIN_CHID;
  if (!cx && fold) {  // right-combined plan (real slices; complex operators use the mix form)
    std::vector<MixTerm> rc;
    std::vector<int> per_t(d, 0);
    for (int t = 0; t < d; ++t)
      for (int w = 0; w < s->Wl; ++w)
        for (int si = 0; si < d; ++si) {
          bool any = false;
          for (int v = 0; v < s->Wr; ++v)
            if (s->O(w, t, si, v) != 0.0) { rc.push_back({(int32_t)s->rc_w.size(), v, s->O(w, t, si, v)}); any = true; }
          if (any) { s->rc_w.push_back(w); s->rc_s.push_back(si); s->rc_t.push_back(t); per_t[t]++; }
        }
    for (int t = 0; t < d; ++t) if (per_t[t] > s->rc_nseg) s->rc_nseg = per_t[t];
    HIPCHK(mix_plan_create(rc, (int)s->rc_w.size(), s->Wr, &s->rc));
  }
  // (complex slices: the same form with complex C / B / D blocks and exactly real identity corners; they feed the complex
  // mode 3 of mpsk_hac_create_ex, MPSK_HAC_CANONICAL_C128, and nothing else)
  if (odim >= 2 && chi_l[0] == 1 && chi_r[0] == 1 && chi_l[odim - 1] == 1 && chi_r[odim - 1] == 1) {
    const int Wl = s->Wl, Wr = s->Wr;
    bool ok = true;
    for (int t = 0; t < d && ok; ++t)
      for (int si = 0; si < d && ok; ++si) {
        ok = s->O(0, t, si, 0) == (t == si ? 1.0 : 0.0) && s->O(Wl - 1, t, si, Wr - 1) == (t == si ? 1.0 : 0.0) &&
             s->Oi(0, t, si, 0) == 0.0 && s->Oi(Wl - 1, t, si, Wr - 1) == 0.0;
        for (int v = 0; v < Wr - 1 && ok; ++v)
          for (int w = 1; w < Wl && ok; ++w) ok = s->O(w, t, si, v) == 0.0 && s->Oi(w, t, si, v) == 0.0;
      }
    if (ok) {
      std::vector<MixTerm> jr, jl;
      std::vector<char> r_used(d * d, 0), l_used(d * d, 0);
      for (int t = 0; t < d; ++t)
        for (int si = 0; si < d; ++si) {
          const int p = si + d * t;
          for (int v = 0; v < Wr; ++v)
            if (s->O(0, t, si, v) != 0.0 || s->Oi(0, t, si, v) != 0.0) {
              jr.push_back({p, v, s->O(0, t, si, v), s->Oi(0, t, si, v)}); r_used[p] = 1;
            }
          for (int w = 1; w < Wl; ++w)
            if (s->O(w, t, si, Wr - 1) != 0.0 || s->Oi(w, t, si, Wr - 1) != 0.0) {
              jl.push_back({p, w, s->O(w, t, si, Wr - 1), s->Oi(w, t, si, Wr - 1)}); l_used[p] = 1;
            }
        }
      // per-t slab lists, padded with an empty slab of the family (one exists whenever a list is shorter than the longest)
      auto lists = [&](const std::vector<char>& used, std::vector<int>& out, int& nseg) {
        int empty = -1;
        for (int p = 0; p < d * d; ++p) if (!used[p]) { empty = p; break; }
        for (int t = 0; t < d; ++t) {
          int n = 0;
          for (int si = 0; si < d; ++si) n += used[si + d * t];
          nseg = std::max(nseg, n);
        }
        out.assign((size_t)d * nseg, empty);
        for (int t = 0; t < d; ++t) {
          int k = 0;
          for (int si = 0; si < d; ++si) if (used[si + d * t]) out[(size_t)t * nseg + k++] = si + d * t;
        }
      };
      lists(r_used, s->jr_p, s->jr_nseg);
      lists(l_used, s->jl_p, s->jl_nseg);
      HIPCHK(mix_plan_create(jr, d * d, Wr, &s->jr));
      HIPCHK(mix_plan_create(jl, d * d, Wl, &s->jl));
      s->jordan = s->jr_nseg > 0 && s->jl_nseg > 0;
      if (s->jordan && !cx) {
        std::vector<MixTerm> tl, tr;
        for (int t = 0; t < d; ++t)
          for (int si = 0; si < d; ++si) {
            for (int v = 1; v < Wr; ++v)
              if (s->O(0, t, si, v) != 0.0) { tl.push_back({t + d * (v - 1), si, s->O(0, t, si, v)}); if (v == Wr - 1) s->tl_dblock = true; }
            for (int w = 1; w < Wl - 1; ++w)
              if (s->O(w, t, si, Wr - 1) != 0.0) tr.push_back({t + d * (w - 1), si, s->O(w, t, si, Wr - 1)});
          }
        HIPCHK(mix_plan_create(tl, d * (Wr - (s->tl_dblock ? 1 : 2)), d, &s->tl));
        HIPCHK(mix_plan_create(tr, d * (Wl - 2), d, &s->tr));
        for (PairPlan* pp : {&s->pl, &s->pr}) {
          pair_plan_build(Wl, Wr, d, s->Ofull.data(), pp == &s->pl, pp);
          if (pp->np == 0) continue;
          if (hipMalloc(&pp->d_coef, sizeof(double) * pp->coef.size()) != hipSuccess) {
            mpsk_mposlice_destroy(s);
            return fail(MPSK_ERR_NOMEM, "pair coefficient table hipMalloc failed");
          }
          HIPCHK(hipMemcpy(pp->d_coef, pp->coef.data(), sizeof(double) * pp->coef.size(), hipMemcpyHostToDevice));
        }
      }
    }
  }
  if (dense) {
    const int Wl = s->Wl, Wr = s->Wr;
    std::vector<double> od((size_t)d * Wl * d * Wr);
    for (int v = 0; v < Wr; ++v)
      for (int t = 0; t < d; ++t)
        for (int w = 0; w < Wl; ++w)
          for (int si = 0; si < d; ++si)
            od[(si + (size_t)d * w) + (size_t)d * Wl * (t + (size_t)d * v)] = s->O(w, t, si, v);
    s->dense = true;
    if (hipMalloc(&s->d_Od, sizeof(double) * od.size()) != hipSuccess) { mpsk_mposlice_destroy(s); return fail(MPSK_ERR_NOMEM, "dense MPO hipMalloc failed"); }
    HIPCHK(hipMemcpy(s->d_Od, od.data(), sizeof(double) * od.size(), hipMemcpyHostToDevice));
    for (int v = 0; v < Wr; ++v)
      for (int t = 0; t < d; ++t)
        for (int w = 0; w < Wl; ++w)
          for (int si = 0; si < d; ++si)
            od[(si + (size_t)d * v) + (size_t)d * Wr * (t + (size_t)d * w)] = s->O(w, t, si, v);
    if (hipMalloc(&s->d_OdR, sizeof(double) * od.size()) != hipSuccess) { mpsk_mposlice_destroy(s); return fail(MPSK_ERR_NOMEM, "dense MPO hipMalloc failed"); }
    HIPCHK(hipMemcpy(s->d_OdR, od.data(), sizeof(double) * od.size(), hipMemcpyHostToDevice));
  }
  *out = s;
  return MPSK_OK;
}

int mpsk_mposlice_create(mpsk_ctx* c, int dtype, int odim, const int32_t* chi_l, const int32_t* chi_r,
                         int d, const int32_t* kind, const double* scalars, const void* const* blocks,
                         mpsk_mposlice** out) {
  return mposlice_build(c, dtype, odim, chi_l, chi_r, d, kind, scalars, blocks, false, out);
}

int mpsk_mposlice_create_dense(mpsk_ctx* c, int dtype, int Wl, int Wr, int d, const void* O, mpsk_mposlice** out) {
  REQUIRE(c && O && out, "NULL argument");
  REQUIRE(dtype == MPSK_F64, "dense MPO slices are MPSK_F64 only (complex DenseMPO is not implemented; build an MPSK_C128 "
                             "slice with mpsk_mposlice_create instead)");
  REQUIRE(Wl > 0 && Wr > 0 && d > 0, "Wl, Wr and d must be positive");
  const int32_t cl = Wl, cr = Wr, kind = MPSK_BLOCK_DENSE;
  const void* blocks[1] = {O};
  return mposlice_build(c, dtype, 1, &cl, &cr, d, &kind, nullptr, blocks, true, out);
}

int mpsk_mposlice_destroy(mpsk_mposlice* s) {
  if (!s) return MPSK_OK;
  mpsk_ctx* c = s->ctx;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  for (auto it = c->pair_plans.begin(); it != c->pair_plans.end();) {
    if (it->first.first == s || it->first.second == s) { mix_plan_destroy(&it->second); it = c->pair_plans.erase(it); }
    else ++it;
  }
  mix_plan_destroy(&s->fwd);
  mix_plan_destroy(&s->bwd);
  mix_plan_destroy(&s->rgt);
  mix_plan_destroy(&s->rc);
  mix_plan_destroy(&s->jr);
  mix_plan_destroy(&s->jl);
  mix_plan_destroy(&s->tl);
  mix_plan_destroy(&s->tr);
  if (s->pl.d_coef) (void)hipFree(s->pl.d_coef);
  if (s->pr.d_coef) (void)hipFree(s->pr.d_coef);
  if (s->d_Od) (void)hipFree(s->d_Od);
  if (s->d_OdR) (void)hipFree(s->d_OdR);
  delete s;
  return MPSK_OK;
}

int mpsk_mposlice_dims(const mpsk_mposlice* s, int* Wl, int* Wr, int* d) {
  REQUIRE(s, "slice is NULL");
  if (Wl) *Wl = s->Wl;
  if (Wr) *Wr = s->Wr;
  if (d) *d = s->d;
  return MPSK_OK;
}

}  // extern "C"

// --------------------------------------------------------------------------------------------
// helpers
// --------------------------------------------------------------------------------------------
int ensure_ws(mpsk_ctx* c, size_t bytes) {
  if (c->pend.active) return fail(MPSK_ERR_INVALID, "a deferred factorization still owns the workspace: call mpsk_qr_commit first");
  if (c->on_side) return fail(MPSK_ERR_INVALID, "workspace users are not accepted on the side stream: call mpsk_ctx_side_end first");
  if (bytes <= c->ws.bytes) return MPSK_OK;
  return mpsk_ctx_workspace_reserve(c, bytes + bytes / 4);
}

// run a GEMM whose K dimension is a list of segments longer than MAXSEG by chunking (beta = 1)
static hipError_t gemm_segments(GemmArgs g, const std::vector<int64_t>& sa, const std::vector<int64_t>& sb,
                                hipStream_t s, const std::vector<int>* sj = nullptr) {
  size_t n = sa.size();
  if (n == 0) return hipErrorInvalidValue;
  double beta0 = g.beta;
  for (size_t i0 = 0; i0 < n; i0 += MAXSEG) {
    int ns = (int)std::min<size_t>(MAXSEG, n - i0);
    g.nseg = ns;
    for (int i = 0; i < ns; ++i) {
      g.segA[i] = sa[i0 + i]; g.segB[i] = sb[i0 + i];
      g.segJ[i] = sj ? (signed char)(*sj)[i0 + i] : 0;
    }
    g.beta = (i0 == 0) ? beta0 : 1.0;
    hipError_t e = gemm_f64(g, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

static hipError_t zero_async(void* p, size_t bytes, hipStream_t s) { return hipMemsetAsync(p, 0, bytes, s); }


namespace {
// The two optional terms of mpsk_qp_apply on top of the plain projection: (lB, AR) joins stage 1 as a second product that
// accumulates into T1, (half, rB) joins stage 3 as a second product that accumulates into y.  Either pair may be null.
struct QpExtra { const double* lB; const double* AR; int Dl2; const double* half; const double* rB; int Dr2; };
}  // namespace

// over MPO levels: level v gives (v strideA, v strideB + pl planeB) for each of the `planes` (1: real, 2: re / im) planes
// of B; levels with used[v] == 0 (used2[v] == 0) are skipped.  Returns false when no segment is left: the result is zero.
static bool level_segs(Segs& s, int W, int64_t strideA, int64_t strideB, const std::vector<char>* used = nullptr,
                       int planes = 1, int64_t planeB = 0, const std::vector<char>* used2 = nullptr) {
  for (int v = 0; v < W; ++v) {
    if ((used && !(*used)[v]) || (used2 && !(*used2)[v])) continue;
    for (int pl = 0; pl < planes; ++pl) {
      s.a.push_back((int64_t)v * strideA); s.b.push_back(pl * planeB + (int64_t)v * strideB);
      if (planes == 2) s.j.push_back(pl);
    }
  }
  return !s.a.empty();
}
// over the physical index: (t strideA, t strideB)
static void phys_segs(Segs& s, int d, int64_t strideA, int64_t strideB) { level_segs(s, d, strideA, strideB); }
static hipError_t gemm_segments(const GemmArgs& g, const Segs& s, hipStream_t st) {
  return gemm_segments(g, s.a, s.b, st, s.j.empty() ? nullptr : &s.j);
}
static int zero_fill(mpsk_ctx* c, void* y, size_t bytes) { HIPCHK(zero_async(y, bytes, c->stream)); return MPSK_OK; }

// stage 2 as a slab mix over MPO levels: T2[v][:,t,:] = sum_{w,s} O[..] T1[w][:,s,:] on slabs [M, d, N]
static hipError_t mix_levels(mpsk_ctx* c, const MixPlan& plan, int d, int M, int N, const double* T1, double* T2) {
  SlabIndex ix{d, 1 << 30, (int64_t)M, (int64_t)M * d * N, 0, (int64_t)M * d};
  return mix_apply(plan, T1, ix, T2, ix, M, N, c->stream);
}

// B of g is a plane pair `stride` doubles apart: two K-segments, the second through the J loader (1: J, 2: -J of A)
static void cx_operand(GemmArgs& g, int64_t stride, int j = 1) { g.nseg = 2; g.segB[1] = stride; g.segJ[1] = (signed char)j; g.cplx = 1; }

// stage 1 of the left-to-right contractions: T1[w] = G[w] X for W slabs G[w] [M, K] and X [K, N] (complex: M = 2 x rows,
// X the plane pair cx_stride apart).  X may come in nblk row blocks, which become K-segments (mpsk_dAC_blocked).
static hipError_t stage1(mpsk_ctx* c, int W, int M, int K, int N, const double* G, const double* X, double* T1, int tag,
                         int nblk = 1, int64_t cx_stride = 0, double beta = 0.0) {
  const int kb = K / nblk;
  GemmArgs g1 = mk(G, X, T1, M, N, kb, M, kb, M);
  g1.batch = W; g1.bsA = (int64_t)M * K; g1.bsB = 0; g1.bsC = (int64_t)M * N;
  g1.nseg = nblk;
  for (int q = 0; q < nblk; ++q) { g1.segA[q] = (int64_t)q * kb * M; g1.segB[q] = (int64_t)q * kb * N; }
  g1.tag = tag; g1.beta = beta;
  if (cx_stride) cx_operand(g1, cx_stride);
  return gemm_f64(g1, c->stream);
}

// device copy of a host offset / segment table (DevTables caches and frees it)
int upload_table(const std::vector<int64_t>& h, const char* what, int64_t** out) {
  int64_t* p = nullptr;
  if (hipMalloc(&p, sizeof(int64_t) * h.size()) != hipSuccess) return fail(MPSK_ERR_NOMEM, std::string(what) + " hipMalloc failed");
  if (hipMemcpy(p, h.data(), sizeof(int64_t) * h.size(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(p);
    return fail(MPSK_ERR_HIP, std::string(what) + " upload failed");
  }
  *out = p;
  return MPSK_OK;
}

// (Wl, Wr, d) of a call that takes either a slice or, with H == NULL, the pass-through dimensions (W, d)
static void site_dims(const mpsk_mposlice* H, int W, int& Wl, int& Wr, int& d) {
  Wl = Wr = W;
  if (H) { Wl = H->Wl; Wr = H->Wr; d = H->d; }
}

static bool hac_check_on() { const char* ev = getenv("MPSK_HAC_CHECK"); return ev && ev[0] == '1'; }

// --------------------------------------------------------------------------------------------
// derivatives
// --------------------------------------------------------------------------------------------
// ---- complex128 operators -----------------------------------------------------------------------------------------
// Every complex tensor argument is interleaved complex128 in TensorKit / Julia layout = a REAL column-major tensor whose
// first dimension is doubled, rows (2 a, 2 a + 1) = (re, im) of row a.  With A_half such a view and B = Br + i Bi:
//   (A B)_half = A_half Br + (J A_half) Bi ,     J (re, im) = (-im, re)
// so a complex product is the real GEMM core with two K-segments (the second through the J-aware A loader, GemmArgs::segJ)
// on a B operand split into planes -- 4x the real flops, the complex optimum; intermediates stay interleaved.
static hipError_t cx_planes(const double* z, size_t n, double* re, double* im, hipStream_t s) {     // interleaved -> planar
  if ((uintptr_t)z % 16 == 0) return deinterleave(z, (int64_t)n, re, im, s);
  hipError_t e = copy_strided(z, 2, 0, re, 1, 0, (int64_t)n, 1, s);
  if (e != hipSuccess) return e;
  return copy_strided(z + 1, 2, 0, im, 1, 0, (int64_t)n, 1, s);
}
// planar copy of an interleaved tensor of n complex elements in the workspace: [re | im], ev2(n) doubles apart
struct CxPlanes {
  size_t off, n;
  CxPlanes(Ws& ws, size_t n_) : off(ws.take(n_, 2)), n(n_) { ws.take(n_, 2); }
  int64_t stride() const { return (int64_t)ev2(n); }
  double* at(mpsk_ctx* c) const { return Ws::at(c, off); }
  hipError_t split(mpsk_ctx* c, const double* z) const { return cx_planes(z, n, at(c), at(c) + ev2(n), c->stream); }
};

// GRp: planar copy of GR ([re plane | im plane], each Wr Dr Dro doubles) if the caller has one (prepared operator), else null.
// Dro: columns of the GR slabs [Dr, Dro] = last dimension of y (the square matvec passes Dro = Dr; mpsk_dAC_proj the bond
// dimension of the state below).
static int dAC_c128(mpsk_ctx* c, const mpsk_mposlice* H, int Dlo, int Dl, int Dr, int Dro, const double* GL, const double* GR,
                    const double* GRp, const double* x, double* y, double alpha = 1.0, double beta = 0.0) {
  // GRp planes are ev2(Wr Dr Dro) doubles apart; alpha / beta: y = alpha H x + beta y, folded into the last GEMM (mpsk_hsum)
  HIPCHK(hipSetDevice(c->device));
  const int d = H->d, Wl = H->Wl, Wr = H->Wr;
  const size_t nx = (size_t)Dl * d * Dr, nG = (size_t)Wr * Dr * Dro, slab = (size_t)2 * Dlo * d * Dr;
  Ws ws;
  const CxPlanes xpl(ws, nx), gpl(ws, GRp ? 0 : nG);      // no region for GR when the caller has the planar copy
  const size_t o_t1 = ws.take(slab * Wl), o_t2 = ws.take(slab * Wr);
  if (int rc = ws.ensure(c)) return rc;
  double *T1 = Ws::at(c, o_t1), *T2 = Ws::at(c, o_t2);
  HIPCHK(xpl.split(c, x));
  const double* gr = GRp;
  if (!gr) { HIPCHK(gpl.split(c, GR)); gr = gpl.at(c); }
  HIPCHK(stage1(c, Wl, 2 * Dlo, Dl, d * Dr, GL, xpl.at(c), T1, 0, 1, xpl.stride()));      // T1[w] = GL[w] x
  HIPCHK(mix_levels(c, H->fwd, d, 2 * Dlo, Dr, T1, T2));
  Segs sg;
  if (!level_segs(sg, Wr, (int64_t)slab, (int64_t)Dr * Dro, &H->col_used, 2, (int64_t)ev2(nG)))
    return beta == 1.0 ? MPSK_OK : zero_fill(c, y, sizeof(double) * 2 * Dlo * d * Dro);
  GemmArgs g3 = mk(T2, gr, y, 2 * Dlo * d, Dro, Dr, (int64_t)2 * Dlo * d, Dr, (int64_t)2 * Dlo * d);
  g3.cplx = 1; g3.alpha = alpha; g3.beta = beta;
  HIPCHK(gemm_segments(g3, sg, c->stream));
  return MPSK_OK;
}

// Dro: columns of the GR slabs [Dr, Dro] = columns of y (mpsk_dC passes Dro = Dr; mpsk_dC_proj_c the bond dimension of the
// state below).
static int dC_c128(mpsk_ctx* c, int W, int Dlo, int Dl, int Dr, int Dro, const double* GL, const double* GR, const double* cm,
                   double* y) {
  HIPCHK(hipSetDevice(c->device));
  const size_t nx = (size_t)Dl * Dr, nG = (size_t)W * Dr * Dro, slab = (size_t)2 * Dlo * Dr;
  Ws ws;
  const CxPlanes xpl(ws, nx), gpl(ws, nG);
  const size_t o_t1 = ws.take(slab * W);
  if (int rc = ws.ensure(c)) return rc;
  double* T1 = Ws::at(c, o_t1);
  HIPCHK(xpl.split(c, cm));
  HIPCHK(gpl.split(c, GR));
  HIPCHK(stage1(c, W, 2 * Dlo, Dl, Dr, GL, xpl.at(c), T1, 0, 1, xpl.stride()));
  Segs sg;
  level_segs(sg, W, (int64_t)slab, (int64_t)Dr * Dro, nullptr, 2, gpl.stride());
  GemmArgs g3 = mk(T1, gpl.at(c), y, 2 * Dlo, Dro, Dr, 2 * Dlo, Dr, 2 * Dlo);
  g3.cplx = 1;
  HIPCHK(gemm_segments(g3, sg, c->stream));
  return MPSK_OK;
}

static int pair_plan(mpsk_ctx* c, const mpsk_mposlice* H1, const mpsk_mposlice* H2, const MixPlan** out) {
  auto key = std::make_pair(H1, H2);
  auto it = c->pair_plans.find(key);
  if (it != c->pair_plans.end()) { *out = &it->second; return MPSK_OK; }
  const int d1 = H1->d, d2 = H2->d, Wl = H1->Wl, Wm = H1->Wr, Wr = H2->Wr;
  // O12[(t1,t2,v) <- (s1,s2,w)] = sum_u O1[w,t1,s1,u] O2[u,t2,s2,v]   (derivatives.jl:128-147)
  std::map<std::pair<int, int>, std::pair<double, double>> acc;
  for (int u = 0; u < Wm; ++u)
    for (int w = 0; w < Wl; ++w)
      for (int t1 = 0; t1 < d1; ++t1)
        for (int s1 = 0; s1 < d1; ++s1) {
          const double a = H1->O(w, t1, s1, u), ai = H1->Oi(w, t1, s1, u);
          if (a == 0.0 && ai == 0.0) continue;
          for (int v = 0; v < Wr; ++v)
            for (int t2 = 0; t2 < d2; ++t2)
              for (int s2 = 0; s2 < d2; ++s2) {
                const double b = H2->O(u, t2, s2, v), bi = H2->Oi(u, t2, s2, v);
                if (b == 0.0 && bi == 0.0) continue;
                int o = t1 + d1 * (t2 + d2 * v), in = s1 + d1 * (s2 + d2 * w);
                auto& e = acc[{o, in}];
                e.first += a * b - ai * bi;
                e.second += a * bi + ai * b;
              }
        }
  std::vector<MixTerm> terms;
  for (auto& kv : acc)
    if (kv.second.first != 0.0 || kv.second.second != 0.0)
      terms.push_back({kv.first.first, kv.first.second, kv.second.first, kv.second.second});
  MixPlan p;
  HIPCHK(mix_plan_create(terms, d1 * d2 * Wr, d1 * d2 * Wl, &p));
  auto res = c->pair_plans.emplace(key, p);
  *out = &res.first->second;
  return MPSK_OK;
}

// x2: [Dl, d1, Dr, d2]; GR: Wr slabs [Dr, Dro]; y2: [Dlo, d1, Dro, d2] (Dro = Dr: mpsk_dAC2)
static int dAC2_c128(mpsk_ctx* c, const mpsk_mposlice* H1, const mpsk_mposlice* H2, int Dlo, int Dl, int Dr, int Dro,
                     const double* GL, const double* GR, const double* x2, double* y2) {
  HIPCHK(hipSetDevice(c->device));
  const int d1 = H1->d, d2 = H2->d, Wl = H1->Wl, Wr = H2->Wr;
  const size_t nx = (size_t)Dl * d1 * Dr * d2, nG = (size_t)Wr * Dr * Dro;
  const size_t plane = (size_t)2 * Dlo * d1 * Dr, slab = plane * d2, oplane = (size_t)2 * Dlo * d1 * Dro;
  Ws ws;
  const CxPlanes xpl(ws, nx), gpl(ws, nG);
  const size_t o_t1 = ws.take(slab * Wl), o_t2 = ws.take(slab * Wr);
  if (int rc = ws.ensure(c)) return rc;
  double *T1 = Ws::at(c, o_t1), *T2 = Ws::at(c, o_t2);
  const MixPlan* plan = nullptr;
  if (int rc = pair_plan(c, H1, H2, &plan)) return rc;
  HIPCHK(xpl.split(c, x2));
  HIPCHK(gpl.split(c, GR));
  HIPCHK(stage1(c, Wl, 2 * Dlo, Dl, d1 * Dr * d2, GL, xpl.at(c), T1, 0, 1, xpl.stride()));
  SlabIndex ix{d1, d2, (int64_t)2 * Dlo, (int64_t)plane, (int64_t)slab, (int64_t)2 * Dlo * d1};
  HIPCHK(mix_apply(*plan, T1, ix, T2, ix, 2 * Dlo, Dr, c->stream));
  Segs sg;
  if (!level_segs(sg, Wr, (int64_t)slab, (int64_t)Dr * Dro, &H2->col_used, 2, gpl.stride()))
    return zero_fill(c, y2, sizeof(double) * oplane * d2);
  GemmArgs g3 = mk(T2, gpl.at(c), y2, 2 * Dlo * d1, Dro, Dr, (int64_t)2 * Dlo * d1, Dr, (int64_t)2 * Dlo * d1);
  g3.batch = d2; g3.bsA = (int64_t)plane; g3.bsB = 0; g3.bsC = (int64_t)oplane; g3.cplx = 1;
  HIPCHK(gemm_segments(g3, sg, c->stream));
  return MPSK_OK;
}

// GLout[v][q,b] = sum GLin[w][p,a] A[a,s,b] O[w,t,s,v] conj(Ab[p,t,q])
// gram (pass-through only, Dr == Drb): gram[w][t,s] = sum conj(Ab[p,t,b]) T1[w][p,s,b] of the stage-1 product, partials
// after T1 in the workspace; GLout == nullptr then skips stage 2 (mpsk_transfer_left_gram)
// envR (with gram, Wl == 1): the [Dr, Drb] matrix that closes the site on the right; gram[t,s] = sum conj(Ab[p,t,q])
// T1[p,s,b] envR[b,q] then comes out of the fused closing product (gram_env), its planar copy of envR behind the partials
static int transfer_left_c128(mpsk_ctx* c, const mpsk_mposlice* H, int Wl, int Wr, int d, int Dl, int Dr, int Dlb, int Drb,
                              const double* GLin, const double* A, const double* Ab, double* GLout,
                              double* gram = nullptr, const double* envR = nullptr) {
  HIPCHK(hipSetDevice(c->device));
  const size_t nA = (size_t)Dl * d * Dr, slab = (size_t)2 * Dlb * d * Dr;
  Ws ws;
  const CxPlanes apl(ws, nA);
  const size_t o_t1 = ws.take(slab * Wl), o_t2 = ws.take(H ? slab * Wr : 0);
  const size_t o_part = ws.take(gram ? site_gram_partial_doubles(Wl, d, true) : 0, 2);  // H == NULL: straight after T1
  const CxPlanes rpl(ws, envR ? (size_t)Dr * Drb : 0);
  if (int rc = ws.ensure(c)) return rc;
  double* T1 = Ws::at(c, o_t1);
  double* T2 = H ? Ws::at(c, o_t2) : T1;
  HIPCHK(apl.split(c, A));
  HIPCHK(stage1(c, Wl, 2 * Dlb, Dl, d * Dr, GLin, apl.at(c), T1, 0, 1, apl.stride()));      // T1[w] = GLin[w] A, rows interleaved
  if (H) HIPCHK(mix_levels(c, H->fwd, d, 2 * Dlb, Dr, T1, T2));
  if (gram && envR) {
    HIPCHK(rpl.split(c, envR));
    HIPCHK(gram_env(d, Dlb, Dr, Drb, T1, rpl.at(c), rpl.stride(), Ab, true, gram, Ws::at(c, o_part), c->stream));
  } else if (gram) HIPCHK(site_gram(Wl, d, Dlb, Dr, T1, Ab, true, gram, Ws::at(c, o_part), c->stream));
  if (!GLout) return MPSK_OK;
  // GLout[v] = Ab^H T2[v]:  K = (re / im, p, t) interleaved on both operands ->  real part = Ab_half^T T2_half,
  // imaginary part = (J Ab_half)^T T2_half ; plane alpha goes to the rows 2 q + alpha of the interleaved result
  for (int al = 0; al < 2; ++al) {
    GemmArgs g3 = mk(Ab, T2, GLout + al, Drb, Dr, 2 * Dlb * d, (int64_t)2 * Dlb * d, (int64_t)2 * Dlb * d, (int64_t)2 * Drb, 1, 0);
    g3.batch = Wr; g3.bsA = 0; g3.bsB = (int64_t)slab; g3.bsC = (int64_t)2 * Drb * Dr;
    g3.cplx = 1; g3.c_rs = 2; g3.segJ[0] = (signed char)al;
    HIPCHK(gemm_f64(g3, c->stream));
  }
  return MPSK_OK;
}

// GRout[w][a,p] = sum A[a,s,b] O[w,t,s,v] conj(Ab[p,t,q]) GRin[v][b,q]   evaluated as  ((A GRin) mixed) Ab^H
static int transfer_right_c128(mpsk_ctx* c, const mpsk_mposlice* H, int Wl, int Wr, int d, int Dl, int Dr, int Dlb, int Drb,
                               const double* A, const double* Ab, const double* GRin, double* GRout) {
  HIPCHK(hipSetDevice(c->device));
  const size_t nG = (size_t)Wr * Dr * Drb, nB = (size_t)Dlb * d * Drb, slab = (size_t)2 * Dl * d * Drb;
  Ws ws;
  const CxPlanes gpl(ws, nG), bpl(ws, nB);
  const size_t o_x = ws.take(slab * Wr), o_y = ws.take(H ? slab * Wl : 0);
  if (int rc = ws.ensure(c)) return rc;
  double *X = Ws::at(c, o_x), *Y = H ? Ws::at(c, o_y) : X;
  HIPCHK(gpl.split(c, GRin));
  HIPCHK(bpl.split(c, Ab));
  // X[v][a,s,q] = sum_b A[a,s,b] GRin[v][b,q]      A as the (2 Dl d) x Dr interleaved matrix
  GemmArgs g1 = mk(A, gpl.at(c), X, 2 * Dl * d, Drb, Dr, (int64_t)2 * Dl * d, Dr, (int64_t)2 * Dl * d);
  g1.batch = Wr; g1.bsA = 0; g1.bsB = (int64_t)Dr * Drb; g1.bsC = (int64_t)slab;
  cx_operand(g1, gpl.stride());
  HIPCHK(gemm_f64(g1, c->stream));
  if (H) HIPCHK(mix_levels(c, H->rgt, d, 2 * Dl, Drb, X, Y));      // Y[w][a,t,q] = sum_{v,s} O[w,t,s,v] X[v][a,s,q]
  // GRout[w][a,p] = sum_{t,q} Y[w][a,(t,q)] conj(Ab[p,(t,q)]) = Y_half Abr^T + (-J Y_half) Abi^T
  GemmArgs g3 = mk(Y, bpl.at(c), GRout, 2 * Dl, Dlb, d * Drb, (int64_t)2 * Dl, Dlb, (int64_t)2 * Dl, 0, 1);
  g3.batch = Wl; g3.bsA = (int64_t)slab; g3.bsB = 0; g3.bsC = (int64_t)2 * Dl * Dlb;
  cx_operand(g3, bpl.stride(), 2);
  HIPCHK(gemm_f64(g3, c->stream));
  return MPSK_OK;
}

// x may be given in `nblk` row blocks (block q = rows [q Dl/nblk, (q+1) Dl/nblk) as a contiguous [Dl/nblk, d, Dr]
// tensor): the blocks become K-segments of the stage-1 GEMM, nothing is re-interleaved (mpsk_dAC_blocked).
// GR: Wr slabs [Dr, Dro], y: [Dlo, d, Dro]; the square matvec is Dro = Dr.
static int dAC_impl(mpsk_ctx* c, const mpsk_mposlice* H, int Dlo, int Dl, int Dr, int Dro, const void* GL, const void* GR,
                    const void* x, int nblk, void* y, double alpha = 1.0, double beta = 0.0, const QpExtra* q = nullptr,
                    size_t ws_base = 0) {
  HIPCHK(hipSetDevice(c->device));
  const int d = H->d, Wl = H->Wl, Wr = H->Wr;
  const size_t slab = (size_t)Dlo * d * Dr;
  Ws ws;
  ws.n = ws_base;                 // the doubles in front belong to the caller (mpsk_qp_heff_site: B and the projected result)
  const size_t o_t1 = ws.take(slab * Wl), o_t2 = ws.take(slab * Wr);
  if (int rc = ws.ensure(c)) return rc;
  double *T1 = Ws::at(c, o_t1), *T2 = Ws::at(c, o_t2);
  // stage 1: T1[w] = GL[w] * x     (batched over w)
  HIPCHK(stage1(c, Wl, Dlo, Dl, d * Dr, (const double*)GL, (const double*)x, T1, 1, nblk));
  if (q && q->lB) HIPCHK(stage1(c, Wl, Dlo, q->Dl2, d * Dr, q->lB, q->AR, T1, 1, 1, 0, 1.0));      // T1[w] += lB[w] AR
  // stage 2: T2[v][:,t,:] = sum_{w,s} O[w,t,s,v] T1[w][:,s,:]
  HIPCHK(mix_levels(c, H->fwd, d, Dlo, Dr, T1, T2));
  // stage 3: y = sum_v T2[v] * GR[v]   (K-segments over v)
  Segs sg;
  if (!level_segs(sg, Wr, (int64_t)slab, (int64_t)Dr * Dro, &H->col_used))
    return beta == 1.0 ? MPSK_OK : zero_fill(c, y, sizeof(double) * Dlo * d * Dro);
  GemmArgs g3 = mk(T2, (const double*)GR, (double*)y, Dlo * d, Dro, Dr, (int64_t)Dlo * d, Dr, (int64_t)Dlo * d);
  g3.tag = 1; g3.alpha = alpha; g3.beta = beta;
  HIPCHK(gemm_segments(g3, sg, c->stream));
  if (q && q->half) {                                                      // y += sum_v half[v] * rB[v]
    Segs sh;
    level_segs(sh, Wr, (int64_t)Dlo * d * q->Dr2, (int64_t)q->Dr2 * Dro, &H->col_used);
    GemmArgs g4 = mk(q->half, q->rB, (double*)y, Dlo * d, Dro, q->Dr2, (int64_t)Dlo * d, q->Dr2, (int64_t)Dlo * d);
    g4.tag = 1; g4.alpha = alpha; g4.beta = 1.0;
    HIPCHK(gemm_segments(g4, sh, c->stream));
  }
  return MPSK_OK;
}

// ---- dense MPO slices (mpsk_mposlice_create_dense): stage 2 on the MFMA GEMM core -------------------------------------
// A dense O[w,t,s,v] has (Wl d)(Wr d) terms: as a slab mix every output slab re-reads Wl d input slabs.  The dense route
// keeps the three-stage decomposition but lays the two intermediates out so that stage 2 is ONE plain GEMM:
//   T1[(r,b), (s,w)] = sum_a GL[w][r,a] x[a,s,b]           stage 1, batched over (s,w) with offset tables
//   T2[(r,b), (t,v)] = sum_(s,w) T1[(r,b), (s,w)] Od[(s,w), (t,v)]      stage 2, M = Dlo Dr, K = d Wl, N = d Wr
//   y[r,t,q]         = sum_v sum_b T2[(r,b), (t,v)] GR[v][b,q]          stage 3, batched over t, K-segments over v
// (r, b) is the row index of both intermediates, so the K index (s,w) of stage 2 has a single stride.  transfer_left
// is the same with (Dlb, Ab) in place of (Dlo, GR); transfer_right already produces U[(b,p), (t,v)] and consumes
// V[(b,p), (s,w)], so only its mix becomes a GEMM (B = Od^T).  Environments keep the slab layout.
// Below a product Wl d (and Wr d) of MPSK_DENSE_MIN_CHID the GEMMs are too narrow to beat the mix (tools/bench_dense_mpo.py):
// such slices take the mix route.  Environment MPSK_DENSE_ROUTE=1 / 0 forces the dense / mix route (tests, A/B).

static bool dense_route(const mpsk_mposlice* H) {
  if (!H || !H->dense || H->dtype != MPSK_F64) return false;
  if (const char* ev = getenv("MPSK_DENSE_ROUTE")) {
    if (ev[0] == '1') return true;
    if (ev[0] == '0') return false;
  }
  return std::min(H->Wl, H->Wr) * H->d >= MPSK_DENSE_MIN_CHID;
}

// device tables [2][W d] of a stage 1 batched over z = s + d w, cached on the slice per (P, Q).  Left (W = Wl, offsets of
// GL / x): tab[z] = w P, tab[W d + z] = s Q.  Right (W = Wr, offsets of the site tensor / GR): tab[z] = s P, tab[W d + z] = v Q.
static int dense_tab(const mpsk_mposlice* H, bool right, int64_t P, int64_t Q, const int64_t** out) {
  const int d = H->d, nz = (right ? H->Wr : H->Wl) * d;
  return (right ? H->dtabR : H->dtab).get({P, Q}, [&](std::vector<int64_t>& h) {
    h.resize((size_t)2 * nz);
    for (int z = 0; z < nz; ++z) { h[z] = (int64_t)(right ? z % d : z / d) * P; h[nz + z] = (int64_t)(right ? z / d : z % d) * Q; }
  }, "dense offset table", out);
}

// stage 1 of the dense route: T[(r,b), (s,w)] = sum_a G[w][r,a] X[a,s,b]   (G: Wl slabs [R, Dk]; X: [Dk, d, Nb])
static int dense_stage1(mpsk_ctx* c, const mpsk_mposlice* H, int R, int Dk, int Nb, const double* G, const double* X, double* T,
                        double beta = 0.0) {
  const int d = H->d;
  const int64_t* tab = nullptr;
  if (int rc = dense_tab(H, false, (int64_t)R * Dk, Dk, &tab)) return rc;
  GemmArgs g1 = mk(G, X, T, R, Nb, Dk, R, (int64_t)Dk * d, R);
  g1.batch = H->Wl * d; g1.bsC = (int64_t)R * Nb;
  g1.tabA = tab; g1.tabB = tab + (size_t)H->Wl * d;
  g1.tabs_even = ((int64_t)R * Dk) % 2 == 0 && Dk % 2 == 0;
  g1.tag = 1; g1.beta = beta;
  HIPCHK(gemm_f64(g1, c->stream));
  return MPSK_OK;
}

// stage 2: T2[(r,b), (t,v)] = T1[(r,b), (s,w)] Od      (rows = R Nb)
static int dense_stage2(mpsk_ctx* c, const mpsk_mposlice* H, int64_t rows, const double* T1, double* T2) {
  const int d = H->d;
  GemmArgs g2 = mk(T1, H->d_Od, T2, (int)rows, d * H->Wr, d * H->Wl, rows, (int64_t)d * H->Wl, rows);
  g2.tag = 1;
  HIPCHK(gemm_f64(g2, c->stream));
  return MPSK_OK;
}

static int dAC_dense(mpsk_ctx* c, const mpsk_mposlice* H, int Dlo, int Dl, int Dr, int Dro, const double* GL, const double* GR,
                     const double* x, double* y, double alpha = 1.0, double beta = 0.0, const QpExtra* q = nullptr,
                     size_t ws_base = 0) {
  HIPCHK(hipSetDevice(c->device));
  const int d = H->d, Wl = H->Wl, Wr = H->Wr;
  const size_t slab = (size_t)Dlo * Dr;               // one (s,w) / (t,v) column of the intermediates
  Ws ws;
  ws.n = ws_base;
  const size_t o_t1 = ws.take(slab * d * Wl), o_t2 = ws.take(slab * d * Wr);
  if (int rc = ws.ensure(c)) return rc;
  double *T1 = Ws::at(c, o_t1), *T2 = Ws::at(c, o_t2);
  if (int rc = dense_stage1(c, H, Dlo, Dl, Dr, GL, x, T1)) return rc;
  if (q && q->lB)
    if (int rc = dense_stage1(c, H, Dlo, q->Dl2, Dr, q->lB, q->AR, T1, 1.0)) return rc;      // T1 += lB AR
  if (int rc = dense_stage2(c, H, (int64_t)slab, T1, T2)) return rc;
  // stage 3: y[:, t, :] = sum_v T2[:, :, t, v] GR[v]    (batch over t; K-segments over v)
  Segs sg;
  if (!level_segs(sg, Wr, (int64_t)d * slab, (int64_t)Dr * Dro, &H->col_used))
    return beta == 1.0 ? MPSK_OK : zero_fill(c, y, sizeof(double) * Dlo * d * Dro);
  GemmArgs g3 = mk(T2, GR, y, Dlo, Dro, Dr, Dlo, Dr, (int64_t)Dlo * d);
  g3.batch = d; g3.bsA = (int64_t)slab; g3.bsB = 0; g3.bsC = Dlo;
  g3.tag = 1; g3.alpha = alpha; g3.beta = beta;
  HIPCHK(gemm_segments(g3, sg, c->stream));
  if (q && q->half) {                                                      // y[:, t, :] += sum_v half[:, :, t, v] rB[v]
    const size_t slab2 = (size_t)Dlo * q->Dr2;
    Segs sh;
    level_segs(sh, Wr, (int64_t)d * slab2, (int64_t)q->Dr2 * Dro, &H->col_used);
    GemmArgs g4 = mk(q->half, q->rB, y, Dlo, Dro, q->Dr2, Dlo, q->Dr2, (int64_t)Dlo * d);
    g4.batch = d; g4.bsA = (int64_t)slab2; g4.bsB = 0; g4.bsC = Dlo;
    g4.tag = 1; g4.alpha = alpha; g4.beta = 1.0;
    HIPCHK(gemm_segments(g4, sh, c->stream));
  }
  return MPSK_OK;
}

// GLout[v][q,b] = sum GLin[w][p,a] A[a,s,b] O[w,t,s,v] Ab[p,t,q]
// (V2, A2 [Dl2, d, Dr]): a second stage-1 product that accumulates into T1 (mpsk_transfer_left_pair)
static int transfer_left_dense(mpsk_ctx* c, const mpsk_mposlice* H, int Dl, int Dr, int Dlb, int Drb, const double* GLin,
                               const double* A, const double* Ab, double* GLout, const double* V2 = nullptr,
                               const double* A2 = nullptr, int Dl2 = 0) {
  const int d = H->d, Wl = H->Wl, Wr = H->Wr;
  const size_t slab = (size_t)Dlb * Dr;
  Ws ws;
  const size_t o_t1 = ws.take(slab * d * Wl), o_t2 = ws.take(slab * d * Wr);
  if (int rc = ws.ensure(c)) return rc;
  double *T1 = Ws::at(c, o_t1), *T2 = Ws::at(c, o_t2);
  if (int rc = dense_stage1(c, H, Dlb, Dl, Dr, GLin, A, T1)) return rc;
  if (V2)
    if (int rc = dense_stage1(c, H, Dlb, Dl2, Dr, V2, A2, T1, 1.0)) return rc;
  if (int rc = dense_stage2(c, H, (int64_t)slab, T1, T2)) return rc;
  // GLout[v][q,b] = sum_t sum_p Ab[p,t,q] T2[(p,b), (t,v)]     (batch over v; K-segments over t)
  Segs sg;
  phys_segs(sg, d, Dlb, (int64_t)slab);
  GemmArgs g3 = mk(Ab, T2, GLout, Drb, Dr, Dlb, (int64_t)Dlb * d, Dlb, Drb, 1, 0);
  g3.batch = Wr; g3.bsA = 0; g3.bsB = (int64_t)slab * d; g3.bsC = (int64_t)Drb * Dr;
  HIPCHK(gemm_segments(g3, sg, c->stream));
  return MPSK_OK;
}

extern "C" {
int mpsk_dAC(mpsk_ctx* c, const mpsk_mposlice* H, int Dlo, int Dl, int Dr, const void* GL, const void* GR,
             const void* x, void* y) {
  REQUIRE(c && H && GL && GR && x && y, "NULL argument");
  REQUIRE(Dlo > 0 && Dl > 0 && Dr > 0, "dimensions must be positive");
  if (H->dtype == MPSK_C128)
    return dAC_c128(c, H, Dlo, Dl, Dr, Dr, (const double*)GL, (const double*)GR, nullptr, (const double*)x, (double*)y);
  if (dense_route(H)) return dAC_dense(c, H, Dlo, Dl, Dr, Dr, (const double*)GL, (const double*)GR, (const double*)x, (double*)y);
  return dAC_impl(c, H, Dlo, Dl, Dr, Dr, GL, GR, x, 1, y);
}

int mpsk_dAC_blocked(mpsk_ctx* c, const mpsk_mposlice* H, int nblk, int Dlo, int Dl, int Dr, const void* GL,
                     const void* GR, const void* xblk, void* y) {
  REQUIRE(c && H && GL && GR && xblk && y, "NULL argument");
  REQUIRE(Dlo > 0 && Dl > 0 && Dr > 0, "dimensions must be positive");
  REQUIRE(nblk >= 1 && nblk <= MAXSEG && Dl % nblk == 0, "nblk must divide Dl (and be <= 32)");
  if (H->dtype == MPSK_C128) {
    if (nblk != 1) return fail(MPSK_ERR_UNSUPPORTED, "mpsk_dAC_blocked: the blocked layout is implemented for MPSK_F64 only");
    return dAC_c128(c, H, Dlo, Dl, Dr, Dr, (const double*)GL, (const double*)GR, nullptr, (const double*)xblk, (double*)y);
  }
  return dAC_impl(c, H, Dlo, Dl, Dr, Dr, GL, GR, xblk, nblk, y);
}

// ac_proj (derivatives.jl:210-217): the matvec with a rectangular right environment, GR slabs [Dr, Dro] (ket leg of the
// state above, bra leg of the state below).  Same three routes as mpsk_dAC with N = Dro in stage 3.
int mpsk_dAC_proj(mpsk_ctx* c, const mpsk_mposlice* H, int Dlo, int Dl, int Dr, int Dro, const void* GL, const void* GR,
                  const void* x, void* y) {
  REQUIRE(c && H && GL && GR && x && y, "NULL argument");
  REQUIRE(Dlo > 0 && Dl > 0 && Dr > 0 && Dro > 0, "dimensions must be positive");
  if (H->dtype == MPSK_C128)
    return dAC_c128(c, H, Dlo, Dl, Dr, Dro, (const double*)GL, (const double*)GR, nullptr, (const double*)x, (double*)y);
  if (dense_route(H)) return dAC_dense(c, H, Dlo, Dl, Dr, Dro, (const double*)GL, (const double*)GR, (const double*)x, (double*)y);
  return dAC_impl(c, H, Dlo, Dl, Dr, Dro, GL, GR, x, 1, y);
}

}  // extern "C"

// ---- prepared operator ---------------------------------------------------------------------------
static int pool_take(mpsk_ctx* c, size_t bytes, void** p, int* idx) {
  int best = -1;
  for (size_t i = 0; i < c->pool.size(); ++i)
    if (!c->pool[i].used && c->pool[i].bytes >= bytes && (best < 0 || c->pool[i].bytes < c->pool[best].bytes)) best = (int)i;
  if (best < 0) {
    // drop idle buffers that are too small before growing (bond dimensions grow monotonically along a chain)
    for (auto& b : c->pool)
      if (!b.used && b.p) { (void)hipStreamSynchronize(c->stream); (void)hipFree(b.p); b.p = nullptr; b.bytes = 0; }
    void* q = nullptr;
    if (hipMalloc(&q, bytes) != hipSuccess) return fail(MPSK_ERR_NOMEM, "prepared-operator buffer hipMalloc failed");
    int slot = -1;
    for (size_t i = 0; i < c->pool.size(); ++i) if (!c->pool[i].p) { slot = (int)i; break; }
    if (slot < 0) { c->pool.push_back({nullptr, 0, false}); slot = (int)c->pool.size() - 1; }
    c->pool[slot] = {q, bytes, false};
    best = slot;
  }
  c->pool[best].used = true;
  // the buffer's previous owner may have been applied on another stream (side-stream sections, rebound ctx): its last
  // applications must have completed before the new owner overwrites GRc
  if (c->pool[best].ev_set && c->pool[best].last != c->stream) (void)hipStreamWaitEvent(c->stream, c->pool[best].ev, 0);
  c->pool[best].ev_set = false;
  *p = c->pool[best].p;
  *idx = best;
  return MPSK_OK;
}

// max |G - I| of one n x n environment slab (MPSK_HAC_CHECK: a debug mode, it synchronises)
static int identity_deviation(mpsk_ctx* c, const double* G, int n, double* dev) {
  std::vector<double> h((size_t)n * n);
  HIPCHK(hipMemcpyAsync(h.data(), G, sizeof(double) * h.size(), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  double m = 0.0;
  for (int j = 0; j < n; ++j)
    for (int i = 0; i < n; ++i) m = std::max(m, std::fabs(h[i + (size_t)n * j] - (i == j ? 1.0 : 0.0)));
  *dev = m;
  return MPSK_OK;
}

// mode 3 (Jordan form): fold GRc0 / GLc into the pool buffer and upload the per-batch segment tables, on the ctx stream.
// Tables (element offsets), one launch: A[d][n1 + n2], B[d][n1 + n2] -- segments k < n1 relative to (x, GRc0), the others
// to (GLc, x); two launches: A1[d][n1], B1[d][n1], A2[d][n2], B2[d][n2].
// GL == nullptr: tables only (the folds of a summed operator are combined from its terms', mpsk_hsum_set_coefs).
static hipError_t hac_jordan_prepare(mpsk_ctx* c, mpsk_hac* h, const double* GL, const double* GR) {
  const mpsk_mposlice* H = h->H;
  const int d = H->d, n1 = h->jn1, n2 = h->jn2;
  const std::vector<int>&p1 = *h->jp1, &p2 = *h->jp2;
  const int Dlo = h->Dlo, Dl = h->Dl, Dr = h->Dr;
  const int64_t tR = (int64_t)Dr * d * Dr, tL = (int64_t)Dlo * d * Dl;     // one t-group of GRc0 / GLc
  // GRc0[(s,t)] = sum_v O[0,t,s,v] GR[v] ;  GLc[(s,t)] = sum_{w>0} O[w,t,s,W-1] GL[w]   (slab p = s + d t)
  SlabIndex ir{1 << 30, 1, (int64_t)Dr * Dr, 0, 0, (int64_t)Dr}, orr{d, 1 << 30, (int64_t)Dr, tR, 0, (int64_t)d * Dr};
  SlabIndex il{1 << 30, 1, (int64_t)Dlo * Dl, 0, 0, (int64_t)Dlo}, ol{d, 1 << 30, (int64_t)Dlo, tL, 0, (int64_t)d * Dlo};
  hipError_t e = hipSuccess;
  if (GL) {
    e = mix_apply(H->jr, GR, ir, h->GRc, orr, Dr, Dr, c->stream);
    if (e == hipSuccess) e = mix_apply(H->jl, GL, il, h->GLc, ol, Dlo, Dl, c->stream);
  }
  if (e != hipSuccess) return e;
  const int n = n1 + n2;
  h->zseg_host.assign((size_t)2 * d * n, 0);
  int64_t* tab = h->zseg_host.data();
  int64_t *a1 = tab, *b1 = tab + (size_t)d * n, *a2 = tab + n1, *b2 = tab + (size_t)d * n + n1;
  int64_t st1 = n, st2 = n;
  if (h->launches == 2) { b1 = tab + (size_t)d * n1; a2 = tab + (size_t)2 * d * n1; b2 = a2 + (size_t)d * n2; st1 = n1; st2 = n2; }
  for (int t = 0; t < d; ++t) {
    for (int k = 0; k < n1; ++k) {
      const int p = p1[(size_t)t * n1 + k], si = p % d, tt = p / d;
      a1[t * st1 + k] = (int64_t)si * Dl;                               // x[:, s, :]
      b1[t * st1 + k] = tt * tR + (int64_t)si * Dr;                     // GRc0[(s, tt)]
    }
    for (int k = 0; k < n2; ++k) {
      const int p = p2[(size_t)t * n2 + k], si = p % d, tt = p / d;
      a2[t * st2 + k] = tt * tL + (int64_t)si * Dlo;                    // GLc[(s, tt)]
      b2[t * st2 + k] = (int64_t)si * Dl;                               // x[:, s, :]
    }
  }
  e = hipMemcpyAsync(h->zseg, tab, sizeof(int64_t) * h->zseg_host.size(), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_up, hipEventDisableTiming | hipEventDisableSystemFence);
  if (e == hipSuccess) e = hipEventRecord(h->ev_up, c->stream);
  return e;
}

extern "C" {
int mpsk_hac_create(mpsk_ctx* c, const mpsk_mposlice* H, int Dlo, int Dl, int Dr, const void* GL, const void* GR,
                    mpsk_hac** out) {
  return mpsk_hac_create_ex(c, H, Dlo, Dl, Dr, GL, GR, 0, out);
}

int mpsk_hac_create_ex(mpsk_ctx* c, const mpsk_mposlice* H, int Dlo, int Dl, int Dr, const void* GL, const void* GR,
                       int flags, mpsk_hac** out) {
  REQUIRE(c && H && GL && GR && out, "NULL argument");
  REQUIRE((flags & ~(MPSK_HAC_CANONICAL | MPSK_HAC_CANONICAL_C128)) == 0, "unknown flags");
  REQUIRE(Dlo > 0 && Dl > 0 && Dr > 0, "dimensions must be positive");
  HIPCHK(hipSetDevice(c->device));
  const int d = H->d, Wl = H->Wl, Wr = H->Wr;
  int wr_used = 0;
  for (int v = 0; v < Wr; ++v) wr_used += H->col_used[v] ? 1 : 0;
  // cost model (stage 1 is the same in both forms): stage-3 slab products at ~50 TFLOP/s, plus -- for the mix form --
  // the slab-mix pass over T1 / T2 (HBM / L3 traffic at ~3 TB/s) and its launch.  Measured on MI355X: the mix costs
  // 24 us at D = 1024 (Heisenberg), a dependent launch ~6 us including its gap.
  const double u3 = 2.0 * Dlo * (double)Dr * Dr;
  const double slab_bytes = 8.0 * Dlo * (double)d * Dr;
  const double t_mix = (double)wr_used * d * u3 / 50e12 + (Wl + wr_used) * slab_bytes / 3e12 + 6e-6;
  const double t_rc = (double)H->rc_nseg * d * u3 / 50e12;
  auto* h = new mpsk_hac();
  h->ctx = c; h->H = H; h->Dlo = Dlo; h->Dl = Dl; h->Dr = Dr; h->GL = (const double*)GL; h->GR = (const double*)GR;
  // Jordan form: only on the caller's promise that level 0 of GL and level W-1 of GR are identities
  const bool jordan = (flags & MPSK_HAC_CANONICAL) && H->jordan && H->dtype == MPSK_F64 && Dlo == Dl;
  if (jordan && hac_check_on()) {
    double dl = 0.0, dr = 0.0;
    int rc = identity_deviation(c, (const double*)GL, Dl, &dl);
    if (!rc) rc = identity_deviation(c, (const double*)GR + (size_t)(Wr - 1) * Dr * Dr, Dr, &dr);
    if (rc) { delete h; return rc; }
    if (!(dl <= 1e-10 && dr <= 1e-10)) {
      delete h;
      char msg[160];
      snprintf(msg, sizeof(msg), "MPSK_HAC_CHECK: environments are not canonical (max|GL[0] - I| = %.3e, max|GR[W-1] - I| = %.3e)", dl, dr);
      return fail(MPSK_ERR_INVALID, msg);
    }
  }
  h->mode = jordan ? 3 : (H->rc_nseg > 0 && t_rc <= t_mix) ? 1 : 0;
  if (const char* ev = getenv("MPSK_HAC_MODE"))
    h->mode = (ev[0] == '3' && jordan) ? 3 : (ev[0] == '1' && H->rc_nseg > 0) ? 1 : 0;
  if (dense_route(H)) h->mode = 4;     // dense slice above the crossover (or MPSK_DENSE_ROUTE=1): GEMM route
  if (H->dtype == MPSK_C128) {
    // complex128: mix form; what is prepared once per site is the planar copy of the right environment (the B operand
    // of stage 3), so that an application converts only x
    h->mode = 2;
    // MPSK_HAC_CANONICAL_C128: the Jordan-form operator for a complex slice.  The conditions of the real mode 3, and the
    // identities are CHECKED here (two small launches, one synchronisation per prepared operator): a candidate whose
    // GL[0] or GR[W-1] is off by more than 1e-10 keeps mode 2 (MPSK_HAC_CHECK=1: fails, as the real mode does).
    bool jc = (flags & MPSK_HAC_CANONICAL_C128) && H->jordan && Dlo == Dl;
    if (jc) {
      const int nbk = 100;
      double dl = 0.0, dr = 0.0;
      HIPCHK(identity_dev_c((const double*)GL, Dl, c->d_scal, nbk, c->stream));
      HIPCHK(identity_dev_c((const double*)GR + (size_t)(Wr - 1) * 2 * Dr * Dr, Dr, c->d_scal + nbk, nbk, c->stream));
      HIPCHK(hipMemcpyAsync(c->h_scal, c->d_scal, sizeof(double) * 2 * nbk, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipStreamSynchronize(c->stream));
      for (int i = 0; i < nbk; ++i) { dl = std::max(dl, c->h_scal[i]); dr = std::max(dr, c->h_scal[nbk + i]); }
      if (!(dl <= 1e-10 && dr <= 1e-10)) {
        if (hac_check_on()) {
          delete h;
          char msg[160];
          snprintf(msg, sizeof(msg), "MPSK_HAC_CHECK: environments are not canonical (max|GL[0] - I| = %.3e, max|GR[W-1] - I| = %.3e)", dl, dr);
          return fail(MPSK_ERR_INVALID, msg);
        }
        jc = false;
      }
    }
    if (jc) {
      // folded slabs p = s + d t, contiguous: GRc0[p] [Dr, Dr] as two planes (the B operand of x GRc0), GLc[p] [Dlo, Dl]
      // interleaved (the A operand of GLc x); the interleaved fold of GR is staged behind them in the same buffer
      h->mode = 3;
      const size_t nR = (size_t)d * d * Dr * Dr, nL = (size_t)d * d * Dlo * Dl;
      void* buf = nullptr;
      if (int rc = pool_take(c, sizeof(double) * (2 * ev2(nR) + 2 * nL + 2 * nR), &buf, &h->pool_idx)) { delete h; return rc; }
      h->GRc = (double*)buf;
      h->GLc = h->GRc + 2 * ev2(nR);
      double* stage = h->GLc + 2 * nL;
      SlabIndex ir{1 << 30, 1, (int64_t)2 * Dr * Dr, 0, 0, (int64_t)2 * Dr}, il{1 << 30, 1, (int64_t)2 * Dlo * Dl, 0, 0, (int64_t)2 * Dlo};
      hipError_t e = mix_apply(H->jr, (const double*)GR, ir, stage, ir, 2 * Dr, Dr, c->stream);
      if (e == hipSuccess) e = cx_planes(stage, nR, h->GRc, h->GRc + ev2(nR), c->stream);
      if (e == hipSuccess) e = mix_apply(H->jl, (const double*)GL, il, h->GLc, il, 2 * Dlo, Dl, c->stream);
      if (e != hipSuccess) {
        (void)hipStreamSynchronize(c->stream);
        c->pool[h->pool_idx].used = false; delete h; return fail(MPSK_ERR_HIP, hipGetErrorString(e));
      }
      *out = h;
      return MPSK_OK;
    }
    const size_t nG = (size_t)Wr * Dr * Dr;
    void* buf = nullptr;
    if (int rc = pool_take(c, sizeof(double) * 2 * ev2(nG), &buf, &h->pool_idx)) { delete h; return rc; }
    h->GRc = (double*)buf;
    hipError_t e = cx_planes((const double*)GR, nG, h->GRc, h->GRc + ev2(nG), c->stream);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(c->stream);
      if (h->ev_up) (void)hipEventDestroy(h->ev_up);
      c->pool[h->pool_idx].used = false; delete h; return fail(MPSK_ERR_HIP, hipGetErrorString(e));
    }
    *out = h;
    return MPSK_OK;
  }
  if (h->mode == 3) {
    // one launch when both operand families share lda / ldb / K (Dl == Dr: the bulk of a chain); MPSK_HAC_LAUNCHES=2
    // forces the two-launch form (A/B switch)
    const char* ev = getenv("MPSK_HAC_LAUNCHES");
    h->launches = (Dl == Dr && !(ev && ev[0] == '2')) ? 1 : 2;
    h->jn1 = H->jr_nseg; h->jn2 = H->jl_nseg; h->jp1 = &H->jr_p; h->jp2 = &H->jl_p;
    const size_t nR = up32((size_t)d * d * Dr * Dr), nL = up32((size_t)d * d * Dlo * Dl);      // 256-B aligned parts
    const size_t bytes = sizeof(double) * (nR + nL) + sizeof(int64_t) * 2 * d * (H->jr_nseg + H->jl_nseg);
    void* buf = nullptr;
    if (int rc = pool_take(c, bytes, &buf, &h->pool_idx)) { delete h; return rc; }
    h->GRc = (double*)buf;
    h->GLc = h->GRc + nR;
    h->zseg = (int64_t*)(h->GLc + nL);
    hipError_t e = hac_jordan_prepare(c, h, (const double*)GL, (const double*)GR);
    if (e != hipSuccess) {
      (void)hipStreamSynchronize(c->stream);
      if (h->ev_up) (void)hipEventDestroy(h->ev_up);
      c->pool[h->pool_idx].used = false; delete h; return fail(MPSK_ERR_HIP, hipGetErrorString(e));
    }
  }
  if (h->mode == 1) {
    const int nc = (int)H->rc_w.size(), ns = H->rc_nseg;
    const size_t slabR = (size_t)Dr * Dr;
    const size_t bytes = sizeof(double) * slabR * (nc + 1) + sizeof(int64_t) * 2 * d * ns + 64;
    void* buf = nullptr;
    if (int rc = pool_take(c, bytes, &buf, &h->pool_idx)) { delete h; return rc; }
    h->GRc = (double*)buf;
    h->zseg = (int64_t*)((char*)buf + ((sizeof(double) * slabR * (nc + 1) + 15) & ~(size_t)15));
    // GRc[c] = sum_v O[w_c, t_c, s_c, v] GR[v] ; zero pad slab at index nc
    SlabIndex ix{1 << 30, 1, (int64_t)slabR, 0, 0, (int64_t)Dr};
    hipError_t e = mix_apply(H->rc, (const double*)GR, ix, h->GRc, ix, Dr, Dr, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->GRc + slabR * nc, 0, sizeof(double) * slabR, c->stream);
    // segment tables: stage-3 batch z = t;  A offset into T1 (slab w, plane s), B offset into GRc (slab c)
    const size_t slab1 = (size_t)Dlo * d * Dr;
    h->zseg_host.assign((size_t)2 * d * ns, 0);
    std::vector<int64_t>& tab = h->zseg_host;
    for (int t = 0; t < d; ++t) {
      int k = 0;
      for (int ci = 0; ci < nc; ++ci)
        if (H->rc_t[ci] == t) {
          tab[(size_t)t * ns + k] = (int64_t)H->rc_w[ci] * slab1 + (int64_t)H->rc_s[ci] * Dlo;
          tab[(size_t)(d + t) * ns + k] = (int64_t)ci * slabR;
          ++k;
        }
      for (; k < ns; ++k) { tab[(size_t)t * ns + k] = 0; tab[(size_t)(d + t) * ns + k] = (int64_t)nc * slabR; }
    }
    if (e == hipSuccess) e = hipMemcpyAsync(h->zseg, tab.data(), sizeof(int64_t) * tab.size(), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&h->ev_up, hipEventDisableTiming | hipEventDisableSystemFence);
    if (e == hipSuccess) e = hipEventRecord(h->ev_up, c->stream);
    if (e != hipSuccess) { c->pool[h->pool_idx].used = false; delete h; return fail(MPSK_ERR_HIP, hipGetErrorString(e)); }
  }
  *out = h;
  return MPSK_OK;
}

int mpsk_hac_destroy(mpsk_hac* h) {
  if (!h) return MPSK_OK;
  if (h->pool_idx >= 0 && h->pool_idx < (int)h->ctx->pool.size()) {
    PoolBuf& b = h->ctx->pool[h->pool_idx];
    b.used = false;
    // stream ordering of the hand-back: everything enqueued so far on the ctx's current stream still reads the buffer
    (void)hipSetDevice(h->ctx->device);
    if (!b.ev) (void)hipEventCreateWithFlags(&b.ev, hipEventDisableTiming | hipEventDisableSystemFence);
    if (b.ev && hipEventRecord(b.ev, h->ctx->stream) == hipSuccess) { b.last = h->ctx->stream; b.ev_set = true; }
  }
  if (h->ev_up) { (void)hipEventSynchronize(h->ev_up); (void)hipEventDestroy(h->ev_up); }   // zseg_host is still being read until then
  delete h;
  return MPSK_OK;
}

int mpsk_hac_info(const mpsk_hac* h, int* mode, int* nslabs) {
  REQUIRE(h, "hac is NULL");
  if (mode) *mode = h->mode;
  if (nslabs) *nslabs = h->mode == 1 ? (int)h->H->rc_w.size() : h->mode == 3 ? h->H->jr.n_out + h->H->jl.n_out : 0;
  return MPSK_OK;
}

}  // extern "C"

// complex mode 3: y[:, t, :] = sum_s x[:, s, :] GRc0[(s, t)] + sum_s GLc[(s, t)] x[:, s, :], two launches batched over t with
// all d values of s as K-segments (re and im plane of the B operand each, the second through the J loader): 16 d^2 D^3
// real flops, against 16 (Wl + Wr) d D^3 of the mix form
static int hac_apply_jordan_c128(mpsk_hac* h, const double* x, double* y, double alpha = 1.0, double beta = 0.0) {
  mpsk_ctx* c = h->ctx;
  const int d = h->H->d, Dlo = h->Dlo, Dl = h->Dl, Dr = h->Dr;
  HIPCHK(hipSetDevice(c->device));
  const size_t nx = (size_t)Dl * d * Dr, nR = (size_t)d * d * Dr * Dr;
  Ws ws;
  const CxPlanes xpl(ws, nx);
  if (int rc = ws.ensure(c)) return rc;
  HIPCHK(xpl.split(c, x));
  Segs s1, s2;      // over the physical index s, both planes of the B operand
  level_segs(s1, d, (int64_t)2 * Dl, (int64_t)Dr * Dr, nullptr, 2, (int64_t)ev2(nR));
  GemmArgs g1 = mk(x, h->GRc, y, 2 * Dlo, Dr, Dr, (int64_t)2 * Dl * d, Dr, (int64_t)2 * Dlo * d);
  g1.batch = d; g1.bsA = 0; g1.bsB = (int64_t)d * Dr * Dr; g1.bsC = (int64_t)2 * Dlo;
  g1.cplx = 1; g1.alpha = alpha; g1.beta = beta;
  HIPCHK(gemm_segments(g1, s1, c->stream));
  level_segs(s2, d, (int64_t)2 * Dlo * Dl, Dl, nullptr, 2, xpl.stride());
  GemmArgs g2 = mk(h->GLc, xpl.at(c), y, 2 * Dlo, Dr, Dl, (int64_t)2 * Dlo, (int64_t)Dl * d, (int64_t)2 * Dlo * d);
  g2.batch = d; g2.bsA = (int64_t)d * 2 * Dlo * Dl; g2.bsB = 0; g2.bsC = (int64_t)2 * Dlo;
  g2.cplx = 1; g2.alpha = alpha; g2.beta = 1.0;
  HIPCHK(gemm_segments(g2, s2, c->stream));
  return MPSK_OK;
}

// y = alpha H x + beta y with alpha / beta in the last GEMM stage of every mode (beta: 0 or 1).  alpha = 1, beta = 0 is
// mpsk_hac_apply; the other values are the accumulated route of mpsk_hsum_apply.
static int hac_apply_ab(mpsk_hac* h, const void* x, int nblk, void* y, double alpha, double beta) {
  mpsk_ctx* c = h->ctx;
  const mpsk_mposlice* H = h->H;
  const int Dlo = h->Dlo, Dl = h->Dl, Dr = h->Dr;
  if (h->mode == 3 && H->dtype == MPSK_C128) {
    if (nblk != 1) return fail(MPSK_ERR_UNSUPPORTED, "mpsk_hac_apply: the blocked layout is implemented for MPSK_F64 only");
    return hac_apply_jordan_c128(h, (const double*)x, (double*)y, alpha, beta);
  }
  if (h->mode == 2) {
    if (nblk != 1) return fail(MPSK_ERR_UNSUPPORTED, "mpsk_hac_apply: the blocked layout is implemented for MPSK_F64 only");
    return dAC_c128(c, H, Dlo, Dl, Dr, Dr, h->GL, h->GR, h->GRc, (const double*)x, (double*)y, alpha, beta);
  }
  if (h->mode == 0 || (h->mode == 4 && nblk != 1)) return dAC_impl(c, H, Dlo, Dl, Dr, Dr, h->GL, h->GR, x, nblk, y, alpha, beta);
  if (h->mode == 4) return dAC_dense(c, H, Dlo, Dl, Dr, Dr, h->GL, h->GR, (const double*)x, (double*)y, alpha, beta);
  HIPCHK(hipSetDevice(c->device));
  if (h->mode == 3) {
    // y[:, t, :] = sum_k x[:, s_k, :] GRc0[(s_k, t)] + sum_k GLc[(s_k, t)] x[:, s_k, :]     (batch over t)
    if (nblk != 1) return fail(MPSK_ERR_UNSUPPORTED, "mpsk_hac_apply: the Jordan-form operator takes the plain vector layout only");
    const int d = H->d, n1 = h->jn1, n2 = h->jn2;
    const bool even = Dlo % 2 == 0 && Dl % 2 == 0 && Dr % 2 == 0;
    GemmArgs g = mk((const double*)x, h->GRc, (double*)y, Dlo, Dr, Dr, (int64_t)Dl * d, (int64_t)Dr * d, (int64_t)Dlo * d);
    g.batch = d; g.bsA = 0; g.bsB = 0; g.bsC = (int64_t)Dlo;
    g.tabs_even = even;
    g.tag = 1; g.alpha = alpha; g.beta = beta;
    if (h->launches == 1) {        // Dl == Dr: the (GLc, x) family has the same lda / ldb / K
      g.A2 = h->GLc; g.B2 = (const double*)x; g.nseg1 = n1;
      g.nseg = n1 + n2; g.zsegA = h->zseg; g.zsegB = h->zseg + (size_t)d * (n1 + n2);
      HIPCHK(gemm_f64(g, c->stream));
      return MPSK_OK;
    }
    g.nseg = n1; g.zsegA = h->zseg; g.zsegB = h->zseg + (size_t)d * n1;
    HIPCHK(gemm_f64(g, c->stream));
    GemmArgs g2 = mk(h->GLc, (const double*)x, (double*)y, Dlo, Dr, Dl, (int64_t)Dlo * d, (int64_t)Dl * d, (int64_t)Dlo * d);
    g2.batch = d; g2.bsA = 0; g2.bsB = 0; g2.bsC = (int64_t)Dlo;
    g2.alpha = alpha; g2.beta = 1.0;
    g2.tabs_even = even;
    g2.tag = 1;
    g2.nseg = n2; g2.zsegA = h->zseg + (size_t)2 * d * n1; g2.zsegB = g2.zsegA + (size_t)d * n2;
    HIPCHK(gemm_f64(g2, c->stream));
    return MPSK_OK;
  }
  const int d = H->d, Wl = H->Wl, ns = H->rc_nseg;
  const size_t slab = (size_t)Dlo * d * Dr;
  Ws ws;
  const size_t o_t1 = ws.take(slab * Wl);
  if (int rc = ws.ensure(c)) return rc;
  double* T1 = Ws::at(c, o_t1);
  // stage 1: T1[w] = GL[w] * x     (batched over w; x possibly in row blocks = K segments)
  HIPCHK(stage1(c, Wl, Dlo, Dl, d * Dr, h->GL, (const double*)x, T1, 1, nblk));
  // stage 3: y[:, t, :] = sum_{c: t_c = t} T1[w_c][:, s_c, :] GRc[c]      (batch over t, per-batch K-segment tables)
  GemmArgs g3 = mk(T1, h->GRc, (double*)y, Dlo, Dr, Dr, (int64_t)Dlo * d, Dr, (int64_t)Dlo * d);
  g3.batch = d; g3.bsA = 0; g3.bsB = 0; g3.bsC = (int64_t)Dlo;
  g3.nseg = ns; g3.zsegA = h->zseg; g3.zsegB = h->zseg + (size_t)d * ns;
  g3.tabs_even = (Dlo % 2 == 0) && (Dr % 2 == 0);
  g3.tag = 1; g3.alpha = alpha; g3.beta = beta;
  HIPCHK(gemm_f64(g3, c->stream));
  return MPSK_OK;
}

extern "C" {
int mpsk_hac_apply(mpsk_hac* h, const void* x, int nblk, void* y) {
  REQUIRE(h && x && y, "NULL argument");
  REQUIRE(nblk >= 1 && nblk <= MAXSEG && h->Dl % nblk == 0, "nblk must divide Dl (and be <= 32)");
  return hac_apply_ab(h, x, nblk, y, 1.0, 0.0);
}

// y = a0 x + a1 (H_AC x): the shifted operator of linsolve(H_AC, b, x0, alg, a0, a1) (corvector.jl:68, :123).  The
// application is mpsk_hac_apply itself (every mode, same launches, same bits); the shift and the scale are ONE fused
// vector pass over x and y behind its last GEMM.  a0 = 0, a1 = 1 adds nothing to mpsk_hac_apply.
int mpsk_hac_apply_axpby(mpsk_hac* h, const double* a1, const void* x, int nblk, const double* a0, void* y) {
  REQUIRE(h && x && y && a0 && a1, "NULL argument");
  REQUIRE(x != y, "x and y must not alias");
  const bool cplx = h->H->dtype == MPSK_C128;
  const bool shift = a0[0] != 0.0 || (cplx && a0[1] != 0.0);
  const bool scale = a1[0] != 1.0 || (cplx && a1[1] != 0.0);
  REQUIRE(!shift || (h->Dlo == h->Dl && nblk == 1), "a shift needs a square operator (Dlo == Dl) on the plain vector layout");
  if (int rc = mpsk_hac_apply(h, x, nblk, y)) return rc;
  if (!shift && !scale) return MPSK_OK;
  mpsk_ctx* c = h->ctx;
  const int64_t n = (int64_t)h->Dlo * h->H->d * h->Dr;
  if (cplx) {
    HIPCHK(vec_axpby_c(a0, shift ? (const double*)x : nullptr, a1, (double*)y, n, c->stream));
  } else if (shift) {
    HIPCHK(vec_axpby(a0[0], (const double*)x, a1[0], (double*)y, n, c->stream));
  } else {
    HIPCHK(vec_scal(a1[0], (double*)y, n, c->stream));
  }
  return MPSK_OK;
}

// ---- summed prepared operator (mpsk_hsum): y = sum_k coefs[k] H_k x for n operators on one site ------------------------
// Route 1 (folded): every term is a mode-3 operator.  Mode 3 is linear in its two folds, so sum_k c_k H_k is ONE mode-3
// operator with the folds sum_k c_k GRc0_k / sum_k c_k GLc_k: the terms keep their folds (their own mpsk_hac), `sum` owns
// the combined pair and the segment tables of the union pattern; mpsk_hsum_set_coefs is one fold_lincomb launch.
// Route 2 (accumulated): the terms are applied one after another, coefs[k] and beta = 1 in the last GEMM of each.
struct mpsk_hsum {
  mpsk_ctx* ctx = nullptr;
  int n = 0, route = 2;
  mpsk_hac* term[MPSK_HSUM_MAX] = {};
  double coef[MPSK_HSUM_MAX] = {};
  mpsk_hac* sum = nullptr;                 // route 1: the combined operator
  std::vector<int> up1, up2;               // route 1, MPSK_F64: per-t slab lists of the union pattern
};

static void hsum_free(mpsk_hsum* s) {
  if (s->sum) (void)mpsk_hac_destroy(s->sum);
  for (int k = 0; k < s->n; ++k) if (s->term[k]) (void)mpsk_hac_destroy(s->term[k]);
  delete s;
}

// route 1: combine the terms' folds into s->sum with the current coefficients (one launch on the ctx stream)
static int hsum_combine(mpsk_hsum* s) {
  const mpsk_hac* h = s->sum;
  const int d = h->H->d;
  const size_t nR = (size_t)d * d * h->Dr * h->Dr, nL = (size_t)d * d * h->Dlo * h->Dl;
  FoldLincombArgs a;
  std::memset(&a, 0, sizeof(a));
  a.n = s->n;
  for (int k = 0; k < s->n; ++k) { a.srcR[k] = s->term[k]->GRc; a.srcL[k] = s->term[k]->GLc; a.coef[k] = s->coef[k]; }
  a.dstR = h->GRc; a.dstL = h->GLc;
  // complex: the two planes of GRc0 (ev2(nR) doubles apart) and the interleaved GLc
  const bool cx = h->H->dtype == MPSK_C128;
  a.nR = (int64_t)(cx ? 2 * ev2(nR) : nR);
  a.nL = (int64_t)(cx ? 2 * nL : nL);
  HIPCHK(hipSetDevice(s->ctx->device));
  HIPCHK(fold_lincomb(a, s->ctx->stream));
  return MPSK_OK;
}

int mpsk_hsum_create(mpsk_ctx* c, int n, const mpsk_mposlice* const* H, int Dlo, int Dl, int Dr, const void* const* GL,
                     const void* const* GR, int flags, mpsk_hsum** out) {
  REQUIRE(c && H && GL && GR && out, "NULL argument");
  REQUIRE(n >= 1 && n <= MPSK_HSUM_MAX, "needs 1 <= n <= 8 terms");
  REQUIRE((flags & ~(MPSK_HAC_CANONICAL | MPSK_HAC_CANONICAL_C128)) == 0, "unknown flags");
  REQUIRE(Dlo > 0 && Dl > 0 && Dr > 0, "dimensions must be positive");
  for (int k = 0; k < n; ++k) {
    REQUIRE(H[k] && GL[k] && GR[k], "NULL term");
    REQUIRE(H[k]->d == H[0]->d && H[k]->dtype == H[0]->dtype, "the terms must share d and dtype");
  }
  auto* s = new mpsk_hsum();
  s->ctx = c;
  for (int k = 0; k < n; ++k) {
    if (int rc = mpsk_hac_create_ex(c, H[k], Dlo, Dl, Dr, GL[k], GR[k], flags, &s->term[k])) { hsum_free(s); return rc; }
    s->n = k + 1;
    s->coef[k] = 1.0;
  }
  bool folded = true;
  for (int k = 0; k < n; ++k) folded = folded && s->term[k]->mode == 3 && s->term[k]->launches == s->term[0]->launches;
  if (folded) {
    const int d = H[0]->d;
    const bool cx = H[0]->dtype == MPSK_C128;
    auto* h = new mpsk_hac();
    h->ctx = c; h->H = H[0]; h->Dlo = Dlo; h->Dl = Dl; h->Dr = Dr; h->GL = nullptr; h->GR = nullptr;
    h->mode = 3; h->launches = s->term[0]->launches;
    s->sum = h;
    const size_t nR = (size_t)d * d * Dr * Dr, nL = (size_t)d * d * Dlo * Dl;
    void* buf = nullptr;
    if (cx) {
      if (int rc = pool_take(c, sizeof(double) * (2 * ev2(nR) + 2 * nL), &buf, &h->pool_idx)) { hsum_free(s); return rc; }
      h->GRc = (double*)buf;
      h->GLc = h->GRc + 2 * ev2(nR);
      // the combine runs over the two planes of GRc0 as one range of 2 ev2(nR) doubles: for odd nR that includes the pad
      // double behind each plane, which no fold writes -- zero it in every term so that nothing uninitialised is read
      if (nR & 1)
        for (int k = 0; k < n; ++k)
          for (int pl = 0; pl < 2; ++pl) {
            hipError_t e = hipMemsetAsync(s->term[k]->GRc + pl * ev2(nR) + nR, 0, sizeof(double), c->stream);
            if (e != hipSuccess) { hsum_free(s); return fail(MPSK_ERR_HIP, hipGetErrorString(e)); }
          }
    } else {
      // union over the terms of the slabs p = s + d t that carry a fold, per t, padded with a slab empty in every term
      std::vector<char> ru((size_t)d * d, 0), lu((size_t)d * d, 0);
      for (int k = 0; k < n; ++k) {
        const mpsk_mposlice* Hk = H[k];
        for (int t = 0; t < d; ++t)
          for (int si = 0; si < d; ++si) {
            for (int v = 0; v < Hk->Wr; ++v) if (Hk->O(0, t, si, v) != 0.0) ru[si + d * t] = 1;
            for (int w = 1; w < Hk->Wl; ++w) if (Hk->O(w, t, si, Hk->Wr - 1) != 0.0) lu[si + d * t] = 1;
          }
      }
      auto lists = [&](const std::vector<char>& used, std::vector<int>& o, int& nseg) {
        int empty = -1;
        for (int p = 0; p < d * d; ++p) if (!used[p]) { empty = p; break; }
        for (int t = 0; t < d; ++t) {
          int m = 0;
          for (int si = 0; si < d; ++si) m += used[si + d * t];
          nseg = std::max(nseg, m);
        }
        o.assign((size_t)d * nseg, empty);
        for (int t = 0; t < d; ++t) {
          int q = 0;
          for (int si = 0; si < d; ++si) if (used[si + d * t]) o[(size_t)t * nseg + q++] = si + d * t;
        }
      };
      lists(ru, s->up1, h->jn1);
      lists(lu, s->up2, h->jn2);
      h->jp1 = &s->up1; h->jp2 = &s->up2;
      const size_t aR = up32(nR), aL = up32(nL);
      const size_t bytes = sizeof(double) * (aR + aL) + sizeof(int64_t) * 2 * d * (h->jn1 + h->jn2);
      if (int rc = pool_take(c, bytes, &buf, &h->pool_idx)) { hsum_free(s); return rc; }
      h->GRc = (double*)buf;
      h->GLc = h->GRc + aR;
      h->zseg = (int64_t*)(h->GLc + aL);
      hipError_t e = hac_jordan_prepare(c, h, nullptr, nullptr);
      if (e != hipSuccess) { (void)hipStreamSynchronize(c->stream); hsum_free(s); return fail(MPSK_ERR_HIP, hipGetErrorString(e)); }
    }
    s->route = 1;
    if (int rc = hsum_combine(s)) { hsum_free(s); return rc; }
  }
  *out = s;
  return MPSK_OK;
}

int mpsk_hsum_set_coefs(mpsk_hsum* s, const double* coefs) {
  REQUIRE(s && coefs, "NULL argument");
  for (int k = 0; k < s->n; ++k) s->coef[k] = coefs[k];
  return s->route == 1 ? hsum_combine(s) : MPSK_OK;
}

int mpsk_hsum_apply(mpsk_hsum* s, const void* x, void* y) {
  REQUIRE(s && x && y, "NULL argument");
  REQUIRE(x != y, "x and y must not alias");
  if (s->route == 1) return hac_apply_ab(s->sum, x, 1, y, 1.0, 0.0);
  for (int k = 0; k < s->n; ++k)
    if (int rc = hac_apply_ab(s->term[k], x, 1, y, s->coef[k], k ? 1.0 : 0.0)) return rc;
  return MPSK_OK;
}

int mpsk_hsum_apply_axpby(mpsk_hsum* s, const double* a1, const void* x, const double* a0, void* y) {
  REQUIRE(s && x && y && a0 && a1, "NULL argument");
  const mpsk_hac* h = s->term[0];
  const bool cplx = h->H->dtype == MPSK_C128;
  const bool shift = a0[0] != 0.0 || (cplx && a0[1] != 0.0);
  const bool scale = a1[0] != 1.0 || (cplx && a1[1] != 0.0);
  REQUIRE(!shift || h->Dlo == h->Dl, "a shift needs a square operator (Dlo == Dl)");
  if (int rc = mpsk_hsum_apply(s, x, y)) return rc;
  if (!shift && !scale) return MPSK_OK;
  const int64_t nel = (int64_t)h->Dlo * h->H->d * h->Dr;
  if (cplx) {
    HIPCHK(vec_axpby_c(a0, shift ? (const double*)x : nullptr, a1, (double*)y, nel, s->ctx->stream));
  } else if (shift) {
    HIPCHK(vec_axpby(a0[0], (const double*)x, a1[0], (double*)y, nel, s->ctx->stream));
  } else {
    HIPCHK(vec_scal(a1[0], (double*)y, nel, s->ctx->stream));
  }
  return MPSK_OK;
}

// GEMM launches of one application (the planar copy of x of a complex operator and the slab mix are not GEMMs)
static int hac_gemm_launches(const mpsk_hac* h) {
  if (h->mode == 3) return h->H->dtype == MPSK_C128 ? 2 : h->launches;
  if (h->mode == 4) return 3;
  return 2;
}

int mpsk_hsum_info(const mpsk_hsum* s, int* route, int* launches_per_apply) {
  REQUIRE(s, "hsum is NULL");
  if (route) *route = s->route;
  if (launches_per_apply) {
    int m = 0;
    if (s->route == 1) m = hac_gemm_launches(s->sum);
    else for (int k = 0; k < s->n; ++k) m += hac_gemm_launches(s->term[k]);
    *launches_per_apply = m;
  }
  return MPSK_OK;
}

int mpsk_hsum_destroy(mpsk_hsum* s) {
  if (s) hsum_free(s);
  return MPSK_OK;
}

// Fixed-budget smallest-real solve with the prepared operator, one call per site (fixedpoint(H_AC, AC, :SR, alg) of
// dmrg.jl:36 with Arnoldi(; krylovdim = m, maxiter = 1) and no convergence test): V[0] = x0 / |x0|, m Krylov steps
// (apply, CGS2 + normalise), Ritz step of the m x m projected matrix on the device, y = normalised Ritz vector.  Nothing is
// read back; the ~30 entry-point calls the host made per site become one (at D = 256 the host could not keep the stream fed).
// V: HOST array of m + 2 device vectors of the operator's size (Krylov basis + assembly scratch); scal: device scratch of
// >= m (2m + 1) + 40 doubles; first_image (optional): receives H (x0 / |x0|) before it is orthogonalised (calc_galerkin of the
// old tensor needs exactly that vector, toolbox.jl:18).  MPSK_F64 operators, unblocked vector layout.
int mpsk_hac_eigsolve_fixed(mpsk_hac* h, const void* x0, int m, void* const* V, void* scal, void* y, void* first_image) {
  REQUIRE(h && x0 && V && scal && y, "NULL argument");
  REQUIRE(m >= 1 && m <= 32, "needs 1 <= m <= 32");
  REQUIRE(h->H->dtype == MPSK_F64, "mpsk_hac_eigsolve_fixed: MPSK_F64 operators only");
  mpsk_ctx* c = h->ctx;
  HIPCHK(hipSetDevice(c->device));
  const int64_t n = (int64_t)h->Dlo * h->H->d * h->Dr;
  REQUIRE(h->Dlo == h->Dl, "mpsk_hac_eigsolve_fixed: the operator must be square (unsharded)");
  double* slot = (double*)scal;
  const int stride = 2 * m + 1;
  double* rbuf = slot + (size_t)m * stride;           // Ritz coefficients [0:32], info [32:35]
  if (int rc = mpsk_vnormalize_dev(c, n, x0, V[0], nullptr)) return rc;
  for (int k = 0; k < m; ++k) {
    if (int rc = mpsk_hac_apply(h, V[k], 1, V[k + 1])) return rc;
    if (k == 0 && first_image) HIPCHK(hipMemcpyAsync(first_image, V[1], sizeof(double) * n, hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(vec_cgs2((const double* const*)V, k + 1, (double*)V[k + 1], n, slot + (size_t)k * stride, c->d_partial, c->stream));
    HIPCHK(vec_scal_rsqrt_dev(slot + (size_t)k * stride + 2 * (k + 1), (double*)V[k + 1], n, c->stream));
  }
  HIPCHK(vec_ritz_small(slot, m, stride, rbuf, rbuf + 32, c->stream));
  HIPCHK(hipMemsetAsync(V[m + 1], 0, sizeof(double) * n, c->stream));
  HIPCHK(vec_multiaxpy((const double* const*)V, rbuf, m, 1.0, (double*)V[m + 1], n, c->stream));
  return mpsk_vnormalize_dev(c, n, V[m + 1], y, nullptr);
}

}  // extern "C"

// y = sum_w GL[w] c GR[w] with GR slabs [Dr, Dro]: one batched GEMM T[w] = GL[w] c, then the segmented-K GEMM over (w, b).
// mpsk_dC passes Dro = Dr, mpsk_dC_proj the bond dimension of the state below.
static int dC_f64(mpsk_ctx* c, int W, int Dlo, int Dl, int Dr, int Dro, const double* GL, const double* GR, const double* cm,
                  double* y) {
  HIPCHK(hipSetDevice(c->device));
  const size_t slab = (size_t)Dlo * Dr;
  Ws ws;
  const size_t o_t1 = ws.take(slab * W);
  if (int rc = ws.ensure(c)) return rc;
  double* T1 = Ws::at(c, o_t1);
  HIPCHK(stage1(c, W, Dlo, Dl, Dr, GL, cm, T1, 1));
  Segs sg;
  level_segs(sg, W, (int64_t)slab, (int64_t)Dr * Dro);
  GemmArgs g3 = mk(T1, GR, y, Dlo, Dro, Dr, Dlo, Dr, Dlo);
  g3.tag = 1;
  HIPCHK(gemm_segments(g3, sg, c->stream));
  return MPSK_OK;
}

extern "C" {
int mpsk_dC(mpsk_ctx* c, int W, int Dlo, int Dl, int Dr, const void* GL, const void* GR, const void* cm, void* y) {
  REQUIRE(c && GL && GR && cm && y, "NULL argument");
  REQUIRE(W > 0 && Dlo > 0 && Dl > 0 && Dr > 0, "dimensions must be positive");
  if (c->dtype == MPSK_C128)
    return dC_c128(c, W, Dlo, Dl, Dr, Dr, (const double*)GL, (const double*)GR, (const double*)cm, (double*)y);
  return dC_f64(c, W, Dlo, Dl, Dr, Dr, (const double*)GL, (const double*)GR, (const double*)cm, (double*)y);
}

// c_proj (derivatives.jl:204-207): the zero-site map with a rectangular right environment, GR slabs [Dr, Dro] (ket leg of the
// state above, bra leg of the state below).  Dro = Dr is mpsk_dC launch for launch.
int mpsk_dC_proj(mpsk_ctx* c, int W, int Dlo, int Dl, int Dr, int Dro, const void* GL, const void* GR, const void* cm,
                 void* y) {
  REQUIRE(c && GL && GR && cm && y, "NULL argument");
  REQUIRE(W > 0 && Dlo > 0 && Dl > 0 && Dr > 0 && Dro > 0, "dimensions must be positive");
  if (c->dtype == MPSK_C128) return fail(MPSK_ERR_UNSUPPORTED, "mpsk_dC_proj: implemented for MPSK_F64 only");
  return dC_f64(c, W, Dlo, Dl, Dr, Dro, (const double*)GL, (const double*)GR, (const double*)cm, (double*)y);
}

// c_proj on interleaved complex128 operands: the body of the complex mpsk_dC with GR slabs [Dr, Dro]; nothing is conjugated.
int mpsk_dC_proj_c(mpsk_ctx* c, int W, int Dlo, int Dl, int Dr, int Dro, const void* GL, const void* GR, const void* cm,
                   void* y) {
  REQUIRE(c && GL && GR && cm && y, "NULL argument");
  REQUIRE(W > 0 && Dlo > 0 && Dl > 0 && Dr > 0 && Dro > 0, "dimensions must be positive");
  if (c->dtype != MPSK_C128) return fail(MPSK_ERR_UNSUPPORTED, "mpsk_dC_proj_c: the ctx must be set to MPSK_C128");
  return dC_c128(c, W, Dlo, Dl, Dr, Dro, (const double*)GL, (const double*)GR, (const double*)cm, (double*)y);
}

int mpsk_dAC2(mpsk_ctx* c, const mpsk_mposlice* H1, const mpsk_mposlice* H2, int Dlo, int Dl, int Dr,
              const void* GL, const void* GR, const void* x2, void* y2) {
  REQUIRE(c && H1 && H2 && GL && GR && x2 && y2, "NULL argument");
  REQUIRE(H1->Wr == H2->Wl, "MPO bond dimensions of the two slices do not match");
  REQUIRE(Dlo > 0 && Dl > 0 && Dr > 0, "dimensions must be positive");
  REQUIRE(H1->dtype == H2->dtype, "the two slices have different scalar types");
  if (H1->dtype == MPSK_C128)
    return dAC2_c128(c, H1, H2, Dlo, Dl, Dr, Dr, (const double*)GL, (const double*)GR, (const double*)x2, (double*)y2);
  HIPCHK(hipSetDevice(c->device));
  const int d1 = H1->d, d2 = H2->d, Wl = H1->Wl, Wr = H2->Wr;
  const size_t plane = (size_t)Dlo * d1 * Dr;      // one s2-plane
  const size_t slab = plane * d2;                  // one w
  Ws ws;
  const size_t o_t1 = ws.take(slab * Wl), o_t2 = ws.take(slab * Wr);
  if (int rc = ws.ensure(c)) return rc;
  double *T1 = Ws::at(c, o_t1), *T2 = Ws::at(c, o_t2);
  const MixPlan* plan = nullptr;
  if (int rc = pair_plan(c, H1, H2, &plan)) return rc;
  HIPCHK(stage1(c, Wl, Dlo, Dl, d1 * Dr * d2, (const double*)GL, (const double*)x2, T1, 1));
  SlabIndex ix{d1, d2, (int64_t)Dlo, (int64_t)plane, (int64_t)slab, (int64_t)Dlo * d1};
  HIPCHK(mix_apply(*plan, T1, ix, T2, ix, Dlo, Dr, c->stream));
  Segs sg;
  if (!level_segs(sg, Wr, (int64_t)slab, (int64_t)Dr * Dr, &H2->col_used)) return zero_fill(c, y2, sizeof(double) * slab);
  GemmArgs g3 = mk(T2, (const double*)GR, (double*)y2, Dlo * d1, Dr, Dr, (int64_t)Dlo * d1, Dr, (int64_t)Dlo * d1);
  g3.tag = 1;
  g3.batch = d2; g3.bsA = (int64_t)plane; g3.bsB = 0; g3.bsC = (int64_t)plane;
  HIPCHK(gemm_segments(g3, sg, c->stream));
  return MPSK_OK;
}

}  // extern "C"

// --------------------------------------------------------------------------------------------
// transfers
// --------------------------------------------------------------------------------------------
// ---- canonical transfers of a Jordan-form slice (mpsk_transfer_left_ex / mpsk_transfer_right_ex) ----------------------
// With level 0 of GLin the identity and A = Ab a left isometry (sum_{p,t} A[p,t,q] A[p,t,b] = delta_qb) the levels of
//   GLout[v][q,b] = sum GLin[w][p,a] A[a,s,b] O[w,t,s,v] A[p,t,q]
// decouple, because a Jordan-form O feeds v < W-1 from level 0 alone:
//   v = 0          GLout[0] = A^T A = 1                                                   written, not computed
//   0 < v < W-1    GLout[v] = A^T T2[v],  T2[v][:,t,:] = sum_s O[0,t,s,v] A[:,s,:]        one elementwise pass, no stage 1
//   v = W-1        GLout[W-1] = A^T T,    T[:,t,:] = sum_s GLc[(s,t)] A[:,s,:] + sum_s O[0,t,s,W-1] A[:,s,:]
// with GLc the left fold of mpsk_hac mode 3 (hac_jordan_prepare), applied by the per-batch-table GEMM of that mode.  T is
// the last slab of T2, so ONE batched TN GEMM produces the levels 1 .. W-1.  Heisenberg: 8 D^3 (fold) + 16 D^3 instead of
// 20 D^3 + 20 D^3.  transfer_right is the mirror image: level W-1 is the identity, 0 < w < W-1 come from the B blocks
// alone, X[w][:,t,:] = sum_s O[w,t,s,W-1] A[:,s,:], level 0 from the right fold, X[0][:,t,:] = sum_s A[:,s,:] GRc0[(s,t)]
// (start level, C blocks and the D block), and GRout[w][a,p] = sum_{t,b} X[w][a,t,b] A[p,t,b] is one batched NT GEMM.
// MPSK_TRANSFER_MODE=0 keeps the dense three-stage route (A/B runs).
static bool transfer_canonical_ok(const mpsk_mposlice* H, int flags, const void* A, const void* Ab, int Dl, int Dr,
                                  int Dlb, int Drb) {
  if (!(flags & MPSK_TRANSFER_CANONICAL) || !H || !H->jordan || H->dtype != MPSK_F64 || dense_route(H)) return false;
  if (A != Ab || Dl != Dlb || Dr != Drb) return false;
  const char* ev = getenv("MPSK_TRANSFER_MODE");
  return !(ev && ev[0] == '0');
}

// Which canonical route: the pair-Gram form of the interior levels (PairPlan) or the level-by-level one.
// MPSK_TRANSFER_MODE (read per call): 1 = level by level, 2 = pair-Gram wherever the slice has a pair plan (A/B runs and
// tests at shapes the model would not send there), unset = pair_route_pays.
static bool transfer_pair_route(const mpsk_mposlice* H, bool left, int Dl, int Dr) {
  const PairPlan& pp = left ? H->pl : H->pr;
  if (pp.np == 0) return false;
  if (const char* ev = getenv("MPSK_TRANSFER_MODE")) {
    if (ev[0] == '1') return false;
    if (ev[0] == '2') return true;
  }
  return left ? pair_route_pays(pp, H->Wr - 2, H->d, Dl, Dr) : pair_route_pays(pp, H->Wl - 2, H->d, Dr, Dl);
}

// device offset tables [2][np] of the pair batch, cached on the slice per Dl: operand offsets i Dl and j Dl into A
static int pair_tab(const mpsk_mposlice* H, bool left, int Dl, const int64_t** out) {
  const PairPlan& pp = left ? H->pl : H->pr;
  return (left ? H->ptabL : H->ptabR).get({Dl}, [&](std::vector<int64_t>& h) {
    h.resize((size_t)2 * pp.np);
    for (int p = 0; p < pp.np; ++p) { h[p] = (int64_t)pp.i[p] * Dl; h[(size_t)pp.np + p] = (int64_t)pp.j[p] * Dl; }
  }, "pair offset table", out);
}

// M_p = op(A_i) op(A_j) for every pair of the plan, ONE launch: left P_ij = A_i^T A_j (TN, K = Dl, Dr x Dr), right
// Q_ij = A_i A_j^T (NT, K = Dr, Dl x Dl), A_s = A[:, s, :] (leading dimension Dl d).  The symmetric products come first
// in the batch and skip their lower tiles (GemmArgs::upper_nb); pair_combine reads them through the upper triangle.
static int pair_products(mpsk_ctx* c, const mpsk_mposlice* H, bool left, int Dl, int Dr, const double* A, double* P) {
  const PairPlan& pp = left ? H->pl : H->pr;
  const int64_t* tab = nullptr;
  if (int rc = pair_tab(H, left, Dl, &tab)) return rc;
  const int n = left ? Dr : Dl, K = left ? Dl : Dr;
  const int64_t ld = (int64_t)Dl * H->d;
  GemmArgs g = mk(A, A, P, n, n, K, ld, ld, n, left ? 1 : 0, left ? 0 : 1);
  g.batch = pp.np; g.tabA = tab; g.tabB = tab + pp.np; g.bsC = (int64_t)n * n;
  g.tabs_even = Dl % 2 == 0;
  if (pp.ndiag > 0) { g.upper_only = 1; g.upper_nb = pp.ndiag; }
  HIPCHK(gemm_f64(g, c->stream));
  return MPSK_OK;
}

// MPSK_HAC_CHECK=1 (debug, synchronises): the promises behind MPSK_TRANSFER_CANONICAL -- the identity level of the input
// environment (n x n at G) and the isometry of A on the contracted side (Gram matrix through c->ws) -- hold to 1e-10
static int transfer_canonical_check(mpsk_ctx* c, const char* who, const double* G, int n, const double* A, int d, int Dl,
                                    int Dr, bool left) {
  double dg = 0.0, da = 0.0;
  if (int rc = identity_deviation(c, G, n, &dg)) return rc;
  const int m = left ? Dr : Dl;
  Ws ws;
  const size_t o_gram = ws.take((size_t)m * m);
  if (int rc = ws.ensure(c)) return rc;
  double* gram = Ws::at(c, o_gram);
  if (left) {        // A^T A over (p, t)
    GemmArgs g = mk(A, A, gram, Dr, Dr, Dl * d, (int64_t)Dl * d, (int64_t)Dl * d, Dr, 1, 0);
    HIPCHK(gemm_f64(g, c->stream));
  } else {           // A A^T over (t, b)
    Segs sg;
    phys_segs(sg, d, Dl, Dl);
    GemmArgs g = mk(A, A, gram, Dl, Dl, Dr, (int64_t)Dl * d, (int64_t)Dl * d, Dl, 0, 1);
    HIPCHK(gemm_segments(g, sg, c->stream));
  }
  if (int rc = identity_deviation(c, gram, m, &da)) return rc;
  if (!(dg <= 1e-10 && da <= 1e-10)) {
    char msg[200];
    snprintf(msg, sizeof(msg), "MPSK_HAC_CHECK: %s is not canonical (max|G[identity level] - I| = %.3e, max|%s - I| = %.3e)",
             who, dg, left ? "A^T A" : "A A^T", da);
    return fail(MPSK_ERR_INVALID, msg);
  }
  return MPSK_OK;
}

// device segment tables [2][d][nseg] of the fold applications, cached on the slice per shape
static int jordan_tab(const mpsk_mposlice* H, bool left, int Dl, int Dr, const int64_t** out) {
  const int d = H->d, n = left ? H->jl_nseg : H->jr_nseg;
  const std::vector<int>& plist = left ? H->jl_p : H->jr_p;
  const int64_t tL = (int64_t)Dl * d * Dl, tR = (int64_t)Dr * d * Dr;
  auto build = [&](std::vector<int64_t>& h) {
    h.resize((size_t)2 * d * n);
    for (int t = 0; t < d; ++t)
      for (int k = 0; k < n; ++k) {
        const int p = plist[(size_t)t * n + k], si = p % d, tt = p / d;
        if (left) { h[(size_t)t * n + k] = tt * tL + (int64_t)si * Dl; h[(size_t)(d + t) * n + k] = (int64_t)si * Dl; }      // GLc[(s,tt)], A[:,s,:]
        else { h[(size_t)t * n + k] = (int64_t)si * Dl; h[(size_t)(d + t) * n + k] = tt * tR + (int64_t)si * Dr; }          // A[:,s,:], GRc0[(s,tt)]
      }
  };
  return left ? H->jtabL.get({Dl}, build, "transfer segment table", out)
              : H->jtabR.get({Dl, Dr}, build, "transfer segment table", out);
}

// Pair-Gram route of transfer_left_canonical.  The interior levels and the D-block term of the finished level are
// combinations of the pair products (pair_combine writes levels 1 .. W-1, or 1 .. W-2 for a slice without a D block); the
// finished level then is a single TN GEMM A^T T of the fold application T = GLc A alone, with beta = 1 on top of the
// D-block term the combination has written (combine first, accumulate second: the GEMM epilogue reads C anyway, the
// elementwise kernel stays write-only).  No mix pass over A and no T2 slabs: the workspace is the fold, one slab for T
// and np Dr^2 doubles of products.
static int transfer_left_pairs(mpsk_ctx* c, const mpsk_mposlice* H, int Dl, int Dr, const double* GLin, const double* A,
                               double* GLout) {
  const int d = H->d, Wr = H->Wr, n2 = H->jl_nseg;
  const PairPlan& pp = H->pl;
  const size_t slab = (size_t)Dl * d * Dr, nD = (size_t)Dr * Dr;
  const int64_t tL = (int64_t)Dl * d * Dl;
  Ws ws;
  const size_t o_glc = ws.take((size_t)d * tL, 32), o_t = ws.take(slab, 32), o_p = ws.take(nD * pp.np);
  if (int rc = ws.ensure(c)) return rc;
  const int64_t* tab = nullptr;
  if (int rc = jordan_tab(H, true, Dl, Dr, &tab)) return rc;
  double *GLc = Ws::at(c, o_glc), *T = Ws::at(c, o_t), *P = Ws::at(c, o_p);
  if (int rc = pair_products(c, H, true, Dl, Dr, A, P)) return rc;
  HIPCHK(identity_slab(GLout, Dr, c->stream));
  HIPCHK(pair_combine(P, pp.np, pp.ndiag, Dr, pp.d_coef, pp.nl, GLout + nD, (int64_t)nD, c->stream));
  // GLc[(s,t)] = sum_{w>0} O[w,t,s,W-1] GLin[w];  T[:,t,:] = sum_k GLc[(s_k,t)] A[:,s_k,:]     (batch over t)
  SlabIndex il{1 << 30, 1, (int64_t)Dl * Dl, 0, 0, (int64_t)Dl}, ol{d, 1 << 30, (int64_t)Dl, tL, 0, (int64_t)d * Dl};
  HIPCHK(mix_apply(H->jl, GLin, il, GLc, ol, Dl, Dl, c->stream));
  GemmArgs g = mk(GLc, A, T, Dl, Dr, Dl, (int64_t)Dl * d, (int64_t)Dl * d, (int64_t)Dl * d);
  g.batch = d; g.bsA = 0; g.bsB = 0; g.bsC = (int64_t)Dl;
  g.nseg = n2; g.zsegA = tab; g.zsegB = tab + (size_t)d * n2;
  g.tabs_even = Dl % 2 == 0;
  g.tag = 1;
  HIPCHK(gemm_f64(g, c->stream));
  // GLout[W-1][q,b] (+)= sum_{(p,t)} A[(p,t),q] T[(p,t),b]
  GemmArgs g3 = mk(A, T, GLout + nD * (Wr - 1), Dr, Dr, Dl * d, (int64_t)Dl * d, (int64_t)Dl * d, Dr, 1, 0);
  g3.beta = pp.nl == Wr - 1 ? 1.0 : 0.0;
  HIPCHK(gemm_f64(g3, c->stream));
  c->n_transfer_pair++;
  return MPSK_OK;
}

static int transfer_left_canonical(mpsk_ctx* c, const mpsk_mposlice* H, int Dl, int Dr, const double* GLin, const double* A,
                                   double* GLout) {
  const int d = H->d, Wr = H->Wr, n2 = H->jl_nseg;
  if (hac_check_on())
    if (int rc = transfer_canonical_check(c, "mpsk_transfer_left_ex", GLin, Dl, A, d, Dl, Dr, true)) return rc;
  if (transfer_pair_route(H, true, Dl, Dr)) return transfer_left_pairs(c, H, Dl, Dr, GLin, A, GLout);
  const size_t slab = (size_t)Dl * d * Dr;                  // one level of T2
  const int64_t tL = (int64_t)Dl * d * Dl;                  // one t-group of GLc
  const size_t nL = (size_t)d * tL;
  Ws ws;
  const size_t o_glc = ws.take(nL, 32), o_t2 = ws.take(slab * (Wr - 1));
  if (int rc = ws.ensure(c)) return rc;
  const int64_t* tab = nullptr;
  if (int rc = jordan_tab(H, true, Dl, Dr, &tab)) return rc;
  double* GLc = Ws::at(c, o_glc);
  double* T2 = Ws::at(c, o_t2);                             // slab v - 1 for v = 1 .. Wr-1
  double* T = T2 + slab * (Wr - 2);
  // GLc[(s,t)] = sum_{w>0} O[w,t,s,W-1] GLin[w]
  SlabIndex il{1 << 30, 1, (int64_t)Dl * Dl, 0, 0, (int64_t)Dl}, ol{d, 1 << 30, (int64_t)Dl, tL, 0, (int64_t)d * Dl};
  HIPCHK(mix_apply(H->jl, GLin, il, GLc, ol, Dl, Dl, c->stream));
  // T2[v][:,t,:] = sum_s O[0,t,s,v] A[:,s,:]     (the D-block part of T included when the slice has one)
  SlabIndex ia{1 << 30, 1, (int64_t)Dl, 0, 0, (int64_t)Dl * d}, ot{d, 1 << 30, (int64_t)Dl, (int64_t)slab, 0, (int64_t)Dl * d};
  HIPCHK(mix_apply(H->tl, A, ia, T2, ot, Dl, Dr, c->stream));
  // T[:,t,:] (+)= sum_k GLc[(s_k,t)] A[:,s_k,:]     (batch over t)
  GemmArgs g = mk(GLc, A, T, Dl, Dr, Dl, (int64_t)Dl * d, (int64_t)Dl * d, (int64_t)Dl * d);
  g.batch = d; g.bsA = 0; g.bsB = 0; g.bsC = (int64_t)Dl;
  g.beta = H->tl_dblock ? 1.0 : 0.0;
  g.nseg = n2; g.zsegA = tab; g.zsegB = tab + (size_t)d * n2;
  g.tabs_even = Dl % 2 == 0;
  g.tag = 1;
  HIPCHK(gemm_f64(g, c->stream));
  HIPCHK(identity_slab(GLout, Dr, c->stream));
  // GLout[v][q,b] = sum_{(p,t)} A[(p,t),q] T2[v][(p,t),b]     v = 1 .. Wr-1
  GemmArgs g3 = mk(A, T2, GLout + (size_t)Dr * Dr, Dr, Dr, Dl * d, (int64_t)Dl * d, (int64_t)Dl * d, Dr, 1, 0);
  g3.batch = Wr - 1; g3.bsA = 0; g3.bsB = (int64_t)slab; g3.bsC = (int64_t)Dr * Dr;
  HIPCHK(gemm_f64(g3, c->stream));
  return MPSK_OK;
}

// Pair-Gram route of transfer_right_canonical: the interior levels from the pair products Q_ij = A_i A_j^T, level 0 from
// the right fold (which already holds the D block) as a single NT GEMM over the physical index, beta = 0.
static int transfer_right_pairs(mpsk_ctx* c, const mpsk_mposlice* H, int Dl, int Dr, const double* A, const double* GRin,
                                double* GRout) {
  const int d = H->d, Wl = H->Wl, n1 = H->jr_nseg;
  const PairPlan& pp = H->pr;
  const size_t slab = (size_t)Dl * d * Dr, nD = (size_t)Dl * Dl;
  const int64_t tR = (int64_t)Dr * d * Dr;
  Ws ws;
  const size_t o_grc = ws.take((size_t)d * tR, 32), o_x = ws.take(slab, 32), o_p = ws.take(nD * pp.np);
  if (int rc = ws.ensure(c)) return rc;
  const int64_t* tab = nullptr;
  if (int rc = jordan_tab(H, false, Dl, Dr, &tab)) return rc;
  double *GRc = Ws::at(c, o_grc), *X = Ws::at(c, o_x), *P = Ws::at(c, o_p);
  if (int rc = pair_products(c, H, false, Dl, Dr, A, P)) return rc;
  HIPCHK(identity_slab(GRout + nD * (Wl - 1), Dl, c->stream));
  HIPCHK(pair_combine(P, pp.np, pp.ndiag, Dl, pp.d_coef, pp.nl, GRout + nD, (int64_t)nD, c->stream));
  // GRc0[(s,t)] = sum_v O[0,t,s,v] GRin[v];  X[:,t,:] = sum_k A[:,s_k,:] GRc0[(s_k,t)]     (batch over t)
  SlabIndex ir{1 << 30, 1, (int64_t)Dr * Dr, 0, 0, (int64_t)Dr}, orr{d, 1 << 30, (int64_t)Dr, tR, 0, (int64_t)d * Dr};
  HIPCHK(mix_apply(H->jr, GRin, ir, GRc, orr, Dr, Dr, c->stream));
  GemmArgs g = mk(A, GRc, X, Dl, Dr, Dr, (int64_t)Dl * d, (int64_t)Dr * d, (int64_t)Dl * d);
  g.batch = d; g.bsA = 0; g.bsB = 0; g.bsC = (int64_t)Dl;
  g.nseg = n1; g.zsegA = tab; g.zsegB = tab + (size_t)d * n1;
  g.tabs_even = Dl % 2 == 0 && Dr % 2 == 0;
  g.tag = 1;
  HIPCHK(gemm_f64(g, c->stream));
  // GRout[0][a,p] = sum_t sum_b X[a,t,b] A[p,t,b]
  Segs sg;
  phys_segs(sg, d, Dl, Dl);
  GemmArgs g3 = mk(X, A, GRout, Dl, Dl, Dr, (int64_t)Dl * d, (int64_t)Dl * d, Dl, 0, 1);
  HIPCHK(gemm_segments(g3, sg, c->stream));
  c->n_transfer_pair++;
  return MPSK_OK;
}

static int transfer_right_canonical(mpsk_ctx* c, const mpsk_mposlice* H, int Dl, int Dr, const double* A, const double* GRin,
                                    double* GRout) {
  const int d = H->d, Wl = H->Wl, Wr = H->Wr, n1 = H->jr_nseg;
  if (hac_check_on())
    if (int rc = transfer_canonical_check(c, "mpsk_transfer_right_ex", GRin + (size_t)(Wr - 1) * Dr * Dr, Dr, A, d, Dl, Dr, false))
      return rc;
  if (transfer_pair_route(H, false, Dl, Dr)) return transfer_right_pairs(c, H, Dl, Dr, A, GRin, GRout);
  const size_t slab = (size_t)Dl * d * Dr;                  // one level of X
  const int64_t tR = (int64_t)Dr * d * Dr;                  // one t-group of GRc0
  const size_t nR = (size_t)d * tR;
  Ws ws;
  const size_t o_grc = ws.take(nR, 32), o_x = ws.take(slab * (Wl - 1));
  if (int rc = ws.ensure(c)) return rc;
  const int64_t* tab = nullptr;
  if (int rc = jordan_tab(H, false, Dl, Dr, &tab)) return rc;
  double* GRc = Ws::at(c, o_grc);
  double* X = Ws::at(c, o_x);                               // slab w for w = 0 .. Wl-2
  // GRc0[(s,t)] = sum_v O[0,t,s,v] GRin[v]
  SlabIndex ir{1 << 30, 1, (int64_t)Dr * Dr, 0, 0, (int64_t)Dr}, orr{d, 1 << 30, (int64_t)Dr, tR, 0, (int64_t)d * Dr};
  HIPCHK(mix_apply(H->jr, GRin, ir, GRc, orr, Dr, Dr, c->stream));
  // X[w][:,t,:] = sum_s O[w,t,s,W-1] A[:,s,:]     w = 1 .. Wl-2
  SlabIndex ia{1 << 30, 1, (int64_t)Dl, 0, 0, (int64_t)Dl * d}, ox{d, 1 << 30, (int64_t)Dl, (int64_t)slab, 0, (int64_t)Dl * d};
  HIPCHK(mix_apply(H->tr, A, ia, X + slab, ox, Dl, Dr, c->stream));
  // X[0][:,t,:] = sum_k A[:,s_k,:] GRc0[(s_k,t)]     (batch over t)
  GemmArgs g = mk(A, GRc, X, Dl, Dr, Dr, (int64_t)Dl * d, (int64_t)Dr * d, (int64_t)Dl * d);
  g.batch = d; g.bsA = 0; g.bsB = 0; g.bsC = (int64_t)Dl;
  g.nseg = n1; g.zsegA = tab; g.zsegB = tab + (size_t)d * n1;
  g.tabs_even = Dl % 2 == 0 && Dr % 2 == 0;
  g.tag = 1;
  HIPCHK(gemm_f64(g, c->stream));
  HIPCHK(identity_slab(GRout + (size_t)(Wl - 1) * Dl * Dl, Dl, c->stream));
  // GRout[w][a,p] = sum_t sum_b X[w][a,t,b] A[p,t,b]     w = 0 .. Wl-2
  Segs sg;
  phys_segs(sg, d, Dl, Dl);
  GemmArgs g3 = mk(X, A, GRout, Dl, Dl, Dr, (int64_t)Dl * d, (int64_t)Dl * d, Dl, 0, 1);
  g3.batch = Wl - 1; g3.bsA = (int64_t)slab; g3.bsB = 0; g3.bsC = (int64_t)Dl * Dl;
  HIPCHK(gemm_segments(g3, sg, c->stream));
  return MPSK_OK;
}

// gram (pass-through only, Dr == Drb): gram[w][t,s] = sum Ab[p,t,b] T1[w][p,s,b] of the stage-1 product, partials after
// T1 in the workspace; GLout == nullptr then skips stage 2 (mpsk_transfer_left_gram)
// envR (with gram, Wl == 1): as in transfer_left_c128
static int transfer_left_f64(mpsk_ctx* c, const mpsk_mposlice* H, int Wl, int Wr, int d, int Dl, int Dr, int Dlb, int Drb,
                             const void* GLin, const void* A, const void* Ab, void* GLout, double* gram,
                             const double* envR = nullptr, const double* V2 = nullptr, const double* A2 = nullptr,
                             int Dl2 = 0) {
  const size_t slab = (size_t)Dlb * d * Dr;
  Ws ws;
  const size_t o_t = ws.take(slab * (Wl + (H ? Wr : 0)), gram ? 32 : 1);      // T1, then T2 when there is a mix
  const size_t o_part = ws.take(gram ? site_gram_partial_doubles(Wl, d, false) : 0);
  if (int rc = ws.ensure(c)) return rc;
  double* T1 = Ws::at(c, o_t);
  double* T2 = H ? T1 + slab * Wl : T1;
  HIPCHK(stage1(c, Wl, Dlb, Dl, d * Dr, (const double*)GLin, (const double*)A, T1, 0));      // T1[w][p,s,b] = sum_a GLin[w][p,a] A[a,s,b]
  if (V2) HIPCHK(stage1(c, Wl, Dlb, Dl2, d * Dr, V2, A2, T1, 0, 1, 0, 1.0));                 // T1[w] += V2[w] A2  (the pair transfer)
  if (H) HIPCHK(mix_levels(c, H->fwd, d, Dlb, Dr, T1, T2));
  if (gram && envR)
    HIPCHK(gram_env(d, Dlb, Dr, Drb, T1, envR, 0, (const double*)Ab, false, gram, Ws::at(c, o_part), c->stream));
  else if (gram) HIPCHK(site_gram(Wl, d, Dlb, Dr, T1, (const double*)Ab, false, gram, Ws::at(c, o_part), c->stream));
  if (!GLout) return MPSK_OK;
  // GLout[v][q,b] = sum_{(p,t)} Ab[(p,t),q] T2[v][(p,t),b]
  GemmArgs g3 = mk((const double*)Ab, T2, (double*)GLout, Drb, Dr, Dlb * d, (int64_t)Dlb * d, (int64_t)Dlb * d, Drb, 1, 0);
  g3.batch = Wr; g3.bsA = 0; g3.bsB = (int64_t)slab; g3.bsC = (int64_t)Drb * Dr;
  HIPCHK(gemm_f64(g3, c->stream));
  return MPSK_OK;
}

extern "C" {
int mpsk_transfer_left_ex(mpsk_ctx* c, const mpsk_mposlice* H, int W, int d, int Dl, int Dr, int Dlb, int Drb,
                          const void* GLin, const void* A, const void* Ab, int flags, void* GLout) {
  REQUIRE(c && GLin && A && Ab && GLout, "NULL argument");
  REQUIRE((flags & ~MPSK_TRANSFER_CANONICAL) == 0, "unknown flags");
  if (transfer_canonical_ok(H, flags, A, Ab, Dl, Dr, Dlb, Drb)) {
    REQUIRE(Dl > 0 && Dr > 0, "dimensions must be positive");
    HIPCHK(hipSetDevice(c->device));
    return transfer_left_canonical(c, H, Dl, Dr, (const double*)GLin, (const double*)A, (double*)GLout);
  }
  return mpsk_transfer_left(c, H, W, d, Dl, Dr, Dlb, Drb, GLin, A, Ab, GLout);
}

int mpsk_transfer_right_ex(mpsk_ctx* c, const mpsk_mposlice* H, int W, int d, int Dl, int Dr, int Dlb, int Drb,
                           const void* A, const void* Ab, const void* GRin, int flags, void* GRout) {
  REQUIRE(c && GRin && A && Ab && GRout, "NULL argument");
  REQUIRE((flags & ~MPSK_TRANSFER_CANONICAL) == 0, "unknown flags");
  if (transfer_canonical_ok(H, flags, A, Ab, Dl, Dr, Dlb, Drb)) {
    REQUIRE(Dl > 0 && Dr > 0, "dimensions must be positive");
    HIPCHK(hipSetDevice(c->device));
    return transfer_right_canonical(c, H, Dl, Dr, (const double*)A, (const double*)GRin, (double*)GRout);
  }
  return mpsk_transfer_right(c, H, W, d, Dl, Dr, Dlb, Drb, A, Ab, GRin, GRout);
}

int mpsk_ctx_transfer_stats(mpsk_ctx* c, long* n_pair) {
  REQUIRE(c, "ctx is NULL");
  if (n_pair) *n_pair = c->n_transfer_pair;
  return MPSK_OK;
}

int mpsk_transfer_pair_model(int Wl, int Wr, int d, const double* O, int Dl, int Dr, int* pairs, int* diagonal, int* levels,
                             int* route) {
  REQUIRE(O && Wl >= 2 && Wr >= 2 && d > 0 && Dl > 0 && Dr > 0, "O is NULL or a dimension is out of range");
  for (int side = 0; side < 2; ++side) {
    PairPlan pp;
    pair_plan_build(Wl, Wr, d, O, side == 0, &pp);
    if (pairs) pairs[side] = pp.np;
    if (diagonal) diagonal[side] = pp.ndiag;
    if (levels) levels[side] = pp.nl;
    if (route) route[side] = (side == 0 ? pair_route_pays(pp, Wr - 2, d, Dl, Dr) : pair_route_pays(pp, Wl - 2, d, Dr, Dl)) ? 1 : 0;
  }
  return MPSK_OK;
}

int mpsk_transfer_left(mpsk_ctx* c, const mpsk_mposlice* H, int W, int d, int Dl, int Dr, int Dlb, int Drb,
                       const void* GLin, const void* A, const void* Ab, void* GLout) {
  REQUIRE(c && GLin && A && Ab && GLout, "NULL argument");
  HIPCHK(hipSetDevice(c->device));
  int Wl, Wr;
  site_dims(H, W, Wl, Wr, d);
  REQUIRE(Wl > 0 && d > 0 && Dl > 0 && Dr > 0 && Dlb > 0 && Drb > 0, "dimensions must be positive");
  if ((H ? H->dtype : c->dtype) == MPSK_C128)
    return transfer_left_c128(c, H, Wl, Wr, d, Dl, Dr, Dlb, Drb, (const double*)GLin, (const double*)A, (const double*)Ab,
                              (double*)GLout);
  if (dense_route(H))
    return transfer_left_dense(c, H, Dl, Dr, Dlb, Drb, (const double*)GLin, (const double*)A, (const double*)Ab, (double*)GLout);
  return transfer_left_f64(c, H, Wl, Wr, d, Dl, Dr, Dlb, Drb, GLin, A, Ab, GLout, nullptr);
}

// The pass-through left transfer plus the site Gram of its stage-1 product: one site of a correlator
// (correlators.jl:10-43).  Vout == NULL: last site of a range, stage 2 is skipped.
int mpsk_transfer_left_gram(mpsk_ctx* c, int W, int d, int Dl, int Dr, int Dlb, int Drb, const void* Vin, const void* A,
                            const void* Ab, void* Vout, void* dev_gram) {
  REQUIRE(c && Vin && A && Ab && dev_gram, "NULL argument");
  REQUIRE(W > 0 && d > 0 && Dl > 0 && Dr > 0 && Dlb > 0 && Drb > 0, "dimensions must be positive");
  REQUIRE(Dr == Drb, "the Gram of the intermediate needs Dr == Drb");
  HIPCHK(hipSetDevice(c->device));
  if (c->dtype == MPSK_C128)
    return transfer_left_c128(c, nullptr, W, W, d, Dl, Dr, Dlb, Drb, (const double*)Vin, (const double*)A, (const double*)Ab,
                              (double*)Vout, (double*)dev_gram);
  return transfer_left_f64(c, nullptr, W, W, d, Dl, Dr, Dlb, Drb, Vin, A, Ab, Vout, (double*)dev_gram);
}

// One site of the matrix elements <bra| O_j |ket> of two states on the same environments (window.transition): the
// pass-through transfer of Lin over (A, Ab) plus dev_gram[t,s] = sum conj(Ab[p,t,q]) Lin[p,a] A[a,s,b] R[b,q], closed on
// the right with R [Dr, Drb].  The stages of Lout are those of mpsk_transfer_left(NULL, W = 1).
int mpsk_transfer_left_gram_env(mpsk_ctx* c, int d, int Dl, int Dr, int Dlb, int Drb, const void* Lin, const void* A,
                                const void* Ab, const void* R, void* Lout, void* dev_gram) {
  REQUIRE(c && Lin && A && Ab && R && dev_gram, "NULL argument");
  REQUIRE(d > 0 && Dl > 0 && Dr > 0 && Dlb > 0 && Drb > 0, "dimensions must be positive");
  REQUIRE(d <= gram_env_max_d(), "physical dimension above the limit of the fused closing product");
  HIPCHK(hipSetDevice(c->device));
  if (c->dtype == MPSK_C128)
    return transfer_left_c128(c, nullptr, 1, 1, d, Dl, Dr, Dlb, Drb, (const double*)Lin, (const double*)A, (const double*)Ab,
                              (double*)Lout, (double*)dev_gram, (const double*)R);
  return transfer_left_f64(c, nullptr, 1, 1, d, Dl, Dr, Dlb, Drb, Lin, A, Ab, Lout, (double*)dev_gram, (const double*)R);
}

// dev_out[w][t,s] = sum_{p,b} conj(Ab[p,t,b]) X[w][p,s,b]: the one-site reduced density matrix for X = Ab = AC
// (expval.jl:23-37).  Asynchronous; the result stays on the device.
int mpsk_site_gram(mpsk_ctx* c, int W, int d, int Dl, int Dr, const void* X, const void* Ab, void* dev_out) {
  REQUIRE(c && X && Ab && dev_out, "NULL argument");
  REQUIRE(W > 0 && d > 0 && Dl > 0 && Dr > 0, "dimensions must be positive");
  HIPCHK(hipSetDevice(c->device));
  const bool cplx = c->dtype == MPSK_C128;
  Ws ws;
  const size_t o_part = ws.take(site_gram_partial_doubles(W, d, cplx));
  if (int rc = ws.ensure(c)) return rc;
  HIPCHK(site_gram(W, d, Dl, Dr, (const double*)X, (const double*)Ab, cplx, (double*)dev_out, Ws::at(c, o_part), c->stream));
  return MPSK_OK;
}

int mpsk_transfer_right(mpsk_ctx* c, const mpsk_mposlice* H, int W, int d, int Dl, int Dr, int Dlb, int Drb,
                        const void* A, const void* Ab, const void* GRin, void* GRout) {
  REQUIRE(c && GRin && A && Ab && GRout, "NULL argument");
  HIPCHK(hipSetDevice(c->device));
  int Wl, Wr;
  site_dims(H, W, Wl, Wr, d);
  REQUIRE(Wl > 0 && d > 0 && Dl > 0 && Dr > 0 && Dlb > 0 && Drb > 0, "dimensions must be positive");
  if ((H ? H->dtype : c->dtype) == MPSK_C128)
    return transfer_right_c128(c, H, Wl, Wr, d, Dl, Dr, Dlb, Drb, (const double*)A, (const double*)Ab, (const double*)GRin,
                               (double*)GRout);
  const size_t plane = (size_t)Dr * Dlb;   // one physical index
  const size_t slab = plane * d;
  Ws ws;
  const size_t o_u = ws.take(slab * Wr), o_v = ws.take(H ? slab * Wl : 0);
  if (int rc = ws.ensure(c)) return rc;
  double *U = Ws::at(c, o_u), *V = H ? Ws::at(c, o_v) : U;
  // U[v][b,p,t] = sum_q GRin[v][b,q] Ab[(p,t),q]
  GemmArgs g1 = mk((const double*)GRin, (const double*)Ab, U, Dr, Dlb * d, Drb, Dr, (int64_t)Dlb * d, Dr, 0, 1);
  g1.batch = Wr; g1.bsA = (int64_t)Dr * Drb; g1.bsB = 0; g1.bsC = (int64_t)slab;
  HIPCHK(gemm_f64(g1, c->stream));
  if (H && dense_route(H)) {
    // V[(b,p), (s,w)] = U[(b,p), (t,v)] Od^T   (U / V are already the two-index views the GEMM needs)
    GemmArgs g2 = mk(U, H->d_Od, V, (int)plane, d * Wl, d * Wr, (int64_t)plane, (int64_t)d * Wl, (int64_t)plane, 0, 1);
    HIPCHK(gemm_f64(g2, c->stream));
  } else if (H) {
    SlabIndex ix{d, 1 << 30, (int64_t)plane, (int64_t)slab, 0, (int64_t)Dr};
    HIPCHK(mix_apply(H->bwd, U, ix, V, ix, Dr, Dlb, c->stream));
  }
  // GRout[w][a,p] = sum_s sum_b A[a,s,b] V[w][s][b,p]
  Segs sg;
  phys_segs(sg, d, Dl, (int64_t)plane);
  GemmArgs g3 = mk((const double*)A, V, (double*)GRout, Dl, Dlb, Dr, (int64_t)Dl * d, Dr, Dl);
  g3.batch = Wl; g3.bsA = 0; g3.bsB = (int64_t)slab; g3.bsC = (int64_t)Dl * Dlb;
  HIPCHK(gemm_segments(g3, sg, c->stream));
  return MPSK_OK;
}

int mpsk_regularize(mpsk_ctx* c, int W, int D1, int D2, void* v, const void* lvec, const void* rvec) {
  REQUIRE(c && v && lvec && rvec, "NULL argument");
  REQUIRE(W > 0 && D1 > 0 && D2 > 0, "dimensions must be positive");
  HIPCHK(hipSetDevice(c->device));
  if (int rc = ensure_ws(c, sizeof(double) * regularize_workspace_doubles(W, D1, D2))) return rc;
  HIPCHK(regularize(W, D1, D2, (double*)v, (const double*)lvec, (const double*)rvec, c->ws.d(), c->stream));
  return MPSK_OK;
}

int mpsk_regularize_axpby(mpsk_ctx* c, int W, int D1, int D2, const void* y, const void* lvec, const void* rvec, double a1,
                          const void* x, double a0, void* out) {
  REQUIRE(c && y && lvec && rvec && out, "NULL argument (only x may be NULL)");
  REQUIRE(W > 0 && D1 > 0 && D2 > 0, "dimensions must be positive");
  REQUIRE(W <= 65535, "at most 65535 slabs");
  HIPCHK(hipSetDevice(c->device));
  const bool cplx = c->dtype == MPSK_C128;
  auto al16 = [](const void* p) { return (uintptr_t)p % 16 == 0; };     // the complex kernels move (re, im) pairs
  REQUIRE(!cplx || (al16(y) && al16(lvec) && al16(rvec) && al16(out) && al16(x)), "complex operands must be 16-byte aligned");
  if (int rc = ensure_ws(c, sizeof(double) * regularize_workspace_doubles(W, D1, D2) * (cplx ? 2 : 1))) return rc;
  HIPCHK(regularize_axpby(cplx, W, D1, D2, (const double*)y, (const double*)lvec, (const double*)rvec, a1, (const double*)x,
                          a0, (double*)out, c->ws.d(), c->stream));
  return MPSK_OK;
}
}  // extern "C"

// --------------------------------------------------------------------------------------------
// bond expansion of a uniform state (changebonds/optimalexpand.jl:16-67, changebonds.jl:13-38)
// --------------------------------------------------------------------------------------------
// mpsk_dAC2_product: H_AC2 applied to the PRODUCT AC[a,s1,m] AR[m,s2,b].  The two-site tensor is never formed: the
// contraction factorises through the middle bond m and the middle MPO leg u,
//   Lh[(a,t1), (u,m)] = sum GL[w][a,a'] AC[a',s1,m] O1[w,t1,s1,u]        (stages 1 + 2 of the one-site matvec)
//   Rh[(u,m), (b,t2)] = sum O2[u,t2,s2,v] AR[m,s2,b'] GR[v][b',b]        (the same from the right, left MPO leg open)
//   Y [(a,t1), (b,t2)] = sum_(u,m) Lh Rh                                   (ONE launch, K = Wm Dm as Wm K-segments,
//                                                                          batched over (t1,t2) with offset tables)
// Each half keeps the layout its slice kind produces (slab mix: [a,t1,m] slabs per u / [m,t2,b] slabs per u; dense GEMM
// route: [(a,m), (t1,u)] / [(m,b), (t2,u)]); the product only needs the (t, u) strides and the leading dimension of each.
// Intermediates: Wl d1 Dl Dm, Wm d1 Dl Dm, Wr d2 Dm Dr, Wm d2 Dm Dr doubles.
struct HalfView { const double* p; int64_t st, su, ld; };    // operand of (t, u) at p + t st + u su, leading dimension ld

static int product_tab(mpsk_ctx* c, int d1, int d2, int64_t sa, int64_t sb, int64_t sc1, int64_t sc2, const int64_t** out,
                       bool* even) {
  *even = sa % 2 == 0 && sb % 2 == 0;
  const int nz = d1 * d2;
  return c->prod_tabs.get({d1, d2, sa, sb, sc1, sc2}, [&](std::vector<int64_t>& h) {
    h.resize((size_t)3 * nz);
    for (int z = 0; z < nz; ++z) {
      const int t1 = z % d1, t2 = z / d1;
      h[z] = t1 * sa; h[nz + z] = t2 * sb; h[2 * nz + z] = t1 * sc1 + t2 * sc2;
    }
  }, "product offset table", out);
}

// left half: T1 (scratch, Wl d Dlo Dm) and L2 (result, Wm d Dlo Dm).  GL: Wl slabs [Dlo, Dl] (Dlo = Dl: mpsk_dAC2_product;
// mpsk_dAC2_proj: the bond dimension of the state below)
static int half_left(mpsk_ctx* c, const mpsk_mposlice* H, int Dlo, int Dl, int Dm, const double* GL, const double* AC,
                     double* T1, double* L2, HalfView* v) {
  const int d = H->d;
  if (dense_route(H)) {
    const int64_t col = (int64_t)Dlo * Dm;
    if (int rc = dense_stage1(c, H, Dlo, Dl, Dm, GL, AC, T1)) return rc;         // T1[(a,m), (s,w)]
    if (int rc = dense_stage2(c, H, col, T1, L2)) return rc;                     // L2[(a,m), (t,u)]
    *v = HalfView{L2, col, col * d, Dlo};
    return MPSK_OK;
  }
  const int64_t slab = (int64_t)Dlo * d * Dm;
  HIPCHK(stage1(c, H->Wl, Dlo, Dl, d * Dm, GL, AC, T1, 1));                        // T1[w] = GL[w] AC
  HIPCHK(mix_levels(c, H->fwd, d, Dlo, Dm, T1, L2));                             // L2[u][a,t,m]
  *v = HalfView{L2, Dlo, slab, (int64_t)Dlo * d};
  return MPSK_OK;
}

// right half: T1 (scratch, Wr d Dm Dro) and R2 (result, Wm d Dm Dro).  GR: Wr slabs [Dr, Dro] (Dro = Dr: mpsk_dAC2_product)
// (AR2 [Dm, d, Dr2], GR2: Wr slabs [Dr2, Dro]): a second stage-1 product that accumulates into T1 (mpsk_transfer_right_pair)
static int half_right(mpsk_ctx* c, const mpsk_mposlice* H, int Dm, int Dr, int Dro, const double* AR, const double* GR,
                      double* T1, double* R2, HalfView* v, const double* AR2 = nullptr, const double* GR2 = nullptr, int Dr2 = 0) {
  const int d = H->d;
  if (dense_route(H)) {
    const int64_t col = (int64_t)Dm * Dro;
    const int64_t* tab = nullptr;
    if (int rc = dense_tab(H, true, Dm, (int64_t)Dr * Dro, &tab)) return rc;
    GemmArgs g1 = mk(AR, GR, T1, Dm, Dro, Dr, (int64_t)Dm * d, Dr, Dm);          // T1[(m,b), (s,v)] = AR[:,s,:] GR[v]
    g1.batch = H->Wr * d; g1.bsC = col;
    g1.tabA = tab; g1.tabB = tab + (size_t)H->Wr * d;
    g1.tabs_even = Dm % 2 == 0 && ((int64_t)Dr * Dro) % 2 == 0;
    g1.tag = 1;
    HIPCHK(gemm_f64(g1, c->stream));
    if (AR2) {
      if (int rc = dense_tab(H, true, Dm, (int64_t)Dr2 * Dro, &tab)) return rc;
      GemmArgs h1 = mk(AR2, GR2, T1, Dm, Dro, Dr2, (int64_t)Dm * d, Dr2, Dm);
      h1.batch = H->Wr * d; h1.bsC = col;
      h1.tabA = tab; h1.tabB = tab + (size_t)H->Wr * d;
      h1.tabs_even = Dm % 2 == 0 && ((int64_t)Dr2 * Dro) % 2 == 0;
      h1.tag = 1; h1.beta = 1.0;
      HIPCHK(gemm_f64(h1, c->stream));
    }
    GemmArgs g2 = mk(T1, H->d_OdR, R2, (int)col, d * H->Wl, d * H->Wr, col, (int64_t)d * H->Wr, col);   // R2[(m,b), (t,u)]
    g2.tag = 1;
    HIPCHK(gemm_f64(g2, c->stream));
    *v = HalfView{R2, col, col * d, Dm};
    return MPSK_OK;
  }
  const int64_t slab = (int64_t)Dm * d * Dro;
  GemmArgs g1 = mk(AR, GR, T1, Dm * d, Dro, Dr, (int64_t)Dm * d, Dr, (int64_t)Dm * d);  // T1[v][(m,s), b] = AR GR[v]
  g1.batch = H->Wr; g1.bsA = 0; g1.bsB = (int64_t)Dr * Dro; g1.bsC = slab;
  g1.tag = 1;
  HIPCHK(gemm_f64(g1, c->stream));
  if (AR2) {
    GemmArgs h1 = mk(AR2, GR2, T1, Dm * d, Dro, Dr2, (int64_t)Dm * d, Dr2, (int64_t)Dm * d);
    h1.batch = H->Wr; h1.bsA = 0; h1.bsB = (int64_t)Dr2 * Dro; h1.bsC = slab;
    h1.tag = 1; h1.beta = 1.0;
    HIPCHK(gemm_f64(h1, c->stream));
  }
  HIPCHK(mix_levels(c, H->rgt, d, Dm, Dro, T1, R2));                             // R2[u][m,t,b]
  *v = HalfView{R2, Dm, slab, (int64_t)Dm * d};
  return MPSK_OK;
}

// The factorised two-site contraction for GL slabs [Dlo, Dl] and GR slabs [Dr, Dro]: Y[Dlo, d1, Dro, d2].  mpsk_dAC2_product
// is the square case (Dlo = Dl, Dro = Dr), mpsk_dAC2_proj the projection on another state's tangent space.
static int dAC2_factorised(mpsk_ctx* c, const mpsk_mposlice* H1, const mpsk_mposlice* H2, int Dlo, int Dl, int Dm, int Dr,
                           int Dro, const void* GL, const void* GR, const void* AC, const void* AR, void* Y) {
  HIPCHK(hipSetDevice(c->device));
  const int d1 = H1->d, d2 = H2->d, Wl = H1->Wl, Wm = H1->Wr, Wr = H2->Wr;
  Ws ws;
  const size_t o_tl = ws.take((size_t)Wl * d1 * Dlo * Dm, 2), o_l2 = ws.take((size_t)Wm * d1 * Dlo * Dm, 2);
  const size_t o_tr = ws.take((size_t)Wr * d2 * Dm * Dro, 2), o_r2 = ws.take((size_t)Wm * d2 * Dm * Dro, 2);
  if (int rc = ws.ensure(c)) return rc;
  double *TL = Ws::at(c, o_tl), *L2 = Ws::at(c, o_l2), *TR = Ws::at(c, o_tr), *R2 = Ws::at(c, o_r2);
  HalfView hl, hr;
  if (int rc = half_left(c, H1, Dlo, Dl, Dm, (const double*)GL, (const double*)AC, TL, L2, &hl)) return rc;
  if (int rc = half_right(c, H2, Dm, Dr, Dro, (const double*)AR, (const double*)GR, TR, R2, &hr)) return rc;
  // Y[a,t1,b,t2] = sum_u sum_m Lh(t1,u)[a,m] Rh(t2,u)[m,b]
  const int64_t plane = (int64_t)Dlo * d1 * Dro;
  Segs sg;
  if (!level_segs(sg, Wm, hl.su, hr.su, &H1->col_used, 1, 0, &H2->row_used)) return zero_fill(c, Y, sizeof(double) * plane * d2);
  const int64_t* tab = nullptr;
  bool even = false;
  if (int rc = product_tab(c, d1, d2, hl.st, hr.st, Dlo, plane, &tab, &even)) return rc;
  GemmArgs g = mk(hl.p, hr.p, (double*)Y, Dlo, Dro, Dm, hl.ld, hr.ld, (int64_t)Dlo * d1);
  g.batch = d1 * d2;
  g.tabA = tab; g.tabB = tab + (size_t)d1 * d2; g.tabC = tab + (size_t)2 * d1 * d2;
  g.tabs_even = even ? 1 : 0;
  g.tag = 1;
  HIPCHK(gemm_segments(g, sg, c->stream));
  return MPSK_OK;
}

extern "C" {
int mpsk_dAC2_product(mpsk_ctx* c, const mpsk_mposlice* H1, const mpsk_mposlice* H2, int Dl, int Dm, int Dr, const void* GL,
                      const void* GR, const void* AC, const void* AR, void* Y) {
  REQUIRE(c && H1 && H2 && GL && GR && AC && AR && Y, "NULL argument");
  REQUIRE(H1->Wr == H2->Wl, "MPO bond dimensions of the two slices do not match");
  REQUIRE(Dl > 0 && Dm > 0 && Dr > 0, "dimensions must be positive");
  REQUIRE(H1->dtype == MPSK_F64 && H2->dtype == MPSK_F64, "MPSK_F64 slices only");
  return dAC2_factorised(c, H1, H2, Dl, Dl, Dm, Dr, Dr, GL, GR, AC, AR, Y);
}

}  // extern "C"

// ---- quasiparticle excitations of a transfer matrix (quasiparticleexcitation.jl:258-293, qpenv.jl:238-251) -----------------
// The three projections of one application share the slice: the (lB, AR) product joins stage 1 of the (GL, B) chain, the
// (GL, AL) chain does not depend on B and is kept by the caller as `half` (stages 1 and 2, half_left), and joins stage 3.
// The pair transfers add two stage-1 products and run stages 2 and 3 once; the right one contracts the ket first
// (half_right, the order of the two-site product), so that both terms meet in one intermediate [Dl, d, Drb].
static int qp_f64_only(const mpsk_ctx* c, const mpsk_mposlice* H, const char* who) {
  if (H->dtype != MPSK_F64 || c->dtype != MPSK_F64) return fail(MPSK_ERR_UNSUPPORTED, std::string(who) + " is implemented for MPSK_F64 only");
  return MPSK_OK;
}

extern "C" {
int mpsk_qp_half_size(const mpsk_mposlice* H, int Dlo, int Dr2, size_t* doubles) {
  REQUIRE(H && doubles, "NULL argument");
  REQUIRE(Dlo > 0 && Dr2 > 0, "dimensions must be positive");
  *doubles = (size_t)Dlo * H->d * Dr2 * H->Wr;
  return MPSK_OK;
}

int mpsk_qp_half(mpsk_ctx* c, const mpsk_mposlice* H, int Dlo, int Dl, int Dr2, const void* GL, const void* A, void* half) {
  REQUIRE(c && H && GL && A && half, "NULL argument");
  REQUIRE(Dlo > 0 && Dl > 0 && Dr2 > 0, "dimensions must be positive");
  if (int rc = qp_f64_only(c, H, "mpsk_qp_half")) return rc;
  HIPCHK(hipSetDevice(c->device));
  Ws ws;
  const size_t o_t1 = ws.take((size_t)Dlo * H->d * Dr2 * H->Wl);
  if (int rc = ws.ensure(c)) return rc;
  HalfView v;
  return half_left(c, H, Dlo, Dl, Dr2, (const double*)GL, (const double*)A, Ws::at(c, o_t1), (double*)half, &v);
}

int mpsk_qp_apply(mpsk_ctx* c, const mpsk_mposlice* H, int Dlo, int Dl, int Dl2, int Dr, int Dr2, int Dro, const void* GL,
                  const void* GR, const void* B, const void* lB, const void* AR, const void* half, const void* rB, void* y) {
  REQUIRE(c && H && GL && GR && B && y, "NULL argument");
  REQUIRE((lB == nullptr) == (AR == nullptr), "lB and AR are given together or not at all");
  REQUIRE((half == nullptr) == (rB == nullptr), "half and rB are given together or not at all");
  REQUIRE(Dlo > 0 && Dl > 0 && Dr > 0 && Dro > 0, "dimensions must be positive");
  REQUIRE((!lB || Dl2 > 0) && (!half || Dr2 > 0), "dimensions must be positive");
  if (int rc = qp_f64_only(c, H, "mpsk_qp_apply")) return rc;
  const QpExtra q{(const double*)lB, (const double*)AR, Dl2, (const double*)half, (const double*)rB, Dr2};
  const QpExtra* qp = (lB || half) ? &q : nullptr;
  if (dense_route(H))
    return dAC_dense(c, H, Dlo, Dl, Dr, Dro, (const double*)GL, (const double*)GR, (const double*)B, (double*)y, 1.0, 0.0, qp);
  return dAC_impl(c, H, Dlo, Dl, Dr, Dro, GL, GR, B, 1, y, 1.0, 0.0, qp);
}

// One site and one real part of the Hamiltonian quasiparticle operator in the left gauge: B = VL X into the workspace, the
// three terms through the stages of mpsk_qp_apply into the workspace, and the pull-back VL^T (.) - E X as one GEMM whose
// store path adds gamma Z (GemmArgs::Z), so that -E X costs neither a pass over the result nor a copy of X.
int mpsk_qp_heff_site(mpsk_ctx* c, const mpsk_mposlice* H, int Dl, int DrL, int Dr, int Dl2, int Dr2, const void* GL,
                      const void* GR, const void* VL, const void* X, double E, const void* lB, const void* AR, const void* half,
                      const void* rB, void* Xout) {
  REQUIRE(c && H && GL && GR && VL && X && Xout, "NULL argument");
  REQUIRE((lB == nullptr) == (AR == nullptr), "lB and AR are given together or not at all");
  REQUIRE((half == nullptr) == (rB == nullptr), "half and rB are given together or not at all");
  REQUIRE(Dl > 0 && Dr > 0 && DrL > 0, "dimensions must be positive");
  REQUIRE((!lB || Dl2 > 0) && (!half || Dr2 > 0), "dimensions must be positive");
  REQUIRE(X != Xout, "Xout must not alias X");
  if (int rc = qp_f64_only(c, H, "mpsk_qp_heff_site")) return rc;
  const int d = H->d;
  REQUIRE((int64_t)Dl * d >= DrL, "the complement of AL has Dl d - DrL columns: DrL must not exceed Dl d");
  const int64_t rows = (int64_t)Dl * d;
  const int n = (int)(rows - DrL);
  if (n == 0) return MPSK_OK;                       // empty complement: nothing to write
  HIPCHK(hipSetDevice(c->device));
  // workspace: B | Y | the intermediates of the three terms (what mpsk_qp_apply takes), reserved in one piece so that the
  // inner ensure() never moves B and Y
  const size_t site = (size_t)rows * Dr;
  Ws ws;
  const size_t o_b = ws.take(site, 2), o_y = ws.take(site, 2);
  const size_t base = ws.n;
  ws.take(site * (size_t)(H->Wl + H->Wr));
  if (int rc = ws.ensure(c)) return rc;
  double *B = Ws::at(c, o_b), *Y = Ws::at(c, o_y);
  GemmArgs gb = mk((const double*)VL, (const double*)X, B, (int)rows, Dr, n, rows, n, rows);          // B = VL X
  HIPCHK(gemm_f64(gb, c->stream));
  const QpExtra q{(const double*)lB, (const double*)AR, Dl2, (const double*)half, (const double*)rB, Dr2};
  const QpExtra* qp = (lB || half) ? &q : nullptr;
  if (int rc = dense_route(H) ? dAC_dense(c, H, Dl, Dl, Dr, Dr, (const double*)GL, (const double*)GR, B, Y, 1.0, 0.0, qp, base)
                              : dAC_impl(c, H, Dl, Dl, Dr, Dr, GL, GR, B, 1, Y, 1.0, 0.0, qp, base))
    return rc;
  GemmArgs gp = mk((const double*)VL, Y, (double*)Xout, n, Dr, (int)rows, rows, rows, n, 1, 0);       // Xout = VL^T Y - E X
  gp.Z = (const double*)X; gp.ldz = n; gp.gamma = -E;
  HIPCHK(gemm_f64(gp, c->stream));
  return MPSK_OK;
}

int mpsk_transfer_left_pair(mpsk_ctx* c, const mpsk_mposlice* H, int Dl1, int Dl2, int Dr, int Dlb, int Drb, const void* V1,
                            const void* A1, const void* V2, const void* A2, const void* Ab, void* out) {
  REQUIRE(c && H && V1 && A1 && V2 && A2 && Ab && out, "NULL argument");
  REQUIRE(Dl1 > 0 && Dl2 > 0 && Dr > 0 && Dlb > 0 && Drb > 0, "dimensions must be positive");
  if (int rc = qp_f64_only(c, H, "mpsk_transfer_left_pair")) return rc;
  HIPCHK(hipSetDevice(c->device));
  if (dense_route(H))
    return transfer_left_dense(c, H, Dl1, Dr, Dlb, Drb, (const double*)V1, (const double*)A1, (const double*)Ab, (double*)out,
                               (const double*)V2, (const double*)A2, Dl2);
  return transfer_left_f64(c, H, H->Wl, H->Wr, H->d, Dl1, Dr, Dlb, Drb, V1, A1, Ab, out, nullptr, nullptr, (const double*)V2,
                           (const double*)A2, Dl2);
}

int mpsk_transfer_right_pair(mpsk_ctx* c, const mpsk_mposlice* H, int Dl, int Dr1, int Dr2, int Dlb, int Drb, const void* A1,
                             const void* V1, const void* A2, const void* V2, const void* Ab, void* out) {
  REQUIRE(c && H && V1 && A1 && V2 && A2 && Ab && out, "NULL argument");
  REQUIRE(Dl > 0 && Dr1 > 0 && Dr2 > 0 && Dlb > 0 && Drb > 0, "dimensions must be positive");
  if (int rc = qp_f64_only(c, H, "mpsk_transfer_right_pair")) return rc;
  HIPCHK(hipSetDevice(c->device));
  const int d = H->d, Wl = H->Wl, Wr = H->Wr;
  const size_t slab = (size_t)Dl * d * Drb;
  Ws ws;
  const size_t o_t1 = ws.take(slab * Wr), o_t2 = ws.take(slab * Wl);
  if (int rc = ws.ensure(c)) return rc;
  HalfView v;
  if (int rc = half_right(c, H, Dl, Dr1, Drb, (const double*)A1, (const double*)V1, Ws::at(c, o_t1), Ws::at(c, o_t2), &v,
                          (const double*)A2, (const double*)V2, Dr2))
    return rc;
  const double* T2 = Ws::at(c, o_t2);
  if (dense_route(H)) {
    // out[w][a,p] = sum_t sum_q T2[(a,q), (t,w)] Ab[p,t,q]     (batch over w; K-segments over t)
    const int64_t col = (int64_t)Dl * Drb;
    Segs sg;
    phys_segs(sg, d, col, Dlb);
    GemmArgs g3 = mk(T2, (const double*)Ab, (double*)out, Dl, Dlb, Drb, Dl, (int64_t)Dlb * d, Dl, 0, 1);
    g3.batch = Wl; g3.bsA = col * d; g3.bsB = 0; g3.bsC = (int64_t)Dl * Dlb;
    HIPCHK(gemm_segments(g3, sg, c->stream));
    return MPSK_OK;
  }
  // out[w][a,p] = sum_{(t,q)} T2[w][a,(t,q)] Ab[p,(t,q)]
  GemmArgs g3 = mk(T2, (const double*)Ab, (double*)out, Dl, Dlb, d * Drb, Dl, Dlb, Dl, 0, 1);
  g3.batch = Wl; g3.bsA = (int64_t)slab; g3.bsB = 0; g3.bsC = (int64_t)Dl * Dlb;
  HIPCHK(gemm_f64(g3, c->stream));
  return MPSK_OK;
}

}  // extern "C"

extern "C" {
// ac2_proj (derivatives.jl:218-226).  MPSK_F64: the factorised contraction above, the two-site tensor of the state above
// is never formed.  MPSK_C128: theta = AC AR is built in a scratch buffer of its own (d2 complex GEMMs, one per physical
// index of the right site) and the rectangular form of the complex two-site matvec runs on it.
int mpsk_dAC2_proj(mpsk_ctx* c, const mpsk_mposlice* H1, const mpsk_mposlice* H2, int Dlo, int Dl, int Dm, int Dr, int Dro,
                   const void* GL, const void* GR, const void* AC, const void* AR, void* Y) {
  REQUIRE(c && H1 && H2 && GL && GR && AC && AR && Y, "NULL argument");
  REQUIRE(H1->Wr == H2->Wl, "MPO bond dimensions of the two slices do not match");
  REQUIRE(Dlo > 0 && Dl > 0 && Dm > 0 && Dr > 0 && Dro > 0, "dimensions must be positive");
  REQUIRE(H1->dtype == H2->dtype, "the two slices have different scalar types");
  if (H1->dtype == MPSK_F64) return dAC2_factorised(c, H1, H2, Dlo, Dl, Dm, Dr, Dro, GL, GR, AC, AR, Y);
  HIPCHK(hipSetDevice(c->device));
  const int d1 = H1->d, d2 = H2->d;
  const size_t plane = (size_t)2 * Dl * d1 * Dr;                 // doubles of one s2-plane of theta[Dl, d1, Dr, d2]
  double* theta = nullptr;
  if (int rc = ex_scratch(c, sizeof(double) * plane * d2, &theta)) return rc;
  for (int s2 = 0; s2 < d2; ++s2)                                // theta[:, :, :, s2] = AC . AR[:, s2, :]
    if (int rc = gemm_c128(c, 0, 0, Dl * d1, Dr, Dm, 1.0, AC, (int64_t)Dl * d1, (const double*)AR + (size_t)2 * s2 * Dm,
                           (int64_t)Dm * d2, 0.0, theta + plane * s2, (int64_t)Dl * d1))
      return rc;
  return dAC2_c128(c, H1, H2, Dlo, Dl, Dr, Dro, (const double*)GL, (const double*)GR, theta, (double*)Y);
}
}  // extern "C"
