// api_pagoda.hip -- the host side of wpca.hip, pagoda.hip, rnorm.hip, sigma1.hip, aspects.hip,
// varnorm.hip and top_aspects.hip: weighted PCA, the PAGODA helpers, the random rounds of
// pagoda.gene.clusters, the aspect redundancy reduction, pagoda.varnorm, pagoda.subtract.aspect
// and the matrix step of pagoda.top.aspects.  (engine.hip is the
// pipeline; a feature's host code lives in the api_ file named after its kernel files.)
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#include "engine_internal.h"
#include "kernels.h"

using namespace scde;
using namespace scde::host;

// ------------------------------------------------------------------ weighted PCA
namespace {
// smoothing coefficients (src/bwpca.cpp:86-100): A (2np+1) x 4, A[:, j] = x^j,
// smoothc = A solve(A^T A, e_0); solved by partial-pivot LU like the K x K systems.
std::vector<double> wpca_smooth_coef(int smooth) {
  const int np = smooth / 2, L = 2 * np + 1;
  std::vector<double> X((size_t)L * 4), sc(L);
  for (int j = 0; j < 4; ++j)
    for (int i = 0; i < L; ++i) X[i + j * L] = std::pow((double)(i - np), (double)j);
  double A[16], b[4] = {1, 0, 0, 0};
  for (int j = 0; j < 4; ++j)
    for (int k = 0; k < 4; ++k) {
      double s = 0;
      for (int i = 0; i < L; ++i) s += X[i + k * L] * X[i + j * L];
      A[k + j * 4] = s;
    }
  int piv[4];
  for (int j = 0; j < 4; ++j) {
    int p = j;
    for (int i = j + 1; i < 4; ++i)
      if (std::fabs(A[i + j * 4]) > std::fabs(A[p + j * 4])) p = i;
    piv[j] = p;
    if (p != j)
      for (int l = 0; l < 4; ++l) std::swap(A[j + l * 4], A[p + l * 4]);
    const double r = 1.0 / A[j + j * 4];
    for (int i = j + 1; i < 4; ++i) A[i + j * 4] *= r;
    for (int l = j + 1; l < 4; ++l)
      for (int i = j + 1; i < 4; ++i) A[i + l * 4] -= A[i + j * 4] * A[j + l * 4];
  }
  for (int j = 0; j < 4; ++j)
    if (piv[j] != j) std::swap(b[j], b[piv[j]]);
  for (int l = 0; l < 4; ++l)
    for (int i = l + 1; i < 4; ++i) b[i] -= b[l] * A[i + l * 4];
  for (int l = 3; l >= 0; --l) {
    b[l] /= A[l + l * 4];
    for (int i = 0; i < l; ++i) b[i] -= b[l] * A[i + l * 4];
  }
  for (int i = 0; i < L; ++i) {
    double s = 0;
    for (int j = 0; j < 4; ++j) s += X[i + j * L] * b[j];
    sc[i] = s;
  }
  return sc;
}

}  // namespace

extern "C" {

int scde_bwpca_batch_dev(scde_ctx* ctx, const double* M_dev, const double* W_dev, int64_t ld, int ncells,
                         int64_t mcols, int nprob, const int* d, const int* npcs, const int* nstarts,
                         const int64_t* col_off, const int* cols, int64_t ncols, const int64_t* perm_off,
                         const int* perms, int64_t nperms, const int64_t* start_off, const double* starts,
                         int64_t nstart_vals, int smooth, double em_tol, int em_maxiter, double* rotation,
                         double* scores, double* scoreweights, double* colmeans, double* stats, int* iterations) {
  FORK_GUARD();
  if (!ctx || !M_dev || !W_dev) return fail(SCDE_EARG, "null argument");
  if (nprob < 0 || ncells <= 0 || ld < ncells || mcols <= 0) return fail(SCDE_EARG, "bad dimensions");
  if (nprob == 0) return SCDE_OK;
  if (!d || !npcs || !nstarts || !col_off || !cols || !start_off || !starts || !rotation || !scores || !stats)
    return fail(SCDE_EARG, "null problem array");
  const int n = ncells;
  for (int64_t i = 0; i < ncols; ++i)
    if (cols[i] < 0 || cols[i] >= mcols) return fail(SCDE_EARG, "column index %d out of range", cols[i]);
  for (int64_t i = 0; i < nperms; ++i)
    if (perms[i] < 0 || perms[i] >= n) return fail(SCDE_EARG, "permutation index out of range");
  std::vector<WpcaProb> P(nprob);
  int64_t o_rot = 0, o_sc = 0, o_var = 0;
  for (int p = 0; p < nprob; ++p) {
    if (d[p] <= 0) return fail(SCDE_EARG, "problem %d: no columns", p);
    if (nstarts[p] <= 0) return fail(SCDE_EARG, "problem %d: nstarts must be positive", p);
    const int K = std::min(npcs[p], d[p]);
    if (K < 1 || K > wpca_max_k()) return fail(SCDE_EARG, "problem %d: npcs must be in [1, %d]", p, wpca_max_k());
    if (col_off[p] < 0 || col_off[p] + d[p] > ncols) return fail(SCDE_EARG, "problem %d: cols out of range", p);
    if (perm_off && perm_off[p] >= 0 && perm_off[p] + (int64_t)d[p] * n > nperms)
      return fail(SCDE_EARG, "problem %d: perms out of range", p);
    if (start_off[p] < 0 || start_off[p] + (int64_t)nstarts[p] * d[p] * K > nstart_vals)
      return fail(SCDE_EARG, "problem %d: starts out of range", p);
    WpcaProb& q = P[p];
    q.d = d[p];
    q.K = K;
    q.nstarts = nstarts[p];
    q.pad = 0;
    q.col_off = col_off[p];
    q.perm_off = perm_off ? perm_off[p] : -1;
    q.start_off = start_off[p];
    q.out_rot = o_rot;
    q.out_sc = o_sc;
    q.out_var = o_var;
    o_rot += (int64_t)d[p] * K;
    o_sc += (int64_t)n * K;
    o_var += K + 2;
  }
  const int64_t tot_sc = o_sc;
  for (auto& q : P) {  // output layout: [rot | scores | scoreweights | colmeans | stats]
    q.out_sc += o_rot;
    q.out_pcw = q.out_sc + tot_sc;
    q.out_cm = q.out_sc + 2 * tot_sc;
    q.out_var += o_rot + 3 * tot_sc;
  }
  const int64_t out_total = o_rot + 3 * tot_sc + o_var;
  const int L = smooth > 0 ? 2 * (smooth / 2) + 1 : 0;
  std::vector<double> sc = L > 0 ? wpca_smooth_coef(smooth) : std::vector<double>(1, 0.0);
  constexpr int kLdsCap = 160 * 1024 - 2048;
  HCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  RCHK(upload(ctx, ctx->wp_cols, cols, sizeof(int) * (size_t)ncols));
  RCHK(upload(ctx, ctx->wp_perms, perms, sizeof(int) * (size_t)(perms ? nperms : 0)));
  RCHK(upload(ctx, ctx->wp_starts, starts, sizeof(double) * (size_t)nstart_vals));
  RCHK(upload(ctx, ctx->wp_smooth, sc.data(), sizeof(double) * sc.size()));
  HCHK(ctx->wp_out.ensure(sizeof(double) * out_total));
  // problems grouped by K; within a group by work (d x nstarts) descending, in chunks
  // whose scratch stays under a budget
  std::vector<int> order(nprob);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
    if (P[a].K != P[b].K) return P[a].K < P[b].K;
    return (int64_t)P[a].d * P[a].nstarts > (int64_t)P[b].d * P[b].nstarts;
  });
  const int64_t kScratchBudget = (int64_t)1 << 28;  // doubles (2 GiB)
  std::vector<int64_t> iters_all;
  std::vector<double> stat_h;
  if (iterations) {
    int64_t tot = 0;
    for (auto& q : P) tot += q.nstarts;
    iters_all.assign(tot, 0);
  }
  std::vector<int64_t> it_base(nprob, 0);
  {
    int64_t b = 0;
    for (int p = 0; p < nprob; ++p) {
      it_base[p] = b;
      b += P[p].nstarts;
    }
  }
  size_t pos = 0;
  while (pos < order.size()) {
    const int K = P[order[pos]].K;
    const int NM = K + K * (K + 1) / 2;
    // chunk: same K, scratch within budget
    size_t end = pos;
    int dmax = 0;
    int64_t need = 0;
    while (end < order.size() && P[order[end]].K == K) {
      const WpcaProb& q = P[order[end]];
      const int dm = std::max(dmax, q.d);
      const bool cl = (size_t)(dm + n) * K * sizeof(double) <= (size_t)kLdsCap;
      const int64_t per = (int64_t)q.nstarts * ((int64_t)q.d * K + 2LL * n * K + (cl ? 0 : (int64_t)n * K) +
                                                (int64_t)q.d * (NM + 1));
      if (end > pos && need + per > kScratchBudget) break;
      need += per;
      dmax = dm;
      ++end;
    }
    const bool cl = (size_t)(dmax + n) * K * sizeof(double) <= (size_t)kLdsCap;
    int64_t so = 0, stt = 0;
    for (size_t i = pos; i < end; ++i) {
      WpcaProb& q = P[order[i]];
      q.sE_off = so;
      so += (int64_t)q.nstarts * q.d * K;
      q.sC_off = so;
      so += (int64_t)q.nstarts * 2 * n * K;
      q.sW_off = so;
      if (!cl) so += (int64_t)q.nstarts * n * K;
      q.mom_off = so;
      so += (int64_t)q.nstarts * q.d * (NM + 1);
      q.stat_off = stt;
      stt += q.nstarts;
    }
    HCHK(ctx->wp_scratch.ensure(sizeof(double) * std::max<int64_t>(so, 1)));
    HCHK(ctx->wp_stat.ensure(sizeof(double) * 4 * std::max<int64_t>(stt, 1)));
    // block list: problems in groups of 8 (one per XCD under round-robin dispatch);
    // the starts of a problem sit 8 blocks apart, on the same XCD, sharing its columns in L2
    std::vector<int2> blocks;
    std::vector<WpcaProb> chunk;
    std::vector<int> kidx;
    for (size_t i = pos; i < end; ++i) {
      chunk.push_back(P[order[i]]);
      kidx.push_back((int)(i - pos));
    }
    // npcs = 1 without smoothing: one workgroup per group of wpca_ms_group() starts
    const bool ms = K == 1 && L == 0 && wpca_ms_ok(n, dmax) && ctx->opt_wpca_ms;
    const int sstep = ms ? wpca_ms_group() : 1;
    for (size_t g0 = 0; g0 < chunk.size(); g0 += 8) {
      const size_t g1 = std::min(chunk.size(), g0 + 8);
      int smax = 0;
      for (size_t i = g0; i < g1; ++i) smax = std::max(smax, chunk[i].nstarts);
      for (int s = 0; s < smax; s += sstep)
        for (size_t x = 0; x < 8; ++x) {
          const size_t i = g0 + x;
          if (i < g1 && s < chunk[i].nstarts) blocks.push_back(make_int2((int)i, s));
          else blocks.push_back(make_int2(-1, 0));  // keeps the 8-block stride
        }
    }
    // drop trailing padding
    while (!blocks.empty() && blocks.back().x < 0) blocks.pop_back();
    RCHK(upload(ctx, ctx->wp_probs, chunk.data(), sizeof(WpcaProb) * chunk.size()));
    RCHK(upload(ctx, ctx->wp_blocks, blocks.data(), sizeof(int2) * blocks.size()));
    RCHK(upload(ctx, ctx->wp_kidx, kidx.data(), sizeof(int) * kidx.size()));
    WpcaLaunch a;
    a.M = M_dev;
    a.W = W_dev;
    a.ld = ld;
    a.n = n;
    a.dmax = dmax;
    a.probs = ctx->wp_probs.as<WpcaProb>();
    a.blocks = ctx->wp_blocks.as<int2>();
    a.cols = ctx->wp_cols.as<int>();
    a.perms = ctx->wp_perms.as<int>();
    a.starts = ctx->wp_starts.as<double>();
    a.maxiter = em_maxiter;
    a.tol = em_tol;
    a.smoothc = ctx->wp_smooth.as<double>();
    a.L = L;
    a.scratch = ctx->wp_scratch.as<double>();
    a.stat = ctx->wp_stat.as<double>();
    a.out = ctx->wp_out.as<double>();
    a.lds_cap = kLdsCap;
    hipEvent_t ev = ctx->mark_begin(SLOT_WPCA_EM);
    if (!blocks.empty()) {
      if (ms) HCHK(launch_wpca_ms(a, (int)blocks.size(), st));
      else HCHK(launch_wpca_em(K, a, (int)blocks.size(), st));
    }
    ctx->mark_end(SLOT_WPCA_EM, ev);
    ev = ctx->mark_begin(SLOT_WPCA_FINAL);
    HCHK(launch_wpca_final(K, a, ctx->wp_kidx.as<int>(), (int)chunk.size(), st));
    ctx->mark_end(SLOT_WPCA_FINAL, ev);
    if (iterations) {
      stat_h.resize((size_t)4 * stt);
      HCHK(hipMemcpyAsync(stat_h.data(), a.stat, sizeof(double) * 4 * stt, hipMemcpyDeviceToHost, st));
      RCHK(ctx->sync());
      for (size_t i = 0; i < chunk.size(); ++i)
        for (int s = 0; s < chunk[i].nstarts; ++s)
          iters_all[it_base[order[pos + i]] + s] = (int64_t)stat_h[(size_t)4 * (chunk[i].stat_off + s) + 2];
    }
    pos = end;
  }
  std::vector<double> out_h(out_total);
  HCHK(hipMemcpyAsync(out_h.data(), ctx->wp_out.p, sizeof(double) * out_total, hipMemcpyDeviceToHost, st));
  RCHK(ctx->sync());
  std::memcpy(rotation, out_h.data(), sizeof(double) * o_rot);
  std::memcpy(scores, out_h.data() + o_rot, sizeof(double) * tot_sc);
  if (scoreweights) std::memcpy(scoreweights, out_h.data() + o_rot + tot_sc, sizeof(double) * tot_sc);
  if (colmeans) std::memcpy(colmeans, out_h.data() + o_rot + 2 * tot_sc, sizeof(double) * tot_sc);
  std::memcpy(stats, out_h.data() + o_rot + 3 * tot_sc, sizeof(double) * o_var);
  if (iterations)
    for (size_t i = 0; i < iters_all.size(); ++i) iterations[i] = (int)iters_all[i];
  return SCDE_OK;
}

// .Call("baileyWPCA", ...) (src/bwpca.cpp:59; bwpca.h:8) on host buffers.
int scde_baileyWPCA(const double* mat, const double* matw, int n, int d, int npcs, int nstarts, int smooth,
                    double em_tol, int em_maxiter, const double* starts, int nshuffles, const int* perms,
                    double* rotation, double* scores, double* scoreweights, double* var, double* totvar,
                    double* randvar) {
  FORK_GUARD();
  if (!mat || !matw || !starts || !rotation || !scores || !var || !totvar) return fail(SCDE_EARG, "null argument");
  if (n <= 0 || d <= 0) return fail(SCDE_EARG, "bad dimensions");
  if (nshuffles < 0 || (nshuffles > 0 && (!perms || !randvar))) return fail(SCDE_EARG, "bad shuffles");
  if (nstarts <= 0) return fail(SCDE_EARG, "nstarts must be positive");
  const int K = std::min(npcs, d);
  if (K < 1) return fail(SCDE_EARG, "npcs must be positive");
  if (K > wpca_max_k()) return fail(SCDE_EARG, "npcs must be in [1, %d]", wpca_max_k());  // before any device work
  scde_ctx* cx = nullptr;
  RCHK(use_ctx(cx));
  const size_t nd = (size_t)n * d;
  RCHK(upload(cx, cx->wp_M, mat, sizeof(double) * nd));
  RCHK(upload(cx, cx->wp_W, matw, sizeof(double) * nd));
  const int np = 1 + nshuffles;
  std::vector<int> dv(np, d), kv(np, npcs), sv(np, nstarts), cols(d);
  std::vector<int64_t> co(np, 0), po(np, -1), so(np);
  std::iota(cols.begin(), cols.end(), 0);
  for (int q = 0; q < np; ++q) {
    so[q] = (int64_t)q * nstarts * d * K;
    if (q > 0) po[q] = (int64_t)(q - 1) * d * n;
  }
  std::vector<double> rot((size_t)np * d * K), sco((size_t)np * n * K), pcw((size_t)np * n * K),
      stats((size_t)np * (K + 2));
  RCHK(scde_bwpca_batch_dev(cx, cx->wp_M.as<double>(), cx->wp_W.as<double>(), n, n, d, np, dv.data(), kv.data(),
                            sv.data(), co.data(), cols.data(), d, po.data(), perms,
                            nshuffles > 0 ? (int64_t)nshuffles * d * n : 0, so.data(), starts,
                            (int64_t)np * nstarts * d * K, smooth, em_tol, em_maxiter, rot.data(), sco.data(),
                            pcw.data(), nullptr, stats.data(), nullptr));
  std::memcpy(rotation, rot.data(), sizeof(double) * d * K);
  std::memcpy(scores, sco.data(), sizeof(double) * n * K);
  if (scoreweights) std::memcpy(scoreweights, pcw.data(), sizeof(double) * n * K);
  std::memcpy(var, stats.data(), sizeof(double) * K);
  *totvar = stats[K];
  for (int s = 0; s < nshuffles; ++s) randvar[s] = *totvar - stats[(size_t)(1 + s) * (K + 2) + K + 1];
  return SCDE_OK;
}

// ------------------------------------------------------------------ PAGODA helpers
// .Call("winsorizeMatrix", Mat, Trim) (src/pagoda.cpp:6-31; pagoda.h:5).  mat: nrow x ncol.
int scde_winsorizeMatrix(const double* mat, int nrow, int ncol, double trim, double* out) {
  FORK_GUARD();
  if (!mat || !out) return fail(SCDE_EARG, "null argument");
  if (nrow < 0 || ncol < 0) return fail(SCDE_EARG, "bad dimensions");
  const size_t nel = (size_t)nrow * ncol;
  const int ntr = (int)std::round(ncol * trim);
  if (nel == 0 || ntr == 0) {
    if (nel) std::memcpy(out, mat, sizeof(double) * nel);
    return SCDE_OK;
  }
  if (ntr < 0 || ntr > ncol - 1)  // the reference indexes sorted[ntr] and sorted[ncol - ntr - 1]
    return fail(SCDE_EARG, "winsorizeMatrix: trim %g out of range for %d columns", trim, ncol);
  int NP = 1;
  while (NP < ncol) NP <<= 1;
  if (NP > 8192 && ntr > 32) return fail(SCDE_EARG, "winsorizeMatrix: ncol > 8192 needs round(ncol * trim) <= 32");
  scde_ctx* cx = nullptr;
  RCHK(use_ctx(cx));
  RCHK(upload(cx, cx->pg_a, mat, sizeof(double) * nel));
  HCHK(cx->pg_b.ensure(sizeof(double) * nel));
  HCHK(launch_winsorize(cx->pg_a.as<double>(), nrow, ncol, ntr, cx->pg_b.as<double>(), cx->stream));
  HCHK(hipMemcpyAsync(out, cx->pg_b.p, sizeof(double) * nel, hipMemcpyDeviceToHost, cx->stream));
  return cx->sync();
}

// .Call("matWCorr", Mat, Matw) (src/pagoda.cpp:41-65; pagoda.h:6).  mat, matw: nrow x ncol;
// out: ncol x ncol (identity diagonal, c(j, i) for j > i, upper triangle 0).
int scde_matWCorr(const double* mat, const double* matw, int nrow, int ncol, double* out) {
  FORK_GUARD();
  if (!mat || !matw || !out) return fail(SCDE_EARG, "null argument");
  if (nrow < 0 || ncol < 0) return fail(SCDE_EARG, "bad dimensions");
  if (ncol == 0) return SCDE_OK;
  scde_ctx* cx = nullptr;
  RCHK(use_ctx(cx));
  const size_t nel = (size_t)nrow * ncol, nout = (size_t)ncol * ncol;
  RCHK(upload(cx, cx->pg_a, mat, sizeof(double) * nel));
  RCHK(upload(cx, cx->pg_b, matw, sizeof(double) * nel));
  HCHK(cx->pg_c.ensure(sizeof(double) * nout));
  HCHK(launch_matwcorr(cx->pg_a.as<double>(), cx->pg_b.as<double>(), nrow, ncol, cx->pg_c.as<double>(),
                       cx->stream));
  HCHK(hipMemcpyAsync(out, cx->pg_c.p, sizeof(double) * nout, hipMemcpyDeviceToHost, cx->stream));
  return cx->sync();
}

// .Call("matCorr", X, Y) = arma::cor(x, y) (src/pagoda.cpp:33-38; pagoda.h:8).  x: nrow x nx,
// y: nrow x ny; out: nx x ny.
int scde_matCorr(const double* x, int nrow, int nx, const double* y, int ny, double* out) {
  FORK_GUARD();
  if (!x || !y || !out) return fail(SCDE_EARG, "null argument");
  if (nrow < 0 || nx < 0 || ny < 0) return fail(SCDE_EARG, "bad dimensions");
  if ((size_t)nx * ny == 0) return SCDE_OK;
  scde_ctx* cx = nullptr;
  RCHK(use_ctx(cx));
  RCHK(upload(cx, cx->pg_a, x, sizeof(double) * (size_t)nrow * nx));
  RCHK(upload(cx, cx->pg_b, y, sizeof(double) * (size_t)nrow * ny));
  HCHK(cx->pg_c.ensure(sizeof(double) * (size_t)nx * ny));
  HCHK(cx->pg_d.ensure(sizeof(double) * 2 * ((size_t)nx + ny)));
  HCHK(launch_matcorr(cx->pg_a.as<double>(), nrow, nx, cx->pg_b.as<double>(), ny, cx->pg_d.as<double>(),
                      cx->pg_c.as<double>(), cx->stream));
  HCHK(hipMemcpyAsync(out, cx->pg_c.p, sizeof(double) * (size_t)nx * ny, hipMemcpyDeviceToHost, cx->stream));
  return cx->sync();
}

// .Call("plSemicompleteCor2", Pl) (src/pagoda.cpp:67-117; pagoda.h:7).  List element p:
// gene indices idx[off[p] .. off[p+1]) (increasing), values val[...].  r: np x np
// correlations over the shared genes (1 on the diagonal); n: np x np union sizes (0 on it).
int scde_plSemicompleteCor2(int np, const int64_t* off, const int* idx, const double* val, double* r, int* n) {
  FORK_GUARD();
  if (np < 0 || (np > 0 && (!off || !r || !n))) return fail(SCDE_EARG, "null argument");
  if (np == 0) return SCDE_OK;
  const int64_t tot = off[np];
  if (off[0] != 0 || tot < 0) return fail(SCDE_EARG, "bad offsets");
  for (int p = 0; p < np; ++p) {
    if (off[p + 1] < off[p]) return fail(SCDE_EARG, "bad offsets");
    for (int64_t e = off[p] + 1; e < off[p + 1]; ++e)
      if (idx[e] <= idx[e - 1]) return fail(SCDE_EARG, "list %d: gene indices must increase", p);
  }
  scde_ctx* cx = nullptr;
  RCHK(use_ctx(cx));
  std::vector<long long> offl(off, off + np + 1);
  RCHK(upload(cx, cx->pg_a, offl.data(), sizeof(long long) * offl.size()));
  RCHK(upload(cx, cx->pg_b, idx, sizeof(int) * (size_t)tot));
  RCHK(upload(cx, cx->pg_c, val, sizeof(double) * (size_t)tot));
  const size_t nn = (size_t)np * np;
  HCHK(cx->pg_d.ensure(sizeof(double) * nn));
  HCHK(cx->pg_e.ensure(sizeof(int) * nn));
  HCHK(launch_plcor(np, cx->pg_a.as<long long>(), cx->pg_b.as<int>(), cx->pg_c.as<double>(), cx->pg_d.as<double>(),
                    cx->pg_e.as<int>(), cx->stream));
  HCHK(hipMemcpyAsync(r, cx->pg_d.p, sizeof(double) * nn, hipMemcpyDeviceToHost, cx->stream));
  HCHK(hipMemcpyAsync(n, cx->pg_e.p, sizeof(int) * nn, hipMemcpyDeviceToHost, cx->stream));
  return cx->sync();
}

// 1 - cor of the columns of a resident nrow x ncol matrix, into a resident ncol x ncol matrix
// (k_matcorr with itself, then 1 - x): pagoda.gene.clusters' distance without a host visit.
int scde_cor_distance_dev(scde_ctx* ctx, const double* x_dev, int nrow, int ncol, double* out_dev) {
  FORK_GUARD();
  if (!x_dev || !out_dev) return fail(SCDE_EARG, "null argument");
  if (nrow < 1 || ncol < 1) return fail(SCDE_EARG, "bad dimensions");
  RCHK(use_ctx(ctx));
  HCHK(ctx->pg_d.ensure(sizeof(double) * 4 * (size_t)ncol));
  HCHK(launch_matcorr(x_dev, nrow, ncol, x_dev, ncol, ctx->pg_d.as<double>(), out_dev, ctx->stream));
  HCHK(launch_one_minus(out_dev, ncol, ctx->stream));
  return ctx->sync();
}

// ------------------------------------------------------------------ pagoda.gene.clusters' random rounds
// (contract in scde_hip.h).  Arguments are checked before the GPU is touched.
int scde_dev_mem_info(scde_ctx* ctx, int64_t* free_bytes, int64_t* total_bytes) {
  FORK_GUARD();
  if (!free_bytes || !total_bytes) return fail(SCDE_EARG, "null argument");
  RCHK(use_ctx(ctx));
  size_t f = 0, t = 0;
  HCHK(hipMemGetInfo(&f, &t));
  *free_bytes = (int64_t)f;
  *total_bytes = (int64_t)t;
  return SCDE_OK;
}

int scde_rnorm_matrix_dev(scde_ctx* ctx, const uint32_t* words, int ngenes, int ncells, double* out_dev) {
  FORK_GUARD();
  if (!words || !out_dev) return fail(SCDE_EARG, "null argument");
  if (ngenes < 1 || ncells < 1) return fail(SCDE_EARG, "bad dimensions");
  RCHK(use_ctx(ctx));
  RCHK(upload(ctx, ctx->gr_raw, words, sizeof(uint32_t) * 2 * (size_t)ngenes * ncells));
  HCHK(launch_rnorm(ctx->gr_raw.as<uint32_t>(), ngenes, ncells, out_dev, ctx->stream));
  return ctx->sync();
}

int scde_winsorize_dev(scde_ctx* ctx, const double* x_dev, int ncells, int ngenes, double trim, double* out_dev) {
  FORK_GUARD();
  if (!x_dev || !out_dev) return fail(SCDE_EARG, "null argument");
  if (x_dev == out_dev) return fail(SCDE_EARG, "winsorize: in place is not supported");
  if (ngenes < 1 || ncells < 1) return fail(SCDE_EARG, "bad dimensions");
  const int ntr = (int)std::round(ncells * trim);
  if (ntr < 0 || ntr > ncells - 1)
    return fail(SCDE_EARG, "winsorize: trim %g out of range for %d cells", trim, ncells);
  int NP = 1;
  while (NP < ncells) NP <<= 1;
  if (NP > 8192 && ntr > 32) return fail(SCDE_EARG, "winsorize: more than 8192 cells need round(cells * trim) <= 32");
  RCHK(use_ctx(ctx));
  if (ntr == 0)
    HCHK(hipMemcpyAsync(out_dev, x_dev, sizeof(double) * (size_t)ncells * ngenes, hipMemcpyDeviceToDevice,
                        ctx->stream));
  else
    HCHK(launch_winsorize_gc(x_dev, ncells, ngenes, ntr, out_dev, ctx->stream));
  return ctx->sync();
}

int scde_keep_absdiff_dev(scde_ctx* ctx, const double* x_dev, int ncells, int ngenes, int* keep) {
  FORK_GUARD();
  if (!x_dev || !keep) return fail(SCDE_EARG, "null argument");
  if (ngenes < 1) return fail(SCDE_EARG, "bad dimensions");
  if (ncells < 2)  // diff() of one value is empty: every gene would be dropped
    return fail(SCDE_EARG, "keep rule: at least 2 cells are needed (ncells = %d)", ncells);
  RCHK(use_ctx(ctx));
  HCHK(ctx->gr_int.ensure(sizeof(int) * (size_t)ngenes));
  HCHK(launch_keep_absdiff(x_dev, ncells, ngenes, ctx->gr_int.as<int>(), ctx->stream));
  HCHK(hipMemcpyAsync(keep, ctx->gr_int.p, sizeof(int) * (size_t)ngenes, hipMemcpyDeviceToHost, ctx->stream));
  return ctx->sync();
}

int scde_gather_cols_dev(scde_ctx* ctx, const double* x_dev, int nrow, int64_t ncol, const int* cols, int nsel,
                         double* out_dev) {
  FORK_GUARD();
  if (!x_dev || !out_dev || (nsel > 0 && !cols)) return fail(SCDE_EARG, "null argument");
  if (nrow < 1 || ncol < 1 || nsel < 0) return fail(SCDE_EARG, "bad dimensions");
  for (int j = 0; j < nsel; ++j)
    if (cols[j] < 0 || cols[j] >= ncol) return fail(SCDE_EARG, "gather: column %d of the list is %d", j, cols[j]);
  if (nsel == 0) return SCDE_OK;
  RCHK(use_ctx(ctx));
  RCHK(upload(ctx, ctx->gr_int, cols, sizeof(int) * (size_t)nsel));
  HCHK(launch_gather_cols(x_dev, nrow, ctx->gr_int.as<int>(), nsel, out_dev, ctx->stream));
  return ctx->sync();
}

int scde_sigma1sq_batch_dev(scde_ctx* ctx, const double* x_dev, int ncells, int64_t ngenes, int nprob,
                            const int64_t* off, const int* idx, double* out) {
  FORK_GUARD();
  if (nprob < 0) return fail(SCDE_EARG, "sigma1sq: nprob must not be negative");
  if (nprob == 0) return SCDE_OK;
  if (!x_dev || !off || !idx || !out) return fail(SCDE_EARG, "null argument");
  if (ncells < 1 || ngenes < 1) return fail(SCDE_EARG, "bad dimensions");
  if (off[0] < 0) return fail(SCDE_EARG, "sigma1sq: negative offset");
  std::vector<long long> po(2 * (size_t)nprob + 1);  // off[nprob + 1], then ws_off[nprob]
  size_t wsd = 0;
  for (int p = 0; p < nprob; ++p) {
    const int64_t q = off[p + 1] - off[p];
    if (q < 1) return fail(SCDE_EARG, "sigma1sq: problem %d has no columns", p);
    for (int64_t t = off[p]; t < off[p + 1]; ++t)
      if (idx[t] < 0 || idx[t] >= ngenes)
        return fail(SCDE_EARG, "sigma1sq: problem %d: column index %d outside [0, %lld)", p, idx[t],
                    (long long)ngenes);
    po[p] = off[p];
    po[nprob + 1 + p] = (long long)wsd;
    wsd += sigma1_ws_doubles(q, ncells);
  }
  po[nprob] = off[nprob];
  RCHK(use_ctx(ctx));
  // the workspace comes first: a batch that does not fit fails here, before any launch
  if (ctx->gr_ws.ensure(sizeof(double) * wsd) != hipSuccess)
    return fail_oom("sigma1sq: out of memory: the workspace of %d problem(s) needs %zu bytes of device memory",
                    nprob, sizeof(double) * wsd);
  const size_t nidx = (size_t)(off[nprob] - off[0]);
  HCHK(ctx->gr_prob.ensure(sizeof(long long) * po.size() + sizeof(int) * nidx));
  long long* d_off = ctx->gr_prob.as<long long>();
  int* d_idx = reinterpret_cast<int*>(d_off + po.size());
  for (int p = 0; p <= nprob; ++p) po[p] -= off[0];
  HCHK(hipMemcpyAsync(d_off, po.data(), sizeof(long long) * po.size(), hipMemcpyHostToDevice, ctx->stream));
  HCHK(hipMemcpyAsync(d_idx, idx + off[0], sizeof(int) * nidx, hipMemcpyHostToDevice, ctx->stream));
  HCHK(ctx->gr_out.ensure((sizeof(double) + sizeof(int)) * (size_t)nprob));
  double* d_out = ctx->gr_out.as<double>();
  int* d_flag = reinterpret_cast<int*>(d_out + nprob);
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  HCHK(launch_sigma1sq(x_dev, ncells, ngenes, nprob, d_off, d_idx, d_off + nprob + 1, ctx->gr_ws.as<double>(), d_out,
                       d_flag, ctx->stream));
  ctx->mark_end(SLOT_OTHER, ev);
  std::vector<int> hf(nprob);
  HCHK(hipMemcpyAsync(out, d_out, sizeof(double) * (size_t)nprob, hipMemcpyDeviceToHost, ctx->stream));
  HCHK(hipMemcpyAsync(hf.data(), d_flag, sizeof(int) * (size_t)nprob, hipMemcpyDeviceToHost, ctx->stream));
  RCHK(ctx->sync());
  if (sizeof(double) * wsd > ((size_t)1 << 30)) ctx->gr_ws.release();
  for (int p = 0; p < nprob; ++p)
    if (hf[p] != 0) return fail(SCDE_EINTERNAL, "sigma1sq: problem %d: a column index failed the device check", p);
  return SCDE_OK;
}

// ------------------------------------------------------------------ aspect redundancy reduction
// pagoda.reduce.loading.redundancy / pagoda.reduce.redundancy and their helpers (aspects.hip;
// contract in scde_hip.h).  Arguments are checked before the GPU is touched.
static int plcor_lists_check(int np, const int64_t* off, const int* idx, const double* val) {
  if (np < 1 || !off || !idx || !val) return fail(SCDE_EARG, "plSemicompleteCor2: null argument or no lists");
  if (off[0] != 0) return fail(SCDE_EARG, "plSemicompleteCor2: off[0] must be 0");
  for (int p = 0; p < np; ++p) {
    if (off[p + 1] < off[p]) return fail(SCDE_EARG, "plSemicompleteCor2: list %d has a negative length", p);
    for (int64_t e = off[p] + 1; e < off[p + 1]; ++e)
      if (idx[e] <= idx[e - 1]) return fail(SCDE_EARG, "plSemicompleteCor2: list %d: gene indices must increase", p);
  }
  return SCDE_OK;
}

int scde_plSemicompleteCor2_dev(scde_ctx* ctx, int np, const int64_t* off, const int* idx, const double* val,
                                double* r_dev, int* n_dev) {
  FORK_GUARD();
  if (!r_dev || !n_dev) return fail(SCDE_EARG, "plSemicompleteCor2: null output");
  RCHK(plcor_lists_check(np, off, idx, val));
  RCHK(use_ctx(ctx));
  const size_t tot = (size_t)off[np];
  std::vector<long long> offl(off, off + np + 1);
  RCHK(upload(ctx, ctx->pg_a, offl.data(), sizeof(long long) * offl.size()));
  RCHK(upload(ctx, ctx->pg_b, idx, sizeof(int) * std::max<size_t>(tot, 1)));
  RCHK(upload(ctx, ctx->pg_c, val, sizeof(double) * std::max<size_t>(tot, 1)));
  HCHK(launch_plcor(np, ctx->pg_a.as<long long>(), ctx->pg_b.as<int>(), ctx->pg_c.as<double>(), r_dev, n_dev,
                    ctx->stream));
  return ctx->sync();  // (offl is read by the copy until here)
}

static int t_renorm_check(const void* r, const void* n, int m, double target_ndf, const void* cr) {
  if (!r || !n || !cr) return fail(SCDE_EARG, "t_renorm: null argument");
  if (m < 1) return fail(SCDE_EARG, "t_renorm: m must be at least 1 (m = %d)", m);
  if (!(target_ndf > 2.0) || !(target_ndf < 1e15))
    return fail(SCDE_EARG, "t_renorm: target_ndf must be above 2 and finite (target_ndf = %g)", target_ndf);
  return SCDE_OK;
}

int scde_t_renorm_dev(scde_ctx* ctx, const double* r_dev, const int* n_dev, int m, double target_ndf,
                      double* cr_dev) {
  FORK_GUARD();
  RCHK(t_renorm_check(r_dev, n_dev, m, target_ndf, cr_dev));
  RCHK(use_ctx(ctx));
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  HCHK(launch_t_renorm(r_dev, n_dev, m, target_ndf, cr_dev, ctx->stream));
  ctx->mark_end(SLOT_OTHER, ev);
  return ctx->sync();
}

int scde_t_renorm_host(scde_ctx* ctx, const double* r, const int* n, int m, double target_ndf, double* cr) {
  FORK_GUARD();
  RCHK(t_renorm_check(r, n, m, target_ndf, cr));
  RCHK(use_ctx(ctx));
  const size_t nn = (size_t)m * m;
  if (ctx->as_r.ensure(sizeof(double) * nn) != hipSuccess || ctx->as_cr.ensure(sizeof(double) * nn) != hipSuccess ||
      ctx->as_n.ensure(sizeof(int) * nn) != hipSuccess)
    return fail_oom("t_renorm: out of memory: three %d x %d matrices need %zu bytes of device memory", m, m,
                    (2 * sizeof(double) + sizeof(int)) * nn);
  HCHK(hipMemcpyAsync(ctx->as_r.p, r, sizeof(double) * nn, hipMemcpyHostToDevice, ctx->stream));
  HCHK(hipMemcpyAsync(ctx->as_n.p, n, sizeof(int) * nn, hipMemcpyHostToDevice, ctx->stream));
  HCHK(launch_t_renorm(ctx->as_r.as<double>(), ctx->as_n.as<int>(), m, target_ndf, ctx->as_cr.as<double>(),
                       ctx->stream));
  HCHK(hipMemcpyAsync(cr, ctx->as_cr.p, sizeof(double) * nn, hipMemcpyDeviceToHost, ctx->stream));
  return ctx->sync();
}

int scde_aspect_distance_dev(scde_ctx* ctx, const double* x_dev, int ncells, int m, const double* cr_dev, int abs,
                             double corr_power, double* out_dev) {
  FORK_GUARD();
  if (!x_dev || !out_dev) return fail(SCDE_EARG, "aspect_distance: null argument");
  if (ncells < 1 || m < 1) return fail(SCDE_EARG, "aspect_distance: bad dimensions (ncells = %d, m = %d)", ncells, m);
  if (cr_dev && !(corr_power == corr_power))
    return fail(SCDE_EARG, "aspect_distance: corr_power is NaN");
  RCHK(use_ctx(ctx));
  if (ctx->as_z.ensure(sizeof(double) * (size_t)ncells * m) != hipSuccess)
    return fail_oom("aspect_distance: out of memory: the scaled patterns need %zu bytes of device memory",
                    sizeof(double) * (size_t)ncells * m);
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  HCHK(launch_aspect_dist(x_dev, ncells, m, ctx->as_z.as<double>(), cr_dev, abs != 0, corr_power, out_dev,
                          ctx->stream));
  ctx->mark_end(SLOT_OTHER, ev);
  return ctx->sync();
}

int scde_matWCorr_distance_dev(scde_ctx* ctx, const double* x_dev, const double* w_dev, int ncells, int m, int abs,
                               double* out_dev) {
  FORK_GUARD();
  if (!x_dev || !w_dev || !out_dev) return fail(SCDE_EARG, "matWCorr_distance: null argument");
  if (ncells < 1 || m < 1)
    return fail(SCDE_EARG, "matWCorr_distance: bad dimensions (ncells = %d, m = %d)", ncells, m);
  RCHK(use_ctx(ctx));
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  HCHK(launch_matwcorr(x_dev, w_dev, ncells, m, out_dev, ctx->stream));
  HCHK(launch_wdist(out_dev, m, abs != 0, ctx->stream));
  ctx->mark_end(SLOT_OTHER, ev);
  return ctx->sync();
}

int scde_collapse_aspects_dev(scde_ctx* ctx, const double* x_dev, const double* w_dev, int ncells, int m, int nclust,
                              const int64_t* off, const int* idx, int scale, int pick_top, double* d_dev,
                              double* dw_dev, int* top, int* fallback, double* orientation) {
  FORK_GUARD();
  if (nclust < 0) return fail(SCDE_EARG, "collapse: nclust must not be negative");
  if (nclust == 0) return SCDE_OK;
  if (!x_dev || !w_dev || !off || !idx || !d_dev || !dw_dev || !top || !fallback || !orientation)
    return fail(SCDE_EARG, "collapse: null argument");
  if (ncells < 2) return fail(SCDE_EARG, "collapse: at least 2 cells are needed (ncells = %d)", ncells);
  if (m < 1) return fail(SCDE_EARG, "collapse: m must be at least 1 (m = %d)", m);
  if (off[0] < 0) return fail(SCDE_EARG, "collapse: negative offset");
  std::vector<long long> po(2 * (size_t)nclust + 1);  // off[nclust + 1], then ws_off[nclust]
  size_t wsd = 0;
  for (int p = 0; p < nclust; ++p) {
    const int64_t q = off[p + 1] - off[p];
    if (q < 1) return fail(SCDE_EARG, "collapse: cluster %d has no rows", p);
    if (q > m) return fail(SCDE_EARG, "collapse: cluster %d lists %lld rows of %d", p, (long long)q, m);
    for (int64_t t = off[p]; t < off[p + 1]; ++t)
      if (idx[t] < 0 || idx[t] >= m)
        return fail(SCDE_EARG, "collapse: cluster %d: row index %d outside [0, %d)", p, idx[t], m);
    po[p] = off[p] - off[0];
    po[nclust + 1 + p] = (long long)wsd;
    wsd += collapse_ws_doubles(q, ncells, pick_top);
  }
  po[nclust] = off[nclust] - off[0];
  RCHK(use_ctx(ctx));
  // the workspace comes first: a batch that does not fit fails here, before any launch
  if (ctx->as_ws.ensure(sizeof(double) * wsd) != hipSuccess)
    return fail_oom("collapse: out of memory: the workspace of %d cluster(s) needs %zu bytes of device memory",
                    nclust, sizeof(double) * wsd);
  const size_t nidx = (size_t)(off[nclust] - off[0]);
  HCHK(ctx->as_prob.ensure(sizeof(long long) * po.size() + sizeof(int) * nidx));
  long long* d_off = ctx->as_prob.as<long long>();
  int* d_idx = reinterpret_cast<int*>(d_off + po.size());
  HCHK(hipMemcpyAsync(d_off, po.data(), sizeof(long long) * po.size(), hipMemcpyHostToDevice, ctx->stream));
  HCHK(hipMemcpyAsync(d_idx, idx + off[0], sizeof(int) * nidx, hipMemcpyHostToDevice, ctx->stream));
  HCHK(ctx->as_out.ensure((sizeof(double) + 2 * sizeof(int)) * (size_t)nclust));
  double* d_cor = ctx->as_out.as<double>();
  int* d_top = reinterpret_cast<int*>(d_cor + nclust);
  int* d_st = d_top + nclust;
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  HCHK(launch_collapse(x_dev, w_dev, ncells, m, nclust, d_off, d_idx, d_off + nclust + 1, ctx->as_ws.as<double>(),
                       scale != 0, pick_top != 0, d_dev, dw_dev, d_top, d_st, d_cor, ctx->stream));
  ctx->mark_end(SLOT_OTHER, ev);
  HCHK(hipMemcpyAsync(orientation, d_cor, sizeof(double) * (size_t)nclust, hipMemcpyDeviceToHost, ctx->stream));
  HCHK(hipMemcpyAsync(top, d_top, sizeof(int) * (size_t)nclust, hipMemcpyDeviceToHost, ctx->stream));
  HCHK(hipMemcpyAsync(fallback, d_st, sizeof(int) * (size_t)nclust, hipMemcpyDeviceToHost, ctx->stream));
  RCHK(ctx->sync());
  if (sizeof(double) * wsd > ((size_t)1 << 30)) ctx->as_ws.release();
  for (int p = 0; p < nclust; ++p)
    if (fallback[p] < 0) return fail(SCDE_EINTERNAL, "collapse: cluster %d: a row index failed the device check", p);
  return SCDE_OK;
}

// ------------------------------------------------------------------ pagoda.varnorm
// pagoda.varnorm's posterior-mode consumer (R/functions.R:1414-1507): modes from
// scde.posteriors' joint posteriors -- dataset-wide and per batch level -- and the weight
// matrices 1 - mfp * sfp.  The magnitudes are as.numeric(colnames(jp)) = exp(marginals)
// through R's 15-significant-digit as.character (R/functions.R:640-643).
static int vn_posterior_jp(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, const int* cellidx, int C,
                           const double* models, int mld, int local_theta, int sq, const double* prior_x, int G,
                           int nboot, int n_cores, double* jp_dev) {
  std::vector<double> mm((size_t)C * 12);
  for (int j = 0; j < 12; ++j)
    for (int c = 0; c < C; ++c) mm[(size_t)c + (size_t)C * j] = models[(size_t)cellidx[c] + (size_t)mld * j];
  for (int c = 0; c < C; ++c) {
    double& ca = mm[(size_t)c + (size_t)C * 4];
    if (ca < 1e-10) ca = 1e-10;  // R/functions.R:579-583
  }
  const std::vector<double> mag = marginals(prior_x, G);
  PostSpec s;
  s.ncells = C;
  s.models = mm.data();
  s.localtheta = local_theta;
  s.squarelogit = sq;
  s.mag = mag.data();
  s.G = G;
  s.nboot = nboot;
  s.postflag = 0;
  s.counts_dev = counts_dev;
  s.ld = ld;
  s.cellidx_host = cellidx;
  s.ngenes = ngenes;
  seeding(n_cores, 0, ngenes, ngenes, s.seeds, s.wset);
  s.rand_kind = g_rand_kind;
  s.jp = jp_dev;
  s.jp_g = 1;
  s.jp_k = ngenes;
  ctx->us[0].ready = false;
  return run_posterior(ctx, s, ctx->us[0]);
}

int scde_pagoda_varnorm_weights_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells,
                                    const double* models, int local_theta, int square_logit_conc,
                                    const double* prior_x, int ngrid, int nboot, int n_cores, const int* batch_codes,
                                    int nbatch, int use_expected_value, double* modes, double* matw,
                                    double* bmatw) {
  FORK_GUARD();
  if (!ctx || !counts_dev || !models || !prior_x || !modes) return fail(SCDE_EARG, "null argument");
  if (ngenes < 0 || ncells <= 0 || ngrid <= 0 || ld < ngenes) return fail(SCDE_EARG, "bad dimensions");
  const bool batch = batch_codes && nbatch > 1;
  if (batch && matw && !bmatw) return fail(SCDE_EARG, "bmatw required with a batch");
  ctx->vn_n = -1;  // what the context keeps for the later stages is valid once this call has finished
  HCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int N = ngenes, C = ncells, G = ngrid;
  // as.numeric(colnames(jp)): exp(marginals) with 15 significant digits
  const std::vector<double> marg = marginals(prior_x, G);
  std::vector<double> mag(G);
  for (int k = 0; k < G; ++k) {
    char buf[64];
    snprintf(buf, sizeof(buf), "%.15g", std::exp(marg[k]));
    mag[k] = strtod(buf, nullptr);
  }
  RCHK(upload(ctx, ctx->diffv, mag.data(), sizeof(double) * G));
  const int nm = batch ? 1 + nbatch : 1;
  HCHK(ctx->vn_modes.ensure(sizeof(double) * std::max<size_t>(1, (size_t)N * nm)));
  HCHK(ctx->jpB.ensure(sizeof(double) * std::max<size_t>(1, (size_t)N * G)));
  double* dmodes = ctx->vn_modes.as<double>();
  std::vector<int> allc(C);
  for (int c = 0; c < C; ++c) allc[c] = c;
  // dataset-wide modes, then one set per batch level
  for (int m = 0; m < nm; ++m) {
    std::vector<int> cells;
    if (m == 0) {
      cells = allc;
    } else {
      for (int c = 0; c < C; ++c) {
        if (batch_codes[c] < 0 || batch_codes[c] >= nbatch) return fail(SCDE_EARG, "batch code out of range");
        if (batch_codes[c] == m - 1) cells.push_back(c);
      }
      if (cells.empty()) return fail(SCDE_EARG, "batch level %d has no cells", m - 1);
    }
    if (N > 0) {
      RCHK(vn_posterior_jp(ctx, counts_dev, ld, N, cells.data(), (int)cells.size(), models, C, local_theta,
                           square_logit_conc, prior_x, G, nboot, n_cores, ctx->jpB.as<double>()));
      HCHK(launch_vn_modes(ctx->jpB.as<double>(), 1, N, N, G, ctx->diffv.as<double>(), use_expected_value,
                           dmodes + (size_t)m * N, st));
    }
  }
  // weight matrices
  RCHK(upload(ctx, ctx->models, models, sizeof(double) * (size_t)C * 12));
  RCHK(upload(ctx, ctx->in1, allc.data(), sizeof(int) * C));
  // (the matrices stay in the context for scde_pagoda_varnorm_moments_dev / _matrix_dev)
  std::vector<long long> off(C, 0);
  for (int pass = 0; pass < (batch ? 2 : 1); ++pass) {
    Buf& keep = pass == 0 ? ctx->vn_matw : ctx->vn_bmatw;
    HCHK(keep.ensure(sizeof(double) * std::max<size_t>(1, (size_t)N * C)));
    if (pass == 1)
      for (int c = 0; c < C; ++c) off[c] = (long long)(1 + batch_codes[c]) * N;
    RCHK(upload(ctx, ctx->in2, off.data(), sizeof(long long) * C));
    HCHK(launch_vn_matw(counts_dev, ld, N, ctx->in1.as<int>(), C, ctx->models.as<double>(), C, square_logit_conc,
                        dmodes, ctx->in2.as<long long>(), keep.as<double>(), st));
    double* host = pass == 0 ? matw : bmatw;
    if (host && (size_t)N * C)
      HCHK(hipMemcpyAsync(host, keep.p, sizeof(double) * (size_t)N * C, hipMemcpyDeviceToHost, st));
    RCHK(ctx->sync());  // in2 is reused by the next pass
  }
  if (N) HCHK(hipMemcpyAsync(modes, dmodes, sizeof(double) * (size_t)N * nm, hipMemcpyDeviceToHost, st));
  RCHK(ctx->sync());
  ctx->vn_n = N;
  ctx->vn_c = C;
  ctx->vn_nb = batch ? nbatch : 0;
  return SCDE_OK;
}

int scde_pagoda_varnorm_weights_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells,
                                     const double* models, int local_theta, int square_logit_conc,
                                     const double* prior_x, int ngrid, int nboot, int n_cores,
                                     const int* batch_codes, int nbatch, int use_expected_value, double* modes,
                                     double* matw, double* bmatw) {
  FORK_GUARD();
  const int* dev = nullptr;
  RCHK(stage_counts(ctx, counts, ld, ngenes, ncells, &dev));
  return scde_pagoda_varnorm_weights_dev(ctx, dev, ngenes, ngenes, ncells, models, local_theta, square_logit_conc,
                                         prior_x, ngrid, nboot, n_cores, batch_codes, nbatch, use_expected_value,
                                         modes, matw, bmatw);
}

// pagoda.varnorm after its weights (varnorm.hip).  The weights come from the caller or, with
// null pointers, from what the last weights call on this context left in HBM.
static int vn_retained(scde_ctx* ctx, int N, int C, int nb, const char* who) {
  if (ctx->vn_n != N || ctx->vn_c != C || ctx->vn_nb != nb)
    return fail(SCDE_EARG,
                "%s: no weights given and the context holds none of this shape (scde_pagoda_varnorm_weights_dev "
                "left %d x %d with %d levels; asked for %d x %d with %d)",
                who, ctx->vn_n, ctx->vn_c, ctx->vn_nb, N, C, nb);
  return SCDE_OK;
}

static int vn_check_codes(const int* codes, int C, int nb) {
  for (int c = 0; c < C; ++c)
    if (codes[c] < 0 || codes[c] >= nb) return fail(SCDE_EARG, "batch code out of range");
  return SCDE_OK;
}

int scde_pagoda_varnorm_moments_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells,
                                    const double* models, int local_theta, const double* modes_dev,
                                    const double* matw_dev, const double* bmatw_dev, const int* batch_codes,
                                    int nbatch, const double* edf_table, int edf_n, double edf_lt0, double edf_h,
                                    double theta_lo, double theta_hi, double weight_df_power, double* out) {
  FORK_GUARD();
  if (!ctx || !counts_dev || !models || !edf_table || !out) return fail(SCDE_EARG, "varnorm_moments: null argument");
  if (ngenes < 0 || ncells <= 0 || ld < ngenes) return fail(SCDE_EARG, "varnorm_moments: bad dimensions");
  if (edf_n < 2 || !(edf_h > 0.0) || !std::isfinite(edf_lt0))
    return fail(SCDE_EARG, "varnorm_moments: the edf table needs at least 2 points on an increasing uniform grid");
  const bool batch = batch_codes && nbatch > 1;
  const int nb = batch ? nbatch : 0;
  if (batch) RCHK(vn_check_codes(batch_codes, ncells, nbatch));
  if (!modes_dev && !matw_dev && !bmatw_dev) {
    RCHK(vn_retained(ctx, ngenes, ncells, nb, "varnorm_moments"));
    modes_dev = ctx->vn_modes.as<double>();
    matw_dev = ctx->vn_matw.as<double>();
    bmatw_dev = batch ? ctx->vn_bmatw.as<double>() : nullptr;
  } else if (!modes_dev || !matw_dev || (batch && !bmatw_dev)) {
    return fail(SCDE_EARG, "varnorm_moments: modes, matw (and bmatw with a batch) go together");
  }
  if (!batch) bmatw_dev = nullptr;
  const int N = ngenes, C = ncells;
  if (N == 0) return SCDE_OK;
  HCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  RCHK(upload(ctx, ctx->models, models, sizeof(double) * (size_t)C * 12));
  RCHK(upload(ctx, ctx->vn_tab, edf_table, sizeof(double) * 2 * (size_t)edf_n));
  if (batch) RCHK(upload(ctx, ctx->vn_int, batch_codes, sizeof(int) * C));
  const int nq = batch ? 7 : 3;
  HCHK(ctx->vn_vec.ensure(sizeof(double) * (size_t)N * nq));
  const VnEdf edf{ctx->vn_tab.as<double>(), ctx->vn_tab.as<double>() + edf_n, edf_n, edf_lt0, edf_h};
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  HCHK(launch_varnorm_moments(counts_dev, ld, N, C, ctx->models.as<double>(), local_theta, modes_dev, matw_dev,
                              bmatw_dev, batch ? ctx->vn_int.as<int>() : nullptr, edf, theta_lo, theta_hi,
                              weight_df_power, ctx->vn_vec.as<double>(), st));
  ctx->mark_end(SLOT_OTHER, ev);
  HCHK(hipMemcpyAsync(out, ctx->vn_vec.p, sizeof(double) * (size_t)N * nq, hipMemcpyDeviceToHost, st));
  return ctx->sync();
}

// host weights into the context's buffers (they become what the context holds)
static int vn_stage_weights(scde_ctx* ctx, int N, int C, int nb, const double* modes, const double* matw,
                            const double* bmatw) {
  ctx->vn_n = -1;
  const size_t nc = sizeof(double) * (size_t)N * C;
  HCHK(ctx->vn_matw.ensure(std::max<size_t>(1, nc)));
  if (nb) HCHK(ctx->vn_bmatw.ensure(std::max<size_t>(1, nc)));
  if (nc) {
    HCHK(hipMemcpyAsync(ctx->vn_matw.p, matw, nc, hipMemcpyHostToDevice, ctx->stream));
    if (nb) HCHK(hipMemcpyAsync(ctx->vn_bmatw.p, bmatw, nc, hipMemcpyHostToDevice, ctx->stream));
  }
  if (modes) {
    const size_t nmb = sizeof(double) * (size_t)N * (1 + nb);
    HCHK(ctx->vn_modes.ensure(std::max<size_t>(1, nmb)));
    if (nmb) HCHK(hipMemcpyAsync(ctx->vn_modes.p, modes, nmb, hipMemcpyHostToDevice, ctx->stream));
  }
  RCHK(ctx->sync());
  if (modes) {
    ctx->vn_n = N;
    ctx->vn_c = C;
    ctx->vn_nb = nb;
  }
  return SCDE_OK;
}

int scde_pagoda_varnorm_moments_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells,
                                     const double* models, int local_theta, const double* modes, const double* matw,
                                     const double* bmatw, const int* batch_codes, int nbatch, const double* edf_table,
                                     int edf_n, double edf_lt0, double edf_h, double theta_lo, double theta_hi,
                                     double weight_df_power, double* out) {
  FORK_GUARD();
  const bool batch = batch_codes && nbatch > 1;
  if (!modes || !matw || (batch && !bmatw)) return fail(SCDE_EARG, "varnorm_moments: null argument");
  const int* dev = nullptr;
  RCHK(stage_counts(ctx, counts, ld, ngenes, ncells, &dev));
  RCHK(vn_stage_weights(ctx, ngenes, ncells, batch ? nbatch : 0, modes, matw, bmatw));
  return scde_pagoda_varnorm_moments_dev(ctx, dev, ngenes, ngenes, ncells, models, local_theta,
                                         ctx->vn_modes.as<double>(), ctx->vn_matw.as<double>(),
                                         batch ? ctx->vn_bmatw.as<double>() : nullptr, batch_codes, nbatch, edf_table,
                                         edf_n, edf_lt0, edf_h, theta_lo, theta_hi, weight_df_power, out);
}

int scde_pagoda_varnorm_matrix_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells,
                                   const double* models, const double* matw_dev, const int* batch_codes, int nbatch,
                                   double weight_k, const double* arv, double* mat, double* matw_out) {
  FORK_GUARD();
  if (!ctx || !counts_dev || !models || !arv || !mat || !matw_out)
    return fail(SCDE_EARG, "varnorm_matrix: null argument");
  if (ngenes < 0 || ncells <= 0 || ld < ngenes) return fail(SCDE_EARG, "varnorm_matrix: bad dimensions");
  const bool batch = batch_codes && nbatch > 1;
  const int nb = batch ? nbatch : 0;
  if (batch) RCHK(vn_check_codes(batch_codes, ncells, nbatch));
  if (!matw_dev) {
    RCHK(vn_retained(ctx, ngenes, ncells, nb, "varnorm_matrix"));
    matw_dev = batch ? ctx->vn_bmatw.as<double>() : ctx->vn_matw.as<double>();
  }
  const int N = ngenes, C = ncells;
  if (N == 0) return SCDE_OK;
  // the cells grouped by level, in cell order within a level: order[C], then lev_off[nlev + 1]
  const int nlev = batch ? nbatch : 1;
  std::vector<int> lists((size_t)C + nlev + 1);
  int* order = lists.data();
  int* off = lists.data() + C;
  int pos = 0;
  for (int L = 0; L < nlev; ++L) {
    off[L] = pos;
    for (int c = 0; c < C; ++c)
      if (!batch || batch_codes[c] == L) order[pos++] = c;
    if (pos == off[L]) return fail(SCDE_EARG, "varnorm_matrix: batch level %d has no cells", L);
  }
  off[nlev] = pos;
  HCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t nc = sizeof(double) * (size_t)N * C;
  if (ctx->vn_mat.ensure(nc) != hipSuccess || ctx->vn_wout.ensure(nc) != hipSuccess ||
      ctx->vn_ws.ensure(sizeof(double) * 3 * (size_t)nlev * N) != hipSuccess)
    return fail_oom("varnorm_matrix: out of memory: mat and matw need %zu bytes of device memory", 2 * nc);
  RCHK(upload(ctx, ctx->models, models, sizeof(double) * (size_t)C * 12));
  RCHK(upload(ctx, ctx->vn_int, lists.data(), sizeof(int) * lists.size()));
  RCHK(upload(ctx, ctx->vn_vec, arv, sizeof(double) * N));
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  HCHK(launch_varnorm_matrix(counts_dev, ld, N, C, ctx->models.as<double>(), ctx->vn_int.as<int>(),
                             ctx->vn_int.as<int>() + C, nlev, batch ? 1 : 0, matw_dev, weight_k,
                             ctx->vn_vec.as<double>(), ctx->vn_ws.as<double>(), ctx->vn_mat.as<double>(),
                             ctx->vn_wout.as<double>(), st));
  ctx->mark_end(SLOT_OTHER, ev);
  HCHK(hipMemcpyAsync(mat, ctx->vn_mat.p, nc, hipMemcpyDeviceToHost, st));
  HCHK(hipMemcpyAsync(matw_out, ctx->vn_wout.p, nc, hipMemcpyDeviceToHost, st));
  const int rc = ctx->sync();
  if (nc > ((size_t)1 << 30)) {  // two matrices of more than 1 GB each are not kept
    ctx->vn_mat.release();
    ctx->vn_wout.release();
  }
  return rc;
}

int scde_pagoda_varnorm_matrix_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells,
                                    const double* models, const double* matw, const int* batch_codes, int nbatch,
                                    double weight_k, const double* arv, double* mat, double* matw_out) {
  FORK_GUARD();
  if (!matw) return fail(SCDE_EARG, "varnorm_matrix: null argument");
  const int* dev = nullptr;
  RCHK(stage_counts(ctx, counts, ld, ngenes, ncells, &dev));
  // (without modes the context holds no complete set afterwards: a later call must bring its own)
  RCHK(vn_stage_weights(ctx, ngenes, ncells, 0, nullptr, matw, nullptr));
  return scde_pagoda_varnorm_matrix_dev(ctx, dev, ngenes, ngenes, ncells, models, ctx->vn_matw.as<double>(),
                                        batch_codes, nbatch, weight_k, arv, mat, matw_out);
}

// pagoda.subtract.aspect (R/functions.R:1850-1862): the aspect centred and scaled to unit
// length on the host (C values), the rest in k_subtract_aspect.
static int vn_aspect_unit(const double* aspect, int C, std::vector<double>& v) {
  v.assign(aspect, aspect + C);
  double mean = 0.0;
  for (int c = 0; c < C; ++c) mean += v[c];
  mean /= C;
  double ss = 0.0;
  for (int c = 0; c < C; ++c) {
    v[c] -= mean;
    ss += v[c] * v[c];
  }
  const double nrm = std::sqrt(ss);
  for (int c = 0; c < C; ++c) v[c] /= nrm;
  return SCDE_OK;
}

int scde_pagoda_subtract_aspect_dev(scde_ctx* ctx, const double* mat_dev, const double* matw_dev, int ngenes,
                                    int ncells, const double* aspect, int center, double* out_dev) {
  FORK_GUARD();
  if (!mat_dev || !matw_dev || !aspect || !out_dev) return fail(SCDE_EARG, "subtract_aspect: null argument");
  if (ngenes < 0 || ncells <= 0) return fail(SCDE_EARG, "subtract_aspect: bad dimensions");
  RCHK(use_ctx(ctx));
  if (ngenes == 0) return SCDE_OK;
  std::vector<double> v;
  RCHK(vn_aspect_unit(aspect, ncells, v));
  RCHK(upload(ctx, ctx->vn_vec, v.data(), sizeof(double) * ncells));
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  HCHK(launch_subtract_aspect(mat_dev, matw_dev, ngenes, ncells, ctx->vn_vec.as<double>(), center, out_dev,
                              ctx->stream));
  ctx->mark_end(SLOT_OTHER, ev);
  return ctx->sync();
}

int scde_pagoda_subtract_aspect_host(scde_ctx* ctx, const double* mat, const double* matw, int ngenes, int ncells,
                                     const double* aspect, int center, double* out) {
  FORK_GUARD();
  if (!mat || !matw || !aspect || !out) return fail(SCDE_EARG, "subtract_aspect: null argument");
  if (ngenes < 0 || ncells <= 0) return fail(SCDE_EARG, "subtract_aspect: bad dimensions");
  RCHK(use_ctx(ctx));
  if (ngenes == 0) return SCDE_OK;
  const size_t nc = sizeof(double) * (size_t)ngenes * ncells;
  if (ctx->vn_mat.ensure(nc) != hipSuccess || ctx->vn_wout.ensure(nc) != hipSuccess ||
      ctx->pg_a.ensure(nc) != hipSuccess)
    return fail_oom("subtract_aspect: out of memory: three %d x %d matrices need %zu bytes of device memory",
                    ngenes, ncells, 3 * nc);
  HCHK(hipMemcpyAsync(ctx->vn_mat.p, mat, nc, hipMemcpyHostToDevice, ctx->stream));
  HCHK(hipMemcpyAsync(ctx->vn_wout.p, matw, nc, hipMemcpyHostToDevice, ctx->stream));
  RCHK(scde_pagoda_subtract_aspect_dev(ctx, ctx->vn_mat.as<double>(), ctx->vn_wout.as<double>(), ngenes, ncells,
                                       aspect, center, ctx->pg_a.as<double>()));
  HCHK(hipMemcpyAsync(out, ctx->pg_a.p, nc, hipMemcpyDeviceToHost, ctx->stream));
  return ctx->sync();
}

// ------------------------------------------------------------------ pagoda.top.aspects
// The matrix step (top_aspects.hip; contract in scde_hip.h).  Arguments are checked before the
// GPU is touched.
static int top_aspects_check(const void* x, const void* w, const void* num, int m, int ncells, const void* xv,
                             const void* xvw) {
  if (m < 0 || ncells < 1) return fail(SCDE_EARG, "top_aspects: bad dimensions (m = %d, ncells = %d)", m, ncells);
  if (m > 0 && (!x || !w || !num || !xv || !xvw)) return fail(SCDE_EARG, "top_aspects: null argument");
  return SCDE_OK;
}

int scde_top_aspects_dev(scde_ctx* ctx, const double* x_dev, const double* w_dev, const double* num, int m, int ncells,
                         double* xv_dev, double* xvw_dev) {
  FORK_GUARD();
  RCHK(top_aspects_check(x_dev, w_dev, num, m, ncells, xv_dev, xvw_dev));
  RCHK(use_ctx(ctx));
  if (m == 0) return SCDE_OK;
  RCHK(upload(ctx, ctx->ta_num, num, sizeof(double) * (size_t)m));
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  HCHK(launch_top_aspects(x_dev, w_dev, ctx->ta_num.as<double>(), m, ncells, xv_dev, xvw_dev, ctx->stream));
  ctx->mark_end(SLOT_OTHER, ev);
  return ctx->sync();
}

int scde_top_aspects(scde_ctx* ctx, const double* x, const double* w, const double* num, int m, int ncells, double* xv,
                     double* xvw) {
  FORK_GUARD();
  RCHK(top_aspects_check(x, w, num, m, ncells, xv, xvw));
  RCHK(use_ctx(ctx));
  if (m == 0) return SCDE_OK;
  const size_t nc = sizeof(double) * (size_t)m * ncells;
  if (ctx->ta_x.ensure(nc) != hipSuccess || ctx->ta_w.ensure(nc) != hipSuccess || ctx->ta_xv.ensure(nc) != hipSuccess ||
      ctx->ta_xvw.ensure(nc) != hipSuccess)
    return fail_oom("top_aspects: out of memory: four %d x %d matrices need %zu bytes of device memory", m, ncells,
                    4 * nc);
  HCHK(hipMemcpyAsync(ctx->ta_x.p, x, nc, hipMemcpyHostToDevice, ctx->stream));
  HCHK(hipMemcpyAsync(ctx->ta_w.p, w, nc, hipMemcpyHostToDevice, ctx->stream));
  RCHK(scde_top_aspects_dev(ctx, ctx->ta_x.as<double>(), ctx->ta_w.as<double>(), num, m, ncells,
                            ctx->ta_xv.as<double>(), ctx->ta_xvw.as<double>()));
  HCHK(hipMemcpyAsync(xv, ctx->ta_xv.p, nc, hipMemcpyDeviceToHost, ctx->stream));
  HCHK(hipMemcpyAsync(xvw, ctx->ta_xvw.p, nc, hipMemcpyDeviceToHost, ctx->stream));
  return ctx->sync();
}
}  // extern "C"
