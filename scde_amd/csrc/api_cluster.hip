// api_cluster.hip -- the host side of dist.hip, rdist.hip, hclust.hip, olo.hip, tsne.hip, knn.hip,
// knn_fit.hip, error_models.hip and nb2_fit.hip: the cell-to-cell distance measures, stats::dist,
// hierarchical clustering, optimal leaf ordering, exact t-SNE, and the error-model fitters
// (knn.error.models, scde.error.models).  (engine.hip is
// the pipeline; a feature's host code lives in the api_ file named after its kernel files.)
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "engine_internal.h"
#include "kernels.h"

using namespace scde;
using namespace scde::host;

extern "C" {

// ------------------------------------------------------------------ cell-to-cell distance measures
// The vignette's "Adjusted distance measures" (vignettes/diffexp.md:231-301) on the device
// (dist.hip).  Arguments are checked before the GPU is touched.
static int dist_check(const void* in, int64_t ld, int ngenes, int ncells, const double* models, const double* out) {
  if (!in || !models || !out) return fail(SCDE_EARG, "null argument");
  if (ncells < 1) return fail(SCDE_EARG, "ncells must be at least 1");
  if (ngenes < 0 || ld < ngenes) return fail(SCDE_EARG, "bad dimensions");
  return SCDE_OK;
}

// per-cell constants corr.b, corr.a, conc.b, conc.a, conc.a2 (model columns 3, 4, 0, 1, 11)
static int dist_cellp(scde_ctx* ctx, const double* models, int C, int sq) {
  std::vector<double> cellp((size_t)5 * C);
  const int mcol[5] = {3, 4, 0, 1, 11};
  for (int j = 0; j < 5; ++j)
    for (int c = 0; c < C; ++c) cellp[(size_t)j * C + c] = (j == 4 && !sq) ? 0.0 : models[(size_t)mcol[j] * C + c];
  return upload(ctx, ctx->ds_cell, cellp.data(), sizeof(double) * cellp.size());
}

static int dist_out(scde_ctx* ctx, int C, double* out) {
  HCHK(hipMemcpyAsync(out, ctx->ds_out.p, sizeof(double) * (size_t)C * C, hipMemcpyDeviceToHost, ctx->stream));
  return ctx->sync();
}

int scde_wcorr_sep_dev(scde_ctx* ctx, const double* x_dev, const double* u_dev, int64_t ld, int ngenes, int ncells,
                       double* out) {
  FORK_GUARD();
  RCHK(dist_check(x_dev, ld, ngenes, ncells, u_dev, out));
  RCHK(use_ctx(ctx));
  HCHK(ctx->ds_out.ensure(sizeof(double) * (size_t)ncells * ncells));
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);  // the pair kernels are timed in slot "other"
  HCHK(launch_wcorr_gram(x_dev, u_dev, ld, ngenes, ncells, ctx->ds_out.as<double>(), 0, ctx->stream));
  ctx->mark_end(SLOT_OTHER, ev);
  return dist_out(ctx, ncells, out);
}

int scde_wcorr_sep_host(scde_ctx* ctx, const double* x, const double* u, int64_t ld, int ngenes, int ncells,
                        double* out) {
  FORK_GUARD();
  RCHK(dist_check(x, ld, ngenes, ncells, u, out));
  RCHK(use_ctx(ctx));
  RCHK(put_matrix(ctx, ctx->ds_x, x, ld, ngenes, ncells));
  RCHK(put_matrix(ctx, ctx->ds_u, u, ld, ngenes, ncells));
  return scde_wcorr_sep_dev(ctx, ctx->ds_x.as<double>(), ctx->ds_u.as<double>(), ngenes, ngenes, ncells, out);
}

int scde_reciprocal_corr_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells,
                             const double* models, int square_logit_conc, double k, double* out) {
  FORK_GUARD();
  RCHK(dist_check(counts_dev, ld, ngenes, ncells, models, out));
  if (!(k >= 0 && k <= 1)) return fail(SCDE_EARG, "k must be in [0, 1]");
  RCHK(use_ctx(ctx));
  const int N = ngenes, C = ncells, sq = square_logit_conc != 0;
  const size_t nb = sizeof(double) * std::max<size_t>(1, (size_t)N * C);
  RCHK(dist_cellp(ctx, models, C, sq));
  HCHK(ctx->ds_x.ensure(nb));
  HCHK(ctx->ds_f.ensure(nb));
  HCHK(ctx->ds_out.ensure(sizeof(double) * (size_t)C * C));
  HCHK(launch_dist_prep(counts_dev, ld, N, C, ctx->ds_cell.as<double>(), sq, ctx->ds_x.as<double>(),
                        ctx->ds_f.as<double>(), nullptr, ctx->stream));
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  HCHK(launch_recip_corr(ctx->ds_x.as<double>(), ctx->ds_f.as<double>(), N, C, ctx->ds_cell.as<double>(), sq, k,
                         ctx->ds_out.as<double>(), ctx->stream));
  ctx->mark_end(SLOT_OTHER, ev);
  return dist_out(ctx, C, out);
}

int scde_reciprocal_corr_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells,
                              const double* models, int square_logit_conc, double k, double* out) {
  FORK_GUARD();
  RCHK(dist_check(counts, ld, ngenes, ncells, models, out));
  if (!(k >= 0 && k <= 1)) return fail(SCDE_EARG, "k must be in [0, 1]");
  const int* dev = nullptr;
  RCHK(stage_counts(ctx, counts, ld, ngenes, ncells, &dev));
  return scde_reciprocal_corr_dev(ctx, dev, ngenes, ngenes, ncells, models, square_logit_conc, k, out);
}

int scde_mode_fail_corr_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells,
                            const double* models, int square_logit_conc, const double* modes,
                            const double* jp_modes, double* out) {
  FORK_GUARD();
  RCHK(dist_check(counts_dev, ld, ngenes, ncells, models, out));
  if (!modes || !jp_modes) return fail(SCDE_EARG, "null argument");
  RCHK(use_ctx(ctx));
  const int N = ngenes, C = ncells, sq = square_logit_conc != 0;
  const size_t nb = sizeof(double) * std::max<size_t>(1, (size_t)N * C);
  RCHK(dist_cellp(ctx, models, C, sq));
  RCHK(put_matrix(ctx, ctx->ds_f, modes, N, N, C));
  RCHK(put_matrix(ctx, ctx->ds_jpm, jp_modes, N, N, 1));
  HCHK(ctx->ds_x.ensure(nb));
  HCHK(ctx->ds_u.ensure(nb));
  HCHK(ctx->ds_out.ensure(sizeof(double) * (size_t)C * C));
  HCHK(launch_dist_mode_prep(counts_dev, ld, N, C, ctx->ds_cell.as<double>(), sq, ctx->ds_f.as<double>(),
                             ctx->ds_jpm.as<double>(), ctx->ds_x.as<double>(), ctx->ds_u.as<double>(), ctx->stream));
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  HCHK(launch_wcorr_gram(ctx->ds_x.as<double>(), ctx->ds_u.as<double>(), N, N, C, ctx->ds_out.as<double>(), 0,
                         ctx->stream));
  ctx->mark_end(SLOT_OTHER, ev);
  return dist_out(ctx, C, out);
}

int scde_mode_fail_corr_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells,
                             const double* models, int square_logit_conc, const double* modes,
                             const double* jp_modes, double* out) {
  FORK_GUARD();
  RCHK(dist_check(counts, ld, ngenes, ncells, models, out));
  if (!modes || !jp_modes) return fail(SCDE_EARG, "null argument");
  const int* dev = nullptr;
  RCHK(stage_counts(ctx, counts, ld, ngenes, ncells, &dev));
  return scde_mode_fail_corr_dev(ctx, dev, ngenes, ngenes, ncells, models, square_logit_conc, modes, jp_modes, out);
}

static int direct_check(double k, int nsim) {
  if (!(k >= 0 && k <= 1)) return fail(SCDE_EARG, "k must be in [0, 1]");
  if (nsim < 1) return fail(SCDE_EARG, "nsim must be at least 1");
  return SCDE_OK;
}

int scde_direct_corr_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells,
                         const double* models, int square_logit_conc, double k, int nsim, const double* uniforms,
                         uint64_t seed, double* out) {
  FORK_GUARD();
  RCHK(dist_check(counts_dev, ld, ngenes, ncells, models, out));
  RCHK(direct_check(k, nsim));
  RCHK(use_ctx(ctx));
  const int N = ngenes, C = ncells, sq = square_logit_conc != 0;
  const long long NC = (long long)N * C;
  const size_t nb = sizeof(double) * std::max<size_t>(1, (size_t)NC);
  RCHK(dist_cellp(ctx, models, C, sq));
  HCHK(ctx->ds_x0.ensure(nb));
  HCHK(ctx->ds_p.ensure(nb));
  HCHK(ctx->ds_x.ensure(nb));
  HCHK(ctx->ds_u.ensure(nb));
  if (uniforms) HCHK(ctx->ds_f.ensure(nb));
  HCHK(ctx->ds_out.ensure(sizeof(double) * (size_t)C * C));
  HCHK(launch_dist_prep(counts_dev, ld, N, C, ctx->ds_cell.as<double>(), sq, ctx->ds_x0.as<double>(), nullptr,
                        ctx->ds_p.as<double>(), ctx->stream));
  // the rounds run one after the other on the stream and add into the result in round order
  for (int s = 0; s < nsim; ++s) {
    if (uniforms && NC)
      HCHK(hipMemcpyAsync(ctx->ds_f.p, uniforms + (size_t)s * NC, sizeof(double) * NC, hipMemcpyHostToDevice,
                          ctx->stream));
    HCHK(launch_dist_direct_prep(ctx->ds_x0.as<double>(), ctx->ds_p.as<double>(), NC, k,
                                 uniforms ? ctx->ds_f.as<double>() : nullptr, dist_sim_key(seed, s),
                                 ctx->ds_x.as<double>(), ctx->ds_u.as<double>(), ctx->stream));
    hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
    HCHK(launch_wcorr_gram(ctx->ds_x.as<double>(), ctx->ds_u.as<double>(), N, N, C, ctx->ds_out.as<double>(), s > 0,
                           ctx->stream));
    ctx->mark_end(SLOT_OTHER, ev);
  }
  RCHK(dist_out(ctx, C, out));
  for (size_t e = 0; e < (size_t)C * C; ++e) out[e] /= (double)nsim;
  return SCDE_OK;
}

int scde_direct_corr_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells, const double* models,
                          int square_logit_conc, double k, int nsim, const double* uniforms, uint64_t seed,
                          double* out) {
  FORK_GUARD();
  RCHK(dist_check(counts, ld, ngenes, ncells, models, out));
  RCHK(direct_check(k, nsim));
  const int* dev = nullptr;
  RCHK(stage_counts(ctx, counts, ld, ngenes, ncells, &dev));
  return scde_direct_corr_dev(ctx, dev, ngenes, ngenes, ncells, models, square_logit_conc, k, nsim, uniforms, seed,
                              out);
}

// ------------------------------------------------------------------ stats::dist
// R's dist between the rows of an n x p matrix (rdist.hip; contract in scde_hip.h).  Arguments
// are checked before the GPU is touched.
static int rdist_check(const void* x, int64_t ld, int n, int p, int method, const void* out) {
  if (!x || !out) return fail(SCDE_EARG, "null argument");
  if (n < 1 || p < 0) return fail(SCDE_EARG, "dist: n must be at least 1 and p at least 0");
  if (ld < n) return fail(SCDE_EARG, "dist: ld must be at least n");
  if (method < 0 || method > 2)
    return fail(SCDE_EARG, "dist: unknown method code %d (0 euclidean, 1 manhattan, 2 maximum)", method);
  if (n > (1 << 21)) return fail(SCDE_EARG, "dist: more than %d objects", 1 << 21);
  return SCDE_OK;
}

int scde_dist_dev(scde_ctx* ctx, const double* x_dev, int64_t ld, int n, int p, int method, double* out_dev) {
  FORK_GUARD();
  RCHK(rdist_check(x_dev, ld, n, p, method, out_dev));
  RCHK(use_ctx(ctx));
  HCHK(ctx->rd_flag.ensure(sizeof(int)));
  HCHK(launch_rdist_flag(x_dev, ld, n, p, ctx->rd_flag.as<int>(), ctx->stream));
  int flag = 0;
  HCHK(hipMemcpyAsync(&flag, ctx->rd_flag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
  RCHK(ctx->sync());
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  HCHK(launch_rdist(x_dev, ld, n, p, method, flag != 0, out_dev, ctx->stream));
  ctx->mark_end(SLOT_OTHER, ev);
  return ctx->sync();
}

int scde_dist_host(scde_ctx* ctx, const double* x, int64_t ld, int n, int p, int method, double* out) {
  FORK_GUARD();
  RCHK(rdist_check(x, ld, n, p, method, out));
  RCHK(use_ctx(ctx));
  const size_t ob = sizeof(double) * (size_t)n * n;
  if (ctx->hc_in.ensure(ob) != hipSuccess)
    return fail_oom("dist: out of memory: the result needs %zu bytes of device memory", ob);
  RCHK(put_matrix(ctx, ctx->rd_x, x, ld, n, p));
  int rc = scde_dist_dev(ctx, ctx->rd_x.as<double>(), n, n, p, method, ctx->hc_in.as<double>());
  if (rc == SCDE_OK) {
    hipError_t e = hipMemcpyAsync(out, ctx->hc_in.p, ob, hipMemcpyDeviceToHost, ctx->stream);
    rc = e != hipSuccess ? fail(SCDE_EHIP, "dist: %s", hipGetErrorString(e)) : ctx->sync();
  }
  if (sizeof(double) * (size_t)n * p > ((size_t)1 << 30)) ctx->rd_x.release();
  if (ob > ((size_t)1 << 30)) ctx->hc_in.release();
  return rc;
}

// ------------------------------------------------------------------ hierarchical clustering
// stats::hclust / cutree's tree for the monotone linkages (hclust.hip; contract in scde_hip.h).
// Arguments are checked before the GPU is touched.

// a host n x n matrix (hclust's, order.optimal's) into hc_in; the caller drops it afterwards
// (drop_square) when it is more than 1 GB
static int stage_square(scde_ctx* ctx, const double* d, int64_t ld, int n, const char* who) {
  if (ctx->hc_in.ensure(sizeof(double) * (size_t)n * n) != hipSuccess)
    return fail_oom("%s: out of memory: the matrix needs %zu bytes of device memory", who,
                    sizeof(double) * (size_t)n * n);
  return put_matrix(ctx, ctx->hc_in, d, ld, n, n);
}

static void drop_square(scde_ctx* ctx, int n) {
  if (sizeof(double) * (size_t)n * n > ((size_t)1 << 30)) ctx->hc_in.release();
}

static int hclust_run(scde_ctx* ctx, int nprob, const double* d_dev, const int64_t* off, const int64_t* ldv,
                      const int* n, int method, int* merge, double* height, int* order) {
  RCHK(use_ctx(ctx));
  std::vector<HclustProblem> pr(nprob);
  size_t wsb = 0, steps = 0;
  for (int p = 0; p < nprob; ++p) {
    pr[p] = {(long long)off[p], (long long)ldv[p], (long long)wsb, (long long)steps, n[p]};
    wsb += hclust_ws_bytes(n[p]);
    steps += (size_t)n[p] - 1;
  }
  // the workspace comes first: a problem that does not fit fails here, before any launch
  if (ctx->hc_ws.ensure(wsb) != hipSuccess)
    return fail_oom("hclust: out of memory: the workspace of %d problem(s) needs %zu bytes of device memory",
                    nprob, wsb);
  RCHK(upload(ctx, ctx->hc_prob, pr.data(), sizeof(HclustProblem) * pr.size()));
  // oh (doubles), flags (long long), oi, oj (ints)
  const size_t ob = steps * (sizeof(double) + 2 * sizeof(int)) + sizeof(long long) * nprob;
  HCHK(ctx->hc_out.ensure(ob));
  double* oh = ctx->hc_out.as<double>();
  long long* flag = reinterpret_cast<long long*>(oh + steps);
  int* oi = reinterpret_cast<int*>(flag + nprob);
  int* oj = oi + steps;
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  HCHK(launch_hclust(d_dev, ctx->hc_prob.as<HclustProblem>(), nprob, method, ctx->hc_ws.as<char>(), oi, oj, oh, flag,
                     ctx->stream));
  ctx->mark_end(SLOT_OTHER, ev);
  std::vector<char> host(ob);
  HCHK(hipMemcpyAsync(host.data(), ctx->hc_out.p, ob, hipMemcpyDeviceToHost, ctx->stream));
  RCHK(ctx->sync());
  if (wsb > ((size_t)1 << 30)) ctx->hc_ws.release();  // a 20,000-object workspace is 3.2 GB: not kept
  const double* hh = reinterpret_cast<const double*>(host.data());
  const long long* hf = reinterpret_cast<const long long*>(hh + steps);
  const int* hi = reinterpret_cast<const int*>(hf + nprob);
  const int* hj = hi + steps;
  for (int p = 0; p < nprob; ++p) {
    if (hf[p] >= 0)
      return fail(SCDE_EARG, "hclust: problem %d: non-finite distance at row %lld, column %lld (1-based)", p,
                  hf[p] % n[p] + 1, hf[p] / n[p] + 1);
    if (hf[p] != -1)
      return fail(SCDE_EINTERNAL, "hclust: problem %d: no pair to merge at step %lld", p, -2 - hf[p]);
  }
  size_t so = 0, oo = 0;
  for (int p = 0; p < nprob; ++p) {
    hclust_encode(n[p], hi + so, hj + so, hh + so, method, merge + 2 * so, height + so, order + oo);
    so += (size_t)n[p] - 1;
    oo += (size_t)n[p];
  }
  return SCDE_OK;
}

static int hclust_check(const void* d, int64_t ld, int n, int method, const void* merge, const void* height,
                        const void* order) {
  if (!d || !merge || !height || !order) return fail(SCDE_EARG, "null argument");
  if (n < 2) return fail(SCDE_EARG, "hclust: at least 2 objects are needed (n = %d)", n);
  if (ld < n) return fail(SCDE_EARG, "hclust: ld must be at least n");
  if (method < 0 || method > 5)
    return fail(SCDE_EARG, "hclust: unknown method code %d (0 ward.D, 1 ward.D2, 2 single, 3 complete, 4 average, "
                "5 mcquitty)", method);
  return SCDE_OK;
}

int scde_hclust_dev(scde_ctx* ctx, const double* d_dev, int64_t ld, int n, int method, int* merge, double* height,
                    int* order) {
  FORK_GUARD();
  RCHK(hclust_check(d_dev, ld, n, method, merge, height, order));
  const int64_t off = 0;
  return hclust_run(ctx, 1, d_dev, &off, &ld, &n, method, merge, height, order);
}

int scde_hclust_host(scde_ctx* ctx, const double* d, int64_t ld, int n, int method, int* merge, double* height,
                     int* order) {
  FORK_GUARD();
  RCHK(hclust_check(d, ld, n, method, merge, height, order));
  RCHK(use_ctx(ctx));
  RCHK(stage_square(ctx, d, ld, n, "hclust"));
  const int64_t off = 0, ldn = n;
  const int rc = hclust_run(ctx, 1, ctx->hc_in.as<double>(), &off, &ldn, &n, method, merge, height, order);
  drop_square(ctx, n);
  return rc;
}

int scde_hclust_batch_dev(scde_ctx* ctx, int nprob, const double* d_dev, const int64_t* off, const int* n,
                          int method, int* merge, double* height, int* order) {
  FORK_GUARD();
  if (nprob < 0) return fail(SCDE_EARG, "hclust: nprob must not be negative");
  if (nprob == 0) return SCDE_OK;
  if (!off || !n) return fail(SCDE_EARG, "null argument");
  std::vector<int64_t> ldv(nprob);
  for (int p = 0; p < nprob; ++p) {
    if (off[p] < 0) return fail(SCDE_EARG, "hclust: problem %d: negative offset", p);
    RCHK(hclust_check(d_dev, n[p], n[p], method, merge, height, order));
    ldv[p] = n[p];
  }
  return hclust_run(ctx, nprob, d_dev, off, ldv.data(), n, method, merge, height, order);
}

// ------------------------------------------------------------------ optimal leaf ordering
// cba::order.optimal (olo.hip; contract in scde_hip.h).  The arguments and the merge matrix are
// checked on the host before the GPU is touched.
static int olo_check(const void* d, int64_t ld, int n, const int* merge, const int* merge_out, const int* order_out) {
  if (!d || !merge || !merge_out || !order_out) return fail(SCDE_EARG, "null argument");
  if (n < 2) return fail(SCDE_EARG, "order.optimal: at least 2 objects are needed (n = %d)", n);
  if (ld < n) return fail(SCDE_EARG, "order.optimal: ld must be at least n");
  const uintptr_t mb = (uintptr_t)merge, mob = (uintptr_t)merge_out, oob = (uintptr_t)order_out;
  const uintptr_t me = mb + sizeof(int) * 2 * (size_t)(n - 1), moe = mob + sizeof(int) * 2 * (size_t)(n - 1),
                  ooe = oob + sizeof(int) * (size_t)n;
  if ((mob < me && mb < moe) || (oob < me && mb < ooe) || (oob < moe && mob < ooe))
    return fail(SCDE_EARG, "order.optimal: merge_out and order_out must not alias merge or each other");
  char msg[256];
  if (olo_check_merge(n, merge, msg, sizeof(msg))) return fail(SCDE_EARG, "%s", msg);
  return SCDE_OK;
}

static int olo_run(scde_ctx* ctx, const double* d_dev, int64_t ld, int n, const int* merge, int* merge_out,
                   int* order_out, double* length) {
  char msg[256] = "";
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  const int rc = olo_solve(ctx->stream, d_dev, ld, n, merge, merge_out, order_out, length, ctx->st_olo, msg,
                           sizeof(msg));
  ctx->mark_end(SLOT_OTHER, ev);
  RCHK(ctx->sync());
  if (rc) return fail(rc == 1 ? SCDE_EARG : rc == 2 ? SCDE_EHIP : SCDE_EINTERNAL, "%s", msg);
  return SCDE_OK;
}

int scde_order_optimal_dev(scde_ctx* ctx, const double* d_dev, int64_t ld, int n, const int* merge, int* merge_out,
                           int* order_out, double* length) {
  FORK_GUARD();
  RCHK(olo_check(d_dev, ld, n, merge, merge_out, order_out));
  RCHK(use_ctx(ctx));
  return olo_run(ctx, d_dev, ld, n, merge, merge_out, order_out, length);
}

int scde_order_optimal_host(scde_ctx* ctx, const double* d, int64_t ld, int n, const int* merge, int* merge_out,
                            int* order_out, double* length) {
  FORK_GUARD();
  RCHK(olo_check(d, ld, n, merge, merge_out, order_out));
  for (int j = 0; j < n - 1; ++j)
    for (int i = j + 1; i < n; ++i)
      if (!std::isfinite(d[i + (size_t)j * ld]))
        return fail(SCDE_EARG, "order.optimal: non-finite distance at row %d, column %d (1-based)", i + 1, j + 1);
  RCHK(use_ctx(ctx));
  RCHK(stage_square(ctx, d, ld, n, "order.optimal"));
  const int rc = olo_run(ctx, ctx->hc_in.as<double>(), n, n, merge, merge_out, order_out, length);
  drop_square(ctx, n);
  return rc;
}

// ------------------------------------------------------------------ exact t-SNE
// The 2-D embedding of a distance matrix (tsne.hip; contract in scde_hip.h).  Arguments are
// checked before the GPU is touched.
static int tsne_check_n(int n) {
  if (n < 4) return fail(SCDE_EARG, "tsne: at least 4 objects are needed (n = %d)", n);
  return SCDE_OK;
}

static int tsne_check_perplexity(int n, double perplexity) {
  RCHK(tsne_check_n(n));
  if (!(perplexity >= 1.0) || !(3.0 * perplexity <= (double)(n - 1)))
    return fail(SCDE_EARG, "tsne: perplexity must be at least 1 and 3 * perplexity at most n - 1 (perplexity = %g, "
                "n = %d)", perplexity, n);
  return SCDE_OK;
}

static int tsne_check_params(const TsneParams& p, int iter0, int niter) {
  if (!std::isfinite(p.eta) || !std::isfinite(p.exaggeration) || !std::isfinite(p.momentum) ||
      !std::isfinite(p.final_momentum))
    return fail(SCDE_EARG, "tsne: eta, exaggeration, momentum and final_momentum must be finite");
  if (iter0 < 0 || niter < 0) return fail(SCDE_EARG, "tsne: iter0 and the number of iterations must not be negative");
  return SCDE_OK;
}

static int tsne_check_ws(int n, const void* ws, int64_t ws_bytes) {
  if (!ws || ws_bytes < (int64_t)tsne_ws_bytes(n))
    return fail(SCDE_EARG, "tsne: the workspace is missing or too small (%lld bytes given, scde_tsne_ws_bytes(%d) = "
                "%zu)", ws ? (long long)ws_bytes : 0ll, n, tsne_ws_bytes(n));
  if ((uintptr_t)ws & 7) return fail(SCDE_EARG, "tsne: the workspace must be 8-byte aligned");
  return SCDE_OK;
}

static int tsne_rc(int rc, const char* msg) {
  return rc ? fail(rc == 1 ? SCDE_EARG : SCDE_EHIP, "%s", msg) : SCDE_OK;
}

int scde_tsne_ws_bytes(int n, int64_t* bytes) {
  if (!bytes) return fail(SCDE_EARG, "null argument");
  RCHK(tsne_check_n(n));
  *bytes = (int64_t)tsne_ws_bytes(n);
  return SCDE_OK;
}

int scde_tsne_affinities_dev(scde_ctx* ctx, const double* d_dev, int64_t ld, int n, double perplexity, int squared,
                             double* P_dev, double* beta, void* ws_dev, int64_t ws_bytes) {
  FORK_GUARD();
  if (!d_dev || !P_dev || !beta) return fail(SCDE_EARG, "null argument");
  RCHK(tsne_check_perplexity(n, perplexity));
  if (ld < n) return fail(SCDE_EARG, "tsne: ld must be at least n");
  RCHK(tsne_check_ws(n, ws_dev, ws_bytes));
  RCHK(use_ctx(ctx));
  char msg[256] = "";
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  const int rc = tsne_affinities(ctx->stream, d_dev, ld, n, perplexity, squared, P_dev, beta,
                                 static_cast<char*>(ws_dev), msg, sizeof(msg));
  ctx->mark_end(SLOT_OTHER, ev);
  return tsne_rc(rc, msg);
}

int scde_tsne_iterate_dev(scde_ctx* ctx, const double* P_dev, int n, double eta, double exaggeration,
                          int stop_lying_iter, int mom_switch_iter, double momentum, double final_momentum,
                          int iter0, int niter, double* Y_dev, double* uY_dev, double* gains_dev, void* ws_dev,
                          int64_t ws_bytes) {
  FORK_GUARD();
  if (!P_dev || !Y_dev || !uY_dev || !gains_dev) return fail(SCDE_EARG, "null argument");
  RCHK(tsne_check_n(n));
  const TsneParams prm = {eta, exaggeration, momentum, final_momentum, stop_lying_iter, mom_switch_iter};
  RCHK(tsne_check_params(prm, iter0, niter));
  RCHK(tsne_check_ws(n, ws_dev, ws_bytes));
  if (((uintptr_t)Y_dev | (uintptr_t)uY_dev | (uintptr_t)gains_dev) & 15)
    return fail(SCDE_EARG, "tsne: Y, uY and gains must be 16-byte aligned");
  RCHK(use_ctx(ctx));
  char msg[256] = "";
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  const int rc = tsne_iterate(ctx->stream, P_dev, n, prm, iter0, niter, Y_dev, uY_dev, gains_dev,
                              static_cast<char*>(ws_dev), msg, sizeof(msg));
  ctx->mark_end(SLOT_OTHER, ev);
  return tsne_rc(rc, msg);
}

int scde_tsne_cost_dev(scde_ctx* ctx, const double* P_dev, int n, const double* Y_dev, double* costs, void* ws_dev,
                       int64_t ws_bytes) {
  FORK_GUARD();
  if (!P_dev || !Y_dev || !costs) return fail(SCDE_EARG, "null argument");
  RCHK(tsne_check_n(n));
  RCHK(tsne_check_ws(n, ws_dev, ws_bytes));
  if ((uintptr_t)Y_dev & 15) return fail(SCDE_EARG, "tsne: Y must be 16-byte aligned");
  RCHK(use_ctx(ctx));
  char msg[256] = "";
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  const int rc = tsne_cost(ctx->stream, P_dev, n, Y_dev, costs, static_cast<char*>(ws_dev), msg, sizeof(msg));
  ctx->mark_end(SLOT_OTHER, ev);
  return tsne_rc(rc, msg);
}

int scde_tsne_host(scde_ctx* ctx, const double* d, int64_t ld, int n, double perplexity, int squared, double eta,
                   double exaggeration, int stop_lying_iter, int mom_switch_iter, double momentum,
                   double final_momentum, int max_iter, uint32_t seed, const double* Y_init, double* Y, double* costs,
                   double* beta, double* P) {
  FORK_GUARD();
  if (!d || !Y || !costs || !beta) return fail(SCDE_EARG, "null argument");
  RCHK(tsne_check_perplexity(n, perplexity));
  if (ld < n) return fail(SCDE_EARG, "tsne: ld must be at least n");
  const TsneParams prm = {eta, exaggeration, momentum, final_momentum, stop_lying_iter, mom_switch_iter};
  RCHK(tsne_check_params(prm, 0, max_iter));
  const size_t nn = (size_t)n;
  std::vector<double> y0(2 * nn);
  if (Y_init) {
    std::copy(Y_init, Y_init + 2 * nn, y0.begin());
  } else {  // 1e-4 * rnorm(2 n) after set.seed(seed), point by point
    uint32_t state[625];
    RCHK(scde_r_set_seed(seed, state));
    RCHK(scde_r_norm_rand(state, (int64_t)(2 * nn), y0.data()));
    for (double& v : y0) v = 1e-4 * v;
  }
  RCHK(use_ctx(ctx));
  // d, P; then Y, uY, gains; then the workspace: one allocation, freed before the call returns
  const size_t mat = (sizeof(double) * nn * nn + 255) / 256 * 256, vec = (16 * nn + 255) / 256 * 256;
  const size_t total = 2 * mat + 3 * vec + tsne_ws_bytes(n);
  char* base = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&base), total) != hipSuccess)
    return fail_oom("tsne: out of memory: %d objects need %zu bytes of device memory", n, total);
  double *dd = reinterpret_cast<double*>(base), *Pd = reinterpret_cast<double*>(base + mat),
         *Yd = reinterpret_cast<double*>(base + 2 * mat), *Ud = reinterpret_cast<double*>(base + 2 * mat + vec),
         *Gd = reinterpret_cast<double*>(base + 2 * mat + 2 * vec);
  char* ws = base + 2 * mat + 3 * vec;
  char msg[256] = "";
  hipStream_t st = ctx->stream;
  std::vector<double> ones(2 * nn, 1.0);
  int rc = 0;
  hipError_t e = hipSuccess;
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  do {
    const size_t row = sizeof(double) * nn;
    if (!ok(ld == n ? hipMemcpyAsync(dd, d, row * nn, hipMemcpyHostToDevice, st)
                    : hipMemcpy2DAsync(dd, row, d, sizeof(double) * (size_t)ld, row, nn, hipMemcpyHostToDevice, st)))
      break;
    if (!ok(hipMemcpyAsync(Yd, y0.data(), 16 * nn, hipMemcpyHostToDevice, st))) break;
    if (!ok(hipMemcpyAsync(Gd, ones.data(), 16 * nn, hipMemcpyHostToDevice, st))) break;
    if (!ok(hipMemsetAsync(Ud, 0, 16 * nn, st))) break;
    if ((rc = tsne_affinities(st, dd, n, n, perplexity, squared, Pd, beta, ws, msg, sizeof(msg)))) break;
    if ((rc = tsne_iterate(st, Pd, n, prm, 0, max_iter, Yd, Ud, Gd, ws, msg, sizeof(msg)))) break;
    if ((rc = tsne_cost(st, Pd, n, Yd, costs, ws, msg, sizeof(msg)))) break;
    if (!ok(hipMemcpyAsync(Y, Yd, 16 * nn, hipMemcpyDeviceToHost, st))) break;
    if (P && !ok(hipMemcpyAsync(P, Pd, sizeof(double) * nn * nn, hipMemcpyDeviceToHost, st))) break;
    ok(hipStreamSynchronize(st));
  } while (false);
  ctx->mark_end(SLOT_OTHER, ev);
  if (e != hipSuccess || rc) (void)hipStreamSynchronize(st);
  const hipError_t ef = hipFree(base);
  if (rc) return tsne_rc(rc, msg);
  if (e != hipSuccess || ef != hipSuccess)
    return fail(SCDE_EHIP, "tsne: %s", hipGetErrorString(e != hipSuccess ? e : ef));
  return SCDE_OK;
}

// ------------------------------------------------------------------ knn.error.models' neighbourhood stage
// knn.hip; contract in scde_hip.h.  Arguments are checked before the GPU is touched.
static int knn_check(const void* counts, int64_t ld, int ngenes, int ncells, const char* who) {
  if (!counts) return fail(SCDE_EARG, "%s: null argument", who);
  if (ncells < 1 || ngenes < 0 || ld < ngenes)
    return fail(SCDE_EARG, "%s: bad dimensions (ngenes = %d, ncells = %d)", who, ngenes, ncells);
  if (ncells > kKnnMaxCells)
    return fail(SCDE_EARG, "%s: %d cells, at most %d are supported", who, ncells, kKnnMaxCells);
  return SCDE_OK;
}

int scde_knn_similarity_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells, int thr,
                            double* out) {
  FORK_GUARD();
  RCHK(knn_check(counts_dev, ld, ngenes, ncells, "knn_similarity"));
  if (!out) return fail(SCDE_EARG, "knn_similarity: null argument");
  RCHK(use_ctx(ctx));
  const int N = ngenes, C = ncells;
  const size_t nb = sizeof(double) * std::max<size_t>(1, (size_t)N * C), cc = sizeof(double) * (size_t)C * C;
  ctx->kn_sim_c = -1;
  if (ctx->ds_x.ensure(nb) != hipSuccess || ctx->ds_u.ensure(nb) != hipSuccess || ctx->kn_sim.ensure(cc) != hipSuccess)
    return fail_oom("knn_similarity: out of memory: two %d x %d matrices and a %d x %d one need %zu bytes", N, C, C, C,
                    2 * nb + cc);
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  HCHK(launch_knn_prep(counts_dev, ld, N, C, thr, ctx->ds_x.as<double>(), ctx->ds_u.as<double>(), ctx->stream));
  HCHK(launch_wcorr_gram(ctx->ds_x.as<double>(), ctx->ds_u.as<double>(), N, N, C, ctx->kn_sim.as<double>(), 0,
                         ctx->stream));
  ctx->mark_end(SLOT_OTHER, ev);
  HCHK(hipMemcpyAsync(out, ctx->kn_sim.p, cc, hipMemcpyDeviceToHost, ctx->stream));
  RCHK(ctx->sync());
  ctx->kn_sim_c = C;
  return SCDE_OK;
}

int scde_knn_similarity_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells, int thr,
                             double* out) {
  FORK_GUARD();
  RCHK(knn_check(counts, ld, ngenes, ncells, "knn_similarity"));
  if (!out) return fail(SCDE_EARG, "knn_similarity: null argument");
  const int* dev = nullptr;
  RCHK(stage_counts(ctx, counts, ld, ngenes, ncells, &dev));
  return scde_knn_similarity_dev(ctx, dev, ngenes, ngenes, ncells, thr, out);
}

// ------------------------------------------------------------------ Spearman (spearman.hip)
int scde_rank_cols_dev(scde_ctx* ctx, const double* x_dev, int nrow, int ncol, double* out_dev) {
  FORK_GUARD();
  if (!x_dev || !out_dev) return fail(SCDE_EARG, "rank_cols: null argument");
  if (nrow < 1 || ncol < 1) return fail(SCDE_EARG, "rank_cols: bad dimensions (nrow = %d, ncol = %d)", nrow, ncol);
  RCHK(use_ctx(ctx));
  double* tmp = nullptr;
  if (x_dev == out_dev && rank_cols_needs_tmp(nrow)) {
    const size_t nb = sizeof(double) * (size_t)nrow * ncol;
    if (ctx->sp_tmp.ensure(nb) != hipSuccess)
      return fail_oom("rank_cols: out of memory: ranking %d rows in place needs %zu bytes of device memory", nrow, nb);
    tmp = ctx->sp_tmp.as<double>();
  }
  HCHK(launch_rank_cols(x_dev, nrow, ncol, out_dev, tmp, ctx->stream));
  return ctx->sync();
}

int scde_rank_cols_host(scde_ctx* ctx, const double* x, int nrow, int ncol, double* out) {
  FORK_GUARD();
  if (!x || !out) return fail(SCDE_EARG, "rank_cols: null argument");
  if (nrow < 1 || ncol < 1) return fail(SCDE_EARG, "rank_cols: bad dimensions (nrow = %d, ncol = %d)", nrow, ncol);
  RCHK(use_ctx(ctx));
  const size_t nb = sizeof(double) * (size_t)nrow * ncol;
  if (ctx->sp_x.ensure(nb) != hipSuccess || (rank_cols_needs_tmp(nrow) && ctx->sp_tmp.ensure(nb) != hipSuccess))
    return fail_oom("rank_cols: out of memory: a %d x %d matrix needs %zu bytes of device memory", nrow, ncol, nb);
  HCHK(hipMemcpyAsync(ctx->sp_x.p, x, nb, hipMemcpyHostToDevice, ctx->stream));
  HCHK(launch_rank_cols(ctx->sp_x.as<double>(), nrow, ncol, ctx->sp_x.as<double>(), ctx->sp_tmp.as<double>(),
                        ctx->stream));
  HCHK(hipMemcpyAsync(out, ctx->sp_x.p, nb, hipMemcpyDeviceToHost, ctx->stream));
  return ctx->sync();
}

// 4 m^3 < 2^63 keeps the centred sums exact in int64
static constexpr int kSpearmanMaxGenes = 1300000;

int scde_spearman_similarity_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells, int thr,
                                 int lds_values, double* out) {
  FORK_GUARD();
  RCHK(knn_check(counts_dev, ld, ngenes, ncells, "spearman_similarity"));
  if (!out) return fail(SCDE_EARG, "spearman_similarity: null argument");
  if (ngenes > kSpearmanMaxGenes)
    return fail(SCDE_EARG, "spearman_similarity: %d genes, at most %d are supported", ngenes, kSpearmanMaxGenes);
  if (lds_values < 0) return fail(SCDE_EARG, "spearman_similarity: lds_values must not be negative");
  RCHK(use_ctx(ctx));
  const int N = ngenes, C = ncells;
  const size_t cb = std::max<size_t>(1, (size_t)spearman_code_bytes(N) * spearman_code_ld(N) * C), cc = sizeof(double) * (size_t)C * C;
  const size_t w1 = spearman_codes_ws_bytes(N, C);
  ctx->kn_sim_c = -1;
  if (ctx->sp_codes.ensure(cb) != hipSuccess || ctx->sp_d.ensure(sizeof(int) * (size_t)C) != hipSuccess ||
      ctx->kn_sim.ensure(cc) != hipSuccess || (w1 && ctx->sp_ws.ensure(w1) != hipSuccess))
    return fail_oom("spearman_similarity: out of memory: the codes of %d x %d counts, a %d x %d matrix and the "
                    "workspace need %zu bytes",
                    N, C, C, C, cb + cc + w1);
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  HCHK(launch_spearman_codes(counts_dev, ld, N, C, thr, ctx->sp_codes.p, ctx->sp_d.as<int>(),
                             w1 ? ctx->sp_ws.as<unsigned>() : nullptr, ctx->stream));
  // the tables are sized from the largest number of distinct values the prepass found
  std::vector<int> D((size_t)C);
  HCHK(hipMemcpyAsync(D.data(), ctx->sp_d.p, sizeof(int) * (size_t)C, hipMemcpyDeviceToHost, ctx->stream));
  RCHK(ctx->sync());
  int dmax = 0;
  for (int c = 0; c < C; ++c) {
    if (D[c] < 0 || D[c] > N) return fail(SCDE_EHIP, "spearman_similarity: cell %d has %d distinct values", c, D[c]);
    dmax = std::max(dmax, D[c]);
  }
  const size_t w2 = spearman_pairs_ws_bytes(C, dmax, lds_values);
  if (w2 && ctx->sp_ws.ensure(w2) != hipSuccess)
    return fail_oom("spearman_similarity: out of memory: the tables of the pairs too large for LDS need %zu bytes",
                    w2);
  HCHK(launch_spearman_pairs(ctx->sp_codes.p, N, C, ctx->sp_d.as<int>(), dmax, lds_values,
                             w2 ? ctx->sp_ws.as<unsigned>() : nullptr, ctx->kn_sim.as<double>(), ctx->stream));
  ctx->mark_end(SLOT_OTHER, ev);
  HCHK(hipMemcpyAsync(out, ctx->kn_sim.p, cc, hipMemcpyDeviceToHost, ctx->stream));
  RCHK(ctx->sync());
  ctx->kn_sim_c = C;
  return SCDE_OK;
}

int scde_spearman_similarity_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells, int thr,
                                  int lds_values, double* out) {
  FORK_GUARD();
  RCHK(knn_check(counts, ld, ngenes, ncells, "spearman_similarity"));
  if (!out) return fail(SCDE_EARG, "spearman_similarity: null argument");
  for (int c = 0; c < ncells; ++c)
    for (int g = 0; g < ngenes; ++g)
      if (counts[(size_t)c * ld + g] < 0)
        return fail(SCDE_EARG, "spearman_similarity: count (%d, %d) is negative", g, c);
  const int* dev = nullptr;
  RCHK(stage_counts(ctx, counts, ld, ngenes, ncells, &dev));
  return scde_spearman_similarity_dev(ctx, dev, ngenes, ngenes, ncells, thr, lds_values, out);
}

int scde_knn_neighbours(scde_ctx* ctx, const double* sim, int ncells, const int* groups, int k, int kmax, int* out) {
  FORK_GUARD();
  const int C = ncells;
  if (C < 1 || C > kKnnMaxCells)
    return fail(SCDE_EARG, "knn_neighbours: %d cells, 1 to %d are supported", C, kKnnMaxCells);
  if (k < 0 || kmax < 0) return fail(SCDE_EARG, "knn_neighbours: k and kmax must not be negative");
  if (kmax > 0 && !out) return fail(SCDE_EARG, "knn_neighbours: null argument");
  // groups as codes 0, 1, ... in order of first appearance; each cell's k = min(k, its group - 1)
  std::vector<int> meta((size_t)2 * C), first, size;
  for (int c = 0; c < C; ++c) {
    const int gc = groups ? groups[c] : 0;
    size_t p = 0;
    while (p < first.size() && first[p] != gc) ++p;
    if (p == first.size()) {
      if (p >= 4096) return fail(SCDE_EARG, "knn_neighbours: more than 4096 groups");
      first.push_back(gc);
      size.push_back(0);
    }
    meta[c] = (int)p;
    ++size[p];
  }
  int need = 0;
  for (int c = 0; c < C; ++c) {
    meta[(size_t)C + c] = std::min(k, size[meta[c]] - 1);
    need = std::max(need, meta[(size_t)C + c]);
  }
  if (kmax < need)
    return fail(SCDE_EARG, "knn_neighbours: kmax = %d, the largest group needs %d columns", kmax, need);
  RCHK(use_ctx(ctx));
  if (!sim && ctx->kn_sim_c != C)
    return fail(SCDE_EARG, "knn_neighbours: no resident similarity of %d cells (the last one had %d)", C,
                ctx->kn_sim_c);
  ctx->kn_nb_c = -1;
  if (kmax == 0) {
    ctx->kn_nb_c = C;
    ctx->kn_nb_k = 0;
    return SCDE_OK;
  }
  if (sim) {
    ctx->kn_sim_c = -1;
    HCHK(ctx->kn_sim.ensure(sizeof(double) * (size_t)C * C));
    HCHK(hipMemcpyAsync(ctx->kn_sim.p, sim, sizeof(double) * (size_t)C * C, hipMemcpyHostToDevice, ctx->stream));
  }
  const size_t ob = sizeof(int) * (size_t)C * kmax;
  HCHK(ctx->kn_nb.ensure(ob));
  RCHK(upload(ctx, ctx->kn_int, meta.data(), sizeof(int) * meta.size()));
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  HCHK(launch_knn_neighbours(ctx->kn_sim.as<double>(), C, ctx->kn_int.as<int>(), ctx->kn_int.as<int>() + C, kmax,
                             ctx->kn_nb.as<int>(), ctx->stream));
  ctx->mark_end(SLOT_OTHER, ev);
  HCHK(hipMemcpyAsync(out, ctx->kn_nb.p, ob, hipMemcpyDeviceToHost, ctx->stream));
  RCHK(ctx->sync());
  if (sim) ctx->kn_sim_c = C;
  ctx->kn_nb_c = C;
  ctx->kn_nb_k = kmax;
  return SCDE_OK;
}

static int knn_mag_check(int ncells, const int* nb, int kmax, const double* ls, int thr, double trim, const void* fpm,
                         const void* nabove) {
  if (!ls || !fpm || !nabove) return fail(SCDE_EARG, "knn_magnitudes: null argument");
  if (kmax < 0) return fail(SCDE_EARG, "knn_magnitudes: kmax must not be negative");
  if (!(trim >= 0.0)) return fail(SCDE_EARG, "knn_magnitudes: trim must be at least 0");
  for (int c = 0; c < ncells; ++c)
    if (!(ls[c] >= 0.0) || std::isinf(ls[c]) || (ls[c] == 0.0 && thr <= 0))  // (0 / 0 has no place in an order)
      return fail(SCDE_EARG, "knn_magnitudes: library size %d is not a finite number %s 0", c,
                  thr <= 0 ? "above" : "of at least");
  if (nb) {
    std::vector<int> seen((size_t)ncells, -1);  // the last row that listed each cell
    for (size_t e = 0; e < (size_t)ncells * kmax; ++e) {
      const int j = nb[e], i = (int)(e / kmax);
      if (j < -1 || j >= ncells)
        return fail(SCDE_EARG, "knn_magnitudes: neighbour %d of cell %d is outside [-1, %d)", j, i, ncells);
      if (j >= 0 && seen[j] == i) return fail(SCDE_EARG, "knn_magnitudes: cell %d lists neighbour %d twice", i, j);
      if (j >= 0) seen[j] = i;
    }
  }
  return SCDE_OK;
}

int scde_knn_magnitudes_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells, const int* nb,
                            int kmax, const double* ls, int thr, double trim, double* fpm, int* nabove) {
  FORK_GUARD();
  RCHK(knn_check(counts_dev, ld, ngenes, ncells, "knn_magnitudes"));
  RCHK(knn_mag_check(ncells, nb, kmax, ls, thr, trim, fpm, nabove));
  RCHK(use_ctx(ctx));
  const int N = ngenes, C = ncells;
  if (!nb && (ctx->kn_nb_c != C || ctx->kn_nb_k != kmax))
    return fail(SCDE_EARG, "knn_magnitudes: no resident neighbours of %d cells x %d (the last were %d x %d)", C, kmax,
                ctx->kn_nb_c, ctx->kn_nb_k);
  if (N == 0) return SCDE_OK;
  const size_t nc = (size_t)N * C;
  if (ctx->kn_fpm.ensure(sizeof(double) * nc) != hipSuccess || ctx->kn_nab.ensure(sizeof(int) * nc) != hipSuccess)
    return fail_oom("knn_magnitudes: out of memory: the %d x %d results need %zu bytes of device memory", N, C,
                    12 * nc);
  if (nb && kmax > 0) {
    ctx->kn_nb_c = -1;
    HCHK(ctx->kn_nb.ensure(sizeof(int) * (size_t)C * kmax));
    HCHK(hipMemcpyAsync(ctx->kn_nb.p, nb, sizeof(int) * (size_t)C * kmax, hipMemcpyHostToDevice, ctx->stream));
  }
  RCHK(upload(ctx, ctx->kn_ls, ls, sizeof(double) * (size_t)C));
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  HCHK(launch_knn_magnitudes(counts_dev, ld, N, C, ctx->kn_nb.as<int>(), kmax, ctx->kn_ls.as<double>(), thr, trim,
                             ctx->kn_fpm.as<double>(), ctx->kn_nab.as<int>(), ctx->stream));
  ctx->mark_end(SLOT_OTHER, ev);
  HCHK(hipMemcpyAsync(fpm, ctx->kn_fpm.p, sizeof(double) * nc, hipMemcpyDeviceToHost, ctx->stream));
  HCHK(hipMemcpyAsync(nabove, ctx->kn_nab.p, sizeof(int) * nc, hipMemcpyDeviceToHost, ctx->stream));
  RCHK(ctx->sync());
  if (nb) {
    ctx->kn_nb_c = C;
    ctx->kn_nb_k = kmax;
  }
  return SCDE_OK;
}

int scde_knn_magnitudes_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells, const int* nb,
                             int kmax, const double* ls, int thr, double trim, double* fpm, int* nabove) {
  FORK_GUARD();
  RCHK(knn_check(counts, ld, ngenes, ncells, "knn_magnitudes"));
  RCHK(knn_mag_check(ncells, nb, kmax, ls, thr, trim, fpm, nabove));
  const int* dev = nullptr;
  RCHK(stage_counts(ctx, counts, ld, ngenes, ncells, &dev));
  return scde_knn_magnitudes_dev(ctx, dev, ngenes, ngenes, ncells, nb, kmax, ls, thr, trim, fpm, nabove);
}

// ------------------------------------------------------------------ the per-cell mixture fits
// knn_fit.hip (knn.error.models; scde.error.models with linear.fit = TRUE) and nb2_fit.hip
// (linear.fit = FALSE); contracts in scde_hip.h.
static int fit_check(const char* who, const double* fpm, const double* fail_prior, int max_iter, int lds_genes,
                     const void* models, const void* iterations, const void* llh, const void* status) {
  if ((fpm == nullptr) != (fail_prior == nullptr) || !models || !iterations || !llh || !status)
    return fail(SCDE_EARG, "%s: null argument", who);
  if (max_iter < 1) return fail(SCDE_EARG, "%s: max_iter must be at least 1", who);
  if (lds_genes < 0 || lds_genes > knn_fit_lds_genes_max())
    return fail(SCDE_EARG, "%s: lds_genes must lie in [0, %d]", who, knn_fit_lds_genes_max());
  return SCDE_OK;
}

static int knn_fit_check(const double* fpm, const double* fail_prior, double theta_lo, double theta_hi, double awp,
                         int max_iter, int lds_genes, const void* models, const void* iterations, const void* llh,
                         const void* status) {
  RCHK(fit_check("knn_fit", fpm, fail_prior, max_iter, lds_genes, models, iterations, llh, status));
  if (!(theta_lo > 0.0) || !(theta_hi > theta_lo) || std::isinf(theta_hi))
    return fail(SCDE_EARG, "knn_fit: the theta range must be 0 < lo < hi < Inf");
  if (!std::isfinite(awp)) return fail(SCDE_EARG, "knn_fit: alpha_weight_power must be finite");
  return SCDE_OK;
}

static int nb2_fit_check(const double* fpm, const double* fail_prior, double background_rate, int max_iter,
                         int lds_genes, const void* models, const void* iterations, const void* llh,
                         const void* status) {
  RCHK(fit_check("nb2_fit", fpm, fail_prior, max_iter, lds_genes, models, iterations, llh, status));
  if (!(background_rate > 0.0) || std::isinf(background_rate))
    return fail(SCDE_EARG, "nb2_fit: background_rate must be a positive finite number");
  return SCDE_OK;
}

// which fit, and its parameters
struct CellFit {
  bool nb2;
  int local_theta;
  double theta_lo, theta_hi, awp;  // knn_fit
  double background_rate;          // nb2_fit
};

// Stages the inputs (or takes the resident ones of the last crossfit_inputs call when fpm and
// fail_prior are null), sizes the workspace, launches the fit and brings the results back.
static int cell_fit_dev(scde_ctx* ctx, const char* who, const CellFit& f, const int* counts_dev, int64_t ld, int N,
                        int C, const double* fpm, const double* fail_prior, int max_iter, int lds_genes,
                        double* models, int* iterations, double* llh, int* status, int* clusters, double* post) {
  const int cap = lds_genes > 0 ? lds_genes : 2048;
  long long nmax = 0;  // the largest cell's valid genes
  if (fail_prior) {
    for (int c = 0; c < C; ++c) {
      long long n = 0;
      const double* p = fail_prior + (size_t)c * N;
      for (int g = 0; g < N; ++g) n += std::isnan(p[g]) ? 0 : 1;
      nmax = std::max(nmax, n);
    }
  }
  RCHK(use_ctx(ctx));
  if (!fail_prior) {
    if (ctx->ci_n != N || ctx->ci_c != C)
      return fail(SCDE_EARG, "%s: no resident inputs of %d genes x %d cells (the last were %d x %d)", who, N, C,
                  ctx->ci_n, ctx->ci_c);
    nmax = ctx->ci_nmax;
  }
  int grid = 1;
  HCHK(f.nb2 ? nb2_fit_resident_groups(cap, &grid) : knn_fit_resident_groups(cap, &grid));
  grid = std::min(grid, C);
  const size_t nc = std::max<size_t>(1, (size_t)N * C);
  const size_t wsb = nmax > cap ? knn_fit_ws_bytes(nmax) * (size_t)grid : 0;
  if ((fail_prior && (ctx->kf_fpm.ensure(sizeof(double) * nc) != hipSuccess ||
                      ctx->kf_fp.ensure(sizeof(double) * nc) != hipSuccess)) ||
      (wsb && ctx->kf_ws.ensure(wsb) != hipSuccess) ||
      (clusters && ctx->kf_cl.ensure(sizeof(int) * nc) != hipSuccess) ||
      (post && ctx->kf_post.ensure(sizeof(double) * nc) != hipSuccess))
    return fail_oom("%s: out of memory: %d x %d inputs and a workspace of %zu bytes", who, N, C, wsb);
  HCHK(ctx->kf_models.ensure(sizeof(double) * 12 * (size_t)C));
  HCHK(ctx->kf_llh.ensure(sizeof(double) * (size_t)C));
  HCHK(ctx->kf_int.ensure(sizeof(int) * 2 * (size_t)C));
  if (fail_prior) {
    ctx->ci_n = ctx->ci_c = -1;  // (the staging buffers are the resident inputs' home)
    if (N > 0) {
      HCHK(hipMemcpyAsync(ctx->kf_fpm.p, fpm, sizeof(double) * (size_t)N * C, hipMemcpyHostToDevice, ctx->stream));
      HCHK(hipMemcpyAsync(ctx->kf_fp.p, fail_prior, sizeof(double) * (size_t)N * C, hipMemcpyHostToDevice,
                          ctx->stream));
    }
  }
  char* ws = wsb ? ctx->kf_ws.as<char>() : nullptr;
  int* cl = clusters ? ctx->kf_cl.as<int>() : nullptr;
  double* po = post ? ctx->kf_post.as<double>() : nullptr;
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  if (f.nb2)
    HCHK(launch_nb2_fit(counts_dev, ld, N, C, ctx->kf_fpm.as<double>(), ctx->kf_fp.as<double>(), f.background_rate,
                        std::log(f.background_rate), max_iter, cap, ws, nmax, grid, ctx->kf_models.as<double>(),
                        ctx->kf_int.as<int>(), ctx->kf_llh.as<double>(), ctx->kf_int.as<int>() + C, cl, po,
                        ctx->stream));
  else
    HCHK(launch_knn_fit(counts_dev, ld, N, C, ctx->kf_fpm.as<double>(), ctx->kf_fp.as<double>(), f.local_theta != 0,
                        f.theta_lo, f.theta_hi, f.awp, max_iter, cap, ws, nmax, grid, ctx->kf_models.as<double>(),
                        ctx->kf_int.as<int>(), ctx->kf_llh.as<double>(), ctx->kf_int.as<int>() + C, cl, po,
                        ctx->stream));
  ctx->mark_end(SLOT_OTHER, ev);
  HCHK(hipMemcpyAsync(models, ctx->kf_models.p, sizeof(double) * 12 * (size_t)C, hipMemcpyDeviceToHost, ctx->stream));
  HCHK(hipMemcpyAsync(iterations, ctx->kf_int.p, sizeof(int) * (size_t)C, hipMemcpyDeviceToHost, ctx->stream));
  HCHK(hipMemcpyAsync(status, ctx->kf_int.as<int>() + C, sizeof(int) * (size_t)C, hipMemcpyDeviceToHost,
                      ctx->stream));
  HCHK(hipMemcpyAsync(llh, ctx->kf_llh.p, sizeof(double) * (size_t)C, hipMemcpyDeviceToHost, ctx->stream));
  if (clusters && N > 0)
    HCHK(hipMemcpyAsync(clusters, ctx->kf_cl.p, sizeof(int) * (size_t)N * C, hipMemcpyDeviceToHost, ctx->stream));
  if (post && N > 0)
    HCHK(hipMemcpyAsync(post, ctx->kf_post.p, sizeof(double) * (size_t)N * C, hipMemcpyDeviceToHost, ctx->stream));
  RCHK(ctx->sync());
  return SCDE_OK;
}

int scde_knn_fit_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells, const double* fpm,
                     const double* fail_prior, int local_theta, double theta_lo, double theta_hi,
                     double alpha_weight_power, int max_iter, int lds_genes, double* models, int* iterations,
                     double* llh, int* status, int* clusters, double* post) {
  FORK_GUARD();
  RCHK(knn_check(counts_dev, ld, ngenes, ncells, "knn_fit"));
  RCHK(knn_fit_check(fpm, fail_prior, theta_lo, theta_hi, alpha_weight_power, max_iter, lds_genes, models, iterations,
                     llh, status));
  const CellFit f = {false, local_theta, theta_lo, theta_hi, alpha_weight_power, 0.0};
  return cell_fit_dev(ctx, "knn_fit", f, counts_dev, ld, ngenes, ncells, fpm, fail_prior, max_iter, lds_genes, models,
                      iterations, llh, status, clusters, post);
}

int scde_knn_fit_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells, const double* fpm,
                      const double* fail_prior, int local_theta, double theta_lo, double theta_hi,
                      double alpha_weight_power, int max_iter, int lds_genes, double* models, int* iterations,
                      double* llh, int* status, int* clusters, double* post) {
  FORK_GUARD();
  RCHK(knn_check(counts, ld, ngenes, ncells, "knn_fit"));
  RCHK(knn_fit_check(fpm, fail_prior, theta_lo, theta_hi, alpha_weight_power, max_iter, lds_genes, models, iterations,
                     llh, status));
  const int* dev = nullptr;
  RCHK(stage_counts(ctx, counts, ld, ngenes, ncells, &dev));
  return scde_knn_fit_dev(ctx, dev, ngenes, ngenes, ncells, fpm, fail_prior, local_theta, theta_lo, theta_hi,
                          alpha_weight_power, max_iter, lds_genes, models, iterations, llh, status, clusters, post);
}

int scde_nb2_fit_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells, const double* fpm,
                     const double* fail_prior, double background_rate, int max_iter, int lds_genes, double* models,
                     int* iterations, double* llh, int* status, int* clusters, double* post) {
  FORK_GUARD();
  RCHK(knn_check(counts_dev, ld, ngenes, ncells, "nb2_fit"));
  RCHK(nb2_fit_check(fpm, fail_prior, background_rate, max_iter, lds_genes, models, iterations, llh, status));
  const CellFit f = {true, 0, 0.0, 0.0, 0.0, background_rate};
  return cell_fit_dev(ctx, "nb2_fit", f, counts_dev, ld, ngenes, ncells, fpm, fail_prior, max_iter, lds_genes, models,
                      iterations, llh, status, clusters, post);
}

int scde_nb2_fit_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells, const double* fpm,
                      const double* fail_prior, double background_rate, int max_iter, int lds_genes, double* models,
                      int* iterations, double* llh, int* status, int* clusters, double* post) {
  FORK_GUARD();
  RCHK(knn_check(counts, ld, ngenes, ncells, "nb2_fit"));
  RCHK(nb2_fit_check(fpm, fail_prior, background_rate, max_iter, lds_genes, models, iterations, llh, status));
  const int* dev = nullptr;
  RCHK(stage_counts(ctx, counts, ld, ngenes, ncells, &dev));
  return scde_nb2_fit_dev(ctx, dev, ngenes, ngenes, ncells, fpm, fail_prior, background_rate, max_iter, lds_genes,
                          models, iterations, llh, status, clusters, post);
}

// ------------------------------------------------------------------ scde.error.models' input stage
// error_models.hip; contract in scde_hip.h.  The lists are checked before the GPU is touched: the
// kernels index with them.
struct CrossfitLists {
  std::vector<int> ints;  // goff (ngroups + 1), members (C), need (C), poff (C + 1), part
  int ngroups = 0;
};

static int crossfit_check(int ncells, const int* groups, const double* ls, const int* part_off,
                          const int* part, int thr, int min_nonfailed, CrossfitLists* out) {
  const int C = ncells;
  if (!ls || !part_off) return fail(SCDE_EARG, "crossfit_inputs: null argument");
  if (thr < 1) return fail(SCDE_EARG, "crossfit_inputs: thr must be at least 1");
  if (min_nonfailed < 0) return fail(SCDE_EARG, "crossfit_inputs: min_nonfailed must not be negative");
  for (int c = 0; c < C; ++c)
    if (!(ls[c] > 0.0) || std::isinf(ls[c]))
      return fail(SCDE_EARG, "crossfit_inputs: library size %d is not a positive finite number", c);
  // groups in order of first appearance; members group by group, each in cell order
  std::vector<int> code((size_t)C), first, size;
  for (int c = 0; c < C; ++c) {
    const int gc = groups ? groups[c] : 0;
    size_t p = 0;
    while (p < first.size() && first[p] != gc) ++p;
    if (p == first.size()) {
      if (p >= 4096) return fail(SCDE_EARG, "crossfit_inputs: more than 4096 groups");
      first.push_back(gc);
      size.push_back(0);
    }
    code[c] = (int)p;
    ++size[p];
  }
  const int G = (int)first.size();
  for (int p = 0; p < G; ++p)
    if (size[p] < 2) return fail(SCDE_EARG, "crossfit_inputs: group %d has a single cell", first[p]);
  if (part_off[0] != 0) return fail(SCDE_EARG, "crossfit_inputs: part_off must start at 0");
  for (int c = 0; c < C; ++c)
    if (part_off[c + 1] < part_off[c]) return fail(SCDE_EARG, "crossfit_inputs: part_off must not decrease");
  const int P = part_off[C];
  if (P > 0 && !part) return fail(SCDE_EARG, "crossfit_inputs: null argument");
  std::vector<int> seen((size_t)C, -1);  // the last cell that listed each cell
  for (int c = 0; c < C; ++c)
    for (int k = part_off[c]; k < part_off[c + 1]; ++k) {
      const int j = part[k];
      if (j < 0 || j >= C || j == c || code[j] != code[c])
        return fail(SCDE_EARG, "crossfit_inputs: partner %d of cell %d is not another cell of its group", j, c);
      if (seen[j] == c) return fail(SCDE_EARG, "crossfit_inputs: cell %d lists partner %d twice", c, j);
      seen[j] = c;
    }
  std::vector<int>& v = out->ints;
  v.assign((size_t)(G + 1) + C + C + (C + 1) + P, 0);
  int* goff = v.data();
  int* members = goff + G + 1;
  int* need = members + C;
  int* poff = need + C;
  int* pl = poff + C + 1;
  for (int p = 0; p < G; ++p) goff[p + 1] = goff[p] + size[p];
  std::vector<int> at(goff, goff + G);
  for (int c = 0; c < C; ++c) {
    members[at[code[c]]++] = c;
    need[c] = std::min(size[code[c]] - 1, min_nonfailed);
  }
  for (int c = 0; c <= C; ++c) poff[c] = part_off[c];
  for (int k = 0; k < P; ++k) pl[k] = part[k];
  out->ngroups = G;
  return SCDE_OK;
}

int scde_crossfit_inputs_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells,
                             const int* groups, const double* ls, const int* part_off, const int* part, int thr,
                             int min_nonfailed, double* fpm, double* fail_prior, int* nabove) {
  FORK_GUARD();
  RCHK(knn_check(counts_dev, ld, ngenes, ncells, "crossfit_inputs"));
  CrossfitLists L;
  RCHK(crossfit_check(ncells, groups, ls, part_off, part, thr, min_nonfailed, &L));
  RCHK(use_ctx(ctx));
  const int N = ngenes, C = ncells, G = L.ngroups;
  ctx->ci_n = ctx->ci_c = -1;
  const size_t nc = std::max<size_t>(1, (size_t)N * C);
  if (ctx->kf_fpm.ensure(sizeof(double) * nc) != hipSuccess || ctx->kf_fp.ensure(sizeof(double) * nc) != hipSuccess ||
      ctx->ci_nab.ensure(sizeof(int) * nc) != hipSuccess)
    return fail_oom("crossfit_inputs: out of memory: the %d x %d results need %zu bytes of device memory", N, C,
                    20 * nc);
  // the lists, then the cells' valid-gene counters
  const size_t li = L.ints.size();
  L.ints.resize(li + (size_t)C, 0);
  RCHK(upload(ctx, ctx->ci_int, L.ints.data(), sizeof(int) * L.ints.size()));
  RCHK(upload(ctx, ctx->ci_ls, ls, sizeof(double) * (size_t)C));
  const int* goff = ctx->ci_int.as<int>();
  const int* members = goff + G + 1;
  const int* need = members + C;
  const int* poff = need + C;
  const int* pl = poff + C + 1;
  int* nvalid = ctx->ci_int.as<int>() + li;
  std::vector<int> nv((size_t)C, 0);
  if (N > 0) {
    hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
    HCHK(launch_crossfit_inputs(counts_dev, ld, N, C, G, goff, members, need, poff, pl, ctx->ci_ls.as<double>(), thr,
                                ctx->kf_fpm.as<double>(), ctx->kf_fp.as<double>(), ctx->ci_nab.as<int>(), nvalid,
                                ctx->stream));
    ctx->mark_end(SLOT_OTHER, ev);
    HCHK(hipMemcpyAsync(nv.data(), nvalid, sizeof(int) * (size_t)C, hipMemcpyDeviceToHost, ctx->stream));
    const size_t db = sizeof(double) * (size_t)N * C;
    if (fpm) HCHK(hipMemcpyAsync(fpm, ctx->kf_fpm.p, db, hipMemcpyDeviceToHost, ctx->stream));
    if (fail_prior) HCHK(hipMemcpyAsync(fail_prior, ctx->kf_fp.p, db, hipMemcpyDeviceToHost, ctx->stream));
    if (nabove)
      HCHK(hipMemcpyAsync(nabove, ctx->ci_nab.p, sizeof(int) * (size_t)N * C, hipMemcpyDeviceToHost, ctx->stream));
  }
  RCHK(ctx->sync());
  long long nmax = 0;
  for (int c = 0; c < C; ++c) nmax = std::max<long long>(nmax, nv[c]);
  ctx->ci_nmax = nmax;
  ctx->ci_n = N;
  ctx->ci_c = C;
  return SCDE_OK;
}

int scde_crossfit_inputs_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells,
                              const int* groups, const double* ls, const int* part_off, const int* part, int thr,
                              int min_nonfailed, double* fpm, double* fail_prior, int* nabove) {
  FORK_GUARD();
  RCHK(knn_check(counts, ld, ngenes, ncells, "crossfit_inputs"));
  CrossfitLists L;
  RCHK(crossfit_check(ncells, groups, ls, part_off, part, thr, min_nonfailed, &L));
  const int* dev = nullptr;
  RCHK(stage_counts(ctx, counts, ld, ngenes, ncells, &dev));
  return scde_crossfit_inputs_dev(ctx, dev, ngenes, ngenes, ncells, groups, ls, part_off, part, thr, min_nonfailed,
                                  fpm, fail_prior, nabove);
}

// ------------------------------------------------------------------ the mixture cross-fit of pairs
// crossfit_fit.hip; contract in scde_hip.h.  The pairs are checked before the GPU is touched: the
// kernel indexes the counts with them.
static int crossfit_fit_check(int ncells, const int* pairs, int npairs, int thr, double min_prior,
                              double zero_lambda, int max_iter, int lds_rows) {
  if (npairs < 0 || (npairs > 0 && !pairs)) return fail(SCDE_EARG, "crossfit_fit: null argument");
  if (thr < 0) return fail(SCDE_EARG, "crossfit_fit: thr must not be negative");
  if (!(min_prior >= 0.0) || !(min_prior < 1.0)) return fail(SCDE_EARG, "crossfit_fit: min_prior must lie in [0, 1)");
  if (!(zero_lambda > 0.0) || std::isinf(zero_lambda))
    return fail(SCDE_EARG, "crossfit_fit: zero_lambda must be a positive finite number");
  if (max_iter < 1) return fail(SCDE_EARG, "crossfit_fit: max_iter must be at least 1");
  if (lds_rows < 0 || lds_rows > crossfit_fit_lds_rows_max())
    return fail(SCDE_EARG, "crossfit_fit: lds_rows must lie in [0, %d]", crossfit_fit_lds_rows_max());
  for (int p = 0; p < npairs; ++p) {
    const int a = pairs[p], b = pairs[(size_t)npairs + p];
    if (a < 0 || a >= ncells || b < 0 || b >= ncells || a == b)
      return fail(SCDE_EARG, "crossfit_fit: pair %d does not hold two different cells in [0, %d)", p, ncells);
  }
  return SCDE_OK;
}

int scde_crossfit_fit_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells, const int* pairs,
                          int npairs, int thr, double min_prior, double zero_lambda, int max_iter, int lds_rows,
                          int* status, int* iterations, double* llh, double* params, int8_t* clusters,
                          double* posterior) {
  FORK_GUARD();
  RCHK(knn_check(counts_dev, ld, ngenes, ncells, "crossfit_fit"));
  RCHK(crossfit_fit_check(ncells, pairs, npairs, thr, min_prior, zero_lambda, max_iter, lds_rows));
  RCHK(use_ctx(ctx));
  const int N = ngenes, P = npairs;
  ctx->cf_n = ctx->cf_p = -1;
  if (P == 0) {
    ctx->cf_pairs_h.clear();
    ctx->cf_status_h.clear();
    ctx->cf_n = N;
    ctx->cf_p = 0;
    return SCDE_OK;
  }
  const int cap = lds_rows > 0 ? lds_rows : 2048;
  int grid = 1;
  HCHK(crossfit_fit_resident_groups(cap, &grid));
  grid = std::min(grid, P);
  const size_t np = std::max<size_t>(1, (size_t)N * P);
  const size_t wsb = N > cap ? crossfit_fit_ws_bytes(N) * (size_t)grid : 0;
  if ((wsb && ctx->cf_ws.ensure(wsb) != hipSuccess) || ctx->cf_cl.ensure(np) != hipSuccess ||
      ctx->cf_post.ensure(sizeof(double) * 2 * np) != hipSuccess)
    return fail_oom("crossfit_fit: out of memory: %d genes x %d pairs of results (%zu bytes) and a workspace of %zu "
                    "bytes", N, P, 17 * np, wsb);
  HCHK(ctx->cf_par.ensure(sizeof(double) * 11 * (size_t)P));
  HCHK(ctx->cf_int.ensure(sizeof(int) * 4 * (size_t)P));
  HCHK(hipMemcpyAsync(ctx->cf_int.p, pairs, sizeof(int) * 2 * (size_t)P, hipMemcpyHostToDevice, ctx->stream));
  int* first = ctx->cf_int.as<int>();
  int* st = first + 2 * (size_t)P;
  int* its = st + P;
  double* par = ctx->cf_par.as<double>();
  double* lh = par + 10 * (size_t)P;
  hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
  HCHK(launch_crossfit_fit(counts_dev, ld, N, P, first, first + P, thr, min_prior, zero_lambda, max_iter, cap,
                           wsb ? ctx->cf_ws.as<char>() : nullptr, N, grid, st, its, lh, par,
                           ctx->cf_cl.as<signed char>(), ctx->cf_post.as<double>(), ctx->stream));
  ctx->mark_end(SLOT_OTHER, ev);
  ctx->cf_status_h.assign((size_t)P, 0);
  HCHK(hipMemcpyAsync(ctx->cf_status_h.data(), st, sizeof(int) * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
  if (iterations) HCHK(hipMemcpyAsync(iterations, its, sizeof(int) * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
  if (llh) HCHK(hipMemcpyAsync(llh, lh, sizeof(double) * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
  if (params) HCHK(hipMemcpyAsync(params, par, sizeof(double) * 10 * (size_t)P, hipMemcpyDeviceToHost, ctx->stream));
  if (clusters && N > 0)
    HCHK(hipMemcpyAsync(clusters, ctx->cf_cl.p, (size_t)N * P, hipMemcpyDeviceToHost, ctx->stream));
  if (posterior && N > 0)
    HCHK(hipMemcpyAsync(posterior, ctx->cf_post.p, sizeof(double) * 2 * (size_t)N * P, hipMemcpyDeviceToHost,
                        ctx->stream));
  RCHK(ctx->sync());
  if (status) std::copy(ctx->cf_status_h.begin(), ctx->cf_status_h.end(), status);
  ctx->cf_pairs_h.assign(pairs, pairs + 2 * (size_t)P);
  ctx->cf_n = N;
  ctx->cf_p = P;
  return SCDE_OK;
}

int scde_crossfit_fit_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells, const int* pairs,
                           int npairs, int thr, double min_prior, double zero_lambda, int max_iter, int lds_rows,
                           int* status, int* iterations, double* llh, double* params, int8_t* clusters,
                           double* posterior) {
  FORK_GUARD();
  RCHK(knn_check(counts, ld, ngenes, ncells, "crossfit_fit"));
  RCHK(crossfit_fit_check(ncells, pairs, npairs, thr, min_prior, zero_lambda, max_iter, lds_rows));
  const int* dev = nullptr;
  RCHK(stage_counts(ctx, counts, ld, ngenes, ncells, &dev));
  return scde_crossfit_fit_dev(ctx, dev, ngenes, ngenes, ncells, pairs, npairs, thr, min_prior, zero_lambda,
                               max_iter, lds_rows, status, iterations, llh, params, clusters, posterior);
}

// ------------------------------------------------------------------ from pair results to the fit's inputs
// error_models.hip's k_reduce_*; contract in scde_hip.h.
struct ReduceLists {
  CrossfitLists L;         // crossfit_check's, from the partner lists the pairs give
  std::vector<int> plist;  // per cell, in the pairs' order: 2 * pair + side
};

static int crossfit_reduce_check(int ngenes, int ncells, const int* groups, const double* ls, const int* pairs,
                                 int npairs, const int* status, const int8_t* clusters, int min_nonfailed,
                                 ReduceLists* out) {
  const int C = ncells, P = npairs;
  if (P < 0 || (P > 0 && !pairs)) return fail(SCDE_EARG, "crossfit_reduce: null argument");
  if (P > (1 << 30)) return fail(SCDE_EARG, "crossfit_reduce: too many pairs");
  for (int p = 0; p < P; ++p) {
    const int a = pairs[p], b = pairs[(size_t)P + p];
    if (a < 0 || a >= C || b < 0 || b >= C || a == b)
      return fail(SCDE_EARG, "crossfit_reduce: pair %d does not hold two different cells in [0, %d)", p, C);
  }
  std::vector<int> off((size_t)C + 1, 0), part(2 * (size_t)P);
  for (int p = 0; p < P; ++p) {
    ++off[(size_t)pairs[p] + 1];
    ++off[(size_t)pairs[(size_t)P + p] + 1];
  }
  for (int c = 0; c < C; ++c) off[c + 1] += off[c];
  std::vector<int> at(off.begin(), off.end() - 1);
  out->plist.assign(2 * (size_t)P, 0);
  for (int p = 0; p < P; ++p)
    for (int side = 0; side < 2; ++side) {
      const int c = pairs[(size_t)side * P + p], o = pairs[(size_t)(1 - side) * P + p];
      part[at[c]] = o;
      out->plist[at[c]++] = 2 * p + side;
    }
  std::vector<double> one;
  if (!ls) one.assign((size_t)C, 1.0);
  RCHK(crossfit_check(C, groups, ls ? ls : one.data(), off.data(), part.data(), 1, min_nonfailed, &out->L));
  if (status) {
    for (int c = 0; c < C; ++c) {
      bool any = off[c + 1] == off[c];
      for (int k = off[c]; k < off[c + 1] && !any; ++k) any = status[out->plist[k] >> 1] == 0;
      if (!any) return fail(SCDE_EARG, "crossfit_reduce: every pair of cell %d failed", c);
    }
  }
  if (clusters)
    for (size_t i = 0; i < (size_t)ngenes * P; ++i)
      if (clusters[i] < 0 || clusters[i] > 3)
        return fail(SCDE_EARG, "crossfit_reduce: clusters must hold the codes 0 to 3");
  return SCDE_OK;
}

int scde_crossfit_reduce_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells,
                             const int* groups, const double* ls, const int* pairs, int npairs, const int* status,
                             const int8_t* clusters, const double* posterior, int min_nonfailed, uint8_t* vil,
                             double* fpm, double* fail_prior, int* nabove) {
  FORK_GUARD();
  RCHK(knn_check(counts_dev, ld, ngenes, ncells, "crossfit_reduce"));
  const bool given = status || clusters || posterior;
  if (given && npairs > 0 && !(status && clusters && posterior))
    return fail(SCDE_EARG, "crossfit_reduce: status, clusters and posterior come together, or all NULL");
  if (!ls && (fpm || fail_prior || nabove))
    return fail(SCDE_EARG, "crossfit_reduce: without library sizes only vil is computed");
  RCHK(use_ctx(ctx));
  const int N = ngenes, C = ncells, P = npairs;
  if (!given) {
    if (ctx->cf_n != N || ctx->cf_p != P || !std::equal(ctx->cf_pairs_h.begin(), ctx->cf_pairs_h.end(), pairs))
      return fail(SCDE_EARG, "crossfit_reduce: no resident fit of these %d pairs over %d genes (the last had %d "
                             "pairs over %d genes)", P, N, ctx->cf_p, ctx->cf_n);
    status = ctx->cf_status_h.data();
  }
  ReduceLists R;
  RCHK(crossfit_reduce_check(N, C, groups, ls, pairs, P, status, given ? clusters : nullptr, min_nonfailed, &R));
  const int G = R.L.ngroups;
  ctx->ci_n = ctx->ci_c = -1;
  const size_t nc = std::max<size_t>(1, (size_t)N * C), np = std::max<size_t>(1, (size_t)N * P);
  if (ctx->kf_fpm.ensure(sizeof(double) * nc) != hipSuccess || ctx->kf_fp.ensure(sizeof(double) * nc) != hipSuccess ||
      ctx->ci_nab.ensure(sizeof(int) * nc) != hipSuccess || ctx->cf_vil.ensure(nc) != hipSuccess ||
      (given && (ctx->cf_cl.ensure(np) != hipSuccess || ctx->cf_post.ensure(sizeof(double) * 2 * np) != hipSuccess)))
    return fail_oom("crossfit_reduce: out of memory: %d x %d results and %d x %d pair results need %zu bytes of "
                    "device memory", N, C, N, P, 21 * nc + 17 * np);
  if (given) {
    ctx->cf_n = ctx->cf_p = -1;  // (the staging buffers are the resident pair results' home)
    if (N > 0 && P > 0) {
      HCHK(hipMemcpyAsync(ctx->cf_cl.p, clusters, (size_t)N * P, hipMemcpyHostToDevice, ctx->stream));
      HCHK(hipMemcpyAsync(ctx->cf_post.p, posterior, sizeof(double) * 2 * (size_t)N * P, hipMemcpyHostToDevice,
                          ctx->stream));
    }
  }
  // the group lists and the partner offsets (crossfit_check's, its partner list replaced by the
  // pair entries), the pairs' status, then the cells' valid-gene counters
  std::vector<int>& v = R.L.ints;
  const size_t head = (size_t)(G + 1) + C + C + (C + 1);
  std::copy(R.plist.begin(), R.plist.end(), v.begin() + head);
  const size_t so = v.size();
  v.insert(v.end(), status, status + P);
  const size_t li = v.size();
  v.resize(li + (size_t)C, 0);
  RCHK(upload(ctx, ctx->cf_red, v.data(), sizeof(int) * v.size()));
  if (ls) RCHK(upload(ctx, ctx->ci_ls, ls, sizeof(double) * (size_t)C));
  const int* goff = ctx->cf_red.as<int>();
  const int* members = goff + G + 1;
  const int* need = members + C;
  const int* poff = need + C;
  const int* pl = poff + C + 1;
  const int* pst = ctx->cf_red.as<int>() + so;
  int* nvalid = ctx->cf_red.as<int>() + li;
  std::vector<int> nv((size_t)C, 0);
  if (N > 0) {
    hipEvent_t ev = ctx->mark_begin(SLOT_OTHER);
    if (ls)
      HCHK(launch_crossfit_reduce(counts_dev, ld, N, C, G, goff, members, need, poff, pl, pst,
                                  ctx->cf_cl.as<signed char>(), ctx->cf_post.as<double>(), ctx->ci_ls.as<double>(),
                                  ctx->cf_vil.as<unsigned char>(), ctx->kf_fpm.as<double>(), ctx->kf_fp.as<double>(),
                                  ctx->ci_nab.as<int>(), nvalid, ctx->stream));
    else
      HCHK(launch_crossfit_vil(N, C, poff, pl, pst, ctx->cf_cl.as<signed char>(), ctx->cf_post.as<double>(),
                               ctx->cf_vil.as<unsigned char>(), ctx->kf_fp.as<double>(), ctx->stream));
    ctx->mark_end(SLOT_OTHER, ev);
    HCHK(hipMemcpyAsync(nv.data(), nvalid, sizeof(int) * (size_t)C, hipMemcpyDeviceToHost, ctx->stream));
    const size_t db = sizeof(double) * (size_t)N * C;
    if (vil) HCHK(hipMemcpyAsync(vil, ctx->cf_vil.p, (size_t)N * C, hipMemcpyDeviceToHost, ctx->stream));
    if (fpm) HCHK(hipMemcpyAsync(fpm, ctx->kf_fpm.p, db, hipMemcpyDeviceToHost, ctx->stream));
    if (fail_prior) HCHK(hipMemcpyAsync(fail_prior, ctx->kf_fp.p, db, hipMemcpyDeviceToHost, ctx->stream));
    if (nabove)
      HCHK(hipMemcpyAsync(nabove, ctx->ci_nab.p, sizeof(int) * (size_t)N * C, hipMemcpyDeviceToHost, ctx->stream));
  }
  RCHK(ctx->sync());
  if (given) {
    ctx->cf_pairs_h.assign(pairs, pairs + 2 * (size_t)P);
    ctx->cf_status_h.assign(status, status + P);
    ctx->cf_n = N;
    ctx->cf_p = P;
  }
  if (ls) {
    long long nmax = 0;
    for (int c = 0; c < C; ++c) nmax = std::max<long long>(nmax, nv[c]);
    ctx->ci_nmax = nmax;
    ctx->ci_n = N;
    ctx->ci_c = C;
  }
  return SCDE_OK;
}

int scde_crossfit_reduce_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells,
                              const int* groups, const double* ls, const int* pairs, int npairs, const int* status,
                              const int8_t* clusters, const double* posterior, int min_nonfailed, uint8_t* vil,
                              double* fpm, double* fail_prior, int* nabove) {
  FORK_GUARD();
  RCHK(knn_check(counts, ld, ngenes, ncells, "crossfit_reduce"));
  const int* dev = nullptr;
  RCHK(stage_counts(ctx, counts, ld, ngenes, ncells, &dev));
  return scde_crossfit_reduce_dev(ctx, dev, ngenes, ngenes, ncells, groups, ls, pairs, npairs, status, clusters,
                                  posterior, min_nonfailed, vil, fpm, fail_prior, nabove);
}
}  // extern "C"
