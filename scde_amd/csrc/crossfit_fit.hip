// The mixture cross-fit of a pair of cells: scde.error.models with threshold.segmentation = FALSE
// (calculate.crossfit.models' flexmix call, R/functions.R:2993-3028), as DESIGN.md section 4.19 and
// include/scde_hip.h state it: a three-component EM over the genes either cell detected -- the
// first cell failed (Poisson(zero_lambda) on its count), both amplified (two negative binomial
// drivers, each cell's count on the log of the other's), the second cell failed -- mixed by a
// multinomial-logit prior in the mean log count.
//
//   k_crossfit_fit  one workgroup (kFitThreads) per pair, the whole EM inside the launch, laid
//                   out as k_nb2_fit: the pair's rows compacted in gene order into per-row vectors
//                   (log(c1 + 1), log(c2 + 1), the drivers' linear predictor and weight, the three
//                   posteriors, both counts, the gene index), in LDS up to `cap` rows and in the
//                   workgroup's HBM workspace above it; every sum by block_sum, so its order
//                   depends on the pair's row count and on which rows have weight 0 alone, and
//                   every thread holds the same bits; the 4 x 4 and 2 x 2 solves are the unrolled
//                   Cholesky every thread runs on those bits, so all control flow is uniform over
//                   the workgroup.  The drivers are nb2_solvers.h's glm_nb_fit, read through two
//                   views of the vectors.  No floating-point atomics: results repeat bit for bit,
//                   whichever pairs share the launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>

#include "device_math.h"
#include "fit_common.h"
#include "kernels.h"
#include "nb2_solvers.h"
#include "wave_ops.h"

namespace scde {

namespace {

// (0, 2, 3 and 5 are glm_nb_fit's own)
enum { kNoRows = 1, kLost = 6 };

constexpr size_t kCfRowBytes = 7 * 8 + 3 * 4;  // 68

struct CfVecs {
  double *l1, *l2, *x, *la, *p1, *p2, *p3;
  int *y1, *y2, *gi;
};

__device__ __forceinline__ CfVecs cf_carve(char* base, size_t cap) {
  CfVecs v;
  v.l1 = reinterpret_cast<double*>(base);
  v.l2 = v.l1 + cap;
  v.x = v.l2 + cap;
  v.la = v.x + cap;
  v.p1 = v.la + cap;
  v.p2 = v.p1 + cap;
  v.p3 = v.p2 + cap;
  v.y1 = reinterpret_cast<int*>(v.p3 + cap);
  v.y2 = v.y1 + cap;
  v.gi = v.y2 + cap;
  return v;
}

__host__ __device__ __forceinline__ size_t cf_vec_bytes(size_t cap) { return (cap * kCfRowBytes + 15) & ~(size_t)15; }

// a driver's view for nb2_solvers.h: the count y on the covariate l
__device__ __forceinline__ FitVecs cf_driver(const CfVecs& v, int* y, double* l) {
  FitVecs f;
  f.l = l;
  f.x = v.x;
  f.w = v.p2;
  f.la = v.la;
  f.mw = nullptr;
  f.y = y;
  f.gi = v.gi;
  return f;
}

// log pi of softmax(0, b0 + b1 x, b2 + b3 x) by a max-shifted log-sum-exp
__device__ __forceinline__ void log_pi3(const double (&b)[4], double x, double (&lp)[3]) {
  const double e2 = b[0] + b[1] * x, e3 = b[2] + b[3] * x;
  const double m = fmax(0.0, fmax(e2, e3));
  const double lse = m + log(exp(-m) + exp(e2 - m) + exp(e3 - m));
  lp[0] = -lse;
  lp[1] = e2 - lse;
  lp[2] = e3 - lse;
}

__device__ double conc_objective3(const CfVecs& v, int n, const double (&b)[4], const FitShared& sh, int tid) {
  double s[1] = {0.0};
  for (int i = tid; i < n; i += kFitThreads) {
    double lp[3];
    log_pi3(b, (v.l1[i] + v.l2[i]) / 2.0, lp);
    s[0] += v.p1[i] * lp[0] + v.p2[i] * lp[1] + v.p3[i] * lp[2];
  }
  block_sum(s, sh, tid);
  return s[0];
}

// concomitant2's Newton on the four multinomial-logit parameters (a2, b2, a3, b3): the gradient
// p_k - pi_k as p_k (sum of the other pi) - pi_k (sum of the other p) and the Hessian's pi_k (1 -
// pi_k) as pi_k (sum of the other pi), so nothing is formed as 1 - pi
__device__ bool concomitant3(const CfVecs& v, int n, double (&beta)[4], const FitShared& sh, int tid) {
  beta[0] = beta[1] = beta[2] = beta[3] = 0.0;
  double f = conc_objective3(v, n, beta, sh, tid);
  for (int step = 0; step < 50; ++step) {
    double s[13];
#pragma unroll
    for (int k = 0; k < 13; ++k) s[k] = 0.0;
    for (int i = tid; i < n; i += kFitThreads) {
      const double x = (v.l1[i] + v.l2[i]) / 2.0;
      const double p1 = v.p1[i], p2 = v.p2[i], p3 = v.p3[i];
      double lp[3];
      log_pi3(beta, x, lp);
      const double q1 = exp(lp[0]), q2 = exp(lp[1]), q3 = exp(lp[2]);
      const double g2 = p2 * (q1 + q3) - (p1 + p3) * q2;
      const double g3 = p3 * (q1 + q2) - (p1 + p2) * q3;
      const double h22 = q2 * (q1 + q3), h33 = q3 * (q1 + q2), h23 = -(q2 * q3);
      s[0] += g2;
      s[1] += x * g2;
      s[2] += g3;
      s[3] += x * g3;
      s[4] += h22;
      s[5] += x * h22;
      s[6] += x * h22 * x;
      s[7] += h23;
      s[8] += x * h23;
      s[9] += x * h23 * x;
      s[10] += h33;
      s[11] += x * h33;
      s[12] += x * h33 * x;
    }
    block_sum(s, sh, tid);
    const double g[4] = {s[0], s[1], s[2], s[3]};
    const double H[4][4] = {{s[4], s[5], s[7], s[8]},
                            {s[5], s[6], s[8], s[9]},
                            {s[7], s[8], s[10], s[11]},
                            {s[8], s[9], s[11], s[12]}};
    double d[4];
    if (!chol_solve(H, g, d)) return false;
    if (!(isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]) && isfinite(d[3]))) return false;
    double t = 1.0, fb = 0.0;
    double bt[4];
    bool taken = false;
    for (int h = 0; h < 30; ++h) {
#pragma unroll
      for (int k = 0; k < 4; ++k) bt[k] = beta[k] + t * d[k];
      fb = conc_objective3(v, n, bt, sh, tid);
      if (isfinite(fb) && fb >= f - 1e-10 * (fabs(f) + 1.0)) {
        taken = true;
        break;
      }
      t *= 0.5;
    }
    if (!taken) return false;
    double mstep = 0.0, mb = 0.0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      mstep = fmax(mstep, fabs(t * d[k]));
      mb = fmax(mb, fabs(bt[k]));
      beta[k] = bt[k];
    }
    f = fb;
    if (mstep / (1.0 + mb) < 1e-10) return true;
  }
  return false;  // (separable data: the maximiser lies at infinity)
}

// one NB driver of component 2: the weights, glm.nb.fit with theta in [0, 1e3], R's negative-slope rule
__device__ int fit_driver(const CfVecs& v, const FitVecs& d, int n, double (&coef)[2], double& theta,
                          const FitShared& sh, int tid) {
  __syncthreads();
  for (int i = tid; i < n; i += kFitThreads) v.la[i] = d.y[i] <= 1 ? v.p2[i] / 1e6 : v.p2[i];
  __syncthreads();
  const int st = glm_nb_fit(d, n, false, 0.0, 0.0, 1e3, coef, theta, sh, tid);
  if (st != kOk) return st;
  if (coef[1] < 0.0) {
    double s[2] = {0.0, 0.0};
    for (int i = tid; i < n; i += kFitThreads) {
      s[0] += (double)d.y[i] * v.la[i];
      s[1] += v.la[i];
    }
    block_sum(s, sh, tid);
    coef[0] = s[0] / (double)n / s[1];
    coef[1] = 0.0;
  }
  return isfinite(coef[0]) && isfinite(coef[1]) ? kOk : kNotFinite;
}

struct CfArgs {
  const int* counts;
  long long ld;
  int N, P;
  const int *first, *second;  // the pairs' cells
  int thr;
  double min_prior, zero_lambda;
  int max_iter;
  int cap;       // rows the LDS vectors hold
  char* ws;      // per workgroup: ws_cap rows of vectors (null: no pair can exceed cap)
  long long ws_cap;
  int* status;   // P
  int* iters;    // P or null
  double* llh;   // P or null
  double* params;  // P x 10 column-major or null
  signed char* clusters;  // P blocks of N, or null
  double* post;           // P blocks of 2 x N (component 1, then component 3), or null
};

__global__ __launch_bounds__(kFitThreads) void k_crossfit_fit(const CfArgs A) {
  extern __shared__ __attribute__((aligned(16))) char fit_lds[];
  FitShared sh;
  sh.red = reinterpret_cast<double*>(fit_lds);
  sh.hist = reinterpret_cast<unsigned*>(fit_lds + kFitHistOff);
  sh.wcnt = reinterpret_cast<int*>(fit_lds + kFitCntOff);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = A.N;

  for (int pair = blockIdx.x; pair < A.P; pair += gridDim.x) {
    const int* cnt1 = A.counts + (long long)A.first[pair] * A.ld;
    const int* cnt2 = A.counts + (long long)A.second[pair] * A.ld;
    signed char* cl_out = A.clusters ? A.clusters + (size_t)pair * N : nullptr;
    double* po1 = A.post ? A.post + (size_t)pair * 2 * N : nullptr;
    double* po3 = po1 ? po1 + N : nullptr;

    // the pair's rows
    int mine = 0;
    for (int g = tid; g < N; g += kFitThreads) mine += (long long)cnt1[g] + (long long)cnt2[g] > 0 ? 1 : 0;
    double nsum[1] = {(double)mine};
    block_sum(nsum, sh, tid);  // (exact: integers below 2^53)
    const int n = (int)nsum[0];
    const bool in_lds = n <= A.cap;
    int status = kOk, its = 0;
    double llh = NAN;
    double beta[4] = {NAN, NAN, NAN, NAN}, ca[2] = {NAN, NAN}, cb[2] = {NAN, NAN}, tha = NAN, thb = NAN;
    const CfVecs v = cf_carve(in_lds ? fit_lds + kFitVecOff : A.ws + (size_t)blockIdx.x * cf_vec_bytes((size_t)A.ws_cap),
                              in_lds ? (size_t)A.cap : (size_t)A.ws_cap);
    if (!in_lds && (!A.ws || n > A.ws_cap)) status = kNoWorkspace;  // (the host sizes the workspace: not reached)
    if (status == kOk && n < 1) status = kNoRows;

    if (status == kOk) {
      // the rows compacted in gene order, with their starting posteriors
      int base = 0;
      for (int g0 = 0; g0 < N; g0 += kFitThreads) {
        const int g = g0 + tid;
        const int c1 = g < N ? cnt1[g] : 0, c2 = g < N ? cnt2[g] : 0;
        const bool row = (long long)c1 + (long long)c2 > 0;
        const unsigned long long mask = __ballot(row);
        const int pre = __popcll(mask & ((1ULL << lane) - 1ULL));
        __syncthreads();
        if (lane == 0) sh.wcnt[wave] = __popcll(mask);
        __syncthreads();
        int off = base, total = 0;
#pragma unroll
        for (int w = 0; w < kFitWaves; ++w) {
          const int c = sh.wcnt[w];
          off += w < wave ? c : 0;
          total += c;
        }
        if (row) {
          const int i = off + pre;
          const bool lo1 = c1 <= A.thr, lo2 = c2 <= A.thr;
          v.l1[i] = log((double)c1 + 1.0);
          v.l2[i] = log((double)c2 + 1.0);
          v.p1[i] = lo1 ? (lo2 ? 0.5 : 1.0) : 0.0;
          v.p2[i] = (!lo1 && !lo2) ? 1.0 : 0.0;
          v.p3[i] = lo2 ? (lo1 ? 0.5 : 1.0) : 0.0;
          v.y1[i] = c1;
          v.y2[i] = c2;
          v.gi[i] = g;
        }
        base += total;
      }
      __syncthreads();
      const FitVecs da = cf_driver(v, v.y1, v.l2), db = cf_driver(v, v.y2, v.l1);
      double llh_old = -INFINITY;
      for (int it = 1; it <= A.max_iter; ++it) {
        its = it;
        // ---- the components' shares of the posteriors this round starts from
        double sp[3] = {0.0, 0.0, 0.0};
        for (int i = tid; i < n; i += kFitThreads) {
          sp[0] += v.p1[i];
          sp[1] += v.p2[i];
          sp[2] += v.p3[i];
        }
        block_sum(sp, sh, tid);
        if (!(sp[0] / (double)n >= A.min_prior) || !(sp[1] / (double)n >= A.min_prior) ||
            !(sp[2] / (double)n >= A.min_prior)) {
          status = kLost;
          break;
        }
        // ---- M-step
        if (!concomitant3(v, n, beta, sh, tid)) {
          status = kNotFinite;
          break;
        }
        status = fit_driver(v, da, n, ca, tha, sh, tid);
        if (status != kOk) break;
        status = fit_driver(v, db, n, cb, thb, sh, tid);
        if (status != kOk) break;
        // ---- E-step
        __syncthreads();
        double ls[1] = {0.0};
        for (int i = tid; i < n; i += kFitThreads) {
          const double l1 = v.l1[i], l2 = v.l2[i], y1 = (double)v.y1[i], y2 = (double)v.y2[i];
          double lp[3];
          log_pi3(beta, (l1 + l2) / 2.0, lp);
          const double mua = link_mu(ca[0] + ca[1] * l2), mub = link_mu(cb[0] + cb[1] * l1);
          const double a1 = lp[0] + dpois_log(y1, A.zero_lambda);
          const double a2 = lp[1] + dnbinom_log(y1, tha, tha / (tha + mua)) + dnbinom_log(y2, thb, thb / (thb + mub));
          const double a3 = lp[2] + dpois_log(y2, A.zero_lambda);
          const double m = fmax(a1, fmax(a2, a3));
          const double lse = m + log(exp(a1 - m) + exp(a2 - m) + exp(a3 - m));
          v.p1[i] = exp(a1 - lse);
          v.p2[i] = exp(a2 - lse);
          v.p3[i] = exp(a3 - lse);
          ls[0] += lse;
        }
        block_sum(ls, sh, tid);
        llh = ls[0];
        if (!isfinite(llh)) {
          status = kNotFinite;
          break;
        }
        if (fabs(llh - llh_old) / (fabs(llh) + 0.1) < 1e-6) break;
        llh_old = llh;
      }
    }

    // ---- the pair's results: every gene cleared, then the rows of a fitted pair
    __syncthreads();
    for (int g = tid; g < N; g += kFitThreads) {
      if (cl_out) cl_out[g] = 0;
      if (po1) {
        po1[g] = NAN;
        po3[g] = NAN;
      }
    }
    __syncthreads();
    if (status == kOk) {
      for (int i = tid; i < n; i += kFitThreads) {
        const int g = v.gi[i];
        const double p1 = v.p1[i], p2 = v.p2[i], p3 = v.p3[i];
        if (cl_out) {
          int k = 1;
          double top = p1;
          if (p2 > top) {
            k = 2;
            top = p2;
          }
          if (p3 > top) k = 3;
          cl_out[g] = (signed char)k;
        }
        if (po1) {
          po1[g] = p1;
          po3[g] = p3;
        }
      }
    }
    if (tid == 0) {
      const bool ok = status == kOk;
      A.status[pair] = status;
      if (A.iters) A.iters[pair] = its;
      if (A.llh) A.llh[pair] = ok ? llh : NAN;
      if (A.params) {
        const size_t P = (size_t)A.P;
        double* m = A.params + pair;
        const double r[10] = {beta[0], beta[1], beta[2], beta[3], ca[0], ca[1], tha, cb[0], cb[1], thb};
#pragma unroll
        for (int k = 0; k < 10; ++k) m[k * P] = ok ? r[k] : NAN;
      }
    }
    __syncthreads();
  }
}

}  // namespace

int crossfit_fit_lds_rows_max() { return (int)((160 * 1024 - kFitVecOff) / kCfRowBytes); }
size_t crossfit_fit_lds_bytes(int lds_rows) { return (size_t)kFitVecOff + cf_vec_bytes((size_t)lds_rows); }
size_t crossfit_fit_ws_bytes(long long ws_cap) { return cf_vec_bytes((size_t)ws_cap); }

hipError_t crossfit_fit_resident_groups(int lds_rows, int* groups) {
  int dev = 0, cus = 0, per = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void*)k_crossfit_fit, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)crossfit_fit_lds_bytes(lds_rows));
  if (e != hipSuccess) return e;
  e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, (const void*)k_crossfit_fit, kFitThreads,
                                                   crossfit_fit_lds_bytes(lds_rows));
  if (e != hipSuccess) return e;
  *groups = std::max(1, per) * std::max(1, cus);
  return hipSuccess;
}

hipError_t launch_crossfit_fit(const int* counts, long long ld, int N, int P, const int* first, const int* second,
                               int thr, double min_prior, double zero_lambda, int max_iter, int lds_rows, char* ws,
                               long long ws_cap, int grid, int* status, int* iters, double* llh, double* params,
                               signed char* clusters, double* post, hipStream_t st) {
  if (P <= 0) return hipSuccess;
  if (lds_rows < 0 || lds_rows > crossfit_fit_lds_rows_max() || grid < 1) return hipErrorInvalidValue;
  CfArgs a;
  a.counts = counts;
  a.ld = ld;
  a.N = N;
  a.P = P;
  a.first = first;
  a.second = second;
  a.thr = thr;
  a.min_prior = min_prior;
  a.zero_lambda = zero_lambda;
  a.max_iter = max_iter;
  a.cap = lds_rows;
  a.ws = ws;
  a.ws_cap = ws_cap;
  a.status = status;
  a.iters = iters;
  a.llh = llh;
  a.params = params;
  a.clusters = clusters;
  a.post = post;
  const size_t lds = crossfit_fit_lds_bytes(lds_rows);
  hipError_t e = hipFuncSetAttribute((const void*)k_crossfit_fit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_crossfit_fit, dim3(std::min(grid, P)), dim3(kFitThreads), lds, st, a);
  return hipGetLastError();
}

}  // namespace scde
