// The per-cell mixture fit of scde.error.models with linear.fit = FALSE (fit.nb2.mixture.model,
// FLXMRnb2glm's fit, glm.nb.fit, custom.glm.fit, MASS::theta.ml; R/functions.R:3630-3651,
// 4002-4010, 4434-4547, 4549-4820), as DESIGN.md section 4.16 and include/scde_hip.h state it: a
// two-component EM per cell -- a Poisson(background_rate) failure component and a negative
// binomial whose log mean is linear in log fpm, mixed by a logistic prior in log fpm -- with, in
// the M-step, a Newton logistic fit and the alternation of an IRLS for the coefficients with a
// Newton for theta.
//
//   k_nb2_fit   one workgroup (kFitThreads) per cell, the whole EM inside the launch, laid out as
//               k_knn_fit (fit_common.h): the valid genes compacted in gene order into per-gene
//               vectors (log fpm, the linear predictor, p2, the IRLS weight, p1, count, gene
//               index), in LDS up to `cap` genes and in the workgroup's HBM workspace above it;
//               every sum by block_sum, so its order depends on the cell's gene count and on which
//               of its genes have weight 0 alone, and every thread holds the same bits; the 2 x 2
//               solves are the unrolled Cholesky every thread runs on those bits, so all control
//               flow is uniform over the workgroup.  No floating-point atomics: results repeat
//               bit for bit, whichever cells share the launch.
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

// ------------------------------------------------------------------ concomitant
__device__ double conc_objective2(const FitVecs& v, int n, const double (&b)[2], const FitShared& sh, int tid) {
  double s[1] = {0.0};
  for (int i = tid; i < n; i += kFitThreads) {
    const double p2 = v.w[i];
    const double eta = b[0] + b[1] * v.l[i];
    s[0] += p2 * log_sigmoid(eta) + (1.0 - p2) * log_sigmoid(-eta);
  }
  block_sum(s, sh, tid);
  return s[0];
}

// k_knn_fit's Newton on two parameters: from 0, a step halved while it lowers the objective by
// more than rounding.  false: the Hessian could not be factorised, or the stopping rule was not
// met within 50 steps.
__device__ bool concomitant2(const FitVecs& v, int n, double (&beta)[2], const FitShared& sh, int tid) {
  beta[0] = beta[1] = 0.0;
  double f = conc_objective2(v, n, beta, sh, tid);
  for (int step = 0; step < 50; ++step) {
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += kFitThreads) {
      const double l = v.l[i], p2 = v.w[i];
      const double eta = beta[0] + beta[1] * l;
      const double lsp = log_sigmoid(eta), lsn = log_sigmoid(-eta);
      const double r = p2 * exp(lsn) - (1.0 - p2) * exp(lsp), h = exp(lsp + lsn);
      s[0] += r;
      s[1] += l * r;
      s[2] += h;
      s[3] += l * h;
      s[4] += l * h * l;
    }
    block_sum(s, sh, tid);
    const double g[2] = {s[0], s[1]};
    const double H[2][2] = {{s[2], s[3]}, {s[3], s[4]}};
    double d[2];
    if (!chol_solve(H, g, d)) return false;
    if (!(isfinite(d[0]) && isfinite(d[1]))) return false;
    double t = 1.0, fb = 0.0;
    double bt[2];
    bool taken = false;
    for (int h = 0; h < 30; ++h) {
      bt[0] = beta[0] + t * d[0];
      bt[1] = beta[1] + t * d[1];
      fb = conc_objective2(v, n, bt, sh, tid);
      if (isfinite(fb) && fb >= f - 1e-10 * (fabs(f) + 1.0)) {
        taken = true;
        break;
      }
      t *= 0.5;
    }
    if (!taken) return false;
    const double mstep = fmax(fabs(t * d[0]), fabs(t * d[1]));
    beta[0] = bt[0];
    beta[1] = bt[1];
    f = fb;
    if (mstep / (1.0 + fmax(fabs(bt[0]), fabs(bt[1]))) < 1e-10) return true;
  }
  return false;  // (separable data: the maximiser lies at infinity)
}

struct Nb2Args {
  const int* counts;
  long long ld;
  int N, C;
  const double* fpm;  // N x C dense
  const double* fp;   // N x C dense, NaN outside the valid genes
  double bg, log_bg;  // background_rate and its log (the host's: fail.r)
  int max_iter;
  int cap;            // valid genes the LDS vectors hold
  char* ws;           // per workgroup: ws_cap genes of vectors (null: no cell exceeds cap)
  long long ws_cap;
  double* models;     // C x 12 column-major
  int* iters;
  double* llh;
  int* status;
  int* clusters;      // N x C or null
  double* post;       // N x C or null
};

__global__ __launch_bounds__(kFitThreads) void k_nb2_fit(const Nb2Args A) {
  extern __shared__ __attribute__((aligned(16))) char fit_lds[];
  FitShared sh;
  sh.red = reinterpret_cast<double*>(fit_lds);
  sh.hist = reinterpret_cast<unsigned*>(fit_lds + kFitHistOff);
  sh.wcnt = reinterpret_cast<int*>(fit_lds + kFitCntOff);
  const int tid = threadIdx.x;
  const int N = A.N;

  for (int cell = blockIdx.x; cell < A.C; cell += gridDim.x) {
    const double* fpm = A.fpm + (size_t)cell * N;
    const double* fp = A.fp + (size_t)cell * N;
    const int* cnt = A.counts + (long long)cell * A.ld;
    int* cl_out = A.clusters ? A.clusters + (size_t)cell * N : nullptr;
    double* po_out = A.post ? A.post + (size_t)cell * N : nullptr;

    // the cell's valid genes
    int mine = 0;
    for (int g = tid; g < N; g += kFitThreads) mine += isnan(fp[g]) ? 0 : 1;
    double nsum[1] = {(double)mine};
    block_sum(nsum, sh, tid);  // (exact: integers below 2^53)
    const int n = (int)nsum[0];
    const bool in_lds = n <= A.cap;
    int status = kOk, its = 0;
    double llh = NAN, theta = NAN;
    double beta[2] = {NAN, NAN}, coef[2] = {NAN, NAN};
    FitVecs v = fit_carve(in_lds ? fit_lds + kFitVecOff : A.ws + (size_t)blockIdx.x * fit_vec_bytes((size_t)A.ws_cap),
                          in_lds ? (size_t)A.cap : (size_t)A.ws_cap);
    if (!in_lds && (!A.ws || n > A.ws_cap)) status = kNoWorkspace;  // (the host sizes the workspace: not reached)

    if (status == kOk) {
      fit_compact(v, sh, N, fpm, fp, cnt, cl_out, po_out, tid);
      __syncthreads();
    }
    if (status == kOk && n < 3) status = kTooFew;
    if (status == kOk) {
      double llh_old = -INFINITY;
      for (int it = 1; it <= A.max_iter; ++it) {
        its = it;
        // ---- M-step
        if (!concomitant2(v, n, beta, sh, tid)) {
          status = kNotFinite;
          break;
        }
        __syncthreads();
        for (int i = tid; i < n; i += kFitThreads) v.la[i] = v.y[i] <= 1 ? v.w[i] / 1e6 : v.w[i];
        __syncthreads();
        status = glm_nb_fit(v, n, false, 0.0, 0.5, INFINITY, coef, theta, sh, tid);
        if (status != kOk) break;
        if (coef[1] < 0.0) {
          // R's "ugly hack to restrict to non-negative slopes": mean(y w) / sum(w), a mean where a
          // log mean belongs
          double s[2] = {0.0, 0.0};
          for (int i = tid; i < n; i += kFitThreads) {
            s[0] += (double)v.y[i] * v.la[i];
            s[1] += v.la[i];
          }
          block_sum(s, sh, tid);
          coef[0] = s[0] / (double)n / s[1];
          coef[1] = 0.0;
        }
        if (!(isfinite(coef[0]) && isfinite(coef[1]))) {
          status = kNotFinite;
          break;
        }
        // ---- E-step: the new posteriors into w (p2) and mw (p1)
        __syncthreads();
        double ls[1] = {0.0};
        for (int i = tid; i < n; i += kFitThreads) {
          const double l = v.l[i], y = (double)v.y[i];
          const double eta = beta[0] + beta[1] * l;
          const double mu = link_mu(coef[0] + coef[1] * l);
          const double a1 = log_sigmoid(-eta) + dpois_log(y, A.bg);
          const double a2 = log_sigmoid(eta) + dnbinom_log(y, theta, theta / (theta + mu));
          const double m = fmax(a1, a2);
          const double lse = m + log(exp(a1 - m) + exp(a2 - m));
          v.mw[i] = exp(a1 - lse);
          v.w[i] = exp(a2 - lse);
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
      if (status == kOk && theta == 0.5) {
        // the "underfit" refit (R/functions.R:3640-3648): theta sits on its lower bound
        __syncthreads();
        for (int i = tid; i < n; i += kFitThreads) v.la[i] = v.w[i] > v.mw[i] ? 1.0 : 0.0;
        __syncthreads();
        status = glm_nb_fit(v, n, true, 0.5, 0.0, 1e5, coef, theta, sh, tid);
        if (status == kOk && !(theta > 0.0)) status = kNotFinite;
      }
    }

    // ---- the cell's results
    __syncthreads();
    if (status != kTooFew && status != kNoWorkspace) {
      for (int i = tid; i < n; i += kFitThreads) {
        const int g = v.gi[i];
        const double p1 = v.mw[i], p2 = v.w[i];
        if (cl_out) cl_out[g] = status == kOk ? (p2 > p1 ? 2 : 1) : 0;
        if (po_out) po_out[g] = status == kOk ? p1 : NAN;
      }
    } else {
      for (int g = tid; g < N; g += kFitThreads) {
        if (cl_out) cl_out[g] = 0;
        if (po_out) po_out[g] = NAN;
      }
    }
    if (tid == 0) {
      const bool ok = status == kOk;
      const size_t C = (size_t)A.C;
      double* m = A.models + cell;
      m[0 * C] = ok ? beta[0] : NAN;
      m[1 * C] = ok ? beta[1] : NAN;
      m[2 * C] = ok ? A.log_bg : NAN;
      m[3 * C] = ok ? coef[0] : NAN;
      m[4 * C] = ok ? coef[1] : NAN;
      m[5 * C] = ok ? theta : NAN;
#pragma unroll
      for (int i = 6; i < 12; ++i) m[i * C] = NAN;
      A.iters[cell] = its;
      A.llh[cell] = ok ? llh : NAN;
      A.status[cell] = status;
    }
    __syncthreads();
  }
}

}  // namespace

hipError_t launch_nb2_fit(const int* counts, long long ld, int N, int C, const double* fpm, const double* fp,
                          double background_rate, double log_background_rate, int max_iter, int lds_genes, char* ws,
                          long long ws_cap, int grid, double* models, int* iters, double* llh, int* status,
                          int* clusters, double* post, hipStream_t st) {
  if (C <= 0) return hipSuccess;
  if (lds_genes < 0 || lds_genes > knn_fit_lds_genes_max() || grid < 1) return hipErrorInvalidValue;
  Nb2Args a;
  a.counts = counts;
  a.ld = ld;
  a.N = N;
  a.C = C;
  a.fpm = fpm;
  a.fp = fp;
  a.bg = background_rate;
  a.log_bg = log_background_rate;
  a.max_iter = max_iter;
  a.cap = lds_genes;
  a.ws = ws;
  a.ws_cap = ws_cap;
  a.models = models;
  a.iters = iters;
  a.llh = llh;
  a.status = status;
  a.clusters = clusters;
  a.post = post;
  const size_t lds = knn_fit_lds_bytes(lds_genes);
  hipError_t e = hipFuncSetAttribute((const void*)k_nb2_fit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_nb2_fit, dim3(std::min(grid, C)), dim3(kFitThreads), lds, st, a);
  return hipGetLastError();
}

hipError_t nb2_fit_resident_groups(int lds_genes, int* groups) {
  int dev = 0, cus = 0, per = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void*)k_nb2_fit, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)knn_fit_lds_bytes(lds_genes));
  if (e != hipSuccess) return e;
  e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, (const void*)k_nb2_fit, kFitThreads,
                                                   knn_fit_lds_bytes(lds_genes));
  if (e != hipSuccess) return e;
  *groups = std::max(1, per) * std::max(1, cus);
  return hipSuccess;
}

}  // namespace scde
