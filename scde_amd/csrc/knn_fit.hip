// The per-cell mixture fit of knn.error.models (fit.nb2gth.mixture.model and
// get.compressed.v1.model, R/functions.R:3653-3660, 4058-4187, 3422-3434), as DESIGN.md section
// 4.15 and include/scde_hip.h state it: a two-component EM per cell -- a Poisson(0.1) failure
// component and a negative binomial whose mean is a * fpm, mixed by a logistic prior in log fpm
// and its square -- with, in the M-step, a Newton logistic fit, the closed-form slope, the
// theta.md moment root and (local theta) a five-parameter curve fitted to log alpha by a
// projected Levenberg-Marquardt.
//
//   k_knn_fit   one workgroup (kFitThreads) per cell, the whole EM inside the launch; workgroups
//               stride over the cells when there are more cells than groups.  The cell's valid
//               genes (fail_prior not NaN) are compacted in gene order into per-gene vectors
//               (log fpm, fpm, posterior, log alpha, weight, count, gene index): in LDS when the
//               cell has at most `cap` valid genes, in the workgroup's HBM workspace otherwise
//               (the same code through generic pointers).  Every sum is taken by block_sum: each
//               thread adds its genes tid, tid + kFitThreads, ... in that order, the lanes are
//               combined by wave_sum's butterfly and the waves in wave order through LDS, so a
//               sum's order depends on the cell's gene count alone and every thread holds the
//               same bits.  The 3 x 3 and 5 x 5 solves are unrolled Cholesky factorisations every
//               thread runs on those bits; all control flow is therefore uniform over the
//               workgroup.  The two quantiles of the curve's start come from an exact radix
//               select (8 passes of 8 bits over the order-preserving integer image of the
//               doubles, a 256-bin histogram of integer LDS atomics).  No floating-point
//               atomics: results repeat bit for bit, whichever cells share the launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>

#include "device_math.h"
#include "fit_common.h"
#include "kernels.h"
#include "wave_ops.h"

namespace scde {

namespace {

constexpr double kLn10 = 2.302585092994045684017991454684;

// ------------------------------------------------------------------ concomitant
__device__ double conc_objective(const FitVecs& v, int n, const double (&b)[3], const FitShared& sh, int tid) {
  double s[1] = {0.0};
  for (int i = tid; i < n; i += kFitThreads) {
    const double l = v.l[i], p2 = v.w[i];
    const double eta = b[0] + b[1] * l + b[2] * (l * l);
    s[0] += p2 * log_sigmoid(eta) + (1.0 - p2) * log_sigmoid(-eta);
  }
  block_sum(s, sh, tid);
  return s[0];
}

// Newton from 0 on the concave objective; a step is halved while it lowers the objective by more
// than rounding.  false: the Hessian could not be factorised, or the stopping rule was not met
// within 50 steps.
__device__ bool concomitant(const FitVecs& v, int n, double (&beta)[3], const FitShared& sh, int tid) {
  beta[0] = beta[1] = beta[2] = 0.0;
  double f = conc_objective(v, n, beta, sh, tid);
  for (int step = 0; step < 50; ++step) {
    double s[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) s[k] = 0.0;
    for (int i = tid; i < n; i += kFitThreads) {
      const double l = v.l[i], p2 = v.w[i], l2 = l * l;
      const double eta = beta[0] + beta[1] * l + beta[2] * l2;
      // p2 - sigma and sigma (1 - sigma) without cancellation: saturated genes keep a smooth,
      // positive curvature (1 - sigma in floating point is 0 from eta = 37 on)
      const double lsp = log_sigmoid(eta), lsn = log_sigmoid(-eta);
      const double r = p2 * exp(lsn) - (1.0 - p2) * exp(lsp), h = exp(lsp + lsn);
      s[0] += r;
      s[1] += l * r;
      s[2] += l2 * r;
      s[3] += h;
      s[4] += l * h;
      s[5] += l2 * h;  // (1, l2) and (l, l)
      s[6] += l * h * l;
      s[7] += l * h * l2;
      s[8] += l2 * h * l2;
    }
    block_sum(s, sh, tid);
    const double g[3] = {s[0], s[1], s[2]};
    const double H[3][3] = {{s[3], s[4], s[5]}, {s[4], s[6], s[7]}, {s[5], s[7], s[8]}};
    double d[3];
    if (!chol_solve(H, g, d)) return false;
    if (!(isfinite(d[0]) && isfinite(d[1]) && isfinite(d[2]))) return false;
    double t = 1.0, fb = 0.0;
    double bt[3];
    bool taken = false;
    for (int h = 0; h < 30; ++h) {
#pragma unroll
      for (int k = 0; k < 3; ++k) bt[k] = beta[k] + t * d[k];
      fb = conc_objective(v, n, bt, sh, tid);
      if (isfinite(fb) && fb >= f - 1e-10 * (fabs(f) + 1.0)) {
        taken = true;
        break;
      }
      t *= 0.5;
    }
    if (!taken) return false;
    double mstep = 0.0, mbeta = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      mstep = fmax(mstep, fabs(t * d[k]));
      beta[k] = bt[k];
      mbeta = fmax(mbeta, fabs(bt[k]));
    }
    f = fb;
    if (mstep / (1.0 + mbeta) < 1e-10) return true;
  }
  return false;  // (separable data: the maximiser lies at infinity)
}

// ------------------------------------------------------------------ theta.md's moment equation
// left side minus right side, and the derivative, at th (mw holds y log(max(1, y) / mu))
__device__ void theta_sums(const FitVecs& v, int n, double a, double th, double target, double& g, double& d,
                           const FitShared& sh, int tid) {
  double s[2] = {0.0, 0.0};
  for (int i = tid; i < n; i += kFitThreads) {
    const double y = (double)v.y[i], mu = a * v.x[i], w2 = v.w[i] * 2.0;
    const double r = (y + th) / (mu + th);
    const double lr = log(r);
    s[0] += w2 * (v.mw[i] - (y + th) * lr);
    s[1] += w2 * (r - 1.0 - lr);
  }
  block_sum(s, sh, tid);
  g = s[0] - target;
  d = s[1];
}

__device__ double theta_root(const FitVecs& v, int n, double a, double sw, double lo, double hi, const FitShared& sh,
                             int tid) {
  const double target = sw - 1.0;
  double g_lo, g_hi, d;
  theta_sums(v, n, a, lo, target, g_lo, d, sh, tid);
  theta_sums(v, n, a, hi, target, g_hi, d, sh, tid);
  if (!(isfinite(g_lo) && isfinite(g_hi))) return NAN;
  if (g_lo >= 0.0) return lo;
  if (g_hi <= 0.0) return hi;
  double ba = lo, bb = hi, t = sqrt(lo * hi);
  for (int it = 0; it < 100; ++it) {
    double g;
    theta_sums(v, n, a, t, target, g, d, sh, tid);
    if (g == 0.0) break;
    if (g < 0.0) ba = t;
    else bb = t;
    double tn = t - g / d;
    if (!(tn > ba && tn < bb)) tn = sqrt(ba * bb);
    const bool done = fabs(tn - t) <= 1e-14 * t;
    t = tn;
    if (done) break;
  }
  return t;
}

// ------------------------------------------------------------------ the curve of log alpha
// f(l) = b + (t - b) P, P = (1 + 10^((m - l) s))^-r through the stable softplus
__device__ __forceinline__ double curve_value(const double (&p)[5], double l) {
  const double z = (p[2] - l) * p[3] * kLn10;
  const double sp = fmax(z, 0.0) + log1p(exp(-fabs(z)));
  return p[0] + (p[1] - p[0]) * exp(-p[4] * sp);
}

// objective, J'WJ (lower triangle, row by row) and J'We at p
__device__ void lm_eval(const FitVecs& v, int n, const double (&p)[5], double& f, double (&A)[5][5], double (&g)[5],
                        const FitShared& sh, int tid) {
  double s[21];
#pragma unroll
  for (int k = 0; k < 21; ++k) s[k] = 0.0;
  const double tb = p[1] - p[0];
  for (int i = tid; i < n; i += kFitThreads) {
    const double l = v.l[i], W = v.mw[i];
    const double z = (p[2] - l) * p[3] * kLn10;
    const double sp = fmax(z, 0.0) + log1p(exp(-fabs(z)));
    const double P = exp(-p[4] * sp);
    const double e = v.la[i] - (p[0] + tb * P);
    const double q = exp(z - sp);
    const double c = tb * (-p[4]) * P * q * kLn10;
    const double J[5] = {1.0 - P, P, c * p[3], c * (p[2] - l), tb * (-P * sp)};
    s[0] += W * e * e;
    int at = 1;
#pragma unroll
    for (int r = 0; r < 5; ++r) {
      const double jw = J[r] * W;
      s[16 + r] += jw * e;
#pragma unroll
      for (int c2 = 0; c2 <= r; ++c2) s[at++] += jw * J[c2];
    }
  }
  block_sum(s, sh, tid);
  f = s[0];
  int at = 1;
#pragma unroll
  for (int r = 0; r < 5; ++r) {
    g[r] = s[16 + r];
#pragma unroll
    for (int c2 = 0; c2 <= r; ++c2) {
      A[r][c2] = s[at];
      A[c2][r] = s[at++];
    }
  }
}

// order-preserving integer image of a double (ascending)
__device__ __forceinline__ unsigned long long order_key(double d) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(d);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}
__device__ __forceinline__ double order_value(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffULL) : ~k;
  return __longlong_as_double((long long)b);
}

// the k-th smallest (0-based) of la over the genes with (l < mid) == low: radix select
__device__ double select_kth(const FitVecs& v, int n, double mid, bool low, int k, const FitShared& sh, int tid) {
  unsigned long long prefix = 0ULL;
  for (int shift = 56; shift >= 0; shift -= 8) {
    __syncthreads();
    sh.hist[tid] = 0u;  // kFitThreads == 256 bins
    __syncthreads();
    for (int i = tid; i < n; i += kFitThreads) {
      if ((v.l[i] < mid) != low) continue;
      const unsigned long long key = order_key(v.la[i]);
      if (shift == 56 || (key >> (shift + 8)) == prefix) atomicAdd(&sh.hist[(unsigned)(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    int b = 0;
    unsigned cum = 0;
    for (; b < 255; ++b) {
      const unsigned c = sh.hist[b];
      if (cum + c > (unsigned)k) break;
      cum += c;
    }
    k -= (int)cum;
    prefix = (prefix << 8) | (unsigned long long)b;
  }
  return order_value(prefix);
}

// R's type-7 quantile of that subset (m genes, m >= 1)
__device__ double subset_quantile(const FitVecs& v, int n, double mid, bool low, int m, double p, const FitShared& sh,
                                  int tid) {
  const double h = (double)(m - 1) * p;
  const int lo = (int)floor(h);
  const int hi = min(lo + 1, m - 1);
  const double a = select_kth(v, n, mid, low, lo, sh, tid);
  const double b = hi == lo ? a : select_kth(v, n, mid, low, hi, sh, tid);
  return a + (h - (double)lo) * (b - a);
}

__device__ __forceinline__ double box_lo(int i) {
  return i == 0 ? -100.0 : i == 1 ? -10.0 : i == 2 ? -100.0 : i == 3 ? -100.0 : 0.1;
}
__device__ __forceinline__ double box_hi(int i) {
  return i == 0 ? 10.0 : i == 1 ? 100.0 : i == 2 ? 100.0 : i == 3 ? 0.0 : 20.0;
}

// Projected Levenberg-Marquardt in R's box from par (clipped by the caller).  false: the start or
// its objective is not finite.
__device__ bool lm_fit(const FitVecs& v, int n, double (&par)[5], const FitShared& sh, int tid) {
#pragma unroll
  for (int i = 0; i < 5; ++i)
    if (!isfinite(par[i])) return false;
  double f, A[5][5], g[5];
  lm_eval(v, n, par, f, A, g, sh, tid);
  if (!isfinite(f)) return false;
  double lam = 1e-3;
  for (int step = 0; step < 100; ++step) {
    bool hold[5], all_held = true;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      hold[i] = (par[i] <= box_lo(i) && g[i] < 0.0) || (par[i] >= box_hi(i) && g[i] > 0.0) || !(A[i][i] > 0.0);
      all_held = all_held && hold[i];
    }
    if (all_held) break;
    bool accepted = false;
    double ft = 0.0, At[5][5], gt[5], pt[5];
    for (int trial = 0; trial < 12; ++trial) {
      double M[5][5], gg[5], d[5];
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        gg[i] = hold[i] ? 0.0 : g[i];
#pragma unroll
        for (int j = 0; j < 5; ++j)
          M[i][j] = (hold[i] || hold[j]) ? (i == j ? 1.0 : 0.0) : (i == j ? A[i][i] * (1.0 + lam) : A[i][j]);
      }
      chol_solve(M, gg, d);  // (a failed factorisation leaves NaN in d: the trial is rejected below)
      bool fin = true;
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        pt[i] = fmin(fmax(par[i] + d[i], box_lo(i)), box_hi(i));
        fin = fin && isfinite(par[i] + d[i]);
      }
      if (fin) {
        lm_eval(v, n, pt, ft, At, gt, sh, tid);
        if (isfinite(ft) && ft < f) {
          accepted = true;
          lam /= 10.0;
          break;
        }
      }
      lam *= 10.0;
    }
    if (!accepted) break;
    const double dec = f - ft, f_old = f;
    f = ft;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
      par[i] = pt[i];
      g[i] = gt[i];
#pragma unroll
      for (int j = 0; j < 5; ++j) A[i][j] = At[i][j];
    }
    if (dec <= 1e-14 * f_old) break;
  }
  return true;
}

struct FitArgs {
  const int* counts;
  long long ld;
  int N, C;
  const double* fpm;  // N x C dense
  const double* fp;   // N x C dense, NaN outside the valid genes
  int local_theta;
  double theta_lo, theta_hi, awp;
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

__global__ __launch_bounds__(kFitThreads) void k_knn_fit(const FitArgs A) {
  extern __shared__ __attribute__((aligned(16))) char fit_lds[];
  FitShared sh;
  sh.red = reinterpret_cast<double*>(fit_lds);
  sh.hist = reinterpret_cast<unsigned*>(fit_lds + kFitHistOff);
  sh.wcnt = reinterpret_cast<int*>(fit_lds + kFitCntOff);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
    int status = 0, its = 0;
    double llh = NAN;
    double beta[3] = {NAN, NAN, NAN}, par[5] = {NAN, NAN, NAN, NAN, NAN}, a = NAN, theta = NAN;
    FitVecs v = fit_carve(in_lds ? fit_lds + kFitVecOff : A.ws + (size_t)blockIdx.x * fit_vec_bytes((size_t)A.ws_cap),
                          in_lds ? (size_t)A.cap : (size_t)A.ws_cap);
    if (!in_lds && (!A.ws || n > A.ws_cap)) status = 4;  // (the host sizes the workspace: not reached)

    if (status == 0) {
      fit_compact(v, sh, N, fpm, fp, cnt, cl_out, po_out, tid);
      __syncthreads();
    }

    if (status == 0 && n < 3) status = 1;
    if (status == 0) {
      // the range of l and the genes below its middle: the same in every round
      double mm[2] = {-INFINITY, -INFINITY};
      for (int i = tid; i < n; i += kFitThreads) {
        mm[0] = fmax(mm[0], v.l[i]);
        mm[1] = fmax(mm[1], -v.l[i]);
      }
      mm[0] = wave_max(mm[0]);
      mm[1] = wave_max(mm[1]);
      __syncthreads();
      if (lane == 0) {
        sh.red[wave * 2] = mm[0];
        sh.red[wave * 2 + 1] = mm[1];
      }
      __syncthreads();
      double lmax = sh.red[0], lmin = sh.red[1];
#pragma unroll
      for (int w = 1; w < kFitWaves; ++w) {
        lmax = fmax(lmax, sh.red[w * 2]);
        lmin = fmax(lmin, sh.red[w * 2 + 1]);
      }
      lmin = -lmin;
      const double mid = (lmin + lmax) / 2.0;
      double nl[1] = {0.0};
      for (int i = tid; i < n; i += kFitThreads) nl[0] += v.l[i] < mid ? 1.0 : 0.0;
      block_sum(nl, sh, tid);
      const int nlow = (int)nl[0];

      double llh_old = -INFINITY;
      for (int it = 1; it <= A.max_iter; ++it) {
        its = it;
        // ---- M-step
        if (!concomitant(v, n, beta, sh, tid)) {
          status = 3;
          break;
        }
        double s3[3] = {0.0, 0.0, 0.0};
        for (int i = tid; i < n; i += kFitThreads) {
          const double w = v.w[i];
          s3[0] += w * v.x[i];
          s3[1] += w * (double)v.y[i];
          s3[2] += w;
        }
        block_sum(s3, sh, tid);
        if (!(s3[0] > 0.0)) {
          status = 2;
          break;
        }
        a = s3[1] / s3[0];
        if (!(a > 0.0 && isfinite(a))) {
          status = 3;
          break;
        }
        for (int i = tid; i < n; i += kFitThreads) {
          const double y = (double)v.y[i], mu = a * v.x[i];
          v.mw[i] = y > 0.0 ? y * log(fmax(1.0, y) / mu) : 0.0;
        }
        __syncthreads();
        theta = theta_root(v, n, a, s3[2], A.theta_lo, A.theta_hi, sh, tid);
        if (A.local_theta) {
          __syncthreads();
          for (int i = tid; i < n; i += kFitThreads) {
            const double y = (double)v.y[i], mu = a * v.x[i];
            const double t = y / mu - 1.0;
            double al = t * t - 1.0 / mu;
            const double alo = 1.0 / A.theta_hi, ahi = 1.0 / A.theta_lo;
            al = al < alo ? alo : (al > ahi ? ahi : al);  // (a NaN stays: the cell fails)
            v.la[i] = log(al);
            v.mw[i] = v.w[i] * pow(al, A.awp);
          }
          __syncthreads();
          const double bot = nlow > 0 ? subset_quantile(v, n, mid, true, nlow, 0.025, sh, tid) : NAN;
          const double top = n - nlow > 0 ? subset_quantile(v, n, mid, false, n - nlow, 0.975, sh, tid) : NAN;
          par[0] = bot;
          par[1] = top;
          par[2] = mid;
          par[3] = -1.0;
          par[4] = 0.5;
#pragma unroll
          for (int i = 0; i < 5; ++i) par[i] = fmin(fmax(par[i], box_lo(i)), box_hi(i));  // (NaN stays NaN)
          if (isnan(bot)) par[0] = NAN;
          if (isnan(top)) par[1] = NAN;
          if (!lm_fit(v, n, par, sh, tid)) {
            status = 3;
            break;
          }
        }
        bool fin = isfinite(beta[0]) && isfinite(beta[1]) && isfinite(beta[2]) && isfinite(theta) &&
                   isfinite(log(a));
        if (A.local_theta) {
#pragma unroll
          for (int i = 0; i < 5; ++i) fin = fin && isfinite(par[i]);
        }
        if (!fin) {
          status = 3;
          break;
        }
        // ---- E-step: the new posteriors into w (p2) and mw (p1)
        __syncthreads();
        double ls[1] = {0.0};
        for (int i = tid; i < n; i += kFitThreads) {
          const double l = v.l[i], y = (double)v.y[i], mu = a * v.x[i];
          const double eta = beta[0] + beta[1] * l + beta[2] * (l * l);
          double th = theta;
          if (A.local_theta) {
            th = exp(-curve_value(par, l));
            th = fmin(fmax(th, A.theta_lo), A.theta_hi);  // (fmin / fmax drop a NaN: the lower bound)
            if (isnan(th)) th = A.theta_lo;
          }
          const double a1 = log_sigmoid(-eta) + dpois_log(y, 0.1);
          const double a2 = log_sigmoid(eta) + dnbinom_log(y, th, th / (th + mu));
          const double m = fmax(a1, a2);
          const double lse = m + log(exp(a1 - m) + exp(a2 - m));
          v.mw[i] = exp(a1 - lse);
          v.w[i] = exp(a2 - lse);
          ls[0] += lse;
        }
        block_sum(ls, sh, tid);
        llh = ls[0];
        if (!isfinite(llh)) {
          status = 3;
          break;
        }
        if (fabs(llh - llh_old) / (fabs(llh) + 0.1) < 1e-6) break;
        llh_old = llh;
      }
    }

    // ---- the cell's results
    __syncthreads();
    if (status == 0 || status == 2 || status == 3) {
      for (int i = tid; i < n; i += kFitThreads) {
        const int g = v.gi[i];
        const double p1 = v.mw[i], p2 = v.w[i];
        if (cl_out) cl_out[g] = status == 0 ? (p2 > p1 ? 2 : 1) : 0;
        if (po_out) po_out[g] = status == 0 ? p1 : NAN;
      }
    } else {
      for (int g = tid; g < N; g += kFitThreads) {
        if (cl_out) cl_out[g] = 0;
        if (po_out) po_out[g] = NAN;
      }
    }
    if (tid == 0) {
      const bool ok = status == 0;
      const size_t C = (size_t)A.C;
      double* m = A.models + cell;
      m[0 * C] = ok ? beta[0] : NAN;
      m[1 * C] = ok ? beta[1] : NAN;
      m[2 * C] = ok ? log(0.1) : NAN;
      m[3 * C] = ok ? log(a) : NAN;
      m[4 * C] = ok ? 1.0 : NAN;
      m[5 * C] = ok ? theta : NAN;
#pragma unroll
      for (int i = 0; i < 5; ++i) m[(6 + i) * C] = (ok && A.local_theta) ? par[i] : NAN;
      m[11 * C] = ok ? beta[2] : NAN;
      A.iters[cell] = its;
      A.llh[cell] = ok ? llh : NAN;
      A.status[cell] = status;
    }
    __syncthreads();
  }
}

}  // namespace

int knn_fit_lds_genes_max() { return (int)((160 * 1024 - kFitVecOff) / 48); }

hipError_t launch_knn_fit(const int* counts, long long ld, int N, int C, const double* fpm, const double* fp,
                          int local_theta, double theta_lo, double theta_hi, double awp, int max_iter, int lds_genes,
                          char* ws, long long ws_cap, int grid, double* models, int* iters, double* llh, int* status,
                          int* clusters, double* post, hipStream_t st) {
  if (C <= 0) return hipSuccess;
  if (lds_genes < 0 || lds_genes > knn_fit_lds_genes_max() || grid < 1) return hipErrorInvalidValue;
  FitArgs a;
  a.counts = counts;
  a.ld = ld;
  a.N = N;
  a.C = C;
  a.fpm = fpm;
  a.fp = fp;
  a.local_theta = local_theta;
  a.theta_lo = theta_lo;
  a.theta_hi = theta_hi;
  a.awp = awp;
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
  hipError_t e = hipFuncSetAttribute((const void*)k_knn_fit, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_knn_fit, dim3(std::min(grid, C)), dim3(kFitThreads), lds, st, a);
  return hipGetLastError();
}

size_t knn_fit_lds_bytes(int lds_genes) { return (size_t)kFitVecOff + (size_t)lds_genes * 48; }
size_t knn_fit_ws_bytes(long long ws_cap) { return (size_t)ws_cap * 48; }

hipError_t knn_fit_resident_groups(int lds_genes, int* groups) {
  int dev = 0, cus = 0, per = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  if (e != hipSuccess) return e;
  e = hipFuncSetAttribute((const void*)k_knn_fit, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)knn_fit_lds_bytes(lds_genes));
  if (e != hipSuccess) return e;
  e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, (const void*)k_knn_fit, kFitThreads,
                                                   knn_fit_lds_bytes(lds_genes));
  if (e != hipSuccess) return e;
  *groups = std::max(1, per) * std::max(1, cus);
  return hipSuccess;
}

}  // namespace scde
