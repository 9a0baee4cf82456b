// nb2_solvers.h -- glm.nb.fit as scde_nb2_fit_*'s contract states it (custom.glm.fit's IRLS with the
// design [1, l] and the log link, MASS::theta.ml, the alternation of the two), for the EM kernels
// that fit a negative binomial driver inside one workgroup: k_nb2_fit (nb2_fit.hip) and
// k_crossfit_fit (crossfit_fit.hip).  The functions read a problem's rows through FitVecs: l the
// covariate, y the count, la the weight (rows of weight 0 take no part), x the linear predictor
// (scratch: written by every fit).  Every sum is fit_common.h's block_sum.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

#include "device_math.h"
#include "fit_common.h"

namespace scde {

namespace {

enum { kOk = 0, kTooFew = 1, kNoWeight = 2, kNotFinite = 3, kNoWorkspace = 4, kIrlsFailed = 5 };

// the log link's linkinv and mu.eta: pmax(exp(eta), .Machine$double.eps) (a NaN stays)
__device__ __forceinline__ double link_mu(double eta) {
  const double m = exp(eta);
  return m < DBL_EPSILON ? DBL_EPSILON : m;
}

// the family of one IRLS: Poisson, or MASS's negative.binomial(th)
struct Family {
  bool nb;
  double th;
};

__device__ __forceinline__ double dev_resid(double y, double mu, double wt, const Family& f) {
  double r;
  if (f.nb) r = y * log(fmax(1.0, y) / mu) - (y + f.th) * log((y + f.th) / (mu + f.th));
  else r = y > 0.0 ? y * log(y / mu) - (y - mu) : mu;
  return 2.0 * wt * r;
}

// the deviance over the genes of positive weight: at the per-gene linear predictor v.x
// (coef null) or at coef[0] + coef[1] l
__device__ double deviance(const FitVecs& v, int n, const double* coef, const Family& f, const FitShared& sh,
                           int tid) {
  double s[1] = {0.0};
  for (int i = tid; i < n; i += kFitThreads) {
    const double wt = v.la[i];
    if (!(wt > 0.0)) continue;
    const double eta = coef ? coef[0] + coef[1] * v.l[i] : v.x[i];
    s[0] += dev_resid((double)v.y[i], link_mu(eta), wt, f);
  }
  block_sum(s, sh, tid);
  return s[0];
}

// custom.glm.fit with the design [1, l] and the log link from the linear predictor in v.x, which
// holds coef[0] + coef[1] l afterwards.  kOk or kIrlsFailed.
__device__ int irls(const FitVecs& v, int n, const Family& f, int maxit, double (&coef)[2], const FitShared& sh,
                    int tid) {
  const double eps = 1e-8;
  double dev_old = deviance(v, n, nullptr, f, sh, tid);
  if (!isfinite(dev_old)) return kIrlsFailed;
  bool have_old = false, first = true;
  double coef_old[2] = {0.0, 0.0};
  for (int it = 0; it < maxit; ++it) {
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += kFitThreads) {
      const double wt = v.la[i];
      if (!(wt > 0.0)) continue;
      const double l = v.l[i], y = (double)v.y[i];
      const double eta = first ? v.x[i] : coef[0] + coef[1] * l;
      const double mu = link_mu(eta);
      const double var = f.nb ? mu + mu * mu / f.th : mu;
      const double W = wt * (mu * mu) / var;
      const double z = eta + (y - mu) / mu;
      const double Wl = W * l;
      s[0] += W;
      s[1] += Wl;
      s[2] += Wl * l;
      s[3] += W * z;
      s[4] += Wl * z;
    }
    block_sum(s, sh, tid);
    first = false;
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 5; ++k) fin = fin && isfinite(s[k]);
    if (!fin) return kIrlsFailed;
    const double A[2][2] = {{s[0], s[1]}, {s[1], s[2]}};
    const double g[2] = {s[3], s[4]};
    double start[2];
    if (!chol_solve(A, g, start) || !(isfinite(start[0]) && isfinite(start[1]))) return kIrlsFailed;
    double dev = deviance(v, n, start, f, sh, tid);
    if (!isfinite(dev)) {
      if (!have_old) return kIrlsFailed;
      int ii = 1;
      while (!isfinite(dev)) {
        if (ii > maxit) return kIrlsFailed;
        ++ii;
        start[0] = (start[0] + coef_old[0]) / 2.0;
        start[1] = (start[1] + coef_old[1]) / 2.0;
        dev = deviance(v, n, start, f, sh, tid);
      }
    }
    if (have_old && (dev - dev_old) / (0.1 + fabs(dev)) > 3.0 * eps) {
      int ii = 1;
      while ((dev - dev_old) / (0.1 + fabs(dev)) > 3.0 * eps) {
        if (ii > maxit) break;
        ++ii;
        start[0] = (start[0] + coef_old[0]) / 2.0;
        start[1] = (start[1] + coef_old[1]) / 2.0;
        dev = deviance(v, n, start, f, sh, tid);
      }
    }
    coef[0] = start[0];
    coef[1] = start[1];
    if (fabs(dev - dev_old) / (0.1 + fabs(dev)) < eps) break;
    dev_old = dev;
    coef_old[0] = start[0];
    coef_old[1] = start[1];
    have_old = true;
  }
  __syncthreads();
  for (int i = tid; i < n; i += kFitThreads) v.x[i] = coef[0] + coef[1] * v.l[i];
  __syncthreads();
  return kOk;
}

// MASS::theta.ml(y, mu, sum(w), w, limit = 20) at mu = linkinv(v.x); abs(t0)
__device__ double theta_ml(const FitVecs& v, int n, double sw, const FitShared& sh, int tid) {
  double s0[1] = {0.0};
  for (int i = tid; i < n; i += kFitThreads) {
    const double wt = v.la[i];
    if (!(wt > 0.0)) continue;
    const double t = (double)v.y[i] / link_mu(v.x[i]) - 1.0;
    s0[0] += wt * (t * t);
  }
  block_sum(s0, sh, tid);
  double t0 = sw / s0[0];
  double del = 1.0;
  const double stop = 1.220703125e-4;  // .Machine$double.eps^0.25 = 2^-13
  for (int it = 1; it < 20 && fabs(del) > stop; ++it) {
    t0 = fabs(t0);
    double s[2] = {0.0, 0.0};
    const double dg0 = digamma_pos(t0), tg0 = trigamma_pos(t0), lt0 = log(t0);
    for (int i = tid; i < n; i += kFitThreads) {
      const double wt = v.la[i];
      if (!(wt > 0.0)) continue;
      const double y = (double)v.y[i], mu = link_mu(v.x[i]);
      s[0] += wt * (digamma_pos(t0 + y) - dg0 + lt0 + 1.0 - log(t0 + mu) - (y + t0) / (mu + t0));
      const double mt = mu + t0;
      s[1] += wt * (-trigamma_pos(t0 + y) + tg0 - 1.0 / t0 + 2.0 / mt - (y + t0) / (mt * mt));
    }
    block_sum(s, sh, tid);
    del = s[0] / s[1];
    t0 += del;
  }
  return fabs(t0);
}

__device__ double nb_loglik(const FitVecs& v, int n, double th, const FitShared& sh, int tid) {
  double s[1] = {0.0};
  const double lgt = lgamma(th), tlt = th * log(th);
  for (int i = tid; i < n; i += kFitThreads) {
    const double wt = v.la[i];
    if (!(wt > 0.0)) continue;
    const double y = (double)v.y[i], mu = link_mu(v.x[i]);
    s[0] += wt * (lgamma(th + y) - lgt - lgamma(y + 1.0) + tlt + y * log(mu + (y == 0.0 ? 1.0 : 0.0)) -
                  (th + y) * log(th + mu));
  }
  block_sum(s, sh, tid);
  return s[0];
}

// glm.nb.fit on the genes of positive weight (v.la); the first fit is Poisson, or
// negative.binomial(init_theta) when has_init.  kOk, kNoWeight, kNotFinite or kIrlsFailed.
__device__ int glm_nb_fit(const FitVecs& v, int n, bool has_init, double init_theta, double lo, double hi,
                          double (&coef)[2], double& theta, const FitShared& sh, int tid) {
  double c[2] = {0.0, 0.0};
  for (int i = tid; i < n; i += kFitThreads) {
    const double wt = v.la[i];
    if (!(wt > 0.0)) continue;
    c[0] += 1.0;
    c[1] += wt;
  }
  block_sum(c, sh, tid);
  const int n_ok = (int)c[0];
  const double sw = c[1];
  if (n_ok < 1) return kNoWeight;
  __syncthreads();
  for (int i = tid; i < n; i += kFitThreads) {
    const double y = (double)v.y[i];
    v.x[i] = log(has_init ? y + (y == 0.0 ? 1.0 / 6.0 : 0.0) : y + 0.1);  // the families' mustart
  }
  __syncthreads();
  Family fam = {has_init, init_theta};
  int st = irls(v, n, fam, 20, coef, sh, tid);
  if (st != kOk) return st;
  double th = theta_ml(v, n, sw, sh, tid);
  if (!isfinite(th)) return kNotFinite;
  th = fmin(fmax(th, lo), hi);
  const double d1 = sqrt(2.0 * (double)max(1, n_ok - 2));
  double del = 1.0;
  double lm = nb_loglik(v, n, th, sh, tid);
  double lm0 = lm + 2.0 * d1;
  for (int it = 1; it <= 20 && fabs(lm0 - lm) / d1 + fabs(del) > 1e-8; ++it) {
    const double t0 = th;
    th = theta_ml(v, n, sw, sh, tid);  // (from the mu before this round's refit, as R)
    if (!isfinite(th)) return kNotFinite;
    th = fmin(fmax(th, lo), hi);
    fam.nb = true;
    fam.th = t0;
    st = irls(v, n, fam, 200, coef, sh, tid);
    if (st != kOk) return st;
    del = t0 - th;
    lm0 = lm;
    lm = nb_loglik(v, n, th, sh, tid);
  }
  if (!(isfinite(lm) && isfinite(coef[0]) && isfinite(coef[1]))) return kNotFinite;
  theta = th;
  return kOk;
}

}  // namespace

}  // namespace scde
