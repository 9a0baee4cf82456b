// api_stats.hip -- the host side of prior.hip and bh.hip, and the host-only statistics beside
// them: scde.expression.prior, BH-corrected Z scores, R's random number generator, bwpca's
// shuffles.  (engine.hip is the pipeline; a feature's host code lives in the api_ file named
// after its kernel files.)
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "engine_internal.h"
#include "kernels.h"

using namespace scde;
using namespace scde::host;

namespace {

// R pnorm upper tail (Cody, R nmath pnorm.c pnorm_both), x >= 0 path used by BH
double pnorm_upper(double x) {
  static const double a[5] = {2.2352520354606839287, 161.02823106855587881, 1067.6894854603709582,
                              18154.981253343561249, 0.065682337918207449113};
  static const double b[4] = {47.20258190468824187, 976.09855173777669322, 10260.932208618978205,
                              45507.789335026729956};
  static const double c[9] = {0.39894151208813466764, 8.8831497943883759412, 93.506656132177855979,
                              597.27027639480026226,  2494.5375852903726711, 6848.1904505362823326,
                              11602.651437647350124,  9842.7148383839780218, 1.0765576773720192317e-8};
  static const double d[8] = {22.266688044328115691, 235.38790178262499861, 1519.377599407554805,
                              6485.558298266760755,  18615.571640885098091, 34900.952721145977266,
                              38912.003286093271411, 19685.429676859990727};
  static const double pp[6] = {0.21589853405795699,     0.1274011611602473639, 0.022235277870649807,
                               0.001421619193227893466, 2.9112874951168792e-5, 0.02307344176494017303};
  static const double q[5] = {1.28426009614491121, 0.468238212480865118, 0.0659881378689285515,
                              0.00378239633202758244, 7.29751555083966205e-5};
  const double M_1_SQRT_2PI = 0.398942280401432677939946059934, M_SQRT_32 = 5.656854249492380195206754896838;
  if (std::isnan(x)) return x;
  const double y = std::fabs(x);
  double xnum, xden, temp, xsq, del, cum, ccum;
  if (y <= 0.67448975) {
    if (y > DBL_EPSILON * 0.5) {
      xsq = x * x;
      xnum = a[4] * xsq;
      xden = xsq;
      for (int i = 0; i < 3; ++i) {
        xnum = (xnum + a[i]) * xsq;
        xden = (xden + b[i]) * xsq;
      }
    } else {
      xnum = xden = 0.0;
    }
    temp = x * (xnum + a[3]) / (xden + b[3]);
    cum = 0.5 + temp;
    ccum = 0.5 - temp;
  } else if (y <= M_SQRT_32) {
    xnum = c[8] * y;
    xden = y;
    for (int i = 0; i < 7; ++i) {
      xnum = (xnum + c[i]) * y;
      xden = (xden + d[i]) * y;
    }
    temp = (xnum + c[7]) / (xden + d[7]);
    xsq = std::trunc(y * 16) / 16;
    del = (y - xsq) * (y + xsq);
    cum = std::exp(-xsq * xsq * 0.5) * std::exp(-del * 0.5) * temp;
    ccum = 1.0 - cum;
    if (x > 0.) std::swap(cum, ccum);
  } else if ((-37.5193 < x && x < 8.2924) || (-8.2924 < x && x < 37.5193)) {
    xsq = 1.0 / (x * x);
    xnum = pp[5] * xsq;
    xden = xsq;
    for (int i = 0; i < 4; ++i) {
      xnum = (xnum + pp[i]) * xsq;
      xden = (xden + q[i]) * xsq;
    }
    temp = xsq * (xnum + pp[4]) / (xden + q[4]);
    temp = (M_1_SQRT_2PI - temp) / y;
    xsq = std::trunc(x * 16) / 16;
    del = (x - xsq) * (x + xsq);
    cum = std::exp(-xsq * xsq * 0.5) * std::exp(-del * 0.5) * temp;
    ccum = 1.0 - cum;
    if (x > 0.) std::swap(cum, ccum);
  } else {
    if (x > 0) {
      cum = 1.;
      ccum = 0.;
    } else {
      cum = 0.;
      ccum = 1.;
    }
  }
  return ccum;
}

double qnorm_host(double p, bool lower_tail) {
  if (std::isnan(p)) return p;
  if (p < 0 || p > 1) return NAN;
  if (p == 0) return lower_tail ? -INFINITY : INFINITY;
  if (p == 1) return lower_tail ? INFINITY : -INFINITY;
  const double p_ = lower_tail ? p : (0.5 - p + 0.5);
  const double q = p_ - 0.5;
  double r, val;
  if (std::fabs(q) <= .425) {
    r = .180625 - q * q;
    return q *
           (((((((r * 2509.0809287301226727 + 33430.575583588128105) * r + 67265.770927008700853) * r +
                45921.953931549871457) * r + 13731.693765509461125) * r + 1971.5909503065514427) * r +
             133.14166789178437745) * r + 3.387132872796366608) /
           (((((((r * 5226.495278852545925 + 28729.085735721942674) * r + 39307.89580009271061) * r +
                21213.794301586595867) * r + 5394.1960214247511077) * r + 687.1870074920579083) * r +
             42.313330701600911252) * r + 1.);
  }
  if (q < 0)
    r = lower_tail ? p : (0.5 - p + 0.5);
  else
    r = lower_tail ? (0.5 - p + 0.5) : p;
  r = std::sqrt(-std::log(r));
  if (r <= 5.) {
    r += -1.6;
    val = (((((((r * 7.7454501427834140764e-4 + .0227238449892691845833) * r + .24178072517745061177) * r +
                1.27045825245236838258) * r + 3.64784832476320460504) * r + 5.7694972214606914055) * r +
             4.6303378461565452959) * r + 1.42343711074968357734) /
          (((((((r * 1.05075007164441684324e-9 + 5.475938084995344946e-4) * r + .0151986665636164571966) * r +
                .14810397642748007459) * r + .68976733498510000455) * r + 1.6763848301838038494) * r +
             2.05319162663775882187) * r + 1.);
  } else {
    r += -5.;
    val = (((((((r * 2.01033439929228813265e-7 + 2.71155556874348757815e-5) * r + .0012426609473880784386) * r +
                .026532189526576123093) * r + .29656057182850489123) * r + 1.7848265399172913358) * r +
             5.4637849111641143699) * r + 6.6579046435011037772) /
          (((((((r * 2.04426310338993978564e-15 + 1.4215117583164458887e-7) * r + 1.8463183175100546818e-5) * r +
                7.868691311456132591e-4) * r + .0148753612908506148525) * r + .13692988092273580531) * r +
             .59983220655588793769) * r + 1.);
  }
  if (q < 0.0) val = -val;
  return val;
}

}  // namespace

extern "C" {

// ------------------------------------------------------------------ expression prior, BH
// scde.expression.prior (R/functions.R:225-254) on device-resident counts (prior.hip).
int scde_expression_prior_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells,
                              const double* models, int square_logit_conc, int length_out, double pseudo_count,
                              double bw, double max_quantile, const double* max_value, double* x, double* y,
                              double* lp, double* grid_weight, double* max_value_out) {
  FORK_GUARD();
  if (!ctx || !counts_dev || !models || !x || !y) return fail(SCDE_EARG, "null argument");
  if (ngenes <= 0 || ncells <= 0 || ld < ngenes) return fail(SCDE_EARG, "bad dimensions");
  // density grid n <= 4096: k_prior_conv stages y and the 2n kernel values in LDS (96 KiB of 160)
  if (length_out < 1 || length_out > 2047) return fail(SCDE_EARG, "length.out must be in [1, 2047]");
  if (!(bw > 0)) return fail(SCDE_EARG, "bw must be positive");
  if (!max_value && !(max_quantile >= 0 && max_quantile <= 1)) return fail(SCDE_EARG, "'probs' outside [0,1]");
  if ((long long)ngenes * ncells > 0x7fffffffLL) return fail(SCDE_EARG, "ngenes x ncells too large");
  HCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int N = ngenes, C = ncells, L = length_out;
  // per-cell constants: corr.b, corr.a, conc.b, conc.a, conc.a2 (model columns 3, 4, 0, 1, 11)
  std::vector<double> cellp((size_t)5 * C);
  const int mcol[5] = {3, 4, 0, 1, 11};
  for (int j = 0; j < 5; ++j)
    for (int c = 0; c < C; ++c)
      cellp[(size_t)j * C + c] = (j == 4 && !square_logit_conc) ? 0.0 : models[(size_t)mcol[j] * C + c];
  RCHK(upload(ctx, ctx->pr_cell, cellp.data(), sizeof(double) * cellp.size()));
  const int nb = prior_blocks(N, C, 2048);
  HCHK(ctx->pr_part.ensure(sizeof(double) * 6 * nb));
  HCHK(ctx->pr_occ.ensure(sizeof(int) * 256 * (size_t)prior_items(N, C)));
  HCHK(ctx->pr_stats.ensure(sizeof(double) * 4));
  const long long NC = (long long)N * C;
  const bool need_sort = !max_value && max_quantile < 1.0;
  if (need_sort) HCHK(ctx->pr_v.ensure(sizeof(double) * NC));
  hipEvent_t ev = ctx->mark_begin(SLOT_PRIOR_STATS);
  HCHK(launch_prior_stats(counts_dev, ld, N, C, ctx->pr_cell.as<double>(), square_logit_conc,
                          need_sort ? ctx->pr_v.as<double>() : nullptr, ctx->pr_occ.as<int>(),
                          ctx->pr_part.as<double>(), nb,
                          ctx->pr_stats.as<double>(), st));
  ctx->mark_end(SLOT_PRIOR_STATS, ev);
  double stats[4];
  HCHK(hipMemcpyAsync(stats, ctx->pr_stats.p, sizeof(stats), hipMemcpyDeviceToHost, st));
  RCHK(ctx->sync());
  const double wsum = stats[0];
  const long long nfin = (long long)stats[3];
  // totMass = sum(weights[is.finite(x)]) / sum(weights), 1 when every x is finite
  const double tot_mass = nfin == NC ? 1.0 : stats[1] / stats[0];
  double mv;
  if (max_value) {
    mv = *max_value;
  } else if (nfin == 0) {
    return fail(SCDE_EARG, "no finite expression magnitudes for quantile()");
  } else if (!need_sort) {
    mv = stats[2];  // quantile(x, 1) = max
  } else {
    // quantile(x[x < Inf], p, type = 7): the finite values sort first
    size_t wb = 0;
    HCHK(launch_sort_doubles(nullptr, nullptr, NC, nullptr, &wb, st));
    HCHK(ctx->pr_sortw.ensure(wb));
    HCHK(ctx->pr_sorted.ensure(sizeof(double) * NC));
    HCHK(launch_sort_doubles(ctx->pr_v.as<double>(), ctx->pr_sorted.as<double>(), NC, ctx->pr_sortw.p, &wb, st));
    const double index = 1 + (double)std::max<long long>(nfin - 1, 0) * max_quantile;
    const long long lo = (long long)std::floor(index), hi = (long long)std::ceil(index);
    double xl = 0, xh = 0;
    HCHK(hipMemcpyAsync(&xl, ctx->pr_sorted.as<double>() + (lo - 1), sizeof(double), hipMemcpyDeviceToHost, st));
    HCHK(hipMemcpyAsync(&xh, ctx->pr_sorted.as<double>() + (hi - 1), sizeof(double), hipMemcpyDeviceToHost, st));
    RCHK(ctx->sync());
    mv = xl;
    if (index > lo && xh != xl) {
      const double h = index - lo;
      mv = (1 - h) * xl + h * xh;
    }
  }
  if (!(mv > 0) || !std::isfinite(mv)) return fail(SCDE_EARG, "max.value must be positive and finite");
  const int n = prior_grid_n(L);
  HCHK(ctx->pr_hist.ensure(sizeof(unsigned long long) * (size_t)n));
  HCHK(ctx->pr_work.ensure(sizeof(double) * 3 * (size_t)n));
  HCHK(ctx->pr_out.ensure(sizeof(double) * 4 * (size_t)(L + 1)));
  ev = ctx->mark_begin(SLOT_PRIOR_BIN);
  HCHK(launch_prior_bin(counts_dev, ld, N, C, ctx->pr_cell.as<double>(), square_logit_conc, ctx->pr_occ.as<int>(),
                        wsum, mv, bw, L, ctx->pr_hist.as<unsigned long long>(), nb, st));
  ctx->mark_end(SLOT_PRIOR_BIN, ev);
  ev = ctx->mark_begin(SLOT_PRIOR_TAIL);
  HCHK(launch_prior_tail(tot_mass, mv, bw, L, pseudo_count / (double)N, ctx->pr_hist.as<unsigned long long>(),
                         ctx->pr_work.as<double>(), ctx->pr_out.as<double>(), st));
  ctx->mark_end(SLOT_PRIOR_TAIL, ev);
  const size_t m = (size_t)L + 1;
  double* outs[4] = {x, y, lp, grid_weight};
  for (int k = 0; k < 4; ++k)
    if (outs[k])
      HCHK(hipMemcpyAsync(outs[k], ctx->pr_out.as<double>() + k * m, sizeof(double) * m, hipMemcpyDeviceToHost, st));
  if (max_value_out) *max_value_out = mv;
  return ctx->sync();
}

int scde_bh_cz_dev(scde_ctx* ctx, const double* z_dev, int64_t n, double* cz_dev) {
  FORK_GUARD();
  if (!ctx || n < 0 || (n > 0 && (!z_dev || !cz_dev))) return fail(SCDE_EARG, "bad arguments");
  if (n > 0x7fffffff) return fail(SCDE_EARG, "n too large");
  if (n == 0) return SCDE_OK;
  HCHK(hipSetDevice(ctx->device));
  size_t wb = 0;
  HCHK(launch_bh_cz(nullptr, (int)n, nullptr, nullptr, &wb, ctx->stream));
  HCHK(ctx->bhw.ensure(wb));
  HCHK(launch_bh_cz(z_dev, (int)n, cz_dev, ctx->bhw.p, &wb, ctx->stream));
  return ctx->sync();
}

int scde_bh_cz(const double* z, int64_t n, double* cz) {
  if (n < 0 || (n > 0 && (!z || !cz))) return fail(SCDE_EARG, "bad arguments");
  // p.adjust(p, "BH"): i <- n:1; o <- order(p, decreasing = TRUE); pmin(1, cummin(n/i * p[o]))[ro]
  // NA (NaN) p-values are dropped from the adjustment and stay NA, as in R.
  std::vector<double> p(n);
  std::vector<int64_t> o;
  o.reserve(n);
  for (int64_t i = 0; i < n; ++i) {
    p[i] = pnorm_upper(std::fabs(z[i]));
    if (!std::isnan(p[i])) o.push_back(i);
  }
  const int64_t lp = (int64_t)o.size();
  if (lp <= 1) {  // `if (n <= 1) return(p0)`: nothing to adjust
    for (int64_t i = 0; i < n; ++i) {
      const double s = (z[i] > 0) ? 1.0 : (z[i] < 0 ? -1.0 : (std::isnan(z[i]) ? NAN : 0.0));
      cz[i] = s * qnorm_host(p[i], false);
    }
    return SCDE_OK;
  }
  std::stable_sort(o.begin(), o.end(), [&](int64_t a, int64_t b) { return p[a] > p[b]; });
  std::vector<double> adj(n, NAN);
  double cm = INFINITY;
  for (int64_t r = 0; r < lp; ++r) {
    const double i = (double)(lp - r);
    const double v = ((double)lp / i) * p[o[r]];
    if (v < cm) cm = v;
    adj[o[r]] = cm < 1 ? cm : 1;
  }
  for (int64_t i = 0; i < n; ++i) {
    const double s = (z[i] > 0) ? 1.0 : (z[i] < 0 ? -1.0 : (std::isnan(z[i]) ? NAN : 0.0));
    cz[i] = s * qnorm_host(adj[i], false);
  }
  return SCDE_OK;
}


// ------------------------------------------------------------------ R's RNG, shuffles
// R's RNG (src/main/RNG.c) for the host mirror of the R glue: set.seed scrambling,
// Mersenne-Twister unif_rand (with fixup), R >= 3.6 rejection sample().
int scde_r_set_seed(uint32_t seed, uint32_t* state) {
  if (!state) return fail(SCDE_EARG, "null state");
  for (int j = 0; j < 50; ++j) seed = 69069u * seed + 1u;
  for (int j = 0; j < 625; ++j) {
    seed = 69069u * seed + 1u;
    state[j] = seed;
  }
  state[0] = 624;
  return SCDE_OK;
}

static uint32_t r_mt_word(uint32_t* st) {
  static const uint32_t mag01[2] = {0x0u, 0x9908b0dfu};
  uint32_t* mt = st + 1;
  int mti = (int)st[0];
  uint32_t y;
  if (mti >= 624) {
    int kk;
    for (kk = 0; kk < 624 - 397; ++kk) {
      y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu);
      mt[kk] = mt[kk + 397] ^ (y >> 1) ^ mag01[y & 1u];
    }
    for (; kk < 623; ++kk) {
      y = (mt[kk] & 0x80000000u) | (mt[kk + 1] & 0x7fffffffu);
      mt[kk] = mt[kk - 227] ^ (y >> 1) ^ mag01[y & 1u];
    }
    y = (mt[623] & 0x80000000u) | (mt[0] & 0x7fffffffu);
    mt[623] = mt[396] ^ (y >> 1) ^ mag01[y & 1u];
    mti = 0;
  }
  y = mt[mti++];
  y ^= (y >> 11);
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= (y >> 18);
  st[0] = (uint32_t)mti;
  return y;
}

static double r_mt_genrand(uint32_t* st) { return (double)r_mt_word(st) * 2.3283064365386963e-10; }

static double r_unif_rand(uint32_t* st) {
  const double i2_32m1 = 2.328306437080797e-10;
  const double x = r_mt_genrand(st);
  if (x <= 0.0) return 0.5 * i2_32m1;
  if ((1.0 - x) <= 0.0) return 1.0 - 0.5 * i2_32m1;
  return x;
}

int scde_r_unif_rand(uint32_t* state, int64_t n, double* out) {
  if (!state || (n > 0 && !out)) return fail(SCDE_EARG, "null argument");
  for (int64_t i = 0; i < n; ++i) out[i] = r_unif_rand(state);
  return SCDE_OK;
}

int scde_r_mt_words(uint32_t* state, int64_t n, uint32_t* out) {
  if (!state || (n > 0 && !out)) return fail(SCDE_EARG, "null argument");
  for (int64_t i = 0; i < n; ++i) out[i] = r_mt_word(state);
  return SCDE_OK;
}

// norm_rand(), INVERSION (src/nmath/snorm.c): two uniforms per normal, 2^27 the "BIG" there
int scde_r_norm_rand(uint32_t* state, int64_t n, double* out) {
  if (!state || (n > 0 && !out)) return fail(SCDE_EARG, "null argument");
  const double big = 134217728.0;
  for (int64_t i = 0; i < n; ++i) {
    double u = r_unif_rand(state);
    u = (double)(int)(big * u) + r_unif_rand(state);
    out[i] = qnorm_host(u / big, true);
  }
  return SCDE_OK;
}

int scde_r_sample(uint32_t* state, int n, int k, int* out) {
  if (!state || (k > 0 && !out)) return fail(SCDE_EARG, "null argument");
  if (k > n || k < 0) return fail(SCDE_EARG, "cannot take a sample larger than the population");
  std::vector<int> x(std::max(n, 1));
  for (int i = 0; i < n; ++i) x[i] = i;
  for (int i = 0; i < k; ++i) {
    double dv = 0;
    const double dn = (double)n;
    if (dn > 0) {
      const int bits = (int)std::ceil(std::log2(dn));
      do {
        int64_t v = 0;
        for (int b = 0; b <= bits; b += 16) v = 65536 * v + (int)std::floor(r_unif_rand(state) * 65536);
        dv = (double)(v & ((((int64_t)1) << bits) - 1));
      } while (dn <= dv);
    }
    const int j = (int)dv;
    out[i] = x[j] + 1;
    x[j] = x[--n];
  }
  return SCDE_OK;
}

// set_random_matrices (src/bwpca.cpp:41-57) over the platform rand() (srand(seed) first):
// ind = 0..n-1 per shuffle; per column libstdc++ std::random_shuffle (j = rand() % (i+1)).
int scde_shuffle_perms(unsigned int seed, int nshuffles, int d, int n, int* perms) {
  if (nshuffles > 0 && d > 0 && n > 0 && !perms) return fail(SCDE_EARG, "null perms");
  PlatformRand rng(seed, g_rand_kind);
  std::vector<int> ind(std::max(n, 1));
  for (int s = 0; s < nshuffles; ++s) {
    for (int i = 0; i < n; ++i) ind[i] = i;
    for (int c = 0; c < d; ++c) {
      for (int i = 1; i < n; ++i) {
        const int j = rng.next() % (i + 1);
        if (i != j) std::swap(ind[i], ind[j]);
      }
      std::memcpy(perms + ((int64_t)s * d + c) * n, ind.data(), sizeof(int) * n);
    }
  }
  return SCDE_OK;
}

}  // extern "C"
