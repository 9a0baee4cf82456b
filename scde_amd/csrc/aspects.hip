// aspects.hip -- PAGODA's aspect redundancy reduction for gfx950: the numerical pieces of
// pagoda.reduce.loading.redundancy / pagoda.reduce.redundancy (R/functions.R:2490-2526,
// 2559-2610) and their helpers pathway.pc.correlation.distance (5126-5164) and
// collapse.aspect.clusters (5166-5198).  All FP64.  The contract is include/scde_hip.h's.
//
//   k_t_renorm      one lane per pair i < j of the loading correlations: the Student-t
//                   renormalisation to a common number of degrees of freedom, in log space.
//                   With a = (n - 2) / 2 and a' = (target - 2) / 2 the lane matches either the
//                   tail F = I_{1 - r^2}(a, 1/2) (= 2 p) or, when that is above 1/2, the centre
//                   G = I_{r^2}(1/2, a) = 1 - F, whichever is the smaller and so keeps its
//                   relative accuracy as a logarithm.  log I_x(p, q) is the prefactor
//                   p log x + q log(1 - x) - log p - log B(p, q) plus the log of Lentz's continued
//                   fraction, evaluated on the side where it converges (x < (p + 1) / (p + q + 2));
//                   x and 1 - x are both carried as logarithms, so nothing underflows.  The
//                   inversion is a Newton iteration on log(1 - cr^2) (tail) or log(cr^2) (centre)
//                   inside a bracket that starts from the leading term of the series and falls
//                   back to bisection whenever a step leaves it.  No LDS, no barriers: iteration
//                   counts differ per lane.
//   k_unit_cols     the patterns centred and scaled to unit length (two passes per aspect)
//   k_aspect_dist   their Gram matrix -- the Pearson correlation -- on the FP64 matrix cores, one
//                   block per 32 x 32 tile of the lower triangle, with the epilogue fused: the
//                   combined loading x pattern distance (1 - sqrt((1 - pclc) (1 - (1 - cda))))^power,
//                   or 1 - cor / 1 - |cor|; mirrored on store
//   k_wdist         1 - c / 1 - |c| of matWCorr's lower triangle, mirrored
//   k_collapse      one workgroup per cluster of aspects: row variances, the weights, and for a
//                   cluster of several rows the first principal component with its scores: the
//                   Gram matrix of the centred block on the smaller side on the FP64 matrix cores,
//                   Householder tridiagonalisation and Sturm bisection as sigma1.hip's k_sigma1sq
//                   runs them (the Householder vectors are kept below the subdiagonal), inverse
//                   iteration on the tridiagonal matrix (LU with partial pivoting, one thread),
//                   the back-transformation through the Householder vectors, then scores,
//                   orientation, scale.  Every sum runs in an order that depends on the cluster
//                   alone: no atomics, nothing depends on the grid.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "kernels.h"
#include "wave_ops.h"

namespace scde {
namespace {

typedef double d4_t __attribute__((ext_vector_type(4)));

// pair q of the strict upper triangle in column order: q = j (j - 1) / 2 + i, i < j
__device__ __forceinline__ void upper_pair(long long q, int& i, int& j) {
  long long jj = (long long)((1.0 + sqrt(1.0 + 8.0 * (double)q)) * 0.5);
  while (jj * (jj - 1) / 2 > q) --jj;
  while ((jj + 1) * jj / 2 <= q) ++jj;
  j = (int)jj;
  i = (int)(q - jj * (jj - 1) / 2);
}

// ------------------------------------------------------------------ Student-t renormalisation
// log(Gamma(a + 1/2) / Gamma(a)), a > 0: the asymptotic series from a >= 16 (its first omitted
// term is below 3e-18 there), reached from a smaller a by Gamma's recurrence
__device__ double lgamma_half_ratio(double a) {
  double prod = 1.0;
  while (a < 16.0) {
    prod *= a / (a + 0.5);
    a += 1.0;
  }
  const double i1 = 1.0 / a, i2 = i1 * i1;
  const double s = i1 * (-1.0 / 8 + i2 * (1.0 / 192 + i2 * (-1.0 / 640 + i2 * (17.0 / 14336 + i2 * (-31.0 / 18432 +
                   i2 * (691.0 / 180224))))));
  return 0.5 * log(a) + s + log(prod);
}

// log B(a, 1/2) = log Gamma(1/2) - log(Gamma(a + 1/2) / Gamma(a))
__device__ __forceinline__ double lbeta_half(double a) { return 0.57236494292470008707 - lgamma_half_ratio(a); }

// Lentz's evaluation of the continued fraction of I_x(p, q) (converges quickly for
// x < (p + 1) / (p + q + 2)); 1 at x = 0
__device__ double beta_cf(double p, double q, double x) {
  const double tiny = 1e-300;
  const double qab = p + q, qap = p + 1.0, qam = p - 1.0;
  double c = 1.0, d = 1.0 - qab * x / qap;
  if (fabs(d) < tiny) d = tiny;
  d = 1.0 / d;
  double h = d;
  for (int m = 1; m <= 20000; ++m) {
    const double m2 = 2.0 * m;
    double aa = m * (q - m) * x / ((qam + m2) * (p + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    h *= d * c;
    aa = -(p + m) * (qab + m) * x / ((p + m2) * (qap + m2));
    d = 1.0 + aa * d;
    if (fabs(d) < tiny) d = tiny;
    c = 1.0 + aa / c;
    if (fabs(c) < tiny) c = tiny;
    d = 1.0 / d;
    const double del = d * c;
    h *= del;
    if (fabs(del - 1.0) <= 1.2e-16) break;
  }
  return h;
}

struct TailCentre {
  double lF, lG;  // log I_x(a, 1/2), log I_z(1/2, a) = log(1 - F)
  double lz, lx;  // log z, log x at the point of evaluation
};

// For z = r^2 and x = 1 - z, each given with its logarithm.  lb = log B(a, 1/2).
__device__ TailCentre log_tail_centre(double a, double lb, double lz, double z, double lx, double x) {
  TailCentre t;
  t.lz = lz;
  t.lx = lx;
  if (z < 1.5 / (a + 2.5)) {
    t.lG = fmin(0.5 * lz + a * lx + 0.69314718055994530942 - lb + log(beta_cf(0.5, a, z)), 0.0);
    t.lF = log1p(-exp(t.lG));
  } else {
    t.lF = fmin(a * lx + 0.5 * lz - log(a) - lb + log(beta_cf(a, 0.5, x)), 0.0);
    t.lG = log1p(-exp(t.lF));
  }
  return t;
}

// the same at u = log x (tail = true) or u = log z (tail = false), u < 0
__device__ __forceinline__ TailCentre eval_at(bool tail, double a, double lb, double u) {
  const double e = exp(u), c = -expm1(u);            // the variable and its complement
  const double lc = e < 0.5 ? log1p(-e) : log(c);
  return log_tail_centre(a, lb, tail ? lc : u, tail ? c : e, tail ? u : lc, tail ? e : c);
}

__device__ double t_renorm(double r, int n, double at, double lbt) {
  const double ar = fabs(r);
  if (n <= 2 || !(ar < 1.0) || ar == 0.0) return r;  // (NaN and |r| >= 1 included)
  const double a = 0.5 * (double)(n - 2);
  if (a == at) return r;  // the same degrees of freedom on both sides: the identity
  const double lb = lbeta_half(a);
  const double z = ar * ar;
  // far inside the centre G is sqrt(z) / (B(1/2, a) / 2) to the last bit, on both sides
  if (z * (fmax(a, at) + 1.0) < 1.3e-17) return r * exp(lbt - lb);
  const double x = (1.0 - ar) * (1.0 + ar);
  const TailCentre src = log_tail_centre(a, lb, 2.0 * log(ar), z, z < 0.5 ? log1p(-z) : log(x), x);
  const bool tail = src.lF <= -0.69314718055994530942;
  const double target = tail ? src.lF : src.lG;
  // the bracket: the leading term of either series bounds the root on one side
  double lo, hi;
  if (tail) {
    hi = fmin((target + log(at) + lbt) / at, -DBL_MIN);  // F >= x^a / (a B)
    lo = hi;
    double step = 1.0;
    for (int it = 0; it < 2000; ++it) {
      lo -= step;
      step *= 2.0;
      if (eval_at(true, at, lbt, lo).lF <= target) break;
    }
  } else {
    lo = fmin(2.0 * (target - 0.69314718055994530942 + lbt), -DBL_MIN);  // G <= sqrt(z) / (B / 2)
    hi = lo;
    double step = 1.0;
    for (int it = 0; it < 2000; ++it) {
      hi += step;
      step *= 2.0;
      if (hi >= 0.0) {
        hi = 0.0;
        break;
      }
      if (eval_at(false, at, lbt, hi).lG >= target) break;
    }
  }
  double u = tail ? hi : lo;
  for (int it = 0; it < 200; ++it) {
    const TailCentre t = eval_at(tail, at, lbt, u);
    const double h = tail ? t.lF : t.lG;
    if (h > target) hi = u;
    else if (h < target) lo = u;
    else break;
    // d log F / d log x = x^a (1 - x)^(-1/2) / (B F);  d log G / d log z = z^(1/2) (1 - z)^(a - 1) / (B G)
    const double ls = tail ? at * u - 0.5 * t.lz - lbt - t.lF : 0.5 * u + (at - 1.0) * t.lx - lbt - t.lG;
    double un = u - (h - target) * exp(-ls);
    if (!(un > lo && un < hi)) un = 0.5 * (lo + hi);
    if (!(un > lo && un < hi)) break;  // lo and hi are adjacent
    const bool done = fabs(un - u) <= 2.3e-16 * fabs(u);
    u = un;
    if (done) break;
  }
  const double cr = tail ? sqrt(-expm1(u)) : exp(0.5 * u);
  return copysign(cr, r);
}

__global__ __launch_bounds__(256) void k_t_renorm(const double* __restrict__ r, const int* __restrict__ cnt, int m,
                                                  long long npairs, double target_ndf, double* __restrict__ cr) {
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q < m) cr[q * (m + 1)] = r[q * (m + 1)];  // the diagonal keeps x$r's value
  if (q >= npairs) return;
  int i, j;
  upper_pair(q, i, j);
  const long long e = i + (long long)j * m;
  const double at = 0.5 * (target_ndf - 2.0);
  const double v = t_renorm(r[e], cnt[e], at, lbeta_half(at));
  cr[e] = v;
  cr[j + (long long)i * m] = v;
}

// ------------------------------------------------------------------ distances
// z = (x - mean) / sqrt(sum (x - mean)^2) per column of the k x n matrix (two passes, one wave
// per column): the Gram matrix of z is cor(x).  A column that holds one value throughout becomes
// NaN (cor() is NA there)
__global__ __launch_bounds__(256) void k_unit_cols(const double* __restrict__ x, int k, int n, double* __restrict__ z) {
  const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= n) return;
  const int lane = threadIdx.x & 63;
  const double* xc = x + (long long)c * k;
  double* zc = z + (long long)c * k;
  const double x0 = xc[0];
  int diff = 0;
  double s = 0.0;
  for (int i = lane; i < k; i += 64) {
    diff |= xc[i] != x0;
    s += xc[i];
  }
  diff = __any(diff);
  // (the butterflies written out: through wave_sum the compiler orders this kernel differently)
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  const double mean = s / (double)k;
  double q = 0.0;
  for (int i = lane; i < k; i += 64) {
    const double t = xc[i] - mean;
    q += t * t;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o);
  const double nrm = sqrt(q);
  for (int i = lane; i < k; i += 64) zc[i] = diff ? (xc[i] - mean) / nrm : NAN;
}

// c = z'z on the FP64 matrix cores (one block per 32 x 32 tile I >= J, one wave per 16 x 16
// sub-tile, chunks of 32 cells through LDS: the staging of sigma1.hip's Gram phase), then the
// epilogue, written to both triangles.  With cr: (1 - sqrt((1 - pclc) (1 - (1 - cda))))^power,
// pclc = max(0, 1 - |cr|), cda = |c| (ab) or max(c, 0); without: 1 - |c| (ab) or 1 - c.
__global__ __launch_bounds__(256) void k_aspect_dist(const double* __restrict__ Z, int ncells, int m,
                                                     const double* __restrict__ cr, int ab, double power,
                                                     double* __restrict__ d) {
  __shared__ double sx[64][34];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  // tile pair of this block: I >= J, block = I (I + 1) / 2 + J
  int I = (int)((sqrt(8.0 * (double)blockIdx.x + 1.0) - 1.0) * 0.5);
  while (I * (I + 1) / 2 > (int)blockIdx.x) --I;
  while ((I + 1) * (I + 2) / 2 <= (int)blockIdx.x) ++I;
  const int J = (int)blockIdx.x - I * (I + 1) / 2;
  const int r = lane & 15, k4 = lane >> 4;
  const int ra = (wv >> 1) * 16 + r, rb = 32 + (wv & 1) * 16 + r;
  d4_t acc = {0, 0, 0, 0};
  for (int k0 = 0; k0 < ncells; k0 += 32) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int e = tid + 256 * t;
      const int row = e / 32, kk = e % 32;  // lanes run along the cells, contiguous in memory
      const int gc = (row < 32 ? I * 32 : J * 32 - 32) + row;
      const int kq = k0 + kk;
      sx[row][kk] = (gc < m && kq < ncells) ? Z[(long long)gc * ncells + kq] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 32; kk += 4)
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sx[ra][kk + k4], sx[rb][kk + k4], acc, 0, 0, 0);
    __syncthreads();
  }
  const int j = J * 32 + (wv & 1) * 16 + r;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int i = I * 32 + (wv >> 1) * 16 + k4 + 4 * u;
    if (i >= m || j >= m || i < j) continue;  // i >= j is kept and mirrored
    double v = 0.0;
    if (i != j) {
      const double c = acc[u];
      if (!cr) {
        v = ab ? 1.0 - fabs(c) : 1.0 - c;
      } else {
        double cda = c;
        if (ab) cda = fabs(c);
        else if (c < 0.0) cda = 0.0;
        cda = 1.0 - cda;  // as.dist(1 - cda)
        double pclc = 1.0 - fabs(cr[i + (long long)j * m]);
        if (pclc < 0.0) pclc = 0.0;
        v = pow(1.0 - sqrt((1.0 - pclc) * (1.0 - cda)), power);
      }
    }
    d[i + (long long)j * m] = v;
    d[j + (long long)i * m] = v;
  }
}

// matWCorr's lower triangle into a distance, both triangles, zero diagonal
__global__ __launch_bounds__(256) void k_wdist(double* __restrict__ d, int m, int ab) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)m * m) return;
  const int i = (int)(e % m), j = (int)(e / m);
  if (i < j) return;
  if (i == j) {
    d[e] = 0.0;
    return;
  }
  const double c = d[e];
  const double v = ab ? 1.0 - fabs(c) : 1.0 - c;
  d[e] = v;
  d[j + (long long)i * m] = v;
}

// ------------------------------------------------------------------ collapse
constexpr int kCB = 256;                           // threads per cluster
constexpr int kCT = 32, kCK = 32, kCS = kCK + 2;   // Gram tile, chunk of the summed side, LDS row stride

__device__ __forceinline__ double block_sum(double v, double* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

__device__ __forceinline__ double block_max(double v, double* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// R's var of the C values at x (stride 1): two passes, every thread of the block gets it
__device__ __forceinline__ double block_var(const double* x, int C, double* red, double* mean_out) {
  double s = 0.0;
  for (int c = threadIdx.x; c < C; c += kCB) s += x[c];
  const double mean = block_sum(s, red) / (double)C;
  double q = 0.0;
  for (int c = threadIdx.x; c < C; c += kCB) {
    const double t = x[c] - mean;
    q += t * t;
  }
  q = block_sum(q, red);
  if (mean_out) *mean_out = mean;
  return q / (double)(C - 1);
}

__global__ __launch_bounds__(kCB) void k_collapse(const double* __restrict__ X, const double* __restrict__ W, int C,
                                                  int m, const long long* __restrict__ off,
                                                  const int* __restrict__ idx, const long long* __restrict__ ws_off,
                                                  double* ws, int scale, int pick_top, double* __restrict__ D,
                                                  double* __restrict__ Wo, int* __restrict__ top,
                                                  int* __restrict__ status, double* __restrict__ ocor) {
  __shared__ double sx[2 * kCT][kCS];
  __shared__ double red[4];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long o0 = off[p];
  const int k = (int)(off[p + 1] - o0);
  const int* __restrict__ ix = idx + o0;
  double* dcol = D + (long long)p * C;
  double* wcol = Wo + (long long)p * C;
  // no row index is used before all of them have been checked
  int bad = 0;
  for (int t = tid; t < k; t += kCB) bad |= (ix[t] < 0) | (ix[t] >= m);
  if (__syncthreads_or(bad)) {
    if (tid == 0) {
      status[p] = -1;
      top[p] = -1;
      ocor[p] = NAN;
    }
    return;
  }
  const bool pca = k > 1 && !pick_top;
  const bool by_row = k <= C;               // M'M (k x k), else MM' (C x C)
  const int n = pca ? (by_row ? k : C) : 0;  // order of the Gram matrix
  const long long nl = n;
  double* A = ws + ws_off[p];
  double* dg = A + nl * nl;
  double* e2 = dg + n;    // the off-diagonal, squared for the bisection
  double* ee = e2 + n;    // the off-diagonal as it is
  double* vv = ee + n;
  double* wwv = vv + n;
  double* tau = wwv + n;
  double* la = tau + n;   // LU of T - lambda I: diagonal, superdiagonal, multipliers, second superdiagonal
  double* lb = la + n;
  double* lc = lb + n;
  double* ld = lc + n;
  double* lp = ld + n;    // 1.0 where rows were exchanged
  double* y = lp + n;
  double* mean = y + n;   // per row of the cluster
  double* var = mean + k;
  double* v1 = var + k;
  double* av = v1 + k;    // the orientation statistic, per cell

  // ---- row means, variances (R's var), the top row
  for (int t = wv; t < k; t += kCB / 64) {
    const double* xr = X + (long long)ix[t] * C;
    double s = 0.0;
    for (int c = lane; c < C; c += 64) s += xr[c];
    const double mu = wave_sum(s) / (double)C;
    double q = 0.0;
    for (int c = lane; c < C; c += 64) {
      const double d = xr[c] - mu;
      q += d * d;
    }
    q = wave_sum(q);
    if (lane == 0) {
      mean[t] = mu;
      var[t] = q / (double)(C - 1);
    }
  }
  __syncthreads();
  int itop = 0;
  double vmax = var[0];
  for (int t = 1; t < k; ++t)
    if (var[t] > vmax) {  // the first maximum
      vmax = var[t];
      itop = t;
    }
  // ---- weights: colSums(dw[ii, ] * sd(row)) / sum
  double wsum = 0.0;
  for (int c = tid; c < C; c += kCB) {
    double s = 0.0;
    for (int t = 0; t < k; ++t) s += W[(long long)ix[t] * C + c] * sqrt(var[t]);
    wcol[c] = s;
    wsum += s;
  }
  wsum = block_sum(wsum, red);
  for (int c = tid; c < C; c += kCB) wcol[c] = wcol[c] / wsum;
  if (tid == 0) {
    top[p] = ix[itop];
    status[p] = 0;
    ocor[p] = NAN;
  }
  if (!pca) {
    const double* xr = X + (long long)ix[k == 1 ? 0 : itop] * C;
    for (int c = tid; c < C; c += kCB) dcol[c] = xr[c];
    return;
  }

  // ---- 1. Gram matrix of the centred block
  const long long K = by_row ? C : k;  // length of the summed side
  const int r = lane & 15, k4 = lane >> 4;
  const int ra = (wv >> 1) * 16 + r, rb = kCT + (wv & 1) * 16 + r;
  const int nt = (n + kCT - 1) / kCT;
  double gmax = 0.0;
  for (int I = 0; I < nt; ++I)
    for (int J = 0; J <= I; ++J) {
      d4_t acc = {0, 0, 0, 0};
      for (long long k0 = 0; k0 < K; k0 += kCK) {
#pragma unroll
        for (int t = 0; t < 2 * kCT * kCK / kCB; ++t) {
          const int e = tid + kCB * t;
          // lanes run along the side that is contiguous in memory: the cells
          const int row = by_row ? e / kCK : e % (2 * kCT);
          const int kk = by_row ? e % kCK : e / (2 * kCT);
          const int gr = (row < kCT ? I * kCT : J * kCT - kCT) + row;
          const long long kq = k0 + kk;
          double v = 0.0;
          if (gr < n && kq < K)
            v = by_row ? X[(long long)ix[gr] * C + kq] - mean[gr] : X[(long long)ix[kq] * C + gr] - mean[kq];
          sx[row][kk] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kCK; kk += 4)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sx[ra][kk + k4], sx[rb][kk + k4], acc, 0, 0, 0);
        __syncthreads();
      }
      const int j = J * kCT + (wv & 1) * 16 + r;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = I * kCT + (wv >> 1) * 16 + k4 + 4 * u;
        if (i >= n || j >= n || i < j) continue;  // i >= j is kept and mirrored
        const double g = acc[u];
        A[i + j * nl] = g;
        A[j + i * nl] = g;
        gmax = fmax(gmax, g != g ? INFINITY : fabs(g));
      }
    }
  gmax = block_max(gmax, red);  // (its barriers publish A)
  double sigma = 0.0;
  bool have_vec = false;
  if (!(gmax < INFINITY)) {
    // a non-finite pattern: NaN scores, and the orientation is reported as NaN
    for (int c = tid; c < C; c += kCB) dcol[c] = NAN;
    return;
  }
  if (gmax > 0.0 && n > 1) {
    int ex;
    (void)frexp(gmax, &ex);
    for (long long t = tid; t < nl * nl; t += kCB) A[t] = ldexp(A[t], -ex);
    __syncthreads();

    // ---- 2. tridiagonalisation; v_k stays in A[k + 2 .., k] (v_k[0] = 1), tau[k] beside it
    for (int kq = 0; kq < n - 2; ++kq) {
      const int mm = n - kq - 1;
      double* col = A + kq * nl + (kq + 1);
      double* A22 = A + (kq + 1) * nl + (kq + 1);
      const double x0 = col[0];
      double ss = 0.0;
      for (int i = 1 + tid; i < mm; i += kCB) ss += col[i] * col[i];
      ss = block_sum(ss, red);
      if (ss == 0.0) {
        if (tid == 0) {
          dg[kq] = A[kq + kq * nl];
          ee[kq] = x0;
          tau[kq] = 0.0;
        }
        continue;
      }
      const double beta = -copysign(sqrt(x0 * x0 + ss), x0);
      const double tk = (beta - x0) / beta;
      const double sc = 1.0 / (x0 - beta);
      for (int i = tid; i < mm; i += kCB) vv[i] = i == 0 ? 1.0 : col[i] * sc;
      __syncthreads();
      double pv = 0.0;
      for (int i = tid; i < mm; i += kCB) {
        double s = 0.0;
        for (int j = 0; j < mm; ++j) s = fma(A22[i + j * nl], vv[j], s);
        s *= tk;
        wwv[i] = s;
        pv = fma(s, vv[i], pv);
      }
      pv = block_sum(pv, red);
      const double alpha = -0.5 * tk * pv;
      for (int i = tid; i < mm; i += kCB) wwv[i] = wwv[i] + alpha * vv[i];
      __syncthreads();
      for (int j = wv; j < mm; j += kCB / 64) {
        const double vj = vv[j], wj = wwv[j];
        for (int i = lane; i < mm; i += 64) A22[i + j * nl] = A22[i + j * nl] - (vv[i] * wj + wwv[i] * vj);
      }
      for (int i = 1 + tid; i < mm; i += kCB) col[i] = vv[i];
      if (tid == 0) {
        dg[kq] = A[kq + kq * nl];
        ee[kq] = beta;
        tau[kq] = tk;
      }
      __syncthreads();
    }
    if (tid == 0) {
      dg[n - 2] = A[(n - 2) + (n - 2) * nl];
      ee[n - 2] = A[(n - 1) + (n - 2) * nl];
      dg[n - 1] = A[(n - 1) + (n - 1) * nl];
      ee[n - 1] = 0.0;
    }
    __syncthreads();

    // ---- 3. the largest eigenvalue (Gershgorin bracket, widened as dstebz widens it)
    double gu = -INFINITY, gl = -INFINITY, emax = 0.0;
    for (int i = tid; i < n; i += kCB) {
      const double rad = (i > 0 ? fabs(ee[i - 1]) : 0.0) + fabs(ee[i]);
      gu = fmax(gu, dg[i] + rad);
      gl = fmax(gl, -(dg[i] - rad));
      emax = fmax(emax, fabs(ee[i]));
      e2[i] = ee[i] * ee[i];
    }
    gu = block_max(gu, red);
    gl = -block_max(gl, red);
    emax = block_max(emax, red);
    const double pivmin = DBL_MIN * fmax(1.0, emax * emax);
    const double tnorm = fmax(fabs(gl), fabs(gu));
    const double slop = 2.1 * tnorm * (DBL_EPSILON * 0.5) * n + 2.1 * pivmin;
    double lo = gl - slop, hi = gu + slop;
    for (int pass = 0; pass < 4096 && nextafter(lo, INFINITY) < hi; ++pass) {
      const double width = hi - lo;
      const double x = lo + width * (tid == 0 ? 0.5 : (double)tid / (double)kCB);
      const bool inside = x > lo && x < hi;
      const bool all_below = inside && sturm_count(dg, e2, n, x, pivmin) == n;
      const double nhi = -block_max(inside && all_below ? -x : -hi, red);
      const double nlo = block_max(inside && !all_below ? x : lo, red);
      hi = nhi;
      lo = nlo;
    }
    const double lam = hi;
    sigma = sqrt(ldexp(fmax(lam, 0.0), ex));

    // ---- 4. its eigenvector: inverse iteration on T - lambda I (LU with partial pivoting)
    if (tid == 0) {
      const double eps3 = DBL_EPSILON * fmax(tnorm, DBL_MIN);
      for (int i = 0; i < n; ++i) {
        la[i] = dg[i] - lam;
        lb[i] = ee[i];
        lc[i] = ee[i];
        ld[i] = 0.0;
        lp[i] = 0.0;
        y[i] = 1.0;
      }
      for (int i = 0; i < n - 1; ++i) {
        if (fabs(la[i]) >= fabs(lc[i])) {
          if (la[i] == 0.0) la[i] = eps3;
          const double mult = lc[i] / la[i];
          lc[i] = mult;
          la[i + 1] = la[i + 1] - mult * lb[i];
        } else {
          const double mult = la[i] / lc[i];
          la[i] = lc[i];
          const double t = la[i + 1];
          la[i + 1] = lb[i] - mult * t;
          if (i < n - 2) {
            ld[i] = lb[i + 1];
            lb[i + 1] = -mult * ld[i];
          }
          lb[i] = t;
          lc[i] = mult;
          lp[i] = 1.0;
        }
      }
      for (int iter = 0; iter < 5; ++iter) {
        if (iter > 0)  // (the first right-hand side is taken as L times a vector of ones)
          for (int i = 0; i < n - 1; ++i) {
            if (lp[i] == 0.0) {
              y[i + 1] = y[i + 1] - lc[i] * y[i];
            } else {
              const double t = y[i];
              y[i] = y[i + 1];
              y[i + 1] = t - lc[i] * y[i];
            }
          }
        double ymax = 0.0;
        for (int i = n - 1; i >= 0; --i) {
          double t = y[i];
          if (i < n - 1) t -= lb[i] * y[i + 1];
          if (i < n - 2) t -= ld[i] * y[i + 2];
          double piv = la[i];
          if (fabs(piv) < eps3) piv = piv < 0.0 ? -eps3 : eps3;
          y[i] = t / piv;
          ymax = fmax(ymax, fabs(y[i]));
        }
        for (int i = 0; i < n; ++i) y[i] = y[i] / ymax;
      }
    }
    __syncthreads();

    // ---- 5. back through the Householder vectors: z = H_0 H_1 ... H_{n-3} y, then unit length
    for (int kq = n - 3; kq >= 0; --kq) {
      const double tk = tau[kq];
      if (tk == 0.0) continue;  // (uniform over the block)
      const int mm = n - kq - 1;
      const double* col = A + kq * nl + (kq + 1);
      double* yy = y + kq + 1;
      double s = 0.0;
      for (int i = tid; i < mm; i += kCB) s = fma(i == 0 ? 1.0 : col[i], yy[i], s);
      s = tk * block_sum(s, red);
      for (int i = tid; i < mm; i += kCB) yy[i] = yy[i] - s * (i == 0 ? 1.0 : col[i]);
      __syncthreads();
    }
    double nn = 0.0;
    for (int i = tid; i < n; i += kCB) nn += y[i] * y[i];
    nn = sqrt(block_sum(nn, red));
    for (int i = tid; i < n; i += kCB) y[i] = y[i] / nn;
    __syncthreads();
    have_vec = true;
  }

  // ---- scores xv = M v1 and the loadings v1
  if (!have_vec) {
    // a centred block of zeros (every row constant), or a single cell
    for (int c = tid; c < C; c += kCB) dcol[c] = 0.0;
    for (int t = tid; t < k; t += kCB) v1[t] = 0.0;
  } else if (by_row) {
    for (int t = tid; t < k; t += kCB) v1[t] = y[t];
    __syncthreads();
    for (int c = tid; c < C; c += kCB) {
      double s = 0.0;
      for (int t = 0; t < k; ++t) s = fma(X[(long long)ix[t] * C + c] - mean[t], v1[t], s);
      dcol[c] = s;
    }
  } else {
    // the cell-side eigenvector times sigma is the score vector; v1 = M' u / sigma
    for (int c = tid; c < C; c += kCB) dcol[c] = sigma * y[c];
    for (int t = wv; t < k; t += kCB / 64) {
      const double* xr = X + (long long)ix[t] * C;
      double s = 0.0;
      for (int c = lane; c < C; c += 64) s = fma(xr[c] - mean[t], y[c], s);
      s = wave_sum(s);
      if (lane == 0) v1[t] = s / sigma;
    }
  }
  __syncthreads();

  // ---- fallback rule, orientation, scale
  double ad = 0.0;
  for (int c = tid; c + 1 < C; c += kCB) ad += fabs(dcol[c + 1] - dcol[c]);
  ad = block_sum(ad, red);
  if (ad == 0.0) {
    if (tid == 0) status[p] = 1;
    return;
  }
  if (!(ad == ad)) return;  // NaN scores: the orientation stays NaN
  for (int c = tid; c < C; c += kCB) {
    double s = 0.0;
    for (int t = 0; t < k; ++t) s += X[(long long)ix[t] * C + c] * fabs(v1[t]);
    av[c] = s / (double)k;
  }
  __syncthreads();
  double mx, ma;
  const double vx = block_var(dcol, C, red, &mx);
  const double va = block_var(av, C, red, &ma);
  double cv = 0.0;
  for (int c = tid; c < C; c += kCB) cv += (dcol[c] - mx) * (av[c] - ma);
  cv = block_sum(cv, red) / (double)(C - 1);
  double cor = cv / (sqrt(vx) * sqrt(va));
  double f = 1.0;
  if (cor < 0.0) {
    f = -1.0;
    cor = -cor;
  }
  if (tid == 0) ocor[p] = cor;
  double sa = 0.0;
  for (int c = tid; c < C; c += kCB) {
    double v = f * dcol[c];
    if (scale) v = v * sqrt(vmax) / sqrt(vx);
    dcol[c] = v;
    sa += fabs(v);
  }
  sa = block_sum(sa, red);
  if (sa == 0.0 && tid == 0) status[p] = 1;
}

}  // namespace

hipError_t launch_t_renorm(const double* r, const int* cnt, int m, double target_ndf, double* cr, hipStream_t st) {
  if (m <= 0) return hipSuccess;
  const long long npairs = (long long)m * (m - 1) / 2;
  const long long nthr = npairs > m ? npairs : m;
  hipLaunchKernelGGL(k_t_renorm, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, r, cnt, m, npairs, target_ndf,
                     cr);
  return hipGetLastError();
}

hipError_t launch_aspect_dist(const double* x, int ncells, int m, double* z, const double* cr, int ab, double power,
                              double* d, hipStream_t st) {
  if (m <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_unit_cols, dim3((m + 3) / 4), dim3(256), 0, st, x, ncells, m, z);
  const int nt = (m + 31) / 32;
  hipLaunchKernelGGL(k_aspect_dist, dim3((unsigned)(nt * (nt + 1) / 2)), dim3(256), 0, st, z, ncells, m, cr, ab, power,
                     d);
  return hipGetLastError();
}

hipError_t launch_wdist(double* d, int m, int ab, hipStream_t st) {
  if (m <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_wdist, dim3((unsigned)(((long long)m * m + 255) / 256)), dim3(256), 0, st, d, m, ab);
  return hipGetLastError();
}

size_t collapse_ws_doubles(long long k, int ncells, int pick_top) {
  const size_t n = (k > 1 && !pick_top) ? (size_t)(k < ncells ? k : ncells) : 0;
  return (n * n + 12 * n + 3 * (size_t)k + (size_t)ncells + 31) / 32 * 32;
}

hipError_t launch_collapse(const double* x, const double* w, int ncells, int m, int nclust, const long long* off,
                           const int* idx, const long long* ws_off, double* ws, int scale, int pick_top, double* d,
                           double* wo, int* top, int* status, double* ocor, hipStream_t st) {
  if (nclust <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_collapse, dim3(nclust), dim3(kCB), 0, st, x, w, ncells, m, off, idx, ws_off, ws, scale,
                     pick_top, d, wo, top, status, ocor);
  return hipGetLastError();
}

}  // namespace scde
