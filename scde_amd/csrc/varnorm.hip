// pagoda.varnorm after its weights (R/functions.R:1511-1619 and 1725-1804) and
// pagoda.subtract.aspect (1850-1862).
//
//   k_varnorm_moments   per gene: the effective degrees of freedom, the weighted NB variance
//                       (and their batch versions), rowSums(matw)
//   k_varnorm_matrix    per gene: the milder weights, the log10 magnitudes, their observed
//                       weighted variance, the batch adjustment of zeros and level means, and
//                       the centred matrix scaled by sqrt(arv / observed variance)
//   k_subtract_aspect   per gene: the weighted projection on a cell pattern removed, re-centred
//
// Layout: every N x C matrix is column-major with the gene contiguous (counts with leading
// dimension ld, the double matrices with N).  A wave takes 64 consecutive genes, one per lane,
// so every load and store of a wave is one contiguous 256- or 512-byte row segment, and a sum
// over a gene's cells is a loop over columns in one lane: no cross-lane step.  A workgroup is
// kVnWaves waves on the same 64 genes; wave w takes every kVnWaves-th cell (of a batch level,
// where the sums are per level) and the waves' partial sums are added through LDS in wave
// order, so a result depends on nothing but the shapes: no atomics, the same bits every run.
// The cell of a wave is uniform, so its model row and batch level are scalar loads.
//
// Nothing N x C is staged: each pass recomputes its per-element values from the counts (an
// int32 read), the gene's modes and the cell's model row; the only double matrices read are
// the weights and the only ones written are mat and matw.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "kernels.h"

namespace scde {

namespace {

constexpr int kVnWaves = 8;  // 512 threads: two waves per SIMD, the whole VGPR file for the FP64 pow / exp / log bodies

__device__ inline int vn_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

// The waves' values of one gene (lane) added in wave order; every wave gets the sum.
__device__ inline double vn_block_sum(double v, double (*red)[64], int w, int lane) {
  red[w][lane] = v;
  __syncthreads();
  double s = red[0][lane];
  for (int k = 1; k < kVnWaves; ++k) s += red[k][lane];
  __syncthreads();
  return s;
}

// get.corr.theta (R/functions.R:4039-4056) for the cell whose model row is (m[j * mld])
__device__ inline double vn_theta(const double* __restrict__ m, long long mld, int local_theta, double lfpm, double lo,
                                  double hi) {
  double th;
  if (local_theta) {
    const double ltb = m[6 * mld], ltt = m[7 * mld], ltm = m[8 * mld], lts = m[9 * mld], ltr = m[10 * mld];
    const double t = pow(1.0 + pow(10.0, (ltm - lfpm) * lts), ltr);
    th = exp(-1.0 * (ltb + (ltt - ltb) / t));
  } else {
    th = m[5 * mld];
  }
  if (th < lo) th = lo;
  if (th > hi) th = hi;
  if (isnan(th)) th = lo;
  return th;
}

// edf(theta) = exp(S(log theta)), S the natural cubic spline through the uniform table
// (values y, second derivatives m2; linear beyond the ends), 1 where theta > 1e3 (1524-1525)
__device__ inline double vn_edf(double theta, const VnEdf& e) {
  if (theta > 1e3) return 1.0;
  const double x = log(theta);
  const double t = (x - e.lt0) / e.h;
  const int n = e.n;
  double s;
  if (!(t >= 0.0)) {
    const double d0 = (e.y[1] - e.y[0]) / e.h - e.h * (2.0 * e.m2[0] + e.m2[1]) / 6.0;
    s = e.y[0] + d0 * (x - e.lt0);
  } else if (t > (double)(n - 1)) {
    const double dn = (e.y[n - 1] - e.y[n - 2]) / e.h + e.h * (2.0 * e.m2[n - 1] + e.m2[n - 2]) / 6.0;
    s = e.y[n - 1] + dn * (x - (e.lt0 + (double)(n - 1) * e.h));
  } else {
    int i = (int)t;  // 0 <= t <= n - 1
    if (i > n - 2) i = n - 2;
    const double b = t - (double)i, a = 1.0 - b;
    s = a * e.y[i] + b * e.y[i + 1] + ((a * a * a - a) * e.m2[i] + (b * b * b - b) * e.m2[i + 1]) * (e.h * e.h / 6.0);
  }
  return exp(s);
}

__device__ inline double vn_pow(double x, double p) { return p == 1.0 ? x : pow(x, p); }

// log10(exp(scde.expression.magnitude) + 1) (1729; magnitude = (log(count) - corr.b) / corr.a)
__device__ inline double vn_x(int count, double corr_a, double corr_b) {
  return log10(exp((log((double)count) - corr_b) / corr_a) + 1.0);
}

// Wilson score upper bound as pagoda.varnorm writes it (1720-1723), z = qnorm(1 - 1e-2)
__device__ inline double vn_wsu(double k, double n) {
  const double z = 2.3263478740408408;
  const double p = k / n;
  const double v =
      (2.0 * n * p + z * z + (z * sqrt(z * z - 1.0 / n + 4.0 * n * p * (1.0 - p) - (4.0 * p - 2.0)) + 1.0)) /
      (2.0 * (n + z * z));
  return v < 1.0 ? v : 1.0;
}

}  // namespace

// out: 7 x N (3 x N without a batch): edf, wvar, rowSums(matw), then bedf, bwvar, rowSums(bmatw),
// bwvar / wvar.  modes: the dataset-wide vector, then one per level.
__global__ __launch_bounds__(kVnWaves * 64) void k_varnorm_moments(
    const int* __restrict__ counts, long long ld, int N, int C, const double* __restrict__ models, int local_theta,
    const double* __restrict__ modes, const double* __restrict__ matw, const double* __restrict__ bmatw,
    const int* __restrict__ codes, VnEdf edf, double th_lo, double th_hi, double power, double* __restrict__ out) {
  __shared__ double red[6][kVnWaves][64];
  const int lane = threadIdx.x & 63, w = vn_wave();
  const int g = blockIdx.x * 64 + lane;
  const int gg = g < N ? g : N - 1;  // lanes past the last gene repeat it and write nothing
  const bool batched = bmatw != nullptr;
  const double lfpm = log(modes[gg]);
  double s[6] = {0, 0, 0, 0, 0, 0};
  for (int c = w; c < C; c += kVnWaves) {
    const double* m = models + c;
    const double corr_b = m[3LL * C], corr_a = m[4LL * C], lambda = exp(m[2LL * C]);
    const double cnt = (double)counts[(long long)c * ld + gg];
    const double mw = matw[(long long)c * N + gg];
    const double mu = exp(lfpm * corr_a + corr_b);
    const double th = vn_theta(m, C, local_theta, lfpm, th_lo, th_hi);
    const double e = vn_pow(mw * vn_edf(th, edf), power);
    const double d = cnt - mu;
    s[0] += e;
    s[1] += e * (d * d) / (mu + mu * mu / th + lambda);
    s[2] += mw;
    if (batched) {
      const double lb = log(modes[(long long)(1 + codes[c]) * N + gg]);
      const double bw = bmatw[(long long)c * N + gg];
      const double mub = exp(lb * corr_a + corr_b);
      const double thb = vn_theta(m, C, local_theta, lb, th_lo, th_hi);
      const double db = cnt - mub;
      s[3] += vn_pow(bw * vn_edf(thb, edf), power);
      s[4] += e * (db * db) / (mub + mub * mub / thb + lambda);  // the dataset-wide edf.mat, as line 1601 reads
      s[5] += bw;
    }
  }
  const int nq = batched ? 6 : 3;
  for (int q = 0; q < nq; ++q) red[q][w][lane] = s[q];
  __syncthreads();
  if (w != 0 || g >= N) return;
  for (int q = 0; q < nq; ++q) {
    double t = red[q][0][lane];
    for (int k = 1; k < kVnWaves; ++k) t += red[q][k][lane];
    s[q] = t;
  }
  const double wvar = s[1] / s[0];
  out[g] = s[0] + 1.0;
  out[(long long)N + g] = wvar;
  out[2LL * N + g] = s[2];
  if (batched) {
    const double bwvar = s[4] / s[3];
    out[3LL * N + g] = s[3] + 1.0;
    out[4LL * N + g] = bwvar;
    out[5LL * N + g] = s[5];
    out[6LL * N + g] = bwvar / wvar;
  }
}

// order: the cells grouped by level (lev_off[nlev + 1]; one level holding every cell without a
// batch); wsrc: matw, or bmatw with a batch; ws: 3 x nlev x N doubles of scratch (a gene's
// entries are written by wave 0 and read by its own workgroup only).
__global__ __launch_bounds__(kVnWaves * 64) void k_varnorm_matrix(
    const int* __restrict__ counts, long long ld, int N, int C, const double* __restrict__ models,
    const int* __restrict__ order, const int* __restrict__ lev_off, int nlev, int batched,
    const double* __restrict__ wsrc, double weight_k, const double* __restrict__ arv, double* __restrict__ ws,
    double* __restrict__ mat, double* __restrict__ matw_out) {
  __shared__ double red[kVnWaves][64];
  const int lane = threadIdx.x & 63, w = vn_wave();
  const int g = blockIdx.x * 64 + lane;
  const int gg = g < N ? g : N - 1;
  const bool owner = w == 0 && g < N;
  double* ws_s = ws;                           // per level: count of x > 0, then the weight scale
  double* ws_w = ws + (long long)nlev * N;     // per level: sum of the milder weights
  double* ws_d = ws + 2LL * nlev * N;          // per level: sum of x * weight, then the shift added to x
  // pass 1: row sums of the milder weights 1 - k (1 - matw) and of x * weight, per level
  double rs = 0.0, sxw = 0.0;
  for (int L = 0; L < nlev; ++L) {
    double k = 0.0, sw = 0.0, sx = 0.0;
    for (int j = lev_off[L] + w; j < lev_off[L + 1]; j += kVnWaves) {
      const int c = order[j];
      const double x = vn_x(counts[(long long)c * ld + gg], models[4LL * C + c], models[3LL * C + c]);
      const double w0 = 1.0 - weight_k * (1.0 - wsrc[(long long)c * N + gg]);
      k += x > 0.0 ? 1.0 : 0.0;
      sw += w0;
      sx += x * w0;
    }
    k = vn_block_sum(k, red, w, lane);
    sw = vn_block_sum(sw, red, w, lane);
    sx = vn_block_sum(sx, red, w, lane);
    rs += sw;
    sxw += sx;
    if (owner && batched) {
      ws_s[(long long)L * N + g] = k;
      ws_w[(long long)L * N + g] = sw;
      ws_d[(long long)L * N + g] = sx;
    }
  }
  // the weights are w0 / rs from here on (1728); their sum is 1
  const double mean = sxw / rs;
  // pass 2: the observed weighted variance before any batch adjustment (1733-1735)
  double ov = 0.0;
  for (int j = w; j < C; j += kVnWaves) {
    const int c = order[j];
    const double x = vn_x(counts[(long long)c * ld + gg], models[4LL * C + c], models[3LL * C + c]);
    const double w0 = 1.0 - weight_k * (1.0 - wsrc[(long long)c * N + gg]);
    const double d = x - mean;
    ov += d * d * w0;
  }
  ov = vn_block_sum(ov, red, w, lane) / rs;
  double vr = arv[gg] / ov;
  if (ov <= 0.0) vr = 0.0;
  const double sq = sqrt(vr);
  // batch adjustment (1740-1772) and the final centring (1803), folded into one shift per level
  if (owner) {
    if (batched) {
      double nbub = INFINITY;
      for (int L = 0; L < nlev; ++L) {
        const double u = vn_wsu(ws_s[(long long)L * N + g], (double)(lev_off[L + 1] - lev_off[L]));
        nbub = u < nbub ? u : nbub;
      }
      double SW = 0.0, SXW = 0.0;
      for (int L = 0; L < nlev; ++L) {
        const double nl = (double)(lev_off[L + 1] - lev_off[L]);
        const double r = ceil(nbub * nl) / ws_s[(long long)L * N + g];
        const double sc = r < 1.0 ? r : 1.0;  // pmin(1, .): a level without a positive x gives inf
        ws_s[(long long)L * N + g] = sc;
        SW += sc * ws_w[(long long)L * N + g] / rs;
        SXW += sc * ws_d[(long long)L * N + g] / rs;
      }
      const double nr = (double)C / SW;
      const double av = SXW / (double)C * nr;
      double tot = 0.0;  // sum of the re-centred x times the adjusted weights
      for (int L = 0; L < nlev; ++L) {
        const double nl = (double)(lev_off[L + 1] - lev_off[L]);
        const double sc = ws_s[(long long)L * N + g];
        const double swl = sc * ws_w[(long long)L * N + g] / rs, sxl = sc * ws_d[(long long)L * N + g] / rs;
        const double shift = sxl * nr / nl;
        tot += sxl + (av - shift) * swl;
        ws_d[(long long)L * N + g] = av - shift;
      }
      const double mean2 = tot / SW;
      for (int L = 0; L < nlev; ++L) ws_d[(long long)L * N + g] -= mean2;
    } else {
      ws_s[g] = 1.0;
      ws_d[g] = -mean;
    }
  }
  __syncthreads();  // wave 0's ws entries, for every wave of the workgroup
  // pass 3: mat and the weights that go with it
  if (g >= N) return;
  for (int L = 0; L < nlev; ++L) {
    const double sc = ws_s[(long long)L * N + g], sh = ws_d[(long long)L * N + g];
    for (int j = lev_off[L] + w; j < lev_off[L + 1]; j += kVnWaves) {
      const int c = order[j];
      const double x = vn_x(counts[(long long)c * ld + g], models[4LL * C + c], models[3LL * C + c]);
      const double w0 = 1.0 - weight_k * (1.0 - wsrc[(long long)c * N + g]);
      mat[(long long)c * N + g] = (x + sh) * sq;
      matw_out[(long long)c * N + g] = w0 / rs * sc;
    }
  }
}

// v: the aspect centred and scaled to unit length.  out = mat - nr v', nr = (mat * matw) v /
// (matw v^2), then (center) minus its weighted row mean (1855-1859).
__global__ __launch_bounds__(kVnWaves * 64) void k_subtract_aspect(const double* __restrict__ mat,
                                                                   const double* __restrict__ matw, int N, int C,
                                                                   const double* __restrict__ v, int center,
                                                                   double* __restrict__ out) {
  __shared__ double red[kVnWaves][64];
  const int lane = threadIdx.x & 63, w = vn_wave();
  const int g = blockIdx.x * 64 + lane;
  const int gg = g < N ? g : N - 1;
  double num = 0.0, den = 0.0;
  for (int c = w; c < C; c += kVnWaves) {
    const double x = mat[(long long)c * N + gg], ww = matw[(long long)c * N + gg], vc = v[c];
    num += x * ww * vc;
    den += ww * (vc * vc);
  }
  num = vn_block_sum(num, red, w, lane);
  den = vn_block_sum(den, red, w, lane);
  const double nr = num / den;
  double mean = 0.0;
  if (center) {
    double sx = 0.0, sw = 0.0;
    for (int c = w; c < C; c += kVnWaves) {
      const double ww = matw[(long long)c * N + gg];
      sx += (mat[(long long)c * N + gg] - v[c] * nr) * ww;
      sw += ww;
    }
    sx = vn_block_sum(sx, red, w, lane);
    sw = vn_block_sum(sw, red, w, lane);
    mean = sx / sw;
  }
  if (g >= N) return;
  for (int c = w; c < C; c += kVnWaves) {
    const double t = mat[(long long)c * N + g] - v[c] * nr;
    out[(long long)c * N + g] = center ? t - mean : t;
  }
}

hipError_t launch_varnorm_moments(const int* counts, long long ld, int N, int C, const double* models, int local_theta,
                                  const double* modes, const double* matw, const double* bmatw, const int* codes,
                                  const VnEdf& edf, double th_lo, double th_hi, double power, double* out,
                                  hipStream_t st) {
  if (N <= 0 || C <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_varnorm_moments, dim3((N + 63) / 64), dim3(kVnWaves * 64), 0, st, counts, ld, N, C, models,
                     local_theta, modes, matw, bmatw, codes, edf, th_lo, th_hi, power, out);
  return hipGetLastError();
}

hipError_t launch_varnorm_matrix(const int* counts, long long ld, int N, int C, const double* models, const int* order,
                                 const int* lev_off, int nlev, int batched, const double* wsrc, double weight_k,
                                 const double* arv, double* ws, double* mat, double* matw_out, hipStream_t st) {
  if (N <= 0 || C <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_varnorm_matrix, dim3((N + 63) / 64), dim3(kVnWaves * 64), 0, st, counts, ld, N, C, models,
                     order, lev_off, nlev, batched, wsrc, weight_k, arv, ws, mat, matw_out);
  return hipGetLastError();
}

hipError_t launch_subtract_aspect(const double* mat, const double* matw, int N, int C, const double* v, int center,
                                  double* out, hipStream_t st) {
  if (N <= 0 || C <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_subtract_aspect, dim3((N + 63) / 64), dim3(kVnWaves * 64), 0, st, mat, matw, N, C, v, center,
                     out);
  return hipGetLastError();
}

}  // namespace scde
