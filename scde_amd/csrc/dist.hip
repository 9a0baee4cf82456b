// dist.hip -- drop-out-adjusted cell-to-cell correlations (the reference vignette's "Adjusted
// distance measures", vignettes/diffexp.md:231-301) for gfx950.  All FP64.
//
//   corr(x, y, w) = (Sxy/s - m1 m2) / sqrt((Sxx/s - m1^2) (Syy/s - m2^2)),
//   s = sum w, m1 = sum(x w)/s, m2 = sum(y w)/s, Sxy = sum(x y w), ...      (boot::corr)
//
//   k_wcorr_gram   weights that factor, w_g(i, j) = u[g, i] u[g, j]: the six raw moments of a
//                  pair are Gram products of U, U.X and U.X^2, accumulated over genes on the
//                  FP64 matrix cores (v_mfma_f64_16x16x4_f64), epilogue in the same kernel
//   k_recip        reciprocal weighting: the weight depends on the pair, so each lane owns
//                  four pairs and runs their six moments over LDS-staged gene chunks
//   k_dist_prep, k_dist_mode_prep, k_dist_direct_prep   the elementwise producers of X, U,
//                  fpm and p.self.fail from resident int32 counts
//
// Every sum runs in a fixed order (gene chunks in sequence, the MFMA's k chain inside a chunk;
// no atomics, no split over genes), so results repeat bit for bit from run to run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "kernels.h"

namespace scde {
namespace {

typedef double d4_t __attribute__((ext_vector_type(4)));

// scde.failure.probability (R/functions.R:725-750): 1 / (exp(conc.a m (+ conc.a2 m^2) + conc.b) + 1), NaN -> 0
template <int SQ>
__device__ __forceinline__ double fail_prob(double conc_a, double conc_a2, double conc_b, double m) {
  double e = conc_a * m;
  if (SQ) e = e + conc_a2 * (m * m);
  const double f = 1.0 / (exp(e + conc_b) + 1.0);
  return isnan(f) ? 0.0 : f;
}

// block b of the lower triangle (I >= J) of an nt x nt tile grid, row by row
__device__ __forceinline__ void tri_tile(int b, int& I, int& J) {
  int i = (int)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
  while ((long long)i * (i + 1) / 2 > b) --i;
  while ((long long)(i + 1) * (i + 2) / 2 <= b) ++i;
  I = i;
  J = b - (int)((long long)i * (i + 1) / 2);
}

__device__ __forceinline__ double corr_epilogue(double s, double swx, double swy, double sxx, double syy,
                                                double sxy) {
  const double m1 = swx / s, m2 = swy / s;
  return (sxy / s - m1 * m2) / sqrt((sxx / s - m1 * m1) * (syy / s - m2 * m2));
}

// cellp: 5 x C per-cell constants (corr.b, corr.a, conc.b, conc.a, conc.a2)
template <int SQ>
__global__ __launch_bounds__(256) void k_dist_prep(const int* __restrict__ counts, long long ld, int N, int C,
                                                   const double* __restrict__ cellp, double* __restrict__ x,
                                                   double* __restrict__ fpm, double* __restrict__ pself) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)N * C) return;
  const int g = (int)(e % N), c = (int)(e / N);
  const double cnt = (double)counts[(long long)c * ld + g];
  const double m = (log(cnt) - cellp[c]) / cellp[C + c];
  if (x) x[e] = log10(cnt + 1.0);
  if (fpm) fpm[e] = m;
  if (pself) pself[e] = fail_prob<SQ>(cellp[3LL * C + c], cellp[4LL * C + c], cellp[2LL * C + c], m);
}

// mode-relative weighting (vignette 285-300): X = log10(exp(modes) + 1),
// U = (1 - sqrt(p.self.fail sqrt(p.self.fail p.mode.fail)))^(1/4)
template <int SQ>
__global__ __launch_bounds__(256) void k_dist_mode_prep(const int* __restrict__ counts, long long ld, int N, int C,
                                                        const double* __restrict__ cellp,
                                                        const double* __restrict__ modes,
                                                        const double* __restrict__ jpm, double* __restrict__ x,
                                                        double* __restrict__ u) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)N * C) return;
  const int g = (int)(e % N), c = (int)(e / N);
  const double cnt = (double)counts[(long long)c * ld + g];
  const double m = (log(cnt) - cellp[c]) / cellp[C + c];
  const double ca = cellp[3LL * C + c], ca2 = cellp[4LL * C + c], cb = cellp[2LL * C + c];
  const double ps = fail_prob<SQ>(ca, ca2, cb, m);
  const double pm = fail_prob<SQ>(ca, ca2, cb, jpm[g]);
  const double matw = 1.0 - sqrt(ps * sqrt(ps * pm));
  x[e] = log10(exp(modes[e]) + 1.0);
  u[e] = sqrt(sqrt(matw));
}

__host__ __device__ inline uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

// direct drop-out (vignette 241-258): entry (g, c) kept with probability q = 1 - p.self.fail k.
// unif: this simulation's genes x cells uniforms, or null for the counter-based generator
// u01 = (mix64(key ^ mix64(g + N c + 1)) >> 11) 2^-53 (key from (seed, simulation), host side).
__global__ __launch_bounds__(256) void k_dist_direct_prep(const double* __restrict__ xin,
                                                          const double* __restrict__ pself, long long NC,
                                                          double k, const double* __restrict__ unif, uint64_t key,
                                                          double* __restrict__ x, double* __restrict__ u) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= NC) return;
  const double u01 =
      unif ? unif[e] : (double)(mix64(key ^ mix64((uint64_t)e + 1)) >> 11) * (1.0 / 9007199254740992.0);
  const double q = 1.0 - pself[e] * k;
  bool keep;
  if (q == 0.0) keep = false;
  else if (q == 1.0) keep = true;
  else if (q <= 0.5) keep = u01 >= 1.0 - q;
  else keep = u01 < q;
  x[e] = keep ? xin[e] : 0.0;
  u[e] = keep ? 1.0 : 0.0;
}

// ---- separable weighted correlation.  One block per 32 x 32 tile of cell pairs (I >= J), one
// wave per 16 x 16 sub-tile.  A chunk of kGK genes of X and U for the tile's 64 cells is read
// along genes (coalesced) through registers into LDS rows of kGS = kGK + 2 doubles; lane (r, k4) then reads row r
// at gene kk + k4 -- 2 r + k4 mod 32 names 32 different 8-byte banks in each half wave.  The
// MFMA operand maps are those of k_stretch_mask (kernels.hip): A[lane & 15][lane >> 4],
// B[lane >> 4][lane & 15]; D column lane & 15, rows (lane >> 4) + 4 j.
constexpr int kGT = 32, kGK = 32, kGS = kGK + 2;

__global__ __launch_bounds__(256) void k_wcorr_gram(const double* __restrict__ X, const double* __restrict__ U,
                                                    long long ld, int N, int C, double* __restrict__ out,
                                                    int accumulate) {
  __shared__ double sx[2 * kGT][kGS], su[2 * kGT][kGS];
  int I, J;
  tri_tile(blockIdx.x, I, J);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int r = lane & 15, k4 = lane >> 4;
  const int ra = (w >> 1) * 16 + r, rb = kGT + (w & 1) * 16 + r;
  d4_t sw = {0, 0, 0, 0}, swx = sw, swy = sw, sxx = sw, syy = sw, sxy = sw;
  // the next chunk's global loads are issued into registers before this chunk's MFMAs, so
  // their latency runs behind the matrix work
  constexpr int kLd = 2 * kGT * kGK / 256;
  double xr[kLd], ur[kLd];
  auto fetch = [&](int g0) {
#pragma unroll
    for (int t = 0; t < kLd; ++t) {
      const int e = tid + 256 * t;
      const int row = e / kGK, gg = e % kGK;
      const int cell = (row < kGT ? I * kGT : J * kGT - kGT) + row;
      const int g = g0 + gg;
      const bool ok = cell < C && g < N;
      const long long a = (long long)cell * ld + g;
      xr[t] = ok ? X[a] : 0.0;
      ur[t] = ok ? U[a] : 0.0;
    }
  };
  fetch(0);
  for (int g0 = 0; g0 < N; g0 += kGK) {
#pragma unroll
    for (int t = 0; t < kLd; ++t) {
      const int e = tid + 256 * t;
      sx[e / kGK][e % kGK] = xr[t];
      su[e / kGK][e % kGK] = ur[t];
    }
    __syncthreads();
    if (g0 + kGK < N) fetch(g0 + kGK);
#pragma unroll
    for (int kk = 0; kk < kGK; kk += 4) {
      const double xa = sx[ra][kk + k4], ua = su[ra][kk + k4];
      const double xb = sx[rb][kk + k4], ub = su[rb][kk + k4];
      const double ba = ua * xa, bb = ub * xb;
      const double ca = ba * xa, cb = bb * xb;
      sw = __builtin_amdgcn_mfma_f64_16x16x4f64(ua, ub, sw, 0, 0, 0);
      swx = __builtin_amdgcn_mfma_f64_16x16x4f64(ba, ub, swx, 0, 0, 0);
      swy = __builtin_amdgcn_mfma_f64_16x16x4f64(ua, bb, swy, 0, 0, 0);
      sxx = __builtin_amdgcn_mfma_f64_16x16x4f64(ca, ub, sxx, 0, 0, 0);
      syy = __builtin_amdgcn_mfma_f64_16x16x4f64(ua, cb, syy, 0, 0, 0);
      sxy = __builtin_amdgcn_mfma_f64_16x16x4f64(ba, bb, sxy, 0, 0, 0);
    }
    __syncthreads();
  }
  const int j = J * kGT + (w & 1) * 16 + r;
  if (j >= C) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int i = I * kGT + (w >> 1) * 16 + k4 + 4 * q;
    if (i >= C) continue;
    // a cell with itself: x is y, so sum(x y w) is sum(x^2 w) -- the same accumulated value, not
    // (u x)(u x) against ((u x) x) u rounded apart (the correlation is then exactly 1, or NaN)
    const double c = corr_epilogue(sw[q], swx[q], swy[q], sxx[q], syy[q], i == j ? sxx[q] : sxy[q]);
    // i >= j is computed and mirrored (a diagonal block holds both orders of its pairs)
    if (I == J && i < j) continue;
    const long long o = i + (long long)j * C, om = j + (long long)i * C;
    out[o] = accumulate ? out[o] + c : c;
    if (i != j) out[om] = accumulate ? out[om] + c : c;
  }
}

// ---- reciprocal weighting (vignette 268-278).  One block per 32 x 32 tile of pairs (I >= J);
// lane (li, jq) owns the pairs (I 32 + li, J 32 + jq + 8 q), q = 0..3: 24 running moments, the
// model constants of its i and of its four j in registers.  Chunks of kRK genes of fpm and
// log10(cd + 1) for the tile's 64 cells are staged [gene][cell] (row stride 65), so a half
// wave reads 32 consecutive i and one broadcast j.
constexpr int kRT = 32, kRK = 32, kRS = 2 * kRT + 1;

template <int SQ>
__global__ __launch_bounds__(256) void k_recip(const double* __restrict__ X, const double* __restrict__ F, int N,
                                               int C, const double* __restrict__ cellp, double k,
                                               double* __restrict__ out) {
  __shared__ double sx[kRK][kRS], sf[kRK][kRS];
  int I, J;
  tri_tile(blockIdx.x, I, J);
  const int tid = threadIdx.x, li = tid & 31, jq = tid >> 5;
  const int i = I * kRT + li;
  const int ic = i < C ? i : C - 1;
  const double ai = cellp[3LL * C + ic], a2i = cellp[4LL * C + ic], bi = cellp[2LL * C + ic];
  double aj[4], a2j[4], bj[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = J * kRT + jq + 8 * q;
    const int jc = j < C ? j : C - 1;
    aj[q] = cellp[3LL * C + jc];
    a2j[q] = cellp[4LL * C + jc];
    bj[q] = cellp[2LL * C + jc];
  }
  double s[4] = {0, 0, 0, 0}, swx[4] = {0, 0, 0, 0}, swy[4] = {0, 0, 0, 0}, sxx[4] = {0, 0, 0, 0},
         syy[4] = {0, 0, 0, 0}, sxy[4] = {0, 0, 0, 0};
  const double k1 = 1.0 - k;
  for (int g0 = 0; g0 < N; g0 += kRK) {
#pragma unroll
    for (int t = 0; t < 2 * kRT * kRK / 256; ++t) {
      const int e = tid + 256 * t;
      const int row = e / kRK, gg = e % kRK;
      const int cell = (row < kRT ? I * kRT : J * kRT - kRT) + row;
      const int g = g0 + gg;
      const bool ok = cell < C && g < N;
      const long long a = (long long)cell * N + g;
      sx[gg][row] = ok ? X[a] : 0.0;
      sf[gg][row] = ok ? F[a] : 0.0;
    }
    __syncthreads();
    const int gl = N - g0 < kRK ? N - g0 : kRK;
    for (int gg = 0; gg < gl; ++gg) {
      const double xi = sx[gg][li], fi = sf[gg][li];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const double xj = sx[gg][kRT + jq + 8 * q], fj = sf[gg][kRT + jq + 8 * q];
        const double p1 = fail_prob<SQ>(ai, a2i, bi, fj);        // cell i's model at j's magnitude
        const double p2 = fail_prob<SQ>(aj[q], a2j[q], bj[q], fi);  // cell j's model at i's magnitude
        const double wt = sqrt((1.0 - p1) * (1.0 - p2)) * k + k1;
        const double wx = wt * xi, wy = wt * xj;
        s[q] += wt;
        swx[q] += wx;
        swy[q] += wy;
        sxx[q] += wx * xi;
        syy[q] += wy * xj;
        sxy[q] += wt * (xi * xj);  // the same value for (i, j) and (j, i)
      }
    }
    __syncthreads();
  }
  if (i >= C) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = J * kRT + jq + 8 * q;
    if (j >= C) continue;
    const double c = corr_epilogue(s[q], swx[q], swy[q], sxx[q], syy[q], sxy[q]);
    // i >= j is computed and mirrored (a diagonal block holds both orders of its pairs)
    if (I == J && i < j) continue;
    out[i + (long long)j * C] = c;
    if (i != j) out[j + (long long)i * C] = c;
  }
}

inline unsigned tri_blocks(int C, int T) {
  const long long nt = (C + T - 1) / T;
  return (unsigned)(nt * (nt + 1) / 2);
}

}  // namespace

uint64_t dist_sim_key(uint64_t seed, int sim) {
  return mix64(seed + 0x9E3779B97F4A7C15ULL * ((uint64_t)sim + 1));
}

hipError_t launch_dist_prep(const int* counts, long long ld, int N, int C, const double* cellp, int sq, double* x,
                            double* fpm, double* pself, hipStream_t st) {
  const long long n = (long long)N * C;
  if (n <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (sq) hipLaunchKernelGGL(k_dist_prep<1>, grid, dim3(256), 0, st, counts, ld, N, C, cellp, x, fpm, pself);
  else hipLaunchKernelGGL(k_dist_prep<0>, grid, dim3(256), 0, st, counts, ld, N, C, cellp, x, fpm, pself);
  return hipGetLastError();
}

hipError_t launch_dist_mode_prep(const int* counts, long long ld, int N, int C, const double* cellp, int sq,
                                 const double* modes, const double* jpm, double* x, double* u, hipStream_t st) {
  const long long n = (long long)N * C;
  if (n <= 0) return hipSuccess;
  const dim3 grid((unsigned)((n + 255) / 256));
  if (sq) hipLaunchKernelGGL(k_dist_mode_prep<1>, grid, dim3(256), 0, st, counts, ld, N, C, cellp, modes, jpm, x, u);
  else hipLaunchKernelGGL(k_dist_mode_prep<0>, grid, dim3(256), 0, st, counts, ld, N, C, cellp, modes, jpm, x, u);
  return hipGetLastError();
}

hipError_t launch_dist_direct_prep(const double* xin, const double* pself, long long NC, double k,
                                   const double* unif, uint64_t key, double* x, double* u, hipStream_t st) {
  if (NC <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_dist_direct_prep, dim3((unsigned)((NC + 255) / 256)), dim3(256), 0, st, xin, pself, NC, k,
                     unif, key, x, u);
  return hipGetLastError();
}

hipError_t launch_wcorr_gram(const double* X, const double* U, long long ld, int N, int C, double* out,
                             int accumulate, hipStream_t st) {
  if (C <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_wcorr_gram, dim3(tri_blocks(C, kGT)), dim3(256), 0, st, X, U, ld, N, C, out, accumulate);
  return hipGetLastError();
}

hipError_t launch_recip_corr(const double* X, const double* F, int N, int C, const double* cellp, int sq, double k,
                             double* out, hipStream_t st) {
  if (C <= 0) return hipSuccess;
  const dim3 grid(tri_blocks(C, kRT));
  if (sq) hipLaunchKernelGGL(k_recip<1>, grid, dim3(256), 0, st, X, F, N, C, cellp, k, out);
  else hipLaunchKernelGGL(k_recip<0>, grid, dim3(256), 0, st, X, F, N, C, cellp, k, out);
  return hipGetLastError();
}

}  // namespace scde
