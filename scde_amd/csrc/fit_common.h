// fit_common.h -- what the per-cell EM kernels (knn_fit.hip, nb2_fit.hip) share: one workgroup of
// kFitThreads per cell, its LDS layout (the sums' landing area, a 256-bin histogram, the wave
// counts, then the per-gene vectors), the fixed-order block sum and the unrolled Cholesky solve.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "wave_ops.h"

namespace scde {

constexpr int kFitThreads = 256;
constexpr int kFitWaves = kFitThreads / 64;
constexpr int kFitMaxSums = 21;
// LDS ahead of the per-gene vectors: the sums' landing area, the histogram, the wave counts
constexpr int kFitRedBytes = kFitWaves * kFitMaxSums * 8;  // 672
constexpr int kFitHistOff = 704;
constexpr int kFitCntOff = kFitHistOff + 256 * 4;
constexpr int kFitVecOff = kFitCntOff + 64;  // 1792, a multiple of 16
static_assert(kFitRedBytes <= kFitHistOff, "the landing area overlaps the histogram");

struct FitVecs {
  double *l, *x, *w, *la, *mw;
  int *y, *gi;
};

__device__ __forceinline__ FitVecs fit_carve(char* base, size_t cap) {
  FitVecs v;
  v.l = reinterpret_cast<double*>(base);
  v.x = v.l + cap;
  v.w = v.x + cap;
  v.la = v.w + cap;
  v.mw = v.la + cap;
  v.y = reinterpret_cast<int*>(v.mw + cap);
  v.gi = v.y + cap;
  return v;
}

struct FitShared {
  double* red;
  unsigned* hist;
  int* wcnt;
};

// v[k] summed over the workgroup, the same bits on every thread
template <int K>
__device__ __forceinline__ void block_sum(double (&v)[K], const FitShared& sh, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) sh.red[wave * K + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double s = sh.red[k];
#pragma unroll
    for (int w = 1; w < kFitWaves; ++w) s += sh.red[w * K + k];
    v[k] = s;
  }
}

// x with A x = g (A symmetric positive definite, its lower triangle read): Cholesky without
// pivoting, unrolled; false when a pivot is not positive
template <int N>
__device__ __forceinline__ bool chol_solve(const double (&A)[N][N], const double (&g)[N], double (&x)[N]) {
  double L[N][N];
  bool ok = true;
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double d = A[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k];
    ok = ok && (d > 0.0);
    L[j][j] = sqrt(d);
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      double s = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      L[i][j] = s / L[j][j];
    }
  }
  double z[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double s = g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i][k] * z[k];
    z[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double s = z[i];
#pragma unroll
    for (int k = i + 1; k < N; ++k) s -= L[k][i] * x[k];
    x[i] = s / L[i][i];
  }
  return ok;
}

__device__ __forceinline__ double log_sigmoid(double eta) { return fmin(eta, 0.0) - log1p(exp(-fabs(eta))); }

// The cell's valid genes (fail prior fp not NaN) compacted in gene order into the vectors: fpm and
// its log, the correlated component's starting posterior 1 - fp, the count and the gene index.
// clusters and post (when given) of the other genes are cleared.
__device__ __forceinline__ void fit_compact(const FitVecs& v, const FitShared& sh, int N, const double* fpm,
                                            const double* fp, const int* cnt, int* cl_out, double* po_out, int tid) {
  const int lane = tid & 63, wave = tid >> 6;
  int base = 0;
  for (int g0 = 0; g0 < N; g0 += kFitThreads) {
    const int g = g0 + tid;
    const double f = g < N ? fp[g] : NAN;
    const bool valid = !isnan(f);
    const unsigned long long mask = __ballot(valid);
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
    if (valid) {
      const int i = off + pre;
      const double x = fpm[g];
      v.x[i] = x;
      v.l[i] = log(x);
      v.w[i] = 1.0 - f;
      v.y[i] = cnt[g];
      v.gi[i] = g;
    } else if (g < N) {
      if (cl_out) cl_out[g] = 0;
      if (po_out) po_out[g] = NAN;
    }
    base += total;
  }
}

__device__ __forceinline__ size_t fit_vec_bytes(size_t cap) { return cap * 48; }

}  // namespace scde
