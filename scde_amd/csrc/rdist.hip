// rdist.hip -- R's stats::dist (euclidean, manhattan, maximum) between the rows of a column-major
// n x p matrix, for gfx950.  All FP64.  The contract (which columns take part, the left-to-right
// sum, the count scaling, the outputs) is include/scde_hip.h's.
//
//   k_rdist_flag   sets one int when any value of x is NaN or infinite.  Every thread that finds
//                  one stores the same 1 (no atomics); the host reads the int and picks the
//                  instantiation of k_rdist.
//   k_rdist<M, C>  one workgroup of 256 lanes per 64 x 64 tile of pairs, lower-triangle tiles only
//                  (tile row >= tile column).  A chunk of kRK columns of both row blocks is staged
//                  in LDS (the loads are contiguous along the rows: x is column-major), the next
//                  chunk's loads are in flight while this one is consumed, and every lane holds a
//                  4 x 4 register block of pairs.  The column index advances in order and a pair's
//                  sum lives in one lane from the first column to the last, so the sum is the
//                  contract's sequential one whatever the tiling.  COUNT = false (no NaN or Inf
//                  anywhere in x: every column takes part) carries no count and no select;
//                  COUNT = true adds 0.0 for a column that drops out, which changes no bit of a
//                  sum that is never -0.0, and keeps an int count per pair.  A tile is written to
//                  both triangles; d(i, j) and d(j, i) of a diagonal tile are written once, from
//                  the lane that holds i > j.
//
// The file is built with -ffp-contract=off: d * d and s + . are two roundings.
// (a - b)^2 == (b - a)^2 and |a - b| == |b - a| exactly, so the mirrored value is the value the
// contract gives for the swapped pair.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "kernels.h"

namespace scde {
namespace {

constexpr int kRT = 64;  // pair-tile edge
constexpr int kRK = 16;  // columns per LDS stage
constexpr int kRR = 4;   // register block edge: (kRT / kRR)^2 = 256 lanes
constexpr int kRB = (kRT / kRR) * (kRT / kRR);
constexpr int kRL = kRK * kRT / kRB;  // values of one operand a lane stages per chunk

__global__ __launch_bounds__(256) void k_rdist_flag(const double* __restrict__ x, long long ld, int n, int p,
                                                    int* __restrict__ flag) {
  const long long tot = (long long)n * p;
  bool bad = false;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < tot; e += (long long)gridDim.x * 256) {
    const double v = x[e % n + (e / n) * ld];
    bad |= !(fabs(v) < INFINITY);
  }
  if (bad) *flag = 1;
}

template <int METHOD, bool COUNT>
__global__ __launch_bounds__(kRB) void k_rdist(const double* __restrict__ x, long long ld, int n, int p,
                                               double* __restrict__ out) {
  __shared__ double sa[kRK][kRT], sb[kRK][kRT];
  // block -> (bi, bj), bi >= bj, blocks numbered row by row: bi (bi + 1) / 2 + bj
  const long long blk = blockIdx.x;
  long long bi = (long long)((sqrt(8.0 * (double)blk + 1.0) - 1.0) * 0.5);
  while (bi * (bi + 1) / 2 > blk) --bi;
  while ((bi + 1) * (bi + 2) / 2 <= blk) ++bi;
  const long long bj = blk - bi * (bi + 1) / 2;
  const int r0 = (int)bi * kRT, c0 = (int)bj * kRT;
  const int tid = threadIdx.x, tx = tid % (kRT / kRR), ty = tid / (kRT / kRR);
  // staging: lane tid takes row (tid & 63) of columns (tid >> 6) + 4 q of the chunk; a row past
  // n reads row 0 and is never written
  const int sr = tid % kRT, sk = tid / kRT;
  const long long ra = r0 + sr < n ? r0 + sr : 0, rb = c0 + sr < n ? c0 + sr : 0;
  // a column past p: 0 - 0 adds nothing to a sum (COUNT = false); NaN takes no part (COUNT = true)
  const double pad = COUNT ? (double)NAN : 0.0;
  double va[kRL], vb[kRL];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int q = 0; q < kRL; ++q) {
      const int k = k0 + sk + q * (kRB / kRT);
      const bool ok = k < p;
      const long long kc = ok ? k : 0;
      va[q] = x[ra + kc * ld];
      vb[q] = x[rb + kc * ld];
      if (!ok) va[q] = vb[q] = pad;
    }
  };
  double acc[kRR][kRR];
  int cnt[kRR][kRR];
#pragma unroll
  for (int i = 0; i < kRR; ++i)
#pragma unroll
    for (int j = 0; j < kRR; ++j) {
      acc[i][j] = 0.0;
      cnt[i][j] = 0;
    }
  if (p > 0) fetch(0);
  for (int k0 = 0; k0 < p; k0 += kRK) {
    __syncthreads();  // the previous chunk is consumed
#pragma unroll
    for (int q = 0; q < kRL; ++q) {
      sa[sk + q * (kRB / kRT)][sr] = va[q];
      sb[sk + q * (kRB / kRT)][sr] = vb[q];
    }
    __syncthreads();
    if (k0 + kRK < p) fetch(k0 + kRK);
#pragma unroll
    for (int kk = 0; kk < kRK; ++kk) {
      double a[kRR], b[kRR];
#pragma unroll
      for (int i = 0; i < kRR; ++i) {
        a[i] = sa[kk][ty * kRR + i];
        b[i] = sb[kk][tx * kRR + i];
      }
#pragma unroll
      for (int i = 0; i < kRR; ++i)
#pragma unroll
        for (int j = 0; j < kRR; ++j) {
          const double d = a[i] - b[j];
          double t = METHOD == 0 ? d * d : fabs(d);
          if (COUNT) {
            const bool in = d == d;  // NaN when either value is NaN, or Inf - Inf
            t = in ? t : 0.0;
            cnt[i][j] += in;
          }
          if (METHOD == 2) acc[i][j] = t > acc[i][j] ? t : acc[i][j];
          else acc[i][j] = acc[i][j] + t;
        }
    }
  }
#pragma unroll
  for (int i = 0; i < kRR; ++i) {
    const long long r = r0 + ty * kRR + i;
    if (r >= n) continue;
#pragma unroll
    for (int j = 0; j < kRR; ++j) {
      const long long c = c0 + tx * kRR + j;
      if (c >= n || c > r) continue;  // (c > r: the diagonal tile's other half)
      double s = acc[i][j];
      const int count = COUNT ? cnt[i][j] : p;
      if (count == 0) s = NAN;
      else if (METHOD != 2 && count != p) s = s / ((double)count / (double)p);
      if (METHOD == 0) s = sqrt(s);
      if (c == r) s = 0.0;
      out[r + c * (long long)n] = s;
      out[c + r * (long long)n] = s;
    }
  }
}

template <int METHOD>
hipError_t rdist_launch(const double* x, long long ld, int n, int p, bool count, double* out, hipStream_t s) {
  const long long nt = ((long long)n + kRT - 1) / kRT, nb = nt * (nt + 1) / 2;
  if (count) hipLaunchKernelGGL((k_rdist<METHOD, true>), dim3((unsigned)nb), dim3(kRB), 0, s, x, ld, n, p, out);
  else hipLaunchKernelGGL((k_rdist<METHOD, false>), dim3((unsigned)nb), dim3(kRB), 0, s, x, ld, n, p, out);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_rdist_flag(const double* x, long long ld, int n, int p, int* flag, hipStream_t s) {
  hipError_t e = hipMemsetAsync(flag, 0, sizeof(int), s);
  if (e != hipSuccess) return e;
  const long long tot = (long long)n * p;
  if (tot == 0) return hipSuccess;
  const long long nb = std::min<long long>((tot + 255) / 256, 2048);
  hipLaunchKernelGGL(k_rdist_flag, dim3((unsigned)nb), dim3(256), 0, s, x, ld, n, p, flag);
  return hipGetLastError();
}

hipError_t launch_rdist(const double* x, long long ld, int n, int p, int method, bool count, double* out,
                        hipStream_t s) {
  switch (method) {
    case 0: return rdist_launch<0>(x, ld, n, p, count, out, s);
    case 1: return rdist_launch<1>(x, ld, n, p, count, out, s);
    case 2: return rdist_launch<2>(x, ld, n, p, count, out, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace scde
