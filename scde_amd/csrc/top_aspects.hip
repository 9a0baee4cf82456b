// The matrix step of pagoda.top.aspects (R/functions.R:2434-2452): the scores of the valid
// aspects centred and scaled, their weights normalised.
//
//   k_top_aspects   per row r of x / w (m x C row-major, an aspect's cells contiguous):
//                     mean = sum(x) / C,  var = sum((x - mean)^2) / (C - 1)      (two passes)
//                     xv[r, c]  = (x[r, c] - mean) * (num[r] / sqrt(var))
//                     xvw[r, c] = w[r, c] / sum(w[r, ])
//
// One workgroup of kTaWaves waves per row.  Lane t takes the cell pairs (2k, 2k + 1), k = t,
// t + T, ... (T threads), as one 16-byte load where the row starts on a 16-byte boundary and as
// two 8-byte loads of the same cells where it does not (an odd C puts every other row there), so
// the cells a lane adds, and their order, depend on C alone.  The last cell of an odd C goes to
// the lane whose pair it would have opened.  A lane's partial goes down its wave by shuffles
// (a fixed tree), the waves' partials through LDS, added in wave order: no atomics, the same
// bits every run and for every placement of the buffers.  The second and third pass read the
// row again; it is at most a few tens of KB and still in L2.
//
// A constant row has var = 0: num / 0 = Inf, (x - mean) = 0, and 0 * Inf = NaN goes out, as the
// arithmetic says (R gives NaN there too).  C = 1 gives 0 / 0 = NaN.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace scde {

namespace {

constexpr int kTaWaves = 4;
constexpr int kTaThreads = kTaWaves * 64;

// The workgroup's sum of v, the same in every lane: shuffles inside a wave, then the waves'
// values from LDS in wave order.
__device__ inline double ta_block_sum(double v, double* red) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) red[w] = v;
  __syncthreads();
  double s = red[0];
  for (int k = 1; k < kTaWaves; ++k) s += red[k];
  __syncthreads();
  return s;
}

// cells 2k and 2k + 1 of a row (2k + 1 < C)
__device__ inline double2 ta_pair(const double* __restrict__ row, int k, bool aligned) {
  if (aligned) return *reinterpret_cast<const double2*>(row + 2 * (size_t)k);
  return make_double2(row[2 * (size_t)k], row[2 * (size_t)k + 1]);
}

__device__ inline void ta_store(double* __restrict__ row, int k, bool aligned, double a, double b) {
  if (aligned) {
    *reinterpret_cast<double2*>(row + 2 * (size_t)k) = make_double2(a, b);
  } else {
    row[2 * (size_t)k] = a;
    row[2 * (size_t)k + 1] = b;
  }
}

__global__ __launch_bounds__(kTaThreads) void k_top_aspects(const double* __restrict__ x,
                                                            const double* __restrict__ w,
                                                            const double* __restrict__ num, int C,
                                                            double* __restrict__ xv, double* __restrict__ xvw) {
  __shared__ double red[kTaWaves];
  const size_t base = (size_t)blockIdx.x * (size_t)C;
  const double* xr = x + base;
  const double* wr = w + base;
  double* ov = xv + base;
  double* ow = xvw + base;
  // (wave-uniform: one answer per row and matrix)
  const bool ax = ((uintptr_t)xr & 15) == 0, aw = ((uintptr_t)wr & 15) == 0;
  const bool av = ((uintptr_t)ov & 15) == 0, ao = ((uintptr_t)ow & 15) == 0;
  const int t = threadIdx.x;
  const int np = C >> 1;                            // whole pairs
  const bool last = (C & 1) && (np % kTaThreads) == t;  // this lane takes cell C - 1

  double sx = 0.0, sw = 0.0;
  for (int k = t; k < np; k += kTaThreads) {
    const double2 a = ta_pair(xr, k, ax), b = ta_pair(wr, k, aw);
    sx += a.x;
    sx += a.y;
    sw += b.x;
    sw += b.y;
  }
  if (last) {
    sx += xr[C - 1];
    sw += wr[C - 1];
  }
  sx = ta_block_sum(sx, red);
  sw = ta_block_sum(sw, red);
  const double mean = sx / (double)C;

  double ss = 0.0;
  for (int k = t; k < np; k += kTaThreads) {
    const double2 a = ta_pair(xr, k, ax);
    const double d0 = a.x - mean, d1 = a.y - mean;
    ss += d0 * d0;
    ss += d1 * d1;
  }
  if (last) {
    const double d = xr[C - 1] - mean;
    ss += d * d;
  }
  ss = ta_block_sum(ss, red);
  const double var = ss / (double)(C - 1);
  const double f = num[blockIdx.x] / sqrt(var);

  for (int k = t; k < np; k += kTaThreads) {
    const double2 a = ta_pair(xr, k, ax), b = ta_pair(wr, k, aw);
    ta_store(ov, k, av, (a.x - mean) * f, (a.y - mean) * f);
    ta_store(ow, k, ao, b.x / sw, b.y / sw);
  }
  if (last) {
    ov[C - 1] = (xr[C - 1] - mean) * f;
    ow[C - 1] = wr[C - 1] / sw;
  }
}

}  // namespace

hipError_t launch_top_aspects(const double* x, const double* w, const double* num, int m, int C, double* xv,
                              double* xvw, hipStream_t st) {
  if (m <= 0 || C <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_top_aspects, dim3(m), dim3(kTaThreads), 0, st, x, w, num, C, xv, xvw);
  return hipGetLastError();
}

}  // namespace scde
