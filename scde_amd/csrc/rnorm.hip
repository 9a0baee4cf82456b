// rnorm.hip -- R's rnorm() stream on the device (src/main/RNG.c, src/nmath/snorm.c, the default
// Mersenne-Twister / INVERSION kinds) for gfx950.
//
// The twister itself is sequential and stays on the host, which uploads its raw tempered 32-bit
// outputs.  k_rnorm turns each pair of them into one normal exactly as norm_rand() does:
//   unif_rand():  y * 2.3283064365386963e-10, moved off 0 and 1 by fixup()
//   norm_rand():  u = unif_rand(); u = (int)(2^27 u) + unif_rand(); qnorm(u / 2^27)
// and lays the values out as matrix(rnorm(ngenes * ncells), nrow = ngenes) stored with a gene's
// cells contiguous: draw t is gene t % ngenes, cell t / ngenes.  Built with -ffp-contract=off, so
// everything before qnorm's log / sqrt is the host's arithmetic bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "device_math.h"
#include "kernels.h"

namespace scde {
namespace {

__device__ __forceinline__ double r_unif(uint32_t y) {
  const double i2_32m1 = 2.328306437080797e-10;
  const double x = (double)y * 2.3283064365386963e-10;
  if (x <= 0.0) return 0.5 * i2_32m1;
  if ((1.0 - x) <= 0.0) return 1.0 - 0.5 * i2_32m1;
  return x;
}

// One thread per output element (writes coalesced along a gene's cells; the two raw words of a
// draw are one 8-byte load).
__global__ __launch_bounds__(256) void k_rnorm(const uint2* __restrict__ raw, int ngenes, int ncells,
                                               double* __restrict__ out) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)ngenes * ncells) return;
  const long long g = e / ncells, c = e % ncells;
  const uint2 w = raw[c * ngenes + g];
  const double big = 134217728.0;
  double u = r_unif(w.x);
  u = (double)(int)(big * u) + r_unif(w.y);
  out[e] = qnorm(u / big, true);
}

}  // namespace

hipError_t launch_rnorm(const uint32_t* raw, int ngenes, int ncells, double* out, hipStream_t st) {
  const long long n = (long long)ngenes * ncells;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rnorm, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st,
                     reinterpret_cast<const uint2*>(raw), ngenes, ncells, out);
  return hipGetLastError();
}

}  // namespace scde
