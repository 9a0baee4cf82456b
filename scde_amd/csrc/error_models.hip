// The input stage of scde.error.models under threshold segmentation (calculate.crossfit.models
// and the head of calculate.individual.models, R/functions.R:3030-3039, 3253-3303), as DESIGN.md
// section 4.16 and include/scde_hip.h state it: for every (gene, cell) the expected magnitude
// from the other cells of the cell's group, the number of those cells that detected the gene,
// and the failed-component starting posterior averaged over the cell's cross-fit partners.
//
//   k_crossfit_inputs  one thread per (gene, group).  Two sweeps over the group's cells in their
//                      order: forward, fpm[g, i] receives the sum of count / ls over the cells
//                      before i; backward, the sum over the cells after i is added and the total
//                      divided by n - 1.  Only positive terms are added (no total-minus-own
//                      cancellation) and the order is the group's cell order.  nabove is the
//                      group's count of detecting paired cells minus the cell's own: integers.
//   k_crossfit_prior   one thread per (gene, cell).  vi from nabove; over the cell's partner list
//                      the two kinds of pair are counted (integers), so the mean of their logs has
//                      no summation order at all; fail_prior and fpm become NaN outside vi.  Each
//                      wave adds its number of valid genes to the cell's counter (an integer
//                      atomic): the host sizes the fit's workspace from it.
// No floating-point atomics; the results repeat bit for bit.
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernels.h"

namespace scde {

namespace {

constexpr int kCfThreads = 256;

__global__ __launch_bounds__(kCfThreads) void k_crossfit_inputs(const int* __restrict__ counts, long long ld, int N,
                                                                const int* __restrict__ goff,
                                                                const int* __restrict__ members,
                                                                const int* __restrict__ poff,
                                                                const double* __restrict__ ls, int thr,
                                                                double* __restrict__ fpm, int* __restrict__ nabove) {
  const int g = blockIdx.x * kCfThreads + threadIdx.x;
  if (g >= N) return;
  const int m0 = goff[blockIdx.y], m1 = goff[blockIdx.y + 1];
  const int n = m1 - m0;
  double run = 0.0;
  int above = 0;
  for (int m = m0; m < m1; ++m) {
    const int c = members[m];
    const int y = counts[(long long)c * ld + g];
    fpm[(size_t)c * N + g] = run;
    run += (double)y / ls[c];
    above += (y >= thr && poff[c + 1] > poff[c]) ? 1 : 0;
  }
  run = 0.0;
  for (int m = m1 - 1; m >= m0; --m) {
    const int c = members[m];
    const int y = counts[(long long)c * ld + g];
    const size_t at = (size_t)c * N + g;
    fpm[at] = (fpm[at] + run) / (double)(n - 1);
    run += (double)y / ls[c];
    nabove[at] = above - ((y >= thr && poff[c + 1] > poff[c]) ? 1 : 0);
  }
}

__global__ __launch_bounds__(kCfThreads) void k_crossfit_prior(const int* __restrict__ counts, long long ld, int N,
                                                               const int* __restrict__ need,
                                                               const int* __restrict__ poff,
                                                               const int* __restrict__ part, int thr,
                                                               const int* __restrict__ nabove,
                                                               double* __restrict__ fpm, double* __restrict__ fp,
                                                               int* __restrict__ nvalid) {
  const int g = blockIdx.x * kCfThreads + threadIdx.x;
  const int c = blockIdx.y;
  bool valid = false;
  if (g < N) {
    const size_t at = (size_t)c * N + g;
    valid = nabove[at] >= need[c];
    double p = NAN;
    if (valid) {
      const int y = counts[(long long)c * ld + g];
      int high = 0, low = 0;
      for (int k = poff[c]; k < poff[c + 1]; ++k) {
        const int z = counts[(long long)part[k] * ld + g];
        if (y + z > 0) {
          if (y < thr && z >= thr) ++high;
          else ++low;
        }
      }
      // R's log(threshold.prior) and log(1 - threshold.prior), threshold.prior = 1 - 1e-6: the
      // second is the double 1 - (1 - 1e-6), which is 1e-6 (1 + 2.9e-11)
      const double tp = 1.0 - 1e-6;
      p = (high + low) > 0 ? exp(((double)high * log(tp) + (double)low * log(1.0 - tp)) / (double)(high + low))
                           : 1.0 - 1e-10;
    } else {
      fpm[at] = NAN;
    }
    fp[at] = p;
  }
  const unsigned long long mask = __ballot(valid);
  if ((threadIdx.x & 63) == 0 && mask) atomicAdd(&nvalid[c], __popcll(mask));
}

// ---- the same stage from any pairs' clusters and posteriors
//   k_reduce_vil     one thread per (gene, cell): over the cell's entries of the pair list, in the
//                    pairs' order and skipping failed pairs, whether every pair puts the gene in a
//                    cluster that is not the cell's failure component (nor 0), and the mean of the
//                    logs of that component's posterior where it is not NaN (the pair's rows) -- a
//                    sequential sum in that order.
//   k_reduce_sweeps  k_crossfit_inputs' two sweeps with vil in the place of count >= thr.
//   k_reduce_final   vi from nabove, NaN outside it, the cells' valid-gene counters.
__global__ __launch_bounds__(kCfThreads) void k_reduce_vil(int N, const int* __restrict__ poff,
                                                           const int* __restrict__ plist,
                                                           const int* __restrict__ pstatus,
                                                           const signed char* __restrict__ clusters,
                                                           const double* __restrict__ post,
                                                           unsigned char* __restrict__ vil,
                                                           double* __restrict__ fp) {
  const int g = blockIdx.x * kCfThreads + threadIdx.x;
  const int c = blockIdx.y;
  if (g >= N) return;
  int nok = 0, cnt = 0;
  bool all = true;
  double s = 0.0;
  for (int k = poff[c]; k < poff[c + 1]; ++k) {
    const int p = plist[k] >> 1, side = plist[k] & 1;
    if (pstatus[p] != 0) continue;
    ++nok;
    const int cl = clusters[(size_t)p * N + g];
    all = all && cl != 0 && (side == 0 ? cl >= 2 : cl <= 2);
    const double q = post[((size_t)p * 2 + side) * N + g];
    if (!isnan(q)) {  // (g is one of the pair's rows)
      s += log(q);
      ++cnt;
    }
  }
  const size_t at = (size_t)c * N + g;
  vil[at] = (nok > 0 && all) ? 1 : 0;
  fp[at] = cnt > 0 ? exp(s / (double)cnt) : 1.0 - 1e-10;
}

__global__ __launch_bounds__(kCfThreads) void k_reduce_sweeps(const int* __restrict__ counts, long long ld, int N,
                                                              const int* __restrict__ goff,
                                                              const int* __restrict__ members,
                                                              const unsigned char* __restrict__ vil,
                                                              const double* __restrict__ ls,
                                                              double* __restrict__ fpm, int* __restrict__ nabove) {
  const int g = blockIdx.x * kCfThreads + threadIdx.x;
  if (g >= N) return;
  const int m0 = goff[blockIdx.y], m1 = goff[blockIdx.y + 1];
  const int n = m1 - m0;
  double run = 0.0;
  int above = 0;
  for (int m = m0; m < m1; ++m) {
    const int c = members[m];
    const int y = counts[(long long)c * ld + g];
    fpm[(size_t)c * N + g] = run;
    run += (double)y / ls[c];
    above += vil[(size_t)c * N + g];
  }
  run = 0.0;
  for (int m = m1 - 1; m >= m0; --m) {
    const int c = members[m];
    const int y = counts[(long long)c * ld + g];
    const size_t at = (size_t)c * N + g;
    fpm[at] = (fpm[at] + run) / (double)(n - 1);
    run += (double)y / ls[c];
    nabove[at] = above - vil[at];
  }
}

__global__ __launch_bounds__(kCfThreads) void k_reduce_final(int N, const int* __restrict__ need,
                                                             const int* __restrict__ nabove,
                                                             double* __restrict__ fpm, double* __restrict__ fp,
                                                             int* __restrict__ nvalid) {
  const int g = blockIdx.x * kCfThreads + threadIdx.x;
  const int c = blockIdx.y;
  bool valid = false;
  if (g < N) {
    const size_t at = (size_t)c * N + g;
    valid = nabove[at] >= need[c];
    if (!valid) {
      fpm[at] = NAN;
      fp[at] = NAN;
    }
  }
  const unsigned long long mask = __ballot(valid);
  if ((threadIdx.x & 63) == 0 && mask) atomicAdd(&nvalid[c], __popcll(mask));
}

}  // namespace

hipError_t launch_crossfit_vil(int N, int C, const int* poff, const int* plist, const int* pstatus,
                               const signed char* clusters, const double* post, unsigned char* vil, double* fplog,
                               hipStream_t st) {
  if (N <= 0 || C <= 0) return hipSuccess;
  if (C > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_reduce_vil, dim3((N + kCfThreads - 1) / kCfThreads, C), dim3(kCfThreads), 0, st, N, poff, plist,
                     pstatus, clusters, post, vil, fplog);
  return hipGetLastError();
}

hipError_t launch_crossfit_reduce(const int* counts, long long ld, int N, int C, int ngroups, const int* goff,
                                  const int* members, const int* need, const int* poff, const int* plist,
                                  const int* pstatus, const signed char* clusters, const double* post,
                                  const double* ls, unsigned char* vil, double* fpm, double* fp, int* nabove,
                                  int* nvalid, hipStream_t st) {
  if (N <= 0 || C <= 0) return hipSuccess;
  if (ngroups < 1 || ngroups > 65535 || C > 65535) return hipErrorInvalidValue;
  const int bx = (N + kCfThreads - 1) / kCfThreads;
  hipLaunchKernelGGL(k_reduce_vil, dim3(bx, C), dim3(kCfThreads), 0, st, N, poff, plist, pstatus, clusters, post, vil,
                     fp);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_reduce_sweeps, dim3(bx, ngroups), dim3(kCfThreads), 0, st, counts, ld, N, goff, members, vil, ls,
                     fpm, nabove);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_reduce_final, dim3(bx, C), dim3(kCfThreads), 0, st, N, need, nabove, fpm, fp, nvalid);
  return hipGetLastError();
}

hipError_t launch_crossfit_inputs(const int* counts, long long ld, int N, int C, int ngroups, const int* goff,
                                  const int* members, const int* need, const int* poff, const int* part,
                                  const double* ls, int thr, double* fpm, double* fp, int* nabove, int* nvalid,
                                  hipStream_t st) {
  if (N <= 0 || C <= 0) return hipSuccess;
  if (ngroups < 1 || ngroups > 65535 || C > 65535) return hipErrorInvalidValue;
  const int bx = (N + kCfThreads - 1) / kCfThreads;
  hipLaunchKernelGGL(k_crossfit_inputs, dim3(bx, ngroups), dim3(kCfThreads), 0, st, counts, ld, N, goff, members,
                     poff, ls, thr, fpm, nabove);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_crossfit_prior, dim3(bx, C), dim3(kCfThreads), 0, st, counts, ld, N, need, poff, part, thr,
                     nabove, fpm, fp, nvalid);
  return hipGetLastError();
}

}  // namespace scde
