// sigma1.hip -- the squared largest singular value of many column blocks of one resident matrix,
// for gfx950: the PC1 variance of every cluster of every random round of pagoda.gene.clusters
// (R/functions.R:2172-2175) in one launch.  All FP64.  The contract is include/scde_hip.h's.
//
//   k_sigma1sq   one workgroup per problem, three phases synchronised by __syncthreads() only:
//     1. the Gram matrix of the smaller side of the ncells x q block M (M'M when q <= ncells,
//        else MM') on the FP64 matrix cores (v_mfma_f64_16x16x4_f64, the operand staging of
//        dist.hip's k_wcorr_gram: 32 x 32 tiles, I >= J, one wave per 16 x 16 sub-tile, chunks of
//        32 of the summed side through LDS), written to both triangles of the workspace and
//        scaled by a power of two so that its largest entry is in [0.5, 1)
//     2. Householder tridiagonalisation (LAPACK dsytd2's recurrences on full symmetric storage,
//        so that rows read coalesced): per step a column norm, a matrix-vector product, a dot
//        product and a symmetric rank-2 update
//     3. the largest eigenvalue of the tridiagonal matrix by Sturm counts (dstebz's pivot
//        recurrence): each pass 256 lanes count at 256 points of the bracket [lo, hi], one of
//        them the midpoint, until no double lies between lo and hi.  hi, the smallest double at
//        which every pivot is <= 0, is the result
// Every sum runs in a fixed order that depends on the problem alone (the MFMA's k chain over
// chunks in sequence; a thread's strided partial, then the wave butterfly, then four waves added
// in order): no atomics, nothing depends on the grid or on the other problems of the launch.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "kernels.h"
#include "wave_ops.h"

namespace scde {
namespace {

typedef double d4_t __attribute__((ext_vector_type(4)));

constexpr int kSB = 256;                           // threads per problem
constexpr int kST = 32, kSK = 32, kSS = kSK + 2;   // Gram tile, chunk of the summed side, LDS row stride

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

__global__ __launch_bounds__(kSB) void k_sigma1sq(const double* __restrict__ X, int ncells, long long ngenes,
                                                  const long long* __restrict__ off, const int* __restrict__ idx,
                                                  const long long* __restrict__ ws_off, double* ws,
                                                  double* __restrict__ out, int* __restrict__ flag) {
  __shared__ double sx[2 * kST][kSS];
  __shared__ double red[4];
  const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const long long o0 = off[p], q = off[p + 1] - o0;
  const int* __restrict__ ix = idx + o0;
  // no column index is used before all of them have been checked
  int bad = 0;
  for (long long t = tid; t < q; t += kSB) bad |= (ix[t] < 0) | (ix[t] >= ngenes);
  if (__syncthreads_or(bad)) {
    if (tid == 0) {
      out[p] = NAN;
      flag[p] = 1;
    }
    return;
  }
  if (tid == 0) flag[p] = 0;
  const bool by_gene = q <= ncells;             // M'M (q x q), else MM' (ncells x ncells)
  const int n = by_gene ? (int)q : ncells;      // order of the Gram matrix
  const long long K = by_gene ? ncells : q;     // length of the summed side
  const long long nl = n;
  double* A = ws + ws_off[p];
  double* dg = A + nl * nl;
  double* e2 = dg + n;
  double* vv = e2 + n;
  double* wwv = vv + n;

  // ---- 1. Gram matrix
  const int r = lane & 15, k4 = lane >> 4;
  const int ra = (wv >> 1) * 16 + r, rb = kST + (wv & 1) * 16 + r;
  const int nt = (n + kST - 1) / kST;
  double gmax = 0.0;
  for (int I = 0; I < nt; ++I)
    for (int J = 0; J <= I; ++J) {
      d4_t acc = {0, 0, 0, 0};
      for (long long k0 = 0; k0 < K; k0 += kSK) {
#pragma unroll
        for (int t = 0; t < 2 * kST * kSK / kSB; ++t) {
          const int e = tid + kSB * t;
          // lanes run along the side that is contiguous in memory: the cells
          const int row = by_gene ? e / kSK : e % (2 * kST);
          const int kk = by_gene ? e % kSK : e / (2 * kST);
          const int gr = (row < kST ? I * kST : J * kST - kST) + row;
          const long long k = k0 + kk;
          double v = 0.0;
          if (gr < n && k < K) v = by_gene ? X[(long long)ix[gr] * ncells + k] : X[(long long)ix[k] * ncells + gr];
          sx[row][kk] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < kSK; kk += 4)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(sx[ra][kk + k4], sx[rb][kk + k4], acc, 0, 0, 0);
        __syncthreads();
      }
      const int j = J * kST + (wv & 1) * 16 + r;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int i = I * kST + (wv >> 1) * 16 + k4 + 4 * u;
        if (i >= n || j >= n || i < j) continue;  // i >= j is kept and mirrored
        const double g = acc[u];
        A[i + j * nl] = g;
        A[j + i * nl] = g;
        gmax = fmax(gmax, g != g ? INFINITY : fabs(g));
      }
    }
  gmax = block_max(gmax, red);  // (its barriers publish A)
  if (gmax == 0.0 || !(gmax < INFINITY) || n == 1) {
    // an all-zero block is exactly 0; one column (or one cell) is its sum of squares; a
    // non-finite entry is NaN
    if (tid == 0) out[p] = gmax == 0.0 ? 0.0 : (gmax < INFINITY ? A[0] : NAN);
    return;
  }
  int ex;
  (void)frexp(gmax, &ex);
  // (ldexp per element: the factor 2^-ex itself is not a double when the maximum is subnormal)
  for (long long t = tid; t < nl * nl; t += kSB) A[t] = ldexp(A[t], -ex);
  __syncthreads();

  // ---- 2. tridiagonalisation: dg the diagonal, e2 the off-diagonal (squared afterwards)
  for (int k = 0; k < n - 2; ++k) {
    const int m = n - k - 1;
    double* col = A + k * nl + (k + 1);   // x = A[k + 1 .., k]
    double* A22 = A + (k + 1) * nl + (k + 1);
    const double x0 = col[0];
    double ss = 0.0;
    for (int i = 1 + tid; i < m; i += kSB) ss += col[i] * col[i];
    ss = block_sum(ss, red);
    if (ss == 0.0) {  // nothing to annihilate (uniform over the block)
      if (tid == 0) {
        dg[k] = A[k + k * nl];
        e2[k] = x0;
      }
      continue;
    }
    const double beta = -copysign(sqrt(x0 * x0 + ss), x0);
    const double tau = (beta - x0) / beta;
    const double sc = 1.0 / (x0 - beta);
    for (int i = tid; i < m; i += kSB) vv[i] = i == 0 ? 1.0 : col[i] * sc;
    __syncthreads();
    // p = tau A22 v (a thread owns rows i, i + 256, ...), pv = p . v
    double pv = 0.0;
    for (int i = tid; i < m; i += kSB) {
      double s = 0.0;
      for (int j = 0; j < m; ++j) s = fma(A22[i + j * nl], vv[j], s);
      s *= tau;
      wwv[i] = s;
      pv = fma(s, vv[i], pv);
    }
    pv = block_sum(pv, red);
    const double alpha = -0.5 * tau * pv;
    for (int i = tid; i < m; i += kSB) wwv[i] = wwv[i] + alpha * vv[i];
    __syncthreads();
    // A22 -= v w' + w v', both triangles (the two products commute, so A22 stays symmetric)
    for (int j = wv; j < m; j += kSB / 64) {
      const double vj = vv[j], wj = wwv[j];
      for (int i = lane; i < m; i += 64) A22[i + j * nl] = A22[i + j * nl] - (vv[i] * wj + wwv[i] * vj);
    }
    if (tid == 0) {
      dg[k] = A[k + k * nl];
      e2[k] = beta;
    }
    __syncthreads();
  }
  if (tid == 0) {
    dg[n - 2] = A[(n - 2) + (n - 2) * nl];
    e2[n - 2] = A[(n - 1) + (n - 2) * nl];
    dg[n - 1] = A[(n - 1) + (n - 1) * nl];
    e2[n - 1] = 0.0;
  }
  __syncthreads();

  // ---- 3. the largest eigenvalue.  Gershgorin bracket, widened as dstebz widens it
  double gu = -INFINITY, gl = -INFINITY, emax = 0.0;  // gl holds -min
  for (int i = tid; i < n; i += kSB) {
    const double rad = (i > 0 ? fabs(e2[i - 1]) : 0.0) + fabs(e2[i]);
    gu = fmax(gu, dg[i] + rad);
    gl = fmax(gl, -(dg[i] - rad));
    emax = fmax(emax, fabs(e2[i]));
  }
  gu = block_max(gu, red);
  gl = -block_max(gl, red);
  emax = block_max(emax, red);
  for (int i = tid; i < n; i += kSB) e2[i] = e2[i] * e2[i];  // (every e2 was read before block_max's barriers)
  __syncthreads();
  const double pivmin = DBL_MIN * fmax(1.0, emax * emax);
  const double tnorm = fmax(fabs(gl), fabs(gu));
  const double slop = 2.1 * tnorm * (DBL_EPSILON * 0.5) * n + 2.1 * pivmin;
  double lo = gl - slop, hi = gu + slop;
  for (int pass = 0; pass < 4096 && nextafter(lo, INFINITY) < hi; ++pass) {
    const double width = hi - lo;
    const double x = lo + width * (tid == 0 ? 0.5 : (double)tid / (double)kSB);
    const bool inside = x > lo && x < hi;
    const bool all_below = inside && sturm_count(dg, e2, n, x, pivmin) == n;
    const double nhi = -block_max(inside && all_below ? -x : -hi, red);
    const double nlo = block_max(inside && !all_below ? x : lo, red);
    hi = nhi;
    lo = nlo;
  }
  if (tid == 0) out[p] = ldexp(hi, ex);
}

}  // namespace

size_t sigma1_ws_doubles(long long ncols, int ncells) {
  const size_t n = (size_t)(ncols < ncells ? ncols : ncells);
  return (n * n + 4 * n + 31) / 32 * 32;
}

hipError_t launch_sigma1sq(const double* x, int ncells, long long ngenes, int nprob, const long long* off,
                           const int* idx, const long long* ws_off, double* ws, double* out, int* flag,
                           hipStream_t st) {
  if (nprob <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_sigma1sq, dim3(nprob), dim3(kSB), 0, st, x, ncells, ngenes, off, idx, ws_off, ws, out, flag);
  return hipGetLastError();
}

}  // namespace scde
