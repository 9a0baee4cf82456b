// boot.hip -- the bootstrap joint posterior in the reference's layout, for gfx950 (FP64).  None of
// these is the default bootstrap (kernels.hip holds it); they are the exact fallback and the options.
//
//   k_boot            src/jpmatLogBoot.cpp:251-271 with one workgroup per gene, lanes over grid
//                     points, 16 bootstrap accumulators per lane, draws folded into per-cell
//                     multiplicities, zero-count baseline: the calls that bootstrap over the T
//                     tables themselves, not over D and ELL rows
//   k_boot_exact      reference-order recomputation of the genes the fast kernels flag degenerate
//                     (sums dominated by clamp values)       [default path: runs when a gene is flagged]
//   k_noboot          nboot == 0 and the ensemble variant (src/jpmatLogBoot.cpp:237-248)
// Block reductions here sum the waves left to right.  The launchers follow the kernels.
#include <hip/hip_runtime.h>
#include <cmath>

#include "kernels.h"
#include "wave_ops.h"

namespace scde {

// ------------------------------------------------------------------ K2: bootstrap
// Wave-level reduce-scatter of BC values: after it, lane l holds the value for
// boot index (l >> (6 - log2 BC)) & (BC - 1) reduced over all 64 lanes.
template <int BC, bool MAX>
__device__ __forceinline__ double wave_reduce_scatter(double (&v)[BC], int lane) {
  constexpr int L2 = (BC == 16) ? 4 : (BC == 8) ? 3 : (BC == 4) ? 2 : (BC == 2) ? 1 : 0;
#pragma unroll
  for (int s = 0; s < L2; ++s) {
    const int half = BC >> (s + 1);
    const int mask = 32 >> s;
    const bool up = (lane & mask) != 0;
#pragma unroll
    for (int j = 0; j < half; ++j) {
      // Both halves are read unconditionally first: a ternary over the array elements
      // lets the optimizer merge the two reads into one lane-dependent index, which
      // lowers to a compare/select chain over the whole register array.
      const double lo = v[j], hi = v[j + half];
      const double send = up ? lo : hi;
      const double keep = up ? hi : lo;
      const double r = __shfl_xor(send, mask, 64);
      v[j] = MAX ? gt_max(keep, r) : keep + r;
    }
  }
  double x = v[0];
#pragma unroll
  for (int mask = 32 >> L2; mask >= 1; mask >>= 1) {
    const double r = __shfl_xor(x, mask, 64);
    x = MAX ? gt_max(x, r) : x + r;
  }
  return x;
}

template <int BC, bool MAX>
__device__ __forceinline__ void block_reduce_bc(double (&v)[BC], double* red, double* fin, int lane, int wid,
                                                int nw) {
  constexpr int L2 = (BC == 16) ? 4 : (BC == 8) ? 3 : (BC == 4) ? 2 : (BC == 2) ? 1 : 0;
  static_assert(BC == 16 || BC == 8 || BC == 4 || BC == 2 || BC == 1, "BC must be a power of two <= 16");
  const double x = wave_reduce_scatter<BC, MAX>(v, lane);
  const int idx = (lane >> (6 - L2)) & (BC - 1);
  if ((lane & ((64 >> L2) - 1)) == 0) red[wid * 16 + idx] = x;
  __syncthreads();
  if (threadIdx.x < BC) {
    double r = red[threadIdx.x];
    for (int w = 1; w < nw; ++w) r = MAX ? gt_max(r, red[w * 16 + threadIdx.x]) : r + red[w * 16 + threadIdx.x];
    fin[threadIdx.x] = r;
  }
  __syncthreads();
}

template <int BC, int KPT>
__device__ __forceinline__ void boot_pass(const BootArgs& a, int g, int b0, int n, const int2* __restrict__ E,
                                          const double* __restrict__ W, const double* __restrict__ Zs,
                                          double (&jpv)[KPT], double* red, double* fin, double* fin2) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nw = blockDim.x >> 6;
  const int G = a.G, GS = a.GS;
  double acc[KPT][BC];
#pragma unroll
  for (int j = 0; j < KPT; ++j) {
    const int k = tid + j * blockDim.x;
#pragma unroll
    for (int i = 0; i < BC; ++i) acc[j][i] = (Zs && k < G) ? Zs[(long long)(b0 + i) * GS + k] : 0.0;
  }
  const double* __restrict__ T = a.T;
  for (int e = 0; e < n; ++e) {
    const int2 en = E[e];
    const int cell = __builtin_amdgcn_readfirstlane(en.x);
    const int col = __builtin_amdgcn_readfirstlane(en.y);
    const int bc = __builtin_amdgcn_readfirstlane(a.base_col ? a.base_col[cell] : -1);
    const double* __restrict__ w = W + (long long)cell * a.Bp + b0;
    double wv[BC];
#pragma unroll
    for (int i = 0; i < BC; ++i) wv[i] = w[i];
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
      const int k = tid + j * blockDim.x;
      if (k < G) {
        double v = T[(long long)col * GS + k];
        if (bc >= 0) v -= T[(long long)bc * GS + k];
#pragma unroll
        for (int i = 0; i < BC; ++i) acc[j][i] = fma(wv[i], v, acc[j][i]);
      }
    }
  }
  // ---- per-boot softmax over the grid (max, exp, sum) ----
  double t[BC];
#pragma unroll
  for (int i = 0; i < BC; ++i) {
    double m = -INFINITY;
#pragma unroll
    for (int j = 0; j < KPT; ++j)
      if (tid + j * (int)blockDim.x < G) m = gt_max(m, acc[j][i]);
    t[i] = m;
  }
  block_reduce_bc<BC, true>(t, red, fin, lane, wid, nw);
  double mx[BC];
#pragma unroll
  for (int i = 0; i < BC; ++i) mx[i] = fin[i];
#pragma unroll
  for (int i = 0; i < BC; ++i) {
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
      const int k = tid + j * blockDim.x;
      const double d = acc[j][i] - mx[i];
      // exp(d) underflows to exactly 0 for d < -745.14; skip the call there
      const double ev = (k < G && d >= -746.0) ? exp(d) : 0.0;
      acc[j][i] = ev;
      s += ev;
    }
    t[i] = s;
  }
  block_reduce_bc<BC, false>(t, red, fin2, lane, wid, nw);
  if (tid < BC) {
    const int b = b0 + tid;
    const double m = mx[tid];
    if (b < a.nboot && !(fabs(m) <= a.degen_thresh)) a.degen[g] = 1;
    fin2[tid] = (b < a.nboot) ? 1.0 / (fin2[tid] * a.norm_mult) : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < BC; ++i) {
    const double r = fin2[i];
#pragma unroll
    for (int j = 0; j < KPT; ++j) jpv[j] = fma(acc[j][i], r, jpv[j]);
  }
  __syncthreads();
}

template <int KPT>
__global__ __launch_bounds__(1024) void k_boot(BootArgs a) {
  __shared__ double red[16 * 16];
  __shared__ double fin[16];
  __shared__ double fin2[16];
  const int tid = threadIdx.x;
  for (int g = blockIdx.x; g < a.ngenes; g += gridDim.x) {
    const int n = a.nnz[g];
    const int2* E = a.ent + (long long)g * a.ent_stride;
    const int set = a.wset ? a.wset[g] : 0;
    const double* W = a.Wt + (long long)set * a.ncells * a.Bp;
    const double* Zs = a.Z ? a.Z + (long long)set * a.Bp * a.GS : nullptr;
    double jpv[KPT];
#pragma unroll
    for (int j = 0; j < KPT; ++j) jpv[j] = 0.0;
    int b0 = 0;
    for (; b0 + 16 <= a.nboot; b0 += 16) boot_pass<16, KPT>(a, g, b0, n, E, W, Zs, jpv, red, fin, fin2);
    if (a.nboot - b0 >= 8) {
      boot_pass<8, KPT>(a, g, b0, n, E, W, Zs, jpv, red, fin, fin2);
      b0 += 8;
    }
    if (a.nboot - b0 >= 4) {
      boot_pass<4, KPT>(a, g, b0, n, E, W, Zs, jpv, red, fin, fin2);
      b0 += 4;
    }
    if (a.nboot - b0 > 0) boot_pass<4, KPT>(a, g, b0, n, E, W, Zs, jpv, red, fin, fin2);
#pragma unroll
    for (int j = 0; j < KPT; ++j) {
      const int k = tid + j * blockDim.x;
      if (k < a.G) a.out[(long long)g * a.out_g + (long long)k * a.out_k] = jpv[j];
    }
  }
}

// ------------------------------------------------------------------ block reductions (simple)
__device__ inline double block_max(double v, double* sh) {
  v = wave_max(v);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if (lane == 0) sh[wid] = v;
  __syncthreads();
  double r = sh[0];
  for (int w = 1; w < nw; ++w) r = gt_max(r, sh[w]);
  return r;
}
__device__ inline double block_sum(double v, double* sh) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
  __syncthreads();
  if (lane == 0) sh[wid] = v;
  __syncthreads();
  double r = sh[0];
  for (int w = 1; w < nw; ++w) r += sh[w];
  return r;
}

// Reference-order fallback: tjp accumulated draw by draw exactly as
// src/jpmatLogBoot.cpp:251-270 does, for genes flagged degenerate by k_boot.
template <int KPT>
__global__ __launch_bounds__(1024) void k_boot_exact(ExactArgs a) {
  __shared__ double sh[16];
  const int g = blockIdx.x + a.g_lo;
  if (!a.degen[g]) return;
  const int tid = threadIdx.x;
  const int set = a.wset ? a.wset[g] : 0;
  const int* dr = a.draws + (long long)set * a.nboot * a.ndraw;
  double jpv[KPT];
  for (int j = 0; j < KPT; ++j) jpv[j] = 0.0;
  for (int b = 0; b < a.nboot; ++b) {
    double t[KPT];
    for (int j = 0; j < KPT; ++j) t[j] = 0.0;
    const long long gu = a.gene_mod > 0 ? g % a.gene_mod : g;  // fused groups: the gene's uci row
    for (int d = 0; d < a.ndraw; ++d) {
      const int cell = dr[(long long)b * a.ndraw + d];
      if (cell < 0) continue;  // the shorter fused group's padding (uniform over the block)
      long long col;
      if (a.uci)
        col = a.ucl_off[cell] + a.uci[gu + a.ld_uci * cell];
      else
        col = (long long)cell * a.ngenes + g;  // jpmat layout: matrix-major rows
      // fused tables: T = D + D[baseline column] (<= 1 ulp of T; clamped values exact)
      const int bc = a.base_col ? a.base_col[cell] : -1;
      const double* base = (bc >= 0 && bc != col) ? a.T + (long long)bc * a.GS : nullptr;
      for (int j = 0; j < KPT; ++j) {
        const int k = tid + j * blockDim.x;
        if (k < a.G) {
          const double tv = base ? __dadd_rn(a.T[col * a.GS + k], base[k]) : a.T[col * a.GS + k];
          t[j] = __dadd_rn(t[j], tv);
        }
      }
    }
    double m = -INFINITY;
    for (int j = 0; j < KPT; ++j)
      if (tid + j * (int)blockDim.x < a.G) m = gt_max(m, t[j]);
    m = block_max(m, sh);
    double s = 0.0;
    for (int j = 0; j < KPT; ++j) {
      const int k = tid + j * blockDim.x;
      t[j] = (k < a.G) ? exp(t[j] - m) : 0.0;
      s += t[j];
    }
    s = block_sum(s, sh);
    const double den = s * a.norm_mult;
    for (int j = 0; j < KPT; ++j) jpv[j] += t[j] / den;
  }
  for (int j = 0; j < KPT; ++j) {
    const int k = tid + j * blockDim.x;
    if (k < a.G) a.out[(long long)g * a.out_g + (long long)k * a.out_k] = jpv[j];
  }
}

// nboot == 0 (src/jpmatLogBoot.cpp:237-248): sum over cells in order, softmax.
template <int KPT>
__global__ __launch_bounds__(1024) void k_noboot(NoBootArgs a) {
  __shared__ double sh[16];
  const int g = blockIdx.x, tid = threadIdx.x;
  double t[KPT];
  for (int j = 0; j < KPT; ++j) t[j] = 0.0;
  for (int c = 0; c < a.ncells; ++c) {
    const long long col = a.ucl_off[c] + a.uci[(long long)g + a.ld_uci * c];
    const double* src = a.T + col * a.GS;
    for (int j = 0; j < KPT; ++j) {
      const int k = tid + j * blockDim.x;
      if (k < a.G) t[j] = __dadd_rn(t[j], src[k]);
    }
  }
  if (a.ensemble) {
    double s = 0.0;
    for (int j = 0; j < KPT; ++j) s += (tid + j * (int)blockDim.x < a.G) ? t[j] : 0.0;
    s = block_sum(s, sh);
    for (int j = 0; j < KPT; ++j) t[j] = t[j] / s;
  } else {
    double m = -INFINITY;
    for (int j = 0; j < KPT; ++j)
      if (tid + j * (int)blockDim.x < a.G) m = gt_max(m, t[j]);
    m = block_max(m, sh);
    double s = 0.0;
    for (int j = 0; j < KPT; ++j) {
      const int k = tid + j * blockDim.x;
      t[j] = (k < a.G) ? exp(t[j] - m) : 0.0;
      s += t[j];
    }
    s = block_sum(s, sh);
    for (int j = 0; j < KPT; ++j) t[j] = t[j] / s;
  }
  for (int j = 0; j < KPT; ++j) {
    const int k = tid + j * blockDim.x;
    if (k < a.G) a.out[(long long)g * a.out_g + (long long)k * a.out_k] = t[j];
  }
}

// ================================================================== launchers
static inline int block_for_grid(int G, int* kpt) {
  int b = ((G + 63) / 64) * 64;
  *kpt = 1;
  while (b > 1024) {
    *kpt *= 2;
    b = ((G + *kpt * 64 - 1) / (*kpt * 64)) * 64;
  }
  return b;
}

hipError_t launch_boot(const BootArgs& a, hipStream_t s) {
  if (a.ngenes <= 0) return hipSuccess;
  int kpt;
  const int block = block_for_grid(a.G, &kpt);
  const int grid = a.ngenes;
  switch (kpt) {
    case 1: hipLaunchKernelGGL(k_boot<1>, dim3(grid), dim3(block), 0, s, a); break;
    case 2: hipLaunchKernelGGL(k_boot<2>, dim3(grid), dim3(block), 0, s, a); break;
    case 4: hipLaunchKernelGGL(k_boot<4>, dim3(grid), dim3(block), 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_boot_exact(const ExactArgs& a, hipStream_t s) {
  const int g_lo = a.g_hi >= 0 ? a.g_lo : 0, g_hi = a.g_hi >= 0 ? a.g_hi : a.ngenes;
  if (g_lo < 0 || g_hi > a.ngenes || g_lo > g_hi) return hipErrorInvalidValue;
  if (g_hi == g_lo) return hipSuccess;
  ExactArgs b = a;
  b.g_lo = g_lo;  // blockIdx.x + g_lo
  int kpt;
  const int block = block_for_grid(a.G, &kpt);
  const dim3 grid(g_hi - g_lo);
  switch (kpt) {
    case 1: hipLaunchKernelGGL(k_boot_exact<1>, grid, dim3(block), 0, s, b); break;
    case 2: hipLaunchKernelGGL(k_boot_exact<2>, grid, dim3(block), 0, s, b); break;
    case 4: hipLaunchKernelGGL(k_boot_exact<4>, grid, dim3(block), 0, s, b); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_noboot(const NoBootArgs& a, hipStream_t s) {
  if (a.ngenes <= 0) return hipSuccess;
  int kpt;
  const int block = block_for_grid(a.G, &kpt);
  switch (kpt) {
    case 1: hipLaunchKernelGGL(k_noboot<1>, dim3(a.ngenes), dim3(block), 0, s, a); break;
    case 2: hipLaunchKernelGGL(k_noboot<2>, dim3(a.ngenes), dim3(block), 0, s, a); break;
    case 4: hipLaunchKernelGGL(k_noboot<4>, dim3(a.ngenes), dim3(block), 0, s, a); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace scde
