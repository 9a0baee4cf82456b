// Spearman rank correlation (contract in include/scde_hip.h):
//
//   k_rank_sort     rank(ties.method = "average", na.last = "keep") of every column of a
//                   column-major matrix, one workgroup per column.  The column goes to LDS as
//                   64-bit keys that order like the doubles (-0 and +0 the same key, NaN the
//                   largest) with the row of each, and is bitonic-sorted; every sorted position
//                   then finds the first and one-past-last position of its key by binary search:
//                   rank = (first + last + 1) / 2.  Up to 8192 rows.
//   k_rank_count    longer columns: rank = #smaller + (#equal + 1) / 2 by counting, the column
//                   passed through LDS in tiles.  O(nrow^2) per column, never in place.
//
//   k_sp_codes      the cell similarity's prepass, one workgroup per cell: the cell's valid counts
//                   (count >= thr) are sorted (invalid ones as a sentinel, last), every sorted
//                   position gets the number of distinct values before it, and every valid gene
//                   the dense code of its value: its index among the cell's D distinct valid
//                   values.  Invalid genes get the code type's largest value.
//   k_sp_pairs      one workgroup per cell i and block of kSpBlock partners j >= i.  Per pair:
//                   the histograms of the two cells' codes over the genes valid in both (integer
//                   LDS atomics), a scan that turns them into the doubled average ranks
//                   A[v] = 2 * below + count + 1, then sum A_i[u_i] A_j[u_j] over the common
//                   genes in int64.  sum a^2 comes from the histogram: sum_v H[v] A[v]^2.  All
//                   sums are integers, so the reduction order changes no bit.  A pair whose two
//                   tables do not fit the LDS given to the launch keeps them in its workgroup's
//                   slice of a global workspace; both paths run the same statements.
// Every table index is a code the prepass produced, below the D it recorded for the cell.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "kernels.h"

namespace scde {

namespace {

constexpr int kRankSortMax = 8192;
constexpr int kRankTile = 2048;
constexpr int kCodeThreads = 1024;
constexpr int kCodeLdsMax = 32768;  // keys sorted in LDS (128 KB)
constexpr int kCodeWsGrid = 256;    // workgroups of a prepass that sorts in the workspace
constexpr int kSpThreads = 256;
constexpr int kSpBlock = 32;
constexpr int kSpLdsValuesMax = 36864;  // 144 KB of table entries
constexpr int kSpGridMax = 4096;
constexpr unsigned kKeyInvalid = 0xffffffffu;
constexpr int kCodePad = 8;  // a cell's codes start on 16 bytes: the pair kernel reads them as uint4

// ------------------------------------------------------------------ rank transform
__device__ inline unsigned long long rank_key(double v) {
  if (isnan(v)) return ~0ULL;
  if (v == 0.0) v = 0.0;  // -0 ties with +0
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}

// first position in the ascending key[0, n) that is not below k / that is above k
__device__ inline int key_lower(const unsigned long long* key, int n, unsigned long long k) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (key[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}
__device__ inline int key_upper(const unsigned long long* key, int n, unsigned long long k) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (key[mid] <= k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(1024) void k_rank_sort(const double* x, int nrow, int NP, double* out) {
  extern __shared__ unsigned long long rk_lds[];  // NP keys, then NP rows
  unsigned long long* key = rk_lds;
  int* row = reinterpret_cast<int*>(rk_lds + NP);
  const int tid = threadIdx.x, nt = blockDim.x;
  const double* xc = x + (size_t)blockIdx.x * nrow;
  double* oc = out + (size_t)blockIdx.x * nrow;
  for (int j = tid; j < NP; j += nt) {
    unsigned long long k = ~0ULL;
    if (j < nrow) {
      const double v = xc[j];
      k = rank_key(v);
      if (k == ~0ULL) oc[j] = v;  // a NaN stays what it is
    }
    key[j] = k;
    row[j] = j;
  }
  __syncthreads();
  for (int size = 2; size <= NP; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < NP / 2; t += nt) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool asc = (lo & size) == 0;
        const unsigned long long ka = key[lo], kb = key[hi];
        if (asc ? kb < ka : ka < kb) {  // equal keys share a rank: their order does not matter
          const int ia = row[lo], ib = row[hi];
          key[lo] = kb;
          key[hi] = ka;
          row[lo] = ib;
          row[hi] = ia;
        }
      }
      __syncthreads();
    }
  }
  const int nvalid = key_lower(key, NP, ~0ULL);  // NaN and the padding sorted last
  for (int r = tid; r < nvalid; r += nt) {
    const unsigned long long k = key[r];
    const int first = key_lower(key, nvalid, k), last = key_upper(key, nvalid, k);
    oc[row[r]] = 0.5 * (double)(first + last + 1);
  }
}

// out must not be x
__global__ __launch_bounds__(256) void k_rank_count(const double* __restrict__ x, int nrow, double* __restrict__ out) {
  __shared__ double tile[kRankTile];
  const int tid = threadIdx.x;
  const double* xc = x + (size_t)blockIdx.x * nrow;
  double* oc = out + (size_t)blockIdx.x * nrow;
  // every thread makes the same number of trips, so the barriers are reached by all
  for (int j0 = 0; j0 < nrow; j0 += 256) {
    const int j = j0 + tid;
    const double v = j < nrow ? xc[j] : NAN;
    int less = 0, eq = 0;
    for (int t0 = 0; t0 < nrow; t0 += kRankTile) {
      const int nt = min(kRankTile, nrow - t0);
      __syncthreads();
      for (int t = tid; t < nt; t += 256) tile[t] = xc[t0 + t];
      __syncthreads();
      for (int t = 0; t < nt; ++t) {
        const double w = tile[t];
        less += w < v ? 1 : 0;
        eq += w == v ? 1 : 0;
      }
    }
    if (j < nrow) oc[j] = isnan(v) ? v : (double)less + 0.5 * (double)(eq + 1);
  }
}

// ------------------------------------------------------------------ block-wide integer helpers
// exclusive prefix sum of v over the workgroup's threads (W waves); total: the sum.  wtot: W ints
template <int W>
__device__ inline int block_excl_scan(int v, int* wtot, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int incl = v;
  for (int off = 1; off < 64; off <<= 1) {
    const int o = __shfl_up(incl, off, 64);
    if (lane >= off) incl += o;
  }
  __syncthreads();  // (wtot may still be read from the previous call)
  if (lane == 63) wtot[wave] = incl;
  __syncthreads();
  int base = 0, tot = 0;
  for (int w = 0; w < W; ++w) {
    const int s = wtot[w];
    base += w < wave ? s : 0;
    tot += s;
  }
  total = tot;
  return base + incl - v;
}

__device__ inline long long wave_sum_ll(long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// ------------------------------------------------------------------ dense codes
__device__ inline int u32_lower(const unsigned* key, int n, unsigned k) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (key[mid] < k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

template <typename CodeT>
__device__ __forceinline__ void codes_of_cell(const int* __restrict__ cc, int N, int ldc, int thr, int NP, unsigned* keys,
                                              CodeT* __restrict__ code, int* wtot, int* dmax, int* dout) {
  constexpr CodeT kNone = (CodeT)~(CodeT)0;
  const int tid = threadIdx.x;
  for (int j = tid; j < NP; j += kCodeThreads) {
    const int cnt = j < N ? cc[j] : -1;
    keys[j] = (cnt >= thr && cnt >= 0) ? (unsigned)cnt : kKeyInvalid;
  }
  if (tid == 0) *dmax = 0;
  __syncthreads();
  for (int size = 2; size <= NP; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < NP / 2; t += kCodeThreads) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool asc = (lo & size) == 0;
        const unsigned ka = keys[lo], kb = keys[hi];
        if (asc ? kb < ka : ka < kb) {
          keys[lo] = kb;
          keys[hi] = ka;
        }
      }
      __syncthreads();
    }
  }
  // every valid gene: the first sorted position of its value (below N, so it fits the code type)
  for (int g = tid; g < N; g += kCodeThreads) {
    const int cnt = cc[g];
    if (cnt >= thr && cnt >= 0) code[g] = (CodeT)u32_lower(keys, NP, (unsigned)cnt);
  }
  // keys[r] <- the number of distinct values before position r's value: each thread owns
  // NP / kCodeThreads consecutive positions
  const int chunk = NP / kCodeThreads, r0 = tid * chunk;
  const unsigned before = r0 > 0 ? keys[r0 - 1] : 0u;
  int nnew = 0;
  {
    unsigned prev = before;
    for (int r = r0; r < r0 + chunk; ++r) {
      const unsigned k = keys[r];
      nnew += (r == 0 || k != prev) ? 1 : 0;
      prev = k;
    }
  }
  int total;
  int run = block_excl_scan<kCodeThreads / 64>(nnew, wtot, total);  // (its barriers: `before` is read by all)
  {
    unsigned prev = before;
    int d = 0;
    for (int r = r0; r < r0 + chunk; ++r) {
      const unsigned k = keys[r];
      run += (r == 0 || k != prev) ? 1 : 0;
      prev = k;
      keys[r] = (unsigned)(run - 1);
      if (k != kKeyInvalid) d = run;
    }
    if (d > 0) atomicMax(dmax, d);
  }
  __syncthreads();
  for (int g = tid; g < ldc; g += kCodeThreads) {  // (the padding up to ldc is not valid either)
    const int cnt = g < N ? cc[g] : -1;
    code[g] = (cnt >= thr && cnt >= 0) ? (CodeT)keys[code[g]] : kNone;
  }
  if (tid == 0) *dout = *dmax;
  __syncthreads();  // keys and dmax are the next cell's
}

// counts N x C (ld); codes ldc x C; D: C.  ws: null (keys in LDS) or gridDim.x slices of NP
template <typename CodeT>
__global__ __launch_bounds__(kCodeThreads) void k_sp_codes(const int* __restrict__ counts, long long ld, int N, int C,
                                                            int ldc, int thr, int NP, unsigned* ws,
                                                            CodeT* __restrict__ codes, int* __restrict__ D) {
  extern __shared__ unsigned cd_lds[];
  __shared__ int wtot[kCodeThreads / 64];
  __shared__ int dmax;
  for (int c = blockIdx.x; c < C; c += gridDim.x) {
    const int* cc = counts + (long long)c * ld;
    CodeT* code = codes + (size_t)c * ldc;
    if (ws) codes_of_cell<CodeT>(cc, N, ldc, thr, NP, ws + (size_t)blockIdx.x * NP, code, wtot, &dmax, D + c);
    else codes_of_cell<CodeT>(cc, N, ldc, thr, NP, cd_lds, code, wtot, &dmax, D + c);
  }
}

// ------------------------------------------------------------------ pairs
// 16 bytes of codes: a column is read in these (its leading dimension is a multiple of kCodePad)
template <typename CodeT>
union CodeVec {
  uint4 q;
  CodeT c[16 / sizeof(CodeT)];
};

// H: Di entries of cell i's table, then Dj of cell j's (zeroed here).  nvec: 16-byte vectors of a
// column.  Returns on thread 0 the pair's similarity.
template <typename CodeT>
__device__ __forceinline__ double pair_similarity(const uint4* __restrict__ ci, const uint4* __restrict__ cj, int nvec,
                                                  int Di, int Dj, unsigned* H, int* wtot, long long* red) {
  constexpr CodeT kNone = (CodeT)~(CodeT)0;
  constexpr int K = 16 / sizeof(CodeT);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned* Hi = H;
  unsigned* Hj = H + Di;
  for (int v = tid; v < Di + Dj; v += kSpThreads) H[v] = 0u;
  __syncthreads();
  for (int v = tid; v < nvec; v += kSpThreads) {
    CodeVec<CodeT> a, b;
    a.q = ci[v];
    b.q = cj[v];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const CodeT ui = a.c[k], uj = b.c[k];
      if (ui != kNone && uj != kNone) {
        atomicAdd(&Hi[ui], 1u);
        atomicAdd(&Hj[uj], 1u);
      }
    }
  }
  __syncthreads();
  // H[v] <- A[v] = 2 * (entries below v) + H[v] + 1; sq[t] = sum_v H[v] A[v]^2
  long long sq[2];
  int m = 0;
  for (int t = 0; t < 2; ++t) {
    unsigned* T = t ? Hj : Hi;
    const int Dt = t ? Dj : Di;
    const int chunk = (Dt + kSpThreads - 1) / kSpThreads;
    const int v0 = min(tid * chunk, Dt), v1 = min(v0 + chunk, Dt);
    int s = 0;
    for (int v = v0; v < v1; ++v) s += (int)T[v];
    int below = block_excl_scan<kSpThreads / 64>(s, wtot, m);
    long long q = 0;
    for (int v = v0; v < v1; ++v) {
      const int h = (int)T[v];
      const long long a = 2LL * below + h + 1;
      q += (long long)h * a * a;
      T[v] = (unsigned)a;
      below += h;
    }
    sq[t] = q;
  }
  __syncthreads();
  long long ab = 0;
  for (int v = tid; v < nvec; v += kSpThreads) {
    CodeVec<CodeT> a, b;
    a.q = ci[v];
    b.q = cj[v];
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const CodeT ui = a.c[k], uj = b.c[k];
      if (ui != kNone && uj != kNone) ab += (long long)Hi[ui] * (long long)Hj[uj];
    }
  }
  ab = wave_sum_ll(ab);
  const long long aa = wave_sum_ll(sq[0]), bb = wave_sum_ll(sq[1]);
  if (lane == 0) {
    red[wave * 3 + 0] = ab;
    red[wave * 3 + 1] = aa;
    red[wave * 3 + 2] = bb;
  }
  __syncthreads();
  double r = NAN;
  if (tid == 0) {
    long long sab = 0, saa = 0, sbb = 0;
    for (int w = 0; w < kSpThreads / 64; ++w) {
      sab += red[w * 3 + 0];
      saa += red[w * 3 + 1];
      sbb += red[w * 3 + 2];
    }
    const long long mm = (long long)m * (m + 1) * (m + 1);
    sab -= mm;
    saa -= mm;
    sbb -= mm;
    if (m > 0 && saa != 0 && sbb != 0) {
      r = __ddiv_rn((double)sab, __dsqrt_rn(__dmul_rn((double)saa, (double)sbb)));
      r = r > 1.0 ? 1.0 : (r < -1.0 ? -1.0 : r);
    }
  }
  __syncthreads();  // red, wtot and H are the next pair's
  return r;
}

// codes ldc x C; D: C; out C x C column-major.  Work item w: cell i = w / nblk and the
// partners j in [max(i, (w % nblk) * kSpBlock), ... + kSpBlock).  lds_cap: table entries in the
// launch's LDS; ws: gridDim.x slices of ws_stride entries for the pairs above it (null: none is).
template <typename CodeT>
__global__ __launch_bounds__(kSpThreads) void k_sp_pairs(const CodeT* __restrict__ codes, int ldc, int C,
                                                          const int* __restrict__ D, int lds_cap, unsigned* ws,
                                                          long long ws_stride, double* __restrict__ out) {
  extern __shared__ unsigned sp_lds[];
  __shared__ int wtot[kSpThreads / 64];
  __shared__ long long red[3 * (kSpThreads / 64)];
  const int nblk = (C + kSpBlock - 1) / kSpBlock;
  const long long nitems = (long long)C * nblk;
  const int nvec = ldc / (16 / (int)sizeof(CodeT));
  for (long long w = blockIdx.x; w < nitems; w += gridDim.x) {
    const int i = (int)(w / nblk), j0 = (int)(w % nblk) * kSpBlock;
    const int j1 = min(C, j0 + kSpBlock);
    const uint4* ci = reinterpret_cast<const uint4*>(codes + (size_t)i * ldc);
    const int Di = D[i];
    for (int j = max(i, j0); j < j1; ++j) {
      const uint4* cj = reinterpret_cast<const uint4*>(codes + (size_t)j * ldc);
      const int Dj = D[j];
      double r;
      if (Di + Dj <= lds_cap) r = pair_similarity<CodeT>(ci, cj, nvec, Di, Dj, sp_lds, wtot, red);
      else r = pair_similarity<CodeT>(ci, cj, nvec, Di, Dj, ws + (size_t)blockIdx.x * ws_stride, wtot, red);
      if (threadIdx.x == 0) {
        out[(size_t)j * C + i] = r;
        out[(size_t)i * C + j] = r;
      }
    }
  }
}

}  // namespace

// ------------------------------------------------------------------ launchers
bool rank_cols_needs_tmp(int nrow) { return nrow > kRankSortMax; }

hipError_t launch_rank_cols(const double* x, int nrow, int ncol, double* out, double* tmp, hipStream_t st) {
  if (nrow <= 0 || ncol <= 0) return hipSuccess;
  if (nrow <= kRankSortMax) {
    int NP = 2;
    while (NP < nrow) NP <<= 1;
    const size_t lds = (size_t)NP * (sizeof(unsigned long long) + sizeof(int));
    hipError_t e = hipFuncSetAttribute((const void*)k_rank_sort, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    const int nt = NP / 2 >= 1024 ? 1024 : (NP / 2 < 64 ? 64 : NP / 2);
    hipLaunchKernelGGL(k_rank_sort, dim3(ncol), dim3(nt), lds, st, x, nrow, NP, out);
    return hipGetLastError();
  }
  double* dst = out == x ? tmp : out;
  if (!dst) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_rank_count, dim3(ncol), dim3(256), 0, st, x, nrow, dst);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || dst == out) return e;
  return hipMemcpyAsync(out, dst, sizeof(double) * (size_t)nrow * ncol, hipMemcpyDeviceToDevice, st);
}

int spearman_code_bytes(int N) { return N <= 65535 ? 2 : 4; }
int spearman_code_ld(int N) { return (std::max(N, 1) + kCodePad - 1) / kCodePad * kCodePad; }

static int codes_np(int N) {
  int NP = kCodeThreads;
  while (NP < N) NP <<= 1;
  return NP;
}

size_t spearman_codes_ws_bytes(int N, int C) {
  const int NP = codes_np(N);
  return NP <= kCodeLdsMax ? 0 : sizeof(unsigned) * (size_t)NP * (size_t)std::min(C, kCodeWsGrid);
}

hipError_t launch_spearman_codes(const int* counts, long long ld, int N, int C, int thr, void* codes, int* D,
                                 unsigned* ws, hipStream_t st) {
  if (C <= 0) return hipSuccess;
  const int NP = codes_np(N);
  const bool in_lds = NP <= kCodeLdsMax;
  if (!in_lds && !ws) return hipErrorInvalidValue;
  const size_t lds = in_lds ? sizeof(unsigned) * (size_t)NP : 0;
  const int grid = in_lds ? C : std::min(C, kCodeWsGrid);
  hipError_t e;
  if (spearman_code_bytes(N) == 2) {
    e = hipFuncSetAttribute((const void*)k_sp_codes<unsigned short>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sp_codes<unsigned short>, dim3(grid), dim3(kCodeThreads), lds, st, counts, ld, N, C,
                       spearman_code_ld(N), thr, NP, in_lds ? nullptr : ws, static_cast<unsigned short*>(codes), D);
  } else {
    e = hipFuncSetAttribute((const void*)k_sp_codes<unsigned>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sp_codes<unsigned>, dim3(grid), dim3(kCodeThreads), lds, st, counts, ld, N, C,
                       spearman_code_ld(N), thr, NP, in_lds ? nullptr : ws, static_cast<unsigned*>(codes), D);
  }
  return hipGetLastError();
}

int spearman_lds_values_max() { return kSpLdsValuesMax; }

static int sp_lds_cap(int lds_values, int dmax) {
  const int cap = lds_values > 0 ? std::min(lds_values, kSpLdsValuesMax) : kSpLdsValuesMax;
  return (int)std::min<long long>(cap, 2LL * dmax);
}

static int sp_grid(int C) {
  const long long nitems = (long long)C * ((C + kSpBlock - 1) / kSpBlock);
  return (int)std::min<long long>(nitems, kSpGridMax);
}

size_t spearman_pairs_ws_bytes(int C, int dmax, int lds_values) {
  if (2LL * dmax <= sp_lds_cap(lds_values, dmax)) return 0;
  return sizeof(unsigned) * 2 * (size_t)dmax * (size_t)sp_grid(C);
}

hipError_t launch_spearman_pairs(const void* codes, int N, int C, const int* D, int dmax, int lds_values, unsigned* ws,
                                 double* out, hipStream_t st) {
  if (C <= 0) return hipSuccess;
  const int cap = sp_lds_cap(lds_values, dmax);
  if (2LL * dmax > cap && !ws) return hipErrorInvalidValue;
  const size_t lds = sizeof(unsigned) * (size_t)std::max(cap, 1);
  const int grid = sp_grid(C);
  hipError_t e;
  if (spearman_code_bytes(N) == 2) {
    e = hipFuncSetAttribute((const void*)k_sp_pairs<unsigned short>, hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sp_pairs<unsigned short>, dim3(grid), dim3(kSpThreads), lds, st,
                       static_cast<const unsigned short*>(codes), spearman_code_ld(N), C, D, cap, ws, 2LL * dmax, out);
  } else {
    e = hipFuncSetAttribute((const void*)k_sp_pairs<unsigned>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_sp_pairs<unsigned>, dim3(grid), dim3(kSpThreads), lds, st,
                       static_cast<const unsigned*>(codes), spearman_code_ld(N), C, D, cap, ws, 2LL * dmax, out);
  }
  return hipGetLastError();
}

}  // namespace scde
