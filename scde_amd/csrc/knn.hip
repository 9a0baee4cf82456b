// The neighbourhood stage of knn.error.models (R/functions.R:1180-1226; contract in
// include/scde_hip.h): the similarity's inputs, the k most similar cells of every cell, and the
// trimmed mean of the neighbours' library-scaled counts.
//
//   k_knn_prep         x = sqrt(count), u = 1 where count >= thr, both 0 elsewhere: what
//                      k_wcorr_gram (dist.hip) turns into the pairwise-complete correlation.
//
//   k_knn_neighbours   one workgroup per cell i.  Row i of the similarity goes to LDS as 64-bit
//                      keys that order like R's order(decreasing = TRUE): a larger similarity has
//                      the larger key, -0 and +0 the same one, NaN the smallest (0, below -Inf).
//                      Candidate j's position is the number of candidates l with key[l] > key[j],
//                      or the same key and l < j: counting, C comparisons per candidate, exact
//                      and the same every run.  Positions below the cell's k are written.
//
//   k_knn_magnitudes   one workgroup (kMagWaves waves) per gene.  The gene's C values
//                      count / ls are sorted once (bitonic, by value then cell index), so each
//                      cell has a rank.  Then one wave per cell i: the ranks of i's valid
//                      neighbours are set in a C-bit mask (integer LDS atomics), the lanes count
//                      their 64-bit words, a prefix sum over the lanes finds the words holding the
//                      lo-th and hi-th set bit and so the two ranks; a second walk over the
//                      neighbours adds the values whose rank lies between them.  Each lane adds
//                      its neighbours in list order, the lanes are combined by an exchange tree:
//                      no floating-point atomics, the same bits every run.  O(k) LDS operations
//                      per (gene, cell) beside the C / 64 mask words.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.h"

namespace scde {

namespace {

constexpr int kMagWaves = 8;
constexpr int kMagThreads = kMagWaves * 64;
constexpr int kNbThreads = 256;

constexpr unsigned kInfoValid = 1u << 30, kInfoAbove = 1u << 31, kInfoRank = 0xffffu;

__global__ __launch_bounds__(256) void k_knn_prep(const int* __restrict__ counts, long long ld, int N, int C, int thr,
                                                  double* __restrict__ x, double* __restrict__ u) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)N * C) return;
  const int g = (int)(e % N), c = (int)(e / N);
  const int cnt = counts[(long long)c * ld + g];
  const bool valid = cnt >= thr;
  x[e] = valid ? sqrt((double)cnt) : 0.0;
  u[e] = valid ? 1.0 : 0.0;
}

// larger similarity -> larger key; NaN -> 0
__device__ inline unsigned long long nb_key(double s) {
  if (isnan(s)) return 0ULL;
  if (s == 0.0) s = 0.0;  // -0 orders as +0
  const unsigned long long b = (unsigned long long)__double_as_longlong(s);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ULL);
}

// sim: C x C column-major; groups, kcell: per cell; out: C x kmax row-major
__global__ __launch_bounds__(kNbThreads) void k_knn_neighbours(const double* __restrict__ sim, int C,
                                                               const int* __restrict__ groups,
                                                               const int* __restrict__ kcell, int kmax,
                                                               int* __restrict__ out) {
  extern __shared__ unsigned long long nb_lds[];  // C keys, then C candidate flags
  unsigned long long* key = nb_lds;
  unsigned char* cand = reinterpret_cast<unsigned char*>(nb_lds + C);
  const int i = blockIdx.x, tid = threadIdx.x;
  const int gi = groups[i], kk = kcell[i];
  for (int j = tid; j < C; j += kNbThreads) {
    key[j] = nb_key(sim[(size_t)j * C + i]);
    cand[j] = (j != i && groups[j] == gi) ? 1 : 0;
  }
  int* row = out + (size_t)i * kmax;
  for (int t = kk + tid; t < kmax; t += kNbThreads) row[t] = -1;
  __syncthreads();
  for (int j = tid; j < C; j += kNbThreads) {
    if (!cand[j]) continue;
    const unsigned long long kj = key[j];
    int pos = 0;
    for (int l = 0; l < C; ++l) {
      const unsigned long long kl = key[l];
      pos += (cand[l] && (kl > kj || (kl == kj && l < j))) ? 1 : 0;
    }
    if (pos < kk) row[pos] = j;
  }
}

// cell a before cell b in the gene's order: by value, then by index; indices >= C (padding) last
__device__ inline bool mag_before(const double* v, int C, int a, int b) {
  if (a >= C) return b >= C && a < b;
  if (b >= C) return true;
  const double va = v[a], vb = v[b];
  return va < vb || (va == vb && a < b);
}

// position (0-based) of the nth (1-based) set bit of m; m has at least nth bits set
__device__ inline int nth_set_bit(unsigned long long m, int nth) {
  for (int q = 1; q < nth; ++q) m &= m - 1;
  return __ffsll(m) - 1;
}

// counts: N x C (ld); nb: C x kmax row-major, entries in [-1, C); ls: C; fpm, nabove: N x C dense
__global__ __launch_bounds__(kMagThreads) void k_knn_magnitudes(const int* __restrict__ counts, long long ld, int N,
                                                                int C, int CP, const int* __restrict__ nb, int kmax,
                                                                const double* __restrict__ ls, int thr, double trim,
                                                                double* __restrict__ fpm, int* __restrict__ nabove) {
  extern __shared__ __attribute__((aligned(16))) double mag_lds[];
  const int W64 = (C + 63) >> 6;  // mask words per wave
  double* v = mag_lds;                                                          // C values
  unsigned long long* mask = reinterpret_cast<unsigned long long*>(v + C);      // kMagWaves x W64
  unsigned* info = reinterpret_cast<unsigned*>(mask + (size_t)kMagWaves * W64);  // C: rank | flags
  unsigned short* sidx = reinterpret_cast<unsigned short*>(info + C);           // CP cells in order
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  for (int j = tid; j < CP; j += kMagThreads) {
    sidx[j] = (unsigned short)j;
    if (j < C) {
      const int cnt = counts[(long long)j * ld + g];
      v[j] = cnt >= thr ? (double)cnt / ls[j] : 0.0;  // (an entry that is not valid only takes a place in the order)
      info[j] = (cnt >= thr ? kInfoValid : 0u) | (cnt > thr ? kInfoAbove : 0u);
    }
  }
  __syncthreads();
  for (int size = 2; size <= CP; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int t = tid; t < CP / 2; t += kMagThreads) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool asc = (lo & size) == 0;
        const int a = sidx[lo], b = sidx[hi];
        const bool swap = asc ? mag_before(v, C, b, a) : mag_before(v, C, a, b);
        if (swap) {
          sidx[lo] = (unsigned short)b;
          sidx[hi] = (unsigned short)a;
        }
      }
      __syncthreads();
    }
  }
  for (int r = tid; r < C; r += kMagThreads) info[sidx[r]] |= (unsigned)r;  // the padding sorted last
  __syncthreads();

  unsigned long long* wm = mask + (size_t)wave * W64;
  unsigned* wm32 = reinterpret_cast<unsigned*>(wm);
  const int nchunks = (W64 + 63) >> 6;
  // every wave makes the same number of trips, so the barriers below are reached by all
  for (int i0 = 0; i0 < C; i0 += kMagWaves) {
    const int i = i0 + wave;
    const bool active = i < C;
    const int* row = nb + (size_t)(active ? i : 0) * kmax;
    if (active)
      for (int w = lane; w < W64; w += 64) wm[w] = 0ULL;
    __syncthreads();
    int above = 0;
    if (active) {
      for (int t = lane; t < kmax; t += 64) {
        const int j = row[t];
        if (j < 0) continue;
        const unsigned inf = info[j];
        above += (int)(inf >> 31);
        if (inf & kInfoValid) {
          const unsigned r = inf & kInfoRank;
          atomicOr(&wm32[r >> 5], 1u << (r & 31));
        }
      }
    }
    __syncthreads();
    if (!active) continue;  // (no barrier below this line)
    int n = 0;
    for (int c = 0; c < nchunks; ++c) {
      const int w = c * 64 + lane;
      n += w < W64 ? __popcll(wm[w]) : 0;
    }
    for (int off = 32; off > 0; off >>= 1) {
      n += __shfl_xor(n, off, 64);
      above += __shfl_xor(above, off, 64);
    }
    double res = NAN;
    if (n > 0) {
      int lo, hi;
      if (trim >= 0.5) {
        lo = (n + 1) >> 1;
        hi = (n >> 1) + 1;
      } else {
        lo = (int)floor((double)n * trim) + 1;
        hi = n + 1 - lo;
      }
      int rlo = -1, rhi = -1, base = 0;
      for (int c = 0; c < nchunks; ++c) {
        const int w = c * 64 + lane;
        const unsigned long long m = w < W64 ? wm[w] : 0ULL;
        const int pc = __popcll(m);
        int incl = pc;
        for (int off = 1; off < 64; off <<= 1) {
          const int o = __shfl_up(incl, off, 64);
          if (lane >= off) incl += o;
        }
        const int excl = base + incl - pc;
        const bool has_lo = lo > excl && lo <= excl + pc;
        const bool has_hi = hi > excl && hi <= excl + pc;
        const int cl = has_lo ? w * 64 + nth_set_bit(m, lo - excl) : -1;
        const int ch = has_hi ? w * 64 + nth_set_bit(m, hi - excl) : -1;
        const unsigned long long bl = __ballot(has_lo), bh = __ballot(has_hi);
        if (bl) rlo = __shfl(cl, __ffsll(bl) - 1, 64);
        if (bh) rhi = __shfl(ch, __ffsll(bh) - 1, 64);
        base += __shfl(incl, 63, 64);
      }
      double s = 0.0;
      for (int t = lane; t < kmax; t += 64) {
        const int j = row[t];
        if (j < 0) continue;
        const unsigned inf = info[j];
        const int r = (int)(inf & kInfoRank);
        if ((inf & kInfoValid) && r >= rlo && r <= rhi) s += v[j];
      }
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
      res = s / (double)(hi - lo + 1);
    }
    if (lane == 0) {
      fpm[(size_t)i * N + g] = res;
      nabove[(size_t)i * N + g] = above;
    }
  }
}

}  // namespace

hipError_t launch_knn_prep(const int* counts, long long ld, int N, int C, int thr, double* x, double* u,
                           hipStream_t st) {
  const long long n = (long long)N * C;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_knn_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, counts, ld, N, C, thr, x, u);
  return hipGetLastError();
}

hipError_t launch_knn_neighbours(const double* sim, int C, const int* groups, const int* kcell, int kmax, int* out,
                                 hipStream_t st) {
  if (C <= 0 || kmax <= 0) return hipSuccess;
  if (C > kKnnMaxCells) return hipErrorInvalidValue;
  const size_t lds = (size_t)C * 9 + 8;
  hipError_t e =
      hipFuncSetAttribute((const void*)k_knn_neighbours, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_knn_neighbours, dim3(C), dim3(kNbThreads), lds, st, sim, C, groups, kcell, kmax, out);
  return hipGetLastError();
}

hipError_t launch_knn_magnitudes(const int* counts, long long ld, int N, int C, const int* nb, int kmax,
                                 const double* ls, int thr, double trim, double* fpm, int* nabove, hipStream_t st) {
  if (N <= 0 || C <= 0) return hipSuccess;
  if (C > kKnnMaxCells) return hipErrorInvalidValue;
  int CP = 2;
  while (CP < C) CP <<= 1;
  const size_t W64 = (size_t)(C + 63) >> 6;
  const size_t lds = (size_t)C * 8 + (size_t)kMagWaves * W64 * 8 + (size_t)C * 4 + (size_t)CP * 2;
  hipError_t e =
      hipFuncSetAttribute((const void*)k_knn_magnitudes, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_knn_magnitudes, dim3(N), dim3(kMagThreads), lds, st, counts, ld, N, C, CP, nb, kmax, ls, thr,
                     trim, fpm, nabove);
  return hipGetLastError();
}

}  // namespace scde
