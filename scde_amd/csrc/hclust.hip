// hclust.hip -- agglomerative hierarchical clustering (R's stats::hclust for the monotone
// linkages ward.D, ward.D2, single, complete, average, mcquitty) for gfx950.  All FP64.
// The contract (pair selection, update formulas, output encoding) is include/scde_hip.h's.
//
//   k_hclust   one workgroup per problem, the whole merge loop on chip (as wpca.hip runs its EM
//              loop): a plain for of n - 1 steps synchronised by __syncthreads() only.  No
//              workgroup ever waits for another one; a batch is a grid of independent blocks.
//
// Per problem the HBM workspace holds a full symmetric working copy W of the distances (rows
// read coalesced; the caller's matrix is never written), a nearest-neighbour cache per row r
// over the columns c > r -- (nn_d, nn_j) = lexicographic min of (W[r][c], c) -- cluster sizes,
// active flags and the list of rows to rescan.  One step:
//   1. block arg-min of (nn_d[r], r) over the active rows: the lexicographic minimum of
//      (d(i, j), i, j), i < j
//   2. Lance-Williams update of row and column i, each thread owning the k it updates; slot j
//      retires.  Row k's cache is kept by comparison where that decides it ((value, index)
//      against the cached pair; index breaks equal distances); rows whose cached neighbour was
//      i or j and grew are listed
//   3. the listed rows (row i always) are rescanned by teams of 64..1024 threads, the fewer
//      rows the wider the team
// Values are compared numerically (-0.0 ties with 0.0); a NaN that overflow produced along the
// way compares as +inf.  Every expression is written in the header's order and the file is
// built with -ffp-contract=off, so a step's arithmetic is the same IEEE operations as a
// left-to-right float64 evaluation.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "kernels.h"

namespace scde {
namespace {

constexpr int kHT = 1024, kHW = kHT / 64;
constexpr int kU = 4;  // elements a thread loads per batch

__device__ __forceinline__ double nan_last(double v) { return v != v ? INFINITY : v; }

__device__ __forceinline__ bool pair_less(double d, int i, double bd, int bi) {
  return d < bd || (d == bd && i < bi);
}

// lexicographic minimum of (d, i) over the wave, in every lane
__device__ __forceinline__ void wave_min(double& d, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double od = __shfl_xor(d, o);
    const int oi = __shfl_xor(i, o);
    if (pair_less(od, oi, d, i)) {
      d = od;
      i = oi;
    }
  }
}

template <int M>
__device__ __forceinline__ double lance_williams(double dik, double djk, double h, double ni, double nj, double nk) {
  if (M == 0 || M == 1) return ((ni + nk) * dik + (nj + nk) * djk - nk * h) / (ni + nj + nk);
  if (M == 2) return fmin(dik, djk);
  if (M == 3) return fmax(dik, djk);
  if (M == 4) return (ni * dik + nj * djk) / (ni + nj);
  return (dik + djk) / 2;
}

template <int M>
__global__ __launch_bounds__(kHT) void k_hclust(const double* src, const HclustProblem* __restrict__ probs,
                                                char* ws, int* __restrict__ oi, int* __restrict__ oj,
                                                double* __restrict__ oh, long long* __restrict__ flag) {
  __shared__ double s_d[kHW];
  __shared__ int s_i[kHW];
  __shared__ long long s_bad[kHW];
  __shared__ int s_cnt;
  const HclustProblem pr = probs[blockIdx.x];
  const int n = pr.n, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long ld = pr.ld, nl = n;
  const double* D = src + pr.src_off;
  double* W = reinterpret_cast<double*>(ws + pr.ws_off);
  double* nnd = W + nl * nl;
  double* sz = nnd + n;
  int* nnj = reinterpret_cast<int*>(sz + n);
  int* list = nnj + n;
  unsigned char* act = reinterpret_cast<unsigned char*>(list + n);
  oi += pr.out_off;
  oj += pr.out_off;
  oh += pr.out_off;

  // ---- entry: the strict lower triangle is checked and copied (squared for ward.D2) into both
  // triangles of W.  bad: the first non-finite pair in column-major (as.dist) order.
  long long bad = LLONG_MAX;
  // (here and in the loops below a thread's kU loads are issued together, ahead of the stores
  // that depend on them: one memory latency per batch, not per element)
  for (int j = 0; j < n - 1; ++j)
    for (int i0 = j + 1 + tid; i0 < n; i0 += kU * kHT) {
      double v[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int i = i0 + u * kHT;
        v[u] = D[(i < n ? i : i0) + j * ld];
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int i = i0 + u * kHT;
        if (i >= n) continue;
        if (!(fabs(v[u]) < INFINITY) && bad == LLONG_MAX) bad = j * nl + i;
        const double x = M == 1 ? v[u] * v[u] : v[u];
        W[j * nl + i] = x;
        W[i * nl + j] = x;
      }
    }
  for (int k = tid; k < n; k += kHT) {
    sz[k] = 1.0;
    act[k] = 1;
    list[k] = k;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long ob = __shfl_xor(bad, o);
    bad = ob < bad ? ob : bad;
  }
  if (lane == 0) s_bad[wave] = bad;
  __syncthreads();
  for (int w = 0; w < kHW; ++w) bad = s_bad[w] < bad ? s_bad[w] : bad;
  if (bad != LLONG_MAX) {  // a flagged problem writes no merges
    if (tid == 0) flag[blockIdx.x] = bad;
    return;
  }

  // rows list[0 .. L) get their cache rebuilt: teams of kHT / teams threads, one row per team
  // and round; the bounds are the same for every thread, so the barriers are too
  auto rescan = [&](int L) {
    int teams = 1;
    while (teams < L && teams < kHW) teams <<= 1;
    const int T = kHT / teams, wpt = T >> 6;
    const int team = tid / T, tt = tid - team * T;
    for (int base = 0; base < L; base += teams) {
      const int e = base + team;
      double bd = INFINITY;
      int bj = INT_MAX, r = 0;
      if (e < L) {
        r = list[e];
        const double* row = W + r * nl;
        for (int c0 = r + 1 + tt; c0 < n; c0 += kU * T) {
          double v[kU];
          bool on[kU];
#pragma unroll
          for (int u = 0; u < kU; ++u) {
            const int c = c0 + u * T, cc = c < n ? c : c0;
            v[u] = row[cc];
            on[u] = act[cc] != 0 && c < n;
          }
#pragma unroll
          for (int u = 0; u < kU; ++u) {
            const double x = nan_last(v[u]);
            if (on[u] && pair_less(x, c0 + u * T, bd, bj)) {
              bd = x;
              bj = c0 + u * T;
            }
          }
        }
      }
      wave_min(bd, bj);
      if (lane == 0) {
        s_d[wave] = bd;
        s_i[wave] = bj;
      }
      __syncthreads();
      if (e < L && tt == 0) {
        for (int w = team * wpt + 1; w < (team + 1) * wpt; ++w)
          if (pair_less(s_d[w], s_i[w], bd, bj)) {
            bd = s_d[w];
            bj = s_i[w];
          }
        nnj[r] = bj == INT_MAX ? -1 : bj;
        nnd[r] = bj == INT_MAX ? INFINITY : W[r * nl + bj];
      }
      __syncthreads();
    }
  };
  rescan(n);

  long long status = -1;
  for (int s = 0; s < n - 1; ++s) {
    // ---- 1. the pair: min of (nn_d[r], r); j follows from the row
    double bd = INFINITY;
    int bi = INT_MAX;
    for (int r0 = tid; r0 < n; r0 += kU * kHT) {
      double v[kU];
      bool on[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int r = r0 + u * kHT, rc = r < n ? r : r0;
        v[u] = nnd[rc];
        on[u] = act[rc] != 0 && nnj[rc] >= 0 && r < n;
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const double x = nan_last(v[u]);
        if (on[u] && pair_less(x, r0 + u * kHT, bd, bi)) {
          bd = x;
          bi = r0 + u * kHT;
        }
      }
    }
    wave_min(bd, bi);
    if (lane == 0) {
      s_d[wave] = bd;
      s_i[wave] = bi;
    }
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    bd = s_d[0];
    bi = s_i[0];
    for (int w = 1; w < kHW; ++w)
      if (pair_less(s_d[w], s_i[w], bd, bi)) {
        bd = s_d[w];
        bi = s_i[w];
      }
    const int i = bi;
    const int j = i < n ? nnj[i] : -1;
    // the cache names a pair i < j < n by construction; anything else is reported, not indexed
    // with (status -2 - step).  Only values no thread writes in this step are looked at (the LDS
    // result and row i's cache: act[j] is cleared below by j's owner), so every thread decides alike
    if (i >= n || j <= i || j >= n) {
      status = -2 - s;
      break;
    }
    const double h = nnd[i];
    // ---- 2. Lance-Williams update of row / column i; thread k owns row k's cache here
    const double ni = sz[i], nj = sz[j];
    double* ri = W + i * nl;
    const double* rj = W + j * nl;
    for (int k0 = tid; k0 < n; k0 += kU * kHT) {
      double dik[kU], djk[kU], nk[kU], cdv[kU];
      int cj[kU];
      bool on[kU];
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int k = k0 + u * kHT, kc = k < n ? k : k0;
        dik[u] = ri[kc];
        djk[u] = rj[kc];
        nk[u] = sz[kc];
        cdv[u] = nnd[kc];
        cj[u] = nnj[kc];
        on[u] = act[kc] != 0 && k < n;
      }
#pragma unroll
      for (int u = 0; u < kU; ++u) {
        const int k = k0 + u * kHT;
        if (!on[u]) continue;
        if (k == i) {
          list[atomicAdd(&s_cnt, 1)] = i;
          continue;
        }
        if (k == j) {
          act[j] = 0;
          continue;
        }
        const double v = lance_williams<M>(dik[u], djk[u], h, ni, nj, nk[u]);
        ri[k] = v;
        W[k * nl + i] = v;
        if (k > j) continue;  // row k's cache covers the columns > k: neither i nor j
        const int c = cj[u];
        if (k > i) {  // column j left
          if (c == j) list[atomicAdd(&s_cnt, 1)] = k;
          continue;
        }
        const double vc = nan_last(v), cd = nan_last(cdv[u]);
        if (c == i || c == j) {
          // every other column was behind (cd, c) and i <= c: (v, i) leads while v <= cd
          if (vc <= cd) {
            nnd[k] = v;
            nnj[k] = i;
          } else {
            list[atomicAdd(&s_cnt, 1)] = k;
          }
        } else if (pair_less(vc, i, cd, c)) {
          nnd[k] = v;
          nnj[k] = i;
        }
      }
    }
    __syncthreads();
    if (tid == 0) {
      sz[i] = ni + nj;
      oi[s] = i;
      oj[s] = j;
      oh[s] = h;
    }
    // ---- 3. rescans (s_cnt is next written after the barriers inside)
    rescan(s_cnt);
  }
  if (tid == 0) flag[blockIdx.x] = status;
}

// 1 - x over an n x n matrix, the diagonal exactly 0 (as.matrix(as.dist(.)))
__global__ __launch_bounds__(256) void k_one_minus(double* __restrict__ x, long long n) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e < n * n) x[e] = e % (n + 1) == 0 ? 0.0 : 1.0 - x[e];
}

}  // namespace

size_t hclust_ws_bytes(int n) {
  const size_t b = sizeof(double) * ((size_t)n * n + 2 * (size_t)n) + sizeof(int) * 2 * (size_t)n + (size_t)n;
  return (b + 255) / 256 * 256;
}

hipError_t launch_hclust(const double* d, const HclustProblem* probs, int nprob, int method, char* ws, int* oi,
                         int* oj, double* oh, long long* flag, hipStream_t st) {
  if (nprob <= 0) return hipSuccess;
  const dim3 grid((unsigned)nprob), block(kHT);
  switch (method) {
    case 0: hipLaunchKernelGGL(k_hclust<0>, grid, block, 0, st, d, probs, ws, oi, oj, oh, flag); break;
    case 1: hipLaunchKernelGGL(k_hclust<1>, grid, block, 0, st, d, probs, ws, oi, oj, oh, flag); break;
    case 2: hipLaunchKernelGGL(k_hclust<2>, grid, block, 0, st, d, probs, ws, oi, oj, oh, flag); break;
    case 3: hipLaunchKernelGGL(k_hclust<3>, grid, block, 0, st, d, probs, ws, oi, oj, oh, flag); break;
    case 4: hipLaunchKernelGGL(k_hclust<4>, grid, block, 0, st, d, probs, ws, oi, oj, oh, flag); break;
    case 5: hipLaunchKernelGGL(k_hclust<5>, grid, block, 0, st, d, probs, ws, oi, oj, oh, flag); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

hipError_t launch_one_minus(double* x, long long n, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_one_minus, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, st, x, n);
  return hipGetLastError();
}

// The kernel's raw steps (slots i < j, height) in R's encoding: O(n) host work.
void hclust_encode(int n, const int* si, const int* sj, const double* sh, int method, int* merge, double* height,
                   int* order) {
  const int m = n - 1;
  std::vector<int> label(n);
  for (int k = 0; k < n; ++k) label[k] = -(k + 1);
  for (int s = 0; s < m; ++s) {
    int a = label[si[s]], b = label[sj[s]];
    // singleton before cluster; two singletons by index (a > b there: -i before -j); two
    // clusters by step
    const bool swap = (a < 0 && b < 0) ? false : (a < 0 || b < 0) ? (b < 0) : (b < a);
    if (swap) std::swap(a, b);
    merge[s] = a;
    merge[m + s] = b;
    label[si[s]] = s + 1;
    height[s] = method == 1 ? std::sqrt(sh[s]) : sh[s];
  }
  // leaves left to right: the last step expanded, column 1 as the left child
  std::vector<int> stack;
  stack.reserve(n);
  stack.push_back(m);
  int o = 0;
  while (!stack.empty()) {
    const int v = stack.back();
    stack.pop_back();
    if (v < 0) {
      order[o++] = -v;
    } else {
      stack.push_back(merge[m + v - 1]);
      stack.push_back(merge[v - 1]);
    }
  }
}

}  // namespace scde
