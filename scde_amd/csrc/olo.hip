// olo.hip -- optimal dendrogram leaf ordering (cba::order.optimal; the dynamic programme of
// Bar-Joseph, Gifford and Jaakkola 2001) for gfx950.  All FP64.  The contract (the table M, the
// top-down choice with its tie rule, the outputs) is include/scde_hip.h's.
//
//   k_olo_gather    d gathered into leaf-position order (both triangles of an n x n matrix D), so
//                   that every subtree is an index interval; the values read are checked finite
//   k_olo_minplus   the min-plus products.  Four waves per 64 x 64 output tile, each taking every
//                   fourth stage of 16 inner indices through its own LDS stage into an 8 x 8
//                   register block per lane; the four blocks are folded at the end.
//                   A node with children L, R takes two steps of two products each:
//                     1. T(u, k) = min_m fl(M(u, m) + D(m, k))    u in L, m in far(L, u), k in R
//                     2. M(u, w) = min_k fl(T(u, k) + M(k, w))    w in R, k in far(R, w)
//                   (a leaf child is the product with inner dimension 1 against M(x, x) = 0).
//                   Both operands are read with the output index contiguous: M is symmetric and
//                   kept in both triangles, and T is stored transposed (T(u, k) at [k][u]).
//   k_olo_root      the root's end points: partial (cost, p, p) minima over L_root x R_root
//   k_olo_back      the top-down choice, one launch per depth below the root and one workgroup
//                   per node of that depth (its end points come from its parent's launch), the
//                   (cost, p, p) arg-min of the node across the workgroup's lanes
//   k_olo_edges     the distances between neighbours of the final order (summed on the host: a
//                   left-to-right float64 sum of n - 1 values)
//
// Schedule.  level(v) = 1 + max(level(children)); the nodes of one level span disjoint intervals
// and need only lower levels, so each level is one launch of step 1 and one of step 2, blocks
// spread over (product, tile) through a prefix of tile counts.  The choice then goes down depth
// by depth.  A tree of `levels` levels takes 2 * levels + levels + 3 launches, all
// stream-ordered; no workgroup ever waits for another one.
//
// The file is built with -ffp-contract=off; fl(a + b) is commutative and min is exact, so any
// tiling or reduction order gives the bits of the contract's left-to-right evaluation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <vector>

#include "kernels.h"

namespace scde {
namespace {

constexpr int kOT = 64;    // output tile edge (one wave: 8 x 8 lanes of 8 x 8 values)
constexpr int kOK = 16;    // inner indices per LDS stage
constexpr int kOR = 8;     // register block edge
constexpr int kOW = 4;     // waves per output tile, each taking every fourth inner stage
constexpr int kBT = 1024;  // k_olo_back's workgroup
constexpr int kBW = kBT / 64;

// out(r, c) = min over i in [i0, i1) of A(r, i) + B(i, c), r in [r0, r1), c in [c0, c1); the
// product's tiles are tile0 .. tile0 + ntr * ntc - 1 of its launch, row tiles major
struct OloTask {
  int r0, r1, i0, i1, c0, c1, tile0, ntc;
};

// a step in position space: L = [lo, mid), R = [mid, hi); lmid / rmid split L / R (-1: a leaf);
// left / right: the children's steps (0-based; -1: a leaf)
struct OloNode {
  int lo, mid, hi, lmid, rmid, left, right, pad;
};

__global__ __launch_bounds__(256) void k_olo_gather(const double* __restrict__ d, long long ld,
                                                    const int* __restrict__ perm, int n, double* __restrict__ D,
                                                    unsigned long long* __restrict__ bad) {
  const int j = blockIdx.y * 256 + threadIdx.x, i = blockIdx.x;
  if (j >= n) return;
  double v = 0.0;
  if (i != j) {
    const int oi = perm[i], oj = perm[j];
    const int row = oi > oj ? oi : oj, col = oi > oj ? oj : oi;
    v = d[row + col * ld];
    if (!(fabs(v) < INFINITY)) atomicMin(bad, (unsigned long long)col * (unsigned long long)n + row);
  }
  D[(long long)i * n + j] = v;
}

// STEP 1: At = M, B = D, out = T transposed.  STEP 2: At = T transposed, B = M, out = M, both
// triangles.  At is indexed [i][r], B [i][c].  The four waves of a workgroup share one output
// tile and take the inner stages in turn (wave w the stages w, w + 4, ...), each with its own
// LDS stage, and fold their register blocks through LDS at the end: min is exact, so the split
// changes no bit, and a product with few tiles and a long inner range -- the deep trees' case --
// has four waves' loads in flight instead of one's.
template <int STEP>
__global__ __launch_bounds__(kOW * 64, 2) void k_olo_minplus(const OloTask* __restrict__ tasks, int ntask,
                                                             const double* __restrict__ At,
                                                             const double* __restrict__ B, double* __restrict__ out,
                                                             long long n) {
  __shared__ double lds[kOW * 2 * kOK * kOT];
  int tl = 0, th = ntask - 1;
  const int blk = blockIdx.x;
  while (tl < th) {
    const int tm = (tl + th + 1) >> 1;
    if (tasks[tm].tile0 <= blk) tl = tm;
    else th = tm - 1;
  }
  const OloTask t = tasks[tl];
  const int tile = blk - t.tile0;
  const int r0 = t.r0 + (tile / t.ntc) * kOT, c0 = t.c0 + (tile % t.ntc) * kOT;
  if (r0 >= t.r1) return;  // (a block past the launch's last tile: never launched)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, tx = lane & 7, ty = lane >> 3;
  double(*sa)[kOT] = reinterpret_cast<double(*)[kOT]>(lds + wave * 2 * kOK * kOT);
  double(*sb)[kOT] = sa + kOK;
  double acc[kOR][kOR];
#pragma unroll
  for (int i = 0; i < kOR; ++i)
#pragma unroll
    for (int j = 0; j < kOR; ++j) acc[i][j] = INFINITY;
  // a lane stages row r0 + lane of A and column c0 + lane of B; outside the product: +inf
  const bool ra_ok = r0 + lane < t.r1, cb_ok = c0 + lane < t.c1;
  const long long ra = ra_ok ? r0 + lane : t.r0, cb = cb_ok ? c0 + lane : t.c0;
  double va[kOK], vb[kOK];
  // one stage of operands into registers; the next stage's loads are in flight while this one's
  // products are formed.  A stage past the inner range is all +inf (every wave makes the same
  // number of rounds, so the barriers are uniform)
  auto fetch = [&](int i0) {
#pragma unroll
    for (int kk = 0; kk < kOK; ++kk) {
      const bool ok = i0 + kk < t.i1;
      const long long i = ok ? i0 + kk : t.i0;
      va[kk] = At[i * n + ra];
      vb[kk] = B[i * n + cb];
      if (!(ok && ra_ok)) va[kk] = INFINITY;
      if (!(ok && cb_ok)) vb[kk] = INFINITY;
    }
  };
  fetch(t.i0 + wave * kOK);
  for (int i0 = t.i0; i0 < t.i1; i0 += kOW * kOK) {
    __syncthreads();  // the previous stage is consumed
#pragma unroll
    for (int kk = 0; kk < kOK; ++kk) {
      sa[kk][lane] = va[kk];
      sb[kk][lane] = vb[kk];
    }
    __syncthreads();
    if (i0 + kOW * kOK < t.i1) fetch(i0 + (kOW + wave) * kOK);
#pragma unroll
    for (int kk = 0; kk < kOK; ++kk) {
      double a[kOR], b[kOR];
#pragma unroll
      for (int i = 0; i < kOR; ++i) {
        a[i] = sa[kk][ty * kOR + i];
        b[i] = sb[kk][tx * kOR + i];
      }
#pragma unroll
      for (int i = 0; i < kOR; ++i)
#pragma unroll
        for (int j = 0; j < kOR; ++j) acc[i][j] = fmin(acc[i][j], a[i] + b[j]);
    }
  }
  // the waves' blocks folded pairwise: h = 2, then 1 upper waves hand theirs to the lower ones
  // (a block is 64 x 64 doubles, half of the LDS; value (i, j) of a lane at [(i * 8 + j) * 64 + lane])
  static_assert(kOW == 4 && kOR * kOR * 64 * 2 == kOW * 2 * kOK * kOT, "two register blocks fill the LDS");
#pragma unroll
  for (int h = kOW / 2; h > 0; h >>= 1) {
    __syncthreads();
    if (wave >= h && wave < 2 * h) {
      double* slot = lds + (wave - h) * (kOR * kOR * 64);
#pragma unroll
      for (int i = 0; i < kOR; ++i)
#pragma unroll
        for (int j = 0; j < kOR; ++j) slot[(i * kOR + j) * 64 + lane] = acc[i][j];
    }
    __syncthreads();
    if (wave < h) {
      const double* slot = lds + wave * (kOR * kOR * 64);
#pragma unroll
      for (int i = 0; i < kOR; ++i)
#pragma unroll
        for (int j = 0; j < kOR; ++j) acc[i][j] = fmin(acc[i][j], slot[(i * kOR + j) * 64 + lane]);
    }
  }
  if (wave != 0) return;
#pragma unroll
  for (int i = 0; i < kOR; ++i) {
    const long long r = r0 + ty * kOR + i;
    if (r >= t.r1) continue;
#pragma unroll
    for (int j = 0; j < kOR; ++j) {
      const long long c = c0 + tx * kOR + j;
      if (c >= t.c1) continue;
      if (STEP == 2) out[r * n + c] = acc[i][j];
      out[c * n + r] = acc[i][j];
    }
  }
}

__device__ __forceinline__ bool olo_less(double d, long long i, double bd, long long bi) {
  return d < bd || (d == bd && i < bi);
}

// lexicographic minimum of (d, i) over the workgroup, in every thread (two barriers)
__device__ __forceinline__ void olo_block_min(double& d, long long& i, double* s_d, long long* s_i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double od = __shfl_xor(d, o);
    const long long oi = __shfl_xor(i, o);
    if (olo_less(od, oi, d, i)) {
      d = od;
      i = oi;
    }
  }
  if ((threadIdx.x & 63) == 0) {
    s_d[threadIdx.x >> 6] = d;
    s_i[threadIdx.x >> 6] = i;
  }
  __syncthreads();
  d = s_d[0];
  i = s_i[0];
  for (int w = 1; w < kBW; ++w)
    if (olo_less(s_d[w], s_i[w], d, i)) {
      d = s_d[w];
      i = s_i[w];
    }
  __syncthreads();
}

// The root's end points, first stage: block g's lexicographic minimum of (M(u, w), p(u), p(w))
// over its share of L_root x R_root
__global__ __launch_bounds__(kBT) void k_olo_root(const OloNode* __restrict__ nodes, const double* __restrict__ M,
                                                  int n, double* __restrict__ pd, long long* __restrict__ pi) {
  __shared__ double s_d[kBW];
  __shared__ long long s_i[kBW];
  const OloNode v = nodes[n - 2];
  const long long nl = n, nc = v.hi - v.mid, tot = (long long)(v.mid - v.lo) * nc;
  double bd = INFINITY;
  long long bi = LLONG_MAX;
  for (long long e = (long long)blockIdx.x * kBT + threadIdx.x; e < tot; e += (long long)gridDim.x * kBT) {
    const long long idx = (v.lo + e / nc) * nl + v.mid + e % nc;
    const double c = M[idx];
    if (olo_less(c, idx, bd, bi)) {
      bd = c;
      bi = idx;
    }
  }
  olo_block_min(bd, bi, s_d, s_i);
  if (threadIdx.x == 0) {
    pd[blockIdx.x] = bd;
    pi[blockIdx.x] = bi;
  }
}

// The top-down choice for the nodes of one depth below the root, one workgroup per node (a
// node's end points were written by its parent's launch).  ex, ey: the left-most and right-most
// leaf of a node's final span, as positions (-1 until the parent has chosen); off: the span's
// offset in the final order.  The root (nroot > 0: the number of k_olo_root's partial minima)
// takes its end points from those.  status stays -1, or becomes s >= 0 (node s found no
// candidate; its subtree is left alone) or -2 - s (node s's minimum is not M(a, b)).
__global__ __launch_bounds__(kBT) void k_olo_back(const int* __restrict__ list, int nroot,
                                                  const double* __restrict__ pd, const long long* __restrict__ pi,
                                                  const OloNode* __restrict__ nodes, const int* __restrict__ perm,
                                                  const double* __restrict__ M, const double* __restrict__ D, int n,
                                                  int* ex, int* ey, int* off, int* __restrict__ flip,
                                                  int* __restrict__ order, unsigned long long* status) {
  __shared__ double s_d[kBW];
  __shared__ long long s_i[kBW];
  const int tid = threadIdx.x, s = list[blockIdx.x];
  const long long nl = n;
  const OloNode v = nodes[s];
  int x, y, o;
  if (nroot > 0) {
    double bd = tid < nroot ? pd[tid] : INFINITY;
    long long bi = tid < nroot ? pi[tid] : LLONG_MAX;
    olo_block_min(bd, bi, s_d, s_i);
    if (bi == LLONG_MAX) {
      if (tid == 0) atomicCAS(status, ~0ull, (unsigned long long)s);
      return;
    }
    x = (int)(bi / nl);
    y = (int)(bi % nl);
    o = 0;
  } else {
    x = ex[s];
    y = ey[s];
    o = off[s];
    if (x < 0) return;  // below a node that found no candidate
  }
  const bool flipped = x >= v.mid;
  const long long a = flipped ? y : x, b = flipped ? x : y;
  const int m0 = v.lmid < 0 ? (int)a : a < v.lmid ? v.lmid : v.lo;
  const int m1 = v.lmid < 0 ? (int)a + 1 : a < v.lmid ? v.mid : v.lmid;
  const int k0 = v.rmid < 0 ? (int)b : b < v.rmid ? v.rmid : v.mid;
  const int k1 = v.rmid < 0 ? (int)b + 1 : b < v.rmid ? v.hi : v.rmid;
  const long long nk = k1 - k0, tot = (long long)(m1 - m0) * nk;
  double bd = INFINITY;
  long long bi = LLONG_MAX;
  for (long long e = tid; e < tot; e += kBT) {
    const long long m = m0 + e / nk, k = k0 + e % nk;
    const double c = (M[a * nl + m] + D[m * nl + k]) + M[b * nl + k];
    if (olo_less(c, m * nl + k, bd, bi)) {
      bd = c;
      bi = m * nl + k;
    }
  }
  olo_block_min(bd, bi, s_d, s_i);
  if (tid != 0) return;
  if (bi == LLONG_MAX) {  // every candidate NaN
    atomicCAS(status, ~0ull, (unsigned long long)s);
    return;
  }
  if (!(bd == M[a * nl + b])) atomicCAS(status, ~0ull, (unsigned long long)(-2ll - s));
  const int m = (int)(bi / nl), k = (int)(bi % nl);
  const int nL = v.mid - v.lo, nR = v.hi - v.mid;
  const int oL = flipped ? o + nR : o, oR = flipped ? o : o + nL;
  flip[s] = flipped ? 1 : 0;
  if (v.left >= 0) {
    ex[v.left] = flipped ? m : (int)a;
    ey[v.left] = flipped ? (int)a : m;
    off[v.left] = oL;
  } else {
    order[oL] = perm[v.lo] + 1;
  }
  if (v.right >= 0) {
    ex[v.right] = flipped ? (int)b : k;
    ey[v.right] = flipped ? k : (int)b;
    off[v.right] = oR;
  } else {
    order[oR] = perm[v.mid] + 1;
  }
}

__global__ __launch_bounds__(256) void k_olo_edges(const double* __restrict__ d, long long ld,
                                                   const int* __restrict__ order, int n, double* __restrict__ e) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n - 1) return;
  const int p = order[i] - 1, q = order[i + 1] - 1;
  if ((unsigned)p >= (unsigned)n || (unsigned)q >= (unsigned)n) {  // (a choice that failed left gaps)
    e[i] = NAN;
    return;
  }
  e[i] = d[(p > q ? p : q) + (p > q ? q : p) * ld];
}

struct Plan {
  std::vector<OloNode> nodes;
  std::vector<int> perm;
  std::vector<OloTask> t1, t2;    // step 1 / step 2 products, sorted by level
  std::vector<int> l1, l2, g1, g2;  // per level: first product, tiles (l*: levels + 1 entries)
  std::vector<int> back, boff;      // the steps by depth below the root; per depth the first (depths + 1)
  double candidates = 0;
};

void add_task(std::vector<OloTask>& ts, int& tiles, double& cand, int r0, int r1, int i0, int i1, int c0, int c1) {
  const int ntr = (r1 - r0 + kOT - 1) / kOT, ntc = (c1 - c0 + kOT - 1) / kOT;
  ts.push_back({r0, r1, i0, i1, c0, c1, tiles, ntc});
  tiles += ntr * ntc;
  cand += (double)(r1 - r0) * (double)(i1 - i0) * (double)(c1 - c0);
}

// merge is a valid tree (olo_check_merge)
void make_plan(int n, const int* merge, Plan& P) {
  const int m = n - 1;
  std::vector<int> size(m), level(m);
  int top = 0;
  for (int s = 0; s < m; ++s) {
    size[s] = 0;
    level[s] = 0;
    for (int c = 0; c < 2; ++c) {
      const int v = merge[c * m + s];
      size[s] += v < 0 ? 1 : size[v - 1];
      level[s] = std::max(level[s], v < 0 ? 1 : level[v - 1] + 1);
    }
    top = std::max(top, level[s]);
  }
  P.nodes.assign(m, OloNode{});
  P.perm.assign(n, 0);
  P.nodes[m - 1].lo = 0;
  for (int s = m - 1; s >= 0; --s) {
    OloNode& v = P.nodes[s];
    const int l = merge[s], r = merge[m + s];
    v.mid = v.lo + (l < 0 ? 1 : size[l - 1]);
    v.hi = v.lo + size[s];
    v.left = l < 0 ? -1 : l - 1;
    v.right = r < 0 ? -1 : r - 1;
    if (l < 0) P.perm[v.lo] = -l - 1;
    else P.nodes[l - 1].lo = v.lo;
    if (r < 0) P.perm[v.mid] = -r - 1;
    else P.nodes[r - 1].lo = v.mid;
  }
  for (int s = 0; s < m; ++s) {  // (a child's mid is final once its own turn above has passed)
    OloNode& v = P.nodes[s];
    v.lmid = v.left < 0 ? -1 : P.nodes[v.left].mid;
    v.rmid = v.right < 0 ? -1 : P.nodes[v.right].mid;
  }
  // top-down: depth below the root (a parent's step is the larger one)
  std::vector<int> depth(m, 0);
  int deepest = 0;
  for (int s = m - 1; s >= 0; --s) {
    for (int c : {P.nodes[s].left, P.nodes[s].right})
      if (c >= 0) depth[c] = depth[s] + 1;
    deepest = std::max(deepest, depth[s]);
  }
  P.boff.assign(deepest + 2, 0);
  for (int s = 0; s < m; ++s) ++P.boff[depth[s] + 1];
  for (int dp = 0; dp <= deepest; ++dp) P.boff[dp + 1] += P.boff[dp];
  P.back.assign(m, 0);
  {
    std::vector<int> at(P.boff.begin(), P.boff.end() - 1);
    for (int s = 0; s < m; ++s) P.back[at[depth[s]]++] = s;
  }
  std::vector<int> by_level(m);
  for (int s = 0; s < m; ++s) by_level[s] = s;
  std::stable_sort(by_level.begin(), by_level.end(), [&](int a, int b) { return level[a] < level[b]; });
  int at = 0;
  for (int lv = 1; lv <= top; ++lv) {
    P.l1.push_back((int)P.t1.size());
    P.l2.push_back((int)P.t2.size());
    int n1 = 0, n2 = 0;
    for (; at < m && level[by_level[at]] == lv; ++at) {
      const OloNode& v = P.nodes[by_level[at]];
      if (v.lmid < 0) {
        add_task(P.t1, n1, P.candidates, v.lo, v.mid, v.lo, v.mid, v.mid, v.hi);
      } else {
        add_task(P.t1, n1, P.candidates, v.lo, v.lmid, v.lmid, v.mid, v.mid, v.hi);
        add_task(P.t1, n1, P.candidates, v.lmid, v.mid, v.lo, v.lmid, v.mid, v.hi);
      }
      if (v.rmid < 0) {
        add_task(P.t2, n2, P.candidates, v.lo, v.mid, v.mid, v.hi, v.mid, v.hi);
      } else {
        add_task(P.t2, n2, P.candidates, v.lo, v.mid, v.rmid, v.hi, v.mid, v.rmid);
        add_task(P.t2, n2, P.candidates, v.lo, v.mid, v.mid, v.rmid, v.rmid, v.hi);
      }
    }
    P.g1.push_back(n1);
    P.g2.push_back(n2);
  }
  P.l1.push_back((int)P.t1.size());
  P.l2.push_back((int)P.t2.size());
}

size_t up256(size_t b) { return (b + 255) / 256 * 256; }

}  // namespace

// 0, or the 1-based row that makes merge no tree over n observations (msg says why)
int olo_check_merge(int n, const int* merge, char* msg, size_t cap) {
  const int m = n - 1;
  std::vector<char> obs(n, 0), step(m, 0);
  for (int s = 0; s < m; ++s)
    for (int c = 0; c < 2; ++c) {
      const int v = merge[c * m + s];
      const char* why = nullptr;
      if (v == 0 || v < -n || v > m) why = "is out of range";
      else if (v < 0 && obs[-v - 1]) why = "names an observation that is used twice";
      else if (v - 1 == s) why = "refers to its own step";
      else if (v - 1 > s) why = "uses a step before it exists";
      else if (v > 0 && step[v - 1]) why = "names a step that is used twice";
      if (why) {
        snprintf(msg, cap, "order.optimal: merge is not a tree over %d observations: row %d, column %d (%d) %s", n,
                 s + 1, c + 1, v, why);
        return s + 1;
      }
      (v < 0 ? obs[-v - 1] : step[v - 1]) = 1;
    }
  // 2 (n - 1) entries, all distinct, out of n observations and the n - 2 steps below the last:
  // every observation and every such step is used exactly once
  return 0;
}

// 0 done; 1 an argument error; 2 a HIP error (out of memory included); 3 an internal error.
// stats: launches, candidates.
int olo_solve(hipStream_t st, const double* d_dev, long long ld, int n, const int* merge, int* merge_out,
              int* order_out, double* length, double* stats, char* msg, size_t cap) {
  const int m = n - 1;
  Plan P;
  make_plan(n, merge, P);
  const size_t nn = (size_t)n * n;
  // M, T (transposed), D; then the small arrays
  size_t o = 0;
  auto take = [&](size_t bytes) {
    const size_t at = o;
    o += up256(bytes);
    return at;
  };
  const size_t oM = take(8 * nn), oT = take(8 * nn), oD = take(8 * nn);
  const size_t oE = take(8 * (size_t)m), oFlag = take(16);
  const size_t oN = take(sizeof(OloNode) * m), oT1 = take(sizeof(OloTask) * P.t1.size()),
               oT2 = take(sizeof(OloTask) * P.t2.size());
  const size_t oPerm = take(4 * (size_t)n), oEx = take(4 * (size_t)m), oEy = take(4 * (size_t)m),
               oOff = take(4 * (size_t)m), oFlip = take(4 * (size_t)m), oOrd = take(4 * (size_t)n),
               oBack = take(4 * (size_t)m), oPd = take(8 * kBT), oPi = take(8 * kBT);
  char* ws = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&ws), o) != hipSuccess) {
    (void)hipGetLastError();
    snprintf(msg, cap, "order.optimal: out of memory: the workspace of %d objects needs %zu bytes of device memory",
             n, o);
    return 2;
  }
  double *M = reinterpret_cast<double*>(ws + oM), *T = reinterpret_cast<double*>(ws + oT),
         *D = reinterpret_cast<double*>(ws + oD), *E = reinterpret_cast<double*>(ws + oE);
  unsigned long long* bad = reinterpret_cast<unsigned long long*>(ws + oFlag);
  unsigned long long* status = bad + 1;
  int* back = reinterpret_cast<int*>(ws + oBack);
  double* pd = reinterpret_cast<double*>(ws + oPd);
  long long* pi = reinterpret_cast<long long*>(ws + oPi);
  OloNode* nodes = reinterpret_cast<OloNode*>(ws + oN);
  OloTask *t1 = reinterpret_cast<OloTask*>(ws + oT1), *t2 = reinterpret_cast<OloTask*>(ws + oT2);
  int *perm = reinterpret_cast<int*>(ws + oPerm), *ex = reinterpret_cast<int*>(ws + oEx),
      *ey = reinterpret_cast<int*>(ws + oEy), *off = reinterpret_cast<int*>(ws + oOff),
      *flip = reinterpret_cast<int*>(ws + oFlip), *ord = reinterpret_cast<int*>(ws + oOrd);
  hipError_t e = hipSuccess;
  int rc = 0;
  double launches = 0;
  std::vector<int> hflip(m);
  std::vector<double> he(m);
  unsigned long long hflag[2] = {~0ull, ~0ull};  // no bad pair yet; the choice's status -1
  auto ok = [&](hipError_t r) {
    if (e == hipSuccess) e = r;
    return e == hipSuccess;
  };
  do {
    if (!ok(hipMemcpyAsync(bad, hflag, 16, hipMemcpyHostToDevice, st))) break;
    if (!ok(hipMemcpyAsync(nodes, P.nodes.data(), sizeof(OloNode) * m, hipMemcpyHostToDevice, st))) break;
    if (!ok(hipMemcpyAsync(t1, P.t1.data(), sizeof(OloTask) * P.t1.size(), hipMemcpyHostToDevice, st))) break;
    if (!ok(hipMemcpyAsync(t2, P.t2.data(), sizeof(OloTask) * P.t2.size(), hipMemcpyHostToDevice, st))) break;
    if (!ok(hipMemcpyAsync(perm, P.perm.data(), 4 * (size_t)n, hipMemcpyHostToDevice, st))) break;
    if (!ok(hipMemcpyAsync(back, P.back.data(), 4 * (size_t)m, hipMemcpyHostToDevice, st))) break;
    if (!ok(hipMemsetAsync(ex, 0xff, 4 * (size_t)m, st))) break;  // -1: no end points yet
    if (!ok(hipMemsetAsync(M, 0, 8 * nn, st))) break;  // M(x, x) = 0; the rest is written before it is read
    hipLaunchKernelGGL(k_olo_gather, dim3((unsigned)n, (unsigned)((n + 255) / 256)), dim3(256), 0, st, d_dev, ld,
                       perm, n, D, bad);
    launches += 1;
    if (!ok(hipGetLastError())) break;
    if (!ok(hipMemcpyAsync(hflag, bad, 8, hipMemcpyDeviceToHost, st))) break;
    if (!ok(hipStreamSynchronize(st))) break;
    if (hflag[0] != ~0ull) {
      snprintf(msg, cap, "order.optimal: non-finite distance at row %llu, column %llu (1-based)",
               hflag[0] % (unsigned long long)n + 1, hflag[0] / (unsigned long long)n + 1);
      rc = 1;
      break;
    }
    const int levels = (int)P.g1.size();
    for (int lv = 0; lv < levels && e == hipSuccess; ++lv) {
      hipLaunchKernelGGL(k_olo_minplus<1>, dim3((unsigned)P.g1[lv]), dim3(kOW * 64), 0, st, t1 + P.l1[lv],
                         P.l1[lv + 1] - P.l1[lv], M, D, T, (long long)n);
      hipLaunchKernelGGL(k_olo_minplus<2>, dim3((unsigned)P.g2[lv]), dim3(kOW * 64), 0, st, t2 + P.l2[lv],
                         P.l2[lv + 1] - P.l2[lv], T, M, M, (long long)n);
      launches += 2;
      ok(hipGetLastError());
    }
    if (e != hipSuccess) break;
    const OloNode& rt = P.nodes[m - 1];
    const long long rtot = (long long)(rt.mid - rt.lo) * (rt.hi - rt.mid);
    const int nroot = (int)std::min<long long>(256, std::max<long long>(1, rtot / 16384));
    hipLaunchKernelGGL(k_olo_root, dim3((unsigned)nroot), dim3(kBT), 0, st, nodes, M, n, pd, pi);
    launches += 1;
    for (size_t dp = 0; dp + 1 < P.boff.size(); ++dp) {
      hipLaunchKernelGGL(k_olo_back, dim3((unsigned)(P.boff[dp + 1] - P.boff[dp])), dim3(kBT), 0, st,
                         back + P.boff[dp], dp == 0 ? nroot : 0, pd, pi, nodes, perm, M, D, n, ex, ey, off, flip, ord,
                         status);
      launches += 1;
    }
    hipLaunchKernelGGL(k_olo_edges, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, d_dev, ld, ord, n, E);
    launches += 1;
    if (!ok(hipGetLastError())) break;
    if (!ok(hipMemcpyAsync(&hflag[1], status, 8, hipMemcpyDeviceToHost, st))) break;
    if (!ok(hipMemcpyAsync(hflip.data(), flip, 4 * (size_t)m, hipMemcpyDeviceToHost, st))) break;
    if (!ok(hipMemcpyAsync(order_out, ord, 4 * (size_t)n, hipMemcpyDeviceToHost, st))) break;
    if (!ok(hipMemcpyAsync(he.data(), E, 8 * (size_t)m, hipMemcpyDeviceToHost, st))) break;
    if (!ok(hipStreamSynchronize(st))) break;
  } while (false);
  if (e != hipSuccess) (void)hipStreamSynchronize(st);
  const hipError_t ef = hipFree(ws);
  if (e != hipSuccess || (rc == 0 && ef != hipSuccess)) {
    snprintf(msg, cap, "order.optimal: %s", hipGetErrorString(e != hipSuccess ? e : ef));
    return 2;
  }
  if (rc) return rc;
  const long long hs = (long long)hflag[1];
  if (hs != -1) {
    if (hs >= 0) snprintf(msg, cap, "order.optimal: step %lld has no finite candidate (the sums overflowed)", hs + 1);
    else snprintf(msg, cap, "order.optimal: the minimum at step %lld is not its table entry", -2 - hs + 1);
    return hs >= 0 ? 1 : 3;
  }
  for (int s = 0; s < m; ++s) {
    merge_out[s] = hflip[s] ? merge[m + s] : merge[s];
    merge_out[m + s] = hflip[s] ? merge[s] : merge[m + s];
  }
  if (length) {
    double sum = 0.0;
    for (int i = 0; i < m; ++i) sum += he[i];
    *length = sum;
  }
  if (stats) {
    stats[0] = launches;
    stats[1] = P.candidates;
  }
  return 0;
}

}  // namespace scde
