// tsne.hip -- exact t-SNE of a precomputed distance matrix (van der Maaten and Hinton 2008, the
// theta = 0 limit of Barnes-Hut t-SNE) into two dimensions, for gfx950.  All FP64.  The contract
// (affinity search, iteration, cost, what is deterministic) is include/scde_hip.h's.
//
//   k_tsne_prep      the caller's strict lower triangle is checked and copied (squared unless it
//                    holds squared distances already) into both triangles of the n x n matrix that
//                    becomes P; the first refused pair goes to a flag the host reads
//   k_tsne_affinity  one workgroup per row: the perplexity search streams the row once per
//                    evaluation; every thread carries the same bisection state (the sums reach all
//                    of them through one fixed lane and wave tree), thread 0 stores beta
//   k_tsne_symm      P_ij = (p_j|i + p_i|j) / 2n in place, tile (a, b) together with tile (b, a)
//   k_tsne_grad      the hot loop.  A block is 64 points i (one per lane) x one chunk of columns
//                    j; the chunk's Y sits in LDS (every lane reads the same entry: a broadcast),
//                    wave w takes the chunk's w-th quarter.  P is symmetric, so the lanes read
//                    P[i + j n]: 512 contiguous bytes per j, and P is read once per iteration.
//                    Per lane five accumulators (A_x, A_y, R_x, R_y, S); the four waves are added
//                    in wave order and the block's partial goes to part[chunk][component][i];
//                    the block's sum of S over its points (a lane tree) goes to bs[chunk][block]
//   k_tsne_update    sumQ from the blocks' sums of S in one fixed tree, per point the partials
//                    added in chunk order, dY, gains, momentum step; the new Y's column sums per
//                    block
//   k_tsne_centre    the column means from the block sums in block order, subtracted
//   k_tsne_rowq, k_tsne_total, k_tsne_cost  the Kullback-Leibler terms per point, one pass over P
//
// No floating-point atomic anywhere: every sum is a loop or tree whose shape depends on n alone,
// so results repeat bit for bit and an iteration does not depend on how many came before it in
// the same call.  The file is built with -ffp-contract=off; the fused operations of the hot loop
// are written as fma().
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "kernels.h"

namespace scde {
namespace {

constexpr int kTile = 32;     // tile edge of k_tsne_prep / k_tsne_symm (blocks of 32 x 8 threads)
constexpr int kRowT = 256;    // threads of the one-workgroup-per-row kernels and the O(n) kernels
constexpr int kRowW = kRowT / 64;
constexpr int kGradRows = 64;   // points per k_tsne_grad block: one per lane
constexpr int kGradWaves = 4;   // each takes a quarter of the block's column chunk
constexpr int kChunkMax = 1024;  // columns per chunk at most (16 KiB of Y in LDS)
constexpr unsigned long long kNoBad = ~0ull;

// the sum of a over the block's kRowT threads, in every thread: lanes by a butterfly (both
// operands of every add are the same two values in either lane, so all lanes hold the same bits),
// then the waves in wave order
__device__ __forceinline__ double block_sum(double a, double* s) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
  __syncthreads();  // s may still be read from the call before
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = a;
  __syncthreads();
  double t = s[0];
#pragma unroll
  for (int w = 1; w < kRowW; ++w) t += s[w];
  return t;
}

// 1 / x for x >= 1: the hardware estimate and one Newton step
__device__ __forceinline__ double recip(double x) {
  const double r = __builtin_amdgcn_rcp(x);
  return fma(r, fma(-x, r, 1.0), r);
}

__global__ __launch_bounds__(kTile * 8) void k_tsne_prep(const double* __restrict__ d, long long ld, int n,
                                                         int squared, double* __restrict__ W,
                                                         unsigned long long* __restrict__ flag) {
  __shared__ double t[kTile][kTile + 1];
  const int a = blockIdx.x, b = blockIdx.y;
  if (a < b) return;
  const int tx = threadIdx.x, ty = threadIdx.y;
  const long long nl = n;
  const int i = a * kTile + tx;
#pragma unroll
  for (int k = 0; k < kTile / 8; ++k) {
    const int c = ty + 8 * k, j = b * kTile + c;
    if (i >= n || j >= n || i < j) continue;
    double x = 0.0;
    if (i > j) {
      const double v = d[i + j * ld];
      x = squared ? v : v * v;
      if (!(v >= 0.0) || !(x < INFINITY)) atomicMin(flag, (unsigned long long)(j * nl + i));
    }
    W[i + j * nl] = x;
    t[c][tx] = x;
  }
  __syncthreads();
  const int iu = b * kTile + tx;  // the mirror image: row in b's range, column in a's
#pragma unroll
  for (int k = 0; k < kTile / 8; ++k) {
    const int r = ty + 8 * k, ju = a * kTile + r;
    if (iu < ju && ju < n) W[iu + ju * nl] = t[tx][r];
  }
}

__global__ __launch_bounds__(kRowT) void k_tsne_affinity(double* __restrict__ W, int n, double log_perp,
                                                         double* __restrict__ beta_out) {
  __shared__ double s_a[kRowW], s_b[kRowW];
  const int i = blockIdx.x, tid = threadIdx.x;
  double* row = W + (long long)i * n;
  double beta = 1.0, lo = -INFINITY, hi = INFINITY, s = 0.0;
  for (int ev = 0;; ++ev) {
    double s0 = 0.0, s1 = 0.0;
#pragma unroll 4
    for (int j = tid; j < n; j += kRowT) {
      const double dd = row[j];
      const double p = j == i ? 0.0 : exp(-beta * dd);
      s0 += p;
      s1 += dd * p;
    }
    s0 = block_sum(s0, s_a);
    s1 = block_sum(s1, s_b);
    s = s0 + DBL_MIN;
    const double delta = beta * s1 / s + log(s) - log_perp;
    if (fabs(delta) < 1e-5 || ev == 199) break;
    if (delta > 0.0) {
      lo = beta;
      beta = hi == INFINITY ? beta * 2.0 : (beta + hi) / 2.0;
    } else {
      hi = beta;
      beta = lo == -INFINITY ? beta / 2.0 : (beta + lo) / 2.0;
    }
  }
  for (int j = tid; j < n; j += kRowT) row[j] = j == i ? 0.0 : exp(-beta * row[j]) / s;
  if (tid == 0) beta_out[i] = beta;
}

__global__ __launch_bounds__(kTile * 8) void k_tsne_symm(double* __restrict__ M, int n) {
  __shared__ double t1[kTile][kTile + 1], t2[kTile][kTile + 1];
  const int a = blockIdx.x, b = blockIdx.y;
  if (a < b) return;
  const int tx = threadIdx.x, ty = threadIdx.y;
  const long long nl = n;
  const double two_n = 2.0 * n;
  const int i1 = a * kTile + tx, i2 = b * kTile + tx;
#pragma unroll
  for (int k = 0; k < kTile / 8; ++k) {
    const int c = ty + 8 * k, j1 = b * kTile + c, j2 = a * kTile + c;
    t1[c][tx] = i1 < n && j1 < n ? M[i1 + j1 * nl] : 0.0;
    t2[c][tx] = i2 < n && j2 < n ? M[i2 + j2 * nl] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < kTile / 8; ++k) {
    const int c = ty + 8 * k, j1 = b * kTile + c, j2 = a * kTile + c;
    if (i1 < n && j1 < n) M[i1 + j1 * nl] = (t1[c][tx] + t2[tx][c]) / two_n;
    if (a != b && i2 < n && j2 < n) M[i2 + j2 * nl] = (t2[c][tx] + t1[tx][c]) / two_n;
  }
}

// part[(chunk * 4 + k) * n + i], k = A_x, A_y, R_x, R_y; bs[chunk * gridDim.x + block] = the block's sum of S
__global__ __launch_bounds__(kGradRows * kGradWaves) void k_tsne_grad(const double* __restrict__ P,
                                                                      const double2* __restrict__ Y, int n,
                                                                      int chunk, double ex,
                                                                      double* __restrict__ part,
                                                                      double* __restrict__ bs) {
  __shared__ double2 sY[kChunkMax];
  __shared__ double red[kGradWaves - 1][5][kGradRows];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i = blockIdx.x * kGradRows + lane;
  const int j0 = blockIdx.y * chunk, j1 = min(n, j0 + chunk);
  for (int t = tid; t < j1 - j0; t += kGradRows * kGradWaves) sY[t] = Y[j0 + t];
  __syncthreads();
  const int per = chunk / kGradWaves;
  const int ja = j0 + wave * per, jb = min(j1, ja + per);
  const int ic = min(i, n - 1);  // lanes past the end compute row n - 1 again and store nothing
  const double2 yi = Y[ic];
  const double* col = P + ic;
  const long long nl = n;
  double ax = 0.0, ay = 0.0, rx = 0.0, ry = 0.0, sq = 0.0;
#pragma unroll 4
  for (int j = ja; j < jb; ++j) {
    const double p = col[j * nl];
    const double2 yj = sY[j - j0];
    const double dx = yi.x - yj.x, dy = yi.y - yj.y;
    const double q = recip(fma(dy, dy, fma(dx, dx, 1.0)));
    const double w = (ex * p) * q;
    ax = fma(w, dx, ax);
    ay = fma(w, dy, ay);
    const double q2 = q * q;
    rx = fma(q2, dx, rx);
    ry = fma(q2, dy, ry);
    sq += j == ic ? 0.0 : q;
  }
  if (wave > 0) {
    double* r = &red[wave - 1][0][lane];
    r[0] = ax;
    r[kGradRows] = ay;
    r[2 * kGradRows] = rx;
    r[3 * kGradRows] = ry;
    r[4 * kGradRows] = sq;
  }
  __syncthreads();
  if (wave != 0) return;
#pragma unroll
  for (int w = 0; w < kGradWaves - 1; ++w) {
    ax += red[w][0][lane];
    ay += red[w][1][lane];
    rx += red[w][2][lane];
    ry += red[w][3][lane];
    sq += red[w][4][lane];
  }
  if (i < n) {
    double* o = part + (long long)blockIdx.y * 4 * nl + i;
    o[0] = ax;
    o[nl] = ay;
    o[2 * nl] = rx;
    o[3 * nl] = ry;
  }
  double t = i < n ? sq : 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) t += __shfl_xor(t, o);
  if (lane == 0) bs[blockIdx.y * gridDim.x + blockIdx.x] = t;
}

__device__ __forceinline__ int sign_of(double x) { return (x > 0.0) - (x < 0.0); }

// sumQ: thread t adds bs[t], bs[t + kRowT], ..., then the block's tree (every block computes the
// same bits).  Y is left uncentred; by[2 * block + c] = the block's sum of the new column c
__global__ __launch_bounds__(kRowT) void k_tsne_update(const double* __restrict__ part, const double* __restrict__ bs,
                                                       int n, int nchunks, int nbs, double eta, double mom,
                                                       double2* __restrict__ Y, double2* __restrict__ uY,
                                                       double2* __restrict__ gains, double* __restrict__ by) {
  __shared__ double s_a[kRowW], s_b[kRowW];
  const int i = blockIdx.x * kRowT + threadIdx.x;
  const long long nl = n;
  double sumq = 0.0;
  for (int b = threadIdx.x; b < nbs; b += kRowT) sumq += bs[b];
  sumq = block_sum(sumq, s_a);
  double2 y = {0.0, 0.0};
  if (i < n) {
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (int c = 0; c < nchunks; ++c)
#pragma unroll
      for (int k = 0; k < 4; ++k) v[k] += part[(c * 4ll + k) * nl + i];
    const double dyv[2] = {v[0] - v[2] / sumq, v[1] - v[3] / sumq};
    const double2 u0 = uY[i], g0 = gains[i];
    y = Y[i];
    double u[2] = {u0.x, u0.y}, g[2] = {g0.x, g0.y}, yy[2] = {y.x, y.y};
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      g[c] = sign_of(dyv[c]) != sign_of(u[c]) ? g[c] + 0.2 : g[c] * 0.8;
      g[c] = fmax(g[c], 0.01);
      u[c] = mom * u[c] - eta * g[c] * dyv[c];
      yy[c] = yy[c] + u[c];
    }
    y = {yy[0], yy[1]};
    Y[i] = y;
    uY[i] = {u[0], u[1]};
    gains[i] = {g[0], g[1]};
  }
  const double tx = block_sum(y.x, s_a), ty = block_sum(y.y, s_b);
  if (threadIdx.x == 0) {
    by[2 * blockIdx.x] = tx;
    by[2 * blockIdx.x + 1] = ty;
  }
}

__global__ __launch_bounds__(kRowT) void k_tsne_centre(const double* __restrict__ by, int n, int nblocks,
                                                       double2* __restrict__ Y) {
  const int i = blockIdx.x * kRowT + threadIdx.x;
  double mx = 0.0, my = 0.0;
  for (int b = 0; b < nblocks; ++b) {
    mx += by[2 * b];
    my += by[2 * b + 1];
  }
  mx = mx / n;
  my = my / n;
  if (i < n) {
    const double2 y = Y[i];
    Y[i] = {y.x - mx, y.y - my};
  }
}

// srow[i] = sum over j != i of Q_ij
__global__ __launch_bounds__(kRowT) void k_tsne_rowq(const double2* __restrict__ Y, int n, double* __restrict__ srow) {
  __shared__ double s_a[kRowW];
  const int i = blockIdx.x;
  const double2 yi = Y[i];
  double s = 0.0;
  for (int j = threadIdx.x; j < n; j += kRowT) {
    const double2 yj = Y[j];
    const double dx = yi.x - yj.x, dy = yi.y - yj.y;
    const double q = recip(fma(dy, dy, fma(dx, dx, 1.0)));
    s += j == i ? 0.0 : q;
  }
  s = block_sum(s, s_a);
  if (threadIdx.x == 0) srow[i] = s;
}

// total[0] = the sum of x[0 .. n): thread t adds x[t], x[t + kRowT], ..., then the block's tree
__global__ __launch_bounds__(kRowT) void k_tsne_total(const double* __restrict__ x, int n, double* __restrict__ total) {
  __shared__ double s_a[kRowW];
  double s = 0.0;
  for (int j = threadIdx.x; j < n; j += kRowT) s += x[j];
  s = block_sum(s, s_a);
  if (threadIdx.x == 0) total[0] = s;
}

__global__ __launch_bounds__(kRowT) void k_tsne_cost(const double* __restrict__ P, const double2* __restrict__ Y, int n,
                                                     const double* __restrict__ total, double* __restrict__ cost) {
  __shared__ double s_a[kRowW];
  const int i = blockIdx.x;
  const double2 yi = Y[i];
  const double sumq = total[0];
  const double* row = P + (long long)i * n;
  double s = 0.0;
  for (int j = threadIdx.x; j < n; j += kRowT) {
    const double2 yj = Y[j];
    const double dx = yi.x - yj.x, dy = yi.y - yj.y;
    const double q = recip(fma(dy, dy, fma(dx, dx, 1.0)));
    const double p = row[j];
    s += j == i ? 0.0 : p * log((p + (double)FLT_MIN) / (q / sumq + (double)FLT_MIN));
  }
  s = block_sum(s, s_a);
  if (threadIdx.x == 0) cost[i] = s;
}

size_t up256(size_t b) { return (b + 255) / 256 * 256; }
int blocks_of(int n) { return (n + kRowT - 1) / kRowT; }

// The workspace: the partials, 3 n doubles for the other stages (the cost's row sums, terms and
// total; the affinities' beta and flag), the gradient blocks' sums of S, the update blocks' sums
// of Y
struct Layout {
  size_t part, comb, bs, by, total;
  explicit Layout(int n) {
    const size_t nn = (size_t)n, nb = (size_t)blocks_of(n), nc = (size_t)tsne_nchunks(n);
    part = 0;
    comb = part + up256(8 * 4 * nn * nc);
    bs = comb + up256(8 * 3 * nn);
    by = bs + up256(8 * nc * (size_t)((n + kGradRows - 1) / kGradRows));
    total = by + up256(16 * nb);
  }
};

bool hip_ok(hipError_t e, char* msg, size_t cap) {
  if (e == hipSuccess) return true;
  snprintf(msg, cap, "tsne: %s", hipGetErrorString(e));
  return false;
}

}  // namespace

// Columns per chunk of k_tsne_grad: a multiple of 64 in [64, kChunkMax] that depends on n alone,
// small enough for some 2,000 blocks where n allows
int tsne_chunk(int n) {
  const int rb = (n + kGradRows - 1) / kGradRows;
  const int want = (2048 + rb - 1) / rb;
  int c = ((n + want - 1) / want + 63) / 64 * 64;
  if (c < 64) c = 64;
  if (c > kChunkMax) c = kChunkMax;
  return c;
}
int tsne_nchunks(int n) { return (n + tsne_chunk(n) - 1) / tsne_chunk(n); }

size_t tsne_ws_bytes(int n) { return Layout(n).total; }

int tsne_affinities(hipStream_t st, const double* d, long long ld, int n, double perplexity, int squared, double* P,
                    double* beta, char* ws, char* msg, size_t cap) {
  const Layout L(n);
  double* beta_dev = reinterpret_cast<double*>(ws + L.comb);
  unsigned long long* flag = reinterpret_cast<unsigned long long*>(beta_dev + n);
  unsigned long long hflag = kNoBad;
  const unsigned nt = (unsigned)((n + kTile - 1) / kTile);
  if (!hip_ok(hipMemcpyAsync(flag, &hflag, 8, hipMemcpyHostToDevice, st), msg, cap)) return 2;
  hipLaunchKernelGGL(k_tsne_prep, dim3(nt, nt), dim3(kTile, 8), 0, st, d, ld, n, squared, P, flag);
  if (!hip_ok(hipGetLastError(), msg, cap)) return 2;
  if (!hip_ok(hipMemcpyAsync(&hflag, flag, 8, hipMemcpyDeviceToHost, st), msg, cap)) return 2;
  if (!hip_ok(hipStreamSynchronize(st), msg, cap)) return 2;
  if (hflag != kNoBad) {
    snprintf(msg, cap, "tsne: the distance at row %llu, column %llu (1-based) is negative or not finite%s",
             hflag % (unsigned long long)n + 1, hflag / (unsigned long long)n + 1,
             squared ? "" : ", or its square is not finite");
    return 1;
  }
  hipLaunchKernelGGL(k_tsne_affinity, dim3((unsigned)n), dim3(kRowT), 0, st, P, n, std::log(perplexity), beta_dev);
  hipLaunchKernelGGL(k_tsne_symm, dim3(nt, nt), dim3(kTile, 8), 0, st, P, n);
  if (!hip_ok(hipGetLastError(), msg, cap)) return 2;
  if (!hip_ok(hipMemcpyAsync(beta, beta_dev, 8 * (size_t)n, hipMemcpyDeviceToHost, st), msg, cap)) return 2;
  if (!hip_ok(hipStreamSynchronize(st), msg, cap)) return 2;
  return 0;
}

int tsne_iterate(hipStream_t st, const double* P, int n, const TsneParams& prm, int iter0, int niter, double* Y,
                 double* uY, double* gains, char* ws, char* msg, size_t cap) {
  const Layout L(n);
  double* part = reinterpret_cast<double*>(ws + L.part);
  double* bs = reinterpret_cast<double*>(ws + L.bs);
  double* by = reinterpret_cast<double*>(ws + L.by);
  const int chunk = tsne_chunk(n), nchunks = tsne_nchunks(n), nb = blocks_of(n);
  const dim3 ggrid((unsigned)((n + kGradRows - 1) / kGradRows), (unsigned)nchunks);
  double2 *Y2 = reinterpret_cast<double2*>(Y), *U2 = reinterpret_cast<double2*>(uY),
          *G2 = reinterpret_cast<double2*>(gains);
  for (int k = 0; k < niter; ++k) {
    const long long t = (long long)iter0 + k;
    const double ex = t <= prm.stop_lying_iter ? prm.exaggeration : 1.0;
    const double mom = t <= prm.mom_switch_iter ? prm.momentum : prm.final_momentum;
    hipLaunchKernelGGL(k_tsne_grad, ggrid, dim3(kGradRows * kGradWaves), 0, st, P, Y2, n, chunk, ex, part, bs);
    hipLaunchKernelGGL(k_tsne_update, dim3((unsigned)nb), dim3(kRowT), 0, st, part, bs, n, nchunks,
                       (int)(ggrid.x * ggrid.y), prm.eta, mom, Y2, U2, G2, by);
    hipLaunchKernelGGL(k_tsne_centre, dim3((unsigned)nb), dim3(kRowT), 0, st, by, n, nb, Y2);
    if ((k & 63) == 63 && !hip_ok(hipGetLastError(), msg, cap)) return 2;
  }
  if (!hip_ok(hipGetLastError(), msg, cap)) return 2;
  if (!hip_ok(hipStreamSynchronize(st), msg, cap)) return 2;
  return 0;
}

int tsne_cost(hipStream_t st, const double* P, int n, const double* Y, double* costs, char* ws, char* msg,
              size_t cap) {
  const Layout L(n);
  double* srow = reinterpret_cast<double*>(ws + L.comb);
  double* cost = srow + n;
  double* total = cost + n;
  const double2* Y2 = reinterpret_cast<const double2*>(Y);
  hipLaunchKernelGGL(k_tsne_rowq, dim3((unsigned)n), dim3(kRowT), 0, st, Y2, n, srow);
  hipLaunchKernelGGL(k_tsne_total, dim3(1), dim3(kRowT), 0, st, srow, n, total);
  hipLaunchKernelGGL(k_tsne_cost, dim3((unsigned)n), dim3(kRowT), 0, st, P, Y2, n, total, cost);
  if (!hip_ok(hipGetLastError(), msg, cap)) return 2;
  if (!hip_ok(hipMemcpyAsync(costs, cost, 8 * (size_t)n, hipMemcpyDeviceToHost, st), msg, cap)) return 2;
  if (!hip_ok(hipStreamSynchronize(st), msg, cap)) return 2;
  return 0;
}

}  // namespace scde
