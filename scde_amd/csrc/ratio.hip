// ratio.hip -- the ratio posterior and its summary, for gfx950 (FP64); on the default path.
//
//   k_ratio_summary   prior-weighted matSlideMult (src/matSlideMult.cpp:5-23; slide_group,
//                     slide_lags) + row normalisation + the lb / mle / ub / ce / Z epilogue
//                     (R/functions.R:3491-3531, 5039-5050), one workgroup per gene
// The launcher follows the kernel.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>

#include "device_math.h"
#include "kernels.h"

namespace scde {

// ------------------------------------------------------------------ K3 helpers
// matSlideMult (src/matSlideMult.cpp:12-20) for R adjacent outputs starting at shift s0:
// X[s] = sum_t A[t + max(s,0)] * B[t + max(-s,0)], t ascending, each product and sum
// rounded separately.  A and B are zero-padded by >= R entries past n, so the R sums can
// all run to the longest one (a padded term adds +0 to a non-negative sum: bit-identical).
// One sliding register window and one shared operand feed R independent sums per step;
// LDS reads are issued 4 steps at a time.
template <int R>
__device__ __forceinline__ void slide_group(const double* __restrict__ A, const double* __restrict__ B, int n,
                                            int s0, double (&c)[R]) {
#pragma unroll
  for (int r = 0; r < R; ++r) c[r] = 0.0;
  double w[R];
  if (s0 >= 0) {
    // output r: sum_{t < n-s0-r} A[t+s0+r] B[t]; longest is r = 0
#pragma unroll
    for (int r = 0; r < R; ++r) w[r] = A[s0 + r];
    const int len = n - s0;
    auto step = [&](double b, double anew) {
#pragma unroll
      for (int r = 0; r < R; ++r) c[r] = __dadd_rn(c[r], __dmul_rn(w[r], b));
#pragma unroll
      for (int r = 0; r + 1 < R; ++r) w[r] = w[r + 1];
      w[R - 1] = anew;
    };
    int t = 0;
    for (; t + 4 <= len; t += 4) {
      const double b0 = B[t], b1 = B[t + 1], b2 = B[t + 2], b3 = B[t + 3];
      const double a0 = A[t + s0 + R], a1 = A[t + s0 + R + 1], a2 = A[t + s0 + R + 2], a3 = A[t + s0 + R + 3];
      step(b0, a0);
      step(b1, a1);
      step(b2, a2);
      step(b3, a3);
    }
    for (; t < len; ++t) step(B[t], A[t + s0 + R]);
  } else if (s0 + R - 1 < 0) {
    // output r: sum_{t < n+s0+r} A[t] B[t-s0-r]; longest is r = R-1
#pragma unroll
    for (int r = 0; r < R; ++r) w[r] = B[-s0 - r];
    const int len = n + s0 + R - 1;
    auto step = [&](double av, double bnew) {
#pragma unroll
      for (int r = 0; r < R; ++r) c[r] = __dadd_rn(c[r], __dmul_rn(av, w[r]));
#pragma unroll
      for (int r = R - 1; r > 0; --r) w[r] = w[r - 1];
      w[0] = bnew;
    };
    int t = 0;
    for (; t + 4 <= len; t += 4) {
      const double a0 = A[t], a1 = A[t + 1], a2 = A[t + 2], a3 = A[t + 3];
      const double b1 = B[t + 1 - s0], b2 = B[t + 2 - s0], b3 = B[t + 3 - s0], b4 = B[t + 4 - s0];
      step(a0, b1);
      step(a1, b2);
      step(a2, b3);
      step(a3, b4);
    }
    for (; t < len; ++t) step(A[t], B[t + 1 - s0]);
  } else {
    // the group that straddles s = 0: one output at a time
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int s = s0 + r;
      const int o1 = s > 0 ? s : 0, o2 = s < 0 ? -s : 0;
      const int len = n - (s < 0 ? -s : s);
      double acc = 0.0;
      for (int t = 0; t < len; ++t) acc = __dadd_rn(acc, __dmul_rn(A[t + o1], B[t + o2]));
      c[r] = acc;
    }
  }
}

// One output, summed over exactly its own n - |s| terms (slide_group's straddling form).  For
// rows with a NaN, an infinity or a negative entry, where a padded term is not +0 (inf * 0 =
// NaN) and so no lag may run past its own length.
__device__ __forceinline__ double slide_one(const double* A, const double* B, int n, int s) {
  const int o1 = s > 0 ? s : 0, o2 = s < 0 ? -s : 0;
  const int len = n - (s < 0 ? -s : s);
  double acc = 0.0;
#pragma unroll 1
  for (int t = 0; t < len; ++t) acc = __dadd_rn(acc, __dmul_rn(A[t + o1], B[t + o2]));
  return acc;
}

// Both sides of the slide in one form: X(d) = sum_t P[t] Q[t + d], t ascending, for R
// adjacent lags d = d0 .. d0+R-1 (s >= 0: P = B, Q = A, d = s; s < 0: P = A, Q = B,
// d = -s), so every lane runs the same instruction stream whichever side its group is on.
// Products are commutative and the terms are summed in the same t order as above:
// bit-identical to slide_group.  Q is zero-padded by >= R past n.
template <int R>
__device__ __forceinline__ void slide_lags(const double* P, const double* Q0, const double* Q1, int n, int d0,
                                           double (&c)[R], int pl = 0, int ph = 1 << 30, int ql = 0,
                                           int qh = 1 << 30) {
  // P is 16-B aligned and t steps by 4: P[t..t+3] is two aligned 16-B reads.  Q0 / Q1 hold
  // the row at an even / odd double offset; the one matching the parity of d0 + R puts
  // Q[t + d0 + R] on a 16-B boundary (ds_read_b128: 16 B per lane in 4 LDS cycles, where
  // ds_read2_b64 takes 16).
  const double* Q = ((d0 + R) & 1) ? Q1 : Q0;
  // Support restriction (bit-identical): a term P[t] Q[t + d] with P[t] == 0 or Q[t + d] ==
  // 0 is +0 (both rows are finite and >= 0; the caller passes full ranges otherwise), and
  // adding +0 to a non-negative partial sum changes nothing, so t only needs to cover
  // [pl, ph] (P nonzero) intersected with the t where some lag's Q[t + d] is nonzero,
  // starting on a multiple of 4 so the aligned reads stay aligned.
  const int tlo = max(max(0, pl), ql - d0 - R + 1);
  const int tend0 = min(min(n - d0, ph + 1), qh - d0 + 1);
  const bool any = tlo < tend0;  // else every term is +0 and so is every sum
  const int t0 = any ? (tlo & ~3) : 0;
  const int tend = any ? tend0 : 0;
  double w[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    c[r] = 0.0;
    w[r] = Q[t0 + d0 + r];
  }
  const int len = tend;
  auto step = [&](double p, double qnew) {
#pragma unroll
    for (int r = 0; r < R; ++r) c[r] = __dadd_rn(c[r], __dmul_rn(w[r], p));
#pragma unroll
    for (int r = 0; r + 1 < R; ++r) w[r] = w[r + 1];
    w[R - 1] = qnew;
  };
  int t = t0;
  for (; t + 4 <= len; t += 4) {
    const double2 pa = *reinterpret_cast<const double2*>(P + t);
    const double2 pb = *reinterpret_cast<const double2*>(P + t + 2);
    const double2 qa = *reinterpret_cast<const double2*>(Q + t + d0 + R);
    const double2 qb = *reinterpret_cast<const double2*>(Q + t + d0 + R + 2);
    step(pa.x, qa.x);
    step(pa.y, qa.y);
    step(pb.x, qb.x);
    step(pb.y, qb.y);
  }
  for (; t < len; ++t) step(P[t], Q[t + d0 + R]);
}

// ------------------------------------------------------------------ K3: ratio posterior + summary
template <int R>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SCDE_RATIO_WPE))) void k_ratio_summary(RatioArgs a) {
  // All LDS is in the dynamic region, every array at a 16-B aligned offset (a static
  // __shared__ in front would shift the base, and misaligned 16-B reads replay):
  //   A, B        the prior-weighted rows at even double offsets, zero-padded to NA >= n + 8
  //               (the sliding windows read past the end; a padded term adds +0 to a
  //               non-negative sum: bit-identical);
  //   A1, B1      the same rows at odd offsets: one of Q / Q1 puts a lane's window on a
  //               16-B boundary, so every slide read is a ds_read_b128;
  //   X           the 2n-1 outputs + 48 doubles of per-wave scratch;
  //   red, red2   8 doubles each; ired, ired2, ired3 8 ints each.
  extern __shared__ __attribute__((aligned(16))) double sh[];
  const int n = a.n, m = 2 * a.n - 1;
  const int NA = (n + 9) & ~1;
  double* A = sh;
  double* B = sh + NA;
  double* A1 = sh + 2 * NA + 1;
  double* B1 = sh + 3 * NA + 1;
  double* X = sh + 4 * NA + 2;
  double* red = X + ((m + 49) & ~1);
  double* red2 = red + 8;
  int* ired = reinterpret_cast<int*>(red2 + 8);
  int* ired2 = ired + 8;
  int* ired3 = ired + 16;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nw = blockDim.x >> 6;
  // Output groups q (R adjacent lags each): s0 = R q - (n-1) >= 0 ("pos": P = B, Q = A),
  // s0 + R - 1 < 0 ("neg": P = A, Q = B), else the one group straddling s = 0.  Each
  // side's groups go to its own waves (the shared operand P[t] is then one address per
  // wave, a broadcast), longest first, so a wave's lanes run similar lengths.
  const int NQ = (m + R - 1) / R;
  const int qpos0 = (n - 1 + R - 1) / R;           // first pos group
  const int NPOS = NQ - qpos0;
  const int NNEG = n > R ? (n - R - 1) / R + 1 : 0;  // groups q < qneg0 with R q + R - 1 < n - 1
  const int NSTR = qpos0 - NNEG;                     // 0 or 1
  int* sup = ired + 24;  // [pl, ph, ql, qh, nonfinite] of the current gene's rows
  for (int g = blockIdx.x; g < a.ngenes; g += gridDim.x) {
    if (tid == 0) {
      sup[0] = 1 << 30;
      sup[1] = -1;
      sup[2] = 1 << 30;
      sup[3] = -1;
      sup[4] = 0;
    }
    __syncthreads();
    for (int k = tid; k < NA && !a.xin; k += blockDim.x) {
      double va = 0.0, vb = 0.0;
      if (k < n) {
        const double y = a.prior_y ? a.prior_y[k] : 1.0;
        const double p1 = a.jp1[(long long)g * a.j1g + (long long)k * a.j1k];
        const double p2 = a.jp2[(long long)g * a.j2g + (long long)k * a.j2k];
        va = a.prior_y ? __dmul_rn(p1, y) : p1;
        vb = a.prior_y ? __dmul_rn(p2, y) : p2;
      }
      A[k] = va;
      B[k] = vb;
      A1[k] = va;
      B1[k] = vb;
      if (k < n) {
        // supports of the two rows (nonzero entries); any non-finite value turns the
        // restriction off (0 * inf is not +0)
        if (va != 0.0) {
          atomicMin(&sup[0], k);
          atomicMax(&sup[1], k);
        }
        if (vb != 0.0) {
          atomicMin(&sup[2], k);
          atomicMax(&sup[3], k);
        }
        if (!isfinite(va) || !isfinite(vb) || va < 0.0 || vb < 0.0) sup[4] = 1;
      }
    }
    __syncthreads();
    int al = 0, ah = 1 << 30, bl = 0, bh = 1 << 30;
    // a row with a NaN, an infinity or a negative entry: every lag over exactly its own terms
    const bool exact = !a.xin && sup[4];
    if (!a.xin && !sup[4]) {
      al = sup[0];
      ah = sup[1];
      bl = sup[2];
      bh = sup[3];
    }
    // matSlideMult (src/matSlideMult.cpp:12-20): X[o] = sum_t A[t + max(s,0)] * B[t + max(-s,0)],
    // s = o - (n-1), t ascending, each product and sum rounded separately.
    dd ls = {0.0, 0.0};
    for (int o = tid; o < m && a.xin; o += blockDim.x) X[o] = a.xin[(long long)g * a.xg + (long long)o * a.xo];
    if (exact && !(SCDE_RATIO_DIAG & 1)) {
      // (block-uniform: sup[] is in LDS) one output per thread, the longest in the middle
      for (int o = tid; o < m; o += blockDim.x) {
        const double v = slide_one(A, B, n, o - (n - 1));
        X[o] = v;
        ls = dd_add_d(ls, v);
      }
    } else if (!a.xin && !(SCDE_RATIO_DIAG & 1)) {
      const int side = nw >= 2 ? (wid & 1) : 0;
      const int wstep = nw >= 2 ? 64 * (nw >> 1) : 64;
      for (int pass = 0; pass < (nw >= 2 ? 1 : 2); ++pass) {
        const int sd = nw >= 2 ? side : pass;
        const int cnt = sd == 0 ? NPOS : NNEG + NSTR;
        for (int i = (nw >= 2 ? (wid >> 1) * 64 : 0) + lane; i < cnt; i += wstep) {
          double c[R];
          if (sd == 0) {  // pos, longest first: q = qpos0 + i, lags d = s0 .. s0 + R - 1
            const int q = qpos0 + i, o0 = R * q, s0 = o0 - (n - 1);
            slide_lags<R>(B, A, A1, n, s0, c, bl, bh, al, ah);
#pragma unroll
            for (int r = 0; r < R; ++r) {
              if (o0 + r < m) {
                X[o0 + r] = c[r];
                ls = dd_add_d(ls, c[r]);
              }
            }
          } else if (i < NNEG) {  // neg, longest first: q = NNEG - 1 - i, lags -s0 - R + 1 ..
            const int q = NNEG - 1 - i, o0 = R * q, s0 = o0 - (n - 1);
            slide_lags<R>(A, B, B1, n, -s0 - R + 1, c, al, ah, bl, bh);
#pragma unroll
            for (int r = 0; r < R; ++r) {
              const int o = o0 + R - 1 - r;
              X[o] = c[r];
              ls = dd_add_d(ls, c[r]);
            }
          } else {  // the group straddling s = 0 (only when (n - 1) % R != 0)
            const int q = NNEG, o0 = R * q;
            slide_group<R>(A, B, n, o0 - (n - 1), c);
#pragma unroll
            for (int r = 0; r < R; ++r) {
              if (o0 + r < m) {
                X[o0 + r] = c[r];
                ls = dd_add_d(ls, c[r]);
              }
            }
          }
        }
      }
    }
    // row sum (R rowSums accumulates in long double): double-double block reduce
    for (int d = 32; d >= 1; d >>= 1) {
      dd o2;
      o2.hi = __shfl_xor(ls.hi, d, 64);
      o2.lo = __shfl_xor(ls.lo, d, 64);
      ls = dd_add(ls, o2);
    }
    if (lane == 0) {
      red[wid] = ls.hi;
      red2[wid] = ls.lo;
    }
    __syncthreads();
    dd tot = {red[0], red2[0]};
    for (int w = 1; w < nw; ++w) tot = dd_add(tot, dd{red[w], red2[w]});
    const bool norm = a.normalize && !a.xin;
    double rs = norm ? dd_to_d(tot) : 1.0;
    __syncthreads();
    if (norm && !isfinite(rs)) {
      // An infinite or NaN output (or an overflowing sum) leaves the double-double sum NaN
      // (inf - inf in its error term), where the reference's long double sum is +-inf unless a
      // NaN or both infinities take part.  A plain sum of the outputs tells the three apart; the
      // order of its terms does not matter to that.  (block-uniform branch: rs is the same in
      // every thread)
      double ps = 0.0;
      for (int o = tid; o < m; o += blockDim.x) ps += X[o];
      for (int d = 32; d >= 1; d >>= 1) ps += __shfl_xor(ps, d, 64);
      if (lane == 0) red[wid] = ps;
      __syncthreads();
      rs = red[0];
      for (int w = 1; w < nw; ++w) rs += red[w];
      __syncthreads();
    }
    for (int o = tid; o < m; o += blockDim.x) {
      const double p = norm ? X[o] / rs : X[o];
      X[o] = p;
      if (a.ratio) a.ratio[(long long)g * a.rg + (long long)o * a.ro] = p;
    }
    __syncthreads();
    if (!a.res || (SCDE_RATIO_DIAG & 2)) continue;
    // ---- quick.distribution.summary: contiguous chunk per thread ----
    const int per = (m + blockDim.x - 1) / blockDim.x;
    const int c0 = tid * per, c1 = min(m, c0 + per);
    dd csum = {0.0, 0.0}, zsum = {0.0, 0.0};
    double bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int o = c0; o < c1; ++o) {
      const double p = X[o];
      csum = dd_add_d(csum, p);
      zsum = dd_add_d(zsum, p + 1e-15);
      if (p > bv) {
        bv = p;
        bi = o;
      }
    }
    // block scan of chunk sums (dd): inclusive within the wave, then exclusive
    dd incl = csum;
    for (int d = 1; d < 64; d <<= 1) {
      dd o2;
      o2.hi = __shfl_up(incl.hi, d, 64);
      o2.lo = __shfl_up(incl.lo, d, 64);
      if (lane >= d) incl = dd_add(o2, incl);
    }
    dd excl;
    excl.hi = __shfl_up(incl.hi, 1, 64);
    excl.lo = __shfl_up(incl.lo, 1, 64);
    if (lane == 0) excl = dd{0.0, 0.0};
    // argmax (first max)
    for (int d = 32; d >= 1; d >>= 1) {
      const double ov = __shfl_xor(bv, d, 64);
      const int oi = __shfl_xor(bi, d, 64);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    // z-sum total
    dd zt = zsum;
    for (int d = 32; d >= 1; d >>= 1) {
      dd o2;
      o2.hi = __shfl_xor(zt.hi, d, 64);
      o2.lo = __shfl_xor(zt.lo, d, 64);
      zt = dd_add(zt, o2);
    }
    __syncthreads();
    if (lane == 63) {
      red[wid] = incl.hi;
      red2[wid] = incl.lo;
    }
    if (lane == 0) {
      ired[wid] = bi;
      X[m + wid] = bv;  // scratch after the row (allocated)
      X[m + 8 + wid] = zt.hi;
      X[m + 16 + wid] = zt.lo;
    }
    __syncthreads();
    dd pre = {0.0, 0.0};
    for (int w = 0; w < wid; ++w) pre = dd_add(pre, dd{red[w], red2[w]});
    dd run = dd_add(pre, excl);
    // walk chunk: lb = last o with cs < 0.025, ub = first o with cs > 0.975
    int lbi = -1, ubi = 0x7fffffff;
    for (int o = c0; o < c1; ++o) {
      run = dd_add_d(run, X[o]);
      const double cs = dd_to_d(run);
      if (cs < 0.025) lbi = o;
      if (cs > (1 - 0.025) && ubi == 0x7fffffff) ubi = o;
    }
    for (int d = 32; d >= 1; d >>= 1) {
      lbi = max(lbi, __shfl_xor(lbi, d, 64));
      ubi = min(ubi, __shfl_xor(ubi, d, 64));
    }
    __syncthreads();
    if (lane == 0) {
      ired2[wid] = lbi;
      ired3[wid] = ubi;
    }
    __syncthreads();
    // Z (R/functions.R:3514-3531): rpost = (p + 1e-15) / rowSums(p + 1e-15);
    // gs = sum(rpost[1:(zi-1)]) (R's 1:0 selects column 1 when zi is the first column),
    // as a block-parallel double-double sum over each thread's chunk.
    dd zt2 = {X[m + 8], X[m + 16]};
    for (int w = 1; w < nw; ++w) zt2 = dd_add(zt2, dd{X[m + 8 + w], X[m + 16 + w]});
    const double rs2 = dd_to_d(zt2);
    const int zend = a.zi == 0 ? 1 : a.zi;
    dd gp = {0.0, 0.0};
    for (int o = c0; o < min(c1, zend); ++o) gp = dd_add_d(gp, (X[o] + 1e-15) / rs2);
    for (int d = 32; d >= 1; d >>= 1) {
      dd o2;
      o2.hi = __shfl_xor(gp.hi, d, 64);
      o2.lo = __shfl_xor(gp.lo, d, 64);
      gp = dd_add(gp, o2);
    }
    if (lane == 0) {
      X[m + 24 + wid] = gp.hi;
      X[m + 32 + wid] = gp.lo;
    }
    __syncthreads();
    if (tid == 0) {
      int lb = ired2[0], ub = ired3[0];
      double mb = X[m];
      int mi = ired[0];
      dd gs = {X[m + 24], X[m + 32]};
      for (int w = 1; w < nw; ++w) {
        lb = max(lb, ired2[w]);
        ub = min(ub, ired3[w]);
        const double v = X[m + w];
        if (v > mb || (v == mb && ired[w] < mi)) {
          mb = v;
          mi = ired[w];
        }
        gs = dd_add(gs, dd{X[m + 24 + w], X[m + 32 + w]});
      }
      if (lb < 0) lb = 0;
      if (ub == 0x7fffffff) ub = m - 1;
      if (mi == 0x7fffffff) mi = 0;
      const double l10_2 = 0.30102999566398119521;
      const double lbv = a.diffv[lb] / l10_2, mlev = a.diffv[mi] / l10_2, ubv = a.diffv[ub] / l10_2;
      double ce = 0.0;
      if (lbv > 0) ce = lbv;
      if (ubv < 0) ce = ubv;
      const double gsd = dd_to_d(gs);
      const double zv = (X[a.zi] + 1e-15) / rs2;
      double zl = qnorm(gsd, false);
      if (zl > 0) zl = 0;
      double zg = qnorm(gsd + zv, false);
      if (zg < 0) zg = 0;
      const double z = (fabs(zl) > fabs(zg)) ? zl : zg;
      const long long N = a.res_ld;
      a.res[g] = lbv;
      a.res[g + N] = mlev;
      a.res[g + 2 * N] = ubv;
      a.res[g + 3 * N] = ce;
      a.res[g + 4 * N] = z;
    }
    __syncthreads();
  }
}

// ================================================================== launchers
namespace {
constexpr size_t kRatioLdsDefault = 64 * 1024;  // what a launch may ask for without opting in
constexpr size_t kRatioLdsMax = 160 * 1024;     // LDS of one gfx950 workgroup
}  // namespace

// the kernel's dynamic LDS (its layout comment): A, B, A1, B1, X + scratch, red, red2, 32 ints
size_t ratio_lds_bytes(int n) {
  const size_t NA = ((size_t)n + 9) & ~(size_t)1;
  return sizeof(double) * (4 * NA + 2 + ((2 * (size_t)n - 1 + 49) & ~(size_t)1) + 16) + sizeof(int) * 32;
}

static int ratio_n_within(size_t bytes) {
  int n = (int)(bytes / (6 * sizeof(double)));  // 6 doubles per point: above the answer
  while (n > 1 && ratio_lds_bytes(n) > bytes) --n;
  return n;
}

int ratio_n_max() { return ratio_n_within(kRatioLdsMax); }

int ratio_n_default_lds() { return ratio_n_within(kRatioLdsDefault); }

hipError_t launch_ratio_summary(const RatioArgs& a, hipStream_t s) {
  if (a.ngenes <= 0) return hipSuccess;
  if (a.n < 1 || a.n > ratio_n_max()) return hipErrorInvalidValue;
  const size_t shm = ratio_lds_bytes(a.n);
  // R = 4: a 4-step unrolled loop rotates the R-wide register window fully (no moves);
  // measured fastest of R = 4, 5, 8 at n = 401, in blocks of 128 threads
  if (shm > kRatioLdsDefault) {
    hipError_t e = hipFuncSetAttribute((const void*)k_ratio_summary<4>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)shm);
    if (e != hipSuccess) return e;
  }
  const int grid = a.ngenes < 65536 ? a.ngenes : 65536;
  hipLaunchKernelGGL(k_ratio_summary<4>, dim3(grid), dim3(128), shm, s, a);
  return hipGetLastError();
}

}  // namespace scde
