// kernels.hip -- the two hot kernel families of the scde differential-expression path on gfx950
// (CDNA4, FP64): the posterior tables and the default bootstrap; their launchers are at the end
// of the file.  This file is what remains of the one-file kernel source, on purpose for now:
// unique.hip (unique-count set, ELL rows, gathers), boot.hip (reference-layout bootstrap, exact
// fallback, nboot = 0) and ratio.hip (ratio posterior and summary) were cut out of it; the two
// families below are still to become tables.hip and boot_fast.hip, each a pure move that
// tools/isa_diff.py checks, after which this file is gone.  The cross-lane primitives are
// wave_ops.h's.  See DESIGN.md for the data layout and rooflines.
//
// Tables:
//   k_cell_prep       per-cell grid vectors mu, log cfp, log(1 - cfp), theta, and with a constant
//                     theta p, q, log p, log q (src/jpmatLogBoot.cpp:131-162)            [default]
//   k_col_consts      per-column constants of the constant-theta forms, one lane per column [default]
//   k_tables_lpc      one LANE per column, a block = 64 columns of one cell: column + argmax +
//                     clamp + fused baseline delta + tile / stretch bounds
//                     (src/jpmatLogBoot.cpp:164-210); tables_column_reg is its in-kernel fallback
//                     for the columns outside its form                 [default, phases 0 and 2]
//   k_tables          one wavefront per column, grid vectors from global memory: phase 1 (each
//                     cell's count-0 column), the columns k_tables_lpc leaves (slow_only) and
//                     grids wider than kTabStagedG                           [default, phase 1]
//   k_tables_cell     the cell-staged column-per-wave form: local theta fits (no per-column
//                     constants) at G <= kTabStagedG
//   k_base_cols, k_delta   baseline columns and D = T - T[baseline] as passes of their own (the
//                     default path has both fused into the tables)
//   k_baseline_z, k_stretch_zu   the baseline cells' part of the bootstrap rows / stretch bounds
//   k_ensemble_cols   ensemble: exp(T) / colsum(exp(T))
// Bootstrap over baseline-delta columns (D) and ELL rows:
//   k_mult, k_zero    draw multiplicities per (set, cell, boot)                            [default]
//   k_zuq             the baseline cells' part of the integer tile bounds                  [default]
//   k_boot_gene       the tile bootstrap's first pass: a 4-wave block per (gene, group of slabs),
//                     16 rows of 32 grid points shared by the group's slabs                [default]
//   k_boot_tiles      the list pass behind it: one wave per slab k_boot_gene could not finish,
//                     four bound tiles each                                                [default]
//   k_boot2_list, k_boot2   every grid point of a slab: the fallback of the two above (list form
//                     from 400 cells per call), and with k_stretch_mask the stretch-skipping
//                     bootstrap of calls without tile bounds            [default as the fallback]
//   k_stretch_mask    stretch upper bounds on the FP64 matrix cores, for k_boot2
//   k_sum_partials    the slabs' partial jp rows added in slab order                       [default]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <utility>

#include "device_math.h"
#include "kernels.h"
#include "wave_ops.h"

namespace scde {

// ------------------------------------------------------------------ K0: cell prep
// models: ncells x 12 column-major (R `mm`), columns per src/jpmatLogBoot.cpp:88-99
__global__ __launch_bounds__(256) void k_cell_prep(const double* __restrict__ models, int ncells, int G, int GS,
                                                   const double* __restrict__ mag, int localtheta,
                                                   int squarelogit, double* __restrict__ mu,
                                                   double* __restrict__ lcfp, double* __restrict__ lcfpr,
                                                   double* __restrict__ theta, double* __restrict__ cellscal,
                                                   double* __restrict__ pq, double* __restrict__ cfpo) {
  const int c = blockIdx.x;
  auto M = [&](int col) { return models[(long long)c + (long long)ncells * col]; };
  const double concb = M(0), conca = M(1), failr = M(2), corrb = M(3), corra = M(4), corrt = M(5);
  const double ltb = M(6), ltt = M(7), ltm = M(8), lts = M(9), ltr = M(10), conca2 = M(11);
  double lmax = -INFINITY;
  for (int k = threadIdx.x; k < G; k += blockDim.x) {
    const double m = mag[k];
    const double muk = exp(m * corra + corrb);
    mu[(long long)c * GS + k] = muk;
    double cf = squarelogit ? (conca + m * conca2) * m : m * conca;
    cf += concb;
    cf = 1.0 / (exp(cf) + 1.0);
    const double lc = log(cf);
    lcfpr[(long long)c * GS + k] = log(1.0 - cf);
    lcfp[(long long)c * GS + k] = lc;
    if (cfpo) cfpo[(long long)c * GS + k] = exp(lc);  // the tables kernels' staged cfp (exp of the stored log)
    lmax = gt_max(lmax, lc);
    double th = corrt;
    if (localtheta) {
      double t = -1.0 * m + ltm;
      t *= lts;
      t = pow(10.0, t) + 1.0;
      t = pow(t, ltr);
      t = (ltt - ltb) / t;
      t += ltb;
      t = exp(-1.0 * t);
      if ((!isfinite(t)) || (t < 1.0e-2)) t = 1.0e-2;
      if (t > 1.0e+3) t = 1.0e+3;
      th = t;
    }
    theta[(long long)c * GS + k] = th;
    if (pq) {  // constant theta: the k_tables fast path's per-point terms (prob as k_tables forms it)
      const double pr = th / (th + muk), qr = 1 - pr;
      double* o = pq + (long long)c * 4 * GS + k;
      o[0] = pr;
      o[GS] = qr;
      o[2 * GS] = log(pr);
      o[3 * GS] = log(qr);
    }
  }
  __shared__ double red[16];
  lmax = wave_max(lmax);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = lmax;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m = red[0];
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) m = gt_max(m, red[w]);
    cellscal[2 * c] = m;
    cellscal[2 * c + 1] = exp(failr);
  }
}

// ------------------------------------------------------------------ K1: tables
// One wavefront per (cell, unique count) column; lanes over grid points.  The per-point
// values live in a per-wave LDS row (not a register array), so the grid loops stay rolled:
// one dnbinom body per kernel instead of one per unrolled point (the unrolled form was
// ~12k instructions with lgamma inlined 8x).  CT: theta is the same at every grid point,
// and the (theta, count)-only terms of dnbinom are computed once per column.
// Per-column constants of the constant-theta fast path, one lane per column (k_tables
// would otherwise evaluate them redundantly in all 64 lanes of the column's wave):
// the kColc record (kernels.h).
__global__ __launch_bounds__(256) void k_col_consts(const int* __restrict__ ucl, const long long* __restrict__ ucl_off,
                                                    long long ncols, int ncells, const double* __restrict__ theta,
                                                    int GS, const double* __restrict__ cellscal,
                                                    double* __restrict__ colc, int* __restrict__ slow) {
  const long long col = (long long)blockIdx.x * 256 + threadIdx.x;
  if (col >= ncols) return;
  int lo = 0, hi = ncells;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ucl_off[mid] <= col) lo = mid; else hi = mid;
  }
  const double x = (double)ucl[col];
  const NbConst nc = nb_const(x, theta[(long long)lo * GS]);
  const NbFast f = nb_fast(nc);
  double* o = colc + col * kColc;
  o[0] = f.ok ? f.n : -1.0;
  if (!f.ok) *slow = 1;  // k_tables_lpc (and its fallback) leave this column to the gated k_tables pass
  o[1] = f.nx;
  o[2] = f.S;
  o[3] = f.hlf;
  o[4] = f.lp;
  o[5] = f.lXn;
  o[6] = f.lnxn;
  o[7] = dpois_log(x, cellscal[2 * lo + 1]);
  const double size = theta[(long long)lo * GS], po = size / (size + x);
  o[8] = log(po);
  o[9] = log(1 - po);
  // the closed form's column constant (k_tables_lpc, tables_column_reg): dnbinom(x; size, p) =
  // log(size / (size + x)) + dbinom_raw(size, n, p, q) and, as bd0(y, n r) = y log(y / n) - y log r
  // + n r - y with p + q = 1, dbinom_raw = S - lf / 2 - size log(size / n) - nx log(nx / n)
  // + size log p + nx log q: everything but the last two terms is this constant
  o[10] = f.ok ? ((f.lp + f.S) - f.hlf) - f.X * f.lXn - f.nx * f.lnxn : 0.0;
}

#ifndef SCDE_KT_DIAG
#define SCDE_KT_DIAG 0  // timing-only builds: 1 trivial dnbinom, 2 no exp, 4 no log, 8 no stores, 16 loop 1
                        // only, 32 staging and constants only, 64 no tile bounds
#endif

// One (cell, unique count) column, one wavefront, lanes over grid points.  The per-cell
// grid vectors (mu, pq, lcfpr, lcfp, theta) and the baseline column come in as pointers:
// global memory (k_tables) or an LDS copy staged once per cell (k_tables_cell).

// base_col / zcol hold global column indices; a chunked tables launch (TablesArgs::col_base)
// sees its columns from col_base on as 0, 1, ...
__device__ __forceinline__ int tab_base_col(const TablesArgs& a, int c) {
  const int b = a.base_col[c];
  return b >= 0 ? b - a.col_base : -1;
}
__device__ __forceinline__ int tab_zcol(const TablesArgs& a, int c) {
  const int z = a.zcol[c];
  return z >= 0 ? z - a.col_base : -1;
}

template <bool CT>
__device__ __forceinline__ void tables_column(const TablesArgs& a, long long col, int c, int phase,
                                              const double* __restrict__ mu, const double* __restrict__ P,
                                              const double* __restrict__ lcfpr, const double* __restrict__ lcfp,
                                              const double* __restrict__ cfpl, const unsigned* __restrict__ uqb,
                                              const double* __restrict__ th, const double* __restrict__ base,
                                              double* __restrict__ v,
                                              const double* etab, const LogTab& lt, int lane, int PS) {
  const int G = a.G;
  const double x = (double)a.ucl[col];
  const double maxcfp = a.cellscal[2 * c];
  double fp;
  NbFast nf;
  nf.ok = false;
  if (CT && P && a.colc) {
    // per-column constants from k_col_consts (wave-uniform scalar loads)
    const double* cc = a.colc + col * kColc;
    nf.n = cc[0];
    nf.nx = cc[1];
    nf.S = cc[2];
    nf.hlf = cc[3];
    nf.lp = cc[4];
    nf.lXn = cc[5];
    nf.lnxn = cc[6];
    fp = cc[7];
    nf.X = th[0];
    nf.ok = nf.n > 0.0;  // k_col_consts stores n = -1 where the fast path does not apply
  } else {
    fp = dpois_log_cold(x, a.cellscal[2 * c + 1]);
  }
  double lmax = -INFINITY;
  if (CT && nf.ok) {
    // fast path: per-point p, q, log p, log q from k_cell_prep; the lane whose mu is
    // overridden by the count (R: x between mu[k] and mu[k+1]) forms its own; edge cases
    // (p or q == 0, np or nq not finite and positive) take the reference dnbinom
#pragma unroll 1
    for (int k = lane; k < G; k += 64) {
      const double muv = mu[k];
      const bool last = (k == G - 1);
      const double mnext = last ? 0.0 : mu[k + 1];
      const bool over = (!last && x > muv && x < mnext) || (last && x > muv);
      double pr = P[k], qr = P[PS + k], lpr = P[2 * PS + k], lqr = P[3 * PS + k];
      // wave-uniform branches around the rare lanes: the count's own grid point, and the
      // exact dnbinom (out of line, the reference as written) where the fast form does not apply
      if (__builtin_amdgcn_ballot_w64(over)) {
        const double t = th[k];
        const double po = t / (t + x);
        pr = over ? po : pr;
        qr = over ? 1 - po : qr;
        lpr = over ? log_tab(po, lt) : lpr;
        lqr = over ? log_tab(1 - po, lt) : lqr;
      }
      double nb;
      if (SCDE_KT_DIAG & 1) {  // timing diagnostic: trivial dnbinom
        nb = lpr * x + lqr;
      } else {
        bool bad;
        nb = dnbinom_fast(nf, pr, qr, lpr, lqr, bad);
        if (__builtin_amdgcn_ballot_w64(bad)) {
          if (bad) nb = dnbinom_log_cold(x, th[k], pr);
        }
      }
      nb += lcfpr[k];
      v[k] = nb;
      lmax = gt_max(lmax, nb);
    }
  } else {
    const NbConst nc = CT ? nb_const(x, th[0]) : NbConst{};
#pragma unroll 1
    for (int k = lane; k < G; k += 64) {
      double muv = mu[k];
      const bool last = (k == G - 1);
      const double mnext = last ? 0.0 : mu[k + 1];
      if ((!last && x > muv && x < mnext) || (last && x > muv)) muv = x;
      const double t = th[k];
      double nb = CT ? dnbinom_log_ct(nc, x, t, t / (t + muv), lt) : dnbinom_log(x, t, t / (t + muv));
      nb += lcfpr[k];
      v[k] = nb;
      lmax = gt_max(lmax, nb);
    }
  }
  double maxp = wave_allreduce<true>(lmax);
  if (maxp < (maxcfp + fp)) maxp = maxcfp + fp;
  double ls = 0.0;
  if (cfpl) {
    // the Poisson term exp(lcfp + fp - maxp) as cfp * exp(fp - maxp): cfp = exp(lcfp) per
    // grid point staged with the cell, one exp per column (a few ulps from the quotient form)
    const double d0 = fp - maxp;
    const double E = d0 >= -746.0 ? exp_tab(d0, etab) : 0.0;
#pragma unroll 1
    for (int k = lane; k < G; k += 64) {
      const double d1 = v[k] - maxp;
      const double e = (SCDE_KT_DIAG & 2) ? d1 * 1e-3 + 1.0 : fma(cfpl[k], E, d1 >= -746.0 ? exp_tab(d1, etab) : 0.0);
      v[k] = e;
      ls += e;
    }
  } else {
#pragma unroll 1
    for (int k = lane; k < G; k += 64) {
      // both arguments are <= 0 (maxp bounds them); exp_tab below -746 would underflow anyway
      const double d1 = v[k] - maxp, d2 = lcfp[k] + fp - maxp;
      const double e = (SCDE_KT_DIAG & 2) ? (d1 + d2) * 1e-3 + 1.0
                                          : (d1 >= -746.0 ? exp_tab(d1, etab) : 0.0) + (d2 >= -746.0 ? exp_tab(d2, etab) : 0.0);
      v[k] = e;
      ls += e;
    }
  }
  const double s = wave_allreduce<false>(ls);
  const double lsum = log_tab(s, lt);  // s >= 1 (the maximum term is exp(0))
  double bv = -INFINITY;
  int bi = 0x7fffffff;
  bool clamp = false;
  double* out = a.T ? a.T + col * a.GS : nullptr;
  // fused delta (phase 2): D = T - T[baseline column of the cell], as k_delta computes it
  double* dout = (phase && a.D) ? a.D + col * a.GS : nullptr;
  const int bc_u = (phase == 2) ? tab_base_col(a, c) : -1;
  // per 64-point stretch j (grid points 64j .. 64j+63, one k_boot2 wave each): the
  // column's maximum, for k_boot2's stretch bounds (U: raw maxima for phase-1 columns,
  // maxima minus the cell's baseline-column maxima for phase-2 columns)
  double* const U = a.U;
  const double* ubase = (U && bc_u >= 0) ? U + (long long)bc_u * kStretchSlots : nullptr;
  bool nanq = false;
  // FP64 tile bounds for k_boot_tiles (UQ set, fused phases): per 16-point tile the column's
  // maximum in units of 2^-8, rounded up; phase-2 columns store it minus their baseline
  // column's value (exact integers, so base + delta >= the column's maximum)
  const bool uqf = a.UQ && phase;
#pragma unroll 1
  for (int j = 0; 64 * j < G; ++j) {
    const int k = lane + 64 * j;
    double r = -INFINITY;
    if (k < G) {
      // log(e / s) as log e - log s (no division); e / s could round differently only
      // below DBL_MIN * s, where the reference's quotient is evaluated as written
      const double e = v[k];
      if (SCDE_KT_DIAG & 4) {
        r = e - lsum;
      } else {
        // the quotient path only for waves that have a lane below 2^-960 (high counts at
        // far grid points); a select would evaluate both logs and the division everywhere
        const bool tiny = !(e >= 0x1p-960);
        r = log_tab(tiny ? 1.0 : e, lt) - lsum;
        if (__builtin_amdgcn_ballot_w64(tiny)) {
          const double rq = log_tab(e / s, lt);
          r = tiny ? rq : r;
        }
      }
      if (r > bv) {
        bv = r;
        bi = k;
      }
      const double mlp = a.minlogprob;
      if (r < mlp) {
        r = mlp;
        clamp = true;
      }
      if (SCDE_KT_DIAG & 8) {
        if (r == 12345.0) dout[k] = r;
      } else {
        if (out) out[k] = r;
        if (dout) dout[k] = base ? r - base[k] : r;
      }
      if (U) v[k] = r;  // the row of final values, for the stretch maxima below
      if (uqf && r != r) nanq = true;
    }
    if (uqf) {
      // this chunk's two 32-point bound tiles (two 16-lane rows each): the maximum in units
      // of 2^-8, rounded up, floored at -2^29 (lanes past the grid and NaN lanes hold the
      // floor; ceil and the scaling are monotone, so this is ceil of the tile maximum)
      int u = row16_max_i32((int)ceil(fmax(r * 256.0, -0x1p29)));
      u = max(u, __shfl_xor(u, 16, 64));
      const int t = 2 * j + (lane >> 5);
      if ((lane & 31) == 0) {
        if (kBTile * t >= G)
          u = 0;
        else if (bc_u >= 0)
          u -= unpacku(uqb ? uqb[t] : a.UQ[(long long)bc_u * kQTiles + t]);
        a.UQ[col * kQTiles + t] = packu(u);
      }
    }
  }
  if (uqf) {
    if (__ballot(nanq) && lane == 0) *a.nanflag = 1;
    const int t = 2 * ((G + 63) / 64) + lane;  // tiles past the chunks: 0
    if (t < kQTiles) a.UQ[col * kQTiles + t] = 0u;
  }
  if (U) {
    // per-stretch maxima from the LDS row: lane l < 8 * stretches takes 8 points of
    // stretch l >> 3, then a 3-step max over its group of 8 lanes; in f32, widened by
    // 2^-23 |m| (the f32 rounding of the values) so the stored value is an upper bound
    const int nst = (G + 63) / 64;
    const int j = lane >> 3, k0 = 64 * j + 8 * (lane & 7);
    float mf = -INFINITY;
    if (j < nst)
      for (int t = 0; t < 8; ++t)
        if (k0 + t < G) mf = gt_maxf(mf, (float)v[k0 + t]);
#pragma unroll
    for (int o = 1; o <= 4; o <<= 1) mf = gt_maxf(mf, __shfl_xor(mf, o, 64));
    if ((lane & 7) == 0 && j < nst) {
      const double m = (double)mf + 0x1p-23 * fabs((double)mf);
      U[col * kStretchSlots + j] = ubase ? m - ubase[j] : m;
    }
  }
  if (dout)
    for (int k = G + lane; k < a.GS; k += 64) dout[k] = 0.0;
  if (a.maxi) {
    // first maximum over the grid (Armadillo max(index), strict '>')
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double ov = __shfl_xor(bv, m, 64);
      const int oi = __shfl_xor(bi, m, 64);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == 0) a.maxi[col] = (bi == 0x7fffffff) ? 0 : bi;
  }
  const unsigned long long anyc = __ballot(clamp);
  if (lane == 0) a.has_clamp[col] = anyc ? 1 : 0;
  if (phase == 1 && lane == 0) a.base_col[c] = (a.use_baseline && !anyc) ? (int)col + a.col_base : -1;
}

__device__ __forceinline__ void tables_tabs(double* etab, double (*ltab)[97]) {
  if (threadIdx.x < 64) etab[threadIdx.x] = kExp2Frac64[threadIdx.x];
  if (threadIdx.x < 97) {
    ltab[0][threadIdx.x] = kLogInvC[threadIdx.x];
    ltab[1][threadIdx.x] = kLogCHi[threadIdx.x];
    ltab[2][threadIdx.x] = kLogCLo[threadIdx.x];
  }
}

// Column-per-wave form, grid vectors read from global memory: phase 1 (one wave per
// cell, its count-0 column) and grids too wide for the staged kernel.
template <bool CT>
__global__ __launch_bounds__(256) void k_tables(TablesArgs a) {
  extern __shared__ double vrow[];  // [4 waves][GS]
  __shared__ double etab[64];
  __shared__ double ltab[3][97];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  tables_tabs(etab, ltab);
  __syncthreads();
  const LogTab lt{ltab[0], ltab[1], ltab[2]};
  if (a.gate && *a.gate == 0) return;
  if (a.slow_only && *reinterpret_cast<const int*>(a.colc + kColc * a.ncols) == 0) return;
  const int phase = a.phase;
  long long col;
  int c;
  if (phase == 1) {
    // one wave per cell: its count-0 column (unique within the cell), first match
    c = blockIdx.x * 4 + wid;
    if (c >= a.ncells) return;
    const long long o1 = a.ucl_off[c + 1];
    long long zc = -1;
    for (long long i0 = a.ucl_off[c]; i0 < o1; i0 += 64) {
      const long long i = i0 + lane;
      const unsigned long long m = __ballot(i < o1 && a.ucl[i] == 0);
      if (m) {
        zc = i0 + __ffsll((long long)m) - 1;
        break;
      }
    }
    if (lane == 0) a.zcol[c] = zc >= 0 ? (int)zc + a.col_base : -1;
    if (zc < 0) {
      if (lane == 0) a.base_col[c] = -1;
      return;
    }
    col = zc;
  } else {
    col = (long long)blockIdx.x * 4 + wid;
    if (a.slow_only) {
      // the columns k_tables_lpc left (colc n < 0): 64 candidates per wave step, grid-stride
      for (long long b0 = col * 64; b0 < a.ncols; b0 += (long long)gridDim.x * 4 * 64) {
        const long long ci = b0 + lane;
        unsigned long long m = __ballot(ci < a.ncols && !(a.colc[ci * kColc] > 0.0));
        while (m) {
          const long long cs = b0 + __ffsll((long long)m) - 1;
          m &= m - 1;
          int lo = 0, hi = a.ncells;
          while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (a.ucl_off[mid] <= cs) lo = mid; else hi = mid;
          }
          if (phase == 2 && cs == tab_zcol(a, lo)) continue;  // done in phase 1
          const long long co = (long long)lo * a.GS;
          const int bc = (phase == 2) ? tab_base_col(a, lo) : -1;
          const double* base = (bc >= 0 && a.D) ? a.D + (long long)bc * a.GS : nullptr;
          tables_column<CT>(a, cs, lo, phase, a.mu + co, (CT && a.pq) ? a.pq + 4 * co : nullptr, a.lcfpr + co,
                            a.lcfp + co, nullptr, nullptr, a.theta + co, base, vrow + (long long)wid * a.GS, etab,
                            lt, lane, a.GS);
        }
      }
      return;
    }
    if (phase == 2 && col == a.ncols) {  // the ELL pad column
      for (int k = lane; k < a.GS; k += 64)
        if (a.D) a.D[col * a.GS + k] = 0.0;
      if (a.U && lane < kStretchSlots) a.U[col * kStretchSlots + lane] = 0.0;
      if (a.UQ && lane < kQTiles) a.UQ[col * kQTiles + lane] = 0u;
      return;
    }
    if (col >= a.ncols) return;
    int lo = 0, hi = a.ncells;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (a.ucl_off[mid] <= col) lo = mid; else hi = mid;
    }
    c = lo;
    if (phase == 2 && col == tab_zcol(a, c)) return;  // done in phase 1
  }
  const long long co = (long long)c * a.GS;
  const int bc = (phase == 2) ? tab_base_col(a, c) : -1;
  const double* base = (bc >= 0 && a.D) ? a.D + (long long)bc * a.GS : nullptr;
  tables_column<CT>(a, col, c, phase, a.mu + co, (CT && a.pq) ? a.pq + 4 * co : nullptr, a.lcfpr + co,
                    a.lcfp + co, nullptr, nullptr, a.theta + co, base, vrow + (long long)wid * a.GS, etab, lt, lane,
                    a.GS);
}

// Cell-staged form (phases 0 and 2, G <= kTabStagedG): one 8-wave block per task
// (cell c, columns [b, e)), the cell's grid vectors and baseline column copied into LDS
// once and shared by the block's waves, which take the task's columns round-robin.
// Without the staging every column's wave re-reads ~9 grid vectors from L2 with a
// dependent-load latency per 64-point step.  LDS rows have stride G (not GS) so two
// blocks fit a CU: (8 + 9) * G * 8 B = 54.5 KB at G = 401.
constexpr int kTabStagedG = 448;
constexpr int kTabWaves = 8;
template <bool CT>
__global__ __launch_bounds__(64 * kTabWaves) __attribute__((amdgpu_waves_per_eu(SCDE_TAB_WPE))) void k_tables_cell(TablesArgs a) {
  extern __shared__ double dyn[];  // vrow [8][G] | mu | P[4] | lcfpr | cfp | th | base, each G
  __shared__ double etab[64];
  __shared__ unsigned suqb[kQTiles];  // the baseline column's tile bounds (phase 2)
  __shared__ double ltab[3][97];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int GS = a.GS, G = a.G;
  tables_tabs(etab, ltab);
  if (a.gate && *a.gate == 0) return;
  const int4 task = a.tasks[blockIdx.x];
  const int c = task.x;
  const int phase = a.phase;
  if (c < 0) {  // the ELL pad column (phase 2)
    if (wid == 0) {
      for (int k = lane; k < GS; k += 64)
        if (a.D) a.D[a.ncols * GS + k] = 0.0;
      if (a.U && lane < kStretchSlots) a.U[a.ncols * kStretchSlots + lane] = 0.0;
      if (a.UQ && lane < kQTiles) a.UQ[a.ncols * kQTiles + lane] = 0u;
    }
    return;
  }
  const bool haveP = CT && a.pq;
  double* smu = dyn + kTabWaves * G;
  double* sP = smu + G;
  double* slr = sP + 4 * G;
  double* slc = slr + G;
  double* sth = slc + G;
  double* sbase = sth + G;
  const long long co = (long long)c * GS;
  const int bc = (phase == 2) ? tab_base_col(a, c) : -1;
  if (bc >= 0 && a.UQ && threadIdx.x < kQTiles) suqb[threadIdx.x] = a.UQ[(long long)bc * kQTiles + threadIdx.x];
  for (int k = threadIdx.x; k < G; k += 64 * kTabWaves) {
    smu[k] = a.mu[co + k];
    slr[k] = a.lcfpr[co + k];
    slc[k] = exp(a.lcfp[co + k]);  // cfp, linear (tables_column's one-exp normalisation)
    sth[k] = a.theta[co + k];
    if (haveP) {
      const double* P = a.pq + 4 * co;
      sP[k] = P[k];
      sP[G + k] = P[GS + k];
      sP[2 * G + k] = P[2 * GS + k];
      sP[3 * G + k] = P[3 * GS + k];
    }
    if (bc >= 0) sbase[k] = a.D[(long long)bc * GS + k];
  }
  __syncthreads();
  const LogTab lt{ltab[0], ltab[1], ltab[2]};
  const int zc = (phase == 2) ? tab_zcol(a, c) : -1;
  for (int col = task.y + wid; col < task.z; col += kTabWaves) {
    if (col == zc) continue;  // done in phase 1
    tables_column<CT>(a, col, c, phase, smu, haveP ? sP : nullptr, slr, nullptr, slc, (bc >= 0) ? suqb : nullptr, sth,
                      (bc >= 0) ? sbase : nullptr, dyn + wid * G, etab, lt, lane, G);
  }
}

// tables_column_reg: the general register-row column (one wave per column; k_tables_lpc's fallback
// for the columns outside its form): a column's 401 grid values stay in seven VGPR pairs through
// the three passes (dnbinom + max, exp + sum, log + stores + tile maxima), the chunk loops
// unrolled so the LDS reads of different chunks overlap.  The NB log-pmf is the closed form (the
// only form: it has no lanes that need the exact dnbinom).  Columns whose constants rule out the
// form (colc n < 0) are left to the gated k_tables pass.
constexpr int kTabChunks = kTabStagedG / 64;

// The staged rows have the fixed stride kTabStagedG (entries G.. are zero pads), so every
// LDS read is lane * 8 plus an immediate offset: no per-chunk address registers (the
// compiler would hoist ~8 per chunk out of the column loop and spill them).
constexpr int kRS = kTabStagedG;
// the closed form reads log p, log q only: seven staged rows (four blocks of 4 waves per CU)
enum { kRowMu = 0, kRowLP = 1, kRowLQ = 2, kRowLcfpr = 3, kRowCfp = 4, kRowLcfp = 5, kRowBase = 6, kTabRegRows = 7 };

// Per grid point k of a column, in log space relative to maxp: t1 = nb_k + log(1 - cfp_k)
// - maxp (the NB term) and t2 = log cfp_k + fp - maxp (the Poisson term); the reference's
// e_k = exp(t1) + exp(t2), s = sum e_k, T_k = log(e_k / s) (src/jpmatLogBoot.cpp:191-193).
//   - the sum: exp(t1) only in chunks with a lane above t1 = -60 (smaller terms are below
//     2^-86 of s >= 1 and do not reach its rounding); exp(t2) = cfp_k exp(fp - maxp);
//   - T_k where one term exceeds the other by e^37.5 (log1p of the ratio < 5e-17):
//     max(t1, t2) - log s, no exp or log per point;
//   - T_k where neither dominates: log(exp(t1) + exp(t2)) - log s (table exp and log), only
//     in chunks that have such a lane;
//   - T_k where max(t1, t2) < -665 (e_k below 2^-960, subnormal ranges): the quotient
//     log(e_k / s) as the reference forms it.
enum { kBoundNone = 0, kBoundTiles = 1, kBoundStretch = 2 };  // the tables kernels' bound output
// GC: the grid length as a compile-time constant (401, the default prior grid), so the
// chunk masks fold away; 0 = a.G at run time
// The tables kernels' T/D rows as non-temporal stores when a.nt_rows (option tables_nt): 1.8 GB per
// config-3 step, read back by the bootstrap long after the caches have turned over (A/B: config 3
// faster in 7 of 9 alternating pairs, at the box-noise level).  Smaller calls keep
// plain stores (engine: rows that fit the last-level cache).  nt is kernel-uniform.
__device__ __forceinline__ void tab_store(double* p, double v, int nt) {
  if (nt)
    __builtin_nontemporal_store(v, p);
  else
    *p = v;
}
typedef double tab_v2d __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void tab_store2(double* p, double a, double b, int nt) {  // p 16-byte aligned
  tab_v2d v;
  v.x = a;
  v.y = b;
  if (nt)
    __builtin_nontemporal_store(v, reinterpret_cast<tab_v2d*>(p));
  else
    *reinterpret_cast<tab_v2d*>(p) = v;
}

template <int BM, int GC>
__device__ __forceinline__ void tables_column_reg(const TablesArgs& a, long long col, int c, int phase,
                                                  const double* __restrict__ sm, bool have_base,
                                                  const unsigned* __restrict__ uqb, const double* etab,
                                                  const LogTab& lt, int lane, double theta, const double* cc,
                                                  double x, double maxcfp, int bc_u) {
  const int G = GC ? GC : a.G;
  if (!(cc[0] > 0.0)) return;  // the gated k_tables pass takes this column
  const double fp = cc[7];
  const double lpo = cc[8], lqo = cc[9];
  const double po = theta / (theta + x);  // the count's own grid point
  if (SCDE_KT_DIAG & 32) {  // timing diagnostic: staging and constants only
    if (po == 12345.0) a.has_clamp[col] = 1;
    return;
  }
  const double* sl = sm + lane;
  double v[kTabChunks];
  double lmax = -INFINITY;
#pragma unroll
  for (int j = 0; j < kTabChunks; ++j) {
    v[j] = -INFINITY;
    if (64 * j < G) {
      const int k = lane + 64 * j;
      const bool in = k < G;
      const bool last = (k == G - 1);
      double lpr = sl[kRowLP * kRS + 64 * j], lqr = sl[kRowLQ * kRS + 64 * j];
      const double muv = sl[kRowMu * kRS + 64 * j], mnext = sl[kRowMu * kRS + 64 * j + 1];
      const bool over = in && ((!last && x > muv && x < mnext) || (last && x > muv));
      if (__builtin_amdgcn_ballot_w64(over)) {
        lpr = over ? lpo : lpr;
        lqr = over ? lqo : lqr;
      }
      // log dnbinom(x; size, p_k) = C + size log p_k + x log q_k (C: the column constant;
      // count 0: size log p_k, as the x == n branch of dbinom_raw).  p_k, q_k are the same
      // rounded values the saddle-point form takes, log p_k and log q_k the staged logs;
      // q_k = 0 (grid point 0) gives -inf for x > 0 and 0 for x = 0, as dbinom_raw.  Against
      // the saddle-point form the difference is below 2e-11 absolute at counts of 5,000 and
      // means of 10^5 (log space), far under the 1e-6 parity bar.
      double nb = (x == 0.0) ? theta * lpr : fma(x, lqr, fma(theta, lpr, cc[10]));
      nb += sl[kRowLcfpr * kRS + 64 * j];
      v[j] = in ? nb : -INFINITY;
      lmax = gt_max(lmax, v[j]);
    }
  }
  if (SCDE_KT_DIAG & 16) {  // timing diagnostic: loop 1 only
    if (lmax == 12345.0) a.has_clamp[col] = 1;
    return;
  }
  double maxp = wave_allreduce<true>(lmax);
  if (maxp < (maxcfp + fp)) maxp = maxcfp + fp;
  const double d0 = fp - maxp;
  const double E = exp_tab(fmax(d0, -746.0), etab);  // exp(fp - maxp); 0 below -746 (and for NaN)
  double ls = 0.0;
#pragma unroll
  for (int j = 0; j < kTabChunks; ++j) {
    if (64 * j < G) {
      const int k = lane + 64 * j;
      const bool in = k < G;
      v[j] -= maxp;  // t1
      double e = sl[kRowCfp * kRS + 64 * j] * E;
      if (!(SCDE_KT_DIAG & 2) && __builtin_amdgcn_ballot_w64(in && v[j] > -60.0)) e += exp_tab(fmax(v[j], -746.0), etab);
      ls += in ? e : 0.0;
    }
  }
  const double s = wave_allreduce<false>(ls);
  const double lsum = log_tab(s, lt);  // s >= 1 (the maximum term is exp(0))
  const bool want_maxi = a.maxi != nullptr;
  double bv = -INFINITY;
  int bi = 0x7fffffff;
  bool clamp = false, nanq = false;
  double* out = a.T ? a.T + col * a.GS : nullptr;
  double* dout = (phase && a.D) ? a.D + col * a.GS : nullptr;
  const double minlp = a.minlogprob;
  unsigned uqv = 0;  // lane t < kQTiles: bound tile t's value (BM == kBoundTiles)
#pragma unroll
  for (int j = 0; j < kTabChunks; ++j) {
    if (64 * j < G) {
      const int k = lane + 64 * j;
      const bool in = k < G;
      const double t1 = v[j], t2 = sl[kRowLcfp * kRS + 64 * j] + d0;
      const double hi = gt_max(t2, t1), lo = (t1 > t2) ? t2 : t1;
      const bool tiny = !(hi >= -665.0);
      const bool mixed = !tiny && !(hi - lo > 37.5);
      double r = hi - lsum;
      if (__builtin_amdgcn_ballot_w64(in && (tiny || mixed))) {
        double e = fma(sl[kRowCfp * kRS + 64 * j], E, exp_tab(fmax(t1, -746.0), etab));
        if (__builtin_amdgcn_ballot_w64(in && tiny)) {
          // subnormal range: the Poisson term as the reference forms it, exp(log cfp_k + fp - maxp),
          // rounded once -- cfp_k E would carry the few bits a subnormal E has left
          const double et = exp_tab(fmax((sl[kRowLcfp * kRS + 64 * j] + fp) - maxp, -746.0), etab) +
                            exp_tab(fmax(t1, -746.0), etab);
          e = tiny ? et : e;
        }
        const double rm = (SCDE_KT_DIAG & 4) ? e - lsum : log_tab(tiny ? e / s : e, lt) - (tiny ? 0.0 : lsum);
        r = (tiny || mixed) ? rm : r;
      }
      if (want_maxi && r > bv && in) {
        bv = r;
        bi = k;
      }
      const bool cl = r < minlp;
      r = cl ? minlp : r;
      clamp = clamp || (cl && in);
      nanq = nanq || (in && r != r);
      // unconditional stores: lanes past the grid write the pad zeros (k < GS always)
      if (!(SCDE_KT_DIAG & 8)) {
        if (out) tab_store(out + k, in ? r : 0.0, a.nt_rows);
        if (dout) tab_store(dout + k, in ? (have_base ? r - sl[kRowBase * kRS + 64 * j] : r) : 0.0, a.nt_rows);
      } else if (r == 12345.0) {
        dout[k] = r;
      }
      r = in ? r : -INFINITY;
      if (BM == kBoundTiles && !(SCDE_KT_DIAG & 64)) {
        // this chunk's two 32-point bound tiles (rows 0-1 and 2-3; row maxima rounded up to
        // 2^-8, floor -2^29): lanes 2j, 2j + 1 collect both rows of their tile (lanes 32 i,
        // 32 i + 16) and keep the larger
        int u = row16_max_i32((int)ceil(fmax(r * 256.0, -0x1p29)));
        const auto sw = __builtin_amdgcn_permlane16_swap((unsigned)u, (unsigned)u, false, false);
        u = max((int)sw[0], (int)sw[1]);  // rows 0-1 | rows 2-3: the bound tile's maximum on every lane
        const int g = __builtin_amdgcn_ds_bpermute(((lane - 2 * j) & 1) << 7, u);
        uqv = ((lane >> 1) == j) ? (unsigned)g : uqv;
      }
      if (BM == kBoundStretch) {  // the stretch maximum (64 points = this chunk), f32 widened
        const float mf = wave_maxf((float)r);
        if (lane == 0) {
          const double m = (double)mf + 0x1p-23 * fabs((double)mf);
          a.U[col * kStretchSlots + j] = (bc_u >= 0) ? m - a.U[(long long)bc_u * kStretchSlots + j] : m;
        }
      }
    }
  }
  if (BM == kBoundTiles) {
    if (__ballot(nanq) && lane == 0) *a.nanflag = 1;
    if (lane < kQTiles) {
      int u = (int)uqv;
      if (kBTile * lane >= G)
        u = 0;
      else if (bc_u >= 0)
        u -= unpacku(uqb[lane]);
      a.UQ[col * kQTiles + lane] = packu(u);
    }
  }
  if (dout)
    for (int k = 64 * ((G + 63) / 64) + lane; k < a.GS; k += 64) dout[k] = 0.0;
  if (want_maxi) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double ov = __shfl_xor(bv, m, 64);
      const int oi = __shfl_xor(bi, m, 64);
      if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
      }
    }
    if (lane == 0) a.maxi[col] = (bi == 0x7fffffff) ? 0 : bi;
  }
  const unsigned long long anyc = __ballot(clamp);
  if (lane == 0) a.has_clamp[col] = anyc ? 1 : 0;
}

// ------------------------------------------------------------------ lane-per-column tables (round 6)
// k_tables_lpc<BM>: the constant-theta FP64 tables (phases 0 and 2, G <= kTabStagedG) with one LANE
// per (cell, unique count) column.  A block takes 64 columns of one cell; its 4 waves split the grid
// into four ranges of ~G/4 points (multiples of kLpcFlush), and each lane walks its column's points
// of the wave's range in order -- so the grid vectors a point needs are the same for the whole wave
// (LDS broadcast reads), the column's maximum and normaliser are one running max / sum per lane
// (four partials per column combined in LDS, in wave order), and the tile and stretch bounds are
// running maxima.  No cross-lane reduction, ballot or per-chunk branch in the hot loops; the loop
// bodies are short (the register-row form (k_tables_reg, round 5) spent most of its time in instruction supply and
// dependency chains: timing builds without its exps or its mixed branch ran 30% faster each though
// the branch runs on 1.5% of the points).  Rows go out through a per-wave LDS transpose, kLpcFlush
// points of 64 columns at a time, as 16-byte stores (64 contiguous bytes per column).
// Per point (src/jpmatLogBoot.cpp:166-206): nb_k = x log q_k + (theta log p_k + log(1 - cfp_k)) + C
// (the closed-form NB log-pmf, section 4.0d; the parenthesis staged per cell), mu' override at the one
// point ks where mu_ks < x < mu_ks+1 (mu nondecreasing, checked per cell), maxp, the normaliser
// s = sum_k (cfp_k exp(fp - maxp) + exp(nb_k - maxp)) in grid order, T_k = max(t1, t2) - log s where
// one term exceeds the other by e^37.5, else log(e_k) - log s, and log(e_k / s) where both terms are
// below e^-665 (the reference's quotient in the subnormal range); clamp at minlogprob.  Columns
// outside this form (count 0, flagged constants, a non-finite maxp, cells with a decreasing mu or a
// NaN / +inf staged value) go through tables_column_reg after the block's lane pass.
#ifndef SCDE_LPC_DIAG
#define SCDE_LPC_DIAG 0  // study builds of k_tables_lpc: 1 no row stores, 2 no pass-2 exps, 4 no mixed points, 8 NaN in [GP, GS)
#endif
// Settled by measurement: the exps go through the 64-entry LDS table (a
// table-free polynomial exp: 0.311 vs 0.300 ms per launch); the rows go out through a per-wave LDS
// transpose (each lane storing its own column: 5 blocks per CU instead of 3, but 0.342 vs 0.306 ms
// per launch at config 3); the log tables are read from global memory, not staged in LDS.
#ifndef LPC_U12
#define LPC_U12 4  // k_tables_lpc: unroll of passes 1 and 2
#endif
#ifndef LPC_U3
#define LPC_U3 8  // k_tables_lpc: unroll of pass 3's flush group
#endif
constexpr int kLpcWaves = 4;
constexpr int kLpcFlush = 8;              // points per register group (and per transposed flush)
constexpr int kLpcTS = kLpcFlush + 1;     // the transpose's row stride (doubles) per column
constexpr int kLpcQB = 0;                 // (log q_k, theta log p_k + log(1 - cfp_k)) pairs
constexpr int kLpcLC = 2 * kTabStagedG;   // (log cfp_k, cfp_k) pairs
constexpr int kLpcBase = 4 * kTabStagedG; // the baseline column (phase 2; 0 past the grid)
constexpr int kLpcR = 5 * kTabStagedG;    // region R: mu_k (the override search), then the passes'
constexpr int kLpcMu = kLpcR;             // partial maxima / sums, then the transposes
constexpr int kLpcPart = kLpcR + kTabStagedG;
constexpr int kLpcRsz = kLpcWaves * 64 * kLpcTS;
constexpr int kLpcLds0 = kLpcR + kLpcRsz;
constexpr int kLpcLds = kLpcLds0 > kTabRegRows * kRS ? kLpcLds0 : kTabRegRows * kRS;  // (the fallback's rows overlay it)
static_assert(kLpcRsz >= kTabStagedG + kLpcWaves * 64, "mu and the partials fit region R");
static_assert(kLpcWaves * 64 * 3 <= kLpcBase, "the combine's arrays overlay the staged rows");
static_assert(kTabTaskCols <= 64, "k_tables_lpc maps one lane to each column of a task: wider tasks would lose columns");

template <int BM>
__global__ __launch_bounds__(64 * kLpcWaves) void k_tables_lpc(TablesArgs a) {
  __shared__ __attribute__((aligned(16))) double lds[kLpcLds];
  __shared__ double etab[64];
  __shared__ unsigned suqb[kQTiles];
  // per-wave head / tail parts of bound segments split between two waves: tiles as ceil(256 max),
  // stretches as (float) max -- the form the bound takes anyway
  __shared__ unsigned spart2[kLpcWaves][2][64];
  double(*spart)[64] = reinterpret_cast<double(*)[64]>(lds + kLpcPart);  // per-wave partial maxima, then sums
  __shared__ int sfb[64];
  __shared__ int nfb;
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int GS = a.GS, G = a.G;
  if (threadIdx.x < 64) etab[threadIdx.x] = kExp2Frac64[threadIdx.x];
  if (a.gate && *a.gate == 0) return;
  const int4 task = a.tasks[blockIdx.x];
  const int c = task.x;
  if (c < 0) {  // the ELL pad column (phase 2)
    if (w == 0) {
      for (int k = lane; k < GS; k += 64)
        if (a.D) a.D[a.ncols * GS + k] = 0.0;
      if (a.U && lane < kStretchSlots) a.U[a.ncols * kStretchSlots + lane] = 0.0;
      if (a.UQ && lane < kQTiles) a.UQ[a.ncols * kQTiles + lane] = 0u;
    }
    return;
  }
  const int phase = a.phase;
  const long long co = (long long)c * GS;
  const int bc = (phase == 2) ? tab_base_col(a, c) : -1;
  if (bc >= 0 && a.UQ && threadIdx.x < kQTiles) suqb[threadIdx.x] = a.UQ[(long long)bc * kQTiles + threadIdx.x];
  if (threadIdx.x == 0) nfb = 0;
  const double theta = a.theta[co];
  const double* P = a.pq + 4 * co;
  int lean = theta > 0.0 && theta <= DBL_MAX;
  for (int k = threadIdx.x; k < kTabStagedG; k += 64 * kLpcWaves) {
    const bool in = k < G;
    double lq = 0.0, B = 0.0, lc = -INFINITY, cf = 0.0, base = 0.0, mu = 0.0;
    if (in) {
      mu = a.mu[co + k];
      const double lp = P[2 * GS + k], lr = a.lcfpr[co + k];
      lq = P[3 * GS + k];
      lc = a.lcfp[co + k];
      cf = a.cfp ? a.cfp[co + k] : exp(lc);
      B = fma(theta, lp, lr);
      if (bc >= 0) base = a.D[(long long)bc * GS + k];
      // false for NaN and +inf; mu nondecreasing
      const bool ok = (k == G - 1 || mu <= a.mu[co + k + 1]) && lp <= DBL_MAX && lq <= DBL_MAX && lr <= DBL_MAX &&
                      lc <= DBL_MAX && cf <= DBL_MAX && cf == cf;
      lean &= ok ? 1 : 0;
    }
    lds[kLpcQB + 2 * k] = lq;
    lds[kLpcQB + 2 * k + 1] = B;
    lds[kLpcLC + 2 * k] = lc;
    lds[kLpcLC + 2 * k + 1] = cf;
    lds[kLpcBase + k] = base;
    lds[kLpcMu + k] = mu;
  }
  lean = __syncthreads_and(lean);
  // the log tables from global memory (cache-resident; the mixed branch that reads them runs on
  // ~1.5% of the points): 2.3 KB less LDS per block, four blocks per CU instead of three
  const LogTab lt{kLogInvC, kLogCHi, kLogCLo};
  const int zc = (phase == 2) ? tab_zcol(a, c) : -1;
  const double maxcfp = a.cellscal[2 * c];
  const double minlp = a.minlogprob;
  // this lane's column and its constants
  const int col = task.y + lane;
  const bool mine = col < task.z && col != zc;
  double x = 1.0, c10 = 0.0, fp = 0.0, lpo = -1.0, lqo = -1.0;
  bool ok = false;
  if (mine) {
    const double* cc = a.colc + (long long)col * kColc;
    const double xx = (double)a.ucl[col], n = cc[0], cten = cc[10];
    if (lean && xx > 0.0 && n > 0.0 && cten >= -DBL_MAX && cten <= DBL_MAX) {
      ok = true;
      x = xx;
      c10 = cten;
      fp = cc[7];
      lpo = cc[8];
      lqo = cc[9];
    }
  }
  // the override point: m = #{k < G : mu_k < x}; ks = m - 1 where x < mu_m (or m = G)
  int ks = -1;
  double nb0o = 0.0;  // the override point's x log q' + theta log p' + log(1 - cfp) (c10 added at use)
  {
    int lo = 0, hi = G;
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (lds[kLpcMu + mid] < x) lo = mid + 1; else hi = mid;
    }
    if (lo >= 1 && (lo == G || x < lds[kLpcMu + lo])) {
      ks = lo - 1;
      nb0o = fma(x, lqo, fma(theta, lpo, a.lcfpr[co + ks]));
    }
  }
  // this wave's grid range [k0, k1) (multiples of kLpcFlush but the last end)
  const int Gr = (G + kLpcFlush - 1) / kLpcFlush * kLpcFlush;
  // (at least 64 points: a bound segment spans at most two waves)
  const int per = max(64, (Gr / kLpcFlush + kLpcWaves - 1) / kLpcWaves * kLpcFlush);
  const int k0 = min(Gr, w * per), k1 = min(G, k0 + per), k1r = min(Gr, k0 + per);
  const double2* QB = reinterpret_cast<const double2*>(lds + kLpcQB);
  const double2* LC = reinterpret_cast<const double2*>(lds + kLpcLC);
  // pass 1: the maximum (the override selected before the last add, so the maximum's operands are
  // arithmetic results and need no canonicalising)
  double m = -INFINITY;
#pragma unroll LPC_U12
  for (int k = k0; k < k1; ++k) {
    const double2 qb = QB[k];
    double nb = fma(x, qb.x, qb.y);
    nb = (k == ks) ? nb0o : nb;
    nb += c10;
    m = fmax(m, nb);
  }
  spart[w][lane] = m;
  __syncthreads();
  m = fmax(fmax(fmax(spart[0][lane], spart[1][lane]), spart[2][lane]), spart[3][lane]);
  double maxp = m;
  if (maxp < (maxcfp + fp)) maxp = maxcfp + fp;
  ok = ok && maxp > -INFINITY && maxp < INFINITY;
  if (!ok) maxp = 0.0;  // (a finite stand-in: the column goes through tables_column_reg)
  const double d0 = fp - maxp;
  const double E = exp_tab(fmax(d0, -746.0), etab);  // exp(fp - maxp); 0 below -746
  // pass 2: the normaliser, every point as if without the override; the one override point's term
  // is swapped in after the loop by the wave whose range holds it
  double ls = 0.0;
#pragma unroll LPC_U12
  for (int k = k0; k < k1; ++k) {
    const double2 qb = QB[k];
    const double cf = LC[k].y;
    const double t1 = (fma(x, qb.x, qb.y) + c10) - maxp;
    double e = cf * E;
    if (!(SCDE_LPC_DIAG & 2)) e += exp_tab(fmax(t1, -746.0), etab);
    ls += e;
  }
  if (ks >= k0 && ks < k1) {
    const double cf = LC[ks].y, tp = (fma(x, QB[ks].x, QB[ks].y) + c10) - maxp, to = (nb0o + c10) - maxp;
    ls += (cf * E + exp_tab(fmax(to, -746.0), etab)) - (cf * E + exp_tab(fmax(tp, -746.0), etab));
  }
  __syncthreads();  // (every wave has read spart)
  spart[w][lane] = ls;
  __syncthreads();
  const double sq = ((spart[0][lane] + spart[1][lane]) + spart[2][lane]) + spart[3][lane];
  const double lsum = log_tab(sq, lt);  // s >= 1 (the maximum term is exp(0))
  __syncthreads();  // (region R becomes the transposes)
  // pass 3: the row, its clamp, bounds and stores
  const bool want_maxi = a.maxi != nullptr;
  double bv = -INFINITY;
  int bi = 0x7fffffff;
  unsigned long long clampm = 0;  // lanes with a point below minlogprob (before the clamp)
  const unsigned long long okm = __builtin_amdgcn_ballot_w64(ok);
  double* tw = lds + kLpcR + w * 64 * kLpcTS;
  double* const T = a.T;
  double* const D = (phase && a.D) ? a.D : nullptr;
  const long long cbase = task.y;
  // bound segments (32-point tiles / 64-point stretches): running maxima; a segment this wave's range
  // holds whole is written here, its head / tail parts go through LDS to the combine below
  constexpr int BSZ = (BM == kBoundStretch) ? 64 : kBTile;
  // a segment's maximum in the bound's own form: ceil(256 max) (tiles), (float) max (stretches) --
  // both monotone, so the form of the maximum is the maximum of the forms
  auto bound_form = [&](double mx) -> unsigned {
    if (BM == kBoundTiles) return (unsigned)(int)ceil(fmax(mx * 256.0, -0x1p29));
    return __float_as_uint((float)mx);
  };
  auto bound_max = [&](unsigned p, unsigned q) -> unsigned {
    if (BM == kBoundTiles) return (unsigned)max((int)p, (int)q);
    return __float_as_uint(fmaxf(__uint_as_float(p), __uint_as_float(q)));
  };
  auto put_bound = [&](int seg, unsigned form) {
    if (!ok) return;
    if (BM == kBoundTiles) {
      int u = (int)form;
      if (bc >= 0) u -= unpacku(suqb[seg]);
      a.UQ[(long long)col * kQTiles + seg] = packu(u);
    } else if (BM == kBoundStretch) {
      const float mf = __uint_as_float(form);
      const double mm = (double)mf + 0x1p-23 * fabs((double)mf);
      a.U[(long long)col * kStretchSlots + seg] = (bc >= 0) ? mm - a.U[(long long)bc * kStretchSlots + seg] : mm;
    }
  };
  double bt = -INFINITY;
  for (int f0 = k0; f0 < k1r; f0 += kLpcFlush) {
#pragma unroll LPC_U3
    for (int kk = 0; kk < kLpcFlush; ++kk) {
      const int k = f0 + kk;
      double r = 0.0;  // pad points of the last flush
      if (k < k1) {
        const double2 qb = QB[k], lcf = LC[k];
        double nb = fma(x, qb.x, qb.y);
        nb = (k == ks) ? nb0o : nb;
        const double t1 = (nb + c10) - maxp, t2 = lcf.x + d0;
        const double hi = fmax(t2, t1);
        const bool tiny = !(hi >= -665.0);
        const bool tm = tiny || !(fabs(t1 - t2) > 37.5);
        r = hi - lsum;
        if (!(SCDE_LPC_DIAG & 4) && __builtin_amdgcn_ballot_w64(ok && tm)) {
          double e = fma(lcf.y, E, exp_tab(fmax(t1, -746.0), etab));
          if (__builtin_amdgcn_ballot_w64(ok && tiny)) {
            // subnormal range: the Poisson term as the reference forms it, exp(log cfp_k + fp - maxp),
            // rounded once -- cfp_k E would carry the few bits a subnormal E has left
            const double et = exp_tab(fmax((lcf.x + fp) - maxp, -746.0), etab) + exp_tab(fmax(t1, -746.0), etab);
            e = tiny ? et / sq : e;
          }
          const double rm = log_tab(e, lt) - (tiny ? 0.0 : lsum);
          r = tm ? rm : r;
        }
        if (want_maxi) {
          const bool better = r > bv;
          bv = better ? r : bv;
          bi = better ? k : bi;
        }
        clampm |= __builtin_amdgcn_ballot_w64(r < minlp);
        r = fmax(r, minlp);
        if (BM != kBoundNone) {
          bt = fmax(bt, r);
          if ((k % BSZ) == BSZ - 1 || k == k1 - 1) {  // (wave-uniform)
            const int seg = k / BSZ;
            const bool head = seg * BSZ < k0, tail = (k % BSZ) != BSZ - 1 && k != G - 1;
            if (!head && !tail)
              put_bound(seg, bound_form(bt));
            else
              spart2[w][tail ? 1 : 0][lane] = bound_form(bt);
            bt = -INFINITY;
          }
        }
      }
      tw[lane * kLpcTS + kk] = r;
    }
    // the flush: 4 lanes per column, 16 columns per store
#pragma unroll
    for (int i = 0; i < ((SCDE_LPC_DIAG & 1) ? 0 : 4); ++i) {
      const int cc_ = i * 16 + (lane >> 2), kp = (lane & 3) * 2;
      if ((okm >> cc_) & 1ull) {
        const double r0 = tw[cc_ * kLpcTS + kp], r1 = tw[cc_ * kLpcTS + kp + 1];
        const long long off = (cbase + cc_) * GS + f0 + kp;
        if (T) tab_store2(T + off, r0, r1, a.nt_rows);
        if (D) {
          const double2 bb = *reinterpret_cast<const double2*>(lds + kLpcBase + f0 + kp);
          tab_store2(D + off, r0 - bb.x, r1 - bb.y, a.nt_rows);
        }
      }
    }
  }
  // zero pads [Gr, GP): flushes of zeros, round-robin over the waves.  GP = the 64-point stretch end
  // (448 at G = 401): the bootstrap kernels read rows up to their last 32-point tile / 64-point
  // stretch; [GP, GS) is alignment only, never read (timing build SCDE_LPC_DIAG & 8 writes NaN there:
  // the GPU suite stays green)
  const int GP = (SCDE_LPC_DIAG & 8) ? GS : min(GS, (G + 63) / 64 * 64);
  for (int f0 = Gr + kLpcFlush * w; f0 < GP; f0 += kLpcFlush * kLpcWaves) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int cc_ = i * 16 + (lane >> 2), kp = (lane & 3) * 2;
      if ((okm >> cc_) & 1ull) {
        const long long off = (cbase + cc_) * GS + f0 + kp;
        const double z = ((SCDE_LPC_DIAG & 8) && f0 >= (G + 63) / 64 * 64) ? __builtin_nan("") : 0.0;
        if (T) tab_store2(T + off, z, z, a.nt_rows);
        if (D) tab_store2(D + off, z, z, a.nt_rows);
      }
    }
  }
  // the four waves' partials: clamp flag, argmax, bound segments split between waves
  __syncthreads();  // (every wave is done with the staged rows: the combine's arrays overlay them)
  double(*sclamp)[64] = reinterpret_cast<double(*)[64]>(lds);
  double(*sbv)[64] = reinterpret_cast<double(*)[64]>(lds + kLpcWaves * 64);
  int(*sbi)[64] = reinterpret_cast<int(*)[64]>(lds + 2 * kLpcWaves * 64);
  sclamp[w][lane] = ((clampm >> lane) & 1ull) ? 1.0 : 0.0;
  sbi[w][lane] = bi;
  sbv[w][lane] = bv;
  __syncthreads();
  if (w == 0 && ok) {
    a.has_clamp[col] = (sclamp[0][lane] + sclamp[1][lane] + sclamp[2][lane] + sclamp[3][lane] > 0.0) ? 1 : 0;
    if (want_maxi) {
      double b = sbv[0][lane];
      int bix = sbi[0][lane];
      for (int v = 1; v < kLpcWaves; ++v)
        if (sbv[v][lane] > b) {  // ties: the earlier wave holds the smaller index
          b = sbv[v][lane];
          bix = sbi[v][lane];
        }
      a.maxi[col] = (bix == 0x7fffffff) ? 0 : bix;
    }
  }
  if (BM != kBoundNone && w > 0 && (k0 % BSZ) != 0 && k0 < G)  // the segment wave w - 1 began and w ended
    put_bound(k0 / BSZ, bound_max(spart2[w - 1][1][lane], spart2[w][0][lane]));
  if (BM == kBoundTiles && w == kLpcWaves - 1)
    for (int t = (G + kBTile - 1) / kBTile; t < kQTiles; ++t)
      if (ok) a.UQ[(long long)col * kQTiles + t] = packu(0);
  // the columns outside the lane pass: tables_column_reg, over the general staged rows
  // (wave 0 alone lists them: every wave holds the same 64 columns, and a cell that is not lean
  // leaves all 64 -- four waves listing them would write 256 entries into sfb's 64)
  if (w == 0 && mine && !ok) sfb[atomicAdd(&nfb, 1)] = col;
  __syncthreads();
  const int nf = nfb;
  if (nf == 0) return;
  double* sm = lds;  // (overlays the lane pass's rows and transposes)
  for (int k = threadIdx.x; k < kRS; k += 64 * kLpcWaves) {
    const bool in = k < G;
    sm[kRowMu * kRS + k] = in ? a.mu[co + k] : 0.0;
    sm[kRowLP * kRS + k] = in ? P[2 * GS + k] : 0.0;
    sm[kRowLQ * kRS + k] = in ? P[3 * GS + k] : 0.0;
    sm[kRowLcfpr * kRS + k] = in ? a.lcfpr[co + k] : 0.0;
    const double lc = in ? a.lcfp[co + k] : -INFINITY;
    sm[kRowCfp * kRS + k] = in ? (a.cfp ? a.cfp[co + k] : exp(lc)) : 0.0;
    sm[kRowLcfp * kRS + k] = lc;
    sm[kRowBase * kRS + k] = (in && bc >= 0) ? a.D[(long long)bc * GS + k] : 0.0;
  }
  __syncthreads();
  for (int i = w; i < nf; i += kLpcWaves) {
    const int fc = __builtin_amdgcn_readfirstlane(sfb[i]);
    tables_column_reg<BM, 0>(a, fc, c, phase, sm, bc >= 0, suqb, etab, lt, lane, theta, a.colc + (long long)fc * kColc,
                             (double)a.ucl[fc], maxcfp, bc);
  }
}

// ------------------------------------------------------------------ baseline / ELL
// base_col[c] = flat column of count 0 in cell c when that column has no
// clamped value, else -1 (cells without a usable baseline are always explicit).
__global__ void k_base_cols(const int* __restrict__ ucl, const long long* __restrict__ ucl_off, int ncells,
                            const unsigned char* __restrict__ has_clamp, int use_baseline,
                            int* __restrict__ base_col) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= ncells) return;
  int bc = -1;
  if (use_baseline) {
    for (long long i = ucl_off[c]; i < ucl_off[c + 1]; ++i) {
      if (ucl[i] == 0) {
        if (!has_clamp[i]) bc = (int)i;
        break;
      }
    }
  }
  base_col[c] = bc;
}

// D[col] = T[col] - T[baseline column of its cell] (or T[col] when the cell has no
// baseline); column ncols is all zeros.  One wavefront per column.
__global__ __launch_bounds__(256) void k_delta(const double* __restrict__ T, const long long* __restrict__ ucl_off,
                                              int ncells, long long ncols, const int* __restrict__ base_col, int G,
                                              int GS, double* __restrict__ D) {
  const int lane = threadIdx.x & 63;
  const long long col = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (col > ncols) return;
  if (col == ncols) {
    for (int k = lane; k < GS; k += 64) D[col * GS + k] = 0.0;
    return;
  }
  int lo = 0, hi = ncells;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (ucl_off[mid] <= col) lo = mid; else hi = mid;
  }
  const int bc = base_col[lo];
  for (int k = lane; k < GS; k += 64) {
    const double t = (k < G) ? T[col * GS + k] : 0.0;
    D[col * GS + k] = (bc >= 0 && k < G) ? t - T[(long long)bc * GS + k] : t;
  }
}

// Z[set][b][k] = sum over baseline cells of W[set][c][b] * T[base_col[c]][k].
// One workgroup per (4 boots, 64-point tile of k, set): wave w takes the cells c = w
// (mod 4), each lane one k with the 4 boots' partial sums (each baseline column read once
// per 4 boots); the 4 waves' partials combine in a fixed order.  Bp is a multiple of 4.
// 16 waves per (set, 4 boots, 64 points), each over every 16th cell, partials added in wave
// order: 4x the waves of a 4-wave block for the same latency-bound chains
constexpr int kZWaves = 16;
__global__ __launch_bounds__(64 * kZWaves) void k_baseline_z(const double* __restrict__ T, int G, int GS,
                                                            const int* __restrict__ base_col, int ncells,
                                                            const double* __restrict__ Wt, int Bp,
                                                            double* __restrict__ Z, int gsets, int gsplit) {
  __shared__ double part[kZWaves][4][64];  // [wave][boot][lane]
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int b0 = blockIdx.x * 4, k = blockIdx.y * 64 + lane, set = blockIdx.z;
  const double* W = Wt + (long long)set * ncells * Bp + b0;
  // fused groups: the set's own group's cells, in that group's order (the same sums as its own call)
  const bool g2 = gsets > 0 && set >= gsets;
  const int clo = g2 ? gsplit : 0, chi = (gsets > 0 && !g2) ? gsplit : ncells;
  double z[4] = {0.0, 0.0, 0.0, 0.0};
  if (k < G) {
    for (int c = clo + wid; c < chi; c += kZWaves) {
      const int bc = base_col[c];
      if (bc < 0) continue;
      const double t = T[(long long)bc * GS + k];
      const double* w = W + (long long)c * Bp;
#pragma unroll
      for (int r = 0; r < 4; ++r) z[r] = fma(w[r], t, z[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) part[wid][r][lane] = z[r];
  __syncthreads();
  if (wid < 4 && k < GS) {
    double s = part[0][wid][lane];
#pragma unroll
    for (int w = 1; w < kZWaves; ++w) s += part[w][wid][lane];
    Z[((long long)set * Bp + b0 + wid) * GS + k] = s;
  }
}

// ZU[set][b][j] = sum over baseline cells of W[set][c][b] * U[base_col[c]][j]: the
// baseline part of k_boot2's stretch upper bounds (U holds the baseline columns' raw
// stretch maxima).  One 256-thread block per (set, boot); threads over cells, then a
// fixed-order tree over the block.
__global__ __launch_bounds__(256) void k_stretch_zu(const double* __restrict__ U, const int* __restrict__ base_col,
                                                    int ncells, const double* __restrict__ Wt, int Bp,
                                                    double* __restrict__ ZU, int gsets, int gsplit) {
  __shared__ double part[256][kStretchSlots + 1];
  const int b = blockIdx.x, set = blockIdx.y, t = threadIdx.x;
  const double* W = Wt + (long long)set * ncells * Bp + b;
  const bool g2 = gsets > 0 && set >= gsets;  // fused groups: the set's own group's cells
  const int clo = g2 ? gsplit : 0, chi = (gsets > 0 && !g2) ? gsplit : ncells;
  double z[kStretchSlots];
#pragma unroll
  for (int j = 0; j < kStretchSlots; ++j) z[j] = 0.0;
  for (int c = clo + t; c < chi; c += 256) {
    const int bc = base_col[c];
    if (bc < 0) continue;
    const double w = W[(long long)c * Bp];
    const double* u = U + (long long)bc * kStretchSlots;
#pragma unroll
    for (int j = 0; j < kStretchSlots; ++j) z[j] = fma(w, u[j], z[j]);
  }
#pragma unroll
  for (int j = 0; j < kStretchSlots; ++j) part[t][j] = z[j];
  __syncthreads();
  for (int h = 128; h >= 1; h >>= 1) {
    if (t < h)
#pragma unroll
      for (int j = 0; j < kStretchSlots; ++j) part[t][j] += part[t + h][j];
    __syncthreads();
  }
  if (t < kStretchSlots) ZU[((long long)set * Bp + b) * kStretchSlots + t] = part[0][t];
}

// Reduce-scatter of BC in {4, 8, 16} values over the wave, all on VALU.  Halving stages
// pair lanes by bit 5, 4 (swaps: after the swap, a + b is the pair sum on every lane,
// no selects), then bit 3 (lane ^ 15), bit 2 (lane ^ 7) with a keep/send select; the
// remaining bits are plain butterflies.  Lane l ends with boot index
// (l >> (6 - log2 BC)) & (BC - 1), summed over all 64 lanes (the masks 32, 16, 15, 7,
// 2, 1 span the six lane bits).
template <int BC, bool MAX>
__device__ __forceinline__ double wave_reduce_scatter_v(double (&v)[BC], int lane) {
  static_assert(BC == 4 || BC == 8 || BC == 16, "BC must be 4, 8 or 16");
#pragma unroll
  for (int j = 0; j < BC / 2; ++j) {
    swap32(v[j], v[j + BC / 2]);
    v[j] = red_op<MAX>(v[j], v[j + BC / 2]);
  }
#pragma unroll
  for (int j = 0; j < BC / 4; ++j) {
    swap16(v[j], v[j + BC / 4]);
    v[j] = red_op<MAX>(v[j], v[j + BC / 4]);
  }
  if constexpr (BC >= 8) {
    const bool up = (lane & 8) != 0;
#pragma unroll
    for (int j = 0; j < BC / 8; ++j) {
      const double lo = v[j], hi = v[j + BC / 8];
      v[j] = red_op<MAX>(up ? hi : lo, dpp_d<kDppMirror>(up ? lo : hi));
    }
  }
  if constexpr (BC >= 16) {
    const bool up = (lane & 4) != 0;
    const double lo = v[0], hi = v[1];
    v[0] = red_op<MAX>(up ? hi : lo, dpp_d<kDppHalfMirror>(up ? lo : hi));
  }
  double x = v[0];
  if constexpr (BC <= 4) x = red_op<MAX>(x, dpp_d<kDppMirror>(x));
  if constexpr (BC <= 8) x = red_op<MAX>(x, dpp_d<kDppHalfMirror>(x));
  x = red_op<MAX>(x, dpp_d<kDppXor2>(x));
  x = red_op<MAX>(x, dpp_d<kDppXor1>(x));
  return x;
}

// Reduce-scatter the per-lane values of segment [I0, I0+BC) across the wave and park
// the wave's partials in red[wid][I0 + idx] (no barrier here).
template <int BC, bool MAX, int NB>
__device__ __forceinline__ void wave_partials(const double (&x)[NB], int I0, bool live, double* red, int lane,
                                              int wid) {
  constexpr int L2 = (BC == 16) ? 4 : (BC == 8) ? 3 : (BC == 4) ? 2 : (BC == 2) ? 1 : 0;
  double t[BC];
#pragma unroll
  for (int i = 0; i < BC; ++i) t[i] = x[I0 + i];  // dead lanes hold -inf / 0 already
  const double r = wave_reduce_scatter_v<BC, MAX>(t, lane);
  const int idx = (lane >> (6 - L2)) & (BC - 1);
  if ((lane & ((64 >> L2) - 1)) == 0) red[wid * 32 + I0 + idx] = r;
}

// All NB boots of a slab at once: one LDS round per reduction.  NB = 16a + 8b + 4c.
template <bool MAX, int NB>
__device__ __forceinline__ void block_reduce_all(const double (&x)[NB], bool live, double* red, double* fin,
                                                 int lane, int wid, int nw) {
#pragma unroll
  for (int i0 = 0; i0 + 16 <= NB; i0 += 16) wave_partials<16, MAX, NB>(x, i0, live, red, lane, wid);
  if constexpr ((NB % 16) >= 8) wave_partials<8, MAX, NB>(x, NB - (NB % 16), live, red, lane, wid);
  if constexpr ((NB % 8) >= 4) wave_partials<4, MAX, NB>(x, NB - (NB % 8), live, red, lane, wid);
  __syncthreads();
  if ((int)threadIdx.x < NB) {
    double r = red[threadIdx.x];
    for (int w = 1; w < nw; ++w) r = MAX ? gt_max(r, red[w * 32 + threadIdx.x]) : r + red[w * 32 + threadIdx.x];
    fin[threadIdx.x] = r;
  }
  __syncthreads();
}

// ---- per-boot maximum in f32 (the softmax shift) ----
// softmax(acc) is invariant to the shift; the reference subtracts the exact row max, we
// subtract m' = (double)(f32 max).  For |m| <= 2^24 (every row that is not flagged
// degenerate) |m - m'| <= 1, so the largest term is exp(m - m') in [1/e, e]: no overflow,
// no loss, results equal to rounding.  Rows beyond 2^24 (including maxima below -FLT_MAX,
// which convert to -inf) are flagged and recomputed in exact order by k_boot_exact.

// f32 twin of wave_reduce_scatter_v (same lane -> index mapping), max only.
template <int BC>
__device__ __forceinline__ float wave_max_scatter_f(float (&v)[BC], int lane) {
  static_assert(BC == 4 || BC == 8 || BC == 16, "BC must be 4, 8 or 16");
#pragma unroll
  for (int j = 0; j < BC / 2; ++j) {
    swap32f(v[j], v[j + BC / 2]);
    v[j] = gt_maxf(v[j], v[j + BC / 2]);
  }
#pragma unroll
  for (int j = 0; j < BC / 4; ++j) {
    swap16f(v[j], v[j + BC / 4]);
    v[j] = gt_maxf(v[j], v[j + BC / 4]);
  }
  if constexpr (BC >= 8) {
    const bool up = (lane & 8) != 0;
#pragma unroll
    for (int j = 0; j < BC / 8; ++j) {
      const float lo = v[j], hi = v[j + BC / 8];
      v[j] = gt_maxf(up ? hi : lo, dpp_f<kDppMirror>(up ? lo : hi));
    }
  }
  if constexpr (BC >= 16) {
    const bool up = (lane & 4) != 0;
    const float lo = v[0], hi = v[1];
    v[0] = gt_maxf(up ? hi : lo, dpp_f<kDppHalfMirror>(up ? lo : hi));
  }
  float x = v[0];
  if constexpr (BC <= 4) x = gt_maxf(x, dpp_f<kDppMirror>(x));
  if constexpr (BC <= 8) x = gt_maxf(x, dpp_f<kDppHalfMirror>(x));
  x = gt_maxf(x, dpp_f<kDppXor2>(x));
  x = gt_maxf(x, dpp_f<kDppXor1>(x));
  return x;
}

template <int BC, int NB>
__device__ __forceinline__ void wave_max_partials(const double (&x)[NB], int I0, float* redf, int lane, int wid) {
  constexpr int L2 = (BC == 16) ? 4 : (BC == 8) ? 3 : 2;
  float t[BC];
#pragma unroll
  for (int i = 0; i < BC; ++i) t[i] = (float)x[I0 + i];
  const float r = wave_max_scatter_f<BC>(t, lane);
  const int idx = (lane >> (6 - L2)) & (BC - 1);
  if ((lane & ((64 >> L2) - 1)) == 0) redf[wid * 32 + I0 + idx] = r;
}

// All NB boots' f32 maxima over one wave -> redf[slot * 32 + boot] (no barrier).
template <int NB>
__device__ __forceinline__ void wave_max_partials_all(const double (&x)[NB], float* redf, int lane, int slot) {
#pragma unroll
  for (int i0 = 0; i0 + 16 <= NB; i0 += 16) wave_max_partials<16, NB>(x, i0, redf, lane, slot);
  if constexpr ((NB % 16) >= 8) wave_max_partials<8, NB>(x, NB - (NB % 16), redf, lane, slot);
  if constexpr ((NB % 8) >= 4) wave_max_partials<4, NB>(x, NB - (NB % 8), redf, lane, slot);
}

// All NB boots' approximate maxima -> fin (as double).  redf: 16 x 32 floats.
template <int NB>
__device__ __forceinline__ void block_max_f32(const double (&x)[NB], float* redf, double* fin, int lane, int wid,
                                              int nw) {
#pragma unroll
  for (int i0 = 0; i0 + 16 <= NB; i0 += 16) wave_max_partials<16, NB>(x, i0, redf, lane, wid);
  if constexpr ((NB % 16) >= 8) wave_max_partials<8, NB>(x, NB - (NB % 16), redf, lane, wid);
  if constexpr ((NB % 8) >= 4) wave_max_partials<4, NB>(x, NB - (NB % 8), redf, lane, wid);
  __syncthreads();
  if ((int)threadIdx.x < NB) {
    float r = redf[threadIdx.x];
    for (int w = 1; w < nw; ++w) r = gt_maxf(r, redf[w * 32 + threadIdx.x]);
    fin[threadIdx.x] = (double)r;
  }
  __syncthreads();
}

// Variants for blocks whose waves outside `wmask` have exited (k_boot2 stretch
// skipping): s_barrier waits only for the surviving waves, the combine reads only their
// slots, and the first surviving wave (`lead`) does it.
template <int NB>
__device__ __forceinline__ void block_max_f32_m(const double (&x)[NB], float* redf, double* fin, int lane, int wid,
                                                int nw, unsigned wmask, int lead) {
#pragma unroll
  for (int i0 = 0; i0 + 16 <= NB; i0 += 16) wave_max_partials<16, NB>(x, i0, redf, lane, wid);
  if constexpr ((NB % 16) >= 8) wave_max_partials<8, NB>(x, NB - (NB % 16), redf, lane, wid);
  if constexpr ((NB % 8) >= 4) wave_max_partials<4, NB>(x, NB - (NB % 8), redf, lane, wid);
  __syncthreads();
  if (wid == lead && lane < NB) {
    float r = -INFINITY;
    for (int w = 0; w < nw; ++w)
      if ((wmask >> w) & 1) r = gt_maxf(r, redf[w * 32 + lane]);
    fin[lane] = (double)r;
  }
  __syncthreads();
}
template <int NB>
__device__ __forceinline__ void block_sum_m(const double (&x)[NB], bool live, double* red, double* fin, int lane,
                                            int wid, int nw, unsigned wmask, int lead) {
#pragma unroll
  for (int i0 = 0; i0 + 16 <= NB; i0 += 16) wave_partials<16, false, NB>(x, i0, live, red, lane, wid);
  if constexpr ((NB % 16) >= 8) wave_partials<8, false, NB>(x, NB - (NB % 16), live, red, lane, wid);
  if constexpr ((NB % 8) >= 4) wave_partials<4, false, NB>(x, NB - (NB % 8), live, red, lane, wid);
  __syncthreads();
  if (wid == lead && lane < NB) {
    double r = 0.0;
    for (int w = 0; w < nw; ++w)
      if ((wmask >> w) & 1) r += red[w * 32 + lane];
    fin[lane] = r;
  }
  __syncthreads();
}

// Grid-stretch masks for k_boot2 (one wave per (gene, boot slab of NB <= 32)).
// A boot's row is Z_b + sum_e W_be D_e; over stretch s (grid points 64s .. 64s+63, one
// k_boot2 wave) it is bounded by the per-column stretch maxima of k_tables (U) and their
// baseline part (ZU):
//   UB_bs = ZU_bs + sum_e W_be U_e,s  >=  every row value in the stretch,
// a (boots x entries) . (entries x stretches) product, done here on the FP64 matrix
// cores (v_mfma_f64_16x16x4: 16 boots x 16 stretch slots x 4 entries per instruction;
// two boot tiles).  Heuristic mask: stretch s is kept when some live boot has
// UB_bs >= max_s' UB_bs' - 50 - slack.  Rigour comes from k_boot2's post-check, which
// compares each skipped stretch's UB with the exact row maximum and sends the slab to
// the redo launch when UB_bs >= max_b - 50 (the softmax cut): skipped stretches only ever
// hold terms the cut zeroes anyway.  Writes UB [gene][slab][8][NB] and mask [gene][slab].
typedef double d4_t __attribute__((ext_vector_type(4)));
template <int NB>
__global__ __launch_bounds__(64) void k_stretch_mask(const int2* __restrict__ ent, const int* __restrict__ nnz,
                                                     int ent_stride, const double* __restrict__ Wt, int Bp,
                                                     int ncells, const int* __restrict__ wset, int G, int P,
                                                     int nboot, const double* __restrict__ U,
                                                     const double* __restrict__ ZU, double slack,
                                                     double* __restrict__ ub_out, int* __restrict__ mask,
                                                     int ngenes) {
  static_assert(NB <= 32, "two 16-boot tiles");
  extern __shared__ int2 es[];  // the gene's entries: each step's gathers then wait on LDS only
  __shared__ double ubs[kStretchSlots][32];
  const int lane = threadIdx.x;
  const int g = blockIdx.x / P, p = blockIdx.x % P;
  if (g >= ngenes) return;
  const int b0 = p * NB, n = nnz[g];
  const int nst = (G + 63) / 64;
  {
    const int2* __restrict__ Eg = ent + (long long)g * ent_stride;
    const int n4s = (n + 3) & ~3;
    for (int e = lane; e < n4s; e += 64) es[e] = Eg[e];
    __syncthreads();
  }
  const int2* E = es;
  const int set = wset ? wset[g] : 0;
  const double* __restrict__ W = Wt + (long long)set * ncells * Bp + b0;
  const int r = lane & 15, k4 = lane >> 4;  // A: boot r, entry k4; B: entry k4, stretch r
  const bool a1ok = 16 + r < NB, bok = r < nst;
  d4_t c0 = {0, 0, 0, 0}, c1 = {0, 0, 0, 0};
  // rows are padded with zero-column entries to a multiple of 8 (U of the pad column is 0)
  const int n4 = (n + 3) & ~3;
#pragma unroll 2
  for (int e0 = 0; e0 < n4; e0 += 4) {
    const int2 x = E[e0 + k4];
    const double* w = W + (long long)x.x * Bp;
    const double a0 = w[r];
    const double a1 = a1ok ? w[16 + r] : 0.0;
    const double bb = bok ? U[(long long)x.y * kStretchSlots + r] : 0.0;
    c0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, bb, c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, bb, c1, 0, 0, 0);
  }
  // C/D (f64 16x16x4): column = lane & 15 (stretch), rows (lane >> 4) + 4 j (boots)
  if (r < nst) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i0 = k4 + 4 * j, i1 = 16 + k4 + 4 * j;
      if (i0 < NB) ubs[r][i0] = c0[j] + ZU[((long long)set * Bp + b0 + i0) * kStretchSlots + r];
      if (i1 < NB) ubs[r][i1] = c1[j] + ZU[((long long)set * Bp + b0 + i1) * kStretchSlots + r];
    }
  }
  __syncthreads();
  double* o = ub_out + (long long)blockIdx.x * kStretchSlots * NB;
  for (int t = lane; t < nst * NB; t += 64) o[t] = ubs[t / NB][t % NB];
  unsigned need = 0;
  if (lane < NB && b0 + lane < nboot) {
    double m = -INFINITY;
    for (int st = 0; st < nst; ++st) m = gt_max(m, ubs[st][lane]);
    for (int st = 0; st < nst; ++st)
      if (!(ubs[st][lane] < m - 50.0 - slack)) need |= 1u << st;
  }
#pragma unroll
  for (int o2 = 32; o2 >= 1; o2 >>= 1) need |= (unsigned)__shfl_xor((int)need, o2, 64);
  if (lane == 0) mask[blockIdx.x] = (int)need;
}

constexpr double kBootExpCut = -50.0;  // k_boot2 softmax terms below e^-50 are dropped

// One block per (gene, boot slab of NB).  Lanes over grid points (k = threadIdx.x,
// G <= blockDim <= GS); NB bootstrap accumulators per lane in VGPRs.  Per ELL entry
// the NB draw multiplicities are wave-uniform (scalar loads, the FMA's SGPR operand)
// and the baseline-delta column is one coalesced 8-byte load per lane.  The P slabs
// of a gene are placed 8 blocks apart (same XCD under round-robin dispatch) so they
// share the gene's columns in L2; each writes a partial jp row, summed in slab order
// by k_sum_partials.
// One (gene g, slab p) per block; k_boot2 maps the grid onto items, k_boot2_list walks the
// compacted item list k_boot_tiles leaves behind.
template <int NB>
__device__ __forceinline__ void boot2_slab(const double* __restrict__ D, const int2* __restrict__ ent,
                                           const int* __restrict__ nnz, int ent_stride,
                                           const double* __restrict__ Wt, int Bp, int ncells,
                                           const int* __restrict__ wset, const double* __restrict__ Z, int G,
                                           int GS, int P, int nboot, double norm_mult, double degen_thresh,
                                           double* __restrict__ part, long long part_stride,
                                           int* __restrict__ degen, int ngenes,
                                           const int* __restrict__ smask, const double* __restrict__ sub,
                                           int* __restrict__ redo, int redo_pass, int g, int p) {
  static_assert(NB % 4 == 0 && NB <= 32, "NB must be a multiple of 4, <= 32");
  constexpr int diag = SCDE_BOOT_DIAG;  // timing-only builds (tools/); 0 in production
  __shared__ double red[16 * 32];
  __shared__ double tsum[64 * NB];  // [16-point tile][boot] partial sums (G <= 1024)
  __shared__ double wfin[16][32];  // [wave][boot] the slab's maxima, then 1 / (S nboot): each wave its own copy
  __shared__ double etab[64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, nw = blockDim.x >> 6;
  const bool live = tid < G;
  const int b0 = p * NB;
  const int n = nnz[g];
  const int2* __restrict__ E = ent + (long long)g * ent_stride;
  const int set = wset ? wset[g] : 0;
  const double* __restrict__ W = Wt + (long long)set * ncells * Bp;
  const double* __restrict__ Zs = Z ? Z + (long long)set * Bp * GS : nullptr;
  // Grid-stretch skipping (smask/sub from k_stretch_mask): this wave's 64 points are
  // left out when its mask bit is clear.  After the row maxima are known, every skipped
  // stretch checks UB_bs < max_b - 51 for its live boots (1 covers the f32 maxima); a
  // failure sends the slab to the redo pass (redo_pass: only flagged slabs, no skipping),
  // so a stretch is only ever left out when all its softmax terms fall below the e^-50
  // cut that zeroes them anyway -- the output is the same as without skipping.
  if (redo_pass == 1 && !redo[(long long)g * P + p]) return;
  const unsigned wmask = smask ? (unsigned)__builtin_amdgcn_readfirstlane(smask[(long long)g * P + p]) : ~0u;
  const int wsid = __builtin_amdgcn_readfirstlane(wid);
  const bool run = (wmask >> wsid) & 1;
  const int lw = __builtin_ffs((int)wmask) - 1;  // first surviving wave: does the combines
  if (wsid == lw) etab[lane] = kExp2Frac64[lane];  // visible after the first reduction's barrier
  if (!run) {
    // a left-out stretch: its partial row is zero; the wave exits (the block's barriers
    // then wait only for the surviving waves, and the combines skip its slots)
    if (live) part[(long long)p * part_stride + (long long)g * GS + tid] = 0.0;
    __builtin_amdgcn_s_waitcnt(0);
    return;
  }
  // Entries in batches of EB, double-buffered in registers: batch e+1's column loads are
  // in flight while batch e accumulates.  ELL rows are padded to a multiple of EB plus
  // one extra batch of zero-column entries, so the look-ahead load is unconditional.
  // The multiplicities come in two boots x EB entries per scalar-load round.
  constexpr int EB = SCDE_BOOT_EB;
  double acc[NB];
  // lanes past the grid start at -inf: their pad columns are 0, so they stay -inf, never
  // win a max and exp to 0 -- the reductions need no per-lane select.  A skipped
  // stretch is set to -inf: its softmax terms are exactly the zeros the cut would give.
#pragma unroll
  for (int i = 0; i < NB; ++i)
    acc[i] = (!live || !run) ? -INFINITY : (Zs ? Zs[(long long)(b0 + i) * GS + tid] : 0.0);
  if (run) {
  const int cell0 = __builtin_amdgcn_readfirstlane(E[0].x), col0 = __builtin_amdgcn_readfirstlane(E[0].y);
  (void)cell0;
  (void)col0;
  int cell[EB];
  double v[EB];
  auto load_batch = [&](int e0, int (&c)[EB], double (&x)[EB]) {
    const int4* __restrict__ E4 = reinterpret_cast<const int4*>(E + e0);
#pragma unroll
    for (int j = 0; j < EB / 2; ++j) {
      const int4 t = E4[j];
      c[2 * j] = t.x;
      c[2 * j + 1] = t.z;
      if (diag & 2) {  // timing diagnostic: every entry reads the first entry's column (loop-invariant)
        x[2 * j] = D[(long long)col0 * GS + tid] * (1.0 + j);
        x[2 * j + 1] = D[(long long)col0 * GS + tid] * (2.0 + j);
      } else {
        x[2 * j] = D[(long long)t.y * GS + tid];
        x[2 * j + 1] = D[(long long)t.w * GS + tid];
      }
    }
  };
  auto accumulate = [&](const int (&c)[EB], const double (&x)[EB]) {
#pragma unroll
    for (int i0 = 0; i0 < NB; i0 += 2) {
      double2 w[EB];
#pragma unroll
      for (int j = 0; j < EB; ++j) {
        if (diag & 1) {  // timing diagnostic: every entry reads the first entry's multiplicities
          w[j] = *reinterpret_cast<const double2*>(W + (long long)cell0 * Bp + b0 + i0);
        } else {
          // 32-bit row offsets (cells x Bp < 2^31): one s_mul_i32 instead of a 64-bit product
          w[j] = *reinterpret_cast<const double2*>(W + (unsigned)(__builtin_amdgcn_readfirstlane(c[j]) * Bp) + b0 +
                                                   i0);
        }
      }
#pragma unroll
      for (int j = 0; j < EB; ++j) {
        acc[i0] = fma(w[j].x, x[j], acc[i0]);
        acc[i0 + 1] = fma(w[j].y, x[j], acc[i0 + 1]);
      }
    }
  };
#if SCDE_BOOT_ASMLD
  // The column loads are issued from inline asm and waited with explicit vmcnt: left to
  // itself the compiler sinks the look-ahead loads into the iteration that consumes them
  // (to fit the 64-VGPR occupancy target), which exposes their latency every batch.  Two
  // register buffers alternate (loop unrolled by 2) so no in-flight register is ever
  // copied; the wait asm ties the consumed buffer, so no FMA is hoisted above it.  Rows
  // are padded to a multiple of 8 plus 8 zero-column entries: every look-ahead batch
  // stays inside the row.
  static_assert(EB == 4, "the asm look-ahead assumes 4-entry batches");
  auto issue = [&](int e0, int (&c)[EB], double (&x)[EB]) {
    const int4* __restrict__ E4 = reinterpret_cast<const int4*>(E + e0);
#pragma unroll
    for (int j = 0; j < EB / 2; ++j) {
      const int4 t = E4[j];
      c[2 * j] = t.x;
      c[2 * j + 1] = t.z;
      // 32-bit column offsets: launch_boot2 checks (ncols + 1) x GS < 2^31
      const double* p0 = D + (unsigned)(((diag & 2) ? col0 : t.y) * GS) + tid;
      const double* p1 = D + (unsigned)(((diag & 2) ? col0 : t.w) * GS) + tid;
      asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(x[2 * j]) : "v"(p0));
      asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(x[2 * j + 1]) : "v"(p1));
    }
  };
  auto ready = [&](double (&x)[EB]) {  // all but the EB youngest column loads have landed
    asm volatile("s_waitcnt vmcnt(4)" : "+v"(x[0]), "+v"(x[1]), "+v"(x[2]), "+v"(x[3]));
  };
  (void)load_batch;
  int cellb[EB];
  double vb[EB];
  // the baseline loads into acc complete here: otherwise the compiler's wait for them
  // lands at the first FMA inside the loop, as a vmcnt(0) executed every iteration
#pragma unroll
  for (int i = 0; i < NB; ++i) asm volatile("" : "+v"(acc[i]));
  issue(0, cell, v);
  // whole pairs of batches, then at most one odd batch: the padding work stays < EB
  // entries (rows of ~40 entries at config 2 would otherwise pad to a multiple of 8)
  const int n4 = (n + EB - 1) & ~(EB - 1);
  int e0 = 0;
  for (; e0 + 2 * EB <= n4; e0 += 2 * EB) {
    issue(e0 + EB, cellb, vb);
    ready(v);
    accumulate(cell, v);
    issue(e0 + 2 * EB, cell, v);
    ready(vb);
    accumulate(cellb, vb);
  }
  if (e0 < n4) {
    issue(e0 + EB, cellb, vb);  // look-ahead slot, unused: keeps the vmcnt bookkeeping uniform
    ready(v);
    accumulate(cell, v);
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(vb[0]), "+v"(vb[1]), "+v"(vb[2]), "+v"(vb[3]));
  }
  // drain the last look-ahead before its registers can be reused
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]));
#else
  load_batch(0, cell, v);
  for (int e0 = 0; e0 < n; e0 += EB) {
    int celln[EB];
    double vn[EB];
    load_batch(e0 + EB, celln, vn);
    accumulate(cell, v);
#pragma unroll
    for (int j = 0; j < EB; ++j) {
      cell[j] = celln[j];
      v[j] = vn[j];
    }
  }
#endif
    }
  // ---- per-boot softmax over the grid: max, exp, sum.  Two block barriers: after the waves'
  // max partials and after their tile partials; every surviving wave then combines the partials
  // itself (the same values in the same order as one combining wave would) into its own LDS
  // row, read back after a wave-level sync -- no second barrier per reduction.
  double* const fm = wfin[wsid];
  if (diag & 8) {  // timing diagnostic: no reductions
    if (lane < NB) fm[lane] = acc[0];
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  } else {
    float* const redf = reinterpret_cast<float*>(red);
#pragma unroll
    for (int i0 = 0; i0 + 16 <= NB; i0 += 16) wave_max_partials<16, NB>(acc, i0, redf, lane, wid);
    if constexpr ((NB % 16) >= 8) wave_max_partials<8, NB>(acc, NB - (NB % 16), redf, lane, wid);
    if constexpr ((NB % 8) >= 4) wave_max_partials<4, NB>(acc, NB - (NB % 8), redf, lane, wid);
    __syncthreads();
    if (lane < NB) {
      float r = -INFINITY;
      for (int w = 0; w < nw; ++w)
        if ((wmask >> w) & 1) r = gt_maxf(r, redf[w * 32 + lane]);
      fm[lane] = (double)r;
    }
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  if (wsid == lw) {
    const bool lb = lane < NB && b0 + lane < nboot;
    // post-check of the left-out stretches against the exact row maxima
    bool fails = false;
    if (smask && lb)
      for (int w = 0; w < nw; ++w)
        if (!((wmask >> w) & 1) && !(sub[((long long)(g * P + p) * kStretchSlots + w) * NB + lane] < fm[lane] - 51.0))
          fails = true;
    const bool flagged = __builtin_amdgcn_ballot_w64(fails) != 0;
    if (flagged && lane == 0) redo[(long long)g * P + p] = 1;
    // a flagged slab's maxima cover the surviving stretches only: the redo pass, with every
    // stretch, decides its degenerate flag
    if (!flagged && lb && !(fabs(fm[lane]) <= degen_thresh)) degen[g] = 1;
  }
  // Softmax terms below e^kBootExpCut (1.9e-22) are dropped: a jp entry loses at most
  // that much (each boot's row sums to >= 1 before the 1/B weighting), far below the
  // 1e-18 absolute floor of SURVEY 8(d)'s tolerance.  Rows are sharply peaked, so for most
  // (wave, boot) pairs no lane of the 64-point stretch is above the cut and the whole
  // wave skips the exp (a wave-uniform branch); inside an active wave the lanes below
  // the cut are zeroed as before.  (k_boot_gene's form -- one branch per wave, all NB boots' terms
  // straight-line -- was tried here as a study build and not kept.)
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const double d = acc[i] - fm[i];
    const bool need = live && d >= kBootExpCut;
    if (diag & 4)  // timing diagnostic: no exp
      acc[i] = live ? d : 0.0;
    else if (__builtin_amdgcn_ballot_w64(need))
      acc[i] = need ? exp_tab(d, etab) : 0.0;
    else
      acc[i] = 0.0;
  }
  if (diag & 8) {
    if (lane < NB) fm[lane] = acc[1];
  } else {
    // per-boot sums from 16-point tile partials added in tile order (row16_sum, the same
    // form as k_boot_tiles): a slab's sums do not depend on which stretches or which
    // kernel computed it (left-out tiles only ever hold terms the cut made zero)
    // The tile sums are row16_sum's: partners lane ^ 1, ^ 2 (the quad), then lane ^ 7 (the other
    // quad of the 8) and lane ^ 15 (the other 8), each step self + partner.  Here the quad steps
    // run as a reduce-scatter over chunks of 4 boots (lane bits 0, 1 pick the boot) and the last
    // two pair the lanes holding the same boot, lane ^ 4 and lane ^ 8 (ds_swizzle): the tile is
    // (Q0 + Q1) + (Q2 + Q3) from the same operand pairs as row16_sum, so the same bits, in 23
    // VALU per 4 boots instead of 48.
    {
      const bool up0 = (lane & 1) != 0, up1 = (lane & 2) != 0;
#pragma unroll
      for (int c = 0; c < NB / 4; ++c) {
        const double x0 = acc[4 * c], x1 = acc[4 * c + 1], x2 = acc[4 * c + 2], x3 = acc[4 * c + 3];
        double k0 = up0 ? x2 : x0, k1 = up0 ? x3 : x1;
        const double s0 = up0 ? x0 : x2, s1 = up0 ? x1 : x3;
        k0 += dpp_d<kDppXor1>(s0);
        k1 += dpp_d<kDppXor1>(s1);
        double kk = up1 ? k1 : k0;
        const double ss = up1 ? k0 : k1;
        kk += dpp_d<kDppXor2>(ss);
        kk += swz_d<0x101F>(kk);  // lane ^ 4
        kk += swz_d<0x201F>(kk);  // lane ^ 8
        if ((lane & 12) == 0) tsum[(4 * wid + (lane >> 4)) * NB + 4 * c + 2 * up0 + up1] = kk;
      }
    }
    __syncthreads();
    if (lane < NB) {
      const int nt = (G + 15) >> 4;
      double r = 0.0;
      for (int t = 0; t < nt; ++t)
        if ((wmask >> (t >> 2)) & 1) r += tsum[t * NB + lane];
      fm[lane] = (b0 + lane < nboot) ? 1.0 / (r * norm_mult) : 0.0;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
  double jpv = 0.0;
#pragma unroll
  for (int i = 0; i < NB; ++i) jpv = fma(acc[i], fm[i], jpv);
  if (live) part[(long long)p * part_stride + (long long)g * GS + tid] = jpv;
}

template <int NB>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(NB <= 20 ? SCDE_BOOT_WPE : 1))) void k_boot2(
    const double* __restrict__ D, const int2* __restrict__ ent,
    const int* __restrict__ nnz, int ent_stride,
    const double* __restrict__ Wt, int Bp, int ncells,
    const int* __restrict__ wset, const double* __restrict__ Z, int G,
    int GS, int P, int nboot, double norm_mult, double degen_thresh,
    double* __restrict__ part, long long part_stride,
    int* __restrict__ degen, int ngenes,
    const int* __restrict__ smask, const double* __restrict__ sub,
    int* __restrict__ redo, int redo_pass) {
  const int within = blockIdx.x % (8 * P);
  const int p = within >> 3;
  const int g = (blockIdx.x / (8 * P)) * 8 + (within & 7);
  if (g >= ngenes) return;
  boot2_slab<NB>(D, ent, nnz, ent_stride, Wt, Bp, ncells, wset, Z, G, GS, P, nboot, norm_mult, degen_thresh, part, part_stride, degen, ngenes, smask, sub, redo, redo_pass, g, p);
}

// k_boot_tiles' fallback: the (gene, slab) items it could not finish, appended to
// list[0 .. *count) (whole slabs, no skipping).  A small grid walks the list, so the usual
// empty fallback costs one short launch, not a block per slab.
// (a rare path: no occupancy target, so the item loop never spills around the asm look-ahead;
// the tile path has G <= 448, blocks of at most 448 threads)
template <int NB>
__global__ __launch_bounds__(512) void k_boot2_list(
    const double* __restrict__ D, const int2* __restrict__ ent, const int* __restrict__ nnz, int ent_stride,
    const double* __restrict__ Wt, int Bp, int ncells, const int* __restrict__ wset, const double* __restrict__ Z,
    int G, int GS, int P, int nboot, double norm_mult, double degen_thresh, double* __restrict__ part,
    long long part_stride, int* __restrict__ degen, int ngenes, const int* __restrict__ count,
    const int* __restrict__ list) {
  const int cnt = __builtin_amdgcn_readfirstlane(*count);
  for (int it = blockIdx.x; it < cnt; it += gridDim.x) {
    const int item = __builtin_amdgcn_readfirstlane(list[it]);
    const int g = item / P, p = item - g * P;
    boot2_slab<NB>(D, ent, nnz, ent_stride, Wt, Bp, ncells, wset, Z, G, GS, P, nboot, norm_mult, degen_thresh, part, part_stride, degen, ngenes, nullptr, nullptr, nullptr, 0, g, p);
    __syncthreads();  // the next item reuses the block's LDS
  }
}

// ------------------------------------------------------------------ baseline tile-bound sums
// ZUq[set][l][t][Bp] = sum over the cells with a baseline column of W8[set][c][b] *
// digit_l(UQ[bc][t]), l < 4: the baseline cells' part of k_boot_tiles' integer tile bounds.
// Block per (set, 32 boots, chunk of kZChunk cells); thread = (bound tile, boot); global atomics
// (exact integers, order-free; ZUq is zeroed first).
constexpr int kZChunk = 64;
__global__ __launch_bounds__(32 * kQTiles) void k_zuq(const unsigned* __restrict__ UQ, const int* __restrict__ base_col,
                                              int ncells, const unsigned char* __restrict__ W8, int Bp,
                                              int* __restrict__ ZUq) {
  const int nch = (ncells + kZChunk - 1) / kZChunk;
  const int t = threadIdx.x >> 5, b = blockIdx.x * 32 + (threadIdx.x & 31), set = blockIdx.y / nch;
  const int c0 = (blockIdx.y % nch) * kZChunk, c1 = min(ncells, c0 + kZChunk);
  const unsigned char* W = W8 + (long long)set * ncells * Bp + b;
  int acc[4] = {0, 0, 0, 0};
  for (int c = c0; c < c1; ++c) {
    const int bc = base_col[c];
    if (bc < 0) continue;
    const int w = W[(long long)c * Bp];
    const unsigned u = UQ[(long long)bc * kQTiles + t];
#pragma unroll
    for (int l = 0; l < 4; ++l) acc[l] += w * (int)(signed char)(u >> (8 * l));
  }
#pragma unroll
  for (int l = 0; l < 4; ++l)
    if (acc[l]) atomicAdd(ZUq + (((long long)set * 4 + l) * kQTiles + t) * Bp + b, acc[l]);
}

// ------------------------------------------------------------------ tile bootstrap
// The tile bootstrap: k_boot2's FP64 bootstrap computed only where it matters.  k_boot_gene
// (below) takes every (gene, slab of NB boots) first, sharing a block's 16 rows among a gene's
// slabs; k_boot_tiles is the list pass behind it, over the slabs whose post-check failed there
// (the list k_boot_gene leaves in `wide`), with a fixed four bound tiles each.  One wave per
// listed slab, four per block; the waves never synchronise with each other.
//   1. bounds UB_bt = ZU_bt + sum_e W_be UQ_et for every boot and 32-point bound tile t (UQ:
//      the tables' per-tile column maxima in units of 2^-8, rounded up; ZU: the baseline
//      cells' part), exact integers on the int8 matrix cores (4 balanced digits), kept in LDS
//      as f32 rounded up;
//   2. the 4 bound tiles with the largest bound over the slab's live boots (8 sum tiles of 16
//      points, 128 points): rows Z_b + sum_e W_be D_e with two grid points per lane, in
//      k_boot2's arithmetic (the same fma chain per (boot, point)); maxima m'_b (f32);
//   3. post-check: every bound tile not computed must have UB_bt < m'_b - 51 for every live
//      boot, else the slab goes whole to k_boot2's fallback launch;
//   4. softmax terms, per-boot sums from 16-point tile partials in tile order, the jp
//      partial row (zeros on the tiles not computed).
// A tile left out has every row value <= UB_bt < m'_b - 51 <= m_b - 50, so all its terms fall
// under the e^-50 cut; maxima, sums and jp rows are therefore bit for bit those of k_boot2
// with every point computed.  Per ELL entry one 16-byte column load (points k0, k0 + 1) and one
// 16-byte multiplicity load (DPP broadcast) feed 2 NB FMAs: these waves are bound by the
// vector-memory instruction rate (the texture addresser), not by the bytes.
constexpr int kTileMax = 28;   // 16-point sum tiles, G <= 448
constexpr int kBTileMax = 14;  // 32-point bound tiles, G <= 448
#ifndef SCDE_TILE_DIAG
#define SCDE_TILE_DIAG 0  // timing builds: 4 = no multiplicity loads,
                          // 8 = every column load from the entry-0 column (cache-resident); k_boot_gene:
                          // 16 = bounds replaced by -inf, 512 = no bound pass, 32 = no row loop, 64 = rows only (no
                          // softmax / sums / rows out), 128 = bound pass loads only, 256 = bound pass without MFMA;
                          // epilogue parts: 1024 = no post-check, 2048 = no per-slab maxima (rows' maxima and
                          // their combine), 4096 = no exps in the softmax, 8192 = no normalisers / partial rows
#endif
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
typedef double d2_t __attribute__((ext_vector_type(2)));

// Logical block of hardware block b under round-robin XCD dispatch (block b runs on XCD
// b % 8): runs of K consecutive logical blocks -- a gene's slabs, and genes adjacent in the
// count-sum order, which share low-count columns -- go to one XCD and run there at about the
// same time, meeting each other's D columns in its L2; the runs rotate over the XCDs, so
// every XCD walks the count-sum order (the work gradient) at the same pace.  Hardware
// blocks g 8K + 8 i + x (x < 8, i < K) take logical g 8K + K x + i; a last partial group
// keeps the identity (a bijection for any n).
#ifndef SCDE_XCD_RUN
#define SCDE_XCD_RUN 16
#endif
__device__ __forceinline__ int xcd_block(int b, int n) {
  constexpr int K = SCDE_XCD_RUN;
  if (K <= 1 || b >= n / (8 * K) * (8 * K)) return b;
  const int r = b % (8 * K);
  return b - r + (r & 7) * K + (r >> 3);
}

// acc += (w on lane J of this lane's 16-lane row) * x, one v_fmac_f64 with a DPP64 source.
// w must come from a load, never from a VALU write in the two preceding instructions (the
// DPP read hazard; tests/test_kernel_resources.py checks the shipped ISA).
template <int J>
__device__ __forceinline__ void fmac_bcast(double& acc, double w, double x) {
  asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(w), "v"(x),
               "n"(J));
}

// A tile's partial sum: the lane's two points, then partners lane^1, ^2 and the 8-lane
// mirror -- the operand pairs of row16_sum over 16 one-point lanes, so the same bits.
__device__ __forceinline__ double pair8_sum(double p0, double p1) {
  double v = p0 + p1;
  v += dpp_d<kDppXor1>(v);
  v += dpp_d<kDppXor2>(v);
  v += dpp_d<kDppHalfMirror>(v);
  return v;
}

// one entry into the two points' NB accumulators: boots 2J, 2J + 1 from lane J of wv
template <int NB, int... J>
__device__ __forceinline__ void fmac_entry2(double (&a0)[NB], double (&a1)[NB], const d2_t& wv, const d2_t& x,
                                            std::integer_sequence<int, J...>) {
  ((fmac_bcast<J>(a0[2 * J], wv.x, x.x), fmac_bcast<J>(a1[2 * J], wv.x, x.y),
    fmac_bcast<J>(a0[2 * J + 1], wv.y, x.x), fmac_bcast<J>(a1[2 * J + 1], wv.y, x.y)),
   ...);
}

#ifndef SCDE_TILE_WPE
// k_boot_tiles occupancy target (waves per SIMD): 2 x NB accumulators (80 VGPRs at NB = 20)
// and two 2-entry load buffers fit 128 VGPRs.  The row loop must not spill: its look-ahead
// registers are written by asm loads the compiler believes complete at once, so a spill or
// copy before the asm wait reads or reuses them early (builds that did faulted on the GPU;
// tests/test_kernel_resources.py checks the shipped ISA for it).
#define SCDE_TILE_WPE 4
#endif
// WB waves per block (4; one item each).  Measured and not kept: a gene's 5 slabs as the 5
// waves of one block (the slabs' column loads did not meet in L1: the same L1 -> L2 request
// count, boot 12.5 -> 14.6 ms at config 4).
// One bound pass (step 1 of k_boot_tiles / k_boot_gene): UB_bt = ZU_bt + sum_e W_be UQ_et for the
// 32 boot slots of one pair-interleaved multiplicity block (boots j and 16 + j in the bytes of pair
// slot j) and every 32-point bound tile t < NTB, exact integers on the int8 matrix cores (C layout
// of the 16x16x64 MFMA: bound tile r, boots 16 bt + 4 h + q), written rounded up to f32 as
// ub[t * ustride + b] for b < nbout.  W8: cell 0's block (cell c at W8 + c * cstride); ZU: the
// baseline digit sums of boot slot 0 (digit l, tile t at ZU + (l * kQTiles + t) * Bq); stage: the
// wave's 1536-word LDS area.  Per 64-entry chunk each lane loads one entry's data with wide loads
// -- its (cell, column), the column's 16 tile bounds (64 B) and the cell's 16 multiplicity pairs
// (32 B) -- and writes them transposed into the staging area; the MFMA fragments are then
// contiguous LDS reads: 7 vector-memory instructions per chunk instead of 40 single-entry gathers.
__device__ __forceinline__ void tile_bound_pass(const int2* __restrict__ E, int n, const unsigned* __restrict__ UQ,
                                                const unsigned char* __restrict__ W8, unsigned cstride,
                                                const int* __restrict__ ZU, int Bq, unsigned* stage, float* ub,
                                                int ustride, int nbout, int NTB, int lane) {
  const int r = lane & 15, h = lane >> 4;
  unsigned* sq = stage;         // [tile t][entry l] tile bounds (64 x 16 words)
  unsigned* sw = stage + 1024;  // [pair r][entry l / 2] multiplicity pairs (two entries a word)
  const int KP = (n + 63) & ~63;
  const int t = r;
  i32x4 acc[2][4];
#pragma unroll
  for (int bt = 0; bt < 2; ++bt)
#pragma unroll
    for (int l = 0; l < 4; ++l)
      acc[bt][l] = *reinterpret_cast<const i32x4*>(ZU + ((long long)l * kQTiles + t) * Bq + 16 * bt + 4 * h);
  for (int e0 = 0; e0 < KP; e0 += 64) {
    const int2 en = E[e0 + lane];  // rows are padded to a multiple of 64 (+ 8): pad entries read column ncols
    const uint4* uq = reinterpret_cast<const uint4*>(UQ + (unsigned)(en.y * kQTiles));
    const uint4 q0 = uq[0], q1 = uq[1], q2 = uq[2], q3 = uq[3];
    const uint4* wp = reinterpret_cast<const uint4*>(W8 + (unsigned)(en.x * cstride));
    const uint4 w0 = wp[0], w1 = wp[1];
    if (SCDE_TILE_DIAG & 128) {  // timing build: the chunk's loads only (results wrong)
      acc[0][0][0] += (int)(q0.x ^ q1.y ^ q2.z ^ q3.w ^ w0.x ^ w1.w);
      continue;
    }
    wave_sync();  // the previous chunk's fragment reads are done before the area is rewritten
    const unsigned qv[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                             q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
#pragma unroll
    for (int tt = 0; tt < 16; ++tt) sq[tt * 64 + lane] = qv[tt];
    // pairs (boot j, boot 16 + j) as 16-bit words: two entries per 32-bit LDS word
    const unsigned wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    unsigned short* sw16 = reinterpret_cast<unsigned short*>(sw);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sw16[(2 * j) * 64 + lane] = (unsigned short)(wv[j] & 0xffffu);
      sw16[(2 * j + 1) * 64 + lane] = (unsigned short)(wv[j] >> 16);
    }
    wave_sync();
    // B fragment: tile t's words of entries 16 h .. 16 h + 15
    const uint4* bq = reinterpret_cast<const uint4*>(sq + t * 64 + 16 * h);
    const uint4 b0v = bq[0], b1v = bq[1], b2v = bq[2], b3v = bq[3];
    const unsigned u[16] = {b0v.x, b0v.y, b0v.z, b0v.w, b1v.x, b1v.y, b1v.z, b1v.w,
                            b2v.x, b2v.y, b2v.z, b2v.w, b3v.x, b3v.y, b3v.z, b3v.w};
    // A fragments: pair r of entries 16 h .. 16 h + 15 (two entries a word)
    const uint4* aw = reinterpret_cast<const uint4*>(sw + r * 32 + 8 * h);
    const uint4 a0v = aw[0], a1v = aw[1];
    const unsigned x2[8] = {a0v.x, a0v.y, a0v.z, a0v.w, a1v.x, a1v.y, a1v.z, a1v.w};
    i32x4 af[2];
    unsigned lo4[4], hi4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      lo4[q] = __builtin_amdgcn_perm(x2[2 * q + 1], x2[2 * q], 0x06040200u);
      hi4[q] = __builtin_amdgcn_perm(x2[2 * q + 1], x2[2 * q], 0x07050301u);
    }
    af[0] = i32x4{(int)lo4[0], (int)lo4[1], (int)lo4[2], (int)lo4[3]};
    af[1] = i32x4{(int)hi4[0], (int)hi4[1], (int)hi4[2], (int)hi4[3]};
    unsigned pl[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      tr4(u[4 * q], u[4 * q + 1], u[4 * q + 2], u[4 * q + 3], pl[0][q], pl[1][q], pl[2][q], pl[3][q]);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const i32x4 bf = {(int)pl[l][0], (int)pl[l][1], (int)pl[l][2], (int)pl[l][3]};
      if (SCDE_TILE_DIAG & 256) {  // timing build: loads and LDS staging, no MFMA (results wrong)
        acc[0][l][0] += bf[0] ^ af[0][1];
        acc[1][l][1] += bf[2] ^ af[1][3];
      } else {
        acc[0][l] = mfma_i8(af[0], bf, acc[0][l]);
        acc[1][l] = mfma_i8(af[1], bf, acc[1][l]);
      }
    }
  }
  if (t < NTB)
#pragma unroll
    for (int bt = 0; bt < 2; ++bt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int b = 16 * bt + 4 * h + q;
        if (b < nbout) {
          const long long v =
              (((long long)acc[bt][3][q] * 256 + acc[bt][2][q]) * 256 + acc[bt][1][q]) * 256 + acc[bt][0][q];
          const double x = (double)v * 0x1p-8;
          float f = (float)x;
          if ((double)f < x) f = nextafterf(f, INFINITY);
          ub[t * ustride + b] = f;
        }
      }
}

// tile_bound_pass over the 64-entry chunks c0, c0 + cstep, ... only and without the baseline part:
// the combined digit sums of each (tile t, boot b < nbout) are added into dsum[t * 32 + b] (int64,
// exact: the bound is linear in the digit sums, so the waves' partial values add up to the full one)
__device__ __forceinline__ void tile_bound_partial(const int2* __restrict__ E, int n, const unsigned* __restrict__ UQ,
                                                const unsigned char* __restrict__ W8, unsigned cstride,
                                                int c0, int cstep, unsigned* stage, long long* dsum, int nbout,
                                                int NTB, int lane) {
  const int r = lane & 15, h = lane >> 4;
  unsigned* sq = stage;         // [tile t][entry l] tile bounds (64 x 16 words)
  unsigned* sw = stage + 1024;  // [pair r][entry l / 2] multiplicity pairs (two entries a word)
  const int KP = (n + 63) & ~63;
  const int t = r;
  i32x4 acc[2][4];
#pragma unroll
  for (int bt = 0; bt < 2; ++bt)
#pragma unroll
    for (int l = 0; l < 4; ++l)
      acc[bt][l] = i32x4{0, 0, 0, 0};
  for (int e0 = 64 * c0; e0 < KP; e0 += 64 * cstep) {
    const int2 en = E[e0 + lane];  // rows are padded to a multiple of 64 (+ 8): pad entries read column ncols
    const uint4* uq = reinterpret_cast<const uint4*>(UQ + (unsigned)(en.y * kQTiles));
    const uint4 q0 = uq[0], q1 = uq[1], q2 = uq[2], q3 = uq[3];
    const uint4* wp = reinterpret_cast<const uint4*>(W8 + (unsigned)(en.x * cstride));
    const uint4 w0 = wp[0], w1 = wp[1];
    wave_sync();  // the previous chunk's fragment reads are done before the area is rewritten
    const unsigned qv[16] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w,
                             q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z, q3.w};
#pragma unroll
    for (int tt = 0; tt < 16; ++tt) sq[tt * 64 + lane] = qv[tt];
    // pairs (boot j, boot 16 + j) as 16-bit words: two entries per 32-bit LDS word
    const unsigned wv[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
    unsigned short* sw16 = reinterpret_cast<unsigned short*>(sw);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      sw16[(2 * j) * 64 + lane] = (unsigned short)(wv[j] & 0xffffu);
      sw16[(2 * j + 1) * 64 + lane] = (unsigned short)(wv[j] >> 16);
    }
    wave_sync();
    // B fragment: tile t's words of entries 16 h .. 16 h + 15
    const uint4* bq = reinterpret_cast<const uint4*>(sq + t * 64 + 16 * h);
    const uint4 b0v = bq[0], b1v = bq[1], b2v = bq[2], b3v = bq[3];
    const unsigned u[16] = {b0v.x, b0v.y, b0v.z, b0v.w, b1v.x, b1v.y, b1v.z, b1v.w,
                            b2v.x, b2v.y, b2v.z, b2v.w, b3v.x, b3v.y, b3v.z, b3v.w};
    // A fragments: pair r of entries 16 h .. 16 h + 15 (two entries a word)
    const uint4* aw = reinterpret_cast<const uint4*>(sw + r * 32 + 8 * h);
    const uint4 a0v = aw[0], a1v = aw[1];
    const unsigned x2[8] = {a0v.x, a0v.y, a0v.z, a0v.w, a1v.x, a1v.y, a1v.z, a1v.w};
    i32x4 af[2];
    unsigned lo4[4], hi4[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      lo4[q] = __builtin_amdgcn_perm(x2[2 * q + 1], x2[2 * q], 0x06040200u);
      hi4[q] = __builtin_amdgcn_perm(x2[2 * q + 1], x2[2 * q], 0x07050301u);
    }
    af[0] = i32x4{(int)lo4[0], (int)lo4[1], (int)lo4[2], (int)lo4[3]};
    af[1] = i32x4{(int)hi4[0], (int)hi4[1], (int)hi4[2], (int)hi4[3]};
    unsigned pl[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
      tr4(u[4 * q], u[4 * q + 1], u[4 * q + 2], u[4 * q + 3], pl[0][q], pl[1][q], pl[2][q], pl[3][q]);
#pragma unroll
    for (int l = 0; l < 4; ++l) {
      const i32x4 bf = {(int)pl[l][0], (int)pl[l][1], (int)pl[l][2], (int)pl[l][3]};
      acc[0][l] = mfma_i8(af[0], bf, acc[0][l]);
      acc[1][l] = mfma_i8(af[1], bf, acc[1][l]);
    }
  }
  if (t < NTB)
#pragma unroll
    for (int bt = 0; bt < 2; ++bt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int b = 16 * bt + 4 * h + q;
        if (b < nbout) {
          const long long v =
              (((long long)acc[bt][3][q] * 256 + acc[bt][2][q]) * 256 + acc[bt][1][q]) * 256 + acc[bt][0][q];
          atomicAdd(reinterpret_cast<unsigned long long*>(&dsum[t * 32 + b]), (unsigned long long)v);
        }
      }
}

// The rows of k_boot_tiles / k_boot_gene: a0/a1[i] = Z_b + sum_e W_be D_e at points k0, k0 + 1 of
// boot b = b0 + i (k0 even: 16-byte aligned pairs; -inf where the point is dead).  Per ELL entry
// one 16-byte column load (both points) and one 16-byte multiplicity load (boots 2J, 2J + 1 on
// lane J of each 16-lane row), then 2 NB v_fmac_f64_dpp row_newbcast:J; loads are issued from
// inline asm in saddr form one batch (2 entries) ahead and waited with an explicit vmcnt, over
// two register buffers.  Each 16-lane row may belong to another slab (b0) and tile (k0).
template <int NB>
__device__ __forceinline__ void tile_rows(double (&a0)[NB], double (&a1)[NB], const double* __restrict__ D,
                                          const int2* __restrict__ E, int n, const double* __restrict__ W,
                                          const double* __restrict__ Zs, int GS, int Bp, int b0, int k0, int r,
                                          bool live, bool l0, bool l1) {
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const d2_t z = live ? *reinterpret_cast<const d2_t*>(Zs + (long long)(b0 + i) * GS + k0) : d2_t{0.0, 0.0};
    a0[i] = l0 ? z.x : -INFINITY;
    a1[i] = l1 ? z.y : -INFINITY;
  }
  {
    constexpr int EB2 = 2;  // entries per batch: 2 x (column pair + multiplicity pair) loads
    const unsigned doff = (unsigned)k0 * 8u;
    const unsigned woff = (unsigned)(b0 + 2 * min(r, NB / 2 - 1)) * 8u;
    d2_t v[EB2], vb[EB2], w[EB2], wb[EB2];
    auto fetch = [&](int e0, int4& t) { t = *reinterpret_cast<const int4*>(E + e0); };
    const int col0 = __builtin_amdgcn_readfirstlane(E[0].y);  // timing build 8: every load from this column
    (void)col0;
    auto issue = [&](int4 t, d2_t (&x)[EB2], d2_t (&wv)[EB2]) {
      asm volatile("" : "+s"(t.x), "+s"(t.y), "+s"(t.z), "+s"(t.w));
      // 32-bit offsets: (ncols + 1) x GS and ncells x Bp are < 2^31 (checked by the launcher)
      const double* d0 = D + (unsigned)(((SCDE_TILE_DIAG & 8) ? col0 : t.y) * GS);
      const double* d1 = D + (unsigned)(((SCDE_TILE_DIAG & 8) ? col0 : t.w) * GS);
      const double* w0 = W + (unsigned)(t.x * Bp);
      const double* w1 = W + (unsigned)(t.z * Bp);
      asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(x[0]) : "v"(doff), "s"(d0));
      if (!(SCDE_TILE_DIAG & 4)) asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(wv[0]) : "v"(woff), "s"(w0));
      asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(x[1]) : "v"(doff), "s"(d1));
      if (!(SCDE_TILE_DIAG & 4)) asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(wv[1]) : "v"(woff), "s"(w1));
    };
    auto ready = [&](d2_t (&x)[EB2], d2_t (&wv)[EB2]) {  // all but the next batch's loads have landed
      if (SCDE_TILE_DIAG & 4)  // timing build: multiplicities loaded once (results wrong)
        asm volatile("s_waitcnt vmcnt(2)" : "+v"(x[0]), "+v"(x[1]), "+v"(wv[0]), "+v"(wv[1]));
      else
        asm volatile("s_waitcnt vmcnt(4)" : "+v"(x[0]), "+v"(x[1]), "+v"(wv[0]), "+v"(wv[1]));
    };
    auto accumulate = [&](const d2_t (&x)[EB2], const d2_t (&wv)[EB2]) {
#pragma unroll
      for (int j = 0; j < EB2; ++j)
        fmac_entry2<NB>(a0, a1, wv[j], x[j], std::make_integer_sequence<int, NB / 2>{});
    };
#pragma unroll
    for (int i = 0; i < NB; ++i) asm volatile("" : "+v"(a0[i]), "+v"(a1[i]));
    // rows are padded to a multiple of 64 entries plus 8 zero-column entries: every fetch and
    // look-ahead batch stays inside the row
    int4 ta, tb;
    fetch(0, ta);
    if (SCDE_TILE_DIAG & 4) {  // timing build: the first entry's multiplicities for every entry
      const double* w0 = W + (unsigned)(ta.x * Bp);
      w[0] = w[1] = wb[0] = wb[1] = *reinterpret_cast<const d2_t*>(w0 + woff / 8);
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(w[0]), "+v"(w[1]), "+v"(wb[0]), "+v"(wb[1]));
    }
    issue(ta, v, w);
    fetch(EB2, tb);
    const int n2 = (n + EB2 - 1) & ~(EB2 - 1);
    int e0 = 0;
    for (; e0 + 2 * EB2 <= n2; e0 += 2 * EB2) {
      issue(tb, vb, wb);
      fetch(e0 + 2 * EB2, ta);
      ready(v, w);
      accumulate(v, w);
      issue(ta, v, w);
      fetch(e0 + 3 * EB2, tb);
      ready(vb, wb);
      accumulate(vb, wb);
    }
    if (e0 < n2) {
      issue(tb, vb, wb);
      ready(v, w);
      accumulate(v, w);
      asm volatile("s_waitcnt vmcnt(0)" : "+v"(vb[0]), "+v"(vb[1]), "+v"(wb[0]), "+v"(wb[1]));
    }
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(v[0]), "+v"(v[1]), "+v"(w[0]), "+v"(w[1]));
  }
}

template <int NB, int WB>
__global__ __launch_bounds__(64 * WB) __attribute__((amdgpu_waves_per_eu(SCDE_TILE_WPE))) void k_boot_tiles(
    const double* __restrict__ D, const int2* __restrict__ ent, const int* __restrict__ nnz, int ent_stride,
    const double* __restrict__ Wt, int Bp, int ncells, const int* __restrict__ wset, const double* __restrict__ Z,
    int G, int GS, int P, int nboot, double norm_mult, double degen_thresh, double* __restrict__ part,
    long long part_stride, int* __restrict__ degen, int ngenes, const unsigned char* __restrict__ W8p, int Bq,
    const unsigned* __restrict__ UQ, const int* __restrict__ ZUq, const int* __restrict__ nanflag, int maxgroups,
    int* __restrict__ redo, int* __restrict__ stats, unsigned* __restrict__ pmask,
    const int* __restrict__ slab_list) {
  static_assert(NB % 4 == 0 && NB <= 20, "NB must be a multiple of 4, <= 20");
  __shared__ float ubs[WB][kBTileMax * NB];  // [wave][bound tile][boot] the slab's bounds
#ifdef SCDE_TILE_TEST_WB1
  __shared__ unsigned bstage[WB][64];  // hazard-test builds: the LDS that would cap occupancy (never run)
#else
  __shared__ unsigned bstage[WB][1024 + 512];  // [wave] bound staging: 16 x 64 tile words | 16 x 32 pair words
#endif
  __shared__ float fmx[WB][32];  // [wave][boot] maxima
  __shared__ double etab[64];
  const int lane = threadIdx.x & 63;
  const int wsid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // slab_list: [0] the number of items, [1 + i] item i = gene * P + slab.  Blocks past the list's
  // end leave before the block barrier (the pass is launched for the longest list the gene
  // blocks may build; most of its blocks find no item)
  if (xcd_block(blockIdx.x, gridDim.x) * WB >= slab_list[0]) return;
  if (threadIdx.x < 64) etab[threadIdx.x] = kExp2Frac64[threadIdx.x];
  __syncthreads();
  // the bound staging area, once the bound loop is done: tile partial sums [slot][boot] |
  // 1 / (S nboot) [boot] (the shipped 4-wave block stays under 40 KB of LDS: four blocks, 16
  // waves per CU)
#ifndef SCDE_TILE_TEST_WB1
  static_assert(2 * (8 * NB + NB) <= (int)(sizeof(bstage[0]) / 4),
                "the staging area must hold the tile sums and the normalisers");
#endif
  double* const tsum = reinterpret_cast<double*>(&bstage[wsid][0]);
  double* const finv = tsum + 8 * NB;
  // ---- the wave's item: one slab a gene block could not finish
  const int idx = xcd_block(blockIdx.x, gridDim.x) * WB + wsid;
  if (idx >= slab_list[0]) return;
  const int it = slab_list[1 + idx];
  const int g = it / P, p = it - g * P;
  if (*nanflag) {  // a NaN in some table: k_boot2 computes every slab
    if (lane == 0) {
      const int q = (long long)g * P + p;
      redo[q] = 1;
      redo[(long long)ngenes * P + 1 + atomicAdd(&redo[(long long)ngenes * P], 1)] = q;
      pmask[q] = ~0u;
    }
    return;
  }
  const int n = nnz[g];
  const int NT = (G + 15) >> 4, NTB = (G + 31) >> 5;  // 16-point sum tiles, 32-point bound tiles
  const int r = lane & 15;
  const int2* __restrict__ E = ent + (long long)g * ent_stride;
  const int set = wset ? wset[g] : 0;
  const int b0 = p * NB;
  // ---- 1. bound tiles (C layout of the 16x16x64 MFMA: bound tile r, boots 16 bt + 4 h + q).  Per
  // 64-entry chunk each lane loads one entry's data with wide loads -- its (cell, column), the
  // column's 16 tile bounds (64 B) and the cell's 16 multiplicity pairs of this slab (32 B) --
  // and writes them transposed into the wave's LDS area; the MFMA fragments are then contiguous
  // LDS reads: 7 vector-memory instructions per chunk instead of 40 single-entry gathers.
  {
    const unsigned pstride = 32u * (unsigned)P;
    const unsigned char* __restrict__ W8 = W8p + (long long)set * ncells * pstride + 32 * p;
    const int* __restrict__ ZU = ZUq + (long long)set * 4 * kQTiles * Bq + b0;
    tile_bound_pass(E, n, UQ, W8, pstride, ZU, Bq, &bstage[wsid][0], ubs[wsid], NB, NB, NTB, lane);
  }
  wave_sync();
  const int nlive = min(NB, nboot - b0);
  // ---- 2. the four bound tiles with the largest bound over the slab's live boots (maxgroups:
  // the tests force the fallback with fewer); all of them when the grid has no more
  float sc = -INFINITY;
  if (lane < NTB)
    for (int b = 0; b < nlive; ++b) sc = fmaxf(sc, ubs[wsid][lane * NB + b]);
  const int nsel = min(max(1, min(maxgroups, 4)), NTB);
  int tl[4] = {0, 0, 0, 0};
  unsigned bd = 0;  // bound tiles computed
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (j < nsel) {
      // the 16 bound-tile scores sit in lanes 0..15: a 16-lane DPP max, read back from lane 0
      float m = sc;
      m = fmaxf(m, dpp_f<kDppXor1>(m));
      m = fmaxf(m, dpp_f<kDppXor2>(m));
      m = fmaxf(m, dpp_f<kDppHalfMirror>(m));
      m = fmaxf(m, dpp_f<kDppMirror>(m));
      m = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(m)));
      const unsigned long long bl = __ballot(lane < NTB && !((bd >> lane) & 1) && sc == m);
      const int t = __ffsll((long long)bl) - 1;
      tl[j] = t;
      bd |= 1u << t;
      if (lane == t) sc = -INFINITY;
    }
  }
  // the 16-point sum tiles of the computed bound tiles
  const unsigned ntmask = (NT >= 32) ? ~0u : ((1u << NT) - 1);
  unsigned done = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < nsel) done |= 3u << (2 * tl[j]);
  done &= ntmask;
  // lane l: row l >> 4 = one bound tile; sum tile slot l >> 3 (its half l >> 3 & 1)
  const int slot = lane >> 3, m2 = lane & 7, row = lane >> 4;
  int mybt = tl[0];
#pragma unroll
  for (int j = 1; j < 4; ++j) mybt = (row == j) ? tl[j] : mybt;
  const int mytile = 2 * mybt + (slot & 1);
  const int k0 = 16 * mytile + 2 * m2;
  const bool live = row < nsel;
  const bool l0 = live && k0 < G, l1 = live && k0 + 1 < G;
  const double* __restrict__ W = Wt + (long long)set * ncells * Bp;
  const double* __restrict__ Zs = Z + (long long)set * Bp * GS;
  // ---- rows: Z_b + sum_e W_be D_e at points k0, k0 + 1 (k0 even: 16-byte aligned pairs)
  double a0[NB], a1[NB];
  tile_rows<NB>(a0, a1, D, E, n, W, Zs, GS, Bp, b0, k0, r, live, l0, l1);
  // the slab's maxima m'_b (f32) over the wave's lanes -> fmx[wsid]
  {
    double mx[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) mx[i] = gt_max(a0[i], a1[i]);
    wave_max_partials_all<NB>(mx, &fmx[0][0], lane, wsid);
  }
  wave_sync();
  // ---- 3. post-check: every bound tile not computed stays below the exact maxima minus 51; a
  // slab that fails goes whole to k_boot2's fallback launch
  bool need = false;
  if (lane < NTB && !((bd >> lane) & 1))
    for (int b = 0; b < nlive; ++b) need |= (double)ubs[wsid][lane * NB + b] >= (double)fmx[wsid][b] - 51.0;
  const bool fail = __ballot(need) != 0;
  if (fail && lane == 0) {
    const int q = g * P + p;
    redo[q] = 1;
    redo[(long long)ngenes * P + 1 + atomicAdd(&redo[(long long)ngenes * P], 1)] = q;
    pmask[q] = ~0u;
    if (stats) {
      atomicAdd(&stats[3], 1);
      atomicAdd(&stats[5], (n + 3) & ~3);
    }
  }
  if (stats && lane == 0) atomicAdd(&stats[4], 2 * ((n + 1) & ~1));  // 128 points = two 64-lane groups' FMAs
  if (fail) return;
  if (lane == 0)
    for (int b = 0; b < nlive; ++b)
      if (!(fabs((double)fmx[wsid][b]) <= degen_thresh)) degen[g] = 1;
  // ---- 4. softmax terms, tile partial sums, jp partial rows
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const double m = (double)fmx[wsid][i];
    const double d0 = a0[i] - m, d1 = a1[i] - m;
    const bool n0 = l0 && d0 >= kBootExpCut, n1 = l1 && d1 >= kBootExpCut;
    if (__builtin_amdgcn_ballot_w64(n0 || n1)) {
      a0[i] = n0 ? exp_tab(d0, etab) : 0.0;
      a1[i] = n1 ? exp_tab(d1, etab) : 0.0;
    } else {
      a0[i] = 0.0;
      a1[i] = 0.0;
    }
    const double ps = pair8_sum(a0[i], a1[i]);
    if (m2 == 0 && live) tsum[slot * NB + i] = ps;
  }
  wave_sync();
  if (lane < NB) {  // lane b: boot b's sum S over the slab's tiles in tile order
    double S = 0.0;
    for (unsigned mm = done; mm; mm &= mm - 1) {
      const int t = __builtin_ffs((int)mm) - 1;
      int sslot = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (tl[j] == (t >> 1) && j < nsel) sslot = 2 * j + (t & 1);
      S += tsum[sslot * NB + lane];
    }
    finv[lane] = (b0 + lane < nboot) ? 1.0 / (S * norm_mult) : 0.0;
  }
  wave_sync();
  {
    double* prow = part + (long long)p * part_stride + (long long)g * GS;
    double j0 = 0.0, j1 = 0.0;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      j0 = fma(a0[i], finv[i], j0);
      j1 = fma(a1[i], finv[i], j1);
    }
    if (l1)
      *reinterpret_cast<d2_t*>(prow + k0) = d2_t{j0, j1};
    else if (l0)
      prow[k0] = j0;
  }
  // tiles not computed stay unwritten: k_sum_partials reads only the tiles in pmask
  if (lane == 0) {
    pmask[(long long)g * P + p] = done;
    if (stats) {
      atomicAdd(&stats[0], 1);
      atomicAdd(&stats[1], __builtin_popcount(done));
      atomicAdd(&stats[2], NT);
      atomicAdd(&stats[6 + __builtin_popcount(done)], 1);
    }
  }
}

// ------------------------------------------------------------------ gene-block tile bootstrap
// k_boot_gene: the tile bootstrap's first pass, one 4-wave block per (gene, group of up to SG
// slabs).  At config 3 a slab needs about three of its thirteen 32-point bound tiles (DESIGN.md
// §4.0: 2: 19%, 3: 79%, 4: 2%), so a fixed four tiles per slab (k_boot_tiles' plan) would compute
// 25% more rows than needed.  Here the block's 16 rows (4 waves x 4 sixteen-lane rows, each one
// (slab, bound tile)) are shared by the group's slabs:
//   1. bounds: wave w computes the group's boot window 32 w .. 32 w + 31 (tile_bound_pass;
//      4 windows = 128 boots >= 5 slabs x 20: one bound pass per 32 boots, not per 20) into LDS;
//   2. plan: per slab its bound tiles ranked by their largest bound over the live boots; every
//      slab gets its top K = min(4, 16 / slabs) tiles, the spare rows the next-ranked tiles of the
//      slabs whose next bound is closest to their top bound (at 5 slabs: 3 each plus one spare);
//   3. rows (tile_rows: each 16-lane row its own slab's multiplicities by DPP64 broadcast and its
//      own tile's points), per-row f32 maxima, per-slab maxima m'_b over the slab's rows;
//   4. post-check per slab exactly as k_boot_tiles (every bound tile not computed must have
//      UB_bt < m'_b - 51 for every live boot); a slab that fails goes to the four-tile list pass
//      (k_boot_tiles over `wide`), whose failures go to k_boot2;
//   5. softmax terms, 16-point tile partials (pair8_sum), per (slab, boot) sums over the slab's
//      computed tiles in tile order, 1 / (S nboot), the partial jp rows.
// Every value is formed exactly as in k_boot_tiles and k_boot2 (same fma chains, maxima, terms,
// tile partials added in tile order), so the outputs are bit-identical to theirs.
// Per 16-lane row, the f32 maxima of N values per lane, as a reduce-scatter by recursive
// halving: lane bits 3, 2, 1, 0 split the index range in turn (partners lane ^ 15, lane ^ 7 by
// row_mirror / row_half_mirror, lane ^ 2, lane ^ 1 by quad_perm), a keep/send select per value and
// step.  (N + 1) / 2 + ... + 2 maxima per lane instead of 4 N; max is exact, so every lane's
// values are the maxima any other order gives.  Lane bits b3..b0 then hold index
// j + H4 b0 + H3 b1 + H2 b2 + H1 b3 in slot j < H4 (H1 = ceil(N / 2), H2 = ceil(H1 / 2), ...),
// where row_scatter_index says it is valid.
template <int N, int CTRL>
__device__ __forceinline__ void row_halve_f(float (&v)[32], bool up) {
  constexpr int H = (N + 1) / 2;
#pragma unroll
  for (int j = 0; j < H; ++j) {
    const float lo = v[j], hi = (j + H < N) ? v[j + H] : -INFINITY;
    v[j] = gt_maxf(up ? hi : lo, dpp_f<CTRL>(up ? lo : hi));
  }
}
template <int N>
__device__ __forceinline__ void row_max_scatter_f(float (&v)[32], int r) {
  constexpr int H1 = (N + 1) / 2, H2 = (H1 + 1) / 2, H3 = (H2 + 1) / 2;
  row_halve_f<N, kDppMirror>(v, (r & 8) != 0);
  row_halve_f<H1, kDppHalfMirror>(v, (r & 4) != 0);
  row_halve_f<H2, kDppXor2>(v, (r & 2) != 0);
  row_halve_f<H3, kDppXor1>(v, (r & 1) != 0);
}
// the index held in slot j of row lane r after row_max_scatter_f<N>, or -1
template <int N>
__device__ __forceinline__ int row_scatter_index(int r, int j) {
  constexpr int H1 = (N + 1) / 2, H2 = (H1 + 1) / 2, H3 = (H2 + 1) / 2, H4 = (H3 + 1) / 2;
  const int p4 = j + H4 * (r & 1), p3 = p4 + H3 * ((r >> 1) & 1), p2 = p3 + H2 * ((r >> 2) & 1),
            p1 = p2 + H1 * ((r >> 3) & 1);
  return (j < H4 && p4 < H3 && p3 < H2 && p2 < H1 && p1 < N) ? p1 : -1;
}

// The quad partials of pair8_sum for N values per lane as a reduce-scatter with its operand pairs
// (the lane's two points, then lane ^ 1, lane ^ 2, each sum self + partner: the same bits): lane
// bits 0, 1 split the index range in turn.  Slot j of lane m (bits b1 b0) then holds index
// j + H2 b1 + H1 b0 where pair_scatter_index says it is valid.  pair8_sum's last step (lane ^ 7:
// the other quad of the 8 lanes) pairs lanes holding different indices here, so it is left to the
// reader: tile partial = quad 0 + quad 1, the same two operands.
template <int N, int CTRL>
__device__ __forceinline__ void pair_halve(double (&v)[32], bool up) {
  constexpr int H = (N + 1) / 2;
#pragma unroll
  for (int j = 0; j < H; ++j) {
    const double lo = v[j], hi = (j + H < N) ? v[j + H] : 0.0;
    v[j] = (up ? hi : lo) + dpp_d<CTRL>(up ? lo : hi);
  }
}
template <int N>
__device__ __forceinline__ void pair4_scatter(double (&v)[32], int m) {
  constexpr int H1 = (N + 1) / 2;
  pair_halve<N, kDppXor1>(v, (m & 1) != 0);
  pair_halve<H1, kDppXor2>(v, (m & 2) != 0);
}
template <int N>
__device__ __forceinline__ int pair_scatter_index(int m, int j) {
  constexpr int H1 = (N + 1) / 2, H2 = (H1 + 1) / 2;
  const int p2 = j + H2 * ((m >> 1) & 1), p1 = p2 + H1 * (m & 1);
  return (j < H2 && p2 < H1 && p1 < N) ? p1 : -1;
}

constexpr int kGeneSlabs = 8;     // slabs per group at most (K >= 2 rows each)
// WB waves per block: the launcher instantiates 4 only.  The kernel text still accepts 3 (12
// rows for 5 slabs, for wide calls whose slabs mostly need two tiles): the fourth 32-boot bound
// window is then split by entry chunks over the three waves (tile_bound_partial, exact int64
// sums in LDS), so no wave does two passes.  No build instantiates that form.
template <int NB, int WB>
__global__ __launch_bounds__(64 * WB) __attribute__((amdgpu_waves_per_eu(SCDE_TILE_WPE))) void k_boot_gene(
    const double* __restrict__ D, const int2* __restrict__ ent, const int* __restrict__ nnz, int ent_stride,
    const double* __restrict__ Wt, int Bp, int ncells, const int* __restrict__ wset, const double* __restrict__ Z,
    int G, int GS, int P, int SG, int nboot, double norm_mult, double degen_thresh, double* __restrict__ part,
    long long part_stride, int* __restrict__ degen, int ngenes, const unsigned char* __restrict__ W8g, int Bq,
    const unsigned* __restrict__ UQ, const int* __restrict__ ZUq, const int* __restrict__ nanflag, int maxgroups,
    int kcap, int* __restrict__ redo, int* __restrict__ stats, const int* __restrict__ order,
    unsigned* __restrict__ pmask, int* __restrict__ wide, int wide_cap, int blk0, double* __restrict__ out,
    long long out_g, long long out_k, int* __restrict__ gdone) {
  static_assert(NB % 4 == 0 && NB <= 20, "NB must be a multiple of 4, <= 20");
  static_assert(WB == 3 || WB == 4, "3 or 4 waves per gene block");
  constexpr int kGeneRows = 4 * WB;
  // bound staging of the waves; once the bounds are in gub: row maxima | tile sums | 1 / (S nboot)
  __shared__ unsigned bstage[WB][1024 + 512];
  __shared__ long long dsum[WB < 4 ? kBTileMax * 32 : 1];  // the split window's partial bounds
  __shared__ float gub[kBTileMax * 128];          // [bound tile][group boot] bounds
  __shared__ float sc[kGeneSlabs][16];            // [slab][bound tile] score
  __shared__ signed char rk[kGeneSlabs][16];      // [slab][rank] bound tile
  __shared__ signed char rowof[kGeneSlabs][16];   // [slab][bound tile] the row computing it, or -1
  __shared__ int rowS[kGeneRows], rowT[kGeneRows];  // [row] slab in the group (-1: no work), bound tile
  __shared__ double fmx[kGeneSlabs][32];          // [slab][boot] maxima m'_b (f32 values)
  __shared__ unsigned bd[kGeneSlabs];             // [slab] bound tiles computed
  __shared__ unsigned failm;                      // slabs whose post-check failed
  __shared__ double etab[64];
  static_assert(kGeneRows * 32 + 2 * (4 * kGeneRows * NB) + 2 * kGeneSlabs * 32 <= WB * (1024 + 512),
                "the staging area must hold the row maxima, tile sums and normalisers");
  float* const rowmax = reinterpret_cast<float*>(&bstage[0][0]);                  // [row][32]
  double* const tsum = reinterpret_cast<double*>(&bstage[0][0] + kGeneRows * 32);  // [sum slot][quad][NB]
  double* const finv = tsum + 4 * kGeneRows * NB;                                 // [slab][32]
  const int lane = threadIdx.x & 63;
  const int wsid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int NGR = (P + SG - 1) / SG;
  const int blk = blk0 + xcd_block(blockIdx.x, gridDim.x);  // blk0: this launch's first block (chunked grids)
  if (blk >= ngenes * NGR) return;  // uniform over the block
  const int gi = blk / NGR, gr = blk - gi * NGR;
  const int g = order ? order[gi] : gi;
  const int s0 = gr * SG, ns = min(SG, P - s0);
  // direct rows (gdone: one block per gene, the slabs' rows fit the staging area): a gene whose
  // slabs all pass their post-checks writes its jp row itself, summed over the slabs in slab order
  // exactly as k_sum_partials adds the partial rows (tiles not computed as +0), and flags gdone[g]
  // so that k_sum_partials leaves the gene alone
  const bool direct = gdone && NGR == 1 && ns * ((G + 31) & ~31) * 8 <= (int)sizeof(bstage);
  if (gdone && threadIdx.x == 0) gdone[g] = 0;
  if (*nanflag) {  // a NaN in some table: k_boot2 computes every slab
    if ((int)threadIdx.x < ns) {
      const int q = g * P + s0 + threadIdx.x;
      redo[q] = 1;
      redo[(long long)ngenes * P + 1 + atomicAdd(&redo[(long long)ngenes * P], 1)] = q;
      pmask[q] = ~0u;
    }
    return;
  }
  if (threadIdx.x < 64) etab[threadIdx.x] = kExp2Frac64[threadIdx.x];
  if (threadIdx.x == 0) failm = 0u;
  if (WB < 4) {
    for (int i = threadIdx.x; i < kBTileMax * 32; i += 64 * WB) dsum[i] = 0;
    __syncthreads();  // zeroed before any wave adds into it
  }
  const int n = nnz[g];
  const int NT = (G + 15) >> 4, NTB = (G + 31) >> 5;  // 16-point sum tiles, 32-point bound tiles
  const int2* __restrict__ E = ent + (long long)g * ent_stride;
  const int set = wset ? wset[g] : 0;
  const int gb0 = s0 * NB, gnb = ns * NB;  // the group's boots (gnb <= 128)
  const int NW = (gnb + 31) >> 5;          // 32-boot bound windows
  const unsigned gstride = (unsigned)NGR * 128u;
  const unsigned char* __restrict__ W8grp = W8g + (long long)set * ncells * gstride + gr * 128;
  const int* __restrict__ ZUset = ZUq + (long long)set * 4 * kQTiles * Bq + gb0;
  // ---- 1. bounds of the group's boot window 32 wsid .. 32 wsid + 31 (with 3 waves: the fourth
  // window split by entry chunks)
  if (!(SCDE_TILE_DIAG & 512) && wsid < NW)  // (512: timing build without the bound pass)
    tile_bound_pass(E, n, UQ, W8grp + 32 * wsid, gstride, ZUset + 32 * wsid, Bq, &bstage[wsid][0], gub + 32 * wsid, 128,
                    min(32, gnb - 32 * wsid), NTB, lane);
  if (SCDE_TILE_DIAG & 16) {  // timing build: the bounds replaced by -inf (no post-check failures; results wrong)
    __syncthreads();
    for (int i = threadIdx.x; i < kBTileMax * 128; i += 64 * WB) gub[i] = -INFINITY;
  }
  if (WB < 4 && NW > WB) {  // (each wave stages in its own area: no barrier before the partial pass)
    tile_bound_partial(E, n, UQ, W8grp + 32 * WB, gstride, wsid, WB, &bstage[wsid][0], dsum, min(32, gnb - 32 * WB),
                       NTB, lane);
    __syncthreads();
    // the split window's bounds: the baseline part (ZU digits) plus the waves' partial sums
    for (int i = threadIdx.x; i < NTB * 32; i += 64 * WB) {
      const int t = i >> 5, b = i & 31;
      if (b < gnb - 32 * WB) {
        const int* zu = ZUset + 32 * WB + b;
        const long long vz = (((long long)zu[(3LL * kQTiles + t) * Bq] * 256 + zu[(2LL * kQTiles + t) * Bq]) * 256 +
                              zu[(1LL * kQTiles + t) * Bq]) * 256 + zu[(long long)t * Bq];
        const double x = (double)(vz + dsum[t * 32 + b]) * 0x1p-8;
        float f = (float)x;
        if ((double)f < x) f = nextafterf(f, INFINITY);
        gub[t * 128 + 32 * WB + b] = f;
      }
    }
  }
  __syncthreads();
  // ---- 2. the plan: per slab the score of each bound tile (its largest bound over the live boots)
  {
    const int s = threadIdx.x >> 4, t = threadIdx.x & 15;
    if (s < kGeneSlabs) {
      float v = -INFINITY;
      if (s < ns && t < NTB) {
        const int nl = min(NB, nboot - (gb0 + s * NB));
        for (int b = 0; b < nl; ++b) v = fmaxf(v, gub[t * 128 + s * NB + b]);
      }
      sc[s][t] = v;
      rowof[s][t] = -1;
    } else if (s < kGeneSlabs + 1 && t < kGeneRows) {
      rowS[t] = -1;
      rowT[t] = 0;
    }
  }
  __syncthreads();
  {  // ranks (ties by tile index)
    const int s = threadIdx.x >> 4, t = threadIdx.x & 15;
    if (s < ns && t < NTB) {
      const float v = sc[s][t];
      int rnk = 0;
      for (int u = 0; u < NTB; ++u) {
        const float w = sc[s][u];
        rnk += (w > v) || (w == v && u < t);
      }
      rk[s][rnk] = (signed char)t;
    }
  }
  __syncthreads();
  // rows per slab (kcap, maxgroups: tests force the list pass / k_boot2 fallback with fewer)
  const int K = min(min(4, kGeneRows / ns), min(NTB, max(1, min(maxgroups, kcap))));
  {
    const int x = threadIdx.x;
    if (x < K * ns) {  // regular rows: slab x / K, rank x % K
      const int s = x / K;
      rowS[x] = s;
      rowT[x] = rk[s][x - s * K];
    } else if (x >= 64 && x < 64 + 2 * ns && maxgroups >= 4 && kcap >= 4) {
      // spare rows: candidates (slab s, rank K + j), j < 2, by how close their bound is to the
      // slab's top bound (ranks of one slab in order: their keys only decrease)
      const int c = x - 64, s = c >> 1, k = K + (c & 1);
      const int nsp = kGeneRows - K * ns;
      if (k < NTB && nsp > 0) {
        const float key = sc[s][rk[s][k]] - sc[s][rk[s][0]];
        int o = 0;
        for (int c2 = 0; c2 < 2 * ns; ++c2) {
          const int s2 = c2 >> 1, k2 = K + (c2 & 1);
          if (k2 >= NTB) continue;
          const float key2 = sc[s2][rk[s2][k2]] - sc[s2][rk[s2][0]];
          o += (key2 > key) || (key2 == key && c2 < c);
        }
        if (o < nsp) {
          rowS[K * ns + o] = s;
          rowT[K * ns + o] = rk[s][k];
        }
      }
    }
  }
  __syncthreads();
  // ---- 3. rows: this lane's row q (one bound tile of one slab), two points per lane
  const int row = lane >> 4, q = 4 * wsid + row;
  const int sq = rowS[q];
  const bool live = sq >= 0;
  const int tq = live ? rowT[q] : 0;
  const int slot = lane >> 3, m2 = lane & 7, r = lane & 15;
  const int k0 = 16 * (2 * tq + (slot & 1)) + 2 * m2;
  const bool l0 = live && k0 < G, l1 = live && k0 + 1 < G;
  const int b0 = gb0 + (live ? sq : 0) * NB;
  const double* __restrict__ W = Wt + (long long)set * ncells * Bp;
  const double* __restrict__ Zs = Z + (long long)set * Bp * GS;
  double a0[NB], a1[NB];
  if (SCDE_TILE_DIAG & 32) {  // timing build: no row loop (results wrong)
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      a0[i] = l0 ? (double)(k0 + i) : -INFINITY;
      a1[i] = l1 ? (double)(k0 + i) : -INFINITY;
    }
  } else {
    tile_rows<NB>(a0, a1, D, E, n, W, Zs, GS, Bp, b0, k0, r, live, l0, l1);
  }
  if (SCDE_TILE_DIAG & 64) {  // timing build: rows only (results wrong)
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < NB; ++i) v += a0[i] + a1[i];
    if (v == 12345.0) part[0] = v;
    return;
  }
  // per-row f32 maxima (max is exact: the same m'_b as any other reduction order)
  if (!(SCDE_TILE_DIAG & 2048)) {
    float v[32];
#pragma unroll
    for (int i = 0; i < NB; ++i) v[i] = (float)gt_max(a0[i], a1[i]);
    row_max_scatter_f<NB>(v, r);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int idx = row_scatter_index<NB>(r, j);
      if (idx >= 0) rowmax[q * 32 + idx] = v[j];
    }
  }
  __syncthreads();
  {
    // the slab's rows: its K regular rows s K .. s K + K - 1, then the spare rows past K ns that
    // the plan gave it (max is exact: any order gives the same m'_b)
    for (int x = threadIdx.x; x < ns * 32; x += 64 * WB) {
      const int s = x >> 5, i = x & 31;
      if (i < NB) {
        float m = -INFINITY;
        if (SCDE_TILE_DIAG & 2048) {
          m = 0.0f;
        } else {
          for (int j = 0; j < K; ++j) m = gt_maxf(m, rowmax[(s * K + j) * 32 + i]);
          for (int q2 = K * ns; q2 < kGeneRows; ++q2)
            if (rowS[q2] == s) m = gt_maxf(m, rowmax[q2 * 32 + i]);
        }
        fmx[s][i] = m;
      }
    }
    if ((int)threadIdx.x < ns) {  // the slab's computed bound tiles and the rows holding them
      const int s = threadIdx.x;
      unsigned b = 0;
      for (int q2 = s * K; q2 < s * K + K; ++q2) {
        b |= 1u << rowT[q2];
        rowof[s][rowT[q2]] = (signed char)q2;
      }
      for (int q2 = K * ns; q2 < kGeneRows; ++q2)
        if (rowS[q2] == s) {
          b |= 1u << rowT[q2];
          rowof[s][rowT[q2]] = (signed char)q2;
        }
      bd[s] = b;
    }
  }
  __syncthreads();
  // ---- 4. post-check per slab (wave w: slabs w, w + 4)
  for (int s = wsid; s < ns; s += WB) {
    const int nl = min(NB, nboot - (gb0 + s * NB));
    // lane (bound tile lane & 15, boots lane >> 4, + 4, ...): four short chains instead of one
    // 20-boot chain per tile (NTB <= 14 < 16)
    const int tt = lane & 15;
    bool need = false;
    if (!(SCDE_TILE_DIAG & 1024) && tt < NTB && !((bd[s] >> tt) & 1))
      for (int b = lane >> 4; b < nl; b += 4) need |= (double)gub[tt * 128 + s * NB + b] >= (double)fmx[s][b] - 51.0;
    if (__ballot(need)) {
      if (lane == 0) {
        atomicOr(&failm, 1u << s);
        const int q = g * P + s0 + s;
        const int pos = atomicAdd(&wide[0], 1);
        if (pos < wide_cap) {  // the four-tile list pass
          wide[1 + pos] = q;
          if (stats) atomicAdd(&stats[35], 1);
        } else {  // past the list pass's launch: k_boot2 takes the slab whole
          redo[q] = 1;
          redo[(long long)ngenes * P + 1 + atomicAdd(&redo[(long long)ngenes * P], 1)] = q;
          pmask[q] = ~0u;
          if (stats) atomicAdd(&stats[3], 1);
        }
      }
    } else if (lane < nl && !(fabs((double)fmx[s][lane]) <= degen_thresh)) {
      degen[g] = 1;
    }
  }
  if (stats && threadIdx.x == 0) atomicAdd(&stats[4], WB * 2 * ((n + 1) & ~1));
  __syncthreads();
  const unsigned fm = failm;
  const bool mine = live && !((fm >> sq) & 1);
  const int sqc = live ? sq : 0;
  // ---- 5. softmax terms, tile partial sums, jp partial rows.  The terms of all NB boots are one
  // straight-line block (no per-boot branch), so the compiler interleaves the NB x 2 independent
  // exp chains instead of running each chain's latency alone.  The exps go through the LDS table
  // (the table-free polynomial and a magic-number rounding variant were slower: DESIGN.md).
  {
    bool any = false;
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const double m = fmx[sqc][i];  // (lanes of no row: l0 = l1 = false, any slab's maxima)
      const double d0 = a0[i] - m, d1 = a1[i] - m;
      const bool n0 = mine && l0 && d0 >= kBootExpCut, n1 = mine && l1 && d1 >= kBootExpCut;
      any |= n0 || n1;
      // (the cut and dead points go in as -1000: exp underflows to exactly +0, no select after it)
      a0[i] = n0 ? d0 : -1000.0;
      a1[i] = n1 ? d1 : -1000.0;
    }
    if (__builtin_amdgcn_ballot_w64(any)) {
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        a0[i] = (SCDE_TILE_DIAG & 4096) ? a0[i] : exp_tab(a0[i], etab);
        a1[i] = (SCDE_TILE_DIAG & 4096) ? a1[i] : exp_tab(a1[i], etab);
      }
    } else {
#pragma unroll
      for (int i = 0; i < NB; ++i) a0[i] = a1[i] = 0.0;
    }
  }
  {
    // quad partials: tsum[sum slot][quad][boot]
    double v[32];
#pragma unroll
    for (int i = 0; i < NB; ++i) v[i] = a0[i] + a1[i];
    pair4_scatter<NB>(v, m2);
#pragma unroll
    for (int j = 0; j < (NB + 3) / 4; ++j) {
      const int idx = pair_scatter_index<NB>(m2, j);
      if (live && idx >= 0) tsum[((2 * q + (slot & 1)) * 2 + (m2 >> 2)) * NB + idx] = v[j];
    }
  }
  __syncthreads();
  for (int x = threadIdx.x; x < ns * 32 && !(SCDE_TILE_DIAG & 8192); x += 64 * WB) {
    const int s = x >> 5, b = x & 31;
    if (b < NB && !((fm >> s) & 1)) {
      double S = 0.0;
      for (unsigned mm = bd[s]; mm; mm &= mm - 1) {  // bound tiles in order, their two sum tiles
        const int t = __builtin_ffs((int)mm) - 1;
        const int q2 = rowof[s][t];
        if (2 * t < NT) S += tsum[(4 * q2) * NB + b] + tsum[(4 * q2 + 1) * NB + b];
        if (2 * t + 1 < NT) S += tsum[(4 * q2 + 2) * NB + b] + tsum[(4 * q2 + 3) * NB + b];
      }
      finv[s * 32 + b] = (gb0 + s * NB + b < nboot) ? 1.0 / (S * norm_mult) : 0.0;
    }
  }
  __syncthreads();
  double j0 = 0.0, j1 = 0.0;
  if (mine && !(SCDE_TILE_DIAG & 8192)) {
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      j0 = fma(a0[i], finv[sq * 32 + i], j0);
      j1 = fma(a1[i], finv[sq * 32 + i], j1);
    }
  }
  if (direct && fm == 0u) {
    // the slabs' rows in LDS ([slab][point], zeros where a slab computed no tile), then per point the
    // sum over the slabs in order: the partial rows k_sum_partials would add, added the same way
    const int GP = (G + 31) & ~31;
    double* rows = reinterpret_cast<double*>(&bstage[0][0]);
    __syncthreads();  // every lane's finv reads are done: the staging area is free
    for (int x = threadIdx.x; x < ns * GP; x += 64 * WB) rows[x] = 0.0;
    __syncthreads();
    if (mine) {
      if (l1)
        *reinterpret_cast<d2_t*>(rows + sq * GP + k0) = d2_t{j0, j1};
      else if (l0)
        rows[sq * GP + k0] = j0;
    }
    __syncthreads();
    double* orow = out + (long long)g * out_g;
    for (int k = threadIdx.x; k < G; k += 64 * WB) {
      double v = rows[k];
      for (int p = 1; p < ns; ++p) v += rows[p * GP + k];
      orow[(long long)k * out_k] = v;
    }
    if (threadIdx.x == 0) gdone[g] = 1;
    if (stats && (int)threadIdx.x < ns) {
      unsigned dn = 0;
      for (unsigned mm = bd[threadIdx.x]; mm; mm &= mm - 1) dn |= 3u << (2 * (__builtin_ffs((int)mm) - 1));
      dn &= (NT >= 32) ? ~0u : ((1u << NT) - 1);
      atomicAdd(&stats[0], 1);
      atomicAdd(&stats[1], __builtin_popcount(dn));
      atomicAdd(&stats[2], NT);
      atomicAdd(&stats[6 + __builtin_popcount(dn)], 1);
    }
    return;
  }
  if (mine && !(SCDE_TILE_DIAG & 8192)) {
    double* prow = part + (long long)(s0 + sq) * part_stride + (long long)g * GS;
    if (l1)
      *reinterpret_cast<d2_t*>(prow + k0) = d2_t{j0, j1};
    else if (l0)
      prow[k0] = j0;
  }
  // tiles not computed stay unwritten: k_sum_partials reads only the tiles in pmask
  if ((int)threadIdx.x < ns && !((fm >> threadIdx.x) & 1)) {
    const unsigned ntmask = (NT >= 32) ? ~0u : ((1u << NT) - 1);
    unsigned dn = 0;
    for (unsigned mm = bd[threadIdx.x]; mm; mm &= mm - 1) dn |= 3u << (2 * (__builtin_ffs((int)mm) - 1));
    dn &= ntmask;
    pmask[(long long)g * P + s0 + threadIdx.x] = dn;
    if (stats) {
      atomicAdd(&stats[0], 1);
      atomicAdd(&stats[1], __builtin_popcount(dn));
      atomicAdd(&stats[2], NT);
      atomicAdd(&stats[6 + __builtin_popcount(dn)], 1);
    }
  }
}

#ifdef SCDE_TILE_TEST_WB1
// hazard-test builds only (tests/test_kernel_resources.py), never run: one-wave blocks with a
// token bound-staging area, whose LDS no longer caps occupancy at 4 waves per SIMD, so
// SCDE_TILE_WPE = 6 squeezes the row loop's registers as the faulting round-2 builds were
template __global__ void k_boot_tiles<20, 1>(const double* __restrict__, const int2* __restrict__, const int* __restrict__,
                                             int, const double* __restrict__, int, int, const int* __restrict__,
                                             const double* __restrict__, int, int, int, int, double, double,
                                             double* __restrict__, long long, int* __restrict__, int,
                                             const unsigned char* __restrict__, int, const unsigned* __restrict__,
                                             const int* __restrict__, const int* __restrict__, int, int* __restrict__,
                                             int* __restrict__, unsigned* __restrict__, const int* __restrict__);
#endif

// jp[g, k] = sum over slabs p (in order) of part[p][g][k]
// pmask (nullable, k_boot_tiles): per (gene, slab) the 16-point tiles written; the others
// are zeros, read as +0.0, so the sums are those of full rows.
__global__ void k_sum_partials(const double* __restrict__ part, long long part_stride, int P, int ngenes, int G,
                               int GS, double* __restrict__ out, long long out_g, long long out_k,
                               const unsigned* __restrict__ pmask, const int* __restrict__ gdone) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)ngenes * G) return;
  const int g = (int)(i / G), k = (int)(i % G);
  if (gdone && gdone[g]) return;  // k_boot_gene wrote the row itself
  const unsigned bit = 1u << (k >> 4);
  double s = (!pmask || (pmask[(long long)g * P] & bit)) ? part[(long long)g * GS + k] : 0.0;
  for (int p = 1; p < P; ++p)
    s += (!pmask || (pmask[(long long)g * P + p] & bit)) ? part[(long long)p * part_stride + (long long)g * GS + k]
                                                         : 0.0;
  out[(long long)g * out_g + (long long)k * out_k] = s;
}

// ensemble: E = exp(T) / colsum(exp(T)) per column (src/jpmatLogBoot.cpp:226-229)
__global__ __launch_bounds__(256) void k_ensemble_cols(const double* __restrict__ T, long long ncols, int G, int GS,
                                                       double* __restrict__ Eo) {
  const int lane = threadIdx.x & 63;
  const long long col = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (col >= ncols) return;
  double ls = 0.0;
  for (int k = lane; k < G; k += 64) ls += exp(T[col * GS + k]);
  const double s = wave_sum(ls);
  for (int k = lane; k < G; k += 64) Eo[col * GS + k] = exp(T[col * GS + k]) / s;
}

// ================================================================== launchers
hipError_t launch_cell_prep(const double* models, int ncells, int G, int GS, const double* mag, int lt, int sq,
                            double* mu, double* lcfp, double* lcfpr, double* theta, double* cellscal,
                            double* pq, hipStream_t s, double* cfp) {
  if (ncells <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_cell_prep, dim3(ncells), dim3(256), 0, s, models, ncells, G, GS, mag, lt, sq, mu, lcfp,
                     lcfpr, theta, cellscal, lt ? nullptr : pq, cfp);
  return hipGetLastError();
}

hipError_t launch_col_consts(const int* ucl, const long long* ucl_off, long long ncols, int ncells,
                             const double* theta, int GS, const double* cellscal, double* colc, hipStream_t s) {
  if (ncols <= 0) return hipSuccess;
  int* slow = reinterpret_cast<int*>(colc + kColc * ncols);  // colc holds kColc * ncols + 1 doubles
  hipError_t e = hipMemsetAsync(slow, 0, sizeof(int), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_col_consts, dim3(div_up(ncols, 256)), dim3(256), 0, s, ucl, ucl_off, ncols, ncells, theta, GS,
                     cellscal, colc, slow);
  return hipGetLastError();
}

hipError_t launch_tables(const TablesArgs& a, hipStream_t s) {
  if (a.ncols <= 0 && a.phase != 2) return hipSuccess;
  if (a.phase != 0 && (!a.D || !a.zcol || !a.base_col)) return hipErrorInvalidValue;
  if (a.phase != 1 && a.tasks && a.ntasks > 0 && a.G <= kTabStagedG && a.const_theta && a.colc && a.pq &&
      a.ncols > 0) {
    // lane-per-column kernel (64-column tasks), then the columns whose constants it and its
    // fallback leave (rare; the launch exits at once unless k_col_consts flagged one)
    const dim3 grid(a.ntasks), block(64 * kLpcWaves);
    const int bm = (a.UQ && a.phase == 2) ? kBoundTiles : (a.U && a.phase == 2) ? kBoundStretch : kBoundNone;
    if (a.GS % kLpcFlush) return hipErrorInvalidValue;
    if (bm == kBoundTiles)
      hipLaunchKernelGGL((k_tables_lpc<kBoundTiles>), grid, block, 0, s, a);
    else if (bm == kBoundStretch)
      hipLaunchKernelGGL((k_tables_lpc<kBoundStretch>), grid, block, 0, s, a);
    else
      hipLaunchKernelGGL((k_tables_lpc<kBoundNone>), grid, block, 0, s, a);
    TablesArgs b = a;
    b.slow_only = 1;
    const size_t shm = sizeof(double) * 4 * (size_t)a.GS;
    if (shm > 64 * 1024) return hipErrorInvalidValue;
    const long long nblk = std::min<long long>(1024, div_up(div_up(a.ncols, 64), 4));
    hipLaunchKernelGGL((k_tables<true>), dim3(nblk), dim3(256), shm, s, b);
    return hipGetLastError();
  }
  if (a.phase != 1 && a.tasks && a.ntasks > 0 && a.G <= kTabStagedG) {
    const size_t shm = sizeof(double) * (kTabWaves + 9) * (size_t)a.G;
    const dim3 grid(a.ntasks), block(64 * kTabWaves);
    if (a.const_theta)
      hipLaunchKernelGGL((k_tables_cell<true>), grid, block, shm, s, a);
    else
      hipLaunchKernelGGL((k_tables_cell<false>), grid, block, shm, s, a);
    return hipGetLastError();
  }
  const long long nwaves = a.phase == 1 ? a.ncells : a.phase == 2 ? a.ncols + 1 : a.ncols;
  if (nwaves <= 0) return hipSuccess;
  const dim3 grid(div_up(nwaves, 4)), block(256);
  const size_t shm = sizeof(double) * 4 * (size_t)a.GS;
  if (shm > 64 * 1024) return hipErrorInvalidValue;
  if (a.const_theta)
    hipLaunchKernelGGL((k_tables<true>), grid, block, shm, s, a);
  else
    hipLaunchKernelGGL((k_tables<false>), grid, block, shm, s, a);
  return hipGetLastError();
}

hipError_t launch_zuq(const unsigned* UQ, const int* base_col, int ncells, const unsigned char* W8, int Bp, int nsets,
                      int* ZUq, hipStream_t s) {
  if (Bp % 32) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(ZUq, 0, sizeof(int) * (size_t)nsets * 4 * kQTiles * Bp, s);
  if (e != hipSuccess) return e;
  const int nch = (ncells + kZChunk - 1) / kZChunk;
  hipLaunchKernelGGL(k_zuq, dim3(Bp / 32, nsets * nch), dim3(32 * kQTiles), 0, s, UQ, base_col, ncells, W8, Bp, ZUq);
  return hipGetLastError();
}

hipError_t launch_base_cols(const int* ucl, const long long* ucl_off, int ncells, const unsigned char* has_clamp,
                            int use_baseline, int* base_col, hipStream_t s) {
  if (ncells <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_base_cols, dim3(div_up(ncells, 128)), dim3(128), 0, s, ucl, ucl_off, ncells, has_clamp,
                     use_baseline, base_col);
  return hipGetLastError();
}

hipError_t launch_delta(const double* T, const long long* ucl_off, int ncells, long long ncols, const int* base_col,
                        int G, int GS, double* D, hipStream_t s) {
  hipLaunchKernelGGL(k_delta, dim3(div_up(ncols + 1, 4)), dim3(256), 0, s, T, ucl_off, ncells, ncols, base_col, G,
                     GS, D);
  return hipGetLastError();
}

hipError_t launch_baseline_z(const double* T, int G, int GS, const int* base_col, int ncells, const double* Wt,
                             int Bp, int nsets, double* Z, hipStream_t s, int gsets, int gsplit) {
  if (gsets < 0 || gsets > nsets || gsplit < 0 || gsplit > ncells) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_baseline_z, dim3(Bp / 4, (GS + 63) / 64, nsets), dim3(64 * kZWaves), 0, s, T, G, GS, base_col, ncells, Wt,
                     Bp, Z, gsets, gsplit);
  return hipGetLastError();
}

hipError_t launch_stretch_zu(const double* U, const int* base_col, int ncells, const double* Wt, int Bp, int nsets,
                             double* ZU, hipStream_t s, int gsets, int gsplit) {
  if (nsets <= 0 || Bp <= 0) return hipSuccess;
  if (gsets < 0 || gsets > nsets || gsplit < 0 || gsplit > ncells) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_stretch_zu, dim3(Bp, nsets), dim3(256), 0, s, U, base_col, ncells, Wt, Bp, ZU, gsets, gsplit);
  return hipGetLastError();
}

int boot2_nb(int nboot) {
  // boots per block slab (a multiple of 4 that fits 4 waves/SIMD without spills):
  // fewest padded boots, then the larger slab
  static const int cand[] = {20, 16, 12, 8, 4};
  int best = 4, best_pad = 1 << 30;
  for (int nb : cand) {
    const int pad = (nboot + nb - 1) / nb * nb - nboot;
    if (pad < best_pad) {
      best_pad = pad;
      best = nb;
    }
  }
  return best;
}

hipError_t launch_boot2(const Boot2Args& a, hipStream_t s) {
  if (a.ngenes <= 0) return hipSuccess;
  // k_boot2 forms column and multiplicity-row offsets in 32 bits
  if ((long long)a.ncols_p1 * a.GS >= (1LL << 31) || (long long)a.ncells * a.Bp >= (1LL << 31))
    return hipErrorInvalidValue;
  const int block = ((a.G + 63) / 64) * 64;
  const int P = (a.nboot + a.nb - 1) / a.nb;
  // stretch skipping: at most 8 stretches (U slots); mask kernel, skipping launch, redo launch
  const int* smask = nullptr;
  const double* sub = nullptr;
  // (the mask kernel stages a gene's entry list in LDS: up to ~7,600 cells)
  if (a.U && a.ZU && a.mask && a.ubuf && a.redo && block <= 64 * kStretchSlots &&
      sizeof(int2) * (size_t)a.ent_stride <= 60 * 1024) {
    // slack of the heuristic: UB's looseness grows with the draws per boot (~0.1 per cell)
    // default 20 + 0.15 C (round 4 A/B: config 2 bootstrap 3.23 -> 3.14 ms per step, 2b 8.25 -> 7.9;
    // was 30 + 0.4 C); the post-check keeps the output exact whatever the slack
    const double slack = std::isnan(a.slack) ? 20.0 + 0.15 * a.ncells : a.slack;  // tests force post-check failures
    const size_t eshm = sizeof(int2) * (size_t)a.ent_stride;
#define SCDE_SM(NBV)                                                                                              \
  case NBV:                                                                                                        \
    hipLaunchKernelGGL(k_stretch_mask<NBV>, dim3(a.ngenes * P), dim3(64), eshm, s, a.ent, a.nnz, a.ent_stride,    \
                       a.Wt, a.Bp, a.ncells, a.wset, a.G, P, a.nboot, a.U, a.ZU, slack, a.ubuf, a.mask, a.ngenes); \
    break;
    switch (a.nb) {
      SCDE_SM(4) SCDE_SM(8) SCDE_SM(12) SCDE_SM(16) SCDE_SM(20) SCDE_SM(24) SCDE_SM(28) SCDE_SM(32)
      default: return hipErrorInvalidValue;
    }
#undef SCDE_SM
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(a.redo, 0, sizeof(int) * ((size_t)a.ngenes * P + 1), s);
    if (e != hipSuccess) return e;
    smask = a.mask;
    sub = a.ubuf;
  }
  const int grid = (a.ngenes + 7) / 8 * 8 * P;
#define SCDE_B2(NBV)                                                                                              \
  case NBV:                                                                                                        \
    hipLaunchKernelGGL(k_boot2<NBV>, dim3(grid), dim3(block), 0, s, a.D, a.ent, a.nnz,          \
                       a.ent_stride, a.Wt, a.Bp,                                                                  \
                       a.ncells, a.wset, a.Z, a.G, a.GS, P, a.nboot, a.norm_mult, a.degen_thresh, a.part,        \
                       a.part_stride, a.degen, a.ngenes, smask, sub, a.redo, RP);                             \
    break;
  {
    // pass 0: with skipping (when set up); pass 1: the slabs the post-check flagged
    const int npass = smask ? 2 : 1;
    for (int RP = 0; RP < npass; ++RP) {
      switch (a.nb) {
        SCDE_B2(4) SCDE_B2(8) SCDE_B2(12) SCDE_B2(16) SCDE_B2(20) SCDE_B2(24) SCDE_B2(28) SCDE_B2(32)
        default: return hipErrorInvalidValue;
      }
      if (RP == 0) smask = nullptr;  // the redo launch recomputes whole slabs
    }
  }
#undef SCDE_B2
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const long long n = (long long)a.ngenes * a.G;
  hipLaunchKernelGGL(k_sum_partials, dim3(div_up(n, 256)), dim3(256), 0, s, a.part, a.part_stride, P, a.ngenes,
                     a.G, a.GS, a.out, a.out_g, a.out_k, nullptr, nullptr);
  return hipGetLastError();
}

// Several buffers zeroed by one launch instead of one fill per buffer (the bootstrap set-up is a
// chain of short dependent launches, each costing ~5 us of launch latency): span i is bytes
// [0, n_i) at p_i (16-B aligned), in 16-byte stores; the last thread of a span writes its tail.
struct ZeroSpans {
  static constexpr int kMax = 6;
  void* p[kMax];
  unsigned long long n[kMax];
  int count;
};
__global__ __launch_bounds__(256) void k_zero(ZeroSpans z) {
  long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  for (int k = 0; k < z.count; ++k) {
    const long long n16 = (long long)(z.n[k] >> 4), chunks = n16 + ((z.n[k] & 15) ? 1 : 0);
    if (i < chunks) {
      unsigned char* b = static_cast<unsigned char*>(z.p[k]);
      if (i < n16) {
        *reinterpret_cast<uint4*>(b + 16 * i) = make_uint4(0, 0, 0, 0);
      } else {
        for (unsigned long long j = 16ull * n16; j < z.n[k]; ++j) b[j] = 0;
      }
      return;
    }
    i -= chunks;
  }
}

static hipError_t launch_zero(const ZeroSpans& z, hipStream_t s) {
  long long total = 0;
  for (int k = 0; k < z.count; ++k) {
    if (reinterpret_cast<uintptr_t>(z.p[k]) & 15) return hipErrorInvalidValue;
    total += (long long)((z.n[k] + 15) >> 4);
  }
  if (total == 0) return hipSuccess;
  hipLaunchKernelGGL(k_zero, dim3((unsigned)div_up(total, 256)), dim3(256), 0, s, z);
  return hipGetLastError();
}

// One block per (boot, seed set): the boot's draws counted per cell in LDS, then the cell column
// of every multiplicity array written (strided, small: cells x boots per set).
__global__ __launch_bounds__(256) void k_mult(const int* __restrict__ draws, int nboot, int ndraw, int ncells, int Bp,
                                              double* __restrict__ Wt, int Bt, unsigned char* __restrict__ W8,
                                              int nb, int P, unsigned char* __restrict__ W8p, int SG, int NGR,
                                              unsigned char* __restrict__ W8g) {
  __shared__ int hist[kMultMaxCells];
  const int b = blockIdx.x, set = blockIdx.y;
  for (int c = threadIdx.x; c < ncells; c += blockDim.x) hist[c] = 0;
  __syncthreads();
  const int* dr = draws + ((long long)set * nboot + b) * ndraw;
  for (int d = threadIdx.x; d < ndraw; d += blockDim.x) {
    const int cell = dr[d];
    if (cell >= 0) atomicAdd(&hist[cell], 1);
  }
  __syncthreads();
  const int p = b / nb, j = b - p * nb;
  const int gr = SG > 0 ? b / (SG * nb) : 0, jg = b - gr * SG * nb, wg = jg >> 5, jj = jg & 31;
  const int slotp = (j < 16) ? 2 * j : 2 * (j - 16) + 1;
  const int slotg = (jj < 16) ? 2 * jj : 2 * (jj - 16) + 1;
  for (int c = threadIdx.x; c < ncells; c += blockDim.x) {
    const int w = hist[c];
    if (!w) continue;  // (the arrays were zeroed)
    const long long sc = (long long)set * ncells + c;
    Wt[sc * Bp + b] = (double)w;
    if (W8) W8[sc * Bt + b] = (unsigned char)w;
    if (W8p && j < 32) W8p[(sc * P + p) * 32 + slotp] = (unsigned char)w;
    if (W8g && jg < 128) W8g[(sc * NGR + gr) * 128 + 32 * wg + slotg] = (unsigned char)w;
  }
}

hipError_t launch_mult(const int* draws, int nsets, int nboot, int ndraw, int ncells, int Bp, double* Wt, int Bt,
                       unsigned char* W8, int nb, int P, unsigned char* W8p, int SG, int NGR, unsigned char* W8g,
                       hipStream_t s) {
  if (ncells <= 0 || ncells > kMultMaxCells || nsets <= 0 || nb <= 0 || Bp < nboot || (W8 && Bt < nboot) ||
      (W8p && P * nb < nboot) || (W8g && (SG <= 0 || NGR * SG * nb < nboot)))
    return hipErrorInvalidValue;
  const size_t sc = (size_t)nsets * ncells;
  ZeroSpans z{};
  z.p[z.count] = Wt;
  z.n[z.count++] = sizeof(double) * sc * Bp;
  if (W8) {
    z.p[z.count] = W8;
    z.n[z.count++] = sc * Bt;
  }
  if (W8p) {
    z.p[z.count] = W8p;
    z.n[z.count++] = sc * P * 32;
  }
  if (W8g) {
    z.p[z.count] = W8g;
    z.n[z.count++] = sc * NGR * 128;
  }
  hipError_t e = launch_zero(z, s);
  if (e != hipSuccess) return e;
  if (nboot <= 0 || ndraw <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_mult, dim3(nboot, nsets), dim3(256), 0, s, draws, nboot, ndraw, ncells, Bp, Wt, Bt, W8, nb, P,
                     W8p, SG, NGR, W8g);
  return hipGetLastError();
}

hipError_t launch_boot_tiles(const Boot2Args& a, const TileBootArgs& tb, hipStream_t s) {
  if (a.ngenes <= 0) return hipSuccess;
  const int P = (a.nboot + a.nb - 1) / a.nb;
  if (a.G > 16 * kTileMax || !a.redo || !tb.W8p || !tb.UQ || !tb.ZUq || !tb.nanflag || !tb.pmask ||
      tb.Bq < (P - 1) * a.nb + 32 || tb.Bq % 32)
    return hipErrorInvalidValue;
  if ((long long)a.ncols_p1 * a.GS >= (1LL << 31) || (long long)a.ncells * a.Bp >= (1LL << 31) ||
      (long long)a.ncells * 32 * P >= (1LL << 31))
    return hipErrorInvalidValue;
  // gene blocks: one 4-wave block per (gene, group of SG slabs) shares 16 rows among the group's
  // slabs; the slabs whose post-check fails take the four-tile pass over `wide`
  if (!tb.W8g || !tb.wide || tb.SG < 1 || tb.SG > kGeneSlabs || tb.SG * a.nb > 128) return hipErrorInvalidValue;
  const int NGR = (P + tb.SG - 1) / tb.SG;
  if ((long long)a.ncells * NGR * 128 >= (1LL << 31) || tb.Bq < (NGR - 1) * tb.SG * a.nb + 128)
    return hipErrorInvalidValue;
  // the launch's genes (a gene chunk, or every gene)
  const int g_lo = tb.g_hi >= 0 ? tb.g_lo : 0, g_hi = tb.g_hi >= 0 ? tb.g_hi : a.ngenes;
  if (g_lo < 0 || g_hi > a.ngenes || g_lo > g_hi) return hipErrorInvalidValue;
  const long long gspan = g_hi - g_lo;
  // redo: [items] fallback flags, [1] the fallback list's length, [items] the list; and the list
  // pass's count wide[0]: one zeroing launch
  ZeroSpans z{};
  z.p[z.count] = a.redo;
  z.n[z.count++] = sizeof(int) * ((size_t)a.ngenes * P + 1);
  z.p[z.count] = tb.wide;
  z.n[z.count++] = sizeof(int);
  const long long items = (long long)a.ngenes * P;
  hipError_t e = launch_zero(z, s);
  if (e != hipSuccess) return e;
  constexpr int WB = 4;
  // slabs a gene block may leave to the four-tile list pass: at most list_cap (16384 by default;
  // k_boot_gene sends further failures to k_boot2).  The cap is rounded down to a multiple of the
  // list pass's WB waves per block: k_boot_gene writes list entries only below it (wide[0] keeps
  // counting past it), and the list pass's grid of items2 / WB blocks must then hold no wave whose
  // index lies in [cap, grid * WB) -- such a wave would read an entry this call never wrote.
  const long long gene_cap = std::max<long long>(WB, ((tb.list_cap > 0 ? tb.list_cap : 16384) / WB) * WB);
  const long long items2 = std::min(gspan * P, gene_cap);
  const long long gblocks = gspan * NGR;
  const long long gblk0 = (long long)g_lo * NGR;
  // gene blocks holding all of a gene's slabs write the finished jp rows of their genes themselves
  int* const gdone = (tb.gdone && tb.SG >= P) ? tb.gdone : nullptr;
#define SCDE_BT(NBV)                                                                                            \
  case NBV:                                                                                                      \
    hipLaunchKernelGGL((k_boot_gene<NBV, 4>), dim3((unsigned)gblocks), dim3(256), 0, s, a.D, a.ent, a.nnz,      \
                       a.ent_stride, a.Wt, a.Bp, a.ncells, a.wset, a.Z, a.G, a.GS, P, tb.SG, a.nboot,          \
                       a.norm_mult, a.degen_thresh, a.part, a.part_stride, a.degen, a.ngenes, tb.W8g, tb.Bq,  \
                       tb.UQ, tb.ZUq, tb.nanflag, tb.maxgroups, tb.kcap, a.redo, tb.stats, tb.order, tb.pmask, \
                       tb.wide, (int)items2, (int)gblk0, a.out, a.out_g, a.out_k, gdone);                      \
    hipLaunchKernelGGL((k_boot_tiles<NBV, WB>), dim3((unsigned)div_up(items2, WB)), dim3(64 * WB), 0, s, a.D,   \
                       a.ent, a.nnz, a.ent_stride, a.Wt, a.Bp, a.ncells, a.wset, a.Z, a.G, a.GS, P, a.nboot,    \
                       a.norm_mult, a.degen_thresh, a.part, a.part_stride, a.degen, a.ngenes, tb.W8p, tb.Bq,    \
                       tb.UQ, tb.ZUq, tb.nanflag, tb.maxgroups, a.redo, tb.stats, tb.pmask, tb.wide);           \
    break;
  switch (a.nb) {
    SCDE_BT(4) SCDE_BT(8) SCDE_BT(12) SCDE_BT(16) SCDE_BT(20)
    default: return hipErrorInvalidValue;
  }
#undef SCDE_BT
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  // slabs the tile kernel left (more tiles than its registers hold, or NaN tables): k_boot2,
  // whole slab, same sums
  // From kListCells cells per call the fallback is rare (config 3: no slab) and a 512-block
  // k_boot2_list walks the compacted list (one short launch instead of one early-exit block
  // per slab).  Below it a fifth of the slabs can fall back (~100 cells per call), and the
  // full-grid k_boot2 with its occupancy target takes the flagged slabs faster.
  constexpr int kListCells = 400;
  const int block2 = ((a.G + 63) / 64) * 64;
  if (a.ncells >= kListCells) {
    const int grid2 = (int)std::min<long long>(items, 512);
#define SCDE_B2L(NBV)                                                                                             \
  case NBV:                                                                                                        \
    hipLaunchKernelGGL(k_boot2_list<NBV>, dim3(grid2), dim3(block2), 0, s, a.D, a.ent, a.nnz,  \
                       a.ent_stride, a.Wt,                                                                        \
                       a.Bp, a.ncells, a.wset, a.Z, a.G, a.GS, P, a.nboot, a.norm_mult, a.degen_thresh, a.part,   \
                       a.part_stride, a.degen, a.ngenes, a.redo + items, a.redo + items + 1);                   \
    break;
    switch (a.nb) {
      SCDE_B2L(4) SCDE_B2L(8) SCDE_B2L(12) SCDE_B2L(16) SCDE_B2L(20)
      default: return hipErrorInvalidValue;
    }
#undef SCDE_B2L
  } else {
    const int grid2 = (a.ngenes + 7) / 8 * 8 * P;
#define SCDE_B2R(NBV)                                                                                             \
  case NBV:                                                                                                        \
    hipLaunchKernelGGL(k_boot2<NBV>, dim3(grid2), dim3(block2), 0, s, a.D, a.ent, a.nnz, a.ent_stride, a.Wt, a.Bp, \
                       a.ncells, a.wset, a.Z, a.G, a.GS, P, a.nboot, a.norm_mult, a.degen_thresh, a.part,        \
                       a.part_stride, a.degen, a.ngenes, nullptr, nullptr, a.redo, 1);                          \
    break;
    switch (a.nb) {
      SCDE_B2R(4) SCDE_B2R(8) SCDE_B2R(12) SCDE_B2R(16) SCDE_B2R(20)
      default: return hipErrorInvalidValue;
    }
#undef SCDE_B2R
  }
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  // the launch's genes' jp rows (a chunk: its rows, offset pointers)
  const long long nn = gspan * a.G;
  if (nn > 0)
    hipLaunchKernelGGL(k_sum_partials, dim3(div_up(nn, 256)), dim3(256), 0, s, a.part + (long long)g_lo * a.GS,
                       a.part_stride, P, (int)gspan, a.G, a.GS, a.out + (long long)g_lo * a.out_g, a.out_g, a.out_k,
                       tb.pmask + (long long)g_lo * P, gdone ? gdone + g_lo : nullptr);
  return hipGetLastError();
}

hipError_t launch_ensemble_cols(const double* T, long long ncols, int G, int GS, double* E, hipStream_t s) {
  if (ncols <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_ensemble_cols, dim3(div_up(ncols, 4)), dim3(256), 0, s, T, ncols, G, GS, E);
  return hipGetLastError();
}
}  // namespace scde
