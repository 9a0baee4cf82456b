// engine_posterior.hip -- the host side of one posterior (run_posterior): logBootPosterior,
// logBootBatchPosterior, scde.posteriors, both differential-expression entries and pagoda.varnorm's
// weights stage all compute their joint posteriors here.
//
// A call is validated, planned (Plan: every launch decision, from the context's options, the spec
// and the number of table columns) and then run as stages over one state (Posterior), in the order
// run_posterior and Posterior::rest list them: cell prep; the unique counts; the tables (piece by
// piece when the counts arrive in pieces); early modes; the joint posterior without a bootstrap, or
// the bootstrap's set-up on the aux stream, the fast or the general bootstrap and the exact rows;
// the outputs.  The unique-count build (build_unique_sets), the draw lists and the model checks
// live here too.  The streams' handoffs, the read-back thread and the entry points that call
// run_posterior are engine.hip's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <functional>
#include <memory>
#include <vector>

#include "engine_internal.h"
#include "kernels.h"

using namespace scde;
using namespace scde::host;

namespace {

// Build ucl/uci for the selected cells on device (R/functions.R:609-610).  Unique
// counts come out sorted ascending rather than in first-appearance order; the order
// only permutes table columns, never values.  Three phases separated by host syncs
// (bitmap sizes need the per-cell maxima; column offsets need the unique counts);
// build_unique_pair interleaves two groups' phases so a DE call syncs twice, not four
// times, and before any heavy kernel is queued.
using UniqueSet = scde_ctx::UniqueSet;
constexpr long long kUniqueFixedWordsMax = 1 << 16;           // counts below 2^22
constexpr double kUniqueFixedBytesMax = double(256 << 20);    // a set's fixed-width bitmaps

int unique_phase1(scde_ctx* cx, const PostSpec& s, UniqueSet& u) {
  const int C = s.ncells, N = s.ngenes;
  hipStream_t st = cx->stream;
  RCHK(upload(cx, u.cellidx, s.cellidx_host, sizeof(int) * C));
  HCHK(u.cmax.ensure(sizeof(int) * C));
  HCHK(u.cmin.ensure(sizeof(int) * C));
  HCHK(launch_cell_minmax(s.counts_dev, s.ld, 0, N, C, u.cellidx.as<int>(), u.cmax.as<int>(), u.cmin.as<int>(), st));
  u.cmax_h.assign(C, 0);
  u.cmin_h.assign(C, 0);
  int* h = u.landing(2 * (size_t)C);
  u.pin_in = h;
  HCHK(hipMemcpyAsync(h ? h : u.cmax_h.data(), u.cmax.p, sizeof(int) * C, hipMemcpyDeviceToHost, st));
  HCHK(hipMemcpyAsync(h ? h + C : u.cmin_h.data(), u.cmin.p, sizeof(int) * C, hipMemcpyDeviceToHost, st));
  return SCDE_OK;
}

int unique_phase2(scde_ctx* cx, const PostSpec& s, UniqueSet& u) {
  const int C = s.ncells, N = s.ngenes;
  hipStream_t st = cx->stream;
  if (u.pin_in) {  // landed (the caller synchronised)
    std::copy(u.pin_in, u.pin_in + C, u.cmax_h.begin());
    std::copy(u.pin_in + C, u.pin_in + 2 * (size_t)C, u.cmin_h.begin());
  }
  u.woff_h.assign(C + 1, 0);
  long long wmax = 1;
  for (int c = 0; c < C; ++c) {
    if (N > 0 && u.cmin_h[c] < 0) return fail(SCDE_EARG, "negative count in cell %d", c);
    u.woff_h[c + 1] = u.woff_h[c] + ((long long)u.cmax_h[c] >> 6) + 1;
    wmax = std::max(wmax, ((long long)u.cmax_h[c] >> 6) + 1);
  }
  // the next fixed-width build of this set: wide enough for these counts (bounded bitmap memory)
  long long fw = u.fixed_words;
  while (fw < wmax && fw < kUniqueFixedWordsMax) fw *= 2;
  if (fw >= wmax && fw != u.fixed_words && (double)C * fw * 8.0 <= kUniqueFixedBytesMax) u.fixed_words = fw;
  RCHK(upload(cx, u.woff, u.woff_h.data(), sizeof(long long) * (C + 1)));
  u.woff_fixed = 0;
  HCHK(u.bits.ensure(sizeof(unsigned long long) * u.woff_h[C]));
  HCHK(hipMemsetAsync(u.bits.p, 0, sizeof(unsigned long long) * u.woff_h[C], st));
  HCHK(launch_mark(s.counts_dev, s.ld, 0, N, C, u.cellidx.as<int>(), u.woff.as<long long>(),
                   u.bits.as<unsigned long long>(), st));
  HCHK(u.rank.ensure(sizeof(int) * u.woff_h[C]));
  HCHK(u.nuniq.ensure(sizeof(int) * C));
  HCHK(launch_rank(u.bits.as<unsigned long long>(), u.woff.as<long long>(), C, u.rank.as<int>(),
                   u.nuniq.as<int>(), st));
  u.nuniq_h.assign(C, 0);
  int* h = u.landing(2 * (size_t)C);  // phase 1's values were copied out by now
  u.pin_in = h;
  HCHK(hipMemcpyAsync(h ? h : u.nuniq_h.data(), u.nuniq.p, sizeof(int) * C, hipMemcpyDeviceToHost, st));
  return SCDE_OK;
}

int unique_phase3(scde_ctx* cx, const PostSpec& s, UniqueSet& u) {
  const int C = s.ncells, N = s.ngenes;
  hipStream_t st = cx->stream;
  if (u.pin_in) std::copy(u.pin_in, u.pin_in + C, u.nuniq_h.begin());
  u.ucl_off_h.assign(C + 1, 0);
  for (int c = 0; c < C; ++c) u.ucl_off_h[c + 1] = u.ucl_off_h[c] + u.nuniq_h[c];
  RCHK(upload(cx, u.ucl_off, u.ucl_off_h.data(), sizeof(long long) * (C + 1)));
  int* ucl = nullptr;
  int* uci = nullptr;
  if (u.into) {  // a piece: into the whole set's arrays (uci sized by the caller)
    const long long need = std::max(u.into_col0 + u.ucl_off_h[C], u.into_cap_hint);
    auto cx_sync = [cx] { return ctx_streams_sync(cx); };
    HCHK(u.into->ucl.grow(u.into_col0 > 0, sizeof(int) * std::max<long long>(1, need), cx_sync));
    ucl = u.into->ucl.as<int>() + u.into_col0;
    uci = u.into->uci.as<int>() + (size_t)N * u.into_c0;
  } else {
    HCHK(u.ucl.ensure(sizeof(int) * std::max<long long>(1, u.ucl_off_h[C])));
    HCHK(u.uci.ensure(sizeof(int) * std::max<long long>(1, (long long)N * C)));
    ucl = u.ucl.as<int>();
    uci = u.uci.as<int>();
  }
  HCHK(launch_fill_ucl(u.bits.as<unsigned long long>(), u.woff.as<long long>(), C, u.rank.as<int>(),
                       u.ucl_off.as<long long>(), ucl, st));
  HCHK(launch_uci(s.counts_dev, s.ld, 0, N, C, u.cellidx.as<int>(), u.woff.as<long long>(),
                  u.bits.as<unsigned long long>(), u.rank.as<int>(), uci, st));
  u.ready = true;
  return SCDE_OK;
}

// Phases 1 and 2 in one, without the per-cell maxima: every cell gets a bitmap of
// u.fixed_words words (1024 at first: counts below 65,536); k_mark flags a negative count or one
// past the bitmap, and such a set is rebuilt with exact widths (phases 1-2), which also widens
// the set's later fixed builds.  One host sync per build.
int unique_phase12_fixed(scde_ctx* cx, const PostSpec& s, UniqueSet& u) {
  const int C = s.ncells, N = s.ngenes;
  hipStream_t st = cx->stream;
  RCHK(upload(cx, u.cellidx, s.cellidx_host, sizeof(int) * C));
  const long long FW = u.fixed_words;
  u.woff_h.resize(C + 1);
  for (int c = 0; c <= C; ++c) u.woff_h[c] = (long long)c * FW;
  // the fixed offsets c * FW are uploaded once per set and width (grow-only; exact-width builds
  // and a new width reset it)
  if (u.woff_fixed_w != FW) u.woff_fixed = 0;
  u.woff_fixed_w = FW;
  if (u.woff_fixed < C + 1) {
    RCHK(upload(cx, u.woff, u.woff_h.data(), sizeof(long long) * (C + 1)));
    u.woff_fixed = C + 1;
  }
  // one memset for the bitmaps and k_mark's flag word after them
  HCHK(u.bits.ensure(sizeof(unsigned long long) * (u.woff_h[C] + 1)));
  HCHK(hipMemsetAsync(u.bits.p, 0, sizeof(unsigned long long) * (u.woff_h[C] + 1), st));
  int* flags = reinterpret_cast<int*>(u.bits.as<unsigned long long>() + u.woff_h[C]);
  HCHK(launch_mark(s.counts_dev, s.ld, 0, N, C, u.cellidx.as<int>(), u.woff.as<long long>(),
                   u.bits.as<unsigned long long>(), st, flags));
  HCHK(u.rank.ensure(sizeof(int) * u.woff_h[C]));
  HCHK(u.nuniq.ensure(sizeof(int) * (C + 1)));
  HCHK(launch_rank(u.bits.as<unsigned long long>(), u.woff.as<long long>(), C, u.rank.as<int>(),
                   u.nuniq.as<int>(), st, flags, u.nuniq.as<int>() + C));
  u.nuniq_h.assign(C, 0);
  u.fixed_flags = 0;
  int* h = u.landing(2 * (size_t)C + 1);
  u.pin_in = h;
  // the unique counts and the flags (nuniq[C]) in one read-back
  if (h) {
    HCHK(hipMemcpyAsync(h, u.nuniq.p, sizeof(int) * (C + 1), hipMemcpyDeviceToHost, st));
  } else {
    HCHK(hipMemcpyAsync(u.nuniq_h.data(), u.nuniq.p, sizeof(int) * C, hipMemcpyDeviceToHost, st));
    HCHK(hipMemcpyAsync(&u.fixed_flags, u.nuniq.as<int>() + C, sizeof(int), hipMemcpyDeviceToHost, st));
  }
  return SCDE_OK;
}

}  // namespace

// ns (1 or 2) cell subsets of the same device counts
int scde::host::build_unique_sets(scde_ctx* cx, const PostSpec* const* s, UniqueSet* const* u, int ns) {
  hipEvent_t ev = cx->mark_begin(SLOT_UNIQUE);
  if (ns < 1 || ns > 4) return fail(SCDE_EINTERNAL, "unique sets per build: 1..4");
  bool exact[4] = {true, true, true, true};
  if (cx->opt_unique_fixed) {
    for (int i = 0; i < ns; ++i) RCHK(unique_phase12_fixed(cx, *s[i], *u[i]));
    HCHK(hipStreamSynchronize(cx->stream));
    for (int i = 0; i < ns; ++i) {
      const int fl = u[i]->pin_in ? u[i]->pin_in[s[i]->ncells] : u[i]->fixed_flags;
      exact[i] = fl != 0;  // a count outside [0, 65536): the exact build (and its error message)
    }
  }
  bool any_exact = false;
  for (int i = 0; i < ns; ++i) any_exact = any_exact || exact[i];
  if (any_exact) {
    for (int i = 0; i < ns; ++i)
      if (exact[i]) RCHK(unique_phase1(cx, *s[i], *u[i]));
    HCHK(hipStreamSynchronize(cx->stream));
    for (int i = 0; i < ns; ++i)
      if (exact[i]) RCHK(unique_phase2(cx, *s[i], *u[i]));
    HCHK(hipStreamSynchronize(cx->stream));
  }
  for (int i = 0; i < ns; ++i) RCHK(unique_phase3(cx, *s[i], *u[i]));
  cx->mark_end(SLOT_UNIQUE, ev);
  return SCDE_OK;
}

namespace {

// The draw lists alone (cell per draw) and the largest multiplicity of a cell in one boot.
void make_draws_lists(const PostSpec& s, std::vector<int>& draws, int& ndraw, int* maxw) {
  const int C = s.ncells, B = s.nboot, nsets = (int)s.seeds.size();
  if (s.batch_call) {
    ndraw = 0;
    for (int k = 0; k < s.nbatch; ++k) ndraw += std::max(0, s.comp[k]);
  } else {
    ndraw = C;
  }
  const size_t per = (size_t)B * std::max(ndraw, 1);
  draws.assign((size_t)nsets * per, -1);
  std::vector<int> hist((size_t)std::max(C, 1), 0);
  int mx = 0;
  for (int set = 0; set < nsets; ++set) {
    PlatformRand rng((unsigned int)s.seeds[set], s.rand_kind);
    int* dr = draws.data() + (size_t)set * per;
    const int c0 = 0, n = C;
    for (int b = 0; b < B; ++b) {
      int* row = dr + (size_t)b * ndraw;
      int d = 0;
      if (!s.batch_call) {
        for (int j = 0; j < n; ++j) row[d++] = c0 + rng.draw(n);
      } else {
        for (int k = 0; k < s.nbatch; ++k) {
          const int* bi = s.batch_vals + s.batch_off[k];
          const int nbk = (int)(s.batch_off[k + 1] - s.batch_off[k]);
          for (int j = 0; j < s.comp[k]; ++j) row[d++] = bi[rng.draw(nbk)];
        }
      }
      for (int j = 0; j < d; ++j) mx = std::max(mx, ++hist[row[j]]);
      for (int j = 0; j < d; ++j) hist[row[j]] = 0;
    }
  }
  if (maxw) *maxw = mx;
}

// Draw lists and per-cell multiplicities for each seed set.  want_W false: the multiplicities are
// left to the device (launch_mult); only their maximum is formed here (*maxw), from a per-boot
// count of the cells drawn.
void make_draws(const PostSpec& s, int Bp, std::vector<int>& draws, std::vector<double>& W, int& ndraw,
                int* maxw = nullptr, bool want_W = true) {
  const int C = s.ncells, B = s.nboot, nsets = (int)s.seeds.size();
  if (!want_W) {
    make_draws_lists(s, draws, ndraw, maxw);
    return;
  }
  if (s.batch_call) {
    ndraw = 0;
    for (int k = 0; k < s.nbatch; ++k) ndraw += std::max(0, s.comp[k]);
  } else {
    ndraw = C;
  }
  draws.assign((size_t)nsets * B * std::max(ndraw, 1), 0);
  W.assign((size_t)nsets * C * Bp, 0.0);
  for (int set = 0; set < nsets; ++set) {
    PlatformRand rng((unsigned int)s.seeds[set], s.rand_kind);
    int* dr = draws.data() + (size_t)set * B * std::max(ndraw, 1);
    double* w = W.data() + (size_t)set * C * Bp;
    for (int b = 0; b < B; ++b) {
      int d = 0;
      if (!s.batch_call) {
        for (int j = 0; j < C; ++j) {
          const int rj = rng.draw(C);
          dr[(size_t)b * ndraw + d++] = rj;
          w[(size_t)rj * Bp + b] += 1.0;
        }
      } else {
        for (int k = 0; k < s.nbatch; ++k) {
          const int nsamp = s.comp[k];
          if (nsamp > 0) {
            const int* bi = s.batch_vals + s.batch_off[k];
            const int nb = (int)(s.batch_off[k + 1] - s.batch_off[k]);
            for (int j = 0; j < nsamp; ++j) {
              const int cell = bi[rng.draw(nb)];
              dr[(size_t)b * ndraw + d++] = cell;
              w[(size_t)cell * Bp + b] += 1.0;
            }
          }
        }
      }
    }
  }
}

// Models whose tables the reference fills with NaN (and with them every joint posterior row of the
// call) are refused before anything is launched: the tables kernels drop a NaN term (their exps are
// guarded by fmax / range tests) and would return finite tables instead.  Per cell, as
// src/jpmatLogBoot.cpp:128-190 forms them: mu = exp(mag corr.a + corr.b) NaN or infinite at a grid
// point; the concomitant's exponent NaN at a grid point; fail.r NaN; constant theta not a positive
// finite number, or so small that theta / (theta + mu) rounds to 0.  The exponents are linear (or,
// with the squared-logit term, a product of linear factors) in the magnitude, so a NaN shows at the
// smallest or the largest magnitude; mu and theta / (theta + mu) are monotone in it.  O(cells) on
// the host.  (include/scde_hip.h, deviations.)
int check_models(const PostSpec& s) {
  const int C = s.ncells, G = s.G;
  double mlo = INFINITY, mhi = -INFINITY;
  for (int k = 0; k < G; ++k) {
    const double m = s.mag[k];
    if (m != m) return fail(SCDE_EARG, "magnitudes[%d] is NaN", k);
    mlo = std::min(mlo, m);
    mhi = std::max(mhi, m);
  }
  auto M = [&](int c, int col) { return s.models[(size_t)c + (size_t)C * col]; };
  for (int c = 0; c < C; ++c) {
    const double concb = M(c, 0), conca = M(c, 1), failr = M(c, 2), corrb = M(c, 3), corra = M(c, 4);
    const double t0 = mlo * corra + corrb, t1 = mhi * corra + corrb;
    if (t0 != t0 || t1 != t1)
      return fail(SCDE_EARG, "model row %d: corr.a = %g, corr.b = %g give a NaN mean at magnitude %g", c, corra, corrb,
                  t0 != t0 ? mlo : mhi);
    const double z0 = (s.squarelogit ? (conca + mlo * M(c, 11)) * mlo : mlo * conca) + concb;
    const double z1 = (s.squarelogit ? (conca + mhi * M(c, 11)) * mhi : mhi * conca) + concb;
    if (z0 != z0 || z1 != z1)
      return fail(SCDE_EARG, "model row %d: conc.a = %g, conc.b = %g%s give a NaN drop-out term at magnitude %g", c,
                  conca, concb, s.squarelogit ? " (with conc.a2)" : "", z0 != z0 ? mlo : mhi);
    if (failr != failr) return fail(SCDE_EARG, "model row %d: fail.r is NaN", c);
    const double tmax = std::max(t0, t1);
    const double th = s.localtheta ? 1.0 : M(c, 5);
    // (fitted models: mu below e^300 and theta above 1e-20 -- nothing can overflow or round to 0,
    // and the call pays no exp here)
    if (tmax < 300.0 && th > 1e-20 && th < INFINITY) continue;
    const double mumax = std::exp(tmax);
    if (!(mumax < INFINITY))
      return fail(SCDE_EARG, "model row %d: corr.a = %g, corr.b = %g give an infinite mean on this grid", c, corra,
                  corrb);
    if (!s.localtheta) {
      if (!(th > 0.0) || !(th < INFINITY))
        return fail(SCDE_EARG, "model row %d: corr.theta = %g is not a positive finite number", c, th);
      if (!(th / (th + mumax) > 0.0))
        return fail(SCDE_EARG, "model row %d: corr.theta = %g against a mean of %g gives probability 0", c, th,
                    mumax);
    }
  }
  return SCDE_OK;
}

// Everything that can refuse a call, before anything is uploaded or launched: the arguments, the
// models, a batch call's composition, and host ucl/uci (source A of the spec).
int validate(const PostSpec& s) {
  const int C = s.ncells, G = s.G, N = s.ngenes;
  if (C <= 0 || G <= 0) return fail(SCDE_EARG, "ncells and ngrid must be positive");
  if (s.nboot < 0) return fail(SCDE_EARG, "nboot must be >= 0");
  if (G > 4096) return fail(SCDE_EARG, "ngrid > 4096 unsupported");
  if (s.seeds.empty()) return fail(SCDE_EINTERNAL, "no seed sets");
  if (!s.models || !s.mag) return fail(SCDE_EARG, "null models or magnitudes");
  RCHK(check_models(s));
  if (s.batch_call) {
    for (int k = 0; k < s.nbatch; ++k) {
      if (s.comp[k] < 0) return fail(SCDE_EARG, "negative composition");
      if (s.comp[k] > 0 && s.batch_off[k + 1] - s.batch_off[k] <= 0)
        return fail(SCDE_EARG, "batch %d has draws but no cells", k);
      for (int64_t i = s.batch_off[k]; i < s.batch_off[k + 1]; ++i)
        if (s.batch_vals[i] < 0 || s.batch_vals[i] >= C) return fail(SCDE_EARG, "BatchIL index out of range");
    }
  }
  if (s.ucl_host) {
    const int64_t* off = s.ucl_off_host;
    if (off[0] != 0) return fail(SCDE_EARG, "ucl_off[0] must be 0");
    for (int c = 0; c < C; ++c)
      if (off[c + 1] < off[c]) return fail(SCDE_EARG, "ucl_off must be non-decreasing");
    // counti against the per-cell list sizes (the reference would read out of bounds)
    for (int c = 0; c < C; ++c) {
      const long long nu = off[c + 1] - off[c];
      const int* col = s.uci_host + (size_t)N * c;
      for (int g = 0; g < N; ++g)
        if (col[g] < 0 || col[g] >= nu) return fail(SCDE_EARG, "counti[%d,%d]=%d out of range [0,%lld)", g, c, col[g], nu);
    }
  }
  return SCDE_OK;
}

// the joint posterior comes from a bootstrap (else: the ensemble, the plain sum, or zeros)
bool bootstraps(const PostSpec& s) { return s.nboot > 0 && (s.batch_call || !s.ensemble); }

// Every launch decision of a call, from the context's options, the spec and the number of table
// columns.  Its column-count conditions hold for fewer columns whenever they hold for more, so a
// call whose counts arrive in pieces plans for 0 columns, launches its tables piece by piece, plans
// again once the count is known and redoes the tables should the two plans differ.
struct Plan {
  // column stride: >= the k_boot2 block (lanes never read past a column); 512 keeps columns
  // 4 KiB-aligned
  int GS;
  // Bootstrap path with G <= 1024 (k_boot2), fused: the tables kernel writes the baseline-delta
  // columns D directly (phase 1: count-0 columns and base_col, phase 2: the rest); T itself is kept
  // only when individual posteriors are returned.
  bool fast, fused, keep_T;
  // k_boot_tiles: G <= 448, nb <= 20, multiplicities <= 127 (int8), int32 digit sums.  The tables
  // are set up for it before the draws exist; should a multiplicity exceed 127 (a cell drawn 128
  // times in one boot), Posterior::rest narrows it and plain k_boot2 runs on the same D columns.
  bool tpath;
  // k_boot2 grid-stretch skipping (G <= 448: at most 7 stretches of 64 points); the tables kernel
  // emits the per-column stretch maxima
  bool stretch_skip;
  bool want_post, want_maxi, want_modes;  // individual outputs the postflag asks for
  int nb;       // FP64 path: boots per slab
  int Bp;       // boots, padded to whole slabs
  int Bt;       // byte multiplicity rows: the last gene group reads 128 boots
  int qstride;  // tile path ELL rows: a multiple of 64 entries (the bound MFMAs' K steps) plus 64
  bool dev_mult;  // fused path: the draw lists on the host, the multiplicity arrays on the device (launch_mult)
  // the decisions the tables depend on (the others follow from these and the spec)
  bool operator==(const Plan& o) const {
    return fast == o.fast && fused == o.fused && keep_T == o.keep_T && tpath == o.tpath &&
           stretch_skip == o.stretch_skip;
  }
};

Plan make_plan(const scde_ctx* cx, const PostSpec& s, long long ncols) {
  const int C = s.ncells, G = s.G;
  Plan p{};
  p.GS = G <= 448 ? 512 : (int)round_up(G, 64);
  p.want_post = s.batch_call ? (s.postflag == 2) : (s.postflag == 2 || s.postflag == 3);
  p.want_maxi = s.batch_call ? (s.postflag == 1) : (s.postflag == 1 || s.postflag == 3);
  p.want_modes = p.want_maxi;
  // k_boot2 forms column and multiplicity-row offsets in 32 bits: past that, the general kernel
  p.fast = ((G + 63) / 64) * 64 <= 1024 && (ncols + 1) * (long long)p.GS < (1LL << 31) &&
           (long long)C * round_up(std::max(s.nboot, 1), 32) < (1LL << 31);
  p.fused = bootstraps(s) && p.fast;
  p.keep_T = !p.fused || (p.want_post && s.post);
  p.nb = p.fast ? boot2_nb(s.nboot) : 16;
  if (p.fast) {
    const int v = cx->opt_boot_nb;  // tuning option: a multiple of 4 in [4, 32]
    if (v >= 4 && v <= 32 && v % 4 == 0) p.nb = v;
  }
  p.tpath = p.fused && s.nboot > 0 && G <= 448 && cx->opt_boot_skip && cx->opt_boot_tiles &&
            C >= cx->opt_boot_tiles_cells && p.nb <= 20 && C < 100000 && (ncols + 1) * (long long)p.GS < (1LL << 31);
  p.stretch_skip = p.fused && !p.tpath && G <= 448 && cx->opt_boot_skip;
  p.Bp = (int)round_up(std::max(s.nboot, 1), p.nb);
  p.Bt = (int)round_up(p.Bp, 32) + 128;
  p.qstride = (int)round_up(std::max(C, 1), 64) + 64;
  p.dev_mult = p.fused && C <= kMultMaxCells;
  return p;
}
// What the bootstrap's set-up and its launches share, fixed once the draws have settled the tile path.
struct BootLayout {
  int nsets;        // draw sets (seeds)
  int P;            // slabs of nb boots
  int stride;       // ELL row stride
  int gene_sg;      // tile path: slabs per k_boot_gene group
  int nchunks;      // tile path: gene chunks
  bool have_order;  // tile path: genes in order of their count sums
  int order_desc;
};

// One call's state and its stages: built once by run_posterior, shared with `rest` when the caller
// runs the second half later.  s and u are the caller's (engine_internal.h: alive until `rest` ran).
struct Posterior {
  scde_ctx* const cx;
  const PostSpec& s;
  UniqueSet& u;
  const int C, G, N;     // cells, grid points, genes
  const hipStream_t st;  // the context's stream at the call
  const bool pieces;     // the counts arrive in pieces: unique sets and tables piece by piece
  Plan plan;             // (for 0 columns until the unique counts are known)
  TablesArgs ta{};
  long long ncols = 0;
  std::vector<int> draws;
  std::vector<double> W;
  int ndraw = 0, maxw = 0;
  BootLayout bl{};
  bool jp_sent = false;     // jp went back in gene chunks (else once at the end)
  bool exact_done = false;  // the exact rows ran per gene chunk
  Posterior(scde_ctx* cx_, const PostSpec& s_, UniqueSet& u_)
      : cx(cx_), s(s_), u(u_), C(s_.ncells), G(s_.G), N(s_.ngenes), st(cx_->stream),
        pieces(s_.npieces > 0 && !s_.ucl_host), plan(make_plan(cx_, s_, 0)) {}
  // pieces with modes_host: each piece's posterior modes go back as soon as its tables are done
  bool modes_pieces() const { return pieces && plan.want_modes && s.modes && s.modes_host && N > 0; }

  // the stages, in call order (run_posterior lists 1-4, rest 5-11)
  int cell_prep();
  int unique_counts();
  int tables_flags(bool zeroed);
  int setup_tables(long long cap, bool keep);
  int launch_tables_range(int c0, int c1, long long col0, const long long* off_d, const std::vector<long long>& off_h,
                          bool last, UniqueSet& tu);
  int whole_tables(bool flags_zeroed);
  int pieces_loop();
  int rest();
  int early_modes();
  void fused_draws();
  int joint_without_bootstrap();
  BootLayout boot_layout() const;
  int upload_host_mult(hipStream_t sa);
  int boot_setup();
  template <class Args> void set_boot_common(Args& a) const;
  template <class Args> void set_boot_sums(Args& a) const;
  int boot2_args(Boot2Args& b2);
  int tile_args(Boot2Args& b2, TileBootArgs& tb);
  int boot_fast();
  int tile_stats();
  int stretch_stats();
  int boot_general();
  int boot_exact(int g_lo, int g_hi);
  int outputs();
};

// ---- stage 1: per-cell grid vectors
int Posterior::cell_prep() {
  const int GS = plan.GS;
  RCHK(upload(cx, cx->models, s.models, sizeof(double) * C * 12));
  RCHK(upload(cx, cx->mag, s.mag, sizeof(double) * G));
  const size_t cg = sizeof(double) * (size_t)C * GS;
  HCHK(cx->mu.ensure(cg));
  HCHK(cx->lcfp.ensure(cg));
  HCHK(cx->cfp.ensure(cg));
  HCHK(cx->lcfpr.ensure(cg));
  HCHK(cx->theta.ensure(cg));
  HCHK(cx->cellscal.ensure(sizeof(double) * 2 * C));
  hipEvent_t ev = cx->mark_begin(SLOT_OTHER);
  if (!s.localtheta) HCHK(cx->pq.ensure(4 * cg));
  HCHK(launch_cell_prep(cx->models.as<double>(), C, G, GS, cx->mag.as<double>(), s.localtheta, s.squarelogit,
                        cx->mu.as<double>(), cx->lcfp.as<double>(), cx->lcfpr.as<double>(), cx->theta.as<double>(),
                        cx->cellscal.as<double>(), s.localtheta ? nullptr : cx->pq.as<double>(), st,
                        cx->cfp.as<double>()));
  cx->mark_end(SLOT_OTHER, ev);
  return SCDE_OK;
}

// ---- stage 2: unique counts -- the host's ucl/uci uploaded, or built on the device (prebuilt by
// build_unique_sets when u.ready; piece by piece with the tables when the counts arrive in pieces)
int Posterior::unique_counts() {
  if (s.ucl_host) {
    u.ucl_off_h.assign(s.ucl_off_host, s.ucl_off_host + C + 1);
    RCHK(upload(cx, u.ucl_off, u.ucl_off_h.data(), sizeof(long long) * (C + 1)));
    RCHK(upload(cx, u.ucl, s.ucl_host, sizeof(int) * std::max<long long>(1, u.ucl_off_h[C])));
    RCHK(upload(cx, u.uci, s.uci_host, sizeof(int) * std::max<long long>(1, (long long)N * C)));
  } else if (!u.ready && !pieces) {
    const PostSpec* sp[1] = {&s};
    UniqueSet* up[1] = {&u};
    RCHK(build_unique_sets(cx, sp, up, 1));
  }
  u.ready = false;  // consumed by this call
  return SCDE_OK;
}

// ---- stage 3: the tables (K1)
// the flag words (zeroed once per call) and the per-cell column slots the planned tables write
int Posterior::tables_flags(bool zeroed) {
  if (plan.tpath && !zeroed) {
    HCHK(cx->qflags.ensure(sizeof(int) * 40));
    HCHK(hipMemsetAsync(cx->qflags.p, 0, sizeof(int) * 40, st));
  }
  if (plan.fused) {
    HCHK(cx->base_col.ensure(sizeof(int) * std::max(1, C)));
    HCHK(cx->zcol.ensure(sizeof(int) * std::max(1, C)));
  }
  return SCDE_OK;
}

// buffers for `cap` columns (pieces: grown keeping what earlier pieces wrote) and the launch
// arguments over the whole column range
int Posterior::setup_tables(long long cap, bool keep) {
  const int GS = plan.GS;
  auto cx_sync = [this] { return ctx_streams_sync(cx); };
  const size_t ncap = (size_t)std::max<long long>(1, cap);
  if (plan.keep_T) HCHK(cx->T.grow(keep, sizeof(double) * ncap * GS, cx_sync));
  HCHK(cx->maxi.grow(keep, sizeof(int) * ncap, cx_sync));
  HCHK(cx->has_clamp.grow(keep, ncap, cx_sync));
  if (plan.tpath) HCHK(cx->ubound.grow(keep, sizeof(unsigned) * kQTiles * (ncap + 1), cx_sync));
  if (plan.fused) {
    HCHK(cx->E.grow(keep, sizeof(double) * (ncap + 1) * GS, cx_sync));
    if (plan.stretch_skip) HCHK(cx->ubound.grow(keep, sizeof(double) * 8 * (ncap + 1), cx_sync));
  }
  if (!s.localtheta) HCHK(cx->colc.grow(keep, sizeof(double) * (kColc * ncap + 1), cx_sync));  // + the slow-column flag
  ta.ucl = u.ucl.as<int>();
  ta.ucl_off = u.ucl_off.as<long long>();
  ta.ncells = C;
  ta.G = G;
  ta.GS = GS;
  ta.mu = cx->mu.as<double>();
  ta.lcfp = cx->lcfp.as<double>();
  ta.lcfpr = cx->lcfpr.as<double>();
  ta.theta = cx->theta.as<double>();
  ta.cellscal = cx->cellscal.as<double>();
  // the reference's clamp, -DBL_MAX / (cells in the call) / 1.1 (src/jpmatLogBoot.cpp:127)
  ta.minlogprob = -1 * DBL_MAX / C / 1.1;
  // rows that fit the 256 MB last-level cache can be read back from it by the bootstrap: plain
  // stores there
  ta.nt_rows = cx->opt_tables_nt == 1 || (cx->opt_tables_nt == 2 && (double)ncap * GS * sizeof(double) > 256.0 * (1 << 20));
  ta.T = plan.keep_T ? cx->T.as<double>() : nullptr;
  ta.maxi = plan.want_maxi ? cx->maxi.as<int>() : nullptr;
  ta.has_clamp = cx->has_clamp.as<unsigned char>();
  ta.const_theta = s.localtheta ? 0 : 1;
  ta.pq = s.localtheta ? nullptr : cx->pq.as<double>();
  ta.colc = s.localtheta ? nullptr : cx->colc.as<double>();
  ta.cfp = cx->cfp.as<double>();
  ta.use_baseline = s.use_baseline ? 1 : 0;
  ta.UQ = plan.tpath ? cx->ubound.as<unsigned>() : nullptr;
  ta.nanflag = plan.tpath ? cx->qflags.as<int>() : nullptr;
  ta.D = plan.fused ? cx->E.as<double>() : nullptr;
  ta.zcol = plan.fused ? cx->zcol.as<int>() : nullptr;
  ta.base_col = plan.fused ? cx->base_col.as<int>() : nullptr;
  ta.U = plan.stretch_skip ? cx->ubound.as<double>() : nullptr;
  return SCDE_OK;
}

// the tables of cells [c0, c1), whose columns [col0, col0 + nc) are described by the
// cell-local offsets off_h (device copy off_d, from 0); last: the pad column's task and p1_ev
int Posterior::launch_tables_range(int c0, int c1, long long col0, const long long* off_d,
                                   const std::vector<long long>& off_h, bool last, UniqueSet& tu) {
  const int GS = plan.GS;
  const int Cc = c1 - c0;
  const long long nc = off_h[Cc];
  TablesArgs tc = ta;
  tc.ucl = ta.ucl + col0;
  tc.ucl_off = off_d;
  tc.ncols = nc;
  tc.ncells = Cc;
  const size_t co = (size_t)c0 * GS;
  tc.mu = ta.mu + co;
  tc.lcfp = ta.lcfp + co;
  tc.lcfpr = ta.lcfpr + co;
  if (tc.cfp) tc.cfp = ta.cfp + co;
  tc.theta = ta.theta + co;
  tc.cellscal = ta.cellscal + 2 * (size_t)c0;
  if (tc.pq) tc.pq = ta.pq + 4 * co;
  if (tc.T) tc.T = ta.T + (size_t)col0 * GS;
  if (tc.maxi) tc.maxi = ta.maxi + col0;
  tc.has_clamp = ta.has_clamp + col0;
  if (tc.colc) tc.colc = ta.colc + (size_t)kColc * col0;
  if (tc.UQ) tc.UQ = ta.UQ + (size_t)kQTiles * col0;
  if (tc.U) tc.U = ta.U + (size_t)8 * col0;
  if (tc.D) tc.D = ta.D + (size_t)col0 * GS;
  if (tc.zcol) tc.zcol = ta.zcol + c0;
  if (tc.base_col) tc.base_col = ta.base_col + c0;
  tc.col_base = (int)col0;
  // cell-staged tables (G <= 448): tasks of up to 64 columns of one cell -- one lane per column in
  // k_tables_lpc (constant theta); with local theta (k_tables_cell, 8 columns per wave) a launch that
  // would fill fewer than 4 rounds of the chip's block slots takes 32-column tasks, so its last
  // round is shorter
  if (G <= 448 && nc > 0) {
    const long long kTaskCols =
        (!s.localtheta || nc / kTabTaskCols >= 4096) ? kTabTaskCols : std::min(32, kTabTaskCols);
    tu.tasks_h.clear();
    for (int c = 0; c < Cc; ++c)
      for (long long b = off_h[c]; b < off_h[c + 1]; b += kTaskCols)
        tu.tasks_h.push_back(make_int4(c, (int)b, (int)std::min(b + kTaskCols, off_h[c + 1]), 0));
    if (plan.fused && last) tu.tasks_h.push_back(make_int4(-1, 0, 0, 0));  // the ELL pad column
    RCHK(upload(cx, tu.tasks, tu.tasks_h.data(), sizeof(int4) * tu.tasks_h.size()));
    tc.tasks = tu.tasks.as<int4>();
    tc.ntasks = (int)tu.tasks_h.size();
  }
  hipEvent_t evt = cx->mark_begin(SLOT_TABLES);
  if (!s.localtheta && nc > 0)
    HCHK(launch_col_consts(tc.ucl, off_d, nc, Cc, tc.theta, GS, tc.cellscal,
                           cx->colc.as<double>() + (size_t)kColc * col0, st));
  if (plan.fused) {
    tc.phase = 1;
    HCHK(launch_tables(tc, st));
    if (last) {
      if (!cx->p1_ev) HCHK(hipEventCreateWithFlags(&cx->p1_ev, hipEventDisableTiming));
      HCHK(handoff_spin(cx, st));
      HCHK(hipEventRecord(cx->p1_ev, st));
    }
    tc.phase = 2;
    HCHK(launch_tables(tc, st));
  } else {
    HCHK(launch_tables(tc, st));
  }
  cx->mark_end(SLOT_TABLES, evt);
  return SCDE_OK;
}

// the tables of every cell in one launch sequence, for the plan of the real column count
int Posterior::whole_tables(bool flags_zeroed) {
  RCHK(tables_flags(flags_zeroed));
  RCHK(setup_tables(ncols, false));
  return launch_tables_range(0, C, 0, u.ucl_off.as<long long>(), u.ucl_off_h, true, cx->task_us);
}

// ---- stage 4: the pieces loop.  Piece j: cells [piece_c[j], piece_c[j+1]) of this spec; its unique
// sets are built (on the copy stream, beside the previous piece's tables) into u's arrays at the
// running column offset, then its tables launch.  Leaves the whole set's offsets in u.ucl_off_h.
int Posterior::pieces_loop() {
  const bool modes_pieces = this->modes_pieces();
  std::vector<long long>& ucl_off_h = u.ucl_off_h;
  HCHK(u.uci.ensure(sizeof(int) * std::max<long long>(1, (long long)N * C)));
  ucl_off_h.assign(C + 1, 0);
  long long col0 = 0;
  int jlast = 0;
  for (int j = 0; j < s.npieces; ++j)
    if (s.piece_c[j + 1] > s.piece_c[j]) jlast = j;
  // the pieces' modes read-backs start once every piece's counts are up: run beside the uploads,
  // the pageable read-backs held them back (config 4: ~1 ms per 120 MB read-back)
  if (modes_pieces) dnl_hold(cx, true);
  using pclock = std::chrono::steady_clock;
  auto pms = [](pclock::time_point a, pclock::time_point b) {
    return std::chrono::duration<double, std::milli>(b - a).count();
  };
  for (int j = 0; j < s.npieces; ++j) {
    const int c0 = s.piece_c[j], c1 = s.piece_c[j + 1];
    const auto tw = pclock::now();
    RCHK(s.piece_ready(j));
    if (j == jlast && modes_pieces) dnl_hold(cx, false);  // (every piece's counts are up)
    const auto th = pclock::now();
    cx->st_piece_wait_ms += pms(tw, th);
    struct Lap {
      scde_ctx* cx;
      pclock::time_point t;
      ~Lap() { cx->st_piece_host_ms += std::chrono::duration<double, std::milli>(pclock::now() - t).count(); }
    } lap{cx, th};
    if (c1 == c0) continue;
    UniqueSet& pu = cx->upc[j];
    PostSpec ps;
    ps.ncells = c1 - c0;
    ps.counts_dev = s.counts_dev;
    ps.ld = s.ld;
    ps.cellidx_host = s.cellidx_host + c0;
    ps.ngenes = N;
    pu.into = &u;
    pu.into_col0 = col0;
    pu.into_c0 = c0;
    pu.into_cap_hint = c0 > 0 ? (long long)((double)col0 / c0 * C * 1.1) : 0;  // leading pieces may be empty
    const PostSpec* sp[1] = {&ps};
    UniqueSet* up[1] = {&pu};
    const hipStream_t main = cx->stream;
    cx->stream = s.piece_stream;
    const int rc = build_unique_sets(cx, sp, up, 1);
    cx->stream = main;
    pu.into = nullptr;
    RCHK(rc);
    HCHK(handoff_spin(cx, s.piece_stream));
    HCHK(hipEventRecord(s.piece_ev[j], s.piece_stream));
    HCHK(handoff_wait(cx, st, s.piece_ev[j]));
    for (int c = c0; c < c1; ++c) ucl_off_h[c + 1] = col0 + pu.ucl_off_h[c - c0 + 1];
    const long long nc = pu.ucl_off_h[c1 - c0];
    // The whole set's column offsets go up on this stream BEFORE the last piece's tables: the
    // bootstrap set-up (ELL rows) reads them on the aux stream, which waits only for p1_ev, the
    // event after the last piece's phase-1 tables.  Uploaded after the loop (rounds 3-4), the ELL
    // builder could read the previous call's offsets -- identical when the same data is run again,
    // garbage after a call on other data (the r04 full-size failure).
    if (j == jlast) RCHK(upload(cx, u.ucl_off, ucl_off_h.data(), sizeof(long long) * (C + 1)));
    // capacity for this piece plus an estimate of the rest (grown keeping the columns so far)
    const long long est = std::max<long long>(col0 + nc, (long long)((double)(col0 + nc) / c1 * C * 1.1));
    RCHK(setup_tables(est, j > 0));
    RCHK(launch_tables_range(c0, c1, col0, pu.ucl_off.as<long long>(), pu.ucl_off_h, j == jlast, pu));
    if (modes_pieces) {  // the piece's posterior modes, read back while the next pieces' tables run
      HCHK(launch_modes(u.uci.as<int>() + (size_t)N * c0, N, N, c1 - c0, pu.ucl_off.as<long long>(),
                        cx->maxi.as<int>() + col0, cx->mag.as<double>(), s.modes + (size_t)N * c0, 1, N, st));
      const size_t bytes = sizeof(double) * (size_t)N * (c1 - c0);
      RCHK(dnl_push(cx, st, s.modes_host + (size_t)N * c0, bytes, s.modes + (size_t)N * c0, bytes, bytes, 1));
    }
    col0 += nc;
  }
  return SCDE_OK;
}

// Stages 5-11: everything after the tables are queued, on the same stream.
int Posterior::rest() {
  RCHK(early_modes());
  if (plan.fused && s.nboot > 0) {
    fused_draws();
    // the tables were set up for the tile path before the draws existed: a multiplicity it cannot
    // hold as a byte (or above option tile_max_mult) takes plain k_boot2 on the same D columns
    plan.tpath = plan.tpath && maxw <= std::min(127, cx->opt_tile_max_mult);
  }
  if (!bootstraps(s)) {
    RCHK(joint_without_bootstrap());
  } else {
    RCHK(boot_setup());
    hipEvent_t ev = cx->mark_begin(SLOT_BOOT);
    if (plan.fast) RCHK(boot_fast());
    else RCHK(boot_general());
    cx->mark_end(SLOT_BOOT, ev);
    if (!exact_done) RCHK(boot_exact(0, N));
  }
  return outputs();
}

// ---- stage 5: individual posterior modes (src/jpmatLogBoot.cpp:277-296): argmax of each cell's
// table column, known as soon as the tables are; computed here so the caller's read-back of the
// (ngenes x ncells) matrix overlaps the bootstrap (pieces with modes_host: done piece by piece)
int Posterior::early_modes() {
  if (!(plan.want_modes && s.modes && s.modes_early && !modes_pieces())) return SCDE_OK;
  HCHK(launch_modes(u.uci.as<int>(), N, N, C, u.ucl_off.as<long long>(), cx->maxi.as<int>(),
                    cx->mag.as<double>(), s.modes, 1, N, st));
  if (s.modes_host) {
    const size_t bytes = sizeof(double) * (size_t)N * C;
    RCHK(dnl_push(cx, st, s.modes_host, bytes, s.modes, bytes, bytes, 1));
  } else {
    if (!cx->modes_ev) HCHK(hipEventCreateWithFlags(&cx->modes_ev, hipEventDisableTiming));
    HCHK(handoff_spin(cx, st));
    HCHK(hipEventRecord(cx->modes_ev, st));
  }
  return SCDE_OK;
}

// the fused path's draws, made after the tables launch (the host's RNG work then overlaps the
// tables kernel instead of leaving the GPU idle in front of it), and the largest multiplicity
void Posterior::fused_draws() {
  if (plan.dev_mult) {
    make_draws(s, plan.Bp, draws, W, ndraw, &maxw, false);
  } else {
    make_draws(s, plan.Bp, draws, W, ndraw);
    maxw = 0;
    for (double w : W) maxw = std::max(maxw, (int)w);
  }
}

// ---- stage 6: the joint posterior without a bootstrap
int Posterior::joint_without_bootstrap() {
  const int GS = plan.GS;
  if (!s.batch_call && s.ensemble) {
    HCHK(cx->E.ensure(sizeof(double) * std::max<long long>(1, ncols) * GS));
    HCHK(launch_ensemble_cols(cx->T.as<double>(), ncols, G, GS, cx->E.as<double>(), st));
    NoBootArgs na{cx->E.as<double>(), G, GS, u.ucl_off.as<long long>(), u.uci.as<int>(), N, C, N, 1,
                  s.jp, s.jp_g, s.jp_k};
    HCHK(launch_noboot(na, st));
  } else if (!s.batch_call) {
    NoBootArgs na{cx->T.as<double>(), G, GS, u.ucl_off.as<long long>(), u.uci.as<int>(), N, C, N, 0,
                  s.jp, s.jp_g, s.jp_k};
    HCHK(launch_noboot(na, st));
  } else {
    // logBootBatchPosterior with Nboot = 0 returns zeros (src/jpmatLogBoot.cpp:469-497)
    HCHK(hipMemsetAsync(s.jp, 0, sizeof(double) * (size_t)N * G, st));
  }
  return SCDE_OK;
}

BootLayout Posterior::boot_layout() const {
  const int nb = plan.nb;
  BootLayout b{};
  b.nsets = (int)s.seeds.size();
  b.P = (s.nboot + nb - 1) / nb;
  // + one look-ahead batch (k_boot2); the tile path's bounds read whole 64-entry steps
  b.stride = plan.tpath ? plan.qstride : (int)round_up(C, 8) + 8;
  // the tile path's first pass, k_boot_gene: groups of gene_sg slabs per 4-wave block (measured
  // against the former wave-per-slab pair mode at config 4: bootstrap 11.16 -> 9.94 ms per step)
  b.gene_sg = plan.tpath ? std::min({b.P, 8, 128 / nb}) : 0;
  // gene chunks (scde.posteriors, R-layout jp): the bootstrap over genes [gch(k), gch(k + 1))
  // finishes (list pass, fallback, slab sums, exact rows) before chunk k + 1 starts; with jp_host,
  // chunk k's jp rows go back to the host while it runs -- the read-back of the last chunk only is
  // left after the bootstrap.  Calls without the read-back thread (modes_overlap 0, the profiling
  // runs) chunk too, in the descending order below, whose L2 reuse is better (config 4: 29.1 ->
  // 24.1 GB of counter bytes, 10.8 -> 9.85 ms of k_boot_gene per step)
  const bool post_layout = s.jp_g == 1 && s.jp_k == N;
  b.nchunks = (plan.tpath && post_layout) ? std::max(1, std::min(cx->opt_jp_chunks, N / 256 + 1)) : 1;
  // tile path: genes in order of their count sums (waves in flight share columns in L2), keyed by
  // the ELL builder; with gene chunks each chunk's genes in order among themselves (the chunk
  // index in the keys' top bits: one sort)
  b.have_order = plan.tpath && plan.fast && cx->opt_tile_order && N > 1;
  // descending (heaviest genes first, shorter tail) for small launches; ascending for large ones.
  // Measured (bootstrap ms per step, ascending -> descending): config 4's 7,500-gene chunks 10.59
  // -> 9.77, config 3's shard of 8 (2,500 genes per lane) 0.70 -> 0.63, config 3 (20,000 genes
  // per lane) 3.95 -> 4.09
  // scde.posteriors (R-layout jp) takes descending order at every chunk size (config 4, k_boot_gene
  // per step, ascending -> descending: chunks of 10,000 genes 26.9 -> 23.9 GB of counter bytes,
  // 10.3 -> 9.77 ms; one launch of 30,000 genes 29.1 -> 24.4 GB)
  constexpr int kDescGenes = 8192;
  b.order_desc = cx->opt_tile_order == 2 ||
                 (cx->opt_tile_order == 3 && (post_layout || (N + b.nchunks - 1) / b.nchunks <= kDescGenes));
  return b;
}

// Host multiplicities as bytes (above kMultMaxCells cells; else launch_mult forms them on the
// device), in launch_mult's three layouts: w8 [set][cell][boot] (baseline bound sums and the tile
// bounds); w8t, for the tile bounds' A fragments, per slab the pairs (boot r, boot 16 + r) of its nb
// boots, so one 16-bit load serves both 16-boot MFMA tiles; w8g (k_boot_gene), per (cell, group of
// gene_sg slabs) four 32-boot windows as pair slots.
int Posterior::upload_host_mult(hipStream_t sa) {
  const int nb = plan.nb, Bp = plan.Bp, Bt = plan.Bt, P = bl.P, SG = bl.gene_sg, NGR = (P + SG - 1) / SG;
  const size_t sc = (size_t)bl.nsets * C;
  auto pair_slot = [](int j) -> size_t { return j < 16 ? 2 * j : 2 * (j - 16) + 1; };  // j in [0, 32)
  std::vector<unsigned char> w8(sc * Bt, 0), w8t(sc * P * 32, 0), w8g(sc * NGR * 128, 0);
  for (size_t r = 0; r < sc; ++r) {  // r = set * C + cell
    const double* wr = W.data() + r * Bp;
    for (int b = 0; b < Bp; ++b) w8[r * Bt + b] = (unsigned char)wr[b];
    for (int sl = 0; sl < P; ++sl)
      for (int j = 0; j < 32 && j < nb; ++j) {
        const int b = sl * nb + j;
        if (b >= Bp) continue;
        w8t[(r * P + sl) * 32 + pair_slot(j)] = (unsigned char)wr[b];
      }
    for (int gr = 0; gr < NGR; ++gr) {
      const int gb0 = gr * SG * nb, gnb = std::min(SG, P - gr * SG) * nb;
      for (int j = 0; j < gnb && j < 128; ++j) {
        const int b = gb0 + j;
        if (b >= Bp) break;
        w8g[(r * NGR + gr) * 128 + 32 * (j >> 5) + pair_slot(j & 31)] = (unsigned char)wr[b];
      }
    }
  }
  RCHK(upload_on(cx, cx->w8, w8.data(), w8.size(), sa));
  RCHK(upload_on(cx, cx->w8t, w8t.data(), w8t.size(), sa));
  RCHK(upload_on(cx, cx->w8g, w8g.data(), w8g.size(), sa));
  return SCDE_OK;
}

// ---- stage 7: the bootstrap's set-up.  Fused path: it reads only phase 1's count-0 columns, so it
// runs on the aux stream, beside phase 2 of the tables, and the main stream joins it at the end.
int Posterior::boot_setup() {
  const int GS = plan.GS, nb = plan.nb, Bp = plan.Bp, Bt = plan.Bt;
  const bool fused = plan.fused, tpath = plan.tpath;
  if (!fused) make_draws(s, Bp, draws, W, ndraw);
  bl = boot_layout();
  const int nsets = bl.nsets;
  hipStream_t sa = st;
  if (fused) {
    if (!cx->aux_stream) HCHK(hipStreamCreateWithFlags(&cx->aux_stream, hipStreamNonBlocking));
    if (!cx->aux_ev) HCHK(hipEventCreateWithFlags(&cx->aux_ev, hipEventDisableTiming));
    sa = cx->aux_stream;
    HCHK(handoff_wait(cx, sa, cx->p1_ev));
  }
  if (!plan.dev_mult) RCHK(upload_on(cx, cx->Wt, W.data(), sizeof(double) * W.size(), sa));
  RCHK(upload_on(cx, cx->draws, draws.data(), sizeof(int) * draws.size(), sa));
  if (!fused) {
    HCHK(cx->base_col.ensure(sizeof(int) * C));
    HCHK(launch_base_cols(u.ucl.as<int>(), u.ucl_off.as<long long>(), C, cx->has_clamp.as<unsigned char>(),
                          s.use_baseline ? 1 : 0, cx->base_col.as<int>(), st));
  }
  HCHK(cx->ent.ensure(sizeof(int2) * std::max<long long>(1, (long long)N * bl.stride)));
  HCHK(cx->nnz.ensure(sizeof(int) * std::max(1, N)));
  hipEvent_t ev = cx->mark_begin(SLOT_OTHER);
  if (!fused) {
    HCHK(cx->E.ensure(sizeof(double) * (size_t)(ncols + 1) * GS));
    HCHK(launch_delta(cx->T.as<double>(), u.ucl_off.as<long long>(), C, ncols, cx->base_col.as<int>(), G, GS,
                      cx->E.as<double>(), st));
  }
  // the baseline columns: T (slow path) or the fused D buffer, which holds T there
  const double* Tbase = fused ? cx->E.as<double>() : cx->T.as<double>();
  if (bl.have_order) {
    HCHK(cx->gkey.ensure(sizeof(unsigned) * N));
    HCHK(cx->gkey2.ensure(sizeof(unsigned) * N));
    HCHK(cx->gidx.ensure(sizeof(int) * N));
    HCHK(cx->gorder.ensure(sizeof(int) * N));
  }
  // ELL rows (and the gene-order keys)
  HCHK(launch_ell(u.uci.as<int>(), N, N, C, u.ucl_off.as<long long>(), cx->base_col.as<int>(), bl.stride, (int)ncols,
                  tpath ? 64 : 8, cx->ent.as<int2>(), cx->nnz.as<int>(), sa, 0,
                  bl.have_order ? u.ucl.as<int>() : nullptr, bl.have_order ? cx->gkey.as<unsigned>() : nullptr,
                  bl.have_order ? cx->gidx.as<int>() : nullptr, 0, N, bl.nchunks, bl.order_desc));
  if (bl.have_order) {
    size_t wb = 0;
    HCHK(launch_gene_order(nullptr, nullptr, N, nullptr, nullptr, nullptr, &wb, sa));
    HCHK(cx->gwork.ensure(std::max<size_t>(wb, 1)));
    HCHK(launch_gene_order(cx->gkey.as<unsigned>(), cx->gidx.as<int>(), N, cx->gkey2.as<unsigned>(),
                           cx->gorder.as<int>(), cx->gwork.p, &wb, sa));
  }
  if (plan.dev_mult) {
    // the multiplicity arrays from the uploaded draw lists, on the device (host loops over
    // sets x cells x boots and their uploads cost ~0.1-0.4 ms of host time per posterior)
    const int NGR = tpath ? (bl.P + bl.gene_sg - 1) / bl.gene_sg : 0;
    const size_t sc = (size_t)nsets * C;
    HCHK(cx->Wt.ensure(sizeof(double) * std::max<size_t>(1, sc * Bp)));
    if (tpath) {
      HCHK(cx->w8.ensure(std::max<size_t>(1, sc * Bt)));
      HCHK(cx->w8t.ensure(std::max<size_t>(1, sc * bl.P * 32)));
      HCHK(cx->w8g.ensure(std::max<size_t>(1, sc * NGR * 128)));
    }
    HCHK(launch_mult(cx->draws.as<int>(), nsets, s.nboot, ndraw, C, Bp, cx->Wt.as<double>(), Bt,
                     tpath ? cx->w8.as<unsigned char>() : nullptr, nb, bl.P,
                     tpath ? cx->w8t.as<unsigned char>() : nullptr, bl.gene_sg, NGR,
                     tpath ? cx->w8g.as<unsigned char>() : nullptr, sa));
  } else if (tpath) {
    RCHK(upload_host_mult(sa));
  }
  if (tpath) {
    HCHK(cx->zubound.ensure(sizeof(int) * (size_t)nsets * 4 * kQTiles * Bt));
    HCHK(launch_zuq(cx->ubound.as<unsigned>(), cx->base_col.as<int>(), C, cx->w8.as<unsigned char>(), Bt, nsets,
                    cx->zubound.as<int>(), sa));
  }
  HCHK(cx->Z.ensure(sizeof(double) * (size_t)nsets * Bp * GS));
  HCHK(launch_baseline_z(Tbase, G, GS, cx->base_col.as<int>(), C, cx->Wt.as<double>(), Bp, nsets,
                         cx->Z.as<double>(), sa));
  if (plan.stretch_skip) {
    HCHK(cx->zubound.ensure(sizeof(double) * 8 * (size_t)nsets * Bp));
    HCHK(launch_stretch_zu(cx->ubound.as<double>(), cx->base_col.as<int>(), C, cx->Wt.as<double>(), Bp, nsets,
                           cx->zubound.as<double>(), sa));
  }
  cx->mark_end(SLOT_OTHER, ev);
  if (nsets > 1) {
    if ((int)s.wset.size() != N) return fail(SCDE_EINTERNAL, "wset size mismatch");
    RCHK(upload_on(cx, cx->wset, s.wset.data(), sizeof(int) * N, sa));
  }
  HCHK(cx->degen.ensure(sizeof(int) * std::max(1, N)));
  HCHK(hipMemsetAsync(cx->degen.p, 0, sizeof(int) * std::max(1, N), sa));
  if (sa != st) {  // the bootstrap waits for the set-up and for phase 2
    HCHK(handoff_spin(cx, sa));
    HCHK(hipEventRecord(cx->aux_ev, sa));
    HCHK(handoff_wait(cx, st, cx->aux_ev));
  }
  return SCDE_OK;
}

// ---- the bootstrap kernels' argument blocks: what all three share
template <class Args>
void Posterior::set_boot_common(Args& a) const {
  a.G = G;
  a.GS = plan.GS;
  a.nboot = s.nboot;
  a.wset = bl.nsets > 1 ? cx->wset.as<int>() : nullptr;
  a.norm_mult = (double)s.nboot;
  a.degen = cx->degen.as<int>();
  a.out = s.jp;
  a.out_g = s.jp_g;
  a.out_k = s.jp_k;
  a.ngenes = N;
}

// and what the kernels that sum (k_boot2 and its tile passes, k_boot) share
template <class Args>
void Posterior::set_boot_sums(Args& a) const {
  set_boot_common(a);
  a.ent = cx->ent.as<int2>();
  a.nnz = cx->nnz.as<int>();
  a.ent_stride = bl.stride;
  a.Wt = cx->Wt.as<double>();
  a.Bp = plan.Bp;
  a.ncells = C;
  a.Z = cx->Z.as<double>();
  a.degen_thresh = 16777216.0;  // 2^24: beyond this the sums' rounding order matters
}

// k_boot2's arguments, with the partial rows' and the stretch mask's buffers
int Posterior::boot2_args(Boot2Args& b2) {
  const size_t slabs = (size_t)bl.P * N;
  set_boot_sums(b2);
  b2.D = cx->E.as<double>();
  b2.ncols_p1 = ncols + 1;
  b2.nb = plan.nb;
  b2.part_stride = (long long)N * plan.GS;
  HCHK(cx->part.ensure(sizeof(double) * std::max<size_t>(1, slabs * plan.GS)));
  b2.part = cx->part.as<double>();
  // the stretch mask's heuristic slack grows with the cells per call (the kernel's default reads
  // ncells, which counts both groups when fused): set here from the cells of one call
  b2.slack = std::isnan(cx->opt_skip_slack) ? 20.0 + 0.15 * C : cx->opt_skip_slack;
  b2.U = plan.stretch_skip ? cx->ubound.as<double>() : nullptr;
  b2.ZU = plan.stretch_skip ? cx->zubound.as<double>() : nullptr;
  if (plan.stretch_skip) {
    HCHK(cx->smask.ensure(sizeof(int) * std::max<size_t>(1, slabs)));
    HCHK(cx->subuf.ensure(sizeof(double) * 8 * plan.nb * std::max<size_t>(1, slabs)));
    HCHK(cx->sredo.ensure(sizeof(int) * (slabs + 1)));
    b2.mask = cx->smask.as<int>();
    b2.ubuf = cx->subuf.as<double>();
    b2.redo = cx->sredo.as<int>();
  }
  return SCDE_OK;
}

// the tile path's arguments and buffers (b2.redo: its fallback flags, list length and list)
int Posterior::tile_args(Boot2Args& b2, TileBootArgs& tb) {
  const size_t slabs = (size_t)bl.P * N;
  HCHK(cx->sredo.ensure(sizeof(int) * (2 * slabs + 1)));
  b2.redo = cx->sredo.as<int>();
  tb.W8p = cx->w8t.as<unsigned char>();
  tb.Bq = plan.Bt;
  tb.UQ = cx->ubound.as<unsigned>();
  tb.ZUq = cx->zubound.as<int>();
  tb.nanflag = cx->qflags.as<int>();
  tb.maxgroups = cx->opt_tile_groups;
  tb.stats = cx->opt_skip_stats ? cx->qflags.as<int>() + 2 : nullptr;
  HCHK(cx->pmask.ensure(sizeof(unsigned) * std::max<size_t>(1, slabs)));
  tb.pmask = cx->pmask.as<unsigned>();
  HCHK(cx->pwide.ensure(sizeof(int) * (1 + slabs)));
  tb.wide = cx->pwide.as<int>();
  tb.SG = bl.gene_sg;
  tb.kcap = cx->opt_gene_rows;
  tb.list_cap = cx->opt_gene_list_cap;
  tb.W8g = cx->w8g.as<unsigned char>();
  HCHK(cx->gdone.ensure(sizeof(int) * std::max(1, N)));
  tb.gdone = cx->gdone.as<int>();
  if (bl.have_order) tb.order = cx->gorder.as<int>();
  return SCDE_OK;
}

// ---- stage 8: the fast bootstrap (G <= 1024): k_boot2 on the D columns, with the stretch mask, or
// the tile path -- in gene chunks when jp goes back in R's layout, each chunk finished (exact rows
// included) and its jp rows on their way to the host before the next starts
int Posterior::boot_fast() {
  const int nchunks = bl.nchunks;
  Boot2Args b2{};
  RCHK(boot2_args(b2));
  cx->st_boot_path = plan.tpath ? 1 : 0;
  if (plan.tpath) {
    TileBootArgs tb{};
    RCHK(tile_args(b2, tb));
    if (nchunks > 1) {
      for (int k = 0; k < nchunks; ++k) {
        tb.g_lo = (int)((long long)N * k / nchunks);
        tb.g_hi = (int)((long long)N * (k + 1) / nchunks);
        HCHK(launch_boot_tiles(b2, tb, st));
        RCHK(boot_exact(tb.g_lo, tb.g_hi));
        if (!s.jp_host) continue;
        // chunk k's rows of the ngenes x ngrid column-major jp
        const size_t pitch = sizeof(double) * N;
        RCHK(dnl_push(cx, st, s.jp_host + tb.g_lo, pitch, s.jp + tb.g_lo, pitch,
                      sizeof(double) * (tb.g_hi - tb.g_lo), G));
      }
      jp_sent = s.jp_host != nullptr;
    } else {
      HCHK(launch_boot_tiles(b2, tb, st));
    }
    if (cx->opt_skip_stats) RCHK(tile_stats());
  } else {
    HCHK(launch_boot2(b2, st));
  }
  if (plan.stretch_skip && cx->opt_skip_stats) RCHK(stretch_stats());  // diagnostics
  return SCDE_OK;
}

// option skip_stats, tile path: the kernels' counters (qflags) into the context's statistics
int Posterior::tile_stats() {
  int h[40];
  HCHK(hipMemcpyAsync(h, cx->qflags.p, sizeof(int) * 40, hipMemcpyDeviceToHost, st));
  HCHK(hipStreamSynchronize(st));
  for (int i = 0; i <= scde_ctx::kQMaxTilesHost; ++i) cx->st_tile_hist[i] += h[8 + i];
  cx->st_skip_slabs += h[2];
  cx->st_skip_kept += h[3];
  cx->st_skip_stretches += h[4];
  cx->st_skip_redo += h[5];
  cx->st_pair_redo += h[37];
  cx->st_boot_f64_fma += (double)h[6] * 64.0 * plan.nb + (double)h[7] * plan.nb * (double)round_up(G, 64);
  return SCDE_OK;
}

// option skip_stats, stretch path: kept stretches and redo slabs from the mask and the redo flags
int Posterior::stretch_stats() {
  const int P = bl.P, nb = plan.nb;
  std::vector<int> m((size_t)P * N), r((size_t)P * N), nz(N);
  HCHK(hipMemcpyAsync(m.data(), cx->smask.p, sizeof(int) * m.size(), hipMemcpyDeviceToHost, st));
  HCHK(hipMemcpyAsync(r.data(), cx->sredo.p, sizeof(int) * r.size(), hipMemcpyDeviceToHost, st));
  HCHK(hipMemcpyAsync(nz.data(), cx->nnz.p, sizeof(int) * nz.size(), hipMemcpyDeviceToHost, st));
  HCHK(hipStreamSynchronize(st));
  const int nst = (G + 63) / 64;
  long long kept = 0, redo = 0;
  double fma = 0;
  for (size_t i = 0; i < m.size(); ++i) {  // i = g * P + p
    const int k = __builtin_popcount((unsigned)m[i]);
    kept += k;
    redo += r[i] != 0;
    fma += (double)(k + (r[i] != 0 ? nst : 0)) * 64.0 * nb * nz[i / P];
  }
  cx->st_boot_f64_fma += fma;
  cx->st_skip_slabs += (double)m.size();
  cx->st_skip_stretches += (double)(m.size() * nst);
  cx->st_skip_kept += (double)kept;
  cx->st_skip_redo += (double)redo;
  return SCDE_OK;
}

// ---- stage 9: the general bootstrap (k_boot on T: above 1,024 grid points, or past 32-bit offsets)
int Posterior::boot_general() {
  BootArgs ba{};
  set_boot_sums(ba);
  ba.T = cx->T.as<double>();
  ba.base_col = cx->base_col.as<int>();
  cx->st_boot_path = 3;
  HCHK(launch_boot(ba, st));
  return SCDE_OK;
}

// ---- stage 10: rows whose sums left the exact range, in the reference's order (genes [g_lo, g_hi))
int Posterior::boot_exact(int g_lo, int g_hi) {
  ExactArgs xa{};
  set_boot_common(xa);
  xa.T = plan.fused ? cx->E.as<double>() : cx->T.as<double>();
  xa.base_col = plan.fused ? cx->base_col.as<int>() : nullptr;
  xa.draws = cx->draws.as<int>();
  xa.ndraw = ndraw;
  xa.ucl_off = u.ucl_off.as<long long>();
  xa.uci = u.uci.as<int>();
  xa.ld_uci = N;
  xa.g_lo = g_lo;
  xa.g_hi = g_hi;
  HCHK(launch_boot_exact(xa, st));
  exact_done = true;
  return SCDE_OK;
}

// ---- stage 11: what is left to hand out -- jp to the host when no gene chunk sent it, and the
// individual outputs (src/jpmatLogBoot.cpp:277-328)
int Posterior::outputs() {
  if (s.jp_host && !jp_sent) {
    if (s.jp_g != 1 || s.jp_k != N) return fail(SCDE_EINTERNAL, "jp_host: jp not in R layout");
    const size_t bytes = sizeof(double) * (size_t)N * G;
    if (bytes) RCHK(dnl_push(cx, st, s.jp_host, bytes, s.jp, bytes, bytes, 1));
  }
  if (plan.want_modes && s.modes && !s.modes_early) {
    HCHK(launch_modes(u.uci.as<int>(), N, N, C, u.ucl_off.as<long long>(), cx->maxi.as<int>(),
                      cx->mag.as<double>(), s.modes, 1, N, st));
    if (s.modes_host) {
      const size_t bytes = sizeof(double) * (size_t)N * C;
      RCHK(dnl_push(cx, st, s.modes_host, bytes, s.modes, bytes, bytes, 1));
    }
  }
  if (plan.want_post && s.post)
    for (int c = 0; c < C; ++c)
      HCHK(launch_post(u.uci.as<int>(), N, N, c, u.ucl_off.as<long long>(), cx->T.as<double>(), G, plan.GS,
                       s.post + (size_t)c * N * G, 1, N, st));
  return SCDE_OK;
}

}  // namespace

// rest (nullable): return once the tables are queued, with the remaining work (modes, draws,
// bootstrap, outputs) in *rest, to be run later on the same stream -- de_run queues both groups'
// tables before either bootstrap, so the second lane's tables start at once
int scde::host::run_posterior(scde_ctx* cx, const PostSpec& s, UniqueSet& u, std::function<int()>* rest) {
  RCHK(validate(s));
  const std::shared_ptr<Posterior> state = std::make_shared<Posterior>(cx, s, u);
  Posterior& p = *state;
  RCHK(p.cell_prep());
  RCHK(p.unique_counts());
  if (!p.pieces) p.plan = make_plan(cx, s, u.ucl_off_h[p.C]);
  const Plan plan0 = p.plan;  // (pieces: for 0 columns)
  RCHK(p.tables_flags(false));
  bool tables_done = false;
  if (p.pieces) {
    RCHK(p.pieces_loop());
    p.plan = make_plan(cx, s, u.ucl_off_h[p.C]);
    tables_done = p.plan == plan0;  // else: the whole tables again, planned for the real column count
  }
  p.ncols = u.ucl_off_h[p.C];
  if (!tables_done) RCHK(p.whole_tables(plan0.tpath));
  if (rest) {
    *rest = [state] { return state->rest(); };
    return SCDE_OK;
  }
  return p.rest();
}
