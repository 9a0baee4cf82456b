/*
 * scde_hip.h -- C ABI of the MI355X-native scde differential-expression path.
 *
 * Two layers:
 *
 *  1. Drop-in replacements for the five native entry points the reference
 *     resolves by name through `.Call(..., PACKAGE = "scde")`
 *     (NAMESPACE:29 useDynLib(scde); no R_registerRoutines).  Arguments are
 *     the R objects the R glue passes, flattened to plain pointers:
 *     matrices are R column-major, list-of-int-vectors become (values,
 *     offsets[n+1]).  Host pointers in, host pointers out; the GPU work is
 *     internal.  The `.Call` shim a maintainer would add is in INTEGRATION.md.
 *
 *  2. The device-resident pipeline (what bench.py times): counts stay in HBM,
 *     one call runs scde.expression.difference for one batch of genes.
 *
 * Every function returns 0 on success or a nonzero SCDE_E* code; the message
 * is available from scde_last_error() (thread-local).  Errors are never
 * silently replaced by a CPU fallback: there is none.
 */
#ifndef SCDE_HIP_H
#define SCDE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCDE_OK 0
#define SCDE_EARG 1   /* invalid argument / shape */
#define SCDE_EHIP 2   /* HIP runtime error (no device, launch failure, OOM) */
#define SCDE_EINTERNAL 3
#define SCDE_EFORK 4  /* a GPU entry in a process forked after this library initialised HIP
                         in its parent (R's mclapply after an n.cores = 1 call): the child
                         cannot use the inherited runtime; nothing was run */

const char* scde_last_error(void);
int scde_version(void); /* 100 * major + minor */

/* Which C-library rand() the bootstrap draws reproduce (the reference calls the
 * platform's srand()/rand(), src/jpmatLogBoot.cpp:221,256):
 *   SCDE_RAND_GLIBC  glibc TYPE_3 (Linux; the default)
 *   SCDE_RAND_DARWIN Darwin/BSD libc Park-Miller (macOS; reproduces the vignette)
 * Process-wide default for layer 1 and scde_posteriors_dev; also read once from
 * the environment variable SCDE_RAND=glibc|darwin. */
#define SCDE_RAND_GLIBC 0
#define SCDE_RAND_DARWIN 2
int scde_set_rand_kind(int kind);
int scde_get_rand_kind(void);

/* ---------------------------------------------------------------- layer 1 */

/* Replaces logBootPosterior  (src/jpmatLogBoot.cpp:100, decl src/jpmatLogBoot.h:8).
 *  models     ncells x 12 col-major (R `mm`, NaN where a column is absent)
 *  ucl_vals   concatenated Ucl list (unique counts per cell), ucl_off[ncells+1]
 *  counti     ngenes x ncells col-major, 0-based index into the cell's Ucl
 *  magnitudes ngrid natural-log magnitudes (marginals)
 *  outputs    jp    ngenes x ngrid col-major                   (always)
 *             modes ngenes x ncells col-major       (return_post in {1,3})
 *             post  ncells consecutive ngenes x ngrid col-major blocks (return_post in {2,3})
 *
 * Deviation from the reference (this entry and every other that forms posterior tables): a model
 * row for which the reference fills the cell's tables, and with them every row of the joint
 * posterior, with NaN is refused with SCDE_EARG before any table is formed (layer 1: before
 * anything is launched), the message naming the model row and the column:
 *   - corr.a / corr.b whose mean exp(mag corr.a + corr.b) is NaN or infinite at a grid point
 *     (a non-positive corr.a on a grid whose first magnitude is -inf; corr.b = 800);
 *   - conc.a / conc.b (conc.a2) whose exponent is NaN at a grid point (conc.a = 0 on such a grid);
 *   - fail.r NaN;
 *   - constant theta (corr.theta) NaN, infinite, zero or negative, or so small against the
 *     largest mean that theta / (theta + mu) rounds to 0 (5e-324);
 *   - a NaN magnitude.
 * Finite tables of extreme models (non-positive slopes on a finite grid, cfp = 0 or 1, fail.r
 * = -inf or overflowing, theta from 1e-8 to 1.7e308) are formed as the reference forms them.
 */
int scde_logBootPosterior(const double* models, int ncells, const int* ucl_vals, const int64_t* ucl_off,
                          const int* counti, int ngenes, const double* magnitudes, int ngrid, int nboot, int seed,
                          int return_post, int local_theta, int square_logit_conc, int ensemble, double* jp,
                          double* modes, double* post);

/* Replaces logBootBatchPosterior  (src/jpmatLogBoot.cpp:343, decl .h:9).
 *  batch_vals/batch_off: BatchIL (0-based cell indices per batch level), nbatch levels
 *  composition: nbatch draws-per-boot counts (R `table(batch[ii])`).
 *  return_post 3 is not handled by the reference (falls through to jp only); same here. */
int scde_logBootBatchPosterior(const double* models, int ncells, const int* ucl_vals, const int64_t* ucl_off,
                               const int* counti, int ngenes, const double* magnitudes, int ngrid,
                               const int* batch_vals, const int64_t* batch_off, const int* composition, int nbatch,
                               int nboot, int seed, int return_post, int local_theta, int square_logit_conc,
                               double* jp, double* modes, double* post);

/* Replaces jpmatLogBoot  (src/jpmatLogBoot.cpp:11, decl .h:6).  mats: nmat pointers
 * to nrows x ncols col-major log-posterior matrices.  out: nrows x ncols col-major. */
int scde_jpmatLogBoot(const double* const* mats, int nmat, int nrows, int ncols, int nboot, int seed, double* out);

/* Replaces jpmatLogBatchBoot  (src/jpmatLogBoot.cpp:48, decl .h:7).  Matll flattened:
 * type k owns mats[type_off[k] .. type_off[k+1]); comp[k] draws per boot. */
int scde_jpmatLogBatchBoot(const double* const* mats, const int* type_off, const int* comp, int ntypes, int nrows,
                           int ncols, int nboot, int seed, double* out);

/* Replaces matSlideMult  (src/matSlideMult.cpp:5, decl src/matSlideMult.h:6).
 * m1, m2: nrows x ncols col-major; out: nrows x (2*ncols-1) col-major. */
int scde_matSlideMult(const double* m1, const double* m2, int nrows, int ncols, double* out);

/* calculate.ratio.posterior + quick.distribution.summary (R/functions.R:3491-3510,
 * 5039-5050) on host buffers.  prior_y may be NULL (skip.prior.adjustment).
 * diffv: 2n-1 column values (as.numeric(colnames)), zi: 0-based index of the
 * expectation column.  ratio (nrows x (2n-1) col-major) and res (nrows x 5
 * col-major: lb, mle, ub, ce, Z) may each be NULL. */
int scde_ratio_summary(const double* pmat1, const double* pmat2, int nrows, int n, const double* prior_y,
                       const double* diffv, int zi, double* ratio, double* res);

/* quick.distribution.summary of an existing ratio posterior (R/functions.R:5039-5050):
 * rpost nrows x m col-major (m odd, rows already normalised), diffv m values, zi the
 * expectation column.  res: nrows x 5 col-major (lb, mle, ub, ce, Z). */
int scde_distribution_summary(const double* rpost, int nrows, int m, const double* diffv, int zi, double* res);

/* BH-adjusted cZ = sign(Z) qnorm(p.adjust(pnorm(|Z|, lower=F), "BH"), lower=F)
 * (R/functions.R:5051).  Host-only. */
int scde_bh_cz(const double* z, int64_t n, double* cz);

/* ---------------------------------------------------------------- layer 2 */

typedef struct scde_ctx scde_ctx;

int scde_ctx_create(int device, scde_ctx** out);
void scde_ctx_destroy(scde_ctx* ctx);
int scde_ctx_synchronize(scde_ctx* ctx);
/* Per-kernel HIP-event timing on the context's stream (0 = off). */
int scde_ctx_set_profiling(scde_ctx* ctx, int on);
/* slot names: 0 tables, 1 boot, 2 ratio_summary, 3 unique, 4 other, 5 prior_stats,
 * 6 prior_bin, 7 prior_tail; ms totals and launch counts */
int scde_ctx_kernel_times(scde_ctx* ctx, double* ms, int64_t* launches, int nslots);
int scde_ctx_reset_kernel_times(scde_ctx* ctx);
/* Options of a context: 20, each the switch of a default path or a documented operating / test mode
 * (defaults are the product settings; the environment is read once, at context creation, for
 * SCDE_OPTIONS -- see scde_ctx_set_option).  Every one leaves the results unchanged unless noted.
 * Bootstrap paths:
 *   "boot_tiles"    1/0  the FP64 bootstrap on bounded 32-point tiles (k_boot_gene gene blocks, their
 *                   four-tile list pass k_boot_tiles; default 1) or k_boot2's 64-point stretches (0)
 *   "boot_tiles_cells"  the cell count from which the tile path is used (default 400; below: k_boot2's
 *                   64-point stretch mask -- config 2b's 200-cell batch posteriors: 8.2 ms of
 *                   bootstrap per step with it against 12.0 with gene blocks)
 *   "boot_skip"     1/0  grid-stretch / tile skipping in the bootstrap (default 1)
 *   "boot_nb"       boots per bootstrap slab (0 = automatic; a multiple of 4 in [4, 32])
 *   "tile_order"    0..3  the tile bootstrap takes the genes in order of their count sums,
 *                   so waves in flight share columns and tiles in L2: 1 ascending, 2 descending
 *                   (heaviest genes first: a shorter tail), 3 (default) descending in
 *                   scde.posteriors calls and in DE launches of at most 8,192 genes, ascending in
 *                   larger DE launches, 0 gene order
 * Test modes forcing the bootstrap's second-chance paths (each must still give the same bits):
 *   "skip_slack"    mask heuristic slack (NaN = default 20 + 0.15 C; negative: redo slabs)
 *   "tile_groups"   32-point tiles the list pass computes per slab, 1..4 (default 4; with 2, slabs
 *                   needing more go to k_boot2 whole)
 *   "tile_max_mult" the largest draw multiplicity the tile path takes (default 127, the int8 bound
 *                   operand; a call with a larger one runs plain k_boot2 on the same columns)
 *   "gene_rows"     1..4 rows per slab a gene block gives each slab at most (default 4; fewer:
 *                   the four-tile list pass takes the rest)
 *   "gene_list_cap" slabs the list pass takes at most (0 = 16384; beyond: k_boot2)
 *   "skip_stats"    1/0  count kept stretches and redo slabs (one host sync per launch)
 * Host pipeline:
 *   "lanes"         2/1  a DE call's second group runs on a peer context (its own streams and
 *                   workspace, same device) beside the first (default 2), or after it (1; bench's
 *                   per-stage timing pass and the rocprof runs use 1).  Memory: the peer holds a
 *                   second grow-only workspace (tables, deltas, slab partials, joint posterior:
 *                   about 2.3 GB at 20k genes x 500 cells per group), so two
 *                   lanes roughly double a DE call's device footprint; setting 1 releases the peer
 *   "pipeline_mb"   host-count DE / scde.posteriors calls whose matrix has at least this many MB
 *                   upload on a copy stream in column pieces that the kernels follow (default 32)
 *   "pieces"        pieces of that upload (the DE call's first group; the posteriors call's
 *                   selected cells), 1..8 (default 5)
 *   "upload_u16"    0..2  host-count ranges of 8 MB or more go up as 16-bit counts: narrowed by 4
 *                   host threads into a pinned ring, widened on the device, counts outside
 *                   [0, 65535] listed and patched in (half the PCIe bytes): 1 (default) in
 *                   scde_posteriors_host calls, 2 in every host entry, 0 none
 *   "modes_overlap" 1/0  scde.posteriors' read-backs run on a read-back thread beside the device
 *                   work (default 1): the modes piece by piece as each piece's tables finish, the
 *                   joint posterior in gene chunks of the bootstrap; 0: both after the bootstrap on
 *                   the main stream (rocprofv3 runs)
 *   "jp_chunks"     1..64 gene chunks of scde.posteriors' gene-block bootstrap (default 4, at most
 *                   one per 256 genes; with or without modes_overlap): each chunk finishes before
 *                   the next starts (chunks of <= 8192 genes run heaviest genes first, which shares
 *                   more columns in L2) and, with modes_overlap, its joint posterior rows are read
 *                   back while the next runs
 * Tables and other kernels:
 *   "unique_fixed"  1/0  build each call's unique count tables with one host sync (fixed
 *                   1024-word bitmaps per cell, counts below 65,536; a set with another count is
 *                   rebuilt with exact widths); default 1, 0 = the exact three-phase build
 *   "tables_nt"     0..2 the posterior-table rows as non-temporal stores: 0 never, 1 always, 2 when
 *                   the call's rows exceed 256 MB (default)
 *   "wpca_ms"       1/0  the multi-start npcs = 1 weighted-PCA kernel (default 1)
 * (Removed in round 6, each measured slower or equal and deleted with its kernels and branches:
 * fuse_groups, boot2_rows / k_boot2t, piece_taper, boot_chunks, ell_chunks, gene_waves /
 * gene3_cells, lane_prio, lane_thread, interleave, defer_boot, upload_staged, upload_threads,
 * pair_cells / gene_blocks (pair mode), gene_direct, rest_thread, tables_pair, task_cols,
 * ratio_window / ratio_block: fixed at their defaults.)
 * Statistics: "skip_slabs", "skip_stretches", "skip_kept", "skip_redo", "degen", "tiles_<i>"
 * (slabs the tile bootstrap -- gene blocks or list pass -- finished with i 16-point tiles),
 * "pair_redo" (slabs the gene blocks left to the four-tile list pass) (with skip_stats);
 * "boot_f64_fma" (FP64 lane FMAs the bootstrap kernels issued), also with skip_stats; "boot_path":
 * the bootstrap kernel of the last posterior (0 k_boot2, 1 k_boot_tiles / k_boot_gene, 3 the
 * general k_boot); "stream_syncs", "arena_syncs" (this context's and its peer's streams drained
 * by a buffer regrowth / a pinned arena wrap) and "buf_reallocs" (process-wide workspace
 * reallocations, each a hipFree): 0 in steady state; "ratio_n_max": the constant largest n
 * (grid points of one row) of scde_matSlideMult, scde_ratio_summary and scde_distribution_summary
 * (m = 2n - 1), whose kernel keeps a gene's rows in LDS ("ratio_n_lds64": the largest n that
 * needs no more than the 64 KiB a launch gets without opting in).  A larger n, a DE grid above it, or a
 * batch-corrected DE grid with 2 * ngrid - 1 above it, is refused with SCDE_EARG. */
/* Options can also come from the environment: SCDE_OPTIONS="name=value,..." is applied to every
 * context as it is created (an unknown name fails the creation). */
int scde_ctx_set_option(scde_ctx* ctx, const char* name, double value);
int scde_ctx_get_stat(scde_ctx* ctx, const char* name, double* value);
/* Test hook: make the next `count` failures happen at fault point `where` ("u16_slot": the second
 * slot of a 16-bit host-count upload fails as if its copy had) -- the error paths' recovery is
 * tested through it (tests/test_gpu_fullsize.py).  "handoff_spin" (count = shader clocks, 0 off):
 * every later call queues a one-wave spin kernel of that length on a stream after each of its
 * cross-stream waits (so the work it produces next starts late) and before each event another
 * stream or thread waits on (each piece's tables and unique sets, the pieces' uploads, the 16-bit
 * ring, the aux set-up, the peer lane's start and finish, the read-back thread's events): a
 * consumer that misses its wait reads unwritten data every time (tests/test_gpu_ordering.py; stat
 * "handoff_spins" counts them).  "skip_lane_join": the next `count` DE calls leave out the main
 * stream's wait for the peer lane -- the ordering tests' negative control.  Not for production
 * use. */
int scde_ctx_inject_fault(scde_ctx* ctx, const char* where, int count);
int scde_ctx_reset_stats(scde_ctx* ctx);

/* scde_logBootPosterior on a context of the caller's (its options, its workspace); NULL: the
 * library's own default context, as scde_logBootPosterior. */
int scde_logBootPosterior_ctx(scde_ctx* ctx, const double* models, int ncells, const int* ucl_vals,
                              const int64_t* ucl_off, const int* counti, int ngenes, const double* magnitudes,
                              int ngrid, int nboot, int seed, int return_post, int local_theta,
                              int square_logit_conc, int ensemble, double* jp, double* modes, double* post);

/* device buffers owned by the context's allocator */
int scde_dev_alloc(scde_ctx* ctx, int64_t bytes, void** dptr);
int scde_dev_free(scde_ctx* ctx, void* dptr);
int scde_h2d(scde_ctx* ctx, void* dst, const void* src, int64_t bytes);
int scde_d2h(scde_ctx* ctx, void* dst, const void* src, int64_t bytes);

/* The same BH cZ on device buffers (z_dev, cz_dev: n doubles in HBM), on the context's
 * stream: pnorm, stable descending radix sort, cummin scan, qnorm.  For the gathered Z
 * of a sharded call (R/functions.R:5051). */
int scde_bh_cz_dev(scde_ctx* ctx, const double* z_dev, int64_t n, double* cz_dev);

typedef struct scde_de_params {
  int ncells;              /* cells (columns of counts) */
  const double* models;    /* host, ncells x 12 col-major (NaN where absent; corr.a clamp applied inside) */
  int local_theta;         /* "corr.ltheta.b" present */
  int square_logit_conc;   /* "conc.a2" present */
  const int* groups;       /* host, per cell: 0 / 1 (level order), -1 = NA */
  const double* prior_x;   /* host, ngrid */
  const double* prior_y;   /* host, ngrid */
  int ngrid;
  int nboot;               /* n.randomizations */
  int n_cores;             /* reference seeding mode: chunk seeds as R's n.cores */
  int64_t gene_offset;     /* first global gene index of this shard */
  int64_t ngenes_total;    /* global number of genes (for chunk seeds) */
  double expectation;      /* R `expectation` (log2 scale) */
  int rand_kind;           /* SCDE_RAND_GLIBC / SCDE_RAND_DARWIN */
  int compute_cz;          /* 1: this call covers every gene; results gain a 6th column cZ (device BH) */
} scde_de_params;

/* scde.expression.difference (R/functions.R:304-407, no batch) on device-resident
 * counts (int32, column-major, leading dimension ld, rows gene_offset.. of the shard
 * start at counts_dev).  results: host ngenes x 5 col-major (lb, mle, ub, ce, Z), or
 * x 6 with cZ when p->compute_cz (whole call = all genes); for shards cZ is left to
 * scde_bh_cz / scde_bh_cz_dev over the gathered Z.  jp1/jp2 (ngenes x ngrid) and
 * ratio (ngenes x (2*ngrid-1)) are optional host outputs, col-major. */
int scde_expression_difference_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes,
                                   const scde_de_params* p, double* results, double* jp1, double* jp2,
                                   double* ratio);

/* Batch-corrected scde.expression.difference (R/functions.R:321-399) on device-resident
 * counts: p as for scde_expression_difference_dev (compute_cz is implied), batch_models
 * ncells x 12 col-major (NULL = p->models), batch_codes[ncells] in [0, nbatch) (level
 * order).  results: host, three consecutive ngenes x 6 col-major blocks (lb, mle, ub, ce,
 * Z, cZ) for batch.adjusted, results, batch.effect.  Optional host outputs, col-major:
 * jp1/jp2 (the groups' joint posteriors, ngenes x ngrid), ratio (the group difference posterior, ngenes x (2*ngrid-1)), adj_ratio (the
 * batch-adjusted posterior, ngenes x (4*ngrid-3)), batch_ratio (ngenes x (2*ngrid-1)). */
int scde_expression_difference_batch_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes,
                                         const scde_de_params* p, const double* batch_models,
                                         const int* batch_codes, int nbatch, double* results, double* jp1,
                                         double* jp2, double* ratio, double* adj_ratio, double* batch_ratio);

/* The same three calls on the caller's HOST count matrix, as the R shim makes them
 * (R/functions.R:304 scde.expression.difference, :566 scde.posteriors; the R glue hands
 * the count matrix to the native side once per call): counts int32 column-major with
 * leading dimension ld >= ngenes and p->ncells (scde_posteriors_host: ncells_total)
 * columns, staged into the context's device buffer on its stream, then the resident
 * pipeline above.  ctx may be NULL: the process-wide default context (device
 * $SCDE_DEVICE, created lazily on first use, i.e. after any fork). */
int scde_expression_difference_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes,
                                    const scde_de_params* p, double* results, double* jp1, double* jp2,
                                    double* ratio);
int scde_expression_difference_batch_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes,
                                          const scde_de_params* p, const double* batch_models,
                                          const int* batch_codes, int nbatch, double* results, double* jp1,
                                          double* jp2, double* ratio, double* adj_ratio, double* batch_ratio);
int scde_posteriors_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells_total,
                         const int* cellidx, int ncells_sel, const double* models_sel, int local_theta,
                         int square_logit_conc, const double* prior_x, int ngrid, int nboot, int n_cores,
                         int64_t gene_offset, int64_t ngenes_total, int return_post, int ensemble,
                         const int* batch_vals, const int64_t* batch_off, const int* composition, int nbatch,
                         double* jp, double* modes, double* post);

/* pagoda.varnorm's posterior-mode consumer (R/functions.R:1414-1507; SURVEY.md section 8(f)
 * row 4).  Runs scde.posteriors (n.cores seeding, nboot randomizations) over all cells and,
 * with a batch (batch_codes[ncells] in [0, nbatch), nbatch > 1), over each level's cells; the
 * modes are jp %*% as.numeric(colnames(jp)) (use_expected_value) or the magnitude of each row's
 * maximum.  Outputs (host): modes (1 [+ nbatch]) x ngenes (dataset-wide, then per level);
 * matw ngenes x ncells = 1 - mfp * sfp with mfp = scde.failure.probability at log(dataset
 * modes) and sfp = ppois(count - 1, exp(fail.r), lower.tail = FALSE) (1466-1474); bmatw (with
 * a batch) the same with each cell's level modes (1485-1506).  models: ncells x 12 col-major.
 * The Poisson tail sfp is good for every exp(fail.r) in (0, inf] and every count: it is a
 * series relative to the point mass at the count (in saddle-point form, never through
 * exp(-exp(fail.r))), run until it converges -- about 9 sqrt(max(count, exp(fail.r))) terms
 * where the two are close.  Against the regularised incomplete gamma function its relative
 * error is about 1e-13 for exp(fail.r) up to 1e6, growing to about 3e-12 at 1e8; fail.r above
 * 709.78 (exp overflows) gives sfp = 1 for every count. */
int scde_pagoda_varnorm_weights_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells,
                                    const double* models, int local_theta, int square_logit_conc,
                                    const double* prior_x, int ngrid, int nboot, int n_cores, const int* batch_codes,
                                    int nbatch, int use_expected_value, double* modes, double* matw, double* bmatw);
int scde_pagoda_varnorm_weights_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells,
                                     const double* models, int local_theta, int square_logit_conc,
                                     const double* prior_x, int ngrid, int nboot, int n_cores,
                                     const int* batch_codes, int nbatch, int use_expected_value, double* modes,
                                     double* matw, double* bmatw);

/* The weights call above also leaves its modes, matw and bmatw in device memory owned by the
 * context, for the two stages below; its host outputs matw / bmatw may then be NULL (modes is
 * always returned).  The context keeps one such set: the next weights call, or a _host entry
 * below, replaces it.
 *
 * pagoda.varnorm, second stage (R/functions.R:1511-1619): per gene g and cell i, at lfpm =
 * log(avmodes[g]): mu = exp(lfpm corr.a_i + corr.b_i); theta = get.corr.theta (4039-4056: the
 * five-parameter local form with local_theta, else corr.theta; clamped to [theta_lo, theta_hi],
 * NaN -> theta_lo); e = (matw[g, i] edf(theta))^weight_df_power; dev = e (count - mu)^2 /
 * (mu + mu^2 / theta + exp(fail.r_i)).  edf(theta) = exp(S(log theta)), S the natural cubic
 * spline (linear beyond its ends) of the uniform table: edf_table holds edf_n values at
 * edf_lt0 + k edf_h, then their edf_n second derivatives (host memory; edf_n >= 2); edf = 1
 * where theta > 1e3.  A gene with avmodes = 0 is evaluated by IEEE rules, like any other.
 * out (host), 3 x ngenes: edf = sum e + 1; wvar = sum dev / sum e; rowSums(matw).  With a batch
 * (batch_codes[ncells] in [0, nbatch), nbatch > 1), 7 x ngenes: then bedf = sum be + 1 with be
 * = (bmatw edf(theta_b))^power at the cell's level modes; bwvar = sum e (count - mu_b)^2 /
 * (mu_b + mu_b^2 / theta_b + exp(fail.r)) / sum be (the dataset-wide e, as line 1601 reads);
 * rowSums(bmatw); bwvar / wvar.
 * modes_dev ((1 + nbatch) x ngenes: dataset-wide, then per level), matw_dev, bmatw_dev (ngenes
 * x ncells column-major, a gene contiguous): device memory, or all three NULL for what the last
 * weights call on ctx left (an error when its shape differs).  models: ncells x 12 col-major,
 * host.  Sums run in a fixed order: the same input gives the same bits. */
int scde_pagoda_varnorm_moments_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells,
                                    const double* models, int local_theta, const double* modes_dev,
                                    const double* matw_dev, const double* bmatw_dev, const int* batch_codes,
                                    int nbatch, const double* edf_table, int edf_n, double edf_lt0, double edf_h,
                                    double theta_lo, double theta_hi, double weight_df_power, double* out);
/* The same on host counts, modes and weights (ctx may be NULL: the default context). */
int scde_pagoda_varnorm_moments_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells,
                                     const double* models, int local_theta, const double* modes, const double* matw,
                                     const double* bmatw, const int* batch_codes, int nbatch, const double* edf_table,
                                     int edf_n, double edf_lt0, double edf_h, double theta_lo, double theta_hi,
                                     double weight_df_power, double* out);

/* pagoda.varnorm, last stage (R/functions.R:1725-1804): w = 1 - weight_k (1 - matw) divided by
 * its row sum; x = log10(exp((log(count) - corr.b_i) / corr.a_i) + 1); ov = weightedMatVar(x, w)
 * (5062-5093, centred, weight-normalised); vr = arv / ov, 0 where ov <= 0; mat = (x - sum x w /
 * sum w) sqrt(vr).  With a batch (matw_dev is then bmatw) first, per level: the count of x > 0,
 * wsu(k, n, qnorm(1 - 1e-2)) (1720-1723), their minimum nbub, the level's weights scaled by
 * pmin(1, ceiling(nbub n_level) / k_level), x minus the level's rowMeans(x w nr) (nr = ncells /
 * sum w) plus the dataset mean rowMeans(x w) nr (1740-1772); the centring uses the scaled
 * weights.  arv: host, ngenes (NaN for a gene outside the fit: its mat row is NaN).  mat,
 * matw_out: host, ngenes x ncells column-major.  matw_dev: device, or NULL for what the last
 * weights call left (bmatw with a batch).  A batch level without cells is an error. */
int scde_pagoda_varnorm_matrix_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells,
                                   const double* models, const double* matw_dev, const int* batch_codes, int nbatch,
                                   double weight_k, const double* arv, double* mat, double* matw_out);
int scde_pagoda_varnorm_matrix_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells,
                                    const double* models, const double* matw, const int* batch_codes, int nbatch,
                                    double weight_k, const double* arv, double* mat, double* matw_out);

/* pagoda.subtract.aspect (R/functions.R:1850-1862) on ngenes x ncells column-major matrices (a
 * gene contiguous): v = the aspect (host, ncells) minus its mean, scaled to unit length; nr =
 * (mat * matw) v / (matw v^2); out = mat - nr v', then (center) minus rowSums(out * matw) /
 * rowSums(matw).  _dev: mat, matw and out in device memory (out may not overlap them). */
int scde_pagoda_subtract_aspect_dev(scde_ctx* ctx, const double* mat_dev, const double* matw_dev, int ngenes,
                                    int ncells, const double* aspect, int center, double* out_dev);
int scde_pagoda_subtract_aspect_host(scde_ctx* ctx, const double* mat, const double* matw, int ngenes, int ncells,
                                     const double* aspect, int center, double* out);

/* scde.expression.prior (R/functions.R:225-254; replaces the R-level function, which has
 * no .Call) on device-resident counts (ngenes x ncells int32, column stride ld).  models:
 * ncells x 12 col-major (conc.b, conc.a, ..., corr.b, corr.a, ..., conc.a2 at column 11 when
 * square_logit_conc).  max_value NULL = quantile(x[x < Inf], max_quantile) of the
 * log10(FPM + 1) magnitudes (type 7).  Outputs (host, length_out + 1 each): x, y, lp,
 * grid_weight (lp / grid_weight may be NULL); max_value_out (nullable) receives the
 * max.value used.  length_out in [1, 2047]. */
int scde_expression_prior_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells,
                              const double* models, int square_logit_conc, int length_out, double pseudo_count,
                              double bw, double max_quantile, const double* max_value, double* x, double* y,
                              double* lp, double* grid_weight, double* max_value_out);

/* scde.posteriors (R/functions.R:566-669) on device-resident counts for the cells
 * listed in cellidx (host, ncells_sel entries).  Outputs are host, col-major.
 * batch_* may be NULL (no batch).  return_post: R postflag (0..3). */
int scde_posteriors_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, const int* cellidx,
                        int ncells_sel, const double* models_sel, int local_theta, int square_logit_conc,
                        const double* prior_x, int ngrid, int nboot, int n_cores, int64_t gene_offset,
                        int64_t ngenes_total, int return_post, int ensemble, const int* batch_vals,
                        const int64_t* batch_off, const int* composition, int nbatch, double* jp, double* modes,
                        double* post);

/* ---------------------------------------------------------------- weighted PCA
 * Bailey's EM weighted PCA behind bwpca() / pagoda.pathway.wPCA() (BASELINE config 5;
 * SURVEY.md section 8(f) row 3).
 *
 * .Call("baileyWPCA", Mat, Matw, Npcs, Nstarts, Smooth, EMtol, EMmaxiter, Seed, Nshuffles)
 * (src/bwpca.cpp:59-182; declared src/bwpca.h:8) on host buffers.  mat, matw: n (cells)
 * x d (genes) col-major.  The reference's random inputs are arguments, produced by the
 * caller exactly as the reference draws them (the .Call shim in INTEGRATION.md):
 *   starts: (1 + nshuffles) x nstarts x (d x K) uniforms, K = min(npcs, d), in draw order
 *           (arma::randu<arma::mat>(d, npcs) per start = R's unif_rand() stream;
 *           src/bwpca.cpp:197-198; Seed is a no-op there);
 *   perms:  nshuffles x d x n row indices (set_random_matrices' std::random_shuffle over
 *           rand(); src/bwpca.cpp:41-57), see scde_shuffle_perms.
 * Outputs: rotation d x K, scores n x K, scoreweights n x K (nullable), var K, totvar,
 * randvar nshuffles (src/bwpca.cpp:164-180).  npcs <= 8. */
int scde_baileyWPCA(const double* mat, const double* matw, int n, int d, int npcs, int nstarts, int smooth,
                    double em_tol, int em_maxiter, const double* starts, int nshuffles, const int* perms,
                    double* rotation, double* scores, double* scoreweights, double* var, double* totvar,
                    double* randvar);

/* A batch of baileyWPCA problems on one device-resident matrix pair: M_dev / W_dev are
 * ncells x mcols col-major (column stride ld), i.e. pagoda's t(varinfo$mat) / t(matw).
 * Problem p: d[p] columns cols[col_off[p] ..], npcs[p] (K = min(npcs, d) <= 8), nstarts[p]
 * starts from starts[start_off[p] ..] (nstarts x d x K uniforms), rows permuted per column
 * by perms[perm_off[p] ..] (d x ncells) when perm_off (nullable) is >= 0.  Outputs (host),
 * concatenated in problem order: rotation d x K, scores / scoreweights / colmeans ncells x K
 * (colmeans[j, k] = mean_g M[j, g] |rotation[g, k]|, pagoda's orientation statistic;
 * scoreweights / colmeans nullable), stats K + 2 per problem (var[K], totvar, the residual
 * of component 1 alone), iterations (nullable) per (problem, start). */
int scde_bwpca_batch_dev(scde_ctx* ctx, const double* M_dev, const double* W_dev, int64_t ld, int ncells,
                         int64_t mcols, int nprob, const int* d, const int* npcs, const int* nstarts,
                         const int64_t* col_off, const int* cols, int64_t ncols, const int64_t* perm_off,
                         const int* perms, int64_t nperms, const int64_t* start_off, const double* starts,
                         int64_t nstart_vals, int smooth, double em_tol, int em_maxiter, double* rotation,
                         double* scores, double* scoreweights, double* colmeans, double* stats, int* iterations);

/* R's RNG (src/main/RNG.c), host side, for the mirror of the R glue: set.seed(seed) into
 * a 625-word Mersenne-Twister state (word 0 = mti), unif_rand() draws, and R >= 3.6
 * sample.int(n, k) without replacement (1-based, rejection sampling). */
int scde_r_set_seed(uint32_t seed, uint32_t* state);
int scde_r_unif_rand(uint32_t* state, int64_t n, double* out);
int scde_r_sample(uint32_t* state, int n, int k, int* out);
/* set_random_matrices' permutations (src/bwpca.cpp:41-57) after srand(seed) with the
 * platform rand() (scde_set_rand_kind): nshuffles x d x n. */
int scde_shuffle_perms(unsigned int seed, int nshuffles, int d, int n, int* perms);

/* ---------------------------------------------------------------- PAGODA helpers
 * The remaining .Call symbols of the package (src/pagoda.cpp; declared src/pagoda.h:5-8),
 * SURVEY.md section 8(f) row 4.  Host buffers, R column-major. */

/* .Call("winsorizeMatrix", Mat, Trim) (src/pagoda.cpp:6-31): per row, the round(ncol * trim)
 * smallest values become the next smallest, the largest the next largest.  ncol <= 8192,
 * or round(ncol * trim) <= 32. */
int scde_winsorizeMatrix(const double* mat, int nrow, int ncol, double trim, double* out);

/* .Call("matWCorr", Mat, Matw) (src/pagoda.cpp:41-65): weighted correlation of columns i < j
 * with weights sqrt(w_i w_j) / sum; out ncol x ncol: 1 on the diagonal, c(j, i) below it,
 * 0 above (as the reference fills it). */
int scde_matWCorr(const double* mat, const double* matw, int nrow, int ncol, double* out);

/* .Call("matCorr", X, Y) = arma::cor(x, y) (src/pagoda.cpp:33-38): x nrow x nx, y nrow x ny,
 * out nx x ny. */
int scde_matCorr(const double* x, int nrow, int nx, const double* y, int ny, double* out);

/* .Call("plSemicompleteCor2", Pl) (src/pagoda.cpp:67-117): np sparse vectors (list element p
 * = gene indices idx[off[p] .. off[p+1]) increasing, values val[...]); r = correlation over
 * the shared genes (np x np, 1 on the diagonal), n = union sizes (np x np, 0 on it). */
int scde_plSemicompleteCor2(int np, const int64_t* off, const int* idx, const double* val, double* r, int* n);

/* ---------------------------------------------------------------- cell-to-cell distance measures
 * The vignette's "Adjusted distance measures" (vignettes/diffexp.md:231-301).  Each entry writes
 * the weighted correlation of every pair of cells, out: ncells x ncells col-major, host, both
 * triangles filled (the distance is 1 - out):
 *   corr(x, y, w) = (Sxy/s - m1 m2) / sqrt((Sxx/s - m1^2) (Syy/s - m2^2)),  s = sum w,
 *   m1 = sum(x w)/s, m2 = sum(y w)/s, Sxy = sum(x y w), Sxx = sum(x^2 w), Syy =
 *   sum(y^2 w) (boot::corr); a pair with zero weight sum or zero weighted variance is NaN.
 * _dev entries take device-resident data (int32 counts, leading dimension ld), _host entries
 * host data they stage themselves; ctx may be NULL (the default context).  models: ncells x 12
 * col-major as everywhere.  SCDE_EARG: null pointers, ncells < 1, k outside [0, 1], nsim < 1. */

/* Weights that factor per cell, w_g(i, j) = u[g, i] u[g, j]; x, u: ngenes x ncells col-major. */
int scde_wcorr_sep_dev(scde_ctx* ctx, const double* x_dev, const double* u_dev, int64_t ld, int ngenes, int ncells,
                       double* out);
int scde_wcorr_sep_host(scde_ctx* ctx, const double* x, const double* u, int64_t ld, int ngenes, int ncells,
                        double* out);

/* Reciprocal weighting (vignette 268-278): x = log10(counts + 1),
 * w = sqrt((1 - f(model_i, fpm[g, j])) (1 - f(model_j, fpm[g, i]))) k + (1 - k), f =
 * scde.failure.probability, fpm = scde.expression.magnitude. */
int scde_reciprocal_corr_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells,
                             const double* models, int square_logit_conc, double k, double* out);
int scde_reciprocal_corr_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells,
                              const double* models, int square_logit_conc, double k, double* out);

/* Mode-relative weighting (vignette 285-300).  modes: ngenes x ncells posterior modes
 * (natural-log magnitudes, host; -inf allowed); jp_modes: per gene, the joint posterior's mode
 * as log(10^prior_x - 1) (host).  x = log10(exp(modes) + 1),
 * w = (matw_i matw_j)^(1/4), matw = 1 - sqrt(p.self.fail sqrt(p.self.fail p.mode.fail)). */
int scde_mode_fail_corr_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells,
                            const double* models, int square_logit_conc, const double* modes,
                            const double* jp_modes, double* out);
int scde_mode_fail_corr_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells,
                             const double* models, int square_logit_conc, const double* modes,
                             const double* jp_modes, double* out);

/* Direct drop-out (vignette 241-258): the mean over nsim rounds of the pairwise-complete
 * Pearson correlation of log10(counts + 1) with entry (g, c) kept with probability
 * q = 1 - p.self.fail[g, c] k.  From a uniform u01: q == 0 drops, q == 1 keeps, q <= 0.5 keeps
 * iff u01 >= 1 - q, q > 0.5 keeps iff u01 < q.  uniforms: host, nsim x ncells x ngenes (round
 * s, cell c, gene g at (s ncells + c) ngenes + g), or NULL for the library's counter-based
 * generator: key_s = mix64(seed + 0x9E3779B97F4A7C15 (s + 1)),
 * u01 = (mix64(key_s ^ mix64(g + ngenes c + 1)) >> 11) 2^-53, mix64 the splitmix64 finalizer. */
int scde_direct_corr_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells,
                         const double* models, int square_logit_conc, double k, int nsim, const double* uniforms,
                         uint64_t seed, double* out);
int scde_direct_corr_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells, const double* models,
                          int square_logit_conc, double k, int nsim, const double* uniforms, uint64_t seed,
                          double* out);

/* ---------------------------------------------------------------- hierarchical clustering
 * R's stats::hclust for the monotone linkages, and what cutree needs, on the device
 * (csrc/hclust.hip: one workgroup per problem, the whole merge loop in one launch).
 *
 * Input.  n >= 2 objects; d: n x n doubles, column-major, leading dimension ld >= n.  Only the
 * strict lower triangle is read (d(i, j) at d[i + j * ld], i > j) -- what as.dist reads; the
 * diagonal and the upper triangle are never read (scde_matWCorr fills only the lower triangle).
 * Every value read must be finite: otherwise SCDE_EARG, the message naming the first offending
 * pair in column-major order (stats::hclust refuses NA/NaN/Inf).  n < 2 is SCDE_EARG.  The
 * caller's matrix is never written.
 *
 * method: 0 ward.D, 1 ward.D2, 2 single, 3 complete, 4 average, 5 mcquitty; any other code is
 * SCDE_EARG (centroid and median are not monotone and are not offered).
 *
 * One step.  Among the active clusters the pair to merge is the lexicographic minimum of
 * (d(i, j), i, j), i < j; values are compared numerically (-0.0 ties with 0.0).  For these
 * linkages that is the pair stats::hclust's nearest-neighbour list picks, ties included (read
 * from its algorithm, not checked against a run of R).  The merged cluster keeps slot i, slot j
 * dies, size[i] += size[j].  Every other active k is updated in float64, each expression
 * evaluated left to right as written, no fused multiply-add (ni, nj, nk the sizes as doubles,
 * h = d(i, j)):
 *   ward.D, ward.D2   ((ni + nk) * dik + (nj + nk) * djk - nk * h) / (ni + nj + nk)
 *   single            min(dik, djk)
 *   complete          max(dik, djk)
 *   average           (ni * dik + nj * djk) / (ni + nj)
 *   mcquitty          (dik + djk) / 2
 * ward.D2 squares every input value once on the way in (d * d) and reports sqrt(h), the square
 * root taken in host code.
 *
 * Outputs (host), in R's encoding.
 *   merge   (n - 1) x 2 ints, column-major.  Negative: a singleton, -(1-based index); positive:
 *           the 1-based step that made the cluster.  Within a row a singleton comes before a
 *           cluster, two singletons in increasing index, two clusters in increasing step.
 *   height  n - 1 doubles.
 *   order   n ints, 1-based: the leaves left to right from expanding the last step
 *           recursively, column 1 as the left child.
 * cutree: k clusters are the state after n - k steps; a height h gives
 * k = n - #{height <= h} (non-monotone heights are an error); labels are 1-based, clusters
 * numbered by the first observation they contain.
 *
 * SCDE_EHIP with an "out of memory" message, before any launch, when the workspace (n^2 + O(n)
 * doubles per problem) cannot be allocated.  ctx may be NULL (the default context). */
int scde_hclust_host(scde_ctx* ctx, const double* d, int64_t ld, int n, int method, int* merge, double* height,
                     int* order);
/* d_dev is resident in HBM and is left unmodified; results go to the host. */
int scde_hclust_dev(scde_ctx* ctx, const double* d_dev, int64_t ld, int n, int method, int* merge, double* height,
                    int* order);
/* nprob problems packed in one device buffer: problem p is n[p] x n[p] at element off[p],
 * ld = n[p].  One launch, one workgroup per problem.  Outputs packed in problem order: merge of
 * problem p at 2 * sum_{q<p}(n[q] - 1), height at sum_{q<p}(n[q] - 1), order at sum_{q<p} n[q].
 * A non-finite value in any problem is SCDE_EARG naming the (0-based) problem. */
int scde_hclust_batch_dev(scde_ctx* ctx, int nprob, const double* d_dev, const int64_t* off, const int* n,
                          int method, int* merge, double* height, int* order);

/* ---------------------------------------------------------------- stats::dist
 * R's dist(x, method) between the rows of x (csrc/rdist.hip), so that hclust(dist(x)) needs no
 * host step.  Stated from R's documentation and from how its C loop reads; not checked against
 * a run of R.
 *
 * Input.  x: n x p doubles, column-major (R's layout), ld >= n, n >= 1, p >= 0.  method:
 * 0 euclidean, 1 manhattan, 2 maximum; any other code is SCDE_EARG.
 *
 * One pair (i, j), i != j.  The columns are walked in increasing order.  With
 * d = x(i, k) - x(j, k), column k takes part when d is not NaN: a NaN in either value and
 * Inf - Inf drop out.  count is the number of columns that took part.  All float64, each
 * operation rounded on its own (no fused multiply-add), the sum evaluated left to right from 0:
 *   euclidean   s += d * d;  count == 0: NaN;  count != p: s = s / ((double)count / p);  sqrt(s)
 *   manhattan   s += |d|;    count == 0: NaN;  count != p: s = s / ((double)count / p);  s
 *   maximum     the largest |d|;  count == 0: NaN;  no scaling
 * The result equals that evaluation bit for bit, whatever the tiling: a pair's sum has one
 * order, and (a - b)^2 == (b - a)^2 exactly, so out(i, j) and out(j, i) hold the same bits.
 *
 * Output.  n x n doubles, column-major, ld = n, both triangles, the diagonal exactly 0: what
 * scde_hclust_* takes.  A NaN distance (no common column) is written as it is; hclust then
 * refuses the matrix.  No atomics: results repeat bit for bit, and the two entries agree bit for
 * bit.  ctx may be NULL. */
int scde_dist_host(scde_ctx* ctx, const double* x, int64_t ld, int n, int p, int method, double* out);
/* x_dev and out_dev are resident in HBM (out_dev: n * n doubles, not overlapping x_dev). */
int scde_dist_dev(scde_ctx* ctx, const double* x_dev, int64_t ld, int n, int p, int method, double* out_dev);

/* ---------------------------------------------------------------- optimal leaf ordering
 * cba::order.optimal(dist, merge), the step of pagoda.cluster.cells after hclust
 * (R/functions.R:2668-2672): among the 2^(n-1) orientations of the tree, the one whose
 * left-to-right leaf order has the smallest summed distance between neighbours (Bar-Joseph,
 * Gifford and Jaakkola 2001), on the device (csrc/olo.hip: min-plus products level by level, the
 * choice walked top-down by one workgroup).
 *
 * Input.  n >= 2 objects; d: n x n doubles, column-major, ld >= n.  Only the strict lower
 * triangle is read, and every value read must be finite: otherwise SCDE_EARG naming the first
 * offending pair in column-major order.  merge: (n - 1) x 2 ints, column-major, R's encoding
 * (negative: an observation; positive: an earlier step).  Row s defines node s with left child L
 * (column 1) and right child R (column 2).  A merge matrix that is no tree over all n
 * observations -- an observation missing or used twice, a step used before it exists, used twice
 * or referring to itself -- is SCDE_EARG naming the row.  The merge matrix (and a host d) are
 * checked on the host before anything is allocated.  The caller's matrices are never written.
 *
 * The table.  p(x): the position of observation x in the input tree's own left-to-right leaf
 * order (recomputed from merge; hclust's order for an hclust result).  M(x, x) = 0, and for a
 * node v with children L, R and every u in L, w in R
 *   M(u, w) = M(w, u) = min over m in far(L, u), k in far(R, w) of
 *                       fl( fl( M(u, m) + d(m, k) ) + M(k, w) )
 * with far(c, x) = {x} for a leaf c, otherwise the leaves of the child of c that does not
 * contain x.  The association is always the L term first, then d, then the R term, whatever
 * orientation is chosen in the end; float64, no contraction; min is numeric (-0.0 ties with
 * 0.0).  Rounded addition is monotone, so the two-step form
 *   T(u, k) = min_m fl( M(u, m) + d(m, k) ),   M(u, w) = min_k fl( T(u, k) + M(k, w) )
 * and any tiling or reduction order give the same bits.
 *
 * The choice, top-down.  The root is never flipped (the reversal of the whole order is not
 * looked at).  Its end points are the lexicographic minimum of (M(u, w), p(u), p(w)), u in
 * L_root, w in R_root.  At a node v whose end points are a in L and b in R -- whichever of the
 * two is the left one -- the joint (m, k) is the lexicographic minimum of
 * (fl( fl( M(a, m) + d(m, k) ) + M(k, b) ), p(m), p(k)) over m in far(L, a), k in far(R, b),
 * always evaluated in this forward form; its cost equals M(a, b) bit for bit.  L continues with
 * the end points (a, m), R with (k, b); v is flipped when its left-most end point lies in R.
 *
 * Outputs (host).
 *   merge_out  merge with the two columns of every flipped row swapped and nothing else changed
 *              (cba's convention; hclust's singleton-first rule no longer holds for such a row)
 *   order_out  n ints, 1-based: the leaves of merge_out left to right
 *   length     (may be NULL) d summed along order_out, left to right, in float64
 * n = 2 returns the input.  merge_out and order_out may not alias merge or each other
 * (SCDE_EARG).
 *
 * Which of several equally short orders cba itself returns is unknown: the tie rule above is
 * this library's own, and nothing here was checked against a run of R or cba.
 *
 * SCDE_EHIP with an "out of memory" message, before any launch, when the workspace (3 n^2 + O(n)
 * doubles: M, T and d in leaf order) cannot be allocated; it is freed before the call returns.
 * Statistics "olo_launches" and "olo_candidates" (one float64 add and one min each) describe
 * the context's last call.  ctx may be NULL. */
int scde_order_optimal_host(scde_ctx* ctx, const double* d, int64_t ld, int n, const int* merge, int* merge_out,
                            int* order_out, double* length);
/* d_dev is resident in HBM and is left unmodified (its values are checked by a kernel); merge is
 * a host array; results go to the host. */
int scde_order_optimal_dev(scde_ctx* ctx, const double* d_dev, int64_t ld, int n, const int* merge, int* merge_out,
                           int* order_out, double* length);

/* 1 - cor(x) of the columns of a resident nrow x ncol column-major matrix (the correlation of
 * scde_matCorr), written to the resident ncol x ncol matrix out_dev, both triangles, the
 * diagonal exactly 0 (as.matrix(as.dist(.))): pagoda.gene.clusters' gene-to-gene distance, ready
 * for scde_hclust_dev. */
int scde_cor_distance_dev(scde_ctx* ctx, const double* x_dev, int nrow, int ncol, double* out_dev);

/* ---------------------------------------------------------------- exact t-SNE of a distance matrix
 * The 2-D embedding the PAGODA walkthrough draws from pagoda.cluster.cells' distance
 * (vignettes/pagoda.md:230-250: Rtsne(cell.clustering$distance, is_distance = TRUE,
 * perplexity = 10)); csrc/tsne.hip.  This is van der Maaten's exact t-SNE, the method that
 * Rtsne(theta = 0) wraps, written from the published algorithm (van der Maaten and Hinton 2008;
 * the gradient in bhtsne's form).  The vignette's call uses Rtsne's default Barnes-Hut
 * approximation (theta = 0.5), of which this is the exact limit; Barnes-Hut is not built.
 * Nothing here was checked against a run of Rtsne: Rtsne is not available to this project.
 *
 * Input.  d: n x n doubles, column-major, leading dimension ld >= n.  Only the strict lower
 * triangle is read (as scde_hclust_* read it; scde_matWCorr's half-filled matrix is accepted as
 * is): delta_ij = d[max(i, j) + min(i, j) ld].  D2_ij = delta_ij^2, or delta_ij itself with
 * squared != 0.  Whether Rtsne squares a precomputed distance in its exact mode is not known
 * here.  A NaN, an infinity or a negative value in the strict lower triangle (also a value whose
 * square overflows) is SCDE_EARG, the message naming the first such pair in column-major order,
 * before any iteration.  n >= 4, perplexity >= 1 and 3 perplexity <= n - 1 (Rtsne's rule), else
 * SCDE_EARG.
 *
 * Affinities, for every row i over j != i.  beta = 1, lo = -inf, hi = +inf; up to 200 evaluations
 *   p_j = exp(-beta D2_ij),  s = sum_j p_j + DBL_MIN,  H = beta (sum_j D2_ij p_j) / s + log s,
 *   delta = H - log(perplexity)
 * stopping when |delta| < 1e-5; otherwise, delta > 0: lo = beta, beta = 2 beta while hi is
 * infinite, else (beta + hi) / 2; delta <= 0: hi = beta, beta = beta / 2 while lo is infinite,
 * else (beta + lo) / 2.  The row keeps p_{j|i} = p_j / s of the last beta it evaluated, and that
 * beta is reported; p_{i|i} = 0.  Then P_ij = (p_{j|i} + p_{i|j}) / (2 n), the paper's form: P
 * is symmetric bit for bit, its diagonal is 0 and it sums to 1 without a global sum.
 *
 * Iteration t = 0 .. max_iter - 1 on the state Y, uY (zeros at t = 0), gains (ones at t = 0),
 * each n x 2.  ex = exaggeration while t <= stop_lying_iter and 1 after it (P itself is never
 * scaled); mom = momentum while t <= mom_switch_iter, final_momentum after it.  With
 * Q_ij = 1 / (1 + |Y_i - Y_j|^2), for every i over j != i
 *   A_i = sum_j ex P_ij Q_ij (Y_i - Y_j),  R_i = sum_j Q_ij^2 (Y_i - Y_j),  S_i = sum_j Q_ij,
 *   sumQ = sum_i S_i,  dY_i = A_i - R_i / sumQ
 * (bhtsne's (P - Q / sumQ) Q form, split so that one pass over P serves an iteration; no factor
 * 4, as in bhtsne).  Per coordinate, with sign(0) = 0:
 *   gain = gain + 0.2 if sign(dY) != sign(uY), else gain * 0.8;  gain = max(gain, 0.01);
 *   uY = mom uY - eta gain dY;  Y = Y + uY
 * and then each column of Y has its mean (column sum / n) subtracted.  Rtsne's defaults:
 * perplexity 30, max_iter 1000, eta 200, exaggeration 12, stop_lying_iter 250,
 * mom_switch_iter 250, momentum 0.5, final_momentum 0.8.
 *
 * Cost.  costs[i] = sum_{j != i} P_ij log((P_ij + FLT_MIN) / (Q_ij / sumQ + FLT_MIN)),
 * FLT_MIN = 2^-126; the sum of costs is the Kullback-Leibler divergence.
 *
 * Initial Y.  The caller's n x 2 matrix, or Y0[i, c] = 1e-4 z[2 i + c] with z the first 2 n
 * values of scde_r_norm_rand after scde_r_set_seed(seed) (R's rnorm after set.seed).  Rtsne's own
 * generator is not known here: the seeded start is this library's choice.
 *
 * Layout.  Y, uY, gains and Y_init are n x 2 row-major (a point's two coordinates adjacent);
 * resident ones must be 16-byte aligned.  P is n x n, both triangles.  beta and costs are host
 * arrays of n.
 *
 * Determinism.  No floating-point atomics; every sum is taken in an order that depends on n
 * alone (Q's reciprocal is the hardware estimate refined by one Newton step).  Results repeat bit
 * for bit from run to run, the host and device entries agree bit for bit, and a run split at any
 * iteration and resumed from (Y, uY, gains, iter0) equals the unsplit run bit for bit.
 *
 * ctx may be NULL.  The device entries take a workspace of scde_tsne_ws_bytes(n) bytes (resident,
 * 8-byte aligned; O(n^2 / 64 + n) doubles); a missing, smaller or misaligned one is SCDE_EARG.  Argument errors leave P and
 * the state untouched; a refused distance leaves the contents of P_dev undefined. */
int scde_tsne_ws_bytes(int n, int64_t* bytes);
/* d_dev resident (left unmodified), P_dev resident n x n (must not overlap d_dev), beta host. */
int scde_tsne_affinities_dev(scde_ctx* ctx, const double* d_dev, int64_t ld, int n, double perplexity, int squared,
                             double* P_dev, double* beta, void* ws_dev, int64_t ws_bytes);
/* Iterations iter0 .. iter0 + niter - 1 on the resident state, in place; niter = 0 does nothing. */
int scde_tsne_iterate_dev(scde_ctx* ctx, const double* P_dev, int n, double eta, double exaggeration,
                          int stop_lying_iter, int mom_switch_iter, double momentum, double final_momentum,
                          int iter0, int niter, double* Y_dev, double* uY_dev, double* gains_dev, void* ws_dev,
                          int64_t ws_bytes);
int scde_tsne_cost_dev(scde_ctx* ctx, const double* P_dev, int n, const double* Y_dev, double* costs, void* ws_dev,
                       int64_t ws_bytes);
/* Upload, affinities, max_iter iterations and the cost in one call, everything on the host side:
 * Y_init may be NULL (the seeded start) and may be Y; P (n x n, may be NULL) receives the
 * affinities.  max_iter = 0 returns the initial Y and its cost.  SCDE_EHIP with an "out of memory"
 * message, before any launch, when the 2 n^2 doubles and the workspace cannot be allocated; they
 * are freed before the call returns. */
int scde_tsne_host(scde_ctx* ctx, const double* d, int64_t ld, int n, double perplexity, int squared, double eta,
                   double exaggeration, int stop_lying_iter, int mom_switch_iter, double momentum,
                   double final_momentum, int max_iter, uint32_t seed, const double* Y_init, double* Y, double* costs,
                   double* beta, double* P);

/* ---------------------------------------------------------------- pagoda.gene.clusters' random rounds
 * The null model of pagoda.gene.clusters (R/functions.R:2131-2192): per round i, set.seed(i), a
 * genes x cells matrix of rnorm, winsorize, drop the genes that fail the keep rule, 1 - cor,
 * hclust, cutree, and per cluster the PC1 variance.  The pieces below work on a round matrix
 * resident in HBM as ncells x ngenes column-major (a gene's cells contiguous), the layout
 * scde_cor_distance_dev takes; scde_amd/cluster.py chains them.  ctx may be NULL. */

/* R's rnorm stream (RNGkind "Mersenne-Twister", "Inversion"), host side, on scde_r_set_seed's
 * state, which is advanced in place.  scde_r_norm_rand: n values of norm_rand(), i.e.
 *   u = unif_rand(); u = (int)(134217728 * u) + unif_rand(); qnorm(u / 134217728)
 * (two uniforms per normal).  scde_r_mt_words: the n raw tempered 32-bit outputs that the next n
 * unif_rand() calls would scale (MT_genrand before its * 2.3283064365386963e-10). */
int scde_r_norm_rand(uint32_t* state, int64_t n, double* out);
int scde_r_mt_words(uint32_t* state, int64_t n, uint32_t* out);
/* matrix(rnorm(ngenes * ncells), nrow = ngenes) from 2 * ngenes * ncells raw words (host): draw t
 * uses words 2 t and 2 t + 1 and is gene t % ngenes, cell t / ngenes; out_dev[g * ncells + c].
 * The scaling, unif_rand's fix-up of 0 and 1, the 2^27 combination and qnorm (AS241) run on
 * the device in the host's arithmetic; only qnorm's log and sqrt may round differently. */
int scde_rnorm_matrix_dev(scde_ctx* ctx, const uint32_t* words, int ngenes, int ncells, double* out_dev);

/* winsorize.matrix per gene on a resident matrix: bit-equal to scde_winsorizeMatrix of the
 * genes x cells matrix.  ncells <= 8192, or round(ncells * trim) <= 32, else SCDE_EARG; out_dev
 * must not be x_dev. */
int scde_winsorize_dev(scde_ctx* ctx, const double* x_dev, int ncells, int ngenes, double trim, double* out_dev);
/* The random rounds' keep rule which(abs(sum(diff(abs(x)))) > 0) (R/functions.R:2146; not the
 * observed half's sum(abs(diff(x)))): per gene the differences |x[k + 1]| - |x[k]|, each rounded
 * to double, are summed in cell order in double-double (R's long-double sum); keep[g] (host,
 * ngenes ints) is 1 iff the rounded sum is not zero.  ncells < 2 is SCDE_EARG (an empty diff
 * drops every gene). */
int scde_keep_absdiff_dev(scde_ctx* ctx, const double* x_dev, int ncells, int ngenes, int* keep);
/* out_dev column j = x_dev column cols[j] (nrow rows; x_dev has ncol columns; cols: host, nsel
 * entries in [0, ncol)); the buffers must not overlap. */
int scde_gather_cols_dev(scde_ctx* ctx, const double* x_dev, int nrow, int64_t ncol, const int* cols, int nsel,
                         double* out_dev);

/* Squared largest singular value, batched (csrc/sigma1.hip).  x_dev: ncells x ngenes resident
 * matrix; problem p is the block M of its columns idx[off[p] .. off[p + 1]) (host lists, any
 * order, at least one column); out[p] (host) = sigma_1(M)^2.  pagoda.gene.clusters' value
 * pcaMethods::sDev(pca(m[, ii], nPcs = 1, center = FALSE))^2 is out[p] / max(1, ncells - 1).
 * One launch, one workgroup per problem: the Gram matrix of the smaller side on the FP64 matrix
 * cores, Householder tridiagonalisation, Sturm bisection of the largest eigenvalue down to
 * adjacent doubles.  The result is bit-repeatable and depends on the problem alone (no atomics;
 * not on the launch, nor on the other problems); it is exactly 0 for an all-zero block, the sum
 * of squares for one column, NaN when the block holds a non-finite value.  Column indices are
 * checked on the host (SCDE_EARG naming the problem) and again on the device before any is used.
 * SCDE_EHIP "out of memory", before the launch, when the workspace (sum over problems of
 * min(columns, ncells)^2 + O(min) doubles) cannot be allocated. */
int scde_sigma1sq_batch_dev(scde_ctx* ctx, const double* x_dev, int ncells, int64_t ngenes, int nprob,
                            const int64_t* off, const int* idx, double* out);

/* ---------------------------------------------------------------- aspect redundancy reduction
 * The numerical pieces of pagoda.reduce.loading.redundancy (R/functions.R:2490-2526) and
 * pagoda.reduce.redundancy (2559-2610) with their helpers pathway.pc.correlation.distance
 * (5126-5164) and collapse.aspect.clusters (5166-5198); csrc/aspects.hip, chained by
 * scde_amd/aspects.py.  m aspects.  Square matrices are m x m column-major and resident in HBM;
 * the patterns x (tam$xv) and their weights w (tam$xvw) are resident as ncells x m column-major
 * (an aspect's cells contiguous), the layout scde_cor_distance_dev takes.  ctx may be NULL.
 * Argument errors are SCDE_EARG with a message naming the offending item. */

/* scde_plSemicompleteCor2 on host lists, leaving r (m x m doubles) and n (m x m ints) in HBM. */
int scde_plSemicompleteCor2_dev(scde_ctx* ctx, int np, const int64_t* off, const int* idx, const double* val,
                                double* r_dev, int* n_dev);

/* The Student-t renormalisation of loading correlations to target_ndf degrees of freedom
 * (R/functions.R:5146-5157).  For a pair with correlation r and union size n, nu = n - 2:
 *   tv = r sqrt(nu / (1 - r^2)),  z = pt(tv, nu, lower = F, log = T),
 *   nr = qt(z, target_ndf - 2, lower = F, log = T),  cr = nr / sqrt(target_ndf - 2 + nr^2).
 * In correlation space p = I_{1 - r^2}(nu / 2, 1/2) / 2 and |cr| solves
 * I_{1 - cr^2}((target_ndf - 2) / 2, 1/2) / 2 = p, sign(cr) = sign(r): an odd map, evaluated in
 * log space (the smaller of the tail p and the central mass 1/2 - p is matched as a logarithm),
 * so tails far below 1e-308 stay finite.  cr = r exactly when n <= 2, |r| >= 1 or r is NaN;
 * r = 0 gives 0; n = target_ndf gives r to rounding.  One deviation from R: R's double evaluation
 * loses the negative side once exp(log p) underflows and falls back to r there; the odd map is
 * used everywhere.
 * Only the pairs above the diagonal (r[i + j m], n[i + j m], i < j) are read and transformed, one
 * lane per pair, the result written to both triangles of cr; cr's diagonal is r's.  FP64, no
 * fast-math.  target_ndf must be finite and above 2; m >= 1.  cr_dev must not be r_dev. */
int scde_t_renorm_dev(scde_ctx* ctx, const double* r_dev, const int* n_dev, int m, double target_ndf,
                      double* cr_dev);
/* The same on host matrices (staged; SCDE_EHIP "out of memory" before any launch). */
int scde_t_renorm_host(scde_ctx* ctx, const double* r, const int* n, int m, double target_ndf, double* cr);

/* The distance between aspects from their patterns.  c = the Pearson correlation of the m columns
 * of x_dev: each column centred and scaled to unit length (two passes), then their Gram matrix
 * on the FP64 matrix cores; NaN for a column that holds a single value (cor() gives NA).
 *   cr_dev given (m x m, from scde_t_renorm_dev or r itself):
 *     pclc = max(0, 1 - |cr|);  cda = |c| (abs) or max(c, 0);  d1 = 1 - cda;
 *     out = (1 - sqrt((1 - pclc) * (1 - d1)))^corr_power          (R/functions.R:2491-2499)
 *   cr_dev NULL:  out = 1 - |c| (abs) or 1 - c                     (R/functions.R:2571-2575)
 * each expression in float64 as written.  Both triangles are written, the diagonal exactly 0.
 * SCDE_EHIP "out of memory", before any launch, when the scaled copy of the patterns (ncells x m
 * doubles) cannot be allocated. */
int scde_aspect_distance_dev(scde_ctx* ctx, const double* x_dev, int ncells, int m, const double* cr_dev, int abs,
                             double corr_power, double* out_dev);

/* 1 - c or 1 - |c| (abs) of c = scde_matWCorr of the patterns with their weights
 * (R/functions.R:2562-2568), both triangles, the diagonal exactly 0. */
int scde_matWCorr_distance_dev(scde_ctx* ctx, const double* x_dev, const double* w_dev, int ncells, int m, int abs,
                               double* out_dev);

/* collapse.aspect.clusters.  Cluster p is the rows idx[off[p] .. off[p + 1]) (host lists, at
 * least one row each) of x_dev / w_dev; column p of d_dev / dw_dev (ncells x nclust, resident)
 * receives its pattern and weights.  One launch, one workgroup per cluster.
 *   weights   colSums(w[rows, ] * sd(row)) / their sum (sd = sqrt of R's var, denominator
 *             ncells - 1), for every cluster
 *   pattern   one row: that row.  pick_top: the row of largest variance (first maximum).
 *             Otherwise, with X the rows transposed and each column centred (ncells x k): v1 its
 *             unit top right singular vector, xv = X v1; a = the per-cell mean over the rows of
 *             (uncentred row) * |v1_i|; xv is negated when cor(xv, a) < 0; with scale,
 *             xv = xv * sqrt(max row var) / sqrt(var(xv)).  v1 comes from the Gram matrix of the
 *             smaller side (k or ncells) on the FP64 matrix cores, Householder
 *             tridiagonalisation, Sturm bisection of the largest eigenvalue, inverse iteration
 *             on the tridiagonal matrix and the back-transformation; when ncells < k the
 *             cell-side eigenvector times sigma_1 is xv.
 * Per cluster, to the host: top[p] = the row of largest variance (first maximum; the row itself
 * for one row); fallback[p] = 1 when sum|diff(xv)| == 0, or sum|xv| == 0 after scaling -- the
 * caller replaces the pattern by |rnorm(ncells, sd = 1e-6)| -- else 0; orientation[p] =
 * cor(xv, a) after the flip (>= 0), NaN for one row, pick_top and fallback clusters.  A non-finite
 * orientation of a cluster that is not a fallback is where R stops.
 * No atomics: results are bit-repeatable and depend on the cluster alone.  Row indices are
 * checked on the host (SCDE_EARG naming the cluster) and again on the device before any is used.
 * ncells >= 2.  SCDE_EHIP "out of memory", before the launch, when the workspace (sum over
 * clusters of min(rows, ncells)^2 + O(rows + ncells) doubles) cannot be allocated. */
int scde_collapse_aspects_dev(scde_ctx* ctx, const double* x_dev, const double* w_dev, int ncells, int m, int nclust,
                              const int64_t* off, const int* idx, int scale, int pick_top, double* d_dev,
                              double* dw_dev, int* top, int* fallback, double* orientation);

/* ---------------------------------------------------------------- pagoda.top.aspects
 * The matrix step of pagoda.top.aspects (R/functions.R:2434-2452; csrc/top_aspects.hip, driven by
 * scde_amd/top_aspects.py; everything before it is host statistics).  x and w are the rows of
 * t(scores) and t(scoreweights) of the m valid aspects, m x ncells row-major (an aspect's cells
 * contiguous); num holds one factor per aspect (host, m values): sqrt(qchisq(.) / n.cells), or
 * the score with use.oe.scale.  Per row r, in float64 as written:
 *   mean = sum(x[r, ]) / ncells;  var = sum((x[r, ] - mean)^2) / (ncells - 1)   (two passes)
 *   xv[r, c]  = (x[r, c] - mean) * (num[r] / sqrt(var))
 *   xvw[r, c] = w[r, c] / sum(w[r, ])
 * A constant row gives NaN (0 * Inf) in xv, a row of one cell NaN (0 / 0); nothing is clamped.
 * One launch, one workgroup per row; the sums are added in an order fixed by ncells alone (no
 * atomics), so results are bit-repeatable and the two entries agree bit for bit.  m >= 0,
 * ncells >= 1; the four matrices must not overlap.  ctx may be NULL. */
/* x_dev, w_dev, xv_dev, xvw_dev resident (m x ncells doubles each). */
int scde_top_aspects_dev(scde_ctx* ctx, const double* x_dev, const double* w_dev, const double* num, int m, int ncells,
                         double* xv_dev, double* xvw_dev);
/* The same on host matrices (staged; SCDE_EHIP "out of memory" before any launch). */
int scde_top_aspects(scde_ctx* ctx, const double* x, const double* w, const double* num, int m, int ncells, double* xv,
                     double* xvw);

/* ---------------------------------------------------------------- knn.error.models, neighbourhood stage
 * What knn.error.models computes before its mixture fit (R/functions.R:1180-1226; csrc/knn.hip,
 * driven by scde_amd/knn.py; the fit itself follows below, scde_knn_fit_*).  counts is int32,
 * ngenes x ncells column-major with leading dimension ld; thr is min.count.threshold and an entry
 * is valid when counts[g, j] >= thr.  Counts are not negative (not checked here: a negative
 * valid count, possible with thr <= 0, gives sqrt's NaN in the similarity and a negative value
 * in fpm, as R's arithmetic does).  At most 8192 cells: more is SCDE_EARG.  ctx may be NULL.
 *
 * Similarity: scde_wcorr_sep of x = sqrt(counts) where valid, 0 elsewhere, and u = valid (both
 * formed on the device): the pairwise-complete Pearson correlation of the cells, in the one-pass
 * form written there.  out is ncells x ncells (host), NaN where a pair is degenerate.  The matrix
 * also stays resident in the context for scde_knn_neighbours. */
int scde_knn_similarity_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells, int thr,
                            double* out);
int scde_knn_similarity_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells, int thr,
                             double* out);
/* Neighbours.  sim is a host ncells x ncells column-major matrix, or NULL for the similarity the
 * last scde_knn_similarity_* call on this context left resident (it must have ncells cells).
 * groups (host, ncells codes, NULL: one group) limits cell i's candidates to the other cells of
 * its group.  Candidate j comes before candidate l when sim[i, j] > sim[i, l], or they are equal
 * (-0 equals +0) and j < l, or sim[i, l] is NaN and sim[i, j] is not, or both are NaN and j < l:
 * R's order(decreasing = TRUE).  Row i of out (host, ncells x kmax row-major, int32, 0-based)
 * receives the first min(k, group size - 1) candidates, then -1; kmax must be at least the
 * largest of these counts.  Positions are found by counting, so the result is exact and the
 * same every run.  The lists also stay resident for scde_knn_magnitudes_*. */
int scde_knn_neighbours(scde_ctx* ctx, const double* sim, int ncells, const int* groups, int k, int kmax, int* out);
/* Expected magnitudes.  nb is a host ncells x kmax row-major list with entries in [-1, ncells)
 * (-1: none), or NULL for the lists the last scde_knn_neighbours call left resident (the same
 * ncells and kmax); ls holds ncells finite library sizes (host), each at least 0 and, when
 * thr <= 0, above 0 (a valid count over a library size of 0 is Inf, as in R).  For gene g and cell i,
 * with S = { counts[g, j] / ls[j] : j in nb[i, ], counts[g, j] >= thr } and n = |S|:
 *   n = 0         fpm[g, i] = NaN
 *   trim >= 0.5   the median of S (the mean of the two middle values when n is even)
 *   otherwise     lo = floor(n * trim) + 1 (the product in double), hi = n + 1 - lo, and
 *                 fpm[g, i] = the mean of the lo-th to hi-th smallest values of S
 * nabove[g, i] = the number of j in nb[i, ] with counts[g, j] > thr (strictly).  fpm (double)
 * and nabove (int32) are host ngenes x ncells column-major.  trim >= 0.  Equal values are ordered
 * by cell index, every sum is taken in an order fixed by the neighbour list alone and there are
 * no floating-point atomics: results are bit-repeatable and the two entries agree bit for bit.
 * A row of nb that lists a cell twice is SCDE_EARG. */
int scde_knn_magnitudes_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells, const int* nb,
                            int kmax, const double* ls, int thr, double trim, double* fpm, int* nabove);
int scde_knn_magnitudes_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells, const int* nb,
                             int kmax, const double* ls, int thr, double trim, double* fpm, int* nabove);

/* ---------------------------------------------------------------- Spearman rank correlation
 * (csrc/spearman.hip, driven by scde_amd/spearman.py and scde_amd/cluster.py)
 *
 * Rank transform.  x is nrow x ncol column-major (a column contiguous); every column of out
 * receives R's rank(column, ties.method = "average", na.last = "keep"): a value's rank is the
 * number of smaller values of its column plus (the number equal to it, itself included, + 1) / 2.
 * Values are FP64; -0.0 and 0.0 tie; a NaN stays the NaN it is and the other values are ranked
 * among the non-NaN ones; +-Inf are ordinary values.  Every rank is a multiple of 0.5 and exact.
 * out may be x (in place).  Columns of up to 8192 rows are sorted in LDS, one workgroup per
 * column; longer ones are ranked by counting, O(nrow^2) per column (in place, that path takes a
 * second nrow x ncol matrix of device memory).  No atomics: results are the same every run and
 * the two entries agree bit for bit.  nrow, ncol >= 1.  ctx may be NULL. */
int scde_rank_cols_dev(scde_ctx* ctx, const double* x_dev, int nrow, int ncol, double* out_dev);
int scde_rank_cols_host(scde_ctx* ctx, const double* x, int nrow, int ncol, double* out);
/* Pairwise-complete Spearman similarity of cells: what knn.error.models(cor.method = "spearman")
 * computes (R/functions.R:1184-1196), stats::cor(method = "spearman", use = "pairwise.complete.obs")
 * of sqrt(counts) with the entries below thr set to NA.  Arguments, layout and limits are those of
 * scde_knn_similarity_*: counts int32, ngenes x ncells column-major with leading dimension ld,
 * valid where counts[g, c] >= thr; out is ncells x ncells (host); at most 8192 cells; and at most
 * 1,300,000 genes, which keeps every sum below exact in int64.  The host entry refuses a negative
 * count (SCDE_EARG); in resident counts a negative entry is never valid.  ctx may be NULL.
 *
 * For cells i and j (i = j included), with S = { g : counts[g, i] >= thr and counts[g, j] >= thr }
 * and m = |S| (sqrt is monotone, so the counts are ranked):
 *   a_g = 2 #{h in S : c_hi < c_gi} + #{h in S : c_hi = c_gi} + 1     twice g's average rank in cell i
 *   b_g = the same in cell j
 *   sum a = sum b = m (m + 1), so with M = m (m + 1)^2
 *   Sab = sum a_g b_g - M,  Saa = sum a_g^2 - M,  Sbb = sum b_g^2 - M   exact int64 integers
 *   out[i, j] = (double)Sab / sqrt((double)Saa * (double)Sbb), clamped to [-1, 1]
 * three correctly rounded operations on exact integers (no fused multiply-add), so the result does
 * not depend on any order of summation.  NaN when m = 0, Saa = 0 or Sbb = 0 (m = 1; a cell whose
 * common genes all tie).  The diagonal goes through the same formula: 1.0, or NaN for a cell with
 * no valid gene or a single valid value.  The matrix is symmetric bit for bit.  R sums the same
 * ranks in long double in two passes; the two agree to rounding, not bit for bit.
 *
 * lds_values: a pair whose two rank tables (one entry per distinct valid value of either cell)
 * have more entries than this keeps them in a global workspace instead of LDS; 0 is the kernel's
 * maximum (36864).  Both paths give the same bits; a small value is the test hook for the
 * workspace path.  The matrix also stays resident in the context for scde_knn_neighbours
 * (sim = NULL), as scde_knn_similarity_* leave theirs. */
int scde_spearman_similarity_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells, int thr,
                                 int lds_values, double* out);
int scde_spearman_similarity_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells, int thr,
                                  int lds_values, double* out);

/* ---------------------------------------------------------------- knn.error.models, mixture fit
 * One two-component EM per cell (fit.nb2gth.mixture.model and get.compressed.v1.model,
 * R/functions.R:3653-3660, 4058-4187, 3422-3434; csrc/knn_fit.hip; the contract, step by step, is
 * DESIGN.md section 4.15).  fpm and fail_prior are host ngenes x ncells column-major, as
 * scde_amd/knn.py's knn_model_inputs gives them: a gene is valid in a cell where fail_prior is not
 * NaN, and fail_prior is then the starting posterior of the failed component (both NULL: what the
 * last scde_crossfit_inputs_* call on this context left resident, of the same ngenes and ncells).
 * Per cell, with y = the valid genes' counts, x = their fpm, l = log x, and posteriors
 * (p1, p2 = 1 - p1), up to max_iter rounds of
 *   concomitant  beta maximising sum p2 log s(eta) + (1 - p2) log(1 - s(eta)), eta = b0 + b1 l + b2 l^2,
 *                s the logistic function: Newton from 0, a step halved while it lowers the objective;
 *                no convergence within 50 steps (separable data) fails the cell
 *   slope        a = sum p2 y / sum p2 x, mu = a x
 *   theta        the root in [theta_lo, theta_hi] of MASS::theta.md's moment equation with weights
 *                p2, or the bound on the side the sign indicates
 *   curve        (local_theta) b, t, m, s, r minimising sum p2 alpha^alpha_weight_power
 *                (log alpha - f(l))^2, f(l) = b + (t - b) / (1 + 10^((m - l) s))^r,
 *                alpha = (y / mu - 1)^2 - 1 / mu clamped to [1 / theta_hi, 1 / theta_lo], in R's box,
 *                by the project's projected Levenberg-Marquardt from R's start
 *   E-step       log p1 ~ log(1 - s(eta)) + dpois(y, 0.1), log p2 ~ log s(eta) + dnbinom(y, size =
 *                theta or exp(-f(l)) clamped to the range, mu); llh = sum of the log-sum-exps
 * until |llh - llh_old| / (|llh| + 0.1) < 1e-6.  Row c of models (host, ncells x 12 column-major,
 * the columns conc.b, conc.a, fail.r, corr.b, corr.a, corr.theta, corr.ltheta.{b,t,m,s,r}, conc.a2)
 * holds b0, b1, log 0.1, log a, 1, theta, the curve (NaN without local_theta), b2 of the last
 * M-step.  iterations[c] is the number of rounds, llh[c] the last log-likelihood, status[c] 0, or
 * 1 (fewer than 3 valid genes), 2 (sum p2 x = 0), 3 (a parameter or the likelihood is not
 * finite): the row and llh are then NaN.  clusters (int32, 1 / 2, 0 outside the valid genes and
 * in a failed cell) and post (the failed component's posterior, NaN likewise) are host ngenes x
 * ncells column-major from the last E-step, or NULL.  lds_genes: a cell with at most this many
 * valid genes keeps its per-gene vectors in LDS, a larger one in an HBM workspace (0: the default,
 * 2048; at most 3376; the results are the same bits either way).  One launch, one workgroup per
 * cell; every sum is taken in an order fixed by the cell's valid-gene count alone and there are
 * no floating-point atomics: results are bit-repeatable, the same whichever cells share the call,
 * and the two entries agree bit for bit.  0 < theta_lo < theta_hi, max_iter >= 1, at most 8192
 * cells.  ctx may be NULL. */
int scde_knn_fit_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells, const double* fpm,
                     const double* fail_prior, int local_theta, double theta_lo, double theta_hi,
                     double alpha_weight_power, int max_iter, int lds_genes, double* models, int* iterations,
                     double* llh, int* status, int* clusters, double* post);
int scde_knn_fit_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells, const double* fpm,
                      const double* fail_prior, int local_theta, double theta_lo, double theta_hi,
                      double alpha_weight_power, int max_iter, int lds_genes, double* models, int* iterations,
                      double* llh, int* status, int* clusters, double* post);

/* ---------------------------------------------------------------- scde.error.models, input stage
 * What scde.error.models computes before its mixture fit when threshold.segmentation = TRUE
 * (calculate.crossfit.models' threshold rule and the head of calculate.individual.models,
 * R/functions.R:3030-3039, 3253-3303; csrc/error_models.hip, driven by scde_amd/error_models.py;
 * DESIGN.md section 4.16).  counts as above; thr = min.count.threshold >= 1.  groups holds ncells
 * codes (host; NULL: one group); every group has at least two cells.  Cell i's cross-fit partners
 * are part[part_off[i] .. part_off[i + 1]) (host, 0-based cells of i's group, not i, none twice;
 * the pair list seen from both of its cells).  A cell is "paired" when it has a partner.  ls holds
 * ncells positive finite library sizes.  For gene g and cell i of a group of n cells:
 *   nabove[g, i]      the number of paired cells j != i of the group with counts[g, j] >= thr
 *   valid             nabove[g, i] >= min(n - 1, min_nonfailed)
 *   fpm[g, i]         (sum over the group's cells before i, in cell order, of counts[g, j] / ls[j]
 *                     + the sum over the cells after i, taken from the last one down) / (n - 1):
 *                     positive terms only, never a total minus the cell's own term; NaN when not valid
 *   fail_prior[g, i]  over the partners j with counts[g, i] + counts[g, j] > 0: h of them have
 *                     counts[g, i] < thr <= counts[g, j], k have not;
 *                     exp((h log(t) + k log(1 - t)) / (h + k)) with t = 1 - 1e-6 and 1 - t as the
 *                     doubles they are (R's threshold.prior), 1 - 1e-10 when h + k = 0; NaN when
 *                     not valid
 * fpm, fail_prior (double) and nabove (int32) are host ngenes x ncells column-major; each may be
 * NULL and is then not copied back.  fpm and fail_prior also stay resident in the context: a
 * following scde_knn_fit_* or scde_nb2_fit_* call on it with the same dimensions may pass NULL for
 * both.  No floating-point atomics and no order left to chance: results are bit-repeatable and
 * the two entries agree bit for bit.  At most 8192 cells.  ctx may be NULL. */
int scde_crossfit_inputs_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells,
                             const int* groups, const double* ls, const int* part_off, const int* part, int thr,
                             int min_nonfailed, double* fpm, double* fail_prior, int* nabove);
int scde_crossfit_inputs_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells,
                              const int* groups, const double* ls, const int* part_off, const int* part, int thr,
                              int min_nonfailed, double* fpm, double* fail_prior, int* nabove);

/* ---------------------------------------------------------------- scde.error.models, mixture fit (linear.fit = FALSE)
 * One two-component EM per cell (fit.nb2.mixture.model: FLXMRnb2glm's fit, glm.nb.fit,
 * custom.glm.fit and MASS::theta.ml, R/functions.R:3630-3651, 4002-4010, 4434-4547, 4549-4820;
 * csrc/nb2_fit.hip; the contract, step by step, is DESIGN.md section 4.16).  fpm and fail_prior as
 * scde_knn_fit_* takes them, or both NULL for what the last scde_crossfit_inputs_* call on this
 * context left resident (the same ngenes and ncells).  Per cell, with y = the valid genes' counts,
 * l = log fpm and posteriors (p1 = fail_prior, p2 = 1 - p1), up to max_iter rounds of
 *   concomitant  (b0, b1) maximising sum p2 log s(eta) + (1 - p2) log(1 - s(eta)), eta = b0 + b1 l:
 *                scde_knn_fit_*'s Newton on two parameters
 *   NB component w = p2, divided by 1e6 where y <= 1; genes of weight 0 take no part.  glm.nb.fit with
 *                the design [1, l] and the log link (mu = max(exp(eta), 2^-52)):
 *                  IRLS      from a per-gene eta: W = w mu^2 / V(mu), z = eta + (y - mu) / mu, the 2 x 2
 *                            weighted normal equations by Cholesky; the step halved (at most maxit times)
 *                            while the deviance is not finite or, from the second iteration on, rises by
 *                            more than 3e-8 (0.1 + |dev|); until |dev - devold| / (0.1 + |dev|) < 1e-8,
 *                            at most maxit iterations
 *                  first     Poisson IRLS from eta = log(y + 0.1), maxit 20
 *                  theta.ml  t = sum w / sum w (y / mu - 1)^2, then at most 19 Newton steps t = |t|,
 *                            t += score / info (digamma, trigamma) until |step| <= 2^-13; |t|,
 *                            clamped to [0.5, Inf)
 *                  rounds    at most 20, while |Lm0 - Lm| / d1 + |theta0 - theta| > 1e-8 (d1 =
 *                            sqrt(2 max(1, genes of positive weight - 2)), Lm the NB log-likelihood,
 *                            Lm0 = Lm + 2 d1 at first): theta.ml at the current mu, then the
 *                            negative.binomial(theta0) IRLS from the current eta, maxit 200
 *                a slope c1 < 0 is replaced by (c0, c1) = (mean(y w) / sum w, 0): R's rule, the
 *                intercept is then a mean where a log mean belongs
 *   E-step       log p1 ~ log(1 - s(eta)) + dpois(y, background_rate), log p2 ~ log s(eta) +
 *                dnbinom(y, size = theta, mu = max(exp(c0 + c1 l), 2^-52)); llh = sum of the log-sum-exps
 * until |llh - llh_old| / (|llh| + 0.1) < 1e-6.  If theta then is exactly 0.5 ("underfit"), glm.nb.fit
 * runs once more with weight 1 on the genes with p2 > p1 and 0 elsewhere, its first IRLS
 * negative.binomial(0.5) from eta = log(y + (y == 0) / 6), theta clamped to [0, 1e5], and replaces
 * (c0, c1, theta).  Row c of models (ncells x 12 column-major, columns as scde_knn_fit_*) holds b0,
 * b1, log background_rate, c0, c1, theta and six NaN.  iterations, llh, status, clusters, post and
 * lds_genes as scde_knn_fit_*; status may also be 2 (no gene of positive weight) and 5 (an IRLS
 * system is singular or not finite, or a halving ran out).  The same guarantees: one launch, one
 * workgroup per cell, every sum in an order fixed by the cell's valid-gene count and its genes of
 * weight 0, no floating-point atomics; results are bit-repeatable, the same whichever cells share
 * the call, and the two entries agree bit for bit.  background_rate > 0, max_iter >= 1, at most
 * 8192 cells.  ctx may be NULL. */
int scde_nb2_fit_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells, const double* fpm,
                     const double* fail_prior, double background_rate, int max_iter, int lds_genes, double* models,
                     int* iterations, double* llh, int* status, int* clusters, double* post);
int scde_nb2_fit_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells, const double* fpm,
                      const double* fail_prior, double background_rate, int max_iter, int lds_genes, double* models,
                      int* iterations, double* llh, int* status, int* clusters, double* post);

/* ---------------------------------------------------------------- scde.error.models, the mixture cross-fit of pairs
 * threshold.segmentation = FALSE: one three-component EM per pair of cells (calculate.crossfit.models'
 * flexmix call, R/functions.R:2993-3028; csrc/crossfit_fit.hip; the contract, step by step and with
 * what could not be checked against flexmix, is DESIGN.md section 4.19).  pairs holds the first
 * cells pairs[0 .. npairs) and the second cells pairs[npairs .. 2 npairs) (host, two different cells
 * each).  Per pair (i, j), c1 = counts[, i], c2 = counts[, j], thr = min.count.threshold:
 *   rows         the genes with c1 + c2 > 0, in gene order; none: status 1
 *   start        the posterior (c1 <= thr, c1 > thr and c2 > thr, c2 <= thr) as 0 / 1, divided by its
 *                sum: (1/2, 0, 1/2) where both counts are <= thr
 * then up to max_iter rounds of
 *   shares       the mean over the rows of each component's posterior, as the round finds them; one
 *                below min_prior ends the pair with status 6 (component lost)
 *   concomitant  x = (log(c1 + 1) + log(c2 + 1)) / 2, pi = softmax(0, a2 + b2 x, a3 + b3 x); (a2, b2,
 *                a3, b3) maximising sum_i sum_k p_ik log pi_ik by Newton from 0 with a 4 x 4 unpivoted
 *                Cholesky, scde_knn_fit_*'s step halving and stopping rule; status 3 when a pivot is
 *                not positive, a halving runs out or 50 steps do not meet the rule (separable data)
 *   drivers      A: y = c1 on l = log(c2 + 1); B: y = c2 on l = log(c1 + 1); each scde_nb2_fit_*'s "NB
 *                component" with w = p2 (divided by 1e6 where y <= 1), theta clamped to [0, 1e3], the
 *                negative-slope rule, no underfit refit; status 2, 3 or 5 as there
 *   E-step       a1 = log pi1 + dpois(c1, zero_lambda), a2 = log pi2 + dnbinom(c1; theta_A, mu_A) +
 *                dnbinom(c2; theta_B, mu_B), a3 = log pi3 + dpois(c2, zero_lambda), all logs, mu =
 *                max(exp(c0 + c1 l), 2^-52); posteriors softmax(a), llh = sum of the log-sum-exps
 *                (not finite: status 3)
 * until |llh - llh_old| / (|llh| + 0.1) < 1e-6.  Outputs (host; each may be NULL and is then not
 * copied back): status, iterations (int32) and llh of npairs; params npairs x 10 column-major (a2,
 * b2, a3, b3, then c0, c1, theta of A and of B; NaN for a failed pair, as llh); clusters int8,
 * npairs blocks of ngenes: 1 / 2 / 3 the arg-max of the final posterior (the lowest index on a
 * tie), 0 outside the pair's rows and throughout a failed pair; posterior, npairs blocks of 2 x
 * ngenes: the final posterior of component 1, then of component 3, NaN where clusters is 0.
 * clusters and posterior stay resident in the context for scde_crossfit_reduce_*.  One launch, one
 * workgroup per pair; a pair with at most lds_rows rows (0: 2048; at most 2383) keeps its vectors
 * in LDS, a larger one in HBM, with the same bits; every sum in an order fixed by the pair's row
 * count and its rows of weight 0, no floating-point atomics; results are bit-repeatable, the same
 * whichever pairs share the call, and the two entries agree bit for bit.  thr >= 0, 0 <= min_prior
 * < 1, zero_lambda > 0, max_iter >= 1, at most 8192 cells.  ctx may be NULL. */
int scde_crossfit_fit_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells, const int* pairs,
                          int npairs, int thr, double min_prior, double zero_lambda, int max_iter, int lds_rows,
                          int* status, int* iterations, double* llh, double* params, int8_t* clusters,
                          double* posterior);
int scde_crossfit_fit_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells, const int* pairs,
                           int npairs, int thr, double min_prior, double zero_lambda, int max_iter, int lds_rows,
                           int* status, int* iterations, double* llh, double* params, int8_t* clusters,
                           double* posterior);

/* ---------------------------------------------------------------- scde.error.models, from pair results to the fit's inputs
 * scde_crossfit_inputs_* for any pairs' clusters and posteriors (R/functions.R:3147-3155, 3253-3303;
 * csrc/error_models.hip).  pairs, status, clusters and posterior as
 * scde_crossfit_fit_* takes and writes them (clusters holds codes 0 to 3); status, clusters and
 * posterior all NULL: what the last scde_crossfit_fit_* call on this context left resident, which
 * must have been given the same pairs and ngenes.  A pair's cells belong to one group and no pair
 * is listed twice; pairs with a status other than 0 take no part; a cell that has pairs, all of
 * them failed, is an error.  For gene g and cell c of a group of n cells:
 *   vil[g, c]         c has a status-0 pair, and in every such pair g has cluster 2 or 3 where c is the
 *                     pair's first cell, 1 or 2 where it is the second (never 0)
 *   nabove[g, c]      the number of cells j != c of the group with vil[g, j]
 *   valid, fpm        as scde_crossfit_inputs_*
 *   fail_prior[g, c]  exp(mean(log q)) over c's status-0 pairs in which g is a row (q is not NaN), q
 *                     the posterior of component 1 where c is the first cell and of component 3 where
 *                     it is the second, the logs summed in the pairs' order; 1 - 1e-10 when there is
 *                     no such pair; NaN when not valid
 * (a row may carry cluster 0 with a posterior: the threshold rule's code for two low counts)
 * vil (uint8), fpm, fail_prior (double) and nabove (int32) are host ngenes x ncells column-major;
 * each may be NULL.  With ls NULL only vil is computed (the library sizes R derives from it are
 * the host's work) and fpm, fail_prior and nabove must be NULL; with ls, fpm and fail_prior stay
 * resident for scde_knn_fit_* / scde_nb2_fit_* as after scde_crossfit_inputs_*.  Bit-repeatable;
 * the two entries agree bit for bit.  ctx may be NULL. */
int scde_crossfit_reduce_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, int ncells,
                             const int* groups, const double* ls, const int* pairs, int npairs, const int* status,
                             const int8_t* clusters, const double* posterior, int min_nonfailed, uint8_t* vil,
                             double* fpm, double* fail_prior, int* nabove);
int scde_crossfit_reduce_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells,
                              const int* groups, const double* ls, const int* pairs, int npairs, const int* status,
                              const int8_t* clusters, const double* posterior, int min_nonfailed, uint8_t* vil,
                              double* fpm, double* fail_prior, int* nabove);

/* Free and total bytes of the context's device (hipMemGetInfo). */
int scde_dev_mem_info(scde_ctx* ctx, int64_t* free_bytes, int64_t* total_bytes);

#ifdef __cplusplus
}
#endif
#endif /* SCDE_HIP_H */
