// kernels.h -- argument blocks and launchers of the kernel files (internal): the DE path's stages
// kernels.hip (the remainder of the one-file source: tables and default bootstrap, still to be
// split), unique.hip, boot.hip and ratio.hip, then the feature files.
#pragma once

#ifndef SCDE_BOOT_WPE
#define SCDE_BOOT_WPE 8  // k_boot2 (NB <= 20) occupancy target: 8 waves per SIMD = 64 VGPRs
#endif
#ifndef SCDE_BOOT_ASMLD
#define SCDE_BOOT_ASMLD 1  // k_boot2 column look-ahead issued from asm with explicit vmcnt waits
#endif
#ifndef SCDE_TAB_WPE
#define SCDE_TAB_WPE 4  // k_tables_cell occupancy target (waves per SIMD)
#endif
#ifndef SCDE_BOOT_EB
#define SCDE_BOOT_EB 4  // ELL entries per k_boot2 batch (rows are padded to a multiple of 8, plus 8)
#endif
#ifndef SCDE_BOOT_DIAG
#define SCDE_BOOT_DIAG 0  // bit switches that remove parts of k_boot2 for timing studies
#endif
#ifndef SCDE_RATIO_WPE
#define SCDE_RATIO_WPE 1  // k_ratio_summary occupancy target (waves per SIMD; 1 = compiler's choice)
#endif
#ifndef SCDE_RATIO_DIAG
#define SCDE_RATIO_DIAG 0  // timing-only builds: 1 skips the slide, 2 the summary (results wrong)
#endif
#ifndef SCDE_WPCA_BLOCK
#define SCDE_WPCA_BLOCK 512  // wpca.hip workgroup size (8 waves)
#endif
#include <hip/hip_runtime.h>

#include <cstdint>

namespace scde {

// k_col_consts record per column: [n or -1, n - x, stirlerr sum, 0.5 lf, log(size/(size+x)),
// log X - log n, log(n - X) - log n, dpois_log(x, failure rate), log po, log(1 - po)] with
// po = size / (size + x) (the count's own grid point), padded to 10 doubles
constexpr int kColc = 11;
// columns per task of the cell-staged tables kernels (k_tables_lpc: one lane per column)
#ifndef SCDE_TAB_TASK_COLS
#define SCDE_TAB_TASK_COLS 64
#endif
constexpr int kTabTaskCols = SCDE_TAB_TASK_COLS;
constexpr int kStretchSlots = 8;  // per-column stretch bounds: ceil(G / 64) <= 7 used

inline int div_up(long long a, long long b) { return (int)((a + b - 1) / b); }

struct TablesArgs {
  const int* ucl;            // flat unique counts, [ncols]
  const long long* ucl_off;  // [ncells + 1]
  long long ncols;
  int ncells;
  int G, GS;
  const double* mu;          // [ncells][GS]
  const double* lcfp;        // [ncells][GS]
  const double* lcfpr;       // [ncells][GS]
  const double* theta;       // [ncells][GS]
  const double* cellscal;    // [ncells][2] = {max log cfp, exp(fail.r)}
  double minlogprob;         // -DBL_MAX / ncells / 1.1
  // k_tables_lpc writes its rows (T, D) as non-temporal stores (the same bits)
  int nt_rows;
  // Rows (T, D): [0, G) values, pads up to the last 64-point stretch zero; k_tables_lpc leaves the
  // slots [ceil64(G), GS) unwritten (alignment only: no reader goes past the last 32-point tile or
  // 64-point stretch -- tests/test_gpu_table_edges.py test_stale_slots_between_calls)
  double* T;                 // [ncols][GS] log-posterior columns
  int* maxi;                 // [ncols] argmax (nullable)
  unsigned char* has_clamp;  // [ncols]
  int const_theta;           // theta is the same at every grid point (no local theta fit)
  const double* pq;          // [ncells][4][GS] p, q, log p, log q (const_theta), nullable
  const double* colc;        // [ncols][kColc] k_col_consts output (with pq), nullable
  const double* cfp = nullptr;  // [ncells][GS] exp(lcfp) from k_cell_prep (nullable: computed when staged)
  // Fused baseline-delta output (bootstrap path; the k_delta pass folded into the tables):
  //   phase 0: every column -> T (no D);
  //   phase 1: one wave per cell, its count-0 column -> D (and T if non-null); writes
  //            zcol[c] and base_col[c] (count-0 column when it has no clamp and use_baseline);
  //   phase 2: every other column -> D = T - T[base_col] (T itself where the cell has no
  //            baseline), pad lanes [G, GS) zeroed, column ncols all zero; T if non-null.
  int phase;
  int use_baseline;
  double* D;      // [ncols + 1][GS]
  int* zcol;      // [ncells] count-0 column or -1
  int* base_col;  // [ncells]
  // chunked launches (the host-count pipeline): every column array above (ucl, T, maxi,
  // has_clamp, D, U, UQ, colc) and the per-cell arrays start at the chunk's first column / cell;
  // zcol and base_col hold global column indices, col_base = the chunk's first global column
  int col_base;
  // Cell-staged tables (phases 0 and 2, G <= 448): per block {cell, first column, end
  // column, 0}; one task with cell -1 writes the ELL pad column (phase 2).  Null: the
  // column-per-wave kernel.
  const int4* tasks;
  int ntasks;
  // Stretch bounds for k_boot2's grid-stretch skipping (nullable): per column and 64-point
  // stretch j, max_j T (phase 1) or max_j T - max_j T[baseline column] (phase 2; the
  // maximum itself where the cell has no baseline); 0 for the pad column.  [ncols + 1][8]
  double* U;
  // k_boot_tiles' tile bounds (phase 2; nullable): per 32-point tile the column's maximum in
  // units of 2^-8, rounded up, as four balanced base-256 digits (packu); phase-2 columns
  // store it minus their baseline column's value.  Pad column: 0.  A NaN sets *nanflag.
  unsigned* UQ;            // [ncols + 1][kQTiles]
  int* nanflag;
  // nullable: the launch does nothing unless *gate != 0 (the exact fallback's T tables are
  // built only when some gene needs them)
  const int* gate;
  // k_tables only: take just the columns k_tables_lpc leaves (colc n < 0, flagged by
  // k_col_consts in the int after colc's last column); the launch exits unless that flag is set
  int slow_only;
};

// ---- k_boot_tiles' integer tile bounds
constexpr int kQTiles = 16;  // 32-point bound tiles per column (G <= 448 uses <= 14)
constexpr int kBTile = 32;   // grid points per bound tile
__host__ __device__ inline unsigned packu(int u) { return ((unsigned)u + 0x80808080u) ^ 0x80808080u; }  // |u| < 2^31
__host__ __device__ inline int unpacku(unsigned p) { return (int)((p ^ 0x80808080u) - 0x80808080u); }
// ZUq[set][l][t][Bp]: the baseline cells' part of the tile bounds (four digits l)
hipError_t launch_zuq(const unsigned* UQ, const int* base_col, int ncells, const unsigned char* W8, int Bp, int nsets,
                      int* ZUq, hipStream_t s);

struct BootArgs {
  const double* T;  // [ncols][GS]
  int G, GS;
  const int2* ent;  // [ngenes][ent_stride] (cell, flat column)
  const int* nnz;   // [ngenes]
  int ent_stride;
  const int* base_col;  // [ncells] baseline column (count 0) or -1; nullable
  const double* Wt;     // [nsets][ncells][Bp] draw multiplicities
  int ncells, Bp, nboot;
  const int* wset;   // [ngenes] draw-set id per gene (nullable -> 0)
  const double* Z;   // [nsets][Bp][GS] baseline sums (nullable)
  double norm_mult;  // nboot for logBoot*Posterior, 1 for jpmat*
  double degen_thresh;
  double* out;
  long long out_g, out_k;
  int* degen;  // [ngenes]
  int ngenes;
};

struct Boot2Args {
  const double* D;  // [ncols + 1][GS] baseline-delta columns (k_delta)
  long long ncols_p1;  // columns of D (ncols + 1)
  const int2* ent;  // [ngenes][ent_stride] (cell, column) -- the k_ell list
  const int* nnz;
  int ent_stride;
  const double* Wt;  // [nsets][ncells][Bp], Bp a multiple of nb
  int Bp, ncells;
  const int* wset;
  const double* Z;  // [nsets][Bp][GS]
  int G, GS, nboot, nb;
  double norm_mult, degen_thresh;
  double* part;  // [ceil(nboot/nb)][ngenes][GS] per-slab partial jp rows
  long long part_stride;
  double* out;
  long long out_g, out_k;
  int* degen;
  int ngenes;
  // Grid-stretch skipping (nullable U disables it; needs G <= 448, nb <= 20): stretch
  // bounds of the columns (TablesArgs::U) and their baseline part ZU [nsets][Bp][8]
  const double* U;
  const double* ZU;
  int* mask;     // [ngenes][P] needed-stretch bits (k_stretch_mask output)
  double* ubuf;  // [ngenes][P][8][nb] stretch upper bounds (k_stretch_mask output)
  int* redo;     // [ngenes][P] slabs whose skipped stretches failed the post-check (tile path:
                 // fallback flags, then the fallback list length and [ngenes * P] list)
  double slack;  // heuristic slack of the mask (NaN: the default 20 + 0.15 C)
};

// The tile bootstrap (with Boot2Args; needs G <= 448): multiplicities as bytes and the tables'
// 16-point tile bounds for the exact integer tile bounds of each (gene, slab).  k_boot_gene: a
// 4-wave block per (gene, group of SG slabs), 16 rows shared by the group's slabs; the slabs it
// cannot finish take k_boot_tiles, the four-tile list pass over `wide`, and its failures k_boot2.
struct TileBootArgs {
  const unsigned char* W8p;  // [nsets][ncells][P][32] draw multiplicities (<= 127): per slab the pairs
                             // (boot r, boot 16 + r) of its boots, r < 16 (0 past the slab's live boots)
  int Bq;                    // ZUq's boot stride: a multiple of 32, >= the last slab's first boot + 32
  const unsigned* UQ;        // [ncols + 1][kQTiles] packed 32-point tile maxima (units of 2^-8, rounded up)
  const int* ZUq;            // [nsets][4][kQTiles][Bq] baseline tile-bound digit sums
  const int* nanflag;        // tables saw a NaN: every slab goes to k_boot2
  int maxgroups;             // 32-point bound tiles computed per slab, 1..4 (4; tests force the fallback with fewer)
  int* stats;                // nullable: [0] slabs, [1] tiles computed, [2] tiles, [3] slabs left to k_boot2,
                             // [4] sum of groups x entries (FMA count / (64 nb)), [5] entries of the slabs left,
                             // [6 + i] slabs that computed i tiles (i <= 28), [35] slabs the gene blocks
                             // left to the list pass
  const int* order;          // nullable: genes in this order (launch_gene_order)
  unsigned* pmask;           // [ngenes][P] tiles each slab's partial row holds (k_sum_partials reads those)
  int* wide = nullptr;       // required: [1 + ngenes * P] the list pass's slabs: [0] length, then g * P + p
  int SG = 0;                // required: slabs per group (1..8, SG x nb <= 128)
  int kcap = 4;              // rows per slab at most (tests force the list pass with fewer)
  int list_cap = 0;          // slabs the list pass takes at most (0: 16384; tests force the overflow to k_boot2)
  const unsigned char* W8g = nullptr;  // required: [nsets][ncells][groups][4 windows][32] the group's boots
                                       // 32 w + j as pair slots (boot 32 w + j, 32 w + 16 + j), 0 past its boots
  // this launch takes genes [g_lo, g_hi) (g_hi < 0: all) -- a posterior's bootstrap in
  // gene chunks, each finished (list pass, fallback, slab sums) before the next, so its jp rows can
  // be read back while the next chunk runs; `order` then holds each chunk's genes sorted within it
  int g_lo = 0, g_hi = -1;
  // gene blocks holding all of a gene's slabs (SG >= P): [ngenes] flags; a gene whose slabs all pass
  // their post-checks gets its jp row from its block (summed in slab order, as k_sum_partials would)
  // and flag 1, so k_sum_partials skips it (null: every row through k_sum_partials)
  int* gdone = nullptr;
};
hipError_t launch_boot_tiles(const Boot2Args& a, const TileBootArgs& tb, hipStream_t s);
// gene order for the tile bootstrap: the keys launch_ell formed (per-gene count sums), sorted
hipError_t launch_gene_order(const unsigned* key, const int* idx, int n, unsigned* key_out, int* order, void* work,
                             size_t* work_bytes, hipStream_t s, int bits = 16);

struct ExactArgs {
  const double* T;  // log tables; or fused D columns when base_col is set (T = D + D[base])
  const int* base_col;
  int G, GS;
  const int* draws;  // [nsets][nboot][ndraw] cell index per draw, reference order (-1: no draw, the
                     // shorter group's padding when two groups are fused)
  int ndraw, nboot;
  long long gene_mod;  // fused groups: gene g reads uci row g % gene_mod (0: g)
  const int* wset;
  const long long* ucl_off;
  const int* uci;  // [ld_uci x ncells] or null for jpmat (column = cell*ngenes + g)
  long long ld_uci;
  double norm_mult;
  const int* degen;
  double* out;
  long long out_g, out_k;
  int ngenes;
  int g_lo = 0, g_hi = -1;  // the launch's genes [g_lo, g_hi) (g_hi < 0: all): a gene chunk
};

struct NoBootArgs {
  const double* T;  // log tables, or normalised exp tables for ensemble
  int G, GS;
  const long long* ucl_off;
  const int* uci;
  long long ld_uci;
  int ncells, ngenes;
  int ensemble;
  double* out;
  long long out_g, out_k;
};

struct RatioArgs {
  const double* jp1;
  long long j1g, j1k;
  const double* jp2;
  long long j2g, j2k;
  const double* prior_y;  // nullable: skip.prior.adjustment
  int n, ngenes;
  int normalize;  // 1: divide by the (long double) row sum (calculate.ratio.posterior); 0: raw matSlideMult
  const double* xin;  // nullable: summarise this ratio matrix [g*xg + o*xo] (m = 2n-1 columns) instead
  long long xg, xo;
  double* ratio;  // nullable; [g*rg + o*ro]
  long long rg, ro;
  const double* diffv;  // [2n-1]
  int zi;
  double* res;  // nullable; column-major res_ld x 5 (lb, mle, ub, ce, Z)
  long long res_ld;
};

hipError_t launch_cell_prep(const double* models, int ncells, int G, int GS, const double* mag, int lt, int sq,
                            double* mu, double* lcfp, double* lcfpr, double* theta, double* cellscal,
                            double* pq, hipStream_t s, double* cfp = nullptr);
hipError_t launch_col_consts(const int* ucl, const long long* ucl_off, long long ncols, int ncells,
                             const double* theta, int GS, const double* cellscal, double* colc, hipStream_t s);
hipError_t launch_tables(const TablesArgs& a, hipStream_t s);
// gsets > 0 (two fused groups): sets from gsets on sum the cells from gsplit on, the others the
// cells before it, each in its group's own order
hipError_t launch_stretch_zu(const double* U, const int* base_col, int ncells, const double* Wt, int Bp, int nsets,
                             double* ZU, hipStream_t s, int gsets = 0, int gsplit = 0);
hipError_t launch_base_cols(const int* ucl, const long long* ucl_off, int ncells, const unsigned char* has_clamp,
                            int use_baseline, int* base_col, hipStream_t s);
// out[i] = in[i] for n 16-bit counts
hipError_t launch_widen16(const unsigned short* in, int* out, size_t n, hipStream_t s);
// out[exc[i].x] = exc[i].y for n listed counts (indices relative to out)
hipError_t launch_patch32(const int2* exc, size_t n, int* out, hipStream_t s);
// padto 8: rows padded to a multiple of 8 plus one batch of 8 (k_boot2's look-ahead); 64: to a
// multiple of 64 plus 8 (the tile bootstrap's bound MFMAs take 64-entry steps)
// cell_off: added to the cell of every entry (a fused second group's cells follow the first's)
// key (nullable, with ucl and idx): the tile bootstrap's 16-bit gene-order keys (log-scaled sums
// of the entries' counts ucl[col]) and gene indices, the launch's genes being genes kg0 .. of kgn
// split into kch gene chunks (the chunk index in the key's top bits; desc: descending within a
// chunk)
hipError_t launch_ell(const int* uci, long long ld_uci, int ngenes, int ncells, const long long* ucl_off,
                      const int* base_col, int stride, int pad_col, int padto, int2* ent, int* nnz, hipStream_t s,
                      int cell_off, const int* ucl = nullptr, unsigned* key = nullptr, int* idx = nullptr,
                      int kg0 = 0, int kgn = 0, int kch = 1, int desc = 0);
hipError_t launch_baseline_z(const double* T, int G, int GS, const int* base_col, int ncells, const double* Wt,
                             int Bp, int nsets, double* Z, hipStream_t s, int gsets = 0, int gsplit = 0);
// Draw multiplicities on the device from the draw lists draws[nsets][nboot][ndraw] (cell index, -1
// = no draw): Wt[set][c][Bp] (doubles), and for the tile path (nullable) W8[set][c][Bt],
// W8p[set][c][P][32] (per slab of nb boots the pairs (j, 16 + j) in slots 2j, 2j + 1) and
// W8g[set][c][NGR][128] (per group of SG slabs four 32-boot windows as pair slots).  The arrays are
// zeroed here first.  ncells <= kMultMaxCells.
constexpr int kMultMaxCells = 16384;
hipError_t launch_mult(const int* draws, int nsets, int nboot, int ndraw, int ncells, int Bp, double* Wt, int Bt,
                       unsigned char* W8, int nb, int P, unsigned char* W8p, int SG, int NGR, unsigned char* W8g,
                       hipStream_t s);
// test hook: one wave spinning `cycles` shader clocks on stream s (handoff_spin)
hipError_t launch_spin(hipStream_t s, long long cycles);
hipError_t launch_boot(const BootArgs& a, hipStream_t s);
hipError_t launch_boot_exact(const ExactArgs& a, hipStream_t s);
int boot2_nb(int nboot);
hipError_t launch_boot2(const Boot2Args& a, hipStream_t s);
hipError_t launch_delta(const double* T, const long long* ucl_off, int ncells, long long ncols, const int* base_col,
                        int G, int GS, double* D, hipStream_t s);
hipError_t launch_noboot(const NoBootArgs& a, hipStream_t s);
hipError_t launch_ensemble_cols(const double* T, long long ncols, int G, int GS, double* E, hipStream_t s);
hipError_t launch_modes(const int* uci, long long ld_uci, int ngenes, int ncells, const long long* ucl_off,
                        const int* maxi, const double* mag, double* modes, long long mg, long long mc,
                        hipStream_t s);
hipError_t launch_post(const int* uci, long long ld_uci, int ngenes, int c, const long long* ucl_off,
                       const double* T, int G, int GS, double* post, long long pg, long long pk, hipStream_t s);
hipError_t launch_cell_minmax(const int* counts, long long ld, long long g0, int ngenes, int ncells,
                              const int* cellidx, int* cmax, int* cmin, hipStream_t s);
hipError_t launch_mark(const int* counts, long long ld, long long g0, int ngenes, int ncells, const int* cellidx,
                       const long long* woff, unsigned long long* bits, hipStream_t s,
                       int* flags = nullptr);
hipError_t launch_rank(const unsigned long long* bits, const long long* woff, int ncells, int* rank, int* nuniq,
                       hipStream_t s,
                       const int* flags_in = nullptr, int* flags_out = nullptr);
hipError_t launch_fill_ucl(const unsigned long long* bits, const long long* woff, int ncells, const int* rank,
                           const long long* ucl_off, int* ucl, hipStream_t s);
hipError_t launch_uci(const int* counts, long long ld, long long g0, int ngenes, int ncells, const int* cellidx,
                      const long long* woff, const unsigned long long* bits, const int* rank, int* uci,
                      hipStream_t s);
hipError_t launch_colmajor_to_rows(const double* src, int nrows, int ncols, int GS, double* dst, hipStream_t s);
// device BH cZ (bh.hip); work == nullptr -> *work_bytes = required size
hipError_t launch_bh_cz(const double* z, int n, double* cz, void* work, size_t* work_bytes, hipStream_t s);

// scde.expression.prior (prior.hip).  cellp: 5 x C (corr.b, corr.a, conc.b, conc.a, conc.a2).
// Stats: out[0..3] = sum w, sum w over finite v, max finite v, count of finite v; occ:
// prior_items(N, C) x 256 count multiplicities (read back by launch_prior_bin); vout (nullable)
// = v per element in R order.
hipError_t launch_prior_stats(const int* counts, long long ld, int N, int C, const double* cellp, int sq,
                              double* vout, int* occ, double* partials, int nb, double* out, hipStream_t s);
long long prior_items(int N, int C);
int prior_blocks(int N, int C, int cap);
int prior_grid_n(int L);
// hist: prior_grid_n(L) u64 (zeroed here); work: 3 x prior_grid_n(L) doubles; out: 4 x (L+1)
// (x, y, lp, grid.weight)
hipError_t launch_prior_bin(const int* counts, long long ld, int N, int C, const double* cellp, int sq,
                            const int* occ, double wsum, double max_value, double bw, int L,
                            unsigned long long* hist, int nb, hipStream_t s);
hipError_t launch_prior_tail(double tot_mass, double max_value, double bw, int L, double pc,
                             const unsigned long long* hist, double* work, double* out, hipStream_t s);
hipError_t launch_sort_doubles(const double* in, double* out, long long n, void* work, size_t* work_bytes,
                               hipStream_t s);
// k_ratio_summary keeps both rows (twice) and the 2n-1 outputs in dynamic LDS: above 64 KiB
// the launcher opts in, above the 160 KiB of a workgroup it returns hipErrorInvalidValue
// without launching.  ratio_n_max() is the largest n that fits (callers refuse a larger one).
size_t ratio_lds_bytes(int n);
int ratio_n_max();
int ratio_n_default_lds();  // the largest n that launches without the opt-in
hipError_t launch_ratio_summary(const RatioArgs& a, hipStream_t s);


// ---- weighted PCA (wpca.hip; src/bwpca.cpp).  One problem = a column subset of the
// resident cells x genes value/weight matrices (column g at M + col*ld), optionally
// row-permuted per column (internal shuffles).  All offsets in elements.
constexpr int kWpcaMaxK = 8;
struct WpcaProb {
  int d, K, nstarts, pad;
  long long col_off;    // cols[col_off .. +d)
  long long perm_off;   // perms[perm_off .. + d*n) or -1
  long long start_off;  // starts[start_off .. + nstarts*d*K): randu(d, K) per start
  long long sE_off;     // scratch: best eigenvectors, nstarts x d x K
  long long sC_off;     // scratch: coefficient slots, nstarts x 2 x n x K
  long long sW_off;     // scratch: working coefficients (when not in LDS), nstarts x n x K
  long long mom_off;    // scratch: moments + smoothing row, nstarts x d x (NM + 1)
  long long stat_off;   // stat rows (pres, bpres, iterations, best slot), one per start
  long long out_rot, out_sc, out_pcw, out_cm, out_var;  // outputs (var: K + 2 doubles)
};
struct WpcaLaunch {
  const double* M;
  const double* W;
  long long ld;
  int n, dmax;
  const WpcaProb* probs;
  const int2* blocks;
  const int* cols;
  const int* perms;
  const double* starts;
  int maxiter;
  double tol;
  const double* smoothc;
  int L;
  double* scratch;
  double* stat;
  double* out;
  int lds_cap;
};
int wpca_max_k();
int wpca_ms_group();
bool wpca_ms_ok(int n, int dmax);
// npcs = 1, em without smoothing: blocks = (problem, first start of a group of wpca_ms_group())
hipError_t launch_wpca_ms(const WpcaLaunch& a, int nblocks, hipStream_t s);
hipError_t launch_wpca_em(int K, const WpcaLaunch& a, int nblocks, hipStream_t s);
hipError_t launch_wpca_final(int K, const WpcaLaunch& a, const int* kidx, int nprob, hipStream_t s);

// ---- PAGODA helpers (pagoda.hip; src/pagoda.cpp).  Matrices column-major.
// winsorize: m k x n, ntr per side; n <= 8192, or ntr <= 32
hipError_t launch_winsorize(const double* m, int k, int n, int ntr, double* out, hipStream_t s);
// matWCorr: m, w k x n -> out n x n
hipError_t launch_matwcorr(const double* m, const double* w, int k, int n, double* out, hipStream_t s);
// matCorr: x k x nx, y k x ny -> out nx x ny; stats: 2 (nx + ny) doubles of scratch
hipError_t launch_matcorr(const double* x, int k, int nx, const double* y, int ny, double* stats, double* out,
                          hipStream_t s);
// plSemicompleteCor2: np lists (off[np + 1], idx, val) -> r, cnt np x np
hipError_t launch_plcor(int np, const long long* off, const int* idx, const double* val, double* r, int* cnt,
                        hipStream_t s);
// pagoda.varnorm's mode consumer: modes from jp (expected value or row-maximum magnitude);
// the weight matrix 1 - mfp * sfp for cells cellidx (matw: ngenes x ncells col-major)
hipError_t launch_vn_modes(const double* jp, long long jg, long long jk, int ngenes, int G, const double* mag,
                           int expected, double* modes, hipStream_t s);
hipError_t launch_vn_matw(const int* counts, long long ld, int ngenes, const int* cellidx, int ncells,
                          const double* models, int mld, int sq, const double* modes, const long long* mode_off,
                          double* matw, hipStream_t s);

// ---- pagoda.varnorm after the weights, pagoda.subtract.aspect (varnorm.hip; contract in
// include/scde_hip.h).  Matrices N x C column-major, a gene contiguous; models C x 12.
// The edf table on the device: n values y and second derivatives m2 of the natural cubic
// spline of log(edf) over the uniform grid lt0 + i h of log(theta)
struct VnEdf {
  const double* y;
  const double* m2;
  int n;
  double lt0, h;
};
// out: 3 x N (edf, wvar, rowSums(matw)), with bmatw / codes 7 x N (+ bedf, bwvar, rowSums(bmatw),
// bwvar / wvar); modes: (1 + levels) x N
hipError_t launch_varnorm_moments(const int* counts, long long ld, int N, int C, const double* models, int local_theta,
                                  const double* modes, const double* matw, const double* bmatw, const int* codes,
                                  const VnEdf& edf, double th_lo, double th_hi, double power, double* out,
                                  hipStream_t s);
// order / lev_off: the cells grouped by level (one level of all cells without a batch); wsrc:
// matw, or bmatw with a batch; ws: 3 x nlev x N doubles of scratch
hipError_t launch_varnorm_matrix(const int* counts, long long ld, int N, int C, const double* models, const int* order,
                                 const int* lev_off, int nlev, int batched, const double* wsrc, double weight_k,
                                 const double* arv, double* ws, double* mat, double* matw_out, hipStream_t s);
// v: the aspect, centred and of unit length
hipError_t launch_subtract_aspect(const double* mat, const double* matw, int N, int C, const double* v, int center,
                                  double* out, hipStream_t s);

// ---- drop-out-adjusted cell-to-cell correlations (dist.hip; vignettes/diffexp.md:231-301).
// Matrices genes x cells column-major; cellp: 5 x C (corr.b, corr.a, conc.b, conc.a, conc.a2).
// x = log10(cd + 1), fpm = scde.expression.magnitude, pself = scde.failure.probability at fpm
// (each nullable), from resident counts
hipError_t launch_dist_prep(const int* counts, long long ld, int N, int C, const double* cellp, int sq, double* x,
                            double* fpm, double* pself, hipStream_t s);
// the mode-relative measure's X = log10(exp(modes) + 1) and U = matw^(1/4)
hipError_t launch_dist_mode_prep(const int* counts, long long ld, int N, int C, const double* cellp, int sq,
                                 const double* modes, const double* jpm, double* x, double* u, hipStream_t s);
// one simulation of the direct measure: masked X / U from uniforms (unif, or the generator keyed
// by dist_sim_key(seed, simulation) when unif is null)
uint64_t dist_sim_key(uint64_t seed, int sim);
hipError_t launch_dist_direct_prep(const double* xin, const double* pself, long long NC, double k,
                                   const double* unif, uint64_t key, double* x, double* u, hipStream_t s);
// correlation with weights u[g, i] u[g, j] (out C x C, both triangles; accumulate: out += corr)
hipError_t launch_wcorr_gram(const double* X, const double* U, long long ld, int N, int C, double* out,
                             int accumulate, hipStream_t s);
// correlation with the reciprocal weights (X, F dense N x C)
hipError_t launch_recip_corr(const double* X, const double* F, int N, int C, const double* cellp, int sq, double k,
                             double* out, hipStream_t s);

// ---- hierarchical clustering (hclust.hip; the contract is in include/scde_hip.h).
// One problem of a launch: the n x n column-major matrix at src + src_off (leading dimension
// ld, strict lower triangle read), its workspace of hclust_ws_bytes(n) at ws + ws_off (bytes, a
// multiple of 256), its n - 1 raw steps at element out_off of oi / oj / oh.
struct HclustProblem {
  long long src_off, ld, ws_off, out_off;
  int n;
};
size_t hclust_ws_bytes(int n);
// one workgroup per problem; method 0..5 (ward.D, ward.D2, single, complete, average, mcquitty).
// Step s of a problem merged slots oi[s] < oj[s] at oh[s] (ward.D2: the squared height).
// flag[p]: -1 done; >= 0 the first non-finite pair, column j * n + row i (no steps written);
// <= -2 an inconsistent neighbour cache at step -2 - flag (an internal error)
hipError_t launch_hclust(const double* d, const HclustProblem* probs, int nprob, int method, char* ws, int* oi,
                         int* oj, double* oh, long long* flag, hipStream_t s);
// x <- 1 - x over an n x n matrix, the diagonal exactly 0 (a correlation matrix into a distance
// matrix, in place)
hipError_t launch_one_minus(double* x, long long n, hipStream_t s);
// R's merge ((n - 1) x 2 column-major), height and order from the raw steps (host)
void hclust_encode(int n, const int* si, const int* sj, const double* sh, int method, int* merge, double* height,
                   int* order);

// ---- optimal leaf ordering (olo.hip; the contract is in include/scde_hip.h).
// 0, or the 1-based row that makes merge ((n - 1) x 2, R's encoding) no tree over n observations;
// msg says why (host)
int olo_check_merge(int n, const int* merge, char* msg, size_t cap);
// The whole computation on a resident n x n matrix (strict lower triangle read) and a checked
// merge: workspace (3 n^2 doubles + O(n)) allocated and freed inside, results to the host.
// 0 done; 1 an argument error (a non-finite distance); 2 a HIP error (out of memory included);
// 3 an internal error; msg holds the text.  stats (may be null): launches, candidates.
int olo_solve(hipStream_t s, const double* d_dev, long long ld, int n, const int* merge, int* merge_out,
              int* order_out, double* length, double* stats, char* msg, size_t cap);

// ---- stats::dist between the rows of a resident column-major n x p matrix (rdist.hip; the
// contract is in include/scde_hip.h).
// *flag = 1 when any value of x is NaN or infinite, otherwise 0
hipError_t launch_rdist_flag(const double* x, long long ld, int n, int p, int* flag, hipStream_t s);
// method 0 euclidean, 1 manhattan, 2 maximum; count = false only for an x without NaN or Inf;
// out: n x n, both triangles, the diagonal 0; n such that the lower-triangle 64 x 64 tiles fit a grid
hipError_t launch_rdist(const double* x, long long ld, int n, int p, int method, bool count, double* out,
                        hipStream_t s);

// ---- exact t-SNE of a distance matrix (tsne.hip; the contract is in include/scde_hip.h).
struct TsneParams {
  double eta, exaggeration, momentum, final_momentum;
  int stop_lying_iter, mom_switch_iter;
};
// columns per chunk of the gradient kernel and the number of chunks: functions of n alone (they
// fix the order of every sum)
int tsne_chunk(int n);
int tsne_nchunks(int n);
// bytes of the workspace every call below takes (a multiple of 256)
size_t tsne_ws_bytes(int n);
// Each call checks nothing but the data, queues its kernels on s and waits for them.  0 done; 1 an
// argument error (a refused distance); 2 a HIP error; msg holds the text.  d: n x n column-major,
// leading dimension ld, strict lower triangle read; P: n x n, receives the affinities (both
// triangles; it must not overlap d); beta, costs: host, n values; Y, uY, gains: resident, n x 2
// row-major, 16-byte aligned
int tsne_affinities(hipStream_t s, const double* d, long long ld, int n, double perplexity, int squared, double* P,
                    double* beta, char* ws, char* msg, size_t cap);
int tsne_iterate(hipStream_t s, const double* P, int n, const TsneParams& prm, int iter0, int niter, double* Y,
                 double* uY, double* gains, char* ws, char* msg, size_t cap);
int tsne_cost(hipStream_t s, const double* P, int n, const double* Y, double* costs, char* ws, char* msg, size_t cap);

// ---- the randomised rounds of pagoda.gene.clusters (rnorm.hip, pagoda.hip, sigma1.hip; contract
// in include/scde_hip.h).  Round matrices are ncells x ngenes column-major (a gene contiguous).
// R's norm_rand() (INVERSION) from raw Mersenne-Twister outputs, two per normal: draw t goes to
// gene t % ngenes, cell t / ngenes
hipError_t launch_rnorm(const uint32_t* raw, int ngenes, int ncells, double* out, hipStream_t s);
// winsorize every gene of an ncells x ngenes matrix (launch_winsorize's kernels on this layout)
hipError_t launch_winsorize_gc(const double* x, int ncells, int ngenes, int ntr, double* out, hipStream_t s);
// keep[g] = (sum over cells of the rounded |x[k + 1]| - |x[k]|, in double-double) != 0
hipError_t launch_keep_absdiff(const double* x, int ncells, int ngenes, int* keep, hipStream_t s);
// out column j = x column cols[j] (nrow rows each)
hipError_t launch_gather_cols(const double* x, int nrow, const int* cols, int ncols, double* out, hipStream_t s);
// Squared largest singular value of the ncells x |cols| blocks of x.  Problem p: columns
// idx[off[p] .. off[p + 1]), a workspace of sigma1_ws_doubles(.) doubles at ws + ws_off[p].
// out[p]: the value; flag[p]: 0, or 1 when a column index was outside [0, ngenes) (out[p] is NaN)
size_t sigma1_ws_doubles(long long ncols, int ncells);
hipError_t launch_sigma1sq(const double* x, int ncells, long long ngenes, int nprob, const long long* off,
                           const int* idx, const long long* ws_off, double* ws, double* out, int* flag,
                           hipStream_t s);
// Sturm count of the pivots <= 0 of T - x I (d: diagonal, e2: squared off-diagonal; dstebz's pivot
// recurrence): the eigenvalue bisections of sigma1.hip and aspects.hip
__device__ __forceinline__ int sturm_count(const double* __restrict__ d, const double* __restrict__ e2, int n,
                                           double x, double pivmin) {
  double q = d[0] - x;
  if (fabs(q) < pivmin) q = -pivmin;
  int c = q <= 0.0;
  for (int i = 1; i < n; ++i) {
    q = d[i] - e2[i - 1] / q - x;
    if (fabs(q) < pivmin) q = -pivmin;
    c += q <= 0.0;
  }
  return c;
}

// ---- aspect redundancy reduction (aspects.hip; contract in include/scde_hip.h).  Square
// matrices are m x m column-major; patterns are ncells x m column-major (an aspect contiguous).
// Student-t renormalisation of the pairs i < j of r (union sizes cnt) to target_ndf, mirrored
// into cr; cr's diagonal is r's
hipError_t launch_t_renorm(const double* r, const int* cnt, int m, double target_ndf, double* cr, hipStream_t s);
// d = the distance from the Pearson correlation c of the m columns of x (ncells x m; z: scratch
// of the same size): with cr the combined loading x pattern distance, without it 1 - c or
// 1 - |c|; NaN for a column that holds a single value; both triangles, diagonal 0
hipError_t launch_aspect_dist(const double* x, int ncells, int m, double* z, const double* cr, int ab, double power,
                              double* d, hipStream_t s);
// d (matWCorr's result: the lower triangle) becomes 1 - c or 1 - |c|, both triangles, diagonal 0
hipError_t launch_wdist(double* d, int m, int ab, hipStream_t s);
// collapse.aspect.clusters: cluster p = rows idx[off[p] .. off[p + 1]) of x / w, a workspace of
// collapse_ws_doubles(.) doubles at ws + ws_off[p]; column p of d / wo receives the pattern and
// the weights.  top[p]: the row of largest variance; status[p]: 0, 1 when the pattern must be
// replaced by the fallback draw, -1 when a row index was outside [0, m); ocor[p]: the orientation
// correlation after the flip (NaN where none was taken)
size_t collapse_ws_doubles(long long k, int ncells, int pick_top);
hipError_t launch_collapse(const double* x, const double* w, int ncells, int m, int nclust, const long long* off,
                           const int* idx, const long long* ws_off, double* ws, int scale, int pick_top, double* d,
                           double* wo, int* top, int* status, double* ocor, hipStream_t s);

// ---- knn.error.models' neighbourhood stage (knn.hip; contract in include/scde_hip.h).  counts
// N x C column-major (ld); x, u, fpm, nabove dense N x C; sim C x C column-major; nb C x kmax
// row-major with entries in [-1, C).  More than kKnnMaxCells cells: hipErrorInvalidValue.
constexpr int kKnnMaxCells = 8192;
hipError_t launch_knn_prep(const int* counts, long long ld, int N, int C, int thr, double* x, double* u,
                           hipStream_t s);
hipError_t launch_knn_neighbours(const double* sim, int C, const int* groups, const int* kcell, int kmax, int* out,
                                 hipStream_t s);
hipError_t launch_knn_magnitudes(const int* counts, long long ld, int N, int C, const int* nb, int kmax,
                                 const double* ls, int thr, double trim, double* fpm, int* nabove, hipStream_t s);

// ---- knn.error.models' mixture fit (knn_fit.hip; contract in include/scde_hip.h).  fpm, fp (the
// starting failed-component posteriors, NaN outside a cell's valid genes), clusters and post are
// N x C dense; models is C x 12 column-major.  A cell with at most lds_genes valid genes keeps its
// per-gene vectors in LDS, a larger one in its workgroup's slice of ws (knn_fit_ws_bytes(ws_cap)
// bytes per workgroup, ws_cap at least the largest cell's valid genes; ws may be null when no
// cell exceeds lds_genes).  grid: workgroups launched (at most C are).
int knn_fit_lds_genes_max();
size_t knn_fit_lds_bytes(int lds_genes);
size_t knn_fit_ws_bytes(long long ws_cap);
hipError_t knn_fit_resident_groups(int lds_genes, int* groups);
hipError_t launch_knn_fit(const int* counts, long long ld, int N, int C, const double* fpm, const double* fp,
                          int local_theta, double theta_lo, double theta_hi, double awp, int max_iter, int lds_genes,
                          char* ws, long long ws_cap, int grid, double* models, int* iters, double* llh, int* status,
                          int* clusters, double* post, hipStream_t s);

// ---- scde.error.models' input stage (error_models.hip; contract in include/scde_hip.h).  counts
// N x C column-major (ld); fpm, fp, nabove dense N x C.  goff (ngroups + 1) cuts members (the
// cells, group by group, each group in cell order); need: per cell, the nabove a valid gene has
// at least; poff (C + 1) cuts part, every cell's cross-fit partners; nvalid (C, zeroed by the
// caller) receives every cell's number of valid genes.  Every group has at least two cells.
hipError_t launch_crossfit_inputs(const int* counts, long long ld, int N, int C, int ngroups, const int* goff,
                                  const int* members, const int* need, const int* poff, const int* part,
                                  const double* ls, int thr, double* fpm, double* fp, int* nabove, int* nvalid,
                                  hipStream_t s);

// ---- scde.error.models' mixture fit with linear.fit = FALSE (nb2_fit.hip; contract in
// include/scde_hip.h).  Arguments, LDS and workspace as launch_knn_fit's (knn_fit_lds_bytes,
// knn_fit_ws_bytes); log_background_rate is written to the models as fail.r.
hipError_t nb2_fit_resident_groups(int lds_genes, int* groups);
hipError_t launch_nb2_fit(const int* counts, long long ld, int N, int C, const double* fpm, const double* fp,
                          double background_rate, double log_background_rate, int max_iter, int lds_genes, char* ws,
                          long long ws_cap, int grid, double* models, int* iters, double* llh, int* status,
                          int* clusters, double* post, hipStream_t s);

// ---- the mixture cross-fit of cell pairs (crossfit_fit.hip; contract in include/scde_hip.h).
// first, second: the P pairs' cells.  status (P) is always written; iters, llh (P), params (P x 10
// column-major), clusters (P blocks of N int8) and post (P blocks of 2 x N: component 1, then
// component 3) may each be null.  A pair with at most lds_rows rows keeps its vectors in LDS, a
// larger one in its workgroup's slice of ws (crossfit_fit_ws_bytes(ws_cap) bytes per workgroup,
// ws_cap at least the largest pair's rows; ws may be null when N <= lds_rows).
int crossfit_fit_lds_rows_max();
size_t crossfit_fit_lds_bytes(int lds_rows);
size_t crossfit_fit_ws_bytes(long long ws_cap);
hipError_t crossfit_fit_resident_groups(int lds_rows, int* groups);
hipError_t launch_crossfit_fit(const int* counts, long long ld, int N, int P, const int* first, const int* second,
                               int thr, double min_prior, double zero_lambda, int max_iter, int lds_rows, char* ws,
                               long long ws_cap, int grid, int* status, int* iters, double* llh, double* params,
                               signed char* clusters, double* post, hipStream_t s);

// ---- from pair results to the per-cell fit's inputs (error_models.hip; contract in
// include/scde_hip.h).  Lists as launch_crossfit_inputs'; the partner list is replaced by plist:
// per cell, poff cuts its entries 2 * pair + side (side 1: the cell is the pair's second), in the
// pairs' order.  pstatus (P), clusters and post as launch_crossfit_fit writes them.  vil: N x C
// uint8.  launch_crossfit_vil is the first step alone (vil; fplog: N x C, the fail prior before vi).
hipError_t launch_crossfit_vil(int N, int C, const int* poff, const int* plist, const int* pstatus,
                               const signed char* clusters, const double* post, unsigned char* vil, double* fplog,
                               hipStream_t s);
hipError_t launch_crossfit_reduce(const int* counts, long long ld, int N, int C, int ngroups, const int* goff,
                                  const int* members, const int* need, const int* poff, const int* plist,
                                  const int* pstatus, const signed char* clusters, const double* post,
                                  const double* ls, unsigned char* vil, double* fpm, double* fp, int* nabove,
                                  int* nvalid, hipStream_t s);

// ---- pagoda.top.aspects' matrix step (top_aspects.hip; contract in include/scde_hip.h).  x, w,
// xv, xvw: m x C row-major (an aspect contiguous); num: m values.  Row r of xv is x's row centred
// times num[r] / sqrt(its variance, denominator C - 1), row r of xvw is w's row over its sum
hipError_t launch_top_aspects(const double* x, const double* w, const double* num, int m, int C, double* xv,
                              double* xvw, hipStream_t s);

// ---- Spearman rank correlation (spearman.hip; contract in include/scde_hip.h).
// launch_rank_cols: x, out nrow x ncol column-major, out == x allowed; tmp (nrow x ncol doubles) is
// needed only when rank_cols_needs_tmp(nrow) and out == x.
bool rank_cols_needs_tmp(int nrow);
hipError_t launch_rank_cols(const double* x, int nrow, int ncol, double* out, double* tmp, hipStream_t s);
// The cell similarity.  counts N x C column-major (ld); codes spearman_code_ld(N) x C,
// spearman_code_bytes(N) bytes an entry, 16-byte aligned; D: every cell's number of distinct valid values (all codes of cell c are below
// D[c], or the code type's largest value where the entry is not valid).  The prepass sorts in
// LDS, or in ws (spearman_codes_ws_bytes(N, C) bytes, 0: not needed).  The pair kernel takes dmax,
// the largest D (read back by the caller), and keeps the tables of a pair with
// D[i] + D[j] <= min(lds_values, spearman_lds_values_max()) entries (lds_values 0: the maximum) in
// LDS, those of a larger pair in ws (spearman_pairs_ws_bytes(C, dmax, lds_values) bytes, 0: none
// is larger).  out: C x C column-major.
int spearman_code_bytes(int N);
int spearman_code_ld(int N);
int spearman_lds_values_max();
size_t spearman_codes_ws_bytes(int N, int C);
size_t spearman_pairs_ws_bytes(int C, int dmax, int lds_values);
hipError_t launch_spearman_codes(const int* counts, long long ld, int N, int C, int thr, void* codes, int* D,
                                 unsigned* ws, hipStream_t s);
hipError_t launch_spearman_pairs(const void* codes, int N, int C, const int* D, int dmax, int lds_values, unsigned* ws,
                                 double* out, hipStream_t s);

}  // namespace scde
