// engine_internal.h -- what the library's host files share: the error macros, the device
// buffer, the context, and the few helpers of the pipeline (engine.hip) that the feature
// files (api_*.hip) call.  Internal: not installed, not included from include/.
//
// Everything here that is a function or a variable lives in scde::host, which has hidden
// visibility: it links across the library's files and is no dynamic symbol of the library.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "scde_hip.h"

#define SCDE_HIDDEN __attribute__((visibility("hidden")))

namespace scde {
namespace host SCDE_HIDDEN {

// sets the thread's error text (scde_last_error) and returns code
int fail(int code, const char* fmt, ...);
// SCDE_OK, or SCDE_EFORK in a fork child of the process that initialised HIP (engine.hip)
int fork_guard();

}  // namespace host
}  // namespace scde

#define FORK_GUARD()                                      \
  do {                                                    \
    if (int fg_ = ::scde::host::fork_guard()) return fg_; \
  } while (0)

#define HCHK(expr)                                                                                     \
  do {                                                                                                 \
    hipError_t e_ = (expr);                                                                            \
    if (e_ != hipSuccess) return ::scde::host::fail(SCDE_EHIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

#define RCHK(expr)            \
  do {                        \
    int r_ = (expr);          \
    if (r_ != SCDE_OK) return r_; \
  } while (0)

namespace scde {
namespace host SCDE_HIDDEN {

inline long long round_up(long long a, long long b) { return (a + b - 1) / b * b; }

// a workspace allocation failed: clears the HIP error, the message is the caller's
template <class... Args>
int fail_oom(const char* fmt, Args... args) {
  (void)hipGetLastError();
  return fail(SCDE_EHIP, fmt, args...);
}

// The C library rand() the reference calls (srand(Seed), then
// `rj = rand()/(RAND_MAX/n)` with rejection; src/jpmatLogBoot.cpp:220-221,255-257),
// with private state.  Its output depends on the platform libc:
//   SCDE_RAND_GLIBC  (0) glibc TYPE_3 additive feedback generator (Linux);
//   SCDE_RAND_DARWIN (2) Darwin/BSD libc: Park-Miller "minimal standard"
//                        x = 16807 x mod (2^31-1), srand(s) keeps s, returns x --
//                        the generator behind the package vignette's printed
//                        results (vignettes/diffexp.md:113-139).
extern int g_rand_kind;

struct PlatformRand {
  int kind;
  int32_t t[31];
  int f = 3, r = 0;
  PlatformRand(unsigned int seed, int k) : kind(k) {
    if (kind == 2) {
      t[0] = (int32_t)seed;
      return;
    }
    if (seed == 0) seed = 1;
    t[0] = (int32_t)seed;
    int32_t word = (int32_t)seed;
    for (int i = 1; i < 31; ++i) {
      const long hi = word / 127773, lo = word % 127773;
      word = (int32_t)(16807 * lo - 2836 * hi);
      if (word < 0) word += 2147483647;
      t[i] = word;
    }
    for (int i = 0; i < 310; ++i) next();
  }
  int next() {
    if (kind == 2) {
      const long hi = t[0] / 127773, lo = t[0] % 127773;
      long x = 16807 * lo - 2836 * hi;
      if (x < 0) x += 0x7fffffff;
      t[0] = (int32_t)x;
      return (int)x;
    }
    const uint32_t v = (uint32_t)t[f] + (uint32_t)t[r];
    t[f] = (int32_t)v;
    if (++f >= 31) f = 0;
    if (++r >= 31) r = 0;
    return (int)(v >> 1);
  }
  int draw(int n) {
    int rj;
    while (n <= (rj = next() / (2147483647 / n))) {
    }
    return rj;
  }
};

// Reallocations of an existing workspace buffer (grow-only, so early calls only): each one is
// a hipFree, which waits for the device, plus -- for grow(keep) -- a copy after the owning
// context's streams are synchronised.  Counted process-wide (stat "buf_reallocs") so a
// regression that reallocates in steady state shows.
extern std::atomic<long long> g_buf_reallocs;

// A device allocation that its owner frees: a Buf member of the context (or of one of its
// unique sets) goes back to the device when the context is destroyed, with no list to keep.
struct Buf {
  void* p = nullptr;
  size_t cap = 0;
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  ~Buf() { release(); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap && p) return hipSuccess;
    if (p) {
      g_buf_reallocs.fetch_add(1, std::memory_order_relaxed);
      hipError_t e = hipFree(p);
      p = nullptr;
      cap = 0;
      if (e != hipSuccess) return e;
    }
    size_t want = std::max<size_t>(bytes, 256);
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  // ensure(bytes), or with keep: grown (25% headroom) keeping the contents, after
  // sync_streams() has drained every stream of the owning context that may still write or
  // read the old allocation (scoped to that context: the peer lane, other contexts and torch
  // streams keep running)
  template <class SyncStreams>
  hipError_t grow(bool keep, size_t bytes, SyncStreams&& sync_streams) {
    if (!keep || !p) return ensure(bytes);
    if (bytes <= cap) return hipSuccess;
    const size_t want = bytes + bytes / 4;
    void* q = nullptr;
    g_buf_reallocs.fetch_add(1, std::memory_order_relaxed);
    hipError_t e = sync_streams();
    if (e == hipSuccess) e = hipMalloc(&q, want);
    if (e == hipSuccess) e = hipMemcpy(q, p, cap, hipMemcpyDeviceToDevice);
    if (e != hipSuccess) {
      if (q) (void)hipFree(q);
      return e;
    }
    (void)hipFree(p);
    p = q;
    cap = want;
    return hipSuccess;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const {
    return reinterpret_cast<T*>(p);
  }
};

}  // namespace host
}  // namespace scde

// kernel-time slots (scde_ctx_kernel_times)
enum {
  SLOT_TABLES = 0,
  SLOT_BOOT = 1,
  SLOT_RATIO = 2,
  SLOT_UNIQUE = 3,
  SLOT_OTHER = 4,
  SLOT_PRIOR_STATS = 5,
  SLOT_PRIOR_BIN = 6,
  SLOT_PRIOR_TAIL = 7,
  SLOT_WPCA_EM = 8,
  SLOT_WPCA_FINAL = 9,
  NSLOTS = 10
};

struct scde_ctx {
  using Buf = scde::host::Buf;
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t home_stream = nullptr;  // `stream` as created (unique builds swap `stream` for a while)
  // host-count entry points: the count upload runs on its own stream, in column chunks, so
  // the first group's kernels start before the second group's columns have arrived
  hipStream_t copy_stream = nullptr;
  hipEvent_t up_ev[2] = {nullptr, nullptr};
  hipEvent_t uq_ev = nullptr;  // the second group's unique sets (built on copy_stream) are ready
  hipEvent_t modes_ev = nullptr;  // run_posterior's posterior modes are computed (they need the tables only)
  // run_posterior's bootstrap set-up (draw uploads, ELL rows, baseline bound sums, Z, gene
  // order) needs only the count-0 columns: it runs on aux_stream after p1_ev (phase 1 of the
  // tables), beside phase 2, and the bootstrap waits for aux_ev
  hipStream_t aux_stream = nullptr;
  hipEvent_t p1_ev = nullptr, aux_ev = nullptr;
  // Pinned staging arena for the small per-call transfers (cell lists, offsets, draws,
  // multiplicities, tasks; the unique builder's size read-backs).  A pageable copy is staged
  // by the runtime and costs 20-40 us of host latency each; from pinned memory it is a plain
  // asynchronous DMA.  Bump-allocated; when full, the device is synchronised (every staged
  // copy has landed) and allocation restarts at 0.
  char* pin = nullptr;
  size_t pin_off = 0;
  // workspace
  Buf models, mag, mu, lcfp, cfp, lcfpr, theta, cellscal, pq, colc, T, E, maxi, has_clamp, base_col, zcol, ent, nnz, Wt, Z, draws,
      ubound, zubound, smask, subuf, sredo,
      degen, wset, prior_y, diffv, jpA, jpB, res, ratio, in1, in2, outbuf, part, bhw;
  // scde.expression.prior
  Buf pr_cell, pr_part, pr_occ, pr_stats, pr_hist, pr_work, pr_out, pr_v, pr_sorted, pr_sortw;
  // weighted PCA (bwpca)
  Buf wp_probs, wp_blocks, wp_kidx, wp_cols, wp_perms, wp_starts, wp_scratch, wp_stat, wp_out, wp_smooth, wp_M, wp_W;
  // PAGODA helpers
  Buf pg_a, pg_b, pg_c, pg_d, pg_e;
  // cell-to-cell distance measures (dist.hip): X, U, fpm / modes, p.self.fail / uniforms, per-cell
  // constants, per-gene modes, the C x C result
  Buf ds_x, ds_u, ds_f, ds_p, ds_x0, ds_cell, ds_jpm, ds_out;
  // hierarchical clustering (hclust.hip): a host matrix staged, the problems' workspaces, the
  // problem descriptors, the raw steps (oi, oj, oh, flags)
  Buf hc_in, hc_ws, hc_prob, hc_out;
  // stats::dist (rdist.hip): a host matrix staged, the non-finite flag (a host call's result is
  // staged in hc_in)
  Buf rd_x, rd_flag;
  // the random rounds of pagoda.gene.clusters: raw twister words, keep flags / column lists,
  // sigma1's problem lists, workspace and results
  Buf gr_raw, gr_int, gr_prob, gr_ws, gr_out;
  // aspect redundancy reduction (aspects.hip): staged host matrices (r, n, cr), the patterns
  // scaled to unit length, the collapse kernel's cluster lists, workspace and per-cluster results
  Buf as_r, as_n, as_cr, as_z, as_prob, as_ws, as_out;
  // pagoda.varnorm: the weights stage's modes and weight matrices kept in HBM for the moments
  // and matrix stages (vn_n x vn_c, vn_nb levels: what the last weights call left), the edf
  // table, the cell lists, the per-level scratch, mat / matw before they go to the host
  Buf vn_modes, vn_matw, vn_bmatw, vn_tab, vn_int, vn_ws, vn_vec, vn_mat, vn_wout;
  int vn_n = -1, vn_c = -1, vn_nb = 0;
  // pagoda.top.aspects: the row factors, and the host entry's staged scores, weights and results
  Buf ta_num, ta_x, ta_w, ta_xv, ta_xvw;
  // knn.error.models' neighbourhood stage: the similarity (kn_sim_c cells; -1: none), the
  // neighbour lists (kn_nb_c x kn_nb_k), groups and per-cell k, library sizes, fpm and nabove
  // before they go to the host
  Buf kn_sim, kn_nb, kn_int, kn_ls, kn_fpm, kn_nab;
  int kn_sim_c = -1, kn_nb_c = -1, kn_nb_k = -1;
  // Spearman (spearman.hip): a host matrix staged for the rank transform and the counting path's
  // second copy; the similarity's dense codes, distinct-value counts and workspace
  Buf sp_x, sp_tmp, sp_codes, sp_d, sp_ws;
  // knn.error.models' mixture fit: fpm and the starting posteriors staged, the workspace of the
  // cells too large for LDS, the results before they go to the host
  Buf kf_fpm, kf_fp, kf_ws, kf_models, kf_int, kf_llh, kf_cl, kf_post;
  // scde.error.models' input stage: the group and partner lists, nabove; its fpm and fail_prior
  // land in kf_fpm / kf_fp and stay there for a fit (ci_n x ci_c, the largest cell has ci_nmax
  // valid genes; ci_n = -1: nothing resident)
  Buf ci_int, ci_ls, ci_nab;
  int ci_n = -1, ci_c = -1;
  long long ci_nmax = 0;
  // the mixture cross-fit of pairs: the pairs' cells, status and iterations, the parameters and
  // llh, the workspace; clusters (int8, cf_p blocks of cf_n genes) and the posteriors stay
  // resident for scde_crossfit_reduce_* with the host's copy of the pairs and their status
  // (cf_n = -1: nothing resident); the reduction's pair status, lists and vil
  Buf cf_int, cf_par, cf_ws, cf_cl, cf_post, cf_red, cf_vil;
  int cf_n = -1, cf_p = -1;
  std::vector<int> cf_pairs_h, cf_status_h;
  // host-count entry points: the call's counts staged here (grow-only, reused across calls)
  Buf counts_in;
  // fixed-point bootstrap: byte multiplicities, flags/counters
  Buf w8, w8t, w8g, qflags;
  // tile bootstrap gene order: keys, sorted keys, indices, order, sort workspace
  Buf gkey, gkey2, gidx, gorder, gwork, pmask, pwide, excd, gdone;
  // options (scde_ctx_set_option; include/scde_hip.h lists them): each a default path's switch or a
  // documented operating / test mode; read from the environment only at creation (SCDE_OPTIONS)
  int opt_boot_skip = 1;         // "boot_skip": grid-stretch / tile skipping in the bootstrap (same bits either way)
  double opt_skip_slack = NAN;   // "skip_slack": mask slack (NaN = 20 + 0.15 C); tests force redo slabs
  int opt_boot_nb = 0;           // "boot_nb": boots per slab (0 = automatic; a multiple of 4 in [4, 32])
  int opt_skip_stats = 0;        // "skip_stats": count kept stretches / redo slabs (a host sync per launch)
  int opt_wpca_ms = 1;           // "wpca_ms": the multi-start npcs = 1 kernel (k_wpca_ms1)
  int opt_boot_tiles = 1;        // "boot_tiles": the FP64 bootstrap on bounded 32-point tiles (k_boot_gene)
  int opt_boot_tiles_cells = 400;  // "boot_tiles_cells": cells per call from which it is used (fewer: the
                                   // rows are wide, most slabs need > 8 tiles, k_boot2's stretches win)
  int opt_tile_groups = 4;       // "tile_groups": 32-point bound tiles the list pass computes per slab (1..4; tests)
  int opt_tile_max_mult = 127;   // "tile_max_mult": largest multiplicity the tile path takes (int8; tests lower it
                                 // to force the fallback onto plain k_boot2 after the tables were set up for tiles)
  int opt_tile_order = 3;        // "tile_order": the tile bootstrap takes genes by count sum (cache sharing):
                                 // 1 ascending, 2 descending (heaviest first), 3 (default: descending in
                                 // scde.posteriors and in DE launches of at most kDescGenes genes, where the
                                 // last, heaviest blocks would set the launch's tail), 0 in gene order
  int opt_unique_fixed = 1;      // "unique_fixed": one host sync per unique build (fixed 1024-word bitmaps)
  int opt_upload_u16 = 1;        // "upload_u16": host-count ranges of >= 8 MB go up as 16-bit counts (U16Ring): 1
                                 // scde.posteriors' host entry, 2 every host entry, 0 none
  int opt_modes_overlap = 1;     // "modes_overlap": scde.posteriors' read-backs (modes piece by piece, jp in gene
                                 // chunks) overlap the tables and the bootstrap from a read-back thread (0: after
                                 // the bootstrap, on the main stream -- rocprofv3 runs, where the pageable
                                 // read-back becomes blit kernels that would share the CUs)
  int opt_jp_chunks = 4;         // "jp_chunks": gene chunks of scde.posteriors' gene-block bootstrap (host entry: each
                                 // chunk's jp rows read back while the next runs; 1: one launch, jp after it)
  int opt_gene_list_cap = 0;     // "gene_list_cap": slabs k_boot_gene's list pass takes at most (0: 16384; tests)
  int opt_gene_rows = 4;         // "gene_rows": rows per slab k_boot_gene gives each slab at most (tests force its
                                 // four-tile list pass with fewer)
  double opt_pipeline_mb = 32;  // "pipeline_mb": host-count DE calls from this many MB of counts upload in two
                                // column ranges, each group starting once its cells are in HBM
  int opt_pieces = 5;           // "pieces": the first group's columns of a pipelined host-count DE call upload
                                // in this many pieces, each piece's unique sets and tables starting as it lands
                                // (round 6, config 3, 5 alternating runs each: 4 pieces 6.49-6.78 ms host ->
                                // host, 5 pieces 6.38-6.48, 6 pieces 6.41-6.58)
  int opt_tables_nt = 2;        // "tables_nt": table rows as non-temporal stores (0 no, 1 yes, 2 when the call's
                                // rows exceed 256 MB)
  int fault_u16 = 0;            // test hook (scde_ctx_inject_fault): 16-bit upload slots to fail
  long long spin_cycles = 0;    // test hook: a spin kernel before every cross-stream handoff (handoff_spin)
  int fault_skip_join = 0;      // test hook: DE calls whose main stream skips its wait for the peer lane
  std::atomic<long long> st_spins{0};  // handoff spins launched (any thread; the peer counts its own)
  int opt_lanes = 2;            // "lanes": a DE call's two group posteriors run concurrently (2: the second
                                // group on `peer`, its own streams and workspace) or one after the other (1)
  // the second lane of a DE call: a context on the same device, created on first use; its
  // options are copied from this one per call and its timings/statistics merged back
  scde_ctx* peer = nullptr;
  hipEvent_t lane_ev[2] = {nullptr, nullptr};  // [0] this stream -> peer, [1] peer -> this stream
  hipEvent_t piece_ev[8] = {nullptr};           // run_posterior's pieces: unique sets built
  hipEvent_t piece_up_ev[8] = {nullptr};        // the pieces' uploads landed (upload worker)
  hipStream_t uq_stream = nullptr;              // the pieces' and the second group's unique builds
  // host-count upload thread (created on first use, lives with the context): a pageable copy
  // blocks its calling thread for the whole transfer, so the pieces go up from here, back to
  // back, while the caller builds unique sets and queues kernels
  struct Uploader {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    bool stop = false, busy = false;
    long long job = 0;
    std::function<int(int)> issue;  // issue(j): upload range j and record its event
    int nranges = 0, issued = 0, err = 0;
    std::string err_msg;  // the worker thread's error text (its g_err is its own)
    std::chrono::steady_clock::time_point t_start;  // the job's start (stat upload_wake_ms)
    double wake_ms = 0, first_ms = 0;  // summed: start -> worker awake, start -> first range issued
  } upl;
  // Device -> host read-backs from a worker thread (a pageable hipMemcpy blocks its calling thread
  // for the whole transfer): scde.posteriors' modes columns piece by piece and its jp rows chunk by
  // chunk, each after the event recorded when its kernels were queued, so the read-back streams
  // out while later pieces' tables and chunks' bootstraps run.  Jobs of one call; dnl_wait drains.
  struct Downloader {
    struct Job {
      int ev;  // index into evs
      void* dst;
      const void* src;
      size_t dpitch, spitch, width, height;
    };
    std::thread th;
    std::mutex m;
    std::condition_variable cv, cvd;
    std::deque<Job> q;
    std::vector<hipEvent_t> evs;
    hipStream_t stream = nullptr;
    int pending = 0, err = 0, nev = 0;
    std::string err_msg;
    bool stop = false;
    bool hold = false;  // jobs queue but wait (dnl_hold): pageable read-backs slow the host-count uploads
  } dnl;
  // 16-bit host-count uploads (option "upload_u16"): a pool of T threads narrows each 4M-count
  // slot of the caller's int32 matrix to uint16 into a pinned ring slot, listing the counts
  // outside [0, 65535] (index, value) as they go; the upload worker sends the slot up, a widening
  // kernel writes the int32 counts behind it on the copy stream and a patch kernel the listed
  // ones (real matrices hold a few: config 4's synthetic 60M counts hold 10) -- half the PCIe bytes (tools/micro/h2d_u16.hip, 240 MB of counts: 2.9 ms
  // against 4.5 ms pageable).  Slots carry a global sequence number q (ring slot q % kRing); the
  // threads may write slot q once q < free_upto, i.e. once slot q - kRing's DMA has completed.
  // Every wait blocks (condition variables, blocking-sync events): spinning threads would eat the
  // process's CPU share that the caller's thread and the lanes' threads need.
  struct U16Ring {
    static constexpr int kRing = 4;
    static constexpr size_t kSlotCounts = size_t(4) << 20;
    unsigned short* pin = nullptr;  // kRing slots
    unsigned short* dev = nullptr;  // kRing device slots (widened from)
    hipEvent_t ev[kRing] = {};
    long long seq = 0;     // next sequence number
    long long issued = 0;  // slots whose DMA is queued
    long long free_upto = kRing;  // (under m, as fin and abort)
    int fin[kRing] = {};
    static constexpr int kMaxT = 32;
    static constexpr int kThreads = 4;  // the narrowing pool's threads (<= kMaxT)
    std::vector<int2> exc[kRing][kMaxT];  // per ring slot and thread: (index in the slot, count)
    std::vector<int2> exc_all;            // one slot's list, uploaded
    bool abort = false;
    std::vector<std::thread> th;
    int T = 0;
    std::mutex m;
    std::condition_variable cv, cvd, cvf;  // job / job done, slot freed / slot narrowed
    long long job = 0;
    int busy = 0;
    bool stop = false;
    const int* src = nullptr;
    size_t n = 0;
    long long q0 = 0;
    int nslots = 0;
    double st_wait_ms = 0, st_issue_ms = 0, st_free_ms = 0;  // issuer: narrowing waits, copy issue, slot frees
  } u16;
  // statistics (scde_ctx_get_stat)
  double st_skip_slabs = 0, st_skip_kept = 0, st_skip_stretches = 0, st_skip_redo = 0, st_degen = 0;
  // host wall time of scde_expression_difference_{dev,host} phases (ms, summed over calls):
  // setup, unique tables (incl. their syncs), posteriors enqueued, ratio + results read back
  double st_host_ms[4] = {0, 0, 0, 0};
  // arithmetic the bootstrap kernels issued (skip_stats runs): FP64 lane FMAs of k_boot2 (kept
  // stretches x 64 lanes x slab boots x entries)
  double st_boot_f64_fma = 0;
  double st_stream_syncs = 0;  // grow(keep) drains of this context's streams (scoped, never the device)
  double st_arena_syncs = 0;   // pinned-arena wraps (this context's streams drained)
  // run_posterior's pieces (host ms): waiting for a piece's upload, then its unique build and tables launch
  double st_piece_wait_ms = 0, st_piece_host_ms = 0;
  double st_pair_redo = 0;  // slabs the gene blocks left to the four-tile list pass (k_boot_tiles)
  double st_olo[2] = {0, 0};  // the last optimal leaf ordering: kernel launches, candidates (add + min each)
  double st_boot_path = -1;  // the bootstrap kernel of the last posterior: 0 k_boot2, 1 k_boot_tiles, 3 general
  static constexpr int kQMaxTilesHost = 28;
  double st_tile_hist[kQMaxTilesHost + 1] = {0};
  // ucl/uci of a cell subset (R/functions.R:609-610); one set per group so both groups'
  // unique tables can be built up front, with their host syncs, before the heavy kernels
  struct UniqueSet {
    Buf cellidx, cmax, cmin, woff, bits, rank, nuniq, ucl, ucl_off, uci, flags;
    std::vector<int> cmax_h, cmin_h, nuniq_h;
    std::vector<long long> woff_h, ucl_off_h;
    // pinned landing area of the phases' device -> host size read-backs: the set's own (not
    // the shared staging arena), so no later staging can recycle it before the host reads it
    int fixed_flags = 0;  // unique_phase12_fixed's flags when no pinned landing area exists
    int woff_fixed = 0;   // entries of woff holding the fixed offsets c * fixed_words (0: other contents)
    // bitmap words per cell of the fixed-width build: 1024 (counts below 65,536), widened to the
    // power of two an exact rebuild needed (so a data set with larger counts pays the rebuild's two
    // extra host syncs once, not on every call), at most kUniqueFixedWordsMax
    long long fixed_words = 1024;
    long long woff_fixed_w = 0;  // the width woff_fixed's offsets were uploaded for
    int* pin_land = nullptr;
    size_t pin_land_cap = 0;  // ints
    const int* pin_in = nullptr;  // this phase's read-back (pin_land, or null: pageable fallback)
    std::vector<int4> tasks_h;  // cell-staged tables tasks (k_tables_cell)
    Buf tasks;
    bool ready = false;
    // a piece of a larger set (run_posterior's pieces): phase 3 writes the unique counts into
    // into->ucl from column into_col0 on (grown to an estimate of the whole set's columns,
    // into_cap_hint) and the count indices into into->uci from cell into_c0 on; its own ucl_off
    // (from 0) serves the piece's tables launch
    UniqueSet* into = nullptr;
    long long into_col0 = 0, into_cap_hint = 0;
    int into_c0 = 0;
    int* landing(size_t n) {
      if (n > pin_land_cap) {
        if (pin_land) (void)hipHostFree(pin_land);
        pin_land = nullptr;
        pin_land_cap = 0;
        if (hipHostMalloc(reinterpret_cast<void**>(&pin_land), sizeof(int) * n, hipHostMallocDefault) != hipSuccess) {
          pin_land = nullptr;
          (void)hipGetLastError();
          return nullptr;
        }
        pin_land_cap = n;
      }
      return pin_land;
    }
    ~UniqueSet() {
      if (pin_land) (void)hipHostFree(pin_land);
    }
  } us[3];
  static constexpr int kMaxPieces = 8;
  UniqueSet upc[kMaxPieces];  // run_posterior's pieces
  UniqueSet task_us;          // run_posterior's tables tasks (unpieced): per context, so lanes sharing a
                              // unique set never write one tasks buffer
  // profiling
  bool profile = false;
  struct Pending {
    int slot;
    hipEvent_t a, b;
  };
  std::vector<Pending> pending;
  std::vector<hipEvent_t> evpool;
  double ms[NSLOTS] = {0};
  long long launches[NSLOTS] = {0};
  std::vector<void*> user_allocs;

  hipEvent_t get_event() {
    if (!evpool.empty()) {
      hipEvent_t e = evpool.back();
      evpool.pop_back();
      return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
  }
  hipEvent_t mark_begin(int slot) {
    if (!profile) return nullptr;
    hipEvent_t a = get_event();
    (void)hipEventRecord(a, stream);
    (void)slot;
    return a;
  }
  void mark_end(int slot, hipEvent_t a) {
    if (!profile || !a) return;
    hipEvent_t b = get_event();
    (void)hipEventRecord(b, stream);
    pending.push_back({slot, a, b});
  }
  int sync() {
    HCHK(hipStreamSynchronize(stream));
    if (peer) {  // the peer lane's timings count as this context's
      RCHK(peer->sync());
      for (int i = 0; i < NSLOTS; ++i) {
        ms[i] += peer->ms[i];
        launches[i] += peer->launches[i];
        peer->ms[i] = 0;
        peer->launches[i] = 0;
      }
    }
    for (auto& p : pending) {
      float t = 0.f;
      if (hipEventElapsedTime(&t, p.a, p.b) == hipSuccess) {
        ms[p.slot] += t;
        launches[p.slot] += 1;
      }
      evpool.push_back(p.a);
      evpool.push_back(p.b);
    }
    pending.clear();
    return SCDE_OK;
  }
  // What is no Buf goes here, in this order: the threads joined first, then the peer, the events,
  // the streams, the pinned arena.  The workspace follows by itself: the Buf members (and the
  // unique sets') are destroyed after this body, so device memory is freed once the streams are
  // gone -- hipFree needs none, and scde_ctx_destroy has synchronised `stream` before.
  ~scde_ctx() {
    if (dnl.th.joinable()) {
      {
        std::lock_guard<std::mutex> lk(dnl.m);
        dnl.stop = true;
      }
      dnl.cv.notify_all();
      dnl.th.join();
    }
    for (auto e : dnl.evs) (void)hipEventDestroy(e);
    if (dnl.stream) (void)hipStreamDestroy(dnl.stream);
    if (upl.th.joinable()) {
      {
        std::lock_guard<std::mutex> lk(upl.m);
        upl.stop = true;
      }
      upl.cv.notify_all();
      upl.th.join();
    }
    if (!u16.th.empty()) {  // (after the upload worker, its only user)
      {
        std::lock_guard<std::mutex> lk(u16.m);
        u16.stop = true;
      }
      u16.cv.notify_all();
      for (auto& t : u16.th) t.join();
    }
    if (u16.pin) (void)hipHostFree(u16.pin);
    if (u16.dev) (void)hipFree(u16.dev);
    for (auto& e : u16.ev)
      if (e) (void)hipEventDestroy(e);
    if (peer) {
      (void)hipStreamSynchronize(peer->stream);
      delete peer;
    }
    for (auto& e : lane_ev)
      if (e) (void)hipEventDestroy(e);
    for (auto& e : piece_ev)
      if (e) (void)hipEventDestroy(e);
    for (auto& e : piece_up_ev)
      if (e) (void)hipEventDestroy(e);
    if (uq_stream) (void)hipStreamDestroy(uq_stream);
    for (void* p : user_allocs) (void)hipFree(p);
    for (auto& p : pending) {
      (void)hipEventDestroy(p.a);
      (void)hipEventDestroy(p.b);
    }
    for (auto e : evpool) (void)hipEventDestroy(e);
    if (stream) (void)hipStreamDestroy(stream);
    if (copy_stream) (void)hipStreamDestroy(copy_stream);
    if (uq_ev) (void)hipEventDestroy(uq_ev);
    if (modes_ev) (void)hipEventDestroy(modes_ev);
    if (p1_ev) (void)hipEventDestroy(p1_ev);
    if (aux_ev) (void)hipEventDestroy(aux_ev);
    if (aux_stream) (void)hipStreamDestroy(aux_stream);
    if (pin) (void)hipHostFree(pin);
    for (auto& e : up_ev)
      if (e) (void)hipEventDestroy(e);
  }
};

namespace scde {
namespace host SCDE_HIDDEN {

// ------------------------------------------------------------------ posterior spec
struct PostSpec {
  int ncells = 0;
  const double* models = nullptr;  // host ncells x 12 col-major
  int localtheta = 0, squarelogit = 0;
  const double* mag = nullptr;  // host G
  int G = 0;
  int nboot = 0;
  int postflag = 0;
  int ensemble = 0;
  bool batch_call = false;  // logBootBatchPosterior semantics
  // source A: host ucl/uci
  const int* ucl_host = nullptr;
  const int64_t* ucl_off_host = nullptr;
  const int* uci_host = nullptr;
  // source B: device counts
  const int* counts_dev = nullptr;
  long long ld = 0;
  const int* cellidx_host = nullptr;
  int ngenes = 0;
  // seeding: per set seed, per gene set (empty -> all set 0)
  std::vector<int> seeds;
  std::vector<int> wset;
  // batch
  const int* batch_vals = nullptr;
  const int64_t* batch_off = nullptr;
  const int* comp = nullptr;
  int nbatch = 0;
  // outputs (device)
  double* jp = nullptr;
  long long jp_g = 0, jp_k = 0;
  double* modes = nullptr;  // ngenes x ncells col-major
  bool modes_early = false;  // modes right after the tables, with cx->modes_ev recorded (copy_modes_out)
  double* post = nullptr;   // ncells blocks of ngenes x G col-major
  bool use_baseline = true;
  int rand_kind = 0;
  // counts arriving in pieces (de_run's host-count pipeline): piece j holds this spec's cells
  // [piece_c[j], piece_c[j + 1]) and is in HBM once piece_ready(j) returned and piece_stream
  // reached the point it recorded; run_posterior builds each piece's unique sets on
  // piece_stream and launches its tables as it arrives (piece_ev: one event per piece)
  int npieces = 0;
  const int* piece_c = nullptr;
  std::function<int(int)> piece_ready;
  hipStream_t piece_stream = nullptr;
  hipEvent_t* piece_ev = nullptr;
  // host destinations read back by the context's Downloader while later work runs (the caller then
  // copies neither and drains the Downloader before returning): modes_host, the modes matrix
  // (pieces: each piece's columns once its tables are done); jp_host, the joint posterior in R's
  // layout (jp_g = 1, jp_k = ngenes) -- with the gene-block bootstrap in jp_chunks gene chunks, each
  // chunk's rows read back while the next chunk's bootstrap runs
  double* modes_host = nullptr;
  double* jp_host = nullptr;
  int jp_chunks = 1;
};

// ------------------------------------------------------------------ engine.hip, for the feature files
// the process's default context (created on first use: SCDE_DEVICE, SCDE_RAND)
int default_ctx(scde_ctx** out);
// an entry point's context: the default one for a null ctx, then its device made current
int use_ctx(scde_ctx*& ctx);

// `bytes` from the host into b (grown as needed) on st / on the context's stream, small
// transfers through the pinned arena
int upload_on(scde_ctx* cx, Buf& b, const void* src, size_t bytes, hipStream_t st);
int upload(scde_ctx* cx, Buf& b, const void* src, size_t bytes);

// a host N x C column-major matrix (leading dimension ld) into a dense device buffer, on the
// context's stream
template <class T>
int put_matrix(scde_ctx* ctx, Buf& b, const T* src, int64_t ld, int N, int C) {
  const size_t row = sizeof(T) * (size_t)N;
  HCHK(b.ensure(std::max<size_t>(1, row * C)));
  if (N == 0) return SCDE_OK;
  if (ld == N) HCHK(hipMemcpyAsync(b.p, src, row * C, hipMemcpyHostToDevice, ctx->stream));
  else
    HCHK(hipMemcpy2DAsync(b.p, row, src, sizeof(T) * (size_t)ld, row, C, hipMemcpyHostToDevice, ctx->stream));
  return SCDE_OK;
}

// the caller's host counts (ngenes x ncols, leading dimension ld) into the context's staging
// buffer; *dev is the dense device matrix (ld = ngenes).  Takes the default context for a null ctx.
int stage_counts(scde_ctx*& ctx, const int* counts, int64_t ld, int ngenes, int ncols, const int** dev);

// scde.posteriors' pieces, as pagoda.varnorm's weights stage runs them
std::vector<double> marginals(const double* prior_x, int G);
void seeding(int n_cores, long long gene_offset, long long N_total, int ngenes, std::vector<int>& seeds,
             std::vector<int>& wset);

// ------------------------------------------------------------------ engine.hip, for engine_posterior.hip
// the ordering tests' spin hook, before every event another stream or host thread waits on; and every
// cross-stream wait: s waits for ev, then spins
hipError_t handoff_spin(scde_ctx* cx, hipStream_t s);
hipError_t handoff_wait(scde_ctx* cx, hipStream_t s, hipEvent_t ev);
// the read-back thread: queue a 2-D read-back after the work queued so far on `after`; hold queued
// read-backs back (on) or let them run (off)
int dnl_push(scde_ctx* cx, hipStream_t after, void* dst, size_t dpitch, const void* src, size_t spitch, size_t width,
             size_t height);
void dnl_hold(scde_ctx* cx, bool on);
// every stream of the context that touches its workspace
hipError_t ctx_streams_sync(scde_ctx* cx);

// ------------------------------------------------------------------ engine_posterior.hip
// ucl/uci of ns (1..4) cell subsets of the same device counts, on the context's stream
int build_unique_sets(scde_ctx* cx, const PostSpec* const* s, scde_ctx::UniqueSet* const* u, int ns);
// One posterior.  rest (nullable): return once the tables are queued, with the remaining work (modes,
// draws, bootstrap, outputs) in *rest, to be run later on the same stream.  *rest refers to s and u:
// the caller keeps both alive and unchanged until it has run.
int run_posterior(scde_ctx* cx, const PostSpec& s, scde_ctx::UniqueSet& u, std::function<int()>* rest = nullptr);

}  // namespace host
}  // namespace scde
