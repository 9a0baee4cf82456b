// engine.hip -- host orchestration and the C ABI (include/scde_hip.h).
//
// Restates the R glue of the path on the host side (R/functions.R:566-669
// scde.posteriors, 3491-3531 ratio posterior / Z, 5039-5051 summary / BH) and
// drives the gfx950 kernels of kernels.hip, unique.hip, boot.hip and ratio.hip (launchers in
// kernels.h) on one HIP stream per context.
//
// Layout of the library's host code: engine.hip is the pipeline -- the context's lifecycle,
// options and statistics, the posterior and differential-expression entry points with their
// lanes, upload and read-back threads, and the cross-stream handoff helpers.  What computes one
// posterior (run_posterior: its plan, unique counts, tables, pieces and bootstrap) is in
// engine_posterior.hip.  A feature's host code lives beside its kernel file's name: api_stats.hip (prior.hip, bh.hip, R's RNG),
// api_pagoda.hip (wpca, pagoda, rnorm, sigma1, aspects, varnorm), api_cluster.hip (dist, hclust,
// olo, tsne).  What they share -- the context, Buf, the error macros, the staging helpers -- is
// in engine_internal.h; a new feature adds its buffers there and its entry points to an api_ file.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cfloat>
#include <cmath>
#include <cerrno>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <deque>
#include <functional>
#include <thread>
#include <atomic>
#include <memory>
#include <unistd.h>
#include <mutex>
#include <numeric>
#include <string>
#include <vector>

#include "engine_internal.h"
#include "kernels.h"

using namespace scde;
using namespace scde::host;

namespace {
thread_local std::string g_err;
}  // namespace

int scde::host::fail(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

// Fork guard (SURVEY.md §8(b) threading row).  The reference's R glue forks mclapply
// workers that each make their own .Call (R/functions.R:606-617), and with n.cores = 1 (or
// N <= n.cores) it calls in the R parent itself (629-637), so a session can initialise HIP
// in the parent and fork later.  A HIP runtime is not fork-safe: a child must not touch the
// state it inherited.  g_hip_pid records the process that made this library's first HIP
// call; any GPU entry in another process (a fork child of it) fails with SCDE_EFORK before
// any HIP call.  A process forked *before* that first call (mclapply from a fresh session)
// sees 0 and initialises its own runtime, as tests/test_fork.py checks.
static std::atomic<pid_t> g_hip_pid{0};

int scde::host::fork_guard() {
  const pid_t me = getpid();
  pid_t p = g_hip_pid.load(std::memory_order_acquire);
  if (p == me) return SCDE_OK;
  if (p == 0 && g_hip_pid.compare_exchange_strong(p, me)) return SCDE_OK;
  if (p == me) return SCDE_OK;
  return fail(SCDE_EFORK,
              "HIP was initialised by process %d before this process (%d) was forked from it; a forked child "
              "cannot use the inherited GPU runtime. Run scde with n.cores = 1 in the parent (the fused entries "
              "honour n.cores for seeding only), or make the first GPU call in the child",
              (int)p, (int)me);
}

int scde::host::g_rand_kind = 0;
std::atomic<long long> scde::host::g_buf_reallocs{0};

namespace {

// R's chunk(seq_len(N), n) = split(x, sort(rank(x) %% n)) (R/functions.R:606):
// label r in 0..n-1 has #{i in 1..N : i %% n == r} genes, chunks in label order.
std::vector<long long> r_chunk_starts(long long N, int n) {
  std::vector<long long> starts;
  long long pos = 0;
  for (int r = 0; r < n; ++r) {
    long long cnt = (r == 0) ? N / n : (N >= r ? (N - r) / n + 1 : 0);
    if (cnt > 0) starts.push_back(pos);
    pos += cnt;
  }
  starts.push_back(N);
  return starts;
}

}  // namespace

// test hook (scde_ctx_inject_fault "handoff_spin"): a spin kernel on the producing stream before every
// event another stream or host thread waits on -- a missing wait then shows as wrong results every time
hipError_t scde::host::handoff_spin(scde_ctx* cx, hipStream_t s) {
  if (cx->spin_cycles <= 0) return hipSuccess;
  ++cx->st_spins;
  return launch_spin(s, cx->spin_cycles);
}
// Every cross-stream wait: stream s waits for ev, then (handoff_spin hook) spins -- the work s
// queues next, the producer side of later handoffs, starts late, so a consumer elsewhere that
// misses its wait on that work reads it before it is written every time.  (The spin before each
// event record delays the signal as well.)
hipError_t scde::host::handoff_wait(scde_ctx* cx, hipStream_t s, hipEvent_t ev) {
  hipError_t e = hipStreamWaitEvent(s, ev, 0);
  if (e == hipSuccess) e = handoff_spin(cx, s);
  return e;
}
// The main stream's wait for the peer lane's posterior (lane_ev[1]) before the ratio.  Test hook
// "skip_lane_join": the next `count` DE calls leave it out -- the negative control of the ordering
// tests (with the spins, the ratio then reads the second group's joint posterior unwritten).
static hipError_t lane_join(scde_ctx* ctx) {
  if (ctx->fault_skip_join > 0) {
    --ctx->fault_skip_join;
    return hipSuccess;
  }
  return handoff_wait(ctx, ctx->stream, ctx->lane_ev[1]);
}

// Downloader: queue a read-back of `height` rows of `width` bytes (pitches in bytes) after the work
// queued so far on `after`; dnl_wait returns once every queued read-back has landed (or failed).
int scde::host::dnl_push(scde_ctx* cx, hipStream_t after, void* dst, size_t dpitch, const void* src, size_t spitch,
                         size_t width, size_t height) {
  auto& d = cx->dnl;
  if (!d.th.joinable()) {
    HCHK(hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking));
    d.th = std::thread([cx] {
      auto& q = cx->dnl;
      (void)hipSetDevice(cx->device);
      std::unique_lock<std::mutex> lk(q.m);
      for (;;) {
        q.cv.wait(lk, [&] { return q.stop || (!q.q.empty() && !q.hold); });
        if (q.stop) return;
        const scde_ctx::Downloader::Job j = q.q.front();
        q.q.pop_front();
        const hipEvent_t ev = q.evs[j.ev];
        lk.unlock();
        hipError_t e = hipEventSynchronize(ev);
        if (e == hipSuccess)
          e = hipMemcpy2DAsync(j.dst, j.dpitch, j.src, j.spitch, j.width, j.height, hipMemcpyDeviceToHost, q.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(q.stream);
        lk.lock();
        if (e != hipSuccess && !q.err) {
          q.err = SCDE_EHIP;
          q.err_msg = hipGetErrorString(e);
        }
        if (--q.pending == 0) q.cvd.notify_all();
      }
    });
  }
  std::lock_guard<std::mutex> lk(d.m);
  if (d.nev == (int)d.evs.size()) {  // one event per job of a call (reused once dnl_wait drained them)
    hipEvent_t e = nullptr;
    // blocking sync: the read-back thread's hipEventSynchronize sleeps instead of spinning through
    // the tables and the bootstrap (the lanes' threads need the CPU share)
    HCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventBlockingSync));
    d.evs.push_back(e);
  }
  const int ei = d.nev++;
  HCHK(handoff_spin(cx, after));
  HCHK(hipEventRecord(d.evs[ei], after));
  d.q.push_back({ei, dst, src, dpitch, spitch, width, height});
  ++d.pending;
  d.cv.notify_all();
  return SCDE_OK;
}

// hold queued read-backs back (on) or let them run (off)
void scde::host::dnl_hold(scde_ctx* cx, bool on) {
  auto& d = cx->dnl;
  {
    std::lock_guard<std::mutex> lk(d.m);
    d.hold = on;
  }
  d.cv.notify_all();
}

int dnl_wait(scde_ctx* cx) {
  auto& d = cx->dnl;
  dnl_hold(cx, false);
  std::unique_lock<std::mutex> lk(d.m);
  d.cvd.wait(lk, [&] { return d.pending == 0; });
  d.nev = 0;
  const int err = d.err;
  const std::string msg = d.err_msg;
  d.err = 0;
  d.err_msg.clear();
  lk.unlock();
  return err ? fail(err, "read-back failed: %s", msg.c_str()) : SCDE_OK;
}

// every stream of the context that touches its workspace (grow(keep) drains these, not the device)
hipError_t scde::host::ctx_streams_sync(scde_ctx* cx) {
  for (hipStream_t st : {cx->stream, cx->home_stream, cx->copy_stream, cx->aux_stream, cx->uq_stream}) {
    if (!st) continue;
    hipError_t e = hipStreamSynchronize(st);
    if (e != hipSuccess) return e;
  }
  cx->st_stream_syncs += 1;
  return hipSuccess;
}

namespace {

constexpr size_t kPinCap = size_t(16) << 20;  // the arena
constexpr size_t kPinMax = size_t(2) << 20;   // larger transfers go direct

// `bytes` of the context's pinned arena (nullptr: too large, or the pinned allocation failed)
char* pin_alloc(scde_ctx* cx, size_t bytes) {
  if (bytes > kPinMax) return nullptr;
  if (!cx->pin) {
    if (hipHostMalloc(reinterpret_cast<void**>(&cx->pin), kPinCap, hipHostMallocDefault) != hipSuccess) {
      cx->pin = nullptr;
      (void)hipGetLastError();
      return nullptr;
    }
    cx->pin_off = 0;
  }
  size_t off = (cx->pin_off + 255) & ~size_t(255);
  if (off + bytes > kPinCap) {
    // reuse from the start: every host -> device copy staged so far must have been read out of
    // the arena first; they are issued on the context's own streams only (device -> host
    // read-backs land in each unique set's own area, never here)
    if (hipStreamSynchronize(cx->stream) != hipSuccess) return nullptr;
    if (cx->home_stream && hipStreamSynchronize(cx->home_stream) != hipSuccess) return nullptr;
    if (cx->copy_stream && hipStreamSynchronize(cx->copy_stream) != hipSuccess) return nullptr;
    if (cx->aux_stream && hipStreamSynchronize(cx->aux_stream) != hipSuccess) return nullptr;
    if (cx->uq_stream && hipStreamSynchronize(cx->uq_stream) != hipSuccess) return nullptr;
    cx->st_arena_syncs += 1;
    off = 0;
  }
  cx->pin_off = off + bytes;
  return cx->pin + off;
}

}  // namespace

int scde::host::upload_on(scde_ctx* cx, Buf& b, const void* src, size_t bytes, hipStream_t st) {
  HCHK(b.ensure(bytes));
  if (!bytes) return SCDE_OK;
  if (char* h = pin_alloc(cx, bytes)) {
    std::memcpy(h, src, bytes);
    src = h;
  }
  HCHK(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, st));
  return SCDE_OK;
}
int scde::host::upload(scde_ctx* cx, Buf& b, const void* src, size_t bytes) {
  return upload_on(cx, b, src, bytes, cx->stream);
}

namespace {
using UniqueSet = scde_ctx::UniqueSet;
}  // namespace

static std::mutex g_default_mu;
static scde_ctx* g_default = nullptr;

int scde::host::default_ctx(scde_ctx** out) {
  std::lock_guard<std::mutex> lk(g_default_mu);
  if (!g_default) {
    int dev = 0;
    if (const char* e = getenv("SCDE_DEVICE")) dev = atoi(e);
    if (const char* r = getenv("SCDE_RAND")) {
      if (!strcmp(r, "darwin")) g_rand_kind = SCDE_RAND_DARWIN;
      if (!strcmp(r, "glibc")) g_rand_kind = SCDE_RAND_GLIBC;
    }
    scde_ctx* c = nullptr;
    RCHK(scde_ctx_create(dev, &c));
    g_default = c;
  }
  *out = g_default;
  return SCDE_OK;
}

int scde::host::use_ctx(scde_ctx*& ctx) {
  if (!ctx) RCHK(default_ctx(&ctx));
  HCHK(hipSetDevice(ctx->device));
  return SCDE_OK;
}

std::vector<double> scde::host::marginals(const double* prior_x, int G) {
  // R/functions.R:575-577: log(pmax(10^x - 1, 0))
  std::vector<double> m(G);
  for (int k = 0; k < G; ++k) {
    double v = std::pow(10.0, prior_x[k]) - 1;
    if (v < 0) v = 0;
    m[k] = std::log(v);
  }
  return m;
}

namespace {

// colnames of the ratio posterior as numbers: seq(x1-xn, xn-x1, length = 2n-1)
// formatted with 15 significant digits and parsed back (R/functions.R:3506, 5040)
std::vector<double> ratio_diffv(const double* x, int n) {
  const int m = 2 * n - 1;
  std::vector<double> rv(m);
  const double from = x[0] - x[n - 1], to = x[n - 1] - x[0];
  const double by = (to - from) / (m - 1);
  for (int i = 0; i < m; ++i) rv[i] = from + (double)i * by;
  rv[0] = from;
  rv[m - 1] = to;
  for (int i = 0; i < m; ++i) {
    char buf[64];
    snprintf(buf, sizeof(buf), "%.15g", rv[i]);
    rv[i] = strtod(buf, nullptr);
  }
  return rv;
}

int expectation_index(const std::vector<double>& diffv, double expectation) {
  const double target = expectation / std::log2(10.0);
  int zi = 0;
  double best = INFINITY;
  for (int i = 0; i < (int)diffv.size(); ++i) {
    const double d = std::fabs(diffv[i] - target);
    if (d < best) {
      best = d;
      zi = i;
    }
  }
  return zi;
}

}  // namespace

// Reference seeding: one draw set per n.cores chunk overlapping this shard.
void scde::host::seeding(int n_cores, long long gene_offset, long long N_total, int ngenes, std::vector<int>& seeds,
             std::vector<int>& wset) {
  seeds.clear();
  wset.clear();
  if (!(n_cores > 1 && N_total > n_cores)) {
    seeds.push_back(1);
    return;
  }
  const std::vector<long long> st = r_chunk_starts(N_total, n_cores);
  wset.assign(ngenes, 0);
  int cur = -1;
  long long last_chunk = -1;
  for (int g = 0; g < ngenes; ++g) {
    const long long gg = gene_offset + g;
    const long long ch = std::upper_bound(st.begin(), st.end(), gg) - st.begin() - 1;
    if (ch != last_chunk) {
      seeds.push_back((int)(st[ch] + 1));
      last_chunk = ch;
      cur = (int)seeds.size() - 1;
    }
    wset[g] = cur;
  }
  if (seeds.size() == 1) wset.clear();
}

static void transpose_rows_to_colmajor(const double* rows, int N, int G, double* out) {
  for (int g = 0; g < N; ++g)
    for (int k = 0; k < G; ++k) out[(size_t)k * N + g] = rows[(size_t)g * G + k];
}

// =================================================================== C ABI
extern "C" {

const char* scde_last_error(void) { return g_err.c_str(); }

int scde_set_rand_kind(int kind) {
  if (kind != SCDE_RAND_GLIBC && kind != SCDE_RAND_DARWIN) return fail(SCDE_EARG, "unknown rand kind %d", kind);
  g_rand_kind = kind;
  return SCDE_OK;
}
int scde_get_rand_kind(void) { return g_rand_kind; }
int scde_version(void) { return 100; }

int scde_ctx_create(int device, scde_ctx** out) {
  FORK_GUARD();
  if (!out) return fail(SCDE_EARG, "null out");
  int n = 0;
  HCHK(hipGetDeviceCount(&n));
  if (n <= 0) return fail(SCDE_EHIP, "no HIP device");
  if (device < 0 || device >= n) return fail(SCDE_EARG, "device %d out of range (%d devices)", device, n);
  HCHK(hipSetDevice(device));
  auto* c = new scde_ctx();
  c->device = device;
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete c;
    return fail(SCDE_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
  }
  c->home_stream = c->stream;
  // SCDE_OPTIONS="name=value,name=value": context options from the environment (tuning runs)
  if (const char* env = std::getenv("SCDE_OPTIONS")) {
    std::string all(env);
    size_t pos = 0;
    while (pos < all.size()) {
      size_t end = all.find(',', pos);
      if (end == std::string::npos) end = all.size();
      const std::string item = all.substr(pos, end - pos);
      pos = end + 1;
      const size_t eq = item.find('=');
      if (item.empty()) continue;
      int rc = SCDE_OK;
      if (eq == std::string::npos) {
        rc = fail(SCDE_EARG, "SCDE_OPTIONS item '%s' is not name=value", item.c_str());
      } else {
        // the whole value must be a number ("lanes=abc" or "lanes=" fail instead of becoming 0)
        const char* vs = item.c_str() + eq + 1;
        char* vend = nullptr;
        errno = 0;
        const double v = std::strtod(vs, &vend);
        if (*vs == '\0' || vend == vs || *vend != '\0' || errno == ERANGE)
          rc = fail(SCDE_EARG, "SCDE_OPTIONS item '%s': value is not a number", item.c_str());
        else
          rc = scde_ctx_set_option(c, item.substr(0, eq).c_str(), v);
      }
      if (rc != SCDE_OK) {
        scde_ctx_destroy(c);
        return rc;
      }
    }
  }
  *out = c;
  return SCDE_OK;
}

void scde_ctx_destroy(scde_ctx* ctx) {
  if (fork_guard() != SCDE_OK) return;  // a forked child leaves the parent's context alone
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  {
    std::lock_guard<std::mutex> lk(g_default_mu);
    if (ctx == g_default) g_default = nullptr;
  }
  delete ctx;
}

int scde_ctx_synchronize(scde_ctx* ctx) {
  FORK_GUARD();
  if (!ctx) return fail(SCDE_EARG, "null ctx");
  HCHK(hipSetDevice(ctx->device));
  return ctx->sync();
}

int scde_ctx_set_profiling(scde_ctx* ctx, int on) {
  if (!ctx) return fail(SCDE_EARG, "null ctx");
  ctx->profile = on != 0;
  return SCDE_OK;
}

int scde_ctx_kernel_times(scde_ctx* ctx, double* ms, int64_t* launches, int nslots) {
  FORK_GUARD();
  if (!ctx) return fail(SCDE_EARG, "null ctx");
  RCHK(ctx->sync());
  for (int i = 0; i < nslots && i < NSLOTS; ++i) {
    if (ms) ms[i] = ctx->ms[i];
    if (launches) launches[i] = ctx->launches[i];
  }
  return SCDE_OK;
}

int scde_ctx_reset_kernel_times(scde_ctx* ctx) {
  FORK_GUARD();
  if (!ctx) return fail(SCDE_EARG, "null ctx");
  RCHK(ctx->sync());
  for (int i = 0; i < NSLOTS; ++i) {
    ctx->ms[i] = 0;
    ctx->launches[i] = 0;
  }
  return SCDE_OK;
}

int scde_ctx_set_option(scde_ctx* ctx, const char* name, double value) {
  if (!ctx || !name) return fail(SCDE_EARG, "null argument");
  const std::string n(name);
  if (n == "boot_skip") ctx->opt_boot_skip = value != 0;
  else if (n == "skip_slack") ctx->opt_skip_slack = value;
  else if (n == "boot_nb") ctx->opt_boot_nb = (int)value;
  else if (n == "skip_stats") ctx->opt_skip_stats = value != 0;
  else if (n == "wpca_ms") ctx->opt_wpca_ms = value != 0;
  else if (n == "boot_tiles") ctx->opt_boot_tiles = value != 0;
  else if (n == "boot_tiles_cells") ctx->opt_boot_tiles_cells = (int)value;
  else if (n == "tile_groups") ctx->opt_tile_groups = (int)value;
  else if (n == "tile_max_mult") ctx->opt_tile_max_mult = (int)value;
  else if (n == "tile_order") ctx->opt_tile_order = (value >= 1 && value <= 3) ? (int)value : 0;
  else if (n == "modes_overlap") ctx->opt_modes_overlap = value != 0;
  else if (n == "jp_chunks") ctx->opt_jp_chunks = std::max(1, std::min(64, (int)value));
  else if (n == "upload_u16") ctx->opt_upload_u16 = (value >= 0 && value <= 2) ? (int)value : 1;
  else if (n == "gene_list_cap") ctx->opt_gene_list_cap = std::max(0, (int)value);
  else if (n == "gene_rows") ctx->opt_gene_rows = std::max(1, std::min(4, (int)value));
  else if (n == "unique_fixed") ctx->opt_unique_fixed = value != 0;
  else if (n == "pipeline_mb") ctx->opt_pipeline_mb = value;
  else if (n == "pieces") ctx->opt_pieces = std::max(1, std::min((int)value, scde_ctx::kMaxPieces));
  else if (n == "tables_nt") ctx->opt_tables_nt = std::min(2, std::max(0, (int)value));
  else if (n == "lanes") {
    ctx->opt_lanes = value >= 2 ? 2 : 1;
    if (ctx->opt_lanes == 1 && ctx->peer) {  // one lane: the peer's workspace goes back to the device
      FORK_GUARD();
      HCHK(hipSetDevice(ctx->device));
      RCHK(ctx->sync());
      delete ctx->peer;
      ctx->peer = nullptr;
    }
  }
  else return fail(SCDE_EARG, "unknown option '%s'", name);
  return SCDE_OK;
}

int scde_ctx_inject_fault(scde_ctx* ctx, const char* where, int count) {
  if (!ctx || !where) return fail(SCDE_EARG, "null argument");
  if (std::string(where) == "u16_slot") ctx->fault_u16 = std::max(0, count);
  else if (std::string(where) == "handoff_spin") ctx->spin_cycles = std::max(0, count);
  else if (std::string(where) == "skip_lane_join") ctx->fault_skip_join = std::max(0, count);
  else return fail(SCDE_EARG, "unknown fault point '%s'", where);
  return SCDE_OK;
}

int scde_ctx_get_stat(scde_ctx* ctx, const char* name, double* value) {
  if (!ctx || !name || !value) return fail(SCDE_EARG, "null argument");
  const std::string n(name);
  if (n == "skip_slabs") *value = ctx->st_skip_slabs;
  else if (n == "skip_stretches") *value = ctx->st_skip_stretches;
  else if (n == "skip_kept") *value = ctx->st_skip_kept;
  else if (n == "boot_f64_fma") *value = ctx->st_boot_f64_fma;
  else if (n == "boot_path") *value = ctx->st_boot_path;
  else if (n == "ratio_n_max") *value = ratio_n_max();  // constants: the largest n of the ratio entries,
  else if (n == "ratio_n_lds64") *value = ratio_n_default_lds();  // and the largest within 64 KiB of LDS
  else if (n == "skip_redo") *value = ctx->st_skip_redo;
  else if (n == "pair_redo") *value = ctx->st_pair_redo;
  else if (n == "degen") *value = ctx->st_degen;
  else if (n == "olo_launches") *value = ctx->st_olo[0];
  else if (n == "olo_candidates") *value = ctx->st_olo[1];
  else if (n == "stream_syncs") *value = ctx->st_stream_syncs + (ctx->peer ? ctx->peer->st_stream_syncs : 0);
  else if (n == "arena_syncs") *value = ctx->st_arena_syncs + (ctx->peer ? ctx->peer->st_arena_syncs : 0);
  else if (n == "piece_wait_ms") *value = ctx->st_piece_wait_ms + (ctx->peer ? ctx->peer->st_piece_wait_ms : 0);
  else if (n == "piece_host_ms") *value = ctx->st_piece_host_ms + (ctx->peer ? ctx->peer->st_piece_host_ms : 0);
  else if (n == "buf_reallocs") *value = (double)g_buf_reallocs.load();
  else if (n == "handoff_spins") *value = (double)(ctx->st_spins.load() + (ctx->peer ? ctx->peer->st_spins.load() : 0));
  // (the upload worker and the 16-bit issuer update these under their mutexes)
  else if (n == "upload_wake_ms" || n == "upload_first_ms") {
    std::lock_guard<std::mutex> lk(ctx->upl.m);
    *value = n == "upload_wake_ms" ? ctx->upl.wake_ms : ctx->upl.first_ms;
  } else if (n == "u16_wait_ms" || n == "u16_issue_ms" || n == "u16_free_ms") {
    std::lock_guard<std::mutex> lk(ctx->u16.m);
    *value = n == "u16_wait_ms" ? ctx->u16.st_wait_ms : n == "u16_issue_ms" ? ctx->u16.st_issue_ms : ctx->u16.st_free_ms;
  }
  else if (n == "host_setup_ms") *value = ctx->st_host_ms[0];
  else if (n == "host_unique_ms") *value = ctx->st_host_ms[1];
  else if (n == "host_post_ms") *value = ctx->st_host_ms[2];
  else if (n == "host_tail_ms") *value = ctx->st_host_ms[3];
  else if (n.rfind("tiles_", 0) == 0 && atoi(n.c_str() + 6) >= 0 && atoi(n.c_str() + 6) <= 28)
    *value = ctx->st_tile_hist[atoi(n.c_str() + 6)];
  else return fail(SCDE_EARG, "unknown statistic '%s'", name);
  return SCDE_OK;
}

int scde_ctx_reset_stats(scde_ctx* ctx) {
  if (!ctx) return fail(SCDE_EARG, "null argument");
  ctx->st_skip_slabs = ctx->st_skip_kept = ctx->st_skip_stretches = ctx->st_skip_redo = ctx->st_degen = 0;
  ctx->st_pair_redo = 0;
  ctx->st_stream_syncs = ctx->st_arena_syncs = 0;
  if (ctx->peer) ctx->peer->st_stream_syncs = ctx->peer->st_arena_syncs = 0;
  ctx->st_piece_wait_ms = ctx->st_piece_host_ms = 0;
  if (ctx->peer) ctx->peer->st_piece_wait_ms = ctx->peer->st_piece_host_ms = 0;
  for (double& x : ctx->st_host_ms) x = 0;
  {
    std::lock_guard<std::mutex> lk(ctx->upl.m);
    ctx->upl.wake_ms = ctx->upl.first_ms = 0;
  }
  {
    std::lock_guard<std::mutex> lk(ctx->u16.m);
    ctx->u16.st_wait_ms = ctx->u16.st_issue_ms = ctx->u16.st_free_ms = 0;
  }
  ctx->st_boot_f64_fma = 0;
  ctx->st_spins = 0;
  if (ctx->peer) ctx->peer->st_spins = 0;
  for (double& x : ctx->st_tile_hist) x = 0;
  return SCDE_OK;
}

int scde_dev_alloc(scde_ctx* ctx, int64_t bytes, void** dptr) {
  FORK_GUARD();
  if (!ctx || !dptr || bytes < 0) return fail(SCDE_EARG, "bad args");
  HCHK(hipSetDevice(ctx->device));
  HCHK(hipMalloc(dptr, std::max<int64_t>(bytes, 1)));
  ctx->user_allocs.push_back(*dptr);
  return SCDE_OK;
}

int scde_dev_free(scde_ctx* ctx, void* dptr) {
  FORK_GUARD();
  if (!ctx) return fail(SCDE_EARG, "null ctx");
  auto it = std::find(ctx->user_allocs.begin(), ctx->user_allocs.end(), dptr);
  if (it == ctx->user_allocs.end()) return fail(SCDE_EARG, "pointer not owned by this context");
  ctx->user_allocs.erase(it);
  HCHK(hipFree(dptr));
  return SCDE_OK;
}

int scde_h2d(scde_ctx* ctx, void* dst, const void* src, int64_t bytes) {
  FORK_GUARD();
  if (!ctx) return fail(SCDE_EARG, "null ctx");
  HCHK(hipSetDevice(ctx->device));
  HCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
  return ctx->sync();
}

int scde_d2h(scde_ctx* ctx, void* dst, const void* src, int64_t bytes) {
  FORK_GUARD();
  if (!ctx) return fail(SCDE_EARG, "null ctx");
  HCHK(hipSetDevice(ctx->device));
  HCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
  return ctx->sync();
}

// ------------------------------------------------------------------ layer 1
// The posterior-mode matrix (ngenes x ncells doubles: 480 MB at config 4) to the host on the
// copy stream, after run_posterior's modes_ev: issued once every kernel of the call is queued
// (a pageable read-back can hold the host thread until it is done), it overlaps the bootstrap.
static int copy_modes_out(scde_ctx* cx, double* host, const double* dev, size_t n) {
  if (!cx->copy_stream) HCHK(hipStreamCreateWithFlags(&cx->copy_stream, hipStreamNonBlocking));
  HCHK(handoff_wait(cx, cx->copy_stream, cx->modes_ev));
  HCHK(hipMemcpyAsync(host, dev, sizeof(double) * n, hipMemcpyDeviceToHost, cx->copy_stream));
  return SCDE_OK;
}

static int logboot_common(scde_ctx* cx, bool batch, const double* models, int ncells, const int* ucl_vals, const int64_t* ucl_off,
                          const int* counti, int ngenes, const double* magnitudes, int ngrid, const int* batch_vals,
                          const int64_t* batch_off, const int* composition, int nbatch, int nboot, int seed,
                          int return_post, int local_theta, int square_logit_conc, int ensemble, double* jp,
                          double* modes, double* post) {
  if (!models || !ucl_vals || !ucl_off || !counti || !magnitudes || !jp)
    return fail(SCDE_EARG, "null input pointer");
  if (ncells <= 0 || ngenes < 0 || ngrid <= 0) return fail(SCDE_EARG, "bad dimensions");
  if (batch) {
    for (int k = 0; k < nbatch; ++k) {
      if (composition[k] > 0 && batch_off[k + 1] - batch_off[k] <= 0)
        return fail(SCDE_EARG, "batch %d has draws but no cells", k);
      for (int64_t i = batch_off[k]; i < batch_off[k + 1]; ++i)
        if (batch_vals[i] < 0 || batch_vals[i] >= ncells) return fail(SCDE_EARG, "BatchIL index out of range");
    }
  }
  RCHK(use_ctx(cx));
  const size_t NG = (size_t)ngenes * ngrid;
  PostSpec s;
  s.ncells = ncells;
  s.models = models;
  s.localtheta = local_theta;
  s.squarelogit = square_logit_conc;
  s.mag = magnitudes;
  s.G = ngrid;
  s.nboot = nboot;
  s.postflag = return_post;
  s.ensemble = batch ? 0 : ensemble;
  s.batch_call = batch;
  s.ucl_host = ucl_vals;
  s.ucl_off_host = ucl_off;
  s.uci_host = counti;
  s.ngenes = ngenes;
  s.seeds = {seed};
  s.rand_kind = g_rand_kind;
  s.batch_vals = batch_vals;
  s.batch_off = batch_off;
  s.comp = composition;
  s.nbatch = nbatch;
  const bool want_modes = (batch ? return_post == 1 : (return_post == 1 || return_post == 3)) && modes;
  const bool want_post = (batch ? return_post == 2 : (return_post == 2 || return_post == 3)) && post;
  HCHK(cx->jpA.ensure(sizeof(double) * std::max<size_t>(1, NG)));
  s.jp = cx->jpA.as<double>();
  s.jp_g = 1;  // R layout: ngenes x ngrid column-major
  s.jp_k = ngenes;
  if (want_modes) {
    HCHK(cx->jpB.ensure(sizeof(double) * std::max<size_t>(1, (size_t)ngenes * ncells)));
    s.modes = cx->jpB.as<double>();
    s.modes_early = ngenes > 0;
  }
  if (want_post) {
    HCHK(cx->outbuf.ensure(sizeof(double) * std::max<size_t>(1, NG * ncells)));
    s.post = cx->outbuf.as<double>();
  }
  cx->us[0].ready = false;
  RCHK(run_posterior(cx, s, cx->us[0]));
  if (s.modes_early) RCHK(copy_modes_out(cx, modes, s.modes, (size_t)ngenes * ncells));
  if (NG) HCHK(hipMemcpyAsync(jp, s.jp, sizeof(double) * NG, hipMemcpyDeviceToHost, cx->stream));
  if (want_post && NG)
    HCHK(hipMemcpyAsync(post, s.post, sizeof(double) * NG * ncells, hipMemcpyDeviceToHost, cx->stream));
  if (s.modes_early) HCHK(hipStreamSynchronize(cx->copy_stream));
  return cx->sync();
}

int scde_logBootPosterior(const double* models, int ncells, const int* ucl_vals, const int64_t* ucl_off,
                          const int* counti, int ngenes, const double* magnitudes, int ngrid, int nboot, int seed,
                          int return_post, int local_theta, int square_logit_conc, int ensemble, double* jp,
                          double* modes, double* post) {
  FORK_GUARD();
  return logboot_common(nullptr, false, models, ncells, ucl_vals, ucl_off, counti, ngenes, magnitudes, ngrid, nullptr,
                        nullptr, nullptr, 0, nboot, seed, return_post, local_theta, square_logit_conc, ensemble, jp,
                        modes, post);
}

int scde_logBootPosterior_ctx(scde_ctx* ctx, const double* models, int ncells, const int* ucl_vals,
                              const int64_t* ucl_off, const int* counti, int ngenes, const double* magnitudes,
                              int ngrid, int nboot, int seed, int return_post, int local_theta,
                              int square_logit_conc, int ensemble, double* jp, double* modes, double* post) {
  FORK_GUARD();
  return logboot_common(ctx, false, models, ncells, ucl_vals, ucl_off, counti, ngenes, magnitudes, ngrid, nullptr,
                        nullptr, nullptr, 0, nboot, seed, return_post, local_theta, square_logit_conc, ensemble, jp,
                        modes, post);
}

int scde_logBootBatchPosterior(const double* models, int ncells, const int* ucl_vals, const int64_t* ucl_off,
                               const int* counti, int ngenes, const double* magnitudes, int ngrid,
                               const int* batch_vals, const int64_t* batch_off, const int* composition, int nbatch,
                               int nboot, int seed, int return_post, int local_theta, int square_logit_conc,
                               double* jp, double* modes, double* post) {
  FORK_GUARD();
  if (!batch_vals || !batch_off || !composition) return fail(SCDE_EARG, "null batch input");
  return logboot_common(nullptr, true, models, ncells, ucl_vals, ucl_off, counti, ngenes, magnitudes, ngrid, batch_vals,
                        batch_off, composition, nbatch, nboot, seed, return_post, local_theta, square_logit_conc, 0,
                        jp, modes, post);
}

// jpmat*: the matrices are the "cells", their rows the "genes", their columns the grid.
static int jpmat_common(const double* const* mats, int nmat, const int* type_off, const int* comp, int ntypes,
                        int nrows, int ncols, int nboot, int seed, double* out) {
  if (!mats || !out || nmat <= 0 || nrows < 0 || ncols <= 0) return fail(SCDE_EARG, "bad jpmat arguments");
  if (ncols > 4096) return fail(SCDE_EARG, "ncols > 4096 unsupported");
  scde_ctx* cx = nullptr;
  RCHK(use_ctx(cx));
  hipStream_t st = cx->stream;
  const int GS = (int)round_up(ncols, 16);
  const size_t per = (size_t)nrows * ncols;
  // stage matrices as row-major tables: column (m, r) = m * nrows + r
  HCHK(cx->T.ensure(sizeof(double) * std::max<size_t>(1, (size_t)nmat * nrows * GS)));
  HCHK(cx->in1.ensure(sizeof(double) * std::max<size_t>(1, per)));
  for (int m = 0; m < nmat; ++m) {
    HCHK(hipMemcpyAsync(cx->in1.p, mats[m], sizeof(double) * per, hipMemcpyHostToDevice, st));
    HCHK(launch_colmajor_to_rows(cx->in1.as<double>(), nrows, ncols, GS, cx->T.as<double>() + (size_t)m * nrows * GS,
                                 st));
  }
  // draws
  const int Bp = (int)round_up(std::max(nboot, 1), 16);
  int ndraw = 0;
  std::vector<int> draws;
  std::vector<double> W((size_t)nmat * Bp, 0.0);
  PlatformRand rng((unsigned int)seed, g_rand_kind);
  if (!type_off) {
    ndraw = nmat;
    draws.resize((size_t)std::max(nboot, 1) * ndraw);
    for (int b = 0; b < nboot; ++b)
      for (int j = 0; j < nmat; ++j) {
        const int rj = rng.draw(nmat);
        draws[(size_t)b * ndraw + j] = rj;
        W[(size_t)rj * Bp + b] += 1.0;
      }
  } else {
    for (int k = 0; k < ntypes; ++k) {
      ndraw += std::max(0, comp[k]);
      if (comp[k] > 0 && type_off[k + 1] - type_off[k] <= 0) return fail(SCDE_EARG, "type %d has no matrices", k);
    }
    draws.resize((size_t)std::max(nboot, 1) * std::max(ndraw, 1));
    for (int b = 0; b < nboot; ++b) {
      int d = 0;
      for (int k = 0; k < ntypes; ++k)
        for (int j = 0; j < comp[k]; ++j) {
          const int m = type_off[k] + rng.draw(type_off[k + 1] - type_off[k]);
          draws[(size_t)b * ndraw + d++] = m;
          W[(size_t)m * Bp + b] += 1.0;
        }
    }
  }
  // every row takes every matrix (no baseline)
  std::vector<int2> ent((size_t)std::max(1, nrows) * nmat);
  for (int r = 0; r < nrows; ++r)
    for (int m = 0; m < nmat; ++m) ent[(size_t)r * nmat + m] = make_int2(m, m * nrows + r);
  std::vector<int> nnz(std::max(1, nrows), nmat);
  RCHK(upload(cx, cx->ent, ent.data(), sizeof(int2) * ent.size()));
  RCHK(upload(cx, cx->nnz, nnz.data(), sizeof(int) * nnz.size()));
  RCHK(upload(cx, cx->Wt, W.data(), sizeof(double) * W.size()));
  RCHK(upload(cx, cx->draws, draws.data(), sizeof(int) * draws.size()));
  HCHK(cx->degen.ensure(sizeof(int) * std::max(1, nrows)));
  HCHK(hipMemsetAsync(cx->degen.p, 0, sizeof(int) * std::max(1, nrows), st));
  HCHK(cx->jpA.ensure(sizeof(double) * std::max<size_t>(1, per)));
  if (nboot == 0) {
    HCHK(hipMemsetAsync(cx->jpA.p, 0, sizeof(double) * std::max<size_t>(1, per), st));
  } else {
    BootArgs ba{};
    ba.T = cx->T.as<double>();
    ba.G = ncols;
    ba.GS = GS;
    ba.ent = cx->ent.as<int2>();
    ba.nnz = cx->nnz.as<int>();
    ba.ent_stride = nmat;
    ba.base_col = nullptr;
    ba.Wt = cx->Wt.as<double>();
    ba.ncells = nmat;
    ba.Bp = Bp;
    ba.nboot = nboot;
    ba.wset = nullptr;
    ba.Z = nullptr;
    ba.norm_mult = 1.0;  // jpmat* do not divide by nboot (src/jpmatLogBoot.cpp:36-38)
    ba.degen_thresh = 16777216.0;
    ba.out = cx->jpA.as<double>();
    ba.out_g = 1;
    ba.out_k = nrows;
    ba.degen = cx->degen.as<int>();
    ba.ngenes = nrows;
    hipEvent_t ev = cx->mark_begin(SLOT_BOOT);
    HCHK(launch_boot(ba, st));
    cx->mark_end(SLOT_BOOT, ev);
    ExactArgs xa{};
    xa.T = ba.T;
    xa.G = ncols;
    xa.GS = GS;
    xa.draws = cx->draws.as<int>();
    xa.ndraw = ndraw;
    xa.nboot = nboot;
    xa.wset = nullptr;
    xa.ucl_off = nullptr;
    xa.uci = nullptr;
    xa.ld_uci = 0;
    xa.norm_mult = 1.0;
    xa.degen = ba.degen;
    xa.out = ba.out;
    xa.out_g = 1;
    xa.out_k = nrows;
    xa.ngenes = nrows;
    HCHK(launch_boot_exact(xa, st));
  }
  if (per) HCHK(hipMemcpyAsync(out, cx->jpA.p, sizeof(double) * per, hipMemcpyDeviceToHost, st));
  return cx->sync();
}

int scde_jpmatLogBoot(const double* const* mats, int nmat, int nrows, int ncols, int nboot, int seed, double* out) {
  FORK_GUARD();
  return jpmat_common(mats, nmat, nullptr, nullptr, 0, nrows, ncols, nboot, seed, out);
}

int scde_jpmatLogBatchBoot(const double* const* mats, const int* type_off, const int* comp, int ntypes, int nrows,
                           int ncols, int nboot, int seed, double* out) {
  FORK_GUARD();
  if (!type_off || !comp || ntypes <= 0) return fail(SCDE_EARG, "bad jpmatLogBatchBoot arguments");
  return jpmat_common(mats, type_off[ntypes], type_off, comp, ntypes, nrows, ncols, nboot, seed, out);
}

// k_ratio_summary holds a gene's rows and outputs in LDS: n above ratio_n_max() cannot be launched
static int ratio_n_check(const char* who, int n) {
  if (n > ratio_n_max())
    return fail(SCDE_EARG, "%s: n = %d grid points; the ratio posterior supports at most n = %d", who, n, ratio_n_max());
  return SCDE_OK;
}

static int ratio_common(const double* pmat1, const double* pmat2, int nrows, int n, const double* prior_y,
                        const double* diffv, int zi, int normalize, double* ratio, double* res) {
  if (!pmat1 || !pmat2 || nrows < 0 || n <= 0) return fail(SCDE_EARG, "bad ratio arguments");
  if (res && (!diffv || zi < 0 || zi >= 2 * n - 1)) return fail(SCDE_EARG, "bad diffv/zi");
  RCHK(ratio_n_check(normalize ? "scde_ratio_summary" : "scde_matSlideMult", n));
  scde_ctx* cx = nullptr;
  RCHK(use_ctx(cx));
  hipStream_t st = cx->stream;
  const size_t per = (size_t)nrows * n, m = 2 * (size_t)n - 1;
  RCHK(upload(cx, cx->in1, pmat1, sizeof(double) * std::max<size_t>(1, per)));
  RCHK(upload(cx, cx->in2, pmat2, sizeof(double) * std::max<size_t>(1, per)));
  if (prior_y) RCHK(upload(cx, cx->prior_y, prior_y, sizeof(double) * n));
  if (res) RCHK(upload(cx, cx->diffv, diffv, sizeof(double) * m));
  HCHK(cx->ratio.ensure(sizeof(double) * std::max<size_t>(1, nrows * m)));
  HCHK(cx->res.ensure(sizeof(double) * std::max<size_t>(1, (size_t)nrows * 5)));
  RatioArgs ra{};
  ra.jp1 = cx->in1.as<double>();
  ra.j1g = 1;
  ra.j1k = nrows;
  ra.jp2 = cx->in2.as<double>();
  ra.j2g = 1;
  ra.j2k = nrows;
  ra.prior_y = prior_y ? cx->prior_y.as<double>() : nullptr;
  ra.n = n;
  ra.ngenes = nrows;
  ra.normalize = normalize;
  ra.ratio = cx->ratio.as<double>();
  ra.rg = 1;
  ra.ro = nrows;
  ra.diffv = res ? cx->diffv.as<double>() : nullptr;
  ra.zi = zi;
  ra.res = res ? cx->res.as<double>() : nullptr;
  ra.res_ld = nrows;
  hipEvent_t ev = cx->mark_begin(SLOT_RATIO);
  HCHK(launch_ratio_summary(ra, st));
  cx->mark_end(SLOT_RATIO, ev);
  if (ratio && nrows) HCHK(hipMemcpyAsync(ratio, ra.ratio, sizeof(double) * nrows * m, hipMemcpyDeviceToHost, st));
  if (res && nrows) HCHK(hipMemcpyAsync(res, ra.res, sizeof(double) * nrows * 5, hipMemcpyDeviceToHost, st));
  return cx->sync();
}

int scde_distribution_summary(const double* rpost, int nrows, int m, const double* diffv, int zi, double* res) {
  FORK_GUARD();
  if (!rpost || !diffv || !res || nrows < 0 || m < 1 || (m % 2) == 0) return fail(SCDE_EARG, "bad summary arguments");
  if (zi < 0 || zi >= m) return fail(SCDE_EARG, "zi out of range");
  RCHK(ratio_n_check("scde_distribution_summary", (m + 1) / 2));
  scde_ctx* cx = nullptr;
  RCHK(use_ctx(cx));
  hipStream_t st = cx->stream;
  const int n = (m + 1) / 2;
  RCHK(upload(cx, cx->in1, rpost, sizeof(double) * std::max<size_t>(1, (size_t)nrows * m)));
  RCHK(upload(cx, cx->diffv, diffv, sizeof(double) * m));
  HCHK(cx->res.ensure(sizeof(double) * std::max<size_t>(1, (size_t)nrows * 5)));
  RatioArgs ra{};
  ra.n = n;
  ra.ngenes = nrows;
  ra.xin = cx->in1.as<double>();
  ra.xg = 1;
  ra.xo = nrows;
  ra.diffv = cx->diffv.as<double>();
  ra.zi = zi;
  ra.res = cx->res.as<double>();
  ra.res_ld = nrows;
  HCHK(launch_ratio_summary(ra, st));
  if (nrows) HCHK(hipMemcpyAsync(res, ra.res, sizeof(double) * nrows * 5, hipMemcpyDeviceToHost, st));
  return cx->sync();
}

int scde_matSlideMult(const double* m1, const double* m2, int nrows, int ncols, double* out) {
  FORK_GUARD();
  if (!out) return fail(SCDE_EARG, "null out");
  return ratio_common(m1, m2, nrows, ncols, nullptr, nullptr, 0, 0, out, nullptr);
}

int scde_ratio_summary(const double* pmat1, const double* pmat2, int nrows, int n, const double* prior_y,
                       const double* diffv, int zi, double* ratio, double* res) {
  FORK_GUARD();
  return ratio_common(pmat1, pmat2, nrows, n, prior_y, diffv, zi, 1, ratio, res);
}

// ------------------------------------------------------------------ layer 2
// Host counts of a host-count entry (de_run: the first group's range in pieces, then the
// second group's range; posteriors_run: the selected cells in pieces), copied on the context's
// copy stream by an UploadWorker.
struct HostUpload {
  const int* counts;
  int64_t ld;
  int ngenes, cut, C;
  bool u16 = false;  // ranges of >= 8 MB as 16-bit counts (upload_cols_u16)
};
// narrow n int32 counts to uint16, appending the counts outside [0, 65535] (negative ones
// included) to `exc` as (i0 + index, count): blocks of 256 narrowed by a vectorised loop, a
// block whose high halves are not all zero scanned again
// The block loop, compiled twice: for the baseline x86-64 target and for AVX2 (8 counts per
// instruction; chosen at run time when the CPU has it).  Returns the OR of the block's high halves.
static inline unsigned narrow_block(const int* s, unsigned short* d, size_t b0, size_t e) {
  unsigned b = 0;
  for (size_t i = b0; i < e; ++i) {
    const unsigned v = (unsigned)s[i];
    b |= v >> 16;
    d[i] = (unsigned short)v;
  }
  return b;
}
__attribute__((target("avx2"))) static unsigned narrow_block_avx2(const int* s, unsigned short* d, size_t b0,
                                                                   size_t e) {
  unsigned b = 0;
  for (size_t i = b0; i < e; ++i) {
    const unsigned v = (unsigned)s[i];
    b |= v >> 16;
    d[i] = (unsigned short)v;
  }
  return b;
}
static const bool g_have_avx2 = __builtin_cpu_supports("avx2");

static void narrow16(const int* s, unsigned short* d, size_t n, int i0, std::vector<int2>& exc) {
  for (size_t b0 = 0; b0 < n; b0 += 256) {
    const size_t e = std::min(n, b0 + 256);
    const unsigned b = g_have_avx2 ? narrow_block_avx2(s, d, b0, e) : narrow_block(s, d, b0, e);
    if (b)
      for (size_t i = b0; i < e; ++i)
        if ((unsigned)s[i] >> 16) exc.push_back(make_int2(i0 + (int)i, s[i]));
  }
}

// the narrowing pool's thread t: per job, its share of every slot, in sequence order
static void u16_thread(scde_ctx* ctx, int t) {
  auto& r = ctx->u16;
  using R = scde_ctx::U16Ring;
  long long seen = 0;
  std::unique_lock<std::mutex> lk(r.m);
  for (;;) {
    r.cv.wait(lk, [&] { return r.stop || r.job != seen; });
    if (r.stop) return;
    seen = r.job;
    const int* src = r.src;
    const size_t n = r.n;
    const long long q0 = r.q0;
    const int nslots = r.nslots, T = r.T;
    for (int sl = 0; sl < nslots; ++sl) {
      const long long q = q0 + sl;
      r.cv.wait(lk, [&] { return r.free_upto > q || r.abort; });
      if (r.abort) break;
      lk.unlock();
      const int k = (int)(q % R::kRing);
      const size_t off = (size_t)sl * R::kSlotCounts;
      const size_t m = std::min(R::kSlotCounts, n - off);
      const size_t a = (m * t / T) & ~size_t(15), e = (t + 1 == T) ? m : ((m * (t + 1) / T) & ~size_t(15));
      r.exc[k][t].clear();
      if (e > a) narrow16(src + off + a, r.pin + (size_t)k * R::kSlotCounts + a, e - a, (int)a, r.exc[k][t]);
      lk.lock();
      if (++r.fin[k] == T) r.cvf.notify_all();
    }
    if (--r.busy == 0) r.cvd.notify_all();
  }
}

// columns [lo, hi) of contiguous host counts as 16-bit counts through U16Ring, widened (and the
// counts outside [0, 65535] patched in) on the copy stream
static int upload_cols_u16(scde_ctx* ctx, const HostUpload& h, int lo, int hi) {
  auto& r = ctx->u16;
  using R = scde_ctx::U16Ring;
  if (!r.pin) {
    HCHK(hipHostMalloc(reinterpret_cast<void**>(&r.pin), sizeof(unsigned short) * R::kRing * R::kSlotCounts,
                       hipHostMallocDefault));
    HCHK(hipMalloc(reinterpret_cast<void**>(&r.dev), sizeof(unsigned short) * R::kRing * R::kSlotCounts));
    for (auto& e : r.ev) HCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming | hipEventBlockingSync));
  }
  static_assert(R::kThreads >= 1 && R::kThreads <= R::kMaxT, "the pool's per-thread lists");
  const int T = R::kThreads;
  if ((int)r.th.size() != T) {  // (re)build the pool (no job is running: the upload worker is its only user)
    if (!r.th.empty()) {
      {
        std::lock_guard<std::mutex> lk(r.m);
        r.stop = true;
      }
      r.cv.notify_all();
      for (auto& t : r.th) t.join();
      r.th.clear();
      r.stop = false;
    }
    {
      std::lock_guard<std::mutex> lk(r.m);
      r.T = T;
    }
    for (int t = 0; t < T; ++t) r.th.emplace_back(u16_thread, ctx, t);
  }
  const size_t n = (size_t)h.ngenes * (size_t)(hi - lo);
  const int* src = h.counts + (size_t)h.ld * lo;
  int* dst = static_cast<int*>(ctx->counts_in.p) + (size_t)h.ngenes * lo;
  const int nslots = (int)((n + R::kSlotCounts - 1) / R::kSlotCounts);
  const long long q0 = r.seq;
  std::unique_lock<std::mutex> lk(r.m);
  r.src = src;
  r.n = n;
  r.q0 = q0;
  r.nslots = nslots;
  r.abort = false;
  r.busy = T;
  ++r.job;
  r.cv.notify_all();
  int rc = SCDE_OK;
  // (the statistics are summed under r.m, where scde_ctx_get_stat reads them)
  double wait_ms = 0, issue_ms = 0, free_ms = 0;
  for (int sl = 0; sl < nslots; ++sl) {
    const long long q = q0 + sl;
    const int k = (int)(q % R::kRing);
    const auto tw = std::chrono::steady_clock::now();
    r.cvf.wait(lk, [&] { return r.fin[k] == T; });
    r.fin[k] = 0;
    lk.unlock();
    const auto ti = std::chrono::steady_clock::now();
    wait_ms += std::chrono::duration<double, std::milli>(ti - tw).count();
    const size_t off = (size_t)sl * R::kSlotCounts;
    const size_t m = std::min(R::kSlotCounts, n - off);
    unsigned short* dslot = r.dev + (size_t)k * R::kSlotCounts;
    hipError_t e = hipMemcpyAsync(dslot, r.pin + (size_t)k * R::kSlotCounts, sizeof(unsigned short) * m,
                                  hipMemcpyHostToDevice, ctx->copy_stream);
    if (e == hipSuccess && ctx->fault_u16 > 0 && sl == std::min(1, nslots - 1)) {  // test hook (scde_ctx_inject_fault)
      --ctx->fault_u16;
      e = hipErrorUnknown;
    }
    if (e == hipSuccess) e = handoff_spin(ctx, ctx->copy_stream);
    if (e == hipSuccess) e = hipEventRecord(r.ev[k], ctx->copy_stream);
    if (e == hipSuccess) e = launch_widen16(dslot, dst + off, m, ctx->copy_stream);
    // the slot's counts outside 16 bits (the threads' lists of ring slot k are complete and
    // untouched until the slot is freed again below)
    r.exc_all.clear();
    for (int t = 0; t < T; ++t) r.exc_all.insert(r.exc_all.end(), r.exc[k][t].begin(), r.exc[k][t].end());
    if (e == hipSuccess && !r.exc_all.empty()) {
      // (a pageable copy has read the host list when it returns; the patch follows it in stream order)
      e = ctx->excd.ensure(sizeof(int2) * std::max<size_t>(r.exc_all.size(), 65536));
      if (e == hipSuccess)
        e = hipMemcpyAsync(ctx->excd.p, r.exc_all.data(), sizeof(int2) * r.exc_all.size(), hipMemcpyHostToDevice,
                           ctx->copy_stream);
      if (e == hipSuccess) e = launch_patch32(ctx->excd.as<int2>(), r.exc_all.size(), dst + off, ctx->copy_stream);
    }
    r.issued = q + 1;
    const auto tf = std::chrono::steady_clock::now();
    issue_ms += std::chrono::duration<double, std::milli>(tf - ti).count();
    // free the ring slot the threads need next (slot q + 1 reuses slot q + 1 - kRing's): wait for
    // that DMA, then let them write (only this thread writes free_upto)
    const long long f = q + 1 - R::kRing;
    const bool advance = e == hipSuccess && r.free_upto <= q + 1;
    if (advance && f >= 0) e = hipEventSynchronize(r.ev[f % R::kRing]);
    free_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf).count();
    lk.lock();
    if (e != hipSuccess) {
      rc = fail(SCDE_EHIP, "%s", hipGetErrorString(e));
      break;
    }
    if (advance) {
      r.free_upto = q + 2;
      r.cv.notify_all();
    }
  }
  if (rc != SCDE_OK) {
    r.abort = true;
    r.cv.notify_all();
  }
  r.cvd.wait(lk, [&] { return r.busy == 0; });
  for (auto& f : r.fin) f = 0;  // (an aborted job leaves partial counts)
  r.seq = r.issued;             // sequence numbers of slots never issued are reused
  r.st_wait_ms += wait_ms;
  r.st_issue_ms += issue_ms;
  r.st_free_ms += free_ms;
  if (rc != SCDE_OK) {
    // an error after slots were issued: free_upto may lag behind seq, and the next job's threads
    // would wait for a slot nobody frees.  Drain the copy stream -- every issued slot's DMA has then
    // finished (or failed) -- and open the whole ring to the next job.
    lk.unlock();
    (void)hipStreamSynchronize(ctx->copy_stream);
    (void)hipGetLastError();
    lk.lock();
    r.free_upto = r.seq + R::kRing;
  }
  lk.unlock();
  return rc;
}

// columns [lo, hi) of the host counts into counts_in, on the copy stream
static int upload_cols(scde_ctx* ctx, const HostUpload& h, int lo, int hi) {
  const size_t row = sizeof(int) * (size_t)h.ngenes;
  if (hi > lo && h.u16 && h.ld == h.ngenes && row * (size_t)(hi - lo) >= (size_t(8) << 20))
    return upload_cols_u16(ctx, h, lo, hi);
  if (hi > lo) {
    char* dst = static_cast<char*>(ctx->counts_in.p) + row * lo;
    const int* src = h.counts + (size_t)h.ld * lo;
    if (h.ld == h.ngenes)
      HCHK(hipMemcpyAsync(dst, src, row * (hi - lo), hipMemcpyHostToDevice, ctx->copy_stream));
    else
      HCHK(hipMemcpy2DAsync(dst, row, src, sizeof(int) * (size_t)h.ld, row, hi - lo, hipMemcpyHostToDevice,
                            ctx->copy_stream));
  }
  return SCDE_OK;
}

// The host-count uploads of one call, issued back to back from a worker thread: a pageable
// copy blocks its calling thread for the whole transfer, so issued from the caller's thread
// each piece would wait for the previous piece's unique-set build (a host sync) and PCIe would
// sit idle in between.  Column ranges [cols[j], cols[j+1]) go up on the copy stream in order,
// each followed by evs[j]; wait(n) returns once the first n are issued (their events recorded).
struct UploadWorker {
  scde_ctx* ctx = nullptr;
  int start(scde_ctx* c, const HostUpload& h, const std::vector<int>& cols, std::vector<hipEvent_t> evs) {
    if (cols.size() != evs.size() + 1)
      return fail(SCDE_EINTERNAL, "upload ranges: %d bounds for %d events", (int)cols.size(), (int)evs.size());
    std::vector<std::pair<int, int>> ranges;
    for (size_t j = 0; j + 1 < cols.size(); ++j) ranges.emplace_back(cols[j], cols[j + 1]);
    return start(c, h, std::move(ranges), std::move(evs));
  }
  // ranges[j] = [lo, hi) in any order (the interleaved two-group upload)
  int start(scde_ctx* c, const HostUpload& h, std::vector<std::pair<int, int>> ranges, std::vector<hipEvent_t> evs) {
    ctx = c;
    auto& u = c->upl;
    if (!u.th.joinable()) {
      u.th = std::thread([c] {
        auto& q = c->upl;
        (void)hipSetDevice(c->device);
        long long seen = 0;
        std::unique_lock<std::mutex> lk(q.m);
        for (;;) {
          q.cv.wait(lk, [&] { return q.stop || q.job != seen; });
          if (q.stop) return;
          seen = q.job;
          const int n = q.nranges;
          auto issue = q.issue;
          const auto t0 = q.t_start;
          q.wake_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
          lk.unlock();
          int rc = SCDE_OK;
          for (int j = 0; j < n && rc == SCDE_OK; ++j) {
            rc = issue(j);
            std::lock_guard<std::mutex> g(q.m);
            if (j == 0)
              q.first_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (rc != SCDE_OK) {
              q.err = rc;
              q.err_msg = g_err;  // g_err is thread-local: hand the worker's message to the caller
            } else {
              ++q.issued;
            }
            q.cv.notify_all();
          }
          lk.lock();
          q.busy = false;
          q.cv.notify_all();
        }
      });
    }
    const int nranges = (int)evs.size();  // (before the vectors move into the closure)
    if ((int)ranges.size() != nranges) return fail(SCDE_EINTERNAL, "upload ranges: %d ranges for %d events",
                                                   (int)ranges.size(), nranges);
    std::lock_guard<std::mutex> lk(u.m);
    u.issue = [c, h, ranges = std::move(ranges), evs = std::move(evs)](int j) -> int {
      RCHK(upload_cols(c, h, ranges[j].first, ranges[j].second));
      HCHK(handoff_spin(c, c->copy_stream));
      HCHK(hipEventRecord(evs[j], c->copy_stream));
      return SCDE_OK;
    };
    u.nranges = nranges;
    u.issued = 0;
    u.err = 0;
    u.err_msg.clear();
    u.busy = true;
    u.t_start = std::chrono::steady_clock::now();
    ++u.job;
    u.cv.notify_all();
    return SCDE_OK;
  }
  int wait(int n) {
    auto& u = ctx->upl;
    std::unique_lock<std::mutex> lk(u.m);
    u.cv.wait(lk, [&] { return u.issued >= n || u.err != 0 || !u.busy; });
    if (u.err) return fail(u.err, "count upload failed: %s", u.err_msg.c_str());
    return u.issued >= n ? SCDE_OK : fail(SCDE_EINTERNAL, "upload range %d never issued", n - 1);
  }
  // the job is finished (every range issued or failed) before the call returns: the next call's
  // job, and the caller's buffers, must not overlap it
  ~UploadWorker() {
    if (!ctx) return;
    auto& u = ctx->upl;
    std::unique_lock<std::mutex> lk(u.m);
    u.cv.wait(lk, [&] { return !u.busy; });
  }
};

// bound j (0..K) of K pieces over [0, total): equal pieces, or with taper decreasing ones
// (weights K, K - 1, .., 1: the last piece, whose unique sets and tables start only after the
// last byte has landed, is the smallest)
static long long piece_bound(long long total, int j, int K) { return total * j / K; }

static int ensure_piece_streams(scde_ctx* ctx) {
  if (!ctx->uq_stream) HCHK(hipStreamCreateWithFlags(&ctx->uq_stream, hipStreamNonBlocking));
  for (int j = 0; j < scde_ctx::kMaxPieces; ++j) {
    if (!ctx->piece_ev[j]) HCHK(hipEventCreateWithFlags(&ctx->piece_ev[j], hipEventDisableTiming));
    if (!ctx->piece_up_ev[j]) HCHK(hipEventCreateWithFlags(&ctx->piece_up_ev[j], hipEventDisableTiming));
  }
  return SCDE_OK;
}


// up (nullable): the host-count entry's upload, in pieces of the selected cells (cellidx
// strictly increasing), each piece's unique sets and tables starting as it lands
static int posteriors_run(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, const int* cellidx,
                          int ncells_sel, const double* models_sel, int local_theta, int square_logit_conc,
                          const double* prior_x, int ngrid, int nboot, int n_cores, int64_t gene_offset,
                          int64_t ngenes_total, int return_post, int ensemble, const int* batch_vals,
                          const int64_t* batch_off, const int* composition, int nbatch, double* jp, double* modes,
                          double* post, const HostUpload* up);

int scde_posteriors_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, const int* cellidx,
                        int ncells_sel, const double* models_sel, int local_theta, int square_logit_conc,
                        const double* prior_x, int ngrid, int nboot, int n_cores, int64_t gene_offset,
                        int64_t ngenes_total, int return_post, int ensemble, const int* batch_vals,
                        const int64_t* batch_off, const int* composition, int nbatch, double* jp, double* modes,
                        double* post) {
  FORK_GUARD();
  return posteriors_run(ctx, counts_dev, ld, ngenes, cellidx, ncells_sel, models_sel, local_theta, square_logit_conc,
                        prior_x, ngrid, nboot, n_cores, gene_offset, ngenes_total, return_post, ensemble, batch_vals,
                        batch_off, composition, nbatch, jp, modes, post, nullptr);
}

static int posteriors_run(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, const int* cellidx,
                          int ncells_sel, const double* models_sel, int local_theta, int square_logit_conc,
                          const double* prior_x, int ngrid, int nboot, int n_cores, int64_t gene_offset,
                          int64_t ngenes_total, int return_post, int ensemble, const int* batch_vals,
                          const int64_t* batch_off, const int* composition, int nbatch, double* jp, double* modes,
                          double* post, const HostUpload* up) {
  if (!ctx || !counts_dev || !cellidx || !models_sel || !prior_x || !jp) return fail(SCDE_EARG, "null argument");
  if (ngenes < 0 || ncells_sel <= 0 || ngrid <= 0) return fail(SCDE_EARG, "bad dimensions");
  HCHK(hipSetDevice(ctx->device));
  const bool batch = batch_vals != nullptr;
  std::vector<double> mm(models_sel, models_sel + (size_t)ncells_sel * 12);
  for (int c = 0; c < ncells_sel; ++c) {
    double& ca = mm[(size_t)c + (size_t)ncells_sel * 4];
    if (ca < 1e-10) ca = 1e-10;  // R/functions.R:579-583
  }
  const std::vector<double> mag = marginals(prior_x, ngrid);
  PostSpec s;
  s.ncells = ncells_sel;
  s.models = mm.data();
  s.localtheta = local_theta;
  s.squarelogit = square_logit_conc;
  s.mag = mag.data();
  s.G = ngrid;
  s.nboot = nboot;
  s.postflag = return_post;
  s.ensemble = batch ? 0 : ensemble;
  s.batch_call = batch;
  s.counts_dev = counts_dev;
  s.ld = ld;
  s.cellidx_host = cellidx;
  s.ngenes = ngenes;
  seeding(n_cores, gene_offset, ngenes_total, ngenes, s.seeds, s.wset);
  s.rand_kind = g_rand_kind;
  s.batch_vals = batch_vals;
  s.batch_off = batch_off;
  s.comp = composition;
  s.nbatch = nbatch;
  const size_t NG = (size_t)ngenes * ngrid;
  HCHK(ctx->jpA.ensure(sizeof(double) * std::max<size_t>(1, NG)));
  s.jp = ctx->jpA.as<double>();
  s.jp_g = 1;
  s.jp_k = ngenes;
  const bool want_modes = (batch ? return_post == 1 : (return_post == 1 || return_post == 3)) && modes;
  const bool want_post = (batch ? return_post == 2 : (return_post == 2 || return_post == 3)) && post;
  if (want_modes) {
    HCHK(ctx->jpB.ensure(sizeof(double) * std::max<size_t>(1, (size_t)ngenes * ncells_sel)));
    s.modes = ctx->jpB.as<double>();
    s.modes_early = ngenes > 0;
  }
  if (want_post) {
    HCHK(ctx->outbuf.ensure(sizeof(double) * std::max<size_t>(1, NG * ncells_sel)));
    s.post = ctx->outbuf.as<double>();
  }
  ctx->us[0].ready = false;
  std::vector<int> piece_c, piece_col;
  UploadWorker uw;
  if (up) {
    const int K = std::max(1, std::min(ctx->opt_pieces, scde_ctx::kMaxPieces));
    for (int j = 0; j <= K; ++j) piece_c.push_back((int)piece_bound(ncells_sel, j, K));
    piece_col.push_back(0);  // piece j uploads columns [piece_col[j], piece_col[j + 1])
    for (int j = 0; j < K; ++j)
      piece_col.push_back(piece_c[j + 1] > piece_c[j] ? cellidx[piece_c[j + 1] - 1] + 1 : piece_col.back());
    RCHK(ensure_piece_streams(ctx));
    RCHK(uw.start(ctx, *up, piece_col, std::vector<hipEvent_t>(ctx->piece_up_ev, ctx->piece_up_ev + K)));
    s.npieces = K;
    s.piece_c = piece_c.data();
    s.piece_stream = ctx->uq_stream;
    s.piece_ev = ctx->piece_ev;
    s.piece_ready = [&](int j) {
      RCHK(uw.wait(j + 1));
      HCHK(handoff_wait(ctx, ctx->uq_stream, ctx->piece_up_ev[j]));
      return SCDE_OK;
    };
  }
  // read-backs from the Downloader thread while the tables and the bootstrap run (modes piece by
  // piece, jp in gene chunks); every queued read-back has landed before this call returns, on
  // every return path (they write into the caller's buffers)
  struct DrainDownloads {
    scde_ctx* cx;
    bool on;
    ~DrainDownloads() {
      if (on) (void)dnl_wait(cx);
    }
  } drain{ctx, ctx->opt_modes_overlap != 0};
  if (drain.on) {
    if (s.modes_early) s.modes_host = modes;
    s.jp_host = jp;
    s.jp_chunks = ctx->opt_jp_chunks;
  }
  RCHK(run_posterior(ctx, s, ctx->us[0]));
  if (s.modes_early && !drain.on)  // after the bootstrap, on the main stream (profiling runs: no blits beside it)
    HCHK(hipMemcpyAsync(modes, s.modes, sizeof(double) * (size_t)ngenes * ncells_sel, hipMemcpyDeviceToHost,
                        ctx->stream));
  if (NG && !drain.on) HCHK(hipMemcpyAsync(jp, s.jp, sizeof(double) * NG, hipMemcpyDeviceToHost, ctx->stream));
  if (want_post && NG)
    HCHK(hipMemcpyAsync(post, s.post, sizeof(double) * NG * ncells_sel, hipMemcpyDeviceToHost, ctx->stream));
  if (drain.on) {
    drain.on = false;
    RCHK(dnl_wait(ctx));
  }
  return ctx->sync();
}

// The second lane of a DE call (opt_lanes = 2): the peer context runs the second group's
// posterior on its own streams and workspace, concurrently with the first group's on this
// context's stream.  Both groups' launches then share the CUs: the second group's small set-up
// kernels and its tables fill the first group's tails instead of waiting behind them.
// The continuations of two lanes' posteriors (draws, set-up kernels, bootstrap launch): with
// option rest_thread the second runs on a host thread of its own beside the first, so its set-up
// does not queue behind the first lane's host-side set-up and bootstrap launch and the two
// bootstraps can overlap; else one after the other.  (Each continuation touches only its own
// context's buffers and streams; a shared unique set is read-only there.)
static int run_rests(scde_ctx* ctx, const std::function<int()>& rest0, const std::function<int()>& rest1) {
  int rc1 = SCDE_OK;
  std::string err1;
  std::thread t1([&] {
    rc1 = hipSetDevice(ctx->device) == hipSuccess ? rest1() : fail(SCDE_EHIP, "hipSetDevice failed");
    if (rc1 != SCDE_OK) err1 = g_err;  // g_err is thread-local
  });
  const int rc0 = rest0();
  const std::string err0 = g_err;
  t1.join();
  if (rc0 != SCDE_OK) return fail(rc0, "%s", err0.c_str());
  if (rc1 != SCDE_OK) return fail(rc1, "%s", err1.c_str());
  return SCDE_OK;
}

static int lane_peer(scde_ctx* cx, scde_ctx** out) {
  if (!cx->peer) {
    scde_ctx* p = nullptr;
    RCHK(scde_ctx_create(cx->device, &p));
    cx->peer = p;
    for (auto& e : cx->lane_ev)
      if (!e) HCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  scde_ctx* p = cx->peer;
  p->opt_boot_skip = cx->opt_boot_skip;
  p->opt_skip_slack = cx->opt_skip_slack;
  p->opt_boot_nb = cx->opt_boot_nb;
  p->opt_skip_stats = cx->opt_skip_stats;
  p->opt_wpca_ms = cx->opt_wpca_ms;
  p->opt_boot_tiles = cx->opt_boot_tiles;
  p->opt_boot_tiles_cells = cx->opt_boot_tiles_cells;
  p->opt_tile_groups = cx->opt_tile_groups;
  p->opt_tile_max_mult = cx->opt_tile_max_mult;
  p->opt_tile_order = cx->opt_tile_order;
  p->opt_jp_chunks = cx->opt_jp_chunks;
  p->opt_unique_fixed = cx->opt_unique_fixed;
  p->opt_gene_rows = cx->opt_gene_rows;
  p->opt_gene_list_cap = cx->opt_gene_list_cap;
  p->opt_tables_nt = cx->opt_tables_nt;
  p->spin_cycles = cx->spin_cycles;
  p->profile = cx->profile;
  *out = p;
  return SCDE_OK;
}

// the peer's statistics added into the context's (and cleared on the peer)
static void merge_peer_stats(scde_ctx* cx) {
  scde_ctx* p = cx->peer;
  if (!p) return;
  cx->st_skip_slabs += p->st_skip_slabs;
  cx->st_skip_kept += p->st_skip_kept;
  cx->st_skip_stretches += p->st_skip_stretches;
  cx->st_skip_redo += p->st_skip_redo;
  cx->st_degen += p->st_degen;
  cx->st_pair_redo += p->st_pair_redo;
  cx->st_boot_f64_fma += p->st_boot_f64_fma;
  for (int i = 0; i <= scde_ctx::kQMaxTilesHost; ++i) cx->st_tile_hist[i] += p->st_tile_hist[i];
  if (p->st_boot_path >= 0) cx->st_boot_path = p->st_boot_path;
  (void)scde_ctx_reset_stats(p);
  p->st_boot_path = -1;
}

// up (nullable): the host-count entry's upload.  With it the groups start one after the other,
// each once its columns are in HBM; without, both unique tables are built first (their host
// syncs back to back), then the two posteriors.  With two lanes the second group's posterior
// runs on the peer context, beside the first's.
static int de_run(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, const scde_de_params* p,
                  double* results, double* jp1, double* jp2, double* ratio, const HostUpload* up);

int scde_expression_difference_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes,
                                   const scde_de_params* p, double* results, double* jp1, double* jp2,
                                   double* ratio) {
  FORK_GUARD();
  return de_run(ctx, counts_dev, ld, ngenes, p, results, jp1, jp2, ratio, nullptr);
}

static int de_run(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes, const scde_de_params* p,
                  double* results, double* jp1, double* jp2, double* ratio, const HostUpload* up) {
  if (!ctx || !counts_dev || !p || !p->models || !p->groups || !p->prior_x || !p->prior_y)
    return fail(SCDE_EARG, "null argument");
  if (ngenes < 0 || p->ncells <= 0 || p->ngrid <= 1) return fail(SCDE_EARG, "bad dimensions");
  RCHK(ratio_n_check("scde_expression_difference", p->ngrid));
  HCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int C = p->ncells, G = p->ngrid;
  using hclock = std::chrono::steady_clock;
  auto hlap = [&, t = hclock::now()](int slot) mutable {
    const auto now = hclock::now();
    ctx->st_host_ms[slot] += std::chrono::duration<double, std::milli>(now - t).count();
    t = now;
  };
  // split cells by group (R/functions.R:372-374, tapply over levels)
  std::vector<int> idx[2];
  for (int c = 0; c < C; ++c)
    if (p->groups[c] == 0 || p->groups[c] == 1) idx[p->groups[c]].push_back(c);
  if (idx[0].empty() || idx[1].empty()) return fail(SCDE_EARG, "both groups need at least one cell");
  const std::vector<double> mag = marginals(p->prior_x, G);
  std::vector<int> seeds, wset;
  seeding(p->n_cores, p->gene_offset, p->ngenes_total > 0 ? p->ngenes_total : ngenes, ngenes, seeds, wset);
  const size_t NG = (size_t)ngenes * G;
  HCHK(ctx->jpA.ensure(sizeof(double) * std::max<size_t>(1, NG)));
  HCHK(ctx->jpB.ensure(sizeof(double) * std::max<size_t>(1, NG)));
  std::vector<double> mm[2];
  PostSpec specs[2];
  for (int gi = 0; gi < 2; ++gi) {
    const int Cg = (int)idx[gi].size();
    mm[gi].assign((size_t)Cg * 12, NAN);
    for (int j = 0; j < 12; ++j)
      for (int c = 0; c < Cg; ++c) mm[gi][(size_t)c + (size_t)Cg * j] = p->models[(size_t)idx[gi][c] + (size_t)C * j];
    for (int c = 0; c < Cg; ++c) {
      double& ca = mm[gi][(size_t)c + (size_t)Cg * 4];
      if (ca < 1e-10) ca = 1e-10;
    }
    PostSpec& s = specs[gi];
    s.ncells = Cg;
    s.models = mm[gi].data();
    s.localtheta = p->local_theta;
    s.squarelogit = p->square_logit_conc;
    s.mag = mag.data();
    s.G = G;
    s.nboot = p->nboot;
    s.counts_dev = counts_dev;
    s.ld = ld;
    s.cellidx_host = idx[gi].data();
    s.ngenes = ngenes;
    s.seeds = seeds;
    s.wset = wset;
    s.rand_kind = p->rand_kind;
    s.jp = (gi == 0 ? ctx->jpA : ctx->jpB).as<double>();
    s.jp_g = G;  // gene-major rows for the ratio kernel
    s.jp_k = 1;
  }
  hlap(0);
  const double* jp_dev[2] = {ctx->jpA.as<double>(), ctx->jpB.as<double>()};
  {
    scde_ctx* lane = ctx;  // the context that runs the second group's posterior
    if (ctx->opt_lanes >= 2) RCHK(lane_peer(ctx, &lane));
    if (up) {
      // group by group, each after its columns have arrived (the first range ends with the
      // last cell of the group whose cells end first)
      int max0 = 0, max1 = 0;
      for (int c : idx[0]) max0 = std::max(max0, c);
      for (int c : idx[1]) max1 = std::max(max1, c);
      const int first = max0 <= max1 ? 0 : 1;
      // the first group's range in pieces, then the second group's range, uploaded back to back by
      // a worker thread: each piece's unique sets and tables start as it lands
      const int K = std::max(1, std::min(ctx->opt_pieces, scde_ctx::kMaxPieces));
      std::vector<int> piece_c, cols;
      const std::vector<int>& ix = idx[first];
      for (int j = 0; j <= K; ++j) {
        const int a = (int)piece_bound(up->cut, j, K);
        cols.push_back(a);
        piece_c.push_back((int)(std::lower_bound(ix.begin(), ix.end(), a) - ix.begin()));
      }
      RCHK(ensure_piece_streams(ctx));
      UploadWorker uw;
      cols.push_back(up->C);
      std::vector<hipEvent_t> evs(ctx->piece_up_ev, ctx->piece_up_ev + K);
      evs.push_back(ctx->up_ev[1]);
      RCHK(uw.start(ctx, *up, cols, evs));
      {
        const int gi = first;
        ctx->us[gi].ready = false;
        PostSpec& sf = specs[gi];
        sf.npieces = K;
        sf.piece_c = piece_c.data();
        sf.piece_stream = ctx->uq_stream;
        sf.piece_ev = ctx->piece_ev;
        sf.piece_ready = [&](int j) {
          RCHK(uw.wait(j + 1));
          HCHK(handoff_wait(ctx, ctx->uq_stream, ctx->piece_up_ev[j]));
          return SCDE_OK;
        };
        hlap(1);
        RCHK(run_posterior(ctx, sf, ctx->us[gi]));
        hlap(2);
      }
      {
        // the second group, once its range is in HBM: its unique sets on the peer lane (or on
        // the unique stream with one lane), so their host sync waits for its small kernels only
        const int gi = 1 - first;
        ctx->us[gi].ready = false;
        RCHK(uw.wait(K + 1));
        const PostSpec* sp[1] = {&specs[gi]};
        UniqueSet* usp[1] = {&ctx->us[gi]};
        if (lane != ctx) {
          HCHK(handoff_wait(lane, lane->stream, ctx->up_ev[1]));
          RCHK(build_unique_sets(lane, sp, usp, 1));
          hlap(1);
          RCHK(run_posterior(lane, specs[gi], ctx->us[gi]));
          HCHK(handoff_spin(lane, lane->stream));
          HCHK(hipEventRecord(ctx->lane_ev[1], lane->stream));
          HCHK(lane_join(ctx));
        } else {
          if (!ctx->uq_ev) HCHK(hipEventCreateWithFlags(&ctx->uq_ev, hipEventDisableTiming));
          HCHK(handoff_wait(ctx, ctx->uq_stream, ctx->up_ev[1]));
          const hipStream_t main = ctx->stream;
          ctx->stream = ctx->uq_stream;
          const int rc = build_unique_sets(ctx, sp, usp, 1);
          ctx->stream = main;
          RCHK(rc);
          HCHK(handoff_spin(ctx, ctx->uq_stream));
          HCHK(hipEventRecord(ctx->uq_ev, ctx->uq_stream));
          HCHK(handoff_wait(ctx, ctx->stream, ctx->uq_ev));
          hlap(1);
          RCHK(run_posterior(ctx, specs[gi], ctx->us[gi]));
        }
        hlap(2);
      }
    } else {
      // both groups' unique tables first (two host syncs, GPU otherwise idle), then the
      // heavy per-group kernels back to back on the stream
      ctx->us[0].ready = ctx->us[1].ready = false;
      const PostSpec* sp[2] = {&specs[0], &specs[1]};
      UniqueSet* up[2] = {&ctx->us[0], &ctx->us[1]};
      HCHK(handoff_spin(ctx, ctx->stream));  // (test hook: the peer's inputs start late)
      RCHK(build_unique_sets(ctx, sp, up, 2));
      hlap(1);
      if (lane != ctx) {
        HCHK(handoff_spin(ctx, ctx->stream));
        HCHK(hipEventRecord(ctx->lane_ev[0], ctx->stream));
        HCHK(handoff_wait(lane, lane->stream, ctx->lane_ev[0]));
      }
      if (lane != ctx) {
        // both groups' tables first, then both bootstraps
        std::function<int()> rest0, rest1;
        RCHK(run_posterior(ctx, specs[0], ctx->us[0], &rest0));
        RCHK(run_posterior(lane, specs[1], ctx->us[1], &rest1));
        RCHK(run_rests(ctx, rest0, rest1));
      } else {
        RCHK(run_posterior(ctx, specs[0], ctx->us[0]));
        RCHK(run_posterior(ctx, specs[1], ctx->us[1]));
      }
      if (lane != ctx) {
        HCHK(handoff_spin(lane, lane->stream));
        HCHK(hipEventRecord(ctx->lane_ev[1], lane->stream));
        HCHK(lane_join(ctx));
      }
      hlap(2);
    }
  }
  // ratio posterior + summary
  const std::vector<double> diffv = ratio_diffv(p->prior_x, G);
  const int zi = expectation_index(diffv, p->expectation);
  const size_t m = 2 * (size_t)G - 1;
  RCHK(upload(ctx, ctx->prior_y, p->prior_y, sizeof(double) * G));
  RCHK(upload(ctx, ctx->diffv, diffv.data(), sizeof(double) * m));
  const int ncol = p->compute_cz ? 6 : 5;
  HCHK(ctx->res.ensure(sizeof(double) * std::max<size_t>(1, (size_t)ngenes * ncol)));
  if (ratio) HCHK(ctx->ratio.ensure(sizeof(double) * std::max<size_t>(1, (size_t)ngenes * m)));
  RatioArgs ra{};
  ra.jp1 = jp_dev[0];
  ra.j1g = G;
  ra.j1k = 1;
  ra.jp2 = jp_dev[1];
  ra.j2g = G;
  ra.j2k = 1;
  ra.prior_y = ctx->prior_y.as<double>();
  ra.n = G;
  ra.ngenes = ngenes;
  ra.normalize = 1;
  ra.ratio = ratio ? ctx->ratio.as<double>() : nullptr;
  ra.rg = 1;
  ra.ro = ngenes;
  ra.diffv = ctx->diffv.as<double>();
  ra.zi = zi;
  ra.res = ctx->res.as<double>();
  ra.res_ld = ngenes;
  hipEvent_t ev = ctx->mark_begin(SLOT_RATIO);
  HCHK(launch_ratio_summary(ra, st));
  ctx->mark_end(SLOT_RATIO, ev);
  if (p->compute_cz && ngenes) {
    size_t wb = 0;
    HCHK(launch_bh_cz(nullptr, ngenes, nullptr, nullptr, &wb, st));
    HCHK(ctx->bhw.ensure(wb));
    HCHK(launch_bh_cz(ra.res + (size_t)4 * ngenes, ngenes, ra.res + (size_t)5 * ngenes, ctx->bhw.p, &wb, st));
  }
  if (results && ngenes)
    HCHK(hipMemcpyAsync(results, ra.res, sizeof(double) * ngenes * ncol, hipMemcpyDeviceToHost, st));
  if (ratio && ngenes) HCHK(hipMemcpyAsync(ratio, ra.ratio, sizeof(double) * ngenes * m, hipMemcpyDeviceToHost, st));
  std::vector<double> tmp;
  if ((jp1 || jp2) && NG) tmp.resize(NG);
  if (jp1 && NG) {
    HCHK(hipMemcpyAsync(tmp.data(), jp_dev[0], sizeof(double) * NG, hipMemcpyDeviceToHost, st));
    RCHK(ctx->sync());
    transpose_rows_to_colmajor(tmp.data(), ngenes, G, jp1);
  }
  if (jp2 && NG) {
    HCHK(hipMemcpyAsync(tmp.data(), jp_dev[1], sizeof(double) * NG, hipMemcpyDeviceToHost, st));
    RCHK(ctx->sync());
    transpose_rows_to_colmajor(tmp.data(), ngenes, G, jp2);
  }
  const int rc = ctx->sync();
  merge_peer_stats(ctx);
  hlap(3);
  return rc;
}

// Batch-corrected scde.expression.difference (R/functions.R:321-399), device resident:
// batch posteriors over all cells with each group's batch composition, the group
// posteriors, three ratio posteriors (batch, groups, and the 1601-column second level of
// the two with skip.prior.adjustment) and their summaries with device BH.
int scde_expression_difference_batch_dev(scde_ctx* ctx, const int* counts_dev, int64_t ld, int ngenes,
                                         const scde_de_params* p, const double* batch_models,
                                         const int* batch_codes, int nbatch, double* results, double* jp1,
                                         double* jp2, double* ratio, double* adj_ratio, double* batch_ratio) {
  FORK_GUARD();
  if (!ctx || !counts_dev || !p || !p->models || !p->groups || !p->prior_x || !p->prior_y || !batch_codes ||
      !results)
    return fail(SCDE_EARG, "null argument");
  if (ngenes < 0 || p->ncells <= 0 || p->ngrid <= 1 || nbatch < 1) return fail(SCDE_EARG, "bad dimensions");
  // (the second-level ratio runs over the 2 G - 1 columns of the first)
  if (p->ngrid > (ratio_n_max() + 1) / 2)
    return fail(SCDE_EARG, "scde_expression_difference_batch: %d grid points; the batch-adjusted ratio posterior "
                "(n = 2 * ngrid - 1) supports at most n = %d", p->ngrid, ratio_n_max());
  HCHK(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const int C = p->ncells, G = p->ngrid, N = ngenes;
  const double* bm = batch_models ? batch_models : p->models;
  std::vector<int> idx[2];
  for (int c = 0; c < C; ++c)
    if (p->groups[c] == 0 || p->groups[c] == 1) idx[p->groups[c]].push_back(c);
  if (idx[0].empty() || idx[1].empty()) return fail(SCDE_EARG, "both groups need at least one cell");
  // BatchIL (0-based cell indices per batch level) and table(batch[ii]) per group; code -1 is
  // an NA batch: tapply (R/functions.R:570) and table leave such cells out of every level
  std::vector<int> bvals;
  std::vector<int64_t> boff(nbatch + 1, 0);
  for (int c = 0; c < C; ++c)
    if (batch_codes[c] < -1 || batch_codes[c] >= nbatch) return fail(SCDE_EARG, "batch code out of range");
  for (int k = 0; k < nbatch; ++k) {
    for (int c = 0; c < C; ++c)
      if (batch_codes[c] == k) bvals.push_back(c);
    boff[k + 1] = (int64_t)bvals.size();
  }
  std::vector<int> comp[2];
  for (int gi = 0; gi < 2; ++gi) {
    comp[gi].assign(nbatch, 0);
    for (int c : idx[gi])
      if (batch_codes[c] >= 0) comp[gi][batch_codes[c]]++;
  }
  const std::vector<double> mag = marginals(p->prior_x, G);
  std::vector<int> seeds, wset;
  seeding(p->n_cores, p->gene_offset, p->ngenes_total > 0 ? p->ngenes_total : N, N, seeds, wset);
  const size_t NG = (size_t)N * G;
  HCHK(ctx->jpA.ensure(sizeof(double) * std::max<size_t>(1, NG)));
  HCHK(ctx->jpB.ensure(sizeof(double) * std::max<size_t>(1, NG)));
  HCHK(ctx->in1.ensure(sizeof(double) * std::max<size_t>(1, NG)));
  HCHK(ctx->in2.ensure(sizeof(double) * std::max<size_t>(1, NG)));
  // model matrices with the slope clamp (R/functions.R:579-583)
  auto clamp_mm = [](std::vector<double>& m, int n) {
    for (int c = 0; c < n; ++c)
      if (m[(size_t)c + (size_t)n * 4] < 1e-10) m[(size_t)c + (size_t)n * 4] = 1e-10;
  };
  std::vector<double> mm[2], mmb(bm, bm + (size_t)C * 12);
  clamp_mm(mmb, C);
  std::vector<int> allc(C);
  for (int c = 0; c < C; ++c) allc[c] = c;
  PostSpec sg[2], sb[2];
  for (int gi = 0; gi < 2; ++gi) {
    const int Cg = (int)idx[gi].size();
    mm[gi].assign((size_t)Cg * 12, NAN);
    for (int j = 0; j < 12; ++j)
      for (int c = 0; c < Cg; ++c) mm[gi][(size_t)c + (size_t)Cg * j] = p->models[(size_t)idx[gi][c] + (size_t)C * j];
    clamp_mm(mm[gi], Cg);
    for (int pass = 0; pass < 2; ++pass) {
      PostSpec& s = pass == 0 ? sg[gi] : sb[gi];
      s.ncells = pass == 0 ? Cg : C;
      s.models = pass == 0 ? mm[gi].data() : mmb.data();
      s.localtheta = p->local_theta;
      s.squarelogit = p->square_logit_conc;
      s.mag = mag.data();
      s.G = G;
      s.nboot = p->nboot;
      s.counts_dev = counts_dev;
      s.ld = ld;
      s.cellidx_host = pass == 0 ? idx[gi].data() : allc.data();
      s.ngenes = N;
      s.seeds = seeds;
      s.wset = wset;
      s.rand_kind = p->rand_kind;
      s.jp_g = G;
      s.jp_k = 1;
      if (pass == 1) {
        s.batch_call = true;
        s.batch_vals = bvals.data();
        s.batch_off = boff.data();
        s.comp = comp[gi].data();
        s.nbatch = nbatch;
      }
    }
    sg[gi].jp = (gi == 0 ? ctx->jpA : ctx->jpB).as<double>();
    sb[gi].jp = (gi == 0 ? ctx->in1 : ctx->in2).as<double>();
  }
  // unique tables: group 0 cells, group 1 cells, all cells (shared by both batch runs)
  {
    for (auto& u : ctx->us) u.ready = false;
    const PostSpec* sp[3] = {&sg[0], &sg[1], &sb[0]};
    UniqueSet* up[3] = {&ctx->us[0], &ctx->us[1], &ctx->us[2]};
    RCHK(build_unique_sets(ctx, sp, up, 3));
  }
  scde_ctx* lane = ctx;  // the second batch posterior and the second group's run on the peer lane
  if (ctx->opt_lanes >= 2) RCHK(lane_peer(ctx, &lane));
  if (lane != ctx) {
    HCHK(handoff_spin(ctx, ctx->stream));
    HCHK(hipEventRecord(ctx->lane_ev[0], ctx->stream));
    HCHK(handoff_wait(lane, lane->stream, ctx->lane_ev[0]));
    std::function<int()> rest0, rest1;
    RCHK(run_posterior(ctx, sb[0], ctx->us[2], &rest0));
    ctx->us[2].ready = true;  // same cells, same counts: reuse for the second batch run
    RCHK(run_posterior(lane, sb[1], ctx->us[2], &rest1));
    RCHK(run_rests(ctx, rest0, rest1));
    RCHK(run_posterior(ctx, sg[0], ctx->us[0], &rest0));
    RCHK(run_posterior(lane, sg[1], ctx->us[1], &rest1));
    RCHK(run_rests(ctx, rest0, rest1));
    HCHK(handoff_spin(lane, lane->stream));
    HCHK(hipEventRecord(ctx->lane_ev[1], lane->stream));
    HCHK(lane_join(ctx));
  } else {
    RCHK(run_posterior(ctx, sb[0], ctx->us[2]));
    ctx->us[2].ready = true;  // same cells, same counts: reuse for the second batch run
    RCHK(run_posterior(ctx, sb[1], ctx->us[2]));
    RCHK(run_posterior(ctx, sg[0], ctx->us[0]));
    RCHK(run_posterior(ctx, sg[1], ctx->us[1]));
  }
  // three ratio posteriors + summaries
  const std::vector<double> dv1 = ratio_diffv(p->prior_x, G);
  const int m = 2 * G - 1, m2 = 2 * m - 1;
  const std::vector<double> dv2 = ratio_diffv(dv1.data(), m);
  RCHK(upload(ctx, ctx->prior_y, p->prior_y, sizeof(double) * G));
  RCHK(upload(ctx, ctx->diffv, dv1.data(), sizeof(double) * m));
  RCHK(upload(ctx, ctx->outbuf, dv2.data(), sizeof(double) * m2));
  HCHK(ctx->ratio.ensure(sizeof(double) * std::max<size_t>(1, (size_t)N * m)));
  HCHK(ctx->part.ensure(sizeof(double) * std::max<size_t>(1, (size_t)N * m)));  // batch ratio
  if (adj_ratio) HCHK(ctx->E.ensure(sizeof(double) * std::max<size_t>(1, (size_t)N * m2)));
  HCHK(ctx->res.ensure(sizeof(double) * std::max<size_t>(1, (size_t)N * 18)));
  double* res = ctx->res.as<double>();
  size_t wb = 0;
  HCHK(launch_bh_cz(nullptr, N, nullptr, nullptr, &wb, st));
  HCHK(ctx->bhw.ensure(wb));
  auto ratio_pass = [&](const double* a1, long long a1g, long long a1k, const double* a2, long long a2g,
                        long long a2k, const double* py, int n, const double* dv, int zi, double* rout,
                        double* rres) -> int {
    RatioArgs ra{};
    ra.jp1 = a1;
    ra.j1g = a1g;
    ra.j1k = a1k;
    ra.jp2 = a2;
    ra.j2g = a2g;
    ra.j2k = a2k;
    ra.prior_y = py;
    ra.n = n;
    ra.ngenes = N;
    ra.normalize = 1;
    ra.ratio = rout;
    ra.rg = 1;
    ra.ro = N;
    ra.diffv = dv;
    ra.zi = zi;
    ra.res = rres;
    ra.res_ld = N;
    hipEvent_t ev = ctx->mark_begin(SLOT_RATIO);
    HCHK(launch_ratio_summary(ra, st));
    ctx->mark_end(SLOT_RATIO, ev);
    if (N) HCHK(launch_bh_cz(rres + (size_t)4 * N, N, rres + (size_t)5 * N, ctx->bhw.p, &wb, st));
    return SCDE_OK;
  };
  // results blocks: [0] batch.adjusted, [1] results, [2] batch.effect (each N x 6)
  double* r_adj = res;
  double* r_res = res + (size_t)6 * N;
  double* r_bat = res + (size_t)12 * N;
  const double* py = ctx->prior_y.as<double>();
  RCHK(ratio_pass(ctx->in1.as<double>(), G, 1, ctx->in2.as<double>(), G, 1, py, G, ctx->diffv.as<double>(),
                  expectation_index(dv1, 0.0), ctx->part.as<double>(), r_bat));
  RCHK(ratio_pass(ctx->jpA.as<double>(), G, 1, ctx->jpB.as<double>(), G, 1, py, G, ctx->diffv.as<double>(),
                  expectation_index(dv1, p->expectation), ctx->ratio.as<double>(), r_res));
  RCHK(ratio_pass(ctx->ratio.as<double>(), 1, N, ctx->part.as<double>(), 1, N, nullptr, m,
                  ctx->outbuf.as<double>(), expectation_index(dv2, p->expectation),
                  adj_ratio ? ctx->E.as<double>() : nullptr, r_adj));
  if (N) {
    HCHK(hipMemcpyAsync(results, res, sizeof(double) * (size_t)N * 18, hipMemcpyDeviceToHost, st));
    if (ratio) HCHK(hipMemcpyAsync(ratio, ctx->ratio.p, sizeof(double) * (size_t)N * m, hipMemcpyDeviceToHost, st));
    if (batch_ratio)
      HCHK(hipMemcpyAsync(batch_ratio, ctx->part.p, sizeof(double) * (size_t)N * m, hipMemcpyDeviceToHost, st));
    if (adj_ratio)
      HCHK(hipMemcpyAsync(adj_ratio, ctx->E.p, sizeof(double) * (size_t)N * m2, hipMemcpyDeviceToHost, st));
  }
  std::vector<double> tmp;
  for (int gi = 0; gi < 2 && NG; ++gi) {
    double* out = gi == 0 ? jp1 : jp2;
    if (!out) continue;
    tmp.resize(NG);
    HCHK(hipMemcpyAsync(tmp.data(), (gi == 0 ? ctx->jpA : ctx->jpB).p, sizeof(double) * NG, hipMemcpyDeviceToHost,
                        st));
    RCHK(ctx->sync());
    transpose_rows_to_colmajor(tmp.data(), N, G, out);
  }
  const int rc = ctx->sync();
  merge_peer_stats(ctx);
  return rc;
}

// ------------------------------------------------------------------ host-count entry points
// The R-level calls as the .Call shim makes them: counts are the caller's host matrix
// (int32, column-major, leading dimension ld >= ngenes, ncols columns).  They are copied
// into the context's staging buffer (dense, ld = ngenes) on its stream and the resident
// pipeline runs on them; everything the caller gets back is host memory.
}  // extern "C"

int scde::host::stage_counts(scde_ctx*& ctx, const int* counts, int64_t ld, int ngenes, int ncols, const int** dev) {
  RCHK(use_ctx(ctx));
  if (!counts) return fail(SCDE_EARG, "null argument");
  if (ngenes < 0 || ncols <= 0 || ld < ngenes) return fail(SCDE_EARG, "bad dimensions");
  RCHK(put_matrix(ctx, ctx->counts_in, counts, ld, ngenes, ncols));
  *dev = ctx->counts_in.as<int>();
  return SCDE_OK;
}

extern "C" {

int scde_expression_difference_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes,
                                    const scde_de_params* p, double* results, double* jp1, double* jp2,
                                    double* ratio) {
  FORK_GUARD();
  if (!p || !p->groups) return fail(SCDE_EARG, "null argument");
  RCHK(ratio_n_check("scde_expression_difference", p->ngrid));  // before the counts are staged
  RCHK(use_ctx(ctx));
  if (!counts) return fail(SCDE_EARG, "null argument");
  const int C = p->ncells;
  if (ngenes < 0 || C <= 0 || ld < ngenes) return fail(SCDE_EARG, "bad dimensions");
  // Small matrices upload in one piece and keep the batched unique-table build: the
  // per-group build costs extra host syncs, which a short transfer does not repay (two lanes,
  // one piece vs pipelined: 2,500 x 1,000 counts 1.84 vs 2.29 ms per call, 5,000 x 1,000 2.89-2.92
  // vs 3.20-3.22, 20k x 200 4.66 vs 4.87; from 32 MB the pipeline wins: 10,000 x 1,000
  // 4.72-4.92 vs 5.00-5.14)
  const size_t kPipelineBytes = (size_t)std::max(0.0, ctx->opt_pipeline_mb) * (size_t(1) << 20);
  if (ngenes == 0 || sizeof(int) * (size_t)ngenes * C < kPipelineBytes) {
    const int* dev = nullptr;
    RCHK(stage_counts(ctx, counts, ld, ngenes, C, &dev));
    return de_run(ctx, dev, ngenes, ngenes, p, results, jp1, jp2, ratio, nullptr);
  }
  // two column ranges: up to the last cell of the group whose cells end first, and the rest
  int max0 = -1, max1 = -1;
  for (int c = 0; c < C; ++c) {
    if (p->groups[c] == 0) max0 = c;
    if (p->groups[c] == 1) max1 = c;
  }
  if (max0 < 0 || max1 < 0) return fail(SCDE_EARG, "both groups need at least one cell");
  const int cut = std::min(max0, max1) + 1;
  if (!ctx->copy_stream) HCHK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
  for (auto& e : ctx->up_ev)
    if (!e) HCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  const size_t row = sizeof(int) * (size_t)ngenes;
  HCHK(ctx->counts_in.ensure(std::max<size_t>(1, row * C)));
  // the previous call's kernels may still read counts_in: the copies wait for them
  HCHK(handoff_spin(ctx, ctx->stream));
  HCHK(hipEventRecord(ctx->up_ev[1], ctx->stream));
  HCHK(handoff_wait(ctx, ctx->copy_stream, ctx->up_ev[1]));
  // (a DE call's upload hides behind the first group's unique sets and tables: as int32, unless
  // upload_u16 = 2 -- config 3 measured 6.78 ms per step with int32 against 7.22 with 16-bit counts,
  // whose narrowing threads then share the CPU with the lanes' threads)
  const HostUpload h{counts, ld, ngenes, cut, C, ctx->opt_upload_u16 == 2};
  return de_run(ctx, ctx->counts_in.as<int>(), ngenes, ngenes, p, results, jp1, jp2, ratio, &h);
}

int scde_expression_difference_batch_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes,
                                          const scde_de_params* p, const double* batch_models,
                                          const int* batch_codes, int nbatch, double* results, double* jp1,
                                          double* jp2, double* ratio, double* adj_ratio, double* batch_ratio) {
  FORK_GUARD();
  if (!p) return fail(SCDE_EARG, "null argument");
  if (p->ngrid > (ratio_n_max() + 1) / 2)  // before the counts are staged
    return fail(SCDE_EARG, "scde_expression_difference_batch: %d grid points; the batch-adjusted ratio posterior "
                "(n = 2 * ngrid - 1) supports at most n = %d", p->ngrid, ratio_n_max());
  const int* dev = nullptr;
  RCHK(stage_counts(ctx, counts, ld, ngenes, p->ncells, &dev));
  return scde_expression_difference_batch_dev(ctx, dev, ngenes, ngenes, p, batch_models, batch_codes, nbatch,
                                              results, jp1, jp2, ratio, adj_ratio, batch_ratio);
}

int scde_posteriors_host(scde_ctx* ctx, const int* counts, int64_t ld, int ngenes, int ncells_total,
                         const int* cellidx, int ncells_sel, const double* models_sel, int local_theta,
                         int square_logit_conc, const double* prior_x, int ngrid, int nboot, int n_cores,
                         int64_t gene_offset, int64_t ngenes_total, int return_post, int ensemble,
                         const int* batch_vals, const int64_t* batch_off, const int* composition, int nbatch,
                         double* jp, double* modes, double* post) {
  FORK_GUARD();
  if (!cellidx) return fail(SCDE_EARG, "null argument");
  for (int i = 0; i < ncells_sel; ++i)
    if (cellidx[i] < 0 || cellidx[i] >= ncells_total) return fail(SCDE_EARG, "cell index %d out of range", cellidx[i]);
  RCHK(use_ctx(ctx));
  bool increasing = ncells_sel > 0;
  for (int i = 1; i < ncells_sel && increasing; ++i) increasing = cellidx[i] > cellidx[i - 1];
  if (ngenes > 0 && counts && ld >= ngenes && increasing && ctx->opt_pieces > 1 &&
      sizeof(int) * (size_t)ngenes * ncells_total >= (size_t)std::max(0.0, ctx->opt_pipeline_mb) * (size_t(1) << 20)) {
    // the selected cells' columns in pieces on the copy stream, each piece's unique sets and
    // tables starting as it lands
    if (!ctx->copy_stream) HCHK(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    for (auto& e : ctx->up_ev)
      if (!e) HCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HCHK(ctx->counts_in.ensure(sizeof(int) * (size_t)ngenes * ncells_total));
    // the previous call's kernels may still read counts_in: the copies wait for them
    HCHK(handoff_spin(ctx, ctx->stream));
    HCHK(hipEventRecord(ctx->up_ev[1], ctx->stream));
    HCHK(handoff_wait(ctx, ctx->copy_stream, ctx->up_ev[1]));
    const HostUpload h{counts, ld, ngenes, 0, ncells_total, ctx->opt_upload_u16 != 0};
    return posteriors_run(ctx, ctx->counts_in.as<int>(), ngenes, ngenes, cellidx, ncells_sel, models_sel, local_theta,
                          square_logit_conc, prior_x, ngrid, nboot, n_cores, gene_offset, ngenes_total, return_post,
                          ensemble, batch_vals, batch_off, composition, nbatch, jp, modes, post, &h);
  }
  const int* dev = nullptr;
  RCHK(stage_counts(ctx, counts, ld, ngenes, ncells_total, &dev));
  return scde_posteriors_dev(ctx, dev, ngenes, ngenes, cellidx, ncells_sel, models_sel, local_theta,
                             square_logit_conc, prior_x, ngrid, nboot, n_cores, gene_offset, ngenes_total,
                             return_post, ensemble, batch_vals, batch_off, composition, nbatch, jp, modes, post);
}

}  // extern "C"
