// unique.hip -- the unique-count set of the scde differential-expression path on gfx950 and the
// gathers through it (R/functions.R:609-610 done on the device).  All on the default path but
// k_spin.
//
//   k_cell_minmax, k_mark, k_rank, k_fill_ucl, k_uci   per cell the sorted unique counts (ucl) and
//                     every gene's index into them (uci), by a bitmap over the cell's count range
//   k_widen16, k_patch32   16-bit host counts widened to the int32 counts the build reads
//   k_ell             per gene the (cell, column) entries of the cells off their baseline column,
//                     padded, and the tile bootstrap's gene-order keys
//   k_modes, k_post   gathers of the tables' argmax / rows through uci
//   k_colmajor_to_rows   jpmat: column-major -> row-major
//   k_spin            test hook: one wave spinning for a number of shader clocks
// The launchers follow the kernels.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdint>

#include "kernels.h"

namespace scde {

// ------------------------------------------------------------------ device unique-count builder
// counts: column-major, column = cellidx[c], rows g0 .. g0+ngenes
__global__ void k_cell_minmax(const int* __restrict__ counts, long long ld, long long g0, int ngenes,
                              const int* __restrict__ cellidx, int* __restrict__ cmax, int* __restrict__ cmin) {
  __shared__ int smax[16], smin[16];
  const int c = blockIdx.x;
  const int* col = counts + (long long)cellidx[c] * ld + g0;
  int mx = 0, mn = 0x7fffffff;
  // 16-byte loads over the aligned middle of the column (one count matrix pass, HBM-bound)
  const int head = (int)min<long long>(ngenes, (4 - (((uintptr_t)col >> 2) & 3)) & 3);
  const int nv = (ngenes - head) >> 2;
  const int4* col4 = reinterpret_cast<const int4*>(col + head);
  for (int i = threadIdx.x; i < nv; i += blockDim.x) {
    const int4 x = col4[i];
    mx = max(mx, max(max(x.x, x.y), max(x.z, x.w)));
    mn = min(mn, min(min(x.x, x.y), min(x.z, x.w)));
  }
  for (int g = threadIdx.x; g < head; g += blockDim.x) {
    mx = max(mx, col[g]);
    mn = min(mn, col[g]);
  }
  for (int g = head + 4 * nv + threadIdx.x; g < ngenes; g += blockDim.x) {
    mx = max(mx, col[g]);
    mn = min(mn, col[g]);
  }
  for (int m = 32; m >= 1; m >>= 1) {
    mx = max(mx, __shfl_xor(mx, m, 64));
    mn = min(mn, __shfl_xor(mn, m, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    smax[threadIdx.x >> 6] = mx;
    smin[threadIdx.x >> 6] = mn;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < (int)(blockDim.x >> 6); ++w) {
      mx = max(mx, smax[w]);
      mn = min(mn, smin[w]);
    }
    mx = max(mx, smax[0]);
    mn = min(mn, smin[0]);
    cmax[c] = mx;
    cmin[c] = mn;
  }
}

// One cell per blockIdx.y, KM genes per thread.  Counts below 64*MW set bits in an LDS
// copy of the cell's first MW bitmap words (most counts are small, and 0 alone is ~2/3 of
// them: global atomics on that one word serialised at L2); the block then flushes at most
// MW global atomicOr.  Larger counts go straight to global memory (sparse words).
template <int KM, int MW>
__global__ __launch_bounds__(256) void k_mark(const int* __restrict__ counts, long long ld, long long g0,
                                              int ngenes, const int* __restrict__ cellidx,
                                              const long long* __restrict__ woff,
                                              unsigned long long* __restrict__ bits, int* __restrict__ flags) {
  __shared__ unsigned long long lw[MW];
  const int c = blockIdx.y;
  if (threadIdx.x < MW) lw[threadIdx.x] = 0ull;
  __syncthreads();
  const int* __restrict__ col = counts + (long long)cellidx[c] * ld + g0;
  unsigned long long* __restrict__ cb = bits + woff[c];
  // flags (fixed-width bitmaps, cmax unknown): bit 0 a negative count, bit 1 a count past the
  // cell's bitmap (the caller rebuilds with exact widths); such counts are not marked
  const long long width = flags ? woff[c + 1] - woff[c] : 0;
  const int base = blockIdx.x * (256 * KM) + threadIdx.x;
#pragma unroll
  for (int j = 0; j < KM; ++j) {
    const int g = base + j * 256;
    bool valid = g < ngenes;
    const int x = valid ? col[g] : 0;
    if (flags && valid && (x < 0 || (x >> 6) >= width)) {
      atomicOr(flags, x < 0 ? 1 : 2);
      valid = false;
    }
    // count 0 (the common case) by ballot: one LDS atomic per wave instead of up to 64
    if (__ballot(valid && x == 0) && (threadIdx.x & 63) == 0) atomicOr(&lw[0], 1ull);
    if (valid && x != 0) {
      const unsigned long long bit = 1ull << (x & 63);
      if ((x >> 6) < MW)
        atomicOr(&lw[x >> 6], bit);
      else
        atomicOr(&cb[x >> 6], bit);
    }
  }
  __syncthreads();
  if (threadIdx.x < MW) {
    const unsigned long long v = lw[threadIdx.x];
    // words beyond the cell's own bitmap are never set (x <= cmax)
    if (v) atomicOr(&cb[threadIdx.x], v);
  }
}

// per cell: exclusive popcount prefix of its bitmap words -> rank, and #unique
__global__ __launch_bounds__(256) void k_rank(const unsigned long long* __restrict__ bits,
                                              const long long* __restrict__ woff, int* __restrict__ rank,
                                              int* __restrict__ nuniq, const int* __restrict__ flags_in,
                                              int* __restrict__ flags_out) {
  __shared__ int wsum[4];
  __shared__ int carry;
  const int c = blockIdx.x;
  const long long w0 = woff[c], w1 = woff[c + 1];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (long long base = w0; base < w1; base += blockDim.x) {
    const long long w = base + threadIdx.x;
    const int pc = (w < w1) ? __popcll(bits[w]) : 0;
    int incl = pc;
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wid] = incl;
    __syncthreads();
    int pre = carry;
    for (int v = 0; v < wid; ++v) pre += wsum[v];
    if (w < w1) rank[w] = pre + incl - pc;
    __syncthreads();
    if (threadIdx.x == 0) carry += wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
  }
  if (threadIdx.x == 0) nuniq[c] = carry;
  // k_mark's flags next to the counts (one read-back for both; k_mark ran before in stream order)
  if (flags_in && c == 0 && threadIdx.x == 0) *flags_out = *flags_in;
}

__global__ __launch_bounds__(256) void k_fill_ucl(const unsigned long long* __restrict__ bits,
                                                  const long long* __restrict__ woff,
                                                  const int* __restrict__ rank,
                                                  const long long* __restrict__ ucl_off, int* __restrict__ ucl) {
  const int c = blockIdx.x;
  const long long w0 = woff[c], w1 = woff[c + 1];
  for (long long w = w0 + threadIdx.x; w < w1; w += blockDim.x) {
    unsigned long long b = bits[w];
    long long pos = ucl_off[c] + rank[w];
    while (b) {
      const int t = __ffsll((long long)b) - 1;
      ucl[pos++] = (int)((w - w0) * 64 + t);
      b &= b - 1;
    }
  }
}

__global__ void k_uci(const int* __restrict__ counts, long long ld, long long g0, int ngenes, int ncells,
                      const int* __restrict__ cellidx, const long long* __restrict__ woff,
                      const unsigned long long* __restrict__ bits, const int* __restrict__ rank,
                      int* __restrict__ uci) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)ngenes * ncells) return;
  const int g = (int)(i % ngenes), c = (int)(i / ngenes);
  const int x = counts[(long long)cellidx[c] * ld + g0 + g];
  const long long w = woff[c] + (x >> 6);
  const unsigned long long below = bits[w] & ((1ull << (x & 63)) - 1ull);
  uci[(long long)g + (long long)ngenes * c] = rank[w] + __popcll(below);
}

// 16-bit host counts widened to the int32 counts the unique-set build reads (U16Ring uploads)
__global__ __launch_bounds__(256) void k_widen16(const unsigned short* __restrict__ in, int* __restrict__ out,
                                                 long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = in[i];
}

// out[idx] = count for each listed (idx, count): the counts the 16-bit upload could not carry
__global__ __launch_bounds__(256) void k_patch32(const int2* __restrict__ exc, long long n, int* __restrict__ out) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[exc[i].x] = exc[i].y;
}

// ELL rows: per gene the (cell, column) pairs of the cells whose column is not the cell's
// baseline, in cell order, then pad entries (cell 0, the zero column) to a multiple of 8 plus
// one look-ahead batch of 8 (k_boot2), or with padto 64 to whole 64-entry steps plus 8 (the tile
// bootstrap's bounds).  A block takes 64 genes and every cell: each 64-cell step of uci (genes
// fastest, as R lays out the count matrix) is read coalesced into an LDS tile (stride 65
// against bank conflicts), then each wave compacts its genes' entries with ballots (mbcnt
// prefix, cell order kept).  (A two-pass build over cell chunks, which fills the CUs a grid of
// ngenes / 64 blocks leaves idle, was measured and lost.)  The block then writes the row
// length, the pad entries and, with `key`, the gene's 16-bit tile-order key: the sum of its
// entries' counts (ucl[col]) on a log scale -- genes of like expression next to each other, so
// that waves in flight share columns -- under its gene chunk's index in the top bits (kch chunks
// of the kgn genes, this launch's genes from kg0), descending when `desc` (heaviest genes first
// within each chunk).  (Measured and not kept: the sum of the count ranks, uci, as the key, without
// the gather: the same bootstrap fetch, 28.5-28.6 GB per launch at config 4.)
// waves per 64-gene block (4, 8 or 16).  8: blocks of 512 threads find room beside the tables
// kernel's blocks (the ELL rows run on the aux stream during phase 2); measured against 16, one box,
// alternating runs: shard of 8 device-resident 1.36-1.60 vs 1.43-1.46 ms, config 4 14.07-14.11 vs
// 14.20-14.25, config 3 equal; 4 waves slower (config 3 6.77-6.93 vs 6.55-6.68 host -> host)
#ifndef SCDE_ELL_WAVES
#define SCDE_ELL_WAVES 8
#endif
constexpr int kEllWaves = SCDE_ELL_WAVES;
constexpr int kEllKeyBits = 16;  // gene-order key width (launch_gene_order sorts these bits)
__global__ __launch_bounds__(64 * kEllWaves) void k_ell(const int* __restrict__ uci, long long ld_uci, int ngenes,
                                             int ncells, const long long* __restrict__ ucl_off,
                                             const int* __restrict__ base_col, int stride, int pad_col,
                                             int padto, int2* __restrict__ ent, int* __restrict__ nnz, int cell_off,
                                             const int* __restrict__ ucl, unsigned* __restrict__ key,
                                             int* __restrict__ idx, int kg0, int kgn, int kch, int desc) {
  __shared__ int tile[64][65];  // [cell][gene]
  // wid through readfirstlane: the wave's genes, rows and entry counts are then scalar values,
  // which keeps the kernel at 6 or more waves per SIMD (as a vector value wid cost 95 VGPRs)
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int g0 = blockIdx.x * 64;
  constexpr int GPW = 64 / kEllWaves;  // genes per wave
  const bool want_key = key != nullptr;
  int n[GPW];
  unsigned long long ks[GPW];  // per lane: its cells' kept counts (the key)
#pragma unroll
  for (int i = 0; i < GPW; ++i) {
    n[i] = 0;
    ks[i] = 0;
  }
  // software pipeline: the next 64-cell step's uci rows (this wave's 4 rows of the tile) and
  // its lane cell's column offset and baseline column are loaded before the current step is
  // compacted, so each step's loads wait behind the previous step's work, not in front of it
  constexpr int RPW = 64 / kEllWaves;  // tile rows per wave
  int pu[RPW];
  long long poff = 0;
  int pbc = -1;
  auto prefetch = [&](int c0) {
#pragma unroll
    for (int r = 0; r < RPW; ++r) {
      const int c = c0 + wid + r * kEllWaves, g = g0 + lane;
      pu[r] = (c < ncells && g < ngenes) ? uci[(long long)g + ld_uci * c] : 0;
    }
    const int c = c0 + lane;
    poff = 0;
    pbc = -1;
    if (c < ncells) {
      poff = ucl_off[c];
      pbc = base_col[c];
    }
  };
  if (ncells > 0) prefetch(0);
  for (int c0 = 0; c0 < ncells; c0 += 64) {
    __syncthreads();
#pragma unroll
    for (int r = 0; r < RPW; ++r) tile[wid + r * kEllWaves][lane] = pu[r];
    const long long off = poff;
    const int bc = pbc;
    __syncthreads();
    if (c0 + 64 < ncells) prefetch(c0 + 64);
    const int c = c0 + lane;
#pragma unroll
    for (int i = 0; i < GPW; ++i) {
      const int gl = wid * GPW + i, g = g0 + gl;
      if (g >= ngenes) break;
      int col = -1;
      bool keep = false;
      if (c < ncells) {
        col = (int)(off + tile[lane][gl]);
        keep = col != bc;
      }
      const unsigned long long m = __ballot(keep);
      const int pos = n[i] + __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0));
      if (keep) ent[(long long)g * stride + pos] = make_int2(c + cell_off, col);
      if (want_key && keep) ks[i] += (unsigned)max(ucl[col], 0);
      n[i] += __popcll(m);
    }
  }
#pragma unroll
  for (int i = 0; i < GPW; ++i) {
    const int g = g0 + wid * GPW + i;
    if (g >= ngenes) break;
    unsigned long long kv = ks[i];
    if (want_key) {
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) kv += __shfl_xor(kv, o, 64);
    }
    const int nn = n[i];
    if (lane == 0) {
      nnz[g] = nn;
      if (want_key) {
        // the gene chunk of gene kg0 + g: chunk k holds [kgn k / kch, kgn (k + 1) / kch)
        const long long gg = (long long)kg0 + g;
        int k = (int)(gg * kch / kgn);
        while (k + 1 < kch && (long long)kgn * (k + 1) / kch <= gg) ++k;
        while (k > 0 && (long long)kgn * k / kch > gg) --k;
        int hb = 0;  // bits of the chunk index
        while ((1 << hb) < kch) ++hb;
        // 16-bit keys (the sort then takes two radix passes, not four): the chunk index, then the
        // count sum on a log scale, (2^(16 - hb) - 1) / 33 steps per octave
        const unsigned vmax = (1u << (kEllKeyBits - hb)) - 1u;
        unsigned v = (unsigned)(log2((double)kv + 1.0) * ((double)vmax / 33.0));
        v = v > vmax ? vmax : v;
        if (desc) v = vmax - v;
        key[g] = (hb ? ((unsigned)k << (kEllKeyBits - hb)) : 0u) | v;
        idx[g] = kg0 + g;
      }
    }
    const int end = padto == 64 ? (nn > 0 ? (nn + 63) & ~63 : 64) + 8 : ((nn + 7) & ~7) + 8;
    int2* E = ent + (long long)g * stride;
    for (int q = nn + lane; q < end && q < stride; q += 64) E[q] = make_int2(0, pad_col);
  }
}

// ------------------------------------------------------------------ modes / post gathers
__global__ void k_modes(const int* __restrict__ uci, long long ld_uci, int ngenes, int ncells,
                        const long long* __restrict__ ucl_off, const int* __restrict__ maxi,
                        const double* __restrict__ mag, double* __restrict__ modes, long long mg, long long mc) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)ngenes * ncells) return;
  const int g = (int)(i % ngenes), c = (int)(i / ngenes);
  const long long col = ucl_off[c] + uci[(long long)g + ld_uci * c];
  modes[g * mg + c * mc] = mag[maxi[col]];
}

__global__ void k_post(const int* __restrict__ uci, long long ld_uci, int ngenes, int c,
                       const long long* __restrict__ ucl_off, const double* __restrict__ T, int G, int GS,
                       double* __restrict__ post, long long pg, long long pk) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)ngenes * G) return;
  const int g = (int)(i % ngenes), k = (int)(i / ngenes);
  const long long col = ucl_off[c] + uci[(long long)g + ld_uci * c];
  post[g * pg + k * pk] = T[col * GS + k];
}

// ------------------------------------------------------------------ jpmat: transpose column-major -> row-major
__global__ void k_colmajor_to_rows(const double* __restrict__ src, int nrows, int ncols, int GS,
                                   double* __restrict__ dst) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)nrows * ncols) return;
  const int r = (int)(i % nrows), k = (int)(i / nrows);
  dst[(long long)r * GS + k] = src[i];
}

// Test hook (scde_ctx_inject_fault "handoff_spin"): one wave that spins for `cycles` shader clocks,
// queued on a producing stream before a cross-stream handoff's event -- a consumer that misses its
// wait then reads the producer's output before it is written, every time, not once in a while.
__global__ void k_spin(long long cycles) {
  const long long t0 = clock64();
  while (clock64() - t0 < cycles) __builtin_amdgcn_s_sleep(1);
}

// ================================================================== launchers
hipError_t launch_spin(hipStream_t s, long long cycles) {
  if (cycles <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, s, std::min(cycles, 100000000LL));  // (at most ~0.05 s)
  return hipGetLastError();
}

hipError_t launch_patch32(const int2* exc, size_t n, int* out, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_patch32, dim3((unsigned)div_up((long long)n, 256)), dim3(256), 0, s, exc, (long long)n, out);
  return hipGetLastError();
}

hipError_t launch_widen16(const unsigned short* in, int* out, size_t n, hipStream_t s) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_widen16, dim3((unsigned)div_up((long long)n, 256)), dim3(256), 0, s, in, out, (long long)n);
  return hipGetLastError();
}

hipError_t launch_ell(const int* uci, long long ld_uci, int ngenes, int ncells, const long long* ucl_off,
                      const int* base_col, int stride, int pad_col, int padto, int2* ent, int* nnz, hipStream_t s,
                      int cell_off, const int* ucl, unsigned* key, int* idx, int kg0, int kgn, int kch, int desc) {
  if (ngenes <= 0) return hipSuccess;
  if (padto == 64 ? stride < ((ncells + 63) & ~63) + 8 || stride < 72 : stride < ((ncells + 7) & ~7) + 8)
    return hipErrorInvalidValue;
  if (cell_off < 0) return hipErrorInvalidValue;
  if (key && (!ucl || !idx || kch < 1 || kgn < kg0 + ngenes || kch > kgn)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_ell, dim3(div_up(ngenes, 64)), dim3(64 * kEllWaves), 0, s, uci, ld_uci, ngenes, ncells, ucl_off,
                     base_col, stride, pad_col, padto, ent, nnz, cell_off, ucl, key, idx, kg0, kgn, kch, desc);
  return hipGetLastError();
}

hipError_t launch_modes(const int* uci, long long ld_uci, int ngenes, int ncells, const long long* ucl_off,
                        const int* maxi, const double* mag, double* modes, long long mg, long long mc,
                        hipStream_t s) {
  const long long n = (long long)ngenes * ncells;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_modes, dim3(div_up(n, 256)), dim3(256), 0, s, uci, ld_uci, ngenes, ncells, ucl_off, maxi,
                     mag, modes, mg, mc);
  return hipGetLastError();
}

hipError_t launch_post(const int* uci, long long ld_uci, int ngenes, int c, const long long* ucl_off,
                       const double* T, int G, int GS, double* post, long long pg, long long pk, hipStream_t s) {
  const long long n = (long long)ngenes * G;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_post, dim3(div_up(n, 256)), dim3(256), 0, s, uci, ld_uci, ngenes, c, ucl_off, T, G, GS,
                     post, pg, pk);
  return hipGetLastError();
}

hipError_t launch_cell_minmax(const int* counts, long long ld, long long g0, int ngenes, int ncells,
                              const int* cellidx, int* cmax, int* cmin, hipStream_t s) {
  if (ncells <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_cell_minmax, dim3(ncells), dim3(256), 0, s, counts, ld, g0, ngenes, cellidx, cmax, cmin);
  return hipGetLastError();
}

hipError_t launch_mark(const int* counts, long long ld, long long g0, int ngenes, int ncells, const int* cellidx,
                       const long long* woff, unsigned long long* bits, hipStream_t s, int* flags) {
  const long long n = (long long)ngenes * ncells;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL((k_mark<8, 16>), dim3(div_up(ngenes, 256 * 8), ncells), dim3(256), 0, s, counts, ld, g0,
                     ngenes, cellidx, woff, bits, flags);
  return hipGetLastError();
}

hipError_t launch_rank(const unsigned long long* bits, const long long* woff, int ncells, int* rank, int* nuniq,
                       hipStream_t s, const int* flags_in, int* flags_out) {
  if (ncells <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_rank, dim3(ncells), dim3(256), 0, s, bits, woff, rank, nuniq, flags_in, flags_out);
  return hipGetLastError();
}

hipError_t launch_fill_ucl(const unsigned long long* bits, const long long* woff, int ncells, const int* rank,
                           const long long* ucl_off, int* ucl, hipStream_t s) {
  if (ncells <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_fill_ucl, dim3(ncells), dim3(256), 0, s, bits, woff, rank, ucl_off, ucl);
  return hipGetLastError();
}

hipError_t launch_uci(const int* counts, long long ld, long long g0, int ngenes, int ncells, const int* cellidx,
                      const long long* woff, const unsigned long long* bits, const int* rank, int* uci,
                      hipStream_t s) {
  const long long n = (long long)ngenes * ncells;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_uci, dim3(div_up(n, 256)), dim3(256), 0, s, counts, ld, g0, ngenes, ncells, cellidx, woff,
                     bits, rank, uci);
  return hipGetLastError();
}

hipError_t launch_colmajor_to_rows(const double* src, int nrows, int ncols, int GS, double* dst, hipStream_t s) {
  const long long n = (long long)nrows * ncols;
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(k_colmajor_to_rows, dim3(div_up(n, 256)), dim3(256), 0, s, src, nrows, ncols, GS, dst);
  return hipGetLastError();
}

}  // namespace scde
