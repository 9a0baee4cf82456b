#!/usr/bin/env python
"""Timing of the Spearman kernels (scde_amd/spearman.py, csrc/spearman.hip).

    python tools/bench_spearman.py [--out profiles/spearman_bench.json] [--shapes 2000x200,20000x1000,20000x3000]
                                   [--reps 3] [--warmup 1] [--no-baseline] [--baseline-pairs 200]

Per shape (genes x cells; bench.py's synthetic counts, min.count.threshold 2 as tools/bench_knn.py),
wall times of calls that end in the library's stream synchronise (a warm-up, then the median of
--reps), host -> host and with the data resident:

  * rank         the rank transform of a cells x genes matrix of normal draws (a gene contiguous,
                 as in pagoda.gene.clusters' random rounds); bytes read and written over the
                 resident time, beside the HBM peak and a device-to-device copy timed in the same run
  * distance     one Spearman gene-cluster distance on the resident matrix: the ranks into a second
                 matrix, then scde_cor_distance_dev (genes x genes, left in HBM)
  * similarity   the pairwise-complete cell similarity, C x C read back; the kernels' own time from
                 the context's HIP events, the same with a threshold above every count (the codes
                 are streamed, no table is touched: what the streaming alone costs), and with the
                 tables forced into the global workspace (lds_values = 8)

The baseline is the numpy / scipy restatement on one CPU thread: scipy.stats.rankdata over the
columns, 1 - numpy.corrcoef of the ranks, and per pair of cells rankdata of the complete cases and
their correlation.  The rank and distance baselines run on at most 2000 / 1000 genes and the
similarity baseline on --baseline-pairs pairs; each is scaled to the whole problem and labelled so.
The library's similarity is also compared bit for bit with tests/spearman_ref.py on 40 pairs.
Prints one JSON document and writes it to --out.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"   # the baseline is one CPU thread; the library's host code does not use them

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_varnorm import HBM_PEAK, _kernel_ms, _median_ms, copy_rate  # noqa: E402

THR = 2


def bench_shape(N, C, reps, warmup, baseline, baseline_pairs):
    import bench
    import spearman_ref as S
    from scde_amd import api, rank_columns, spearman_cell_similarity
    from scde_amd._lib import check, lib
    L, ctx = lib(), api.default_context()
    _, counts, _ = bench.synthetic(9100 + N % 991, N, C, two_groups=True)
    counts = np.asfortranarray(counts, dtype=np.int32)
    rng = np.random.default_rng(N + C)
    x = np.asfortranarray(rng.normal(size=(C, N)))  # cells x genes: a gene contiguous
    r = {"zeros": float(np.mean(counts == 0)), "valid": float(np.mean(counts >= THR))}
    keep = {}

    # ---- rank transform and gene-cluster distance
    def rank_host():
        keep["ranks"] = rank_columns(x)

    r["rank_ms"] = _median_ms(rank_host, reps, warmup)
    bufs = []

    def dev(nbytes):
        p = ctypes.c_void_p()
        check(L.scde_dev_alloc(ctx.handle, nbytes, ctypes.byref(p)))
        bufs.append(p)
        return p
    try:
        xd, rd, gd = dev(x.nbytes), dev(x.nbytes), dev(8 * N * N)
        check(L.scde_h2d(ctx.handle, xd, api._p(x), x.nbytes))

        def rank_resident():
            check(L.scde_rank_cols_dev(ctx.handle, xd, C, N, rd))

        def distance_resident():
            check(L.scde_rank_cols_dev(ctx.handle, xd, C, N, rd))
            check(L.scde_cor_distance_dev(ctx.handle, rd, C, N, gd))

        def pearson_distance_resident():
            check(L.scde_cor_distance_dev(ctx.handle, xd, C, N, gd))

        r["rank_resident_ms"] = _median_ms(rank_resident, reps, warmup)
        r["distance_resident_ms"] = _median_ms(distance_resident, reps, warmup)
        r["pearson_distance_resident_ms"] = _median_ms(pearson_distance_resident, reps, warmup)
        distance_resident()
        gs = min(N, 1000)
        block = np.zeros((N, gs), order="F")  # the first gs columns of the distance
        check(L.scde_d2h(ctx.handle, api._p(block), gd, block.nbytes))
    finally:
        for p in bufs:
            check(L.scde_dev_free(ctx.handle, p))
    r["rank_bytes"] = 16.0 * N * C
    r["rank_bytes_per_s"] = r["rank_bytes"] / (r["rank_resident_ms"] * 1e-3)
    r["rank_share_of_hbm_peak"] = r["rank_bytes_per_s"] / HBM_PEAK

    # ---- cell similarity
    def sim_host():
        keep["sim"] = spearman_cell_similarity(counts, THR)

    r["similarity_ms"] = _median_ms(sim_host, reps, warmup)
    dc = api.DeviceCounts(ctx, counts)
    try:
        def sim_resident():
            keep["sim_resident"] = spearman_cell_similarity(dc, THR)

        def sim_stream_only():
            spearman_cell_similarity(dc, 2 ** 31 - 1)

        def sim_workspace():
            keep["sim_ws"] = spearman_cell_similarity(dc, THR, lds_values=8)

        r["similarity_resident_ms"] = _median_ms(sim_resident, reps, warmup)
        r["similarity_kernel_ms"] = _kernel_ms(ctx, sim_resident, reps)
        r["similarity_stream_only_kernel_ms"] = _kernel_ms(ctx, sim_stream_only, reps)
        r["similarity_workspace_kernel_ms"] = _kernel_ms(ctx, sim_workspace, reps)
    finally:
        dc.free()
    sim = keep["sim"]
    r["similarity_entries_equal"] = bool(sim.tobytes() == keep["sim_resident"].tobytes() == keep["sim_ws"].tobytes())
    r["similarity_nan"] = int(np.isnan(sim).sum())
    d = [len(np.unique(counts[counts[:, c] >= THR, c])) for c in range(C)]
    r["distinct_values_per_cell"] = [int(min(d)), int(max(d))]
    code_bytes = 2 if N <= 65535 else 4
    r["similarity_code_pairs"] = C * (C + 1) / 2 * N * 2.0   # two passes over the genes of every pair
    r["similarity_code_bytes"] = r["similarity_code_pairs"] * 2 * code_bytes
    kms = r["similarity_kernel_ms"]
    if kms > 0:
        r["similarity_code_pairs_per_s"] = r["similarity_code_pairs"] / (kms * 1e-3)
        r["similarity_code_bytes_per_s"] = r["similarity_code_bytes"] / (kms * 1e-3)
        r["similarity_code_bytes_share_of_hbm_peak"] = r["similarity_code_bytes_per_s"] / HBM_PEAK
        r["similarity_pairs_per_s"] = C * (C + 1) / 2 / (kms * 1e-3)
    pairs = [(int(i), int(j)) for i, j in rng.integers(0, C, size=(40, 2))]
    r["similarity_equal_restatement_40_pairs"] = bool(all(
        np.float64(S.pair_similarity(counts[:, i], counts[:, j], THR)).tobytes() == sim[i, j].tobytes()
        for i, j in pairs))

    if baseline:
        from scipy.stats import rankdata
        b = {}
        gs_r = min(N, 2000)
        t0 = time.perf_counter()
        rr = rankdata(x[:, :gs_r], method="average", axis=0)
        t_rank = (time.perf_counter() - t0) * 1e3
        b["rank_ms"] = t_rank * (N / gs_r)
        b["rank_note"] = f"timed on {gs_r} genes, scaled by {N} / {gs_r}" if gs_r < N else "all genes"
        r["rank_equal_scipy"] = bool(np.array_equal(rr, keep["ranks"][:, :gs_r]))
        t0 = time.perf_counter()
        dd = 1 - np.corrcoef(rankdata(x[:, :gs], method="average", axis=0), rowvar=False)
        b["distance_ms"] = (time.perf_counter() - t0) * 1e3 * (N / gs) ** 2
        b["distance_note"] = f"timed on {gs} genes, scaled by ({N} / {gs})^2" if gs < N else "all genes"
        r["distance_max_abs_difference"] = float(np.max(np.abs(dd - block[:gs])))
        bp = [(int(i), int(j)) for i, j in rng.integers(0, C, size=(baseline_pairs, 2))]
        worst = 0.0
        t0 = time.perf_counter()
        ref = []
        for i, j in bp:
            s = (counts[:, i] >= THR) & (counts[:, j] >= THR)
            a, c = rankdata(counts[s, i], method="average"), rankdata(counts[s, j], method="average")
            with np.errstate(all="ignore"):
                ref.append(np.corrcoef(a, c)[0, 1] if s.sum() > 1 else np.nan)
        t_pairs = (time.perf_counter() - t0) * 1e3
        for (i, j), v in zip(bp, ref):
            if not (np.isnan(v) and np.isnan(sim[i, j])):
                worst = max(worst, abs(v - sim[i, j]))
        npairs = C * (C + 1) / 2
        b["similarity_ms"] = t_pairs * npairs / len(bp)
        b["similarity_note"] = f"timed on {len(bp)} pairs, scaled to {int(npairs)}"
        r["similarity_max_abs_difference_scipy"] = float(worst)
        r["numpy"] = b
        r["numpy_over_library"] = {"rank": b["rank_ms"] / r["rank_ms"],
                                   "rank_resident": b["rank_ms"] / r["rank_resident_ms"],
                                   "distance_resident": b["distance_ms"] / r["distance_resident_ms"],
                                   "similarity": b["similarity_ms"] / r["similarity_ms"],
                                   "similarity_resident": b["similarity_ms"] / r["similarity_resident_ms"]}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2000x200,20000x1000,20000x3000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--baseline-pairs", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spearman_bench.json"))
    args = ap.parse_args()
    doc = {"tool": "tools/bench_spearman.py", "reps": args.reps, "warmup": args.warmup, "min_count_threshold": THR,
           "hbm_peak_bytes_per_s": HBM_PEAK, "device_copy_bytes_per_s": copy_rate(), "shapes": {}}
    for shp in args.shapes.split(","):
        N, C = (int(v) for v in shp.split("x"))
        doc["shapes"][shp] = bench_shape(N, C, args.reps, args.warmup, not args.no_baseline, args.baseline_pairs)
        print(shp, json.dumps(doc["shapes"][shp]), flush=True)
    txt = json.dumps(doc, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
