#!/usr/bin/env python
"""Timing of knn.error.models' neighbourhood stage (scde_amd/knn.py, csrc/knn.hip).

    python tools/bench_knn.py [--out profiles/knn_bench.json] [--shapes 2000x200,20000x1000,20000x3000]
                              [--reps 3] [--warmup 1] [--no-baseline] [--baseline-cells 4]

Per shape (genes x cells, bench.py's synthetic counts, k = cells / 4 as in the vignette,
min.count.threshold 2 as there, trim 0.25), host -> host wall times (each call ends in the
library's stream synchronise; a warm-up, then the median of --reps), with the counts resident:

  * similarity   prep + the six Gram products, the C x C result read back
  * neighbours   the counting kernel on the resident similarity, the lists read back
  * magnitudes   the trimmed means on the resident lists, fpm and nabove read back
  * statistics   the host part: library sizes (TMM), vi, the starting posteriors
  * chain        knn_model_inputs from host counts (upload included)

and the kernels' own times from the context's HIP events.  The magnitudes kernel's rate is given
as the bytes it must move over its time (counts read once, the lists once, fpm and nabove
written) beside a device-to-device copy of 1 GiB timed in the same run, and as neighbour visits
(genes x cells x k) per second: it is bound by the visits, not by the bytes.

The baseline is tests/knn_ref.py, the numpy restatement, on one CPU thread.  Its magnitudes are
timed on the first --baseline-cells cells and scaled to all cells, and its similarity on at most
500 cells and scaled by the square of the ratio; both are labelled so in the result.
Prints one JSON document and writes it to --out.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
import warnings

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"   # the baseline is one CPU thread; the library's host code does not use them

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_varnorm import HBM_PEAK, _kernel_ms, _median_ms, copy_rate  # noqa: E402

THR, TRIM = 2, 0.25


def bench_shape(N, C, reps, warmup, baseline, baseline_cells):
    import bench
    import knn_ref as R
    from scde_amd import api, knn
    _, counts, _ = bench.synthetic(9100 + N % 991, N, C, two_groups=True)
    ctx = api.default_context()
    k = C // 4
    mse = min(2000, N)
    keep = {}
    r = {"k": k, "zeros": float(np.mean(counts == 0))}

    def lib_sizes():
        keep["ls"] = knn.estimate_library_sizes(counts, mse, THR)

    r["library_sizes_ms"] = _median_ms(lib_sizes, reps, warmup)
    ls = keep["ls"]
    dc = api.DeviceCounts(ctx, counts)
    try:
        def similarity():
            keep["sim"] = knn.knn_cell_similarity(dc, THR)

        def neighbours():
            keep["nb"] = knn._neighbours(None, C, k, None, ctx.handle)

        def magnitudes():
            keep["fpm"], keep["na"] = knn._magnitudes(dc, None, N, C, None, k, ls, THR, TRIM, ctx.handle)

        for name, fn in (("similarity", similarity), ("neighbours", neighbours), ("magnitudes", magnitudes)):
            r[name + "_ms"] = _median_ms(fn, reps, warmup)
            r[name + "_kernel_ms"] = _kernel_ms(ctx, fn, reps)
    finally:
        dc.free()
    fpm, na, nb = keep["fpm"], keep["na"], keep["nb"]

    def selection():
        with np.errstate(invalid="ignore"):
            vi = (na >= 5) & (fpm > 0)
        keep["vi"], keep["fp"] = vi, knn.fail_priors(counts, fpm, vi, THR)

    r["selection_ms"] = _median_ms(selection, reps, warmup)
    r["statistics_ms"] = r["library_sizes_ms"] + r["selection_ms"]

    def chain():
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            keep["res"] = knn.knn_model_inputs(counts, k=k, min_count_threshold=THR, min_size_entries=mse,
                                               fpm_estimate_trim=TRIM)

    r["chain_ms"] = _median_ms(chain, reps, warmup)
    r["vi_genes_per_cell"] = [int(keep["vi"].sum(0).min()), int(keep["vi"].sum(0).max())]
    nc = float(N) * C
    kms = r["magnitudes_kernel_ms"]
    r["magnitudes_bytes"] = nc * (4 + 8 + 4) + 4.0 * C * k
    r["magnitudes_visits"] = nc * k
    if kms > 0:
        r["magnitudes_bytes_per_s"] = r["magnitudes_bytes"] / (kms * 1e-3)
        r["magnitudes_share_of_hbm_peak"] = r["magnitudes_bytes_per_s"] / HBM_PEAK
        r["magnitudes_visits_per_s"] = r["magnitudes_visits"] / (kms * 1e-3)
    if baseline:
        b = {}
        t0 = time.perf_counter()
        R.estimate_library_sizes(counts, mse, THR)
        b["library_sizes_ms"] = (time.perf_counter() - t0) * 1e3
        cs = min(C, 500)
        t0 = time.perf_counter()
        with np.errstate(all="ignore"):
            R.similarity(counts[:, :cs], THR)
        b["similarity_ms"] = (time.perf_counter() - t0) * 1e3 * (C / cs) ** 2
        b["similarity_note"] = f"timed on {cs} cells, scaled by ({C} / {cs})^2" if cs < C else "all cells"
        t0 = time.perf_counter()
        rnb = R.neighbours(keep["sim"], k)
        b["neighbours_ms"] = (time.perf_counter() - t0) * 1e3
        r["neighbours_equal_restatement"] = bool(np.array_equal(rnb, nb))
        bc = min(C, baseline_cells)
        t0 = time.perf_counter()
        rf, rn = _magnitudes_of_cells(R, counts, nb, ls, bc)
        b["magnitudes_ms"] = (time.perf_counter() - t0) * 1e3 * (C / bc)
        b["magnitudes_note"] = f"timed on the first {bc} cells, scaled by {C} / {bc}"
        with np.errstate(all="ignore"):
            ok = np.isfinite(rf)
            r["max_rel_difference_fpm"] = float(np.max(np.abs(fpm[:, :bc][ok] / rf[ok] - 1), initial=0.0))
        r["nan_positions_equal"] = bool(np.array_equal(np.isnan(rf), np.isnan(fpm[:, :bc])))
        r["nabove_equal"] = bool(np.array_equal(rn, na[:, :bc]))
        t0 = time.perf_counter()
        vi = R.valid_genes(fpm, na, 5, 0)
        R.fail_prior(counts, fpm, vi, THR)
        b["selection_ms"] = (time.perf_counter() - t0) * 1e3
        b["statistics_ms"] = b["library_sizes_ms"] + b["selection_ms"]
        b["stages_ms"] = b["similarity_ms"] + b["neighbours_ms"] + b["magnitudes_ms"] + b["statistics_ms"]
        r["numpy"] = b
        r["stages_ms"] = r["similarity_ms"] + r["neighbours_ms"] + r["magnitudes_ms"] + r["statistics_ms"]
        r["numpy_over_library"] = {s: b[s + "_ms"] / r[s + "_ms"]
                                   for s in ("similarity", "neighbours", "magnitudes", "statistics", "stages")}
    return r


def _magnitudes_of_cells(R, counts, nb, ls, bc):
    """The restatement's fpm and nabove of the first bc cells (genes x bc)."""
    N = counts.shape[0]
    fpm, na = np.full((N, bc), np.nan), np.zeros((N, bc), np.int32)
    for i in range(bc):
        oc = nb[i][nb[i] >= 0]
        sub = counts[:, oc]
        na[:, i] = (sub > THR).sum(axis=1)
        with np.errstate(divide="ignore", invalid="ignore"):
            val = sub / ls[oc]
        ok = sub >= THR
        for g in range(N):
            fpm[g, i] = R.trimmed_mean(val[g, ok[g]], TRIM)
    return fpm, na


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2000x200,20000x1000,20000x3000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--baseline-cells", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_bench.json"))
    args = ap.parse_args()
    doc = {"tool": "tools/bench_knn.py", "reps": args.reps, "warmup": args.warmup, "min_count_threshold": THR,
           "trim": TRIM, "hbm_peak_bytes_per_s": HBM_PEAK, "device_copy_bytes_per_s": copy_rate(), "shapes": {}}
    for shp in args.shapes.split(","):
        N, C = (int(v) for v in shp.split("x"))
        doc["shapes"][shp] = bench_shape(N, C, args.reps, args.warmup, not args.no_baseline, args.baseline_cells)
        print(shp, json.dumps(doc["shapes"][shp]), flush=True)
    txt = json.dumps(doc, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
