#!/usr/bin/env python
"""Timing of knn.error.models' mixture fit (scde_amd/knn.py knn_fit_models, csrc/knn_fit.hip).

    python tools/bench_knn_fit.py [--out profiles/knn_fit_bench.json] [--shapes 2000x200,20000x1000,20000x3000]
                                  [--reps 3] [--warmup 1] [--no-baseline] [--baseline-cells 3]

Per shape (genes x cells, bench.py's synthetic counts, k = cells / 4 and min.count.threshold 2 as
in the vignette), the model inputs come from knn_model_inputs (not timed here: tools/bench_knn.py).
Then, host -> host (the call ends in the library's stream synchronise; a warm-up, then the
median of --reps):

  * fit          knn_fit_models from host counts: fpm, the starting posteriors and the counts
                 go up, the models come back
  * fit_kernel   k_knn_fit alone, from the context's HIP events

The baseline is tests/knn_fit_ref.py, the numpy restatement, on one CPU thread, timed on the
first --baseline-cells cells and scaled to all cells (labelled so).  Its pass counters give the
work: genes visited by each kind of pass, times a source-level operation count per gene (a
library exp, log or log1p counted as 20 operations, a division as 10, an FMA as two: an
estimate, not a counter reading), over the kernel's time, as a share of the FP64 vector peak.
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
    os.environ[_v] = "1"   # the baseline is one CPU thread

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from bench_tsne import FP64_VECTOR_PEAK  # noqa: E402
from bench_varnorm import _kernel_ms, _median_ms  # noqa: E402

THR = 2
# FP64 operations per gene of each pass, counted in csrc/knn_fit.hip's loops as the text above says
OPS = {"concomitant_objective": 100, "concomitant_newton": 95, "theta": 50, "curve": 190, "e_step": 420}


def bench_shape(N, C, reps, warmup, baseline, baseline_cells):
    import bench
    import knn_fit_ref as F
    from scde_amd import api, knn
    _, counts, _ = bench.synthetic(9100 + N % 991, N, C, two_groups=True)
    ctx = api.default_context()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        inputs = knn.knn_model_inputs(counts, k=C // 4, min_count_threshold=THR, min_size_entries=min(2000, N))
    nv = inputs["vi"].sum(axis=0)
    keep = {}

    def fit():
        keep["mm"], keep["det"] = knn.knn_fit_models(inputs, counts, return_details=True, ctx=ctx)

    def fit_plain():
        keep["mm"] = knn.knn_fit_models(inputs, counts, ctx=ctx)

    r = {"k": C // 4, "valid_genes_per_cell": [int(nv.min()), int(np.median(nv)), int(nv.max())]}
    r["fit_ms"] = _median_ms(fit_plain, reps, warmup)
    r["fit_kernel_ms"] = _kernel_ms(ctx, fit_plain, reps)
    fit()
    det = keep["det"]
    r["failed_cells"] = int(np.sum(det["status"] != 0))
    r["em_iterations"] = [int(det["iterations"].min()), float(np.median(det["iterations"])),
                          int(det["iterations"].max())]
    if baseline:
        bc = min(C, baseline_cells)
        F.PASSES.clear()
        t0 = time.perf_counter()
        with np.errstate(all="ignore"):
            ref = F.fit_cells(counts, inputs["fpm"], inputs["fail_prior"], cells=range(bc))
        ms = (time.perf_counter() - t0) * 1e3
        genes = float(nv[:bc].sum())
        scale = float(nv.sum()) / genes if genes else float("nan")
        r["numpy_fit_ms"] = ms * scale
        r["numpy_note"] = f"timed on the first {bc} cells ({ms:.0f} ms), scaled by their share of the valid genes"
        r["numpy_over_library"] = r["numpy_fit_ms"] / r["fit_ms"]
        ok = [i for i in range(bc) if ref[i]["status"] == 0 and det["status"][i] == 0]
        r["max_abs_difference_corr_b"] = float(max((abs(ref[i]["row"][3] - keep["mm"][i, 3]) for i in ok), default=0.0))
        r["iterations_equal"] = bool(all(ref[i]["iterations"] == det["iterations"][i] for i in range(bc)))
        ops = sum(OPS[k] * v for k, v in F.PASSES.items()) * scale
        r["passes_genes_baseline_cells"] = dict(F.PASSES)
        r["estimated_fp64_operations"] = ops
        if r["fit_kernel_ms"] > 0:
            r["estimated_fp64_operations_per_s"] = ops / (r["fit_kernel_ms"] * 1e-3)
            r["estimated_share_of_fp64_vector_peak"] = r["estimated_fp64_operations_per_s"] / FP64_VECTOR_PEAK
        r["slower_than_numpy"] = bool(r["fit_ms"] > r["numpy_fit_ms"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2000x200,20000x1000,20000x3000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--baseline-cells", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_fit_bench.json"))
    args = ap.parse_args()
    doc = {"tool": "tools/bench_knn_fit.py", "reps": args.reps, "warmup": args.warmup, "min_count_threshold": THR,
           "fp64_vector_peak_flop_per_s": FP64_VECTOR_PEAK, "operations_per_gene_and_pass": OPS, "shapes": {}}
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
