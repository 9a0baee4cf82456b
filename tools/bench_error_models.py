#!/usr/bin/env python
"""Timing of scde.error.models (scde_amd/error_models.py; csrc/error_models.hip, csrc/nb2_fit.hip,
csrc/knn_fit.hip).

    python tools/bench_error_models.py [--out profiles/error_models_bench.json] [--shapes 2000x200,20000x1000]
                                       [--reps 3] [--warmup 1] [--no-baseline] [--baseline-cells 3]

Per shape (genes x cells, bench.py's synthetic counts in two equal groups; the defaults of
scde.error.models: min.count.threshold 4, min.nonfailed 3, max.pairs 5000, min.pairs.per.cell 10,
seed 1 where a group has more pairs than that), host -> host (every call ends in the library's
stream synchronise; a warm-up, then the median of --reps):

  * inputs         error_model_inputs with the pairs and the library sizes given (both are host
                   work, timed apart as pairs_ms and library_sizes_ms): the counts go up, fpm, the
                   starting posteriors and nabove come back
  * inputs_kernel  k_crossfit_inputs + k_crossfit_prior alone, from the context's HIP events
  * fit            per linear_fit value, the fit on those inputs from host counts (nb2_fit_models,
                   knn_fit_models): fpm, the starting posteriors and the counts go up, the models
                   come back; fit_kernel is its kernel alone
  * whole          scde_error_models itself, counts to models (pairs and library sizes included)

The baseline is the tests' numpy restatement (tests/error_models_ref.py closed_inputs and
fit_cell_nb2, tests/knn_fit_ref.py fit_cell) on one CPU thread, timed on the first
--baseline-cells cells and scaled to all cells by their share of the valid genes (labelled so).
A stage slower than numpy is reported as such; no threshold is set.  Prints one JSON document and
writes it to --out.
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

from bench_varnorm import _kernel_ms, _median_ms  # noqa: E402

THR, MIN_NONFAILED, SEED = 4, 3, 1


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def bench_shape(N, C, reps, warmup, baseline, baseline_cells):
    import bench
    import error_models_ref as E
    import knn_fit_ref as F
    from scde_amd import api, error_models as EM, knn
    _, counts, groups = bench.synthetic(9300 + N % 991, N, C, two_groups=True)
    ctx = api.default_context()
    mse = min(2000, N)
    pairs, pairs_ms = _timed(lambda: EM.crossfit_pairs(groups, seed=SEED))
    ls, ls_ms = _timed(lambda: knn.estimate_library_sizes(counts, mse, THR))
    keep = {}

    def inputs():
        keep["inputs"] = EM.error_model_inputs(counts, groups=groups, pairs=pairs, library_sizes=ls, ctx=ctx)

    r = {"pairs": int(pairs.shape[1]), "pairs_ms": pairs_ms, "library_sizes_ms": ls_ms}
    r["inputs_ms"] = _median_ms(inputs, reps, warmup)
    r["inputs_kernel_ms"] = _kernel_ms(ctx, inputs, reps)
    inp = keep["inputs"]
    nv = inp["vi"].sum(axis=0)
    r["valid_genes_per_cell"] = [int(nv.min()), int(np.median(nv)), int(nv.max())]
    fits = {"linear_fit_false": lambda **kw: EM.nb2_fit_models(inp, counts, ctx=ctx, **kw),
            "linear_fit_true": lambda **kw: knn.knn_fit_models(inp, counts, ctx=ctx, **kw)}
    for name, fit in fits.items():
        f = {"fit_ms": _median_ms(fit, reps, warmup), "fit_kernel_ms": _kernel_ms(ctx, fit, reps)}
        mm, det = fit(return_details=True)
        keep[name] = (mm, det)
        f["failed_cells"] = int(np.sum(det["status"] != 0))
        f["em_iterations"] = [int(det["iterations"].min()), float(np.median(det["iterations"])),
                              int(det["iterations"].max())]
        linear = name == "linear_fit_true"

        def whole():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                EM.scde_error_models(counts, groups=groups, linear_fit=linear, seed=SEED, min_size_entries=mse, ctx=ctx)
        f["whole_ms"] = _median_ms(whole, reps, warmup)
        r[name] = f
    if baseline:
        bc = min(C, baseline_cells)
        genes = float(nv[:bc].sum())
        scale = float(nv.sum()) / genes if genes else float("nan")
        codes = np.asarray(groups)
        # the input stage of the first cells' group, restricted to those cells' columns of the result
        first = np.flatnonzero(codes == codes[0])
        gp = [(int(a), int(b)) for a, b in pairs.T if codes[a] == codes[0]]
        _, ms = _timed(lambda: E.closed_inputs(counts, [int(c) for c in first], gp, ls, THR, MIN_NONFAILED))
        r["numpy_inputs_ms"] = ms * C / len(first)
        r["numpy_inputs_note"] = (f"closed_inputs on the first group ({len(first)} cells, {ms:.0f} ms), scaled to "
                                  f"{C} cells")
        r["inputs_slower_than_numpy"] = bool(r["inputs_ms"] > r["numpy_inputs_ms"])
        for name, ref_fit in (("linear_fit_false", lambda y, x, p: E.fit_cell_nb2(y, x, p)),
                              ("linear_fit_true", lambda y, x, p: F.fit_cell(y, x, p))):
            t0 = time.perf_counter()
            ref = []
            with np.errstate(all="ignore"):
                for i in range(bc):
                    v = inp["vi"][:, i]
                    ref.append(ref_fit(counts[v, i], inp["fpm"][v, i], inp["fail_prior"][v, i]))
            ms = (time.perf_counter() - t0) * 1e3
            f = r[name]
            mm, det = keep[name]
            f["numpy_fit_ms"] = ms * scale
            f["numpy_note"] = f"timed on the first {bc} cells ({ms:.0f} ms), scaled by their share of the valid genes"
            f["numpy_over_library"] = f["numpy_fit_ms"] / f["fit_ms"]
            ok = [i for i in range(bc) if ref[i]["status"] == 0 and det["status"][i] == 0]
            f["max_abs_difference_corr_b"] = float(max((abs(ref[i]["row"][3] - mm[i, 3]) for i in ok), default=0.0))
            f["iterations_equal"] = bool(all(ref[i]["iterations"] == det["iterations"][i] for i in range(bc)))
            f["slower_than_numpy"] = bool(f["fit_ms"] > f["numpy_fit_ms"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2000x200,20000x1000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--baseline-cells", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "error_models_bench.json"))
    args = ap.parse_args()
    doc = {"tool": "tools/bench_error_models.py", "reps": args.reps, "warmup": args.warmup, "min_count_threshold": THR,
           "min_nonfailed": MIN_NONFAILED, "seed": SEED, "shapes": {}}
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
