#!/usr/bin/env python
"""Timing of the mixture cross-fit of cell pairs (scde_amd/error_models.py crossfit_models and
crossfit=; csrc/crossfit_fit.hip, csrc/error_models.hip).

    python tools/bench_crossfit.py [--out profiles/crossfit_bench.json] [--shapes 2000x200,20000x1000]
                                   [--reps 3] [--warmup 1] [--no-baseline] [--baseline-pairs 3]

Per shape (genes x cells, bench.py's synthetic counts in two equal groups; scde.error.models'
defaults: min.count.threshold 4, min.nonfailed 3, max.pairs 5000, min.pairs.per.cell 10, seed 1
where a group has more pairs than that), host -> host (every call ends in the library's stream
synchronise; a warm-up, then the median of --reps):

  * pair_fit        the pair fit from host counts with its large results left on the device
                    (status, rounds, llh and parameters come back); pair_fit_kernel is k_crossfit_fit
                    alone, from the context's HIP events
  * pair_fit_fetch  crossfit_models itself, clusters and posteriors brought back too (17 bytes a
                    gene and pair; left out where that is more than --fetch-limit-gb)
  * reduce          the reduction of the resident pair results with the library sizes given:
                    vil, fpm, the fail prior and nabove come back; reduce_kernel its kernels alone
  * whole           scde_error_models(crossfit="mixture", linear_fit=False), counts to models,
                    beside whole_threshold, the same call with the threshold rule

The baseline is tests/crossfit_ref.py, the numpy restatement, on one CPU thread: fit_pair timed
on the first --baseline-pairs pairs and scaled to all pairs by their share of the rows, the
reduction timed on one group and scaled by cells (labelled so).  The kernel's work is estimated
from the restatement's passes over the rows (wrappers count the rows each kind of pass visits)
times a source-level operation count per row (a library exp or log counted as 20 operations,
lgamma, digamma or trigamma as 40, a division as 10, an FMA as two: an estimate, not a counter
reading), over the kernel's time, as a share of the FP64 vector peak.  A stage slower than numpy is
reported as such; no threshold is set.  Prints one JSON document and writes it to --out.
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

THR, MIN_NONFAILED, SEED = 4, 3, 1
# FP64 operations per row of each pass, counted in csrc/crossfit_fit.hip's and nb2_solvers.h's loops
OPS = {"log_pi3": 110, "deviance_and_normal_equations": 150, "theta_newton": 200, "nb_loglik": 190, "e_step": 900}


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


class Passes:
    """Counts the rows the restatement's passes visit, by wrapping its module-level functions."""

    def __init__(self, R, E):
        self.n = {k: 0 for k in OPS}
        self.R, self.E = R, E
        self.saved = {}

    def _wrap(self, mod, name, key, rows):
        fn = getattr(mod, name)
        self.saved[mod, name] = fn

        def counted(*a, **kw):
            self.n[key] += rows(*a, **kw)
            return fn(*a, **kw)
        setattr(mod, name, counted)

    def __enter__(self):
        self._wrap(self.R, "log_pi3", "log_pi3", lambda b, x: np.size(x))
        self._wrap(self.E, "deviance", "deviance_and_normal_equations", lambda y, mu, wt, th: np.size(y))
        self._wrap(self.E, "nb_loglik", "nb_loglik", lambda y, mu, wt, th: np.size(y))
        self._wrap(self.E, "digamma", "theta_newton", lambda v: np.size(v) if np.ndim(v) else 0)
        return self

    def __exit__(self, *exc):
        for (mod, name), fn in self.saved.items():
            setattr(mod, name, fn)


def bench_shape(N, C, reps, warmup, baseline, baseline_pairs, fetch_limit):
    import bench
    import crossfit_ref as R
    import error_models_ref as E
    from scde_amd import api, error_models as EM, knn
    _, counts, groups = bench.synthetic(9300 + N % 991, N, C, two_groups=True)
    counts = knn._host_counts(counts)
    codes = EM._codes(groups, C)[0]
    ctx = api.default_context()
    mse = min(2000, N)
    pairs = EM._check_pairs(EM.crossfit_pairs(groups, seed=SEED), codes)
    P = pairs.shape[1]
    keep = {}

    def pair_fit():
        keep["cf"] = EM._crossfit_fit(None, counts, N, C, pairs, THR, 1e-5, 0.1, 200, 0, ctx.handle, fetch=False)

    r = {"pairs": int(P)}
    r["pair_fit_ms"] = _median_ms(pair_fit, reps, warmup)
    r["pair_fit_kernel_ms"] = _kernel_ms(ctx, pair_fit, 1)
    cf = keep["cf"]
    ok = cf["status"] == 0
    r["failed_pairs"] = {str(int(s)): int(np.sum(cf["status"] == s)) for s in np.unique(cf["status"]) if s != 0}
    r["em_iterations"] = [int(cf["iterations"][ok].min()), float(np.median(cf["iterations"][ok])),
                          int(cf["iterations"][ok].max())] if ok.any() else None
    if 17.0 * N * P <= fetch_limit * 2.0 ** 30:
        r["pair_fit_fetch_ms"] = _median_ms(lambda: EM.crossfit_models(counts, groups, pairs=pairs, ctx=ctx), reps, warmup)
    # the reduction of the resident results (the last pair fit's), library sizes given
    dc = api.DeviceCounts(ctx, counts)
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            EM._crossfit_fit(dc, None, N, C, pairs, THR, 1e-5, 0.1, 200, 0, ctx.handle, fetch=False)
            vil = EM._reduce(dc, None, N, C, codes, None, pairs, None, MIN_NONFAILED, ctx.handle)[0]
            ls, r["library_sizes_ms"] = _timed(lambda: knn.estimate_library_sizes(counts, mse, THR, vil=vil))

            def reduce():
                keep["red"] = EM._reduce(dc, None, N, C, codes, None, pairs, ls, MIN_NONFAILED, ctx.handle)
            r["reduce_ms"] = _median_ms(reduce, reps, warmup)
            r["reduce_kernel_ms"] = _kernel_ms(ctx, reduce, reps)
    finally:
        dc.free()
    nv = (~np.isnan(keep["red"][2])).sum(axis=0)
    r["valid_genes_per_cell"] = [int(nv.min()), int(np.median(nv)), int(nv.max())]

    def whole(**kw):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            EM.scde_error_models(counts, groups=groups, linear_fit=False, seed=SEED, min_size_entries=mse, ctx=ctx, **kw)
    r["whole_ms"] = _median_ms(lambda: whole(crossfit="mixture"), reps, warmup)
    r["whole_threshold_ms"] = _median_ms(whole, reps, warmup)
    if baseline:
        bp = min(P, baseline_pairs)
        rows_all = None
        t0 = time.perf_counter()
        with Passes(R, E) as passes, np.errstate(all="ignore"):
            fits = [R.fit_pair(counts[:, i], counts[:, j], thr=THR) for i, j in pairs[:, :bp].T]
        ms = (time.perf_counter() - t0) * 1e3
        rows = np.array([len(f["rows"]) for f in fits], np.float64)
        # every pair's rows: the genes either cell detected
        det = counts > 0
        rows_all = np.array([np.count_nonzero(det[:, i] | det[:, j]) for i, j in pairs.T], np.float64)
        scale = float(rows_all.sum() / rows.sum())
        r["rows_per_pair"] = [int(rows_all.min()), float(np.median(rows_all)), int(rows_all.max())]
        r["numpy_pair_fit_ms"] = ms * scale
        r["numpy_note"] = f"fit_pair timed on the first {bp} pairs ({ms:.0f} ms), scaled by their share of the rows"
        r["numpy_over_library"] = r["numpy_pair_fit_ms"] / r["pair_fit_ms"]
        r["pair_fit_slower_than_numpy"] = bool(r["pair_fit_ms"] > r["numpy_pair_fit_ms"])
        r["baseline_status_equal"] = bool(all(f["status"] == cf["status"][k] for k, f in enumerate(fits)))
        r["baseline_iterations_equal"] = bool(all(f["iterations"] == cf["iterations"][k] for k, f in enumerate(fits)))
        okb = [k for k, f in enumerate(fits) if f["status"] == 0 and cf["status"][k] == 0]
        r["max_abs_difference_a_c0"] = float(max((abs(fits[k]["params"][4] - cf["params"][k, 4]) for k in okb),
                                                 default=0.0))
        n = dict(passes.n)
        n["e_step"] = int(sum(len(f["rows"]) * f["iterations"] for f in fits))
        ops = sum(OPS[k] * v for k, v in n.items()) * scale
        r["passes_rows_baseline_pairs"] = n
        r["estimated_fp64_operations"] = ops
        if r["pair_fit_kernel_ms"] > 0:
            r["estimated_fp64_operations_per_s"] = ops / (r["pair_fit_kernel_ms"] * 1e-3)
            r["estimated_share_of_fp64_vector_peak"] = r["estimated_fp64_operations_per_s"] / FP64_VECTOR_PEAK
        # the reduction: one group of the restatement, scaled by cells
        first = [int(c) for c in np.flatnonzero(codes == codes[0])]
        sub = np.flatnonzero(codes[pairs[0]] == codes[0])[:200]  # (a slice of the pair list bounds the host's memory)
        small = EM.crossfit_models(counts, groups, pairs=np.ascontiguousarray(pairs[:, sub]), ctx=ctx)
        _, ms = _timed(lambda: R.reduce_group(counts, first, small, np.asarray(ls), MIN_NONFAILED))
        per_entry = ms / max(1, 2 * len(sub))
        r["numpy_reduce_ms"] = per_entry * 2 * P
        r["numpy_reduce_note"] = (f"reduce_group on {len(sub)} pairs of the first group ({ms:.0f} ms), scaled to "
                                  f"{P} pairs")
        r["reduce_slower_than_numpy"] = bool(r["reduce_ms"] > r["numpy_reduce_ms"])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2000x200,20000x1000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--baseline-pairs", type=int, default=3)
    ap.add_argument("--fetch-limit-gb", type=float, default=1.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crossfit_bench.json"))
    args = ap.parse_args()
    doc = {"tool": "tools/bench_crossfit.py", "reps": args.reps, "warmup": args.warmup, "min_count_threshold": THR,
           "min_nonfailed": MIN_NONFAILED, "seed": SEED, "fp64_vector_peak_flop_per_s": FP64_VECTOR_PEAK,
           "operations_per_row_and_pass": OPS, "shapes": {}}
    for shp in args.shapes.split(","):
        N, C = (int(v) for v in shp.split("x"))
        doc["shapes"][shp] = bench_shape(N, C, args.reps, args.warmup, not args.no_baseline, args.baseline_pairs,
                                         args.fetch_limit_gb)
        print(shp, json.dumps(doc["shapes"][shp]), flush=True)
    txt = json.dumps(doc, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
