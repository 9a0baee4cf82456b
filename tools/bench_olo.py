#!/usr/bin/env python
"""Timing of the optimal leaf ordering (scde_amd.cluster.order_optimal, csrc/olo.hip) against
scipy.cluster.hierarchy.optimal_leaf_ordering.

    python tools/bench_olo.py [--sizes 1000,3000,10000] [--methods ward.D,single] [--reps 3]
                              [--warmup 1] [--part both|device|scipy] [--scipy-timeout 600]
                              [--caterpillar 1000,3000,10000]
                              [--out profiles/olo_bench.json]

Per size n and linkage, on the Euclidean distances of n points around Gaussian cluster centres
(ward.D gives a bushy tree, single linkage on the same points the deep one):

  device  the tree from scde_amd.hclust (not timed), then the median wall time of the host ->
          host call (scde_order_optimal_host: matrix staged by the library, workspace allocated
          and freed inside, results back on the host) and of the resident call
          (scde_order_optimal_dev); the launches and the candidates (one float64 add and one min
          each) the library counted, the candidates per second of the host -> host call and its
          share of the FP64 vector peak; the tree's depth in levels; the path length before and
          after
  scipy   optimal_leaf_ordering on scipy's own linkage of the same distances (ward.D is scipy's
          "ward" on sqrt(d)), one CPU thread, one run in a fresh process that is ended after
          --scipy-timeout seconds (the size is then recorded as skipped); its time and the path
          length of the order it returned

The device part also times the deepest tree there is: single linkage of n points on a line with
growing gaps, a caterpillar of n - 1 levels and about 3 n launches.

The two parts may run separately (--part) into the same --out file, which is read first and
updated.  Prints one JSON document.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"  # the scipy baseline is single-threaded (set before numpy loads)

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# 256 CUs x 4 SIMDs x 16 FP64 lanes per clock x 2.4 GHz = 39.3e12 FP64 vector instructions per
# second (the 78.6 TFLOP/s vector peak counts an FMA as two); a candidate is two instructions
PEAK_CANDIDATES_PER_S = 256 * 4 * 16 * 2.4e9 / 2
SCIPY_METHOD = {"ward.D": "ward", "single": "single", "complete": "complete", "average": "average"}


def distance_matrix(n, line=False):
    if line:  # points on a line with growing gaps: single linkage gives a caterpillar of n - 1 levels
        x = np.cumsum(1.0 + 1e-4 * np.arange(n))
        return np.asfortranarray(np.abs(x[:, None] - x[None, :]))
    rng = np.random.default_rng(5100 + n)
    centres = rng.normal(0, 4, (8, 5))
    x = centres[rng.integers(0, 8, n)] + rng.normal(0, 1, (n, 5))
    sq = (x * x).sum(1)
    d = np.sqrt(np.maximum(sq[:, None] + sq[None, :] - 2 * x @ x.T, 0))
    d = (d + d.T) / 2
    np.fill_diagonal(d, 0.0)
    return np.asfortranarray(d)


def path_length(d, order):
    from scde_amd.cluster import leaf_order_length
    return float(leaf_order_length(d, order))


def _median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def levels(merge):
    lv = np.zeros(len(merge), np.int64)
    for s, row in enumerate(np.asarray(merge).tolist()):
        lv[s] = 1 + max(0 if v < 0 else lv[v - 1] for v in row)
    return int(lv.max())


def bench_device(n, method, reps, warmup, line=False):
    import ctypes

    from scde_amd import api, hclust
    from scde_amd._lib import check, lib
    L, ctx, P = lib(), api.default_context(), api._p
    d = distance_matrix(n, line)
    hc = hclust(d, method=method, ctx=ctx)
    merge = np.asfortranarray(hc.merge, dtype=np.int32)
    merge_out, order = np.zeros((n - 1, 2), np.int32, order="F"), np.zeros(n, np.int32)
    length = ctypes.c_double()
    host = lambda: check(L.scde_order_optimal_host(ctx.handle, P(d), n, n, P(merge), P(merge_out),  # noqa: E731
                                                   P(order), ctypes.byref(length)))
    h_med, h_min = _median_ms(host, reps, warmup)
    ptr = ctypes.c_void_p()
    check(L.scde_dev_alloc(ctx.handle, d.nbytes, ctypes.byref(ptr)))
    try:
        check(L.scde_h2d(ctx.handle, ptr, P(d), d.nbytes))
        resident = lambda: check(L.scde_order_optimal_dev(ctx.handle, ptr, n, n, P(merge), P(merge_out),  # noqa: E731
                                                          P(order), ctypes.byref(length)))
        r_med, r_min = _median_ms(resident, reps, warmup)
    finally:
        check(L.scde_dev_free(ctx.handle, ptr))
    stat = ctypes.c_double()
    check(L.scde_ctx_get_stat(ctx.handle, b"olo_launches", ctypes.byref(stat)))
    launches = stat.value
    check(L.scde_ctx_get_stat(ctx.handle, b"olo_candidates", ctypes.byref(stat)))
    cand = stat.value
    assert length.value == path_length(d, order)
    return {"host_to_host_ms": h_med, "host_to_host_min_ms": h_min, "resident_ms": r_med, "resident_min_ms": r_min,
            "launches": launches, "levels": levels(hc.merge), "candidates": cand,
            "candidates_per_s": cand / (h_med * 1e-3), "resident_candidates_per_s": cand / (r_med * 1e-3),
            "fraction_of_fp64_vector_peak": cand / (h_med * 1e-3) / PEAK_CANDIDATES_PER_S,
            "resident_fraction_of_fp64_vector_peak": cand / (r_med * 1e-3) / PEAK_CANDIDATES_PER_S,
            "length": length.value, "length_before": path_length(d, hc.order)}


def scipy_child(n, method):
    """One run of scipy's optimal_leaf_ordering; prints a JSON line."""
    from scipy.cluster.hierarchy import leaves_list, linkage, optimal_leaf_ordering
    from scipy.spatial.distance import squareform
    d = distance_matrix(n)
    y = squareform(d, checks=False)
    z = linkage(np.sqrt(y) if method == "ward.D" else y, SCIPY_METHOD[method])
    before = path_length(d, leaves_list(z) + 1)
    t0 = time.perf_counter()
    z2 = optimal_leaf_ordering(z, y)
    ms = (time.perf_counter() - t0) * 1e3
    print(json.dumps({"scipy_ms": ms, "scipy_length": path_length(d, leaves_list(z2) + 1),
                      "scipy_length_before": before}))


def bench_scipy(n, method, timeout):
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--scipy-child", f"{n}:{method}"],
                           capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired:
        return {"scipy_skipped": f"not finished in {timeout:g} s"}
    if r.returncode != 0:
        return {"scipy_skipped": "failed: " + r.stderr.strip().splitlines()[-1] if r.stderr.strip() else "failed"}
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,3000,10000")
    ap.add_argument("--methods", default="ward.D,single")
    ap.add_argument("--caterpillar", default="1000,3000,10000", help="sizes of the caterpillar case (device part)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--part", default="both", choices=["both", "device", "scipy"])
    ap.add_argument("--scipy-timeout", type=float, default=600.0)
    ap.add_argument("--scipy-child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.scipy_child:
        n, method = args.scipy_child.split(":")
        return scipy_child(int(n), method)
    doc = {"tool": "tools/bench_olo.py", "runs": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc.update(reps=args.reps, warmup=args.warmup, fp64_vector_peak_candidates_per_s=PEAK_CANDIDATES_PER_S)

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
    for n in (int(v) for v in args.sizes.split(",") if v):
        for m in args.methods.split(","):
            run = doc["runs"].setdefault(str(n), {}).setdefault(m, {})
            if args.part in ("both", "device"):
                run.update(bench_device(n, m, args.reps, args.warmup))
            if args.part in ("both", "scipy"):
                for k in [k for k in run if k.startswith("scipy_")]:
                    del run[k]
                run.update(bench_scipy(n, m, args.scipy_timeout))
            if "scipy_ms" in run and "host_to_host_ms" in run:
                run["scipy_over_host_to_host"] = run["scipy_ms"] / run["host_to_host_ms"]
                run["scipy_length_over_ours"] = run["scipy_length"] / run["length"]
            print(f"# n={n} {m}: {json.dumps(run)}", file=sys.stderr, flush=True)
            write()
    if args.part in ("both", "device"):
        for n in (int(v) for v in args.caterpillar.split(",") if v):
            doc.setdefault("caterpillar", {})[str(n)] = bench_device(n, "single", args.reps, args.warmup, line=True)
            print(f"# caterpillar n={n}: {json.dumps(doc['caterpillar'][str(n)])}", file=sys.stderr, flush=True)
            write()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
