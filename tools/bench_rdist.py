#!/usr/bin/env python
"""Timing of ``dist`` (scde_amd/cluster.py, csrc/rdist.hip) against scipy's ``pdist``.

    python tools/bench_rdist.py [--shapes 1000x1000,3000x3000,10000x3000,20000x1000]
                                [--methods euclidean,manhattan] [--reps 3] [--warmup 1]
                                [--scipy-rows 3000] [--out profiles/rdist_bench.json]

Per shape n x p and method, on a standard normal matrix: the median wall time of the host -> host
call (scde_dist_host: x uploaded, the n x n result read back) and of the resident call
(scde_dist_dev: x and the result in HBM), each ending in the library's stream synchronise; the
pair kernel's own time from the context's HIP events (slot "other": the flag prepass and the
4-byte read of the flag are outside it); the same with one NaN in x, which selects the counting
instantiation; and scipy.spatial.distance.pdist on this machine's CPU, one thread, one run.
pdist's time is linear in the number of pairs, so above --scipy-rows rows it is timed on the first
--scipy-rows rows and scaled by the ratio of pair counts ("scipy_rows" says which; "scipy_ms" is
then an extrapolation).

Operations: three per element and pair (subtract, multiply or absolute value, add), n (n - 1) / 2
pairs -- the lower-triangle tiles; the diagonal tiles' upper halves are computed and not counted.
"of_fp64_vector_peak" is operations / kernel time over 78.6e12, the quoted FP64 vector rate, which
counts a fused multiply-add as two: without one (the contract forbids it) at most half of it,
39.3e12 instructions/s, can be reached.  Prints one JSON document; --out also writes it after
every shape.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"  # the scipy baseline is single-threaded (set before numpy loads)

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 78.6e12
SCIPY_METRIC = {"euclidean": "euclidean", "manhattan": "cityblock", "maximum": "chebyshev"}


def _times_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def kernel_ms(ctx, fn, reps):
    ctx.set_profiling(True)
    out = []
    try:
        for _ in range(reps):
            ctx.reset_kernel_times()
            fn()
            out.append(ctx.kernel_times()["other"][0])
    finally:
        ctx.set_profiling(False)
    return float(np.median(out))


def bench_shape(n, p, methods, reps, warmup, scipy_rows):
    from scipy.spatial.distance import pdist

    from scde_amd import api
    from scde_amd._lib import check, lib
    from scde_amd.cluster import DIST_METHODS
    L, ctx, P = lib(), api.default_context(), api._p
    x = np.asfortranarray(np.random.default_rng(100 * n + p).standard_normal((n, p)))
    out = np.zeros((n, n), order="F")
    xd, od = ctypes.c_void_p(), ctypes.c_void_p()
    check(L.scde_dev_alloc(ctx.handle, x.nbytes, ctypes.byref(xd)))
    check(L.scde_dev_alloc(ctx.handle, out.nbytes, ctypes.byref(od)))
    res = {}
    try:
        check(L.scde_h2d(ctx.handle, xd, P(x), x.nbytes))
        for m in methods:
            code = DIST_METHODS.index(m)
            host = lambda: check(L.scde_dist_host(ctx.handle, P(x), n, n, p, code, P(out)))  # noqa: E731
            resident = lambda: check(L.scde_dist_dev(ctx.handle, xd, n, n, p, code, od))  # noqa: E731
            h_med, h_min = _times_ms(host, reps, warmup)
            r_med, r_min = _times_ms(resident, reps, warmup)
            k_ms = kernel_ms(ctx, resident, reps)
            # one NaN: the counting instantiation on (all but one element of) the same data
            nan = np.array([np.nan])
            check(L.scde_h2d(ctx.handle, xd, P(nan), 8))
            c_med, _ = _times_ms(resident, reps, warmup)
            ck_ms = kernel_ms(ctx, resident, reps)
            check(L.scde_h2d(ctx.handle, xd, P(x), 8))
            rows = min(n, scipy_rows)
            xs = np.ascontiguousarray(x[:rows])
            t0 = time.perf_counter()
            y = pdist(xs, SCIPY_METRIC[m])
            s_ms = (time.perf_counter() - t0) * 1e3 * (n * (n - 1.0)) / (rows * (rows - 1.0))
            ops = 3.0 * p * n * (n - 1) / 2
            res[m] = {"host_to_host_ms": h_med, "host_to_host_min_ms": h_min, "resident_ms": r_med,
                      "resident_min_ms": r_min, "kernel_ms": k_ms, "counting_resident_ms": c_med,
                      "counting_kernel_ms": ck_ms, "operations": ops, "tera_ops_per_s": ops / (k_ms * 1e-3) / 1e12,
                      "of_fp64_vector_peak": ops / (k_ms * 1e-3) / PEAK,
                      "of_peak_without_fma": ops / (k_ms * 1e-3) / (PEAK / 2),
                      "x_read_GBps_if_once": x.nbytes / (k_ms * 1e-3) / 1e9,
                      "out_write_GBps": out.nbytes / (k_ms * 1e-3) / 1e9,
                      "scipy_ms": s_ms, "scipy_rows": rows, "scipy_runs": 1,
                      "scipy_over_host_to_host": s_ms / h_med, "scipy_over_resident": s_ms / r_med,
                      "check_first_pair": [float(out[1, 0]), float(y[0])]}
            print(f"# {n} x {p} {m}: {json.dumps(res[m])}", file=sys.stderr, flush=True)
    finally:
        L.scde_dev_free(ctx.handle, xd)
        L.scde_dev_free(ctx.handle, od)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="1000x1000,3000x3000,10000x3000,20000x1000")
    ap.add_argument("--methods", default="euclidean,manhattan")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--scipy-rows", type=int, default=3000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    doc = {"tool": "tools/bench_rdist.py", "reps": args.reps, "warmup": args.warmup, "fp64_vector_peak": PEAK,
           "shapes": {}}

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
    for shape in args.shapes.split(","):
        n, p = (int(v) for v in shape.split("x"))
        doc["shapes"][shape] = bench_shape(n, p, args.methods.split(","), args.reps, args.warmup, args.scipy_rows)
        write()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
