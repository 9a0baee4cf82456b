#!/usr/bin/env python
"""Timing of the hierarchical clustering (scde_amd/cluster.py, csrc/hclust.hip) against scipy.

    python tools/bench_hclust.py [--sizes 1000,3000,10000,20000] [--methods ward.D,complete]
                                 [--reps 5] [--warmup 1] [--batch 60x2000]
                                 [--out profiles/hclust_bench.json]

Per size n and method, on the distance matrix 1 - cor of n random 12-vectors: the median wall
time of the host -> host call (scde_hclust_host: the n x n matrix staged by the library) and of
the device-resident call (scde_hclust_dev: the matrix in HBM; merge, height and order still
return to the host), each ending in the library's stream synchronise; the kernel's own time
from the context's HIP events (slot "other"); and scipy.cluster.hierarchy.linkage on the same
matrix (condensed form prepared outside the timed region) on this machine's CPU, one thread.
ward.D is scipy's "ward" on sqrt(d).  Then a batch of problems in one launch
(scde_hclust_batch_dev, matrices resident) against scipy run over the same problems in turn.
Prints one JSON document; --out also writes it (after every size, so a run cut short keeps what
it measured).
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

SCIPY_METHOD = {"ward.D": "ward", "ward.D2": "ward", "single": "single", "complete": "complete",
                "average": "average", "mcquitty": "weighted"}


def _times_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def distance_matrix(n, seed):
    rng = np.random.default_rng(seed)
    d = 1.0 - np.corrcoef(rng.standard_normal((n, 12)))
    np.fill_diagonal(d, 0.0)
    return np.asfortranarray(np.maximum(d, d.T))  # symmetric; both libraries see the same values


def condensed(d):
    from scipy.spatial.distance import squareform
    return squareform(d, checks=False)


def scipy_ms(y, method, reps):
    from scipy.cluster.hierarchy import linkage
    if method == "ward.D":
        y = np.sqrt(y)
    return _times_ms(lambda: linkage(y, SCIPY_METHOD[method]), reps, 0)


class Resident:
    def __init__(self, ctx, a):
        from scde_amd._lib import check, lib
        self.ctx, self.ptr = ctx, ctypes.c_void_p()
        check(lib().scde_dev_alloc(ctx.handle, a.nbytes, ctypes.byref(self.ptr)))
        check(lib().scde_h2d(ctx.handle, self.ptr, a.ctypes.data_as(ctypes.c_void_p), a.nbytes))

    def free(self):
        from scde_amd._lib import check, lib
        check(lib().scde_dev_free(self.ctx.handle, self.ptr))


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


def bench_single(n, methods, reps, warmup):
    from scde_amd import api
    from scde_amd._lib import check, lib
    from scde_amd.cluster import METHODS
    L, ctx, P = lib(), api.default_context(), api._p
    d = distance_matrix(n, 4200 + n)
    y = condensed(d)
    merge, height, order = np.zeros((n - 1, 2), np.int32, order="F"), np.zeros(n - 1), np.zeros(n, np.int32)
    res = {}
    dev = Resident(ctx, d)
    try:
        for m in methods:
            code = METHODS.index(m)
            host = lambda: check(L.scde_hclust_host(ctx.handle, P(d), n, n, code, P(merge), P(height),  # noqa: E731
                                                    P(order)))
            resident = lambda: check(L.scde_hclust_dev(ctx.handle, dev.ptr, n, n, code, P(merge),  # noqa: E731
                                                       P(height), P(order)))
            h_med, h_min = _times_ms(host, reps, warmup)
            r_med, r_min = _times_ms(resident, reps, warmup)
            k_ms = kernel_ms(ctx, resident, 3)
            s_med, s_min = scipy_ms(y, m, reps if n <= 3000 else 1)
            res[m] = {"host_to_host_ms": h_med, "host_to_host_min_ms": h_min, "resident_ms": r_med,
                      "resident_min_ms": r_min, "kernel_ms": k_ms, "scipy_ms": s_med, "scipy_min_ms": s_min,
                      "scipy_runs": reps if n <= 3000 else 1, "scipy_over_host_to_host": s_med / h_med,
                      "scipy_over_resident": s_med / r_med, "top_height": float(height[-1])}
            print(f"# n={n} {m}: {json.dumps(res[m])}", file=sys.stderr, flush=True)
    finally:
        dev.free()
    return res


def bench_batch(nprob, n, methods, reps, warmup):
    from scde_amd import api
    from scde_amd._lib import check, lib
    from scde_amd.cluster import METHODS
    L, ctx, P = lib(), api.default_context(), api._p
    ds = [distance_matrix(n, 9000 + p) for p in range(nprob)]
    packed = np.concatenate([a.ravel(order="F") for a in ds])
    ys = [condensed(a) for a in ds]
    off = (np.arange(nprob, dtype=np.int64) * n * n)
    nn = np.full(nprob, n, np.int32)
    merge, height = np.zeros(2 * nprob * (n - 1), np.int32), np.zeros(nprob * (n - 1))
    order = np.zeros(nprob * n, np.int32)
    res = {}
    dev = Resident(ctx, packed)
    try:
        for m in methods:
            code = METHODS.index(m)
            run = lambda: check(L.scde_hclust_batch_dev(ctx.handle, nprob, dev.ptr, P(off), P(nn), code,  # noqa: E731
                                                        P(merge), P(height), P(order)))
            b_med, b_min = _times_ms(run, reps, warmup)
            from scipy.cluster.hierarchy import linkage
            yy = [np.sqrt(y) for y in ys] if m == "ward.D" else ys
            t0 = time.perf_counter()
            for y in yy:
                linkage(y, SCIPY_METHOD[m])
            s_ms = (time.perf_counter() - t0) * 1e3
            res[m] = {"resident_ms": b_med, "resident_min_ms": b_min, "scipy_ms": s_ms, "scipy_runs": 1,
                      "scipy_over_resident": s_ms / b_med}
            print(f"# batch {nprob}x{n} {m}: {json.dumps(res[m])}", file=sys.stderr, flush=True)
    finally:
        dev.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,3000,10000,20000")
    ap.add_argument("--methods", default="ward.D,complete")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", default="60x2000")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    methods = args.methods.split(",")
    doc = {"tool": "tools/bench_hclust.py", "reps": args.reps, "warmup": args.warmup, "single": {}, "batch": {}}

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
    if args.batch:
        nprob, n = (int(v) for v in args.batch.split("x"))
        doc["batch"][args.batch] = bench_batch(nprob, n, methods, args.reps, args.warmup)
        write()
    for n in (int(v) for v in args.sizes.split(",") if v):
        doc["single"][str(n)] = bench_single(n, methods, args.reps, args.warmup)
        write()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
