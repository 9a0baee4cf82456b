#!/usr/bin/env python
"""Timing of the cell-to-cell distance measures (scde_amd/distance.py, csrc/dist.hip).

    python tools/bench_dist.py [--shapes 2000x1000,20000x1000] [--reps 7] [--warmup 2]
                               [--nsim 10] [--out profiles/dist_bench.json]

Per shape (genes x cells, bench.py's synthetic generator) and measure: the median wall time of
the host -> host call (counts staged by the library) and of the device-resident call (counts in
HBM; the result still returns to the host), each ending in the library's stream synchronise,
and the pair kernel's own time from the context's HIP events (slot "other").  Rates are the
operations the algorithm needs over the kernel time:

  * Gram kernel (mode-relative, direct): 6 MFMA products of 2 x 16 x 16 x 4 flops per 4 genes and
    16 x 16 pairs = 12 flops per (pair, gene), over the 32 x 32 tiles with I >= J;
  * reciprocal kernel: (pair, gene) terms per second over the same tiles, and FP64 vector
    instructions per second at the 99 FP64 VALU instructions per term its gene loop holds
    (104 with conc.a2; counted in the gfx950 ISA).

Then the one comparison the measures were introduced with: the Gram path (scde_wcorr_sep_host)
against scde_matWCorr on the same 1,000 x 400 matrices, alternating, host -> host both.
Prints one JSON document; --out also writes it.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# FP64 VALU instructions per (pair, gene) in k_recip's gene loop (gfx950 ISA), by square_logit_conc
RECIP_VALU_PER_TERM = {0: 99, 1: 104}


def _median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def _kernel_ms(ctx, fn, reps):
    """Median of the pair kernel's time per call (HIP events, slot "other")."""
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


def tile_pairs(C, T=32):
    nt = (C + T - 1) // T
    return nt * (nt + 1) // 2 * T * T


def bench_shape(N, C, reps, warmup, nsim):
    import bench
    from scde_amd import api, distance
    from scde_amd._lib import check, lib
    from scde_amd.models import model_matrix
    models, counts, _ = bench.synthetic(9100 + N % 997, N, C, two_groups=True)
    mm, _, sq = model_matrix(models)
    ctx = api.default_context()
    dc = api.DeviceCounts(ctx, counts)
    L = lib()
    out = np.zeros((C, C), order="F")
    rng = np.random.default_rng(1)
    # the mode measure's inputs: posterior modes stand-ins of the right shape and range
    modes = np.asfortranarray(np.log(np.maximum(counts, 0.5)) + rng.normal(0, 0.1, counts.shape))
    jpm = np.ascontiguousarray(np.log(counts.mean(1) + 1.0))
    P = api._p
    calls = {
        "reciprocal": (
            lambda: check(L.scde_reciprocal_corr_host(ctx.handle, P(counts), N, N, C, P(mm), sq, 0.95, P(out))),
            lambda: check(L.scde_reciprocal_corr_dev(ctx.handle, dc.ptr, N, N, C, P(mm), sq, 0.95, P(out)))),
        "mode_relative": (
            lambda: check(L.scde_mode_fail_corr_host(ctx.handle, P(counts), N, N, C, P(mm), sq, P(modes), P(jpm),
                                                     P(out))),
            lambda: check(L.scde_mode_fail_corr_dev(ctx.handle, dc.ptr, N, N, C, P(mm), sq, P(modes), P(jpm),
                                                    P(out)))),
        "direct": (
            lambda: check(L.scde_direct_corr_host(ctx.handle, P(counts), N, N, C, P(mm), sq, 0.9, nsim, None, 1,
                                                  P(out))),
            lambda: check(L.scde_direct_corr_dev(ctx.handle, dc.ptr, N, N, C, P(mm), sq, 0.9, nsim, None, 1,
                                                 P(out)))),
    }
    terms = tile_pairs(C) * N
    res = {}
    try:
        for name, (host, dev) in calls.items():
            h_med, h_min = _median_ms(host, reps, warmup)
            d_med, d_min = _median_ms(dev, reps, warmup)
            k_ms = _kernel_ms(ctx, dev, max(3, reps // 2))
            r = {"host_to_host_ms": h_med, "host_to_host_min_ms": h_min, "resident_ms": d_med,
                 "resident_min_ms": d_min, "pair_kernel_ms": k_ms}
            if name == "reciprocal":
                r["pair_gene_terms_per_s"] = terms / (k_ms * 1e-3)
                r["valu_fp64_inst_per_s"] = terms * RECIP_VALU_PER_TERM[sq] / (k_ms * 1e-3)
            else:
                rounds = nsim if name == "direct" else 1
                r["rounds"] = rounds
                r["mfma_fp64_flops_per_s"] = 12.0 * terms * rounds / (k_ms * 1e-3)
            res[name] = r
        assert np.isfinite(distance.reciprocal_distance(models, dc)).all()
    finally:
        dc.free()
    return res


def bench_vs_matwcorr(reps, warmup, k=1000, n=400):
    """scde_wcorr_sep_host against scde_matWCorr on the same matrices (the same sums: weights
    sqrt(w_i w_j) = u_i u_j with u = sqrt(w)), alternating."""
    from scde_amd._lib import check, lib
    from scde_amd.api import _p
    L = lib()
    rng = np.random.default_rng(5)
    m = np.asfortranarray(1.0 + rng.normal(size=(k, n)))
    w = np.asfortranarray(rng.uniform(0.05, 1.0, (k, n)))
    u = np.asfortranarray(np.sqrt(w))
    old, new = np.zeros((n, n), order="F"), np.zeros((n, n), order="F")
    f_old = lambda: check(L.scde_matWCorr(_p(m), _p(w), k, n, _p(old)))  # noqa: E731
    f_new = lambda: check(L.scde_wcorr_sep_host(None, _p(m), _p(u), k, k, n, _p(new)))  # noqa: E731
    for _ in range(warmup):
        f_old()
        f_new()
    t_old, t_new = [], []
    for _ in range(reps):
        for f, t in ((f_old, t_old), (f_new, t_new)):
            t0 = time.perf_counter()
            f()
            t.append((time.perf_counter() - t0) * 1e3)
    low = np.tril_indices(n, -1)
    return {"rows": k, "columns": n, "matWCorr_ms": float(np.median(t_old)), "wcorr_sep_ms": float(np.median(t_new)),
            "matWCorr_min_ms": float(np.min(t_old)), "wcorr_sep_min_ms": float(np.min(t_new)),
            "new_over_old": float(np.median(t_new) / np.median(t_old)),
            "max_abs_difference": float(np.max(np.abs(old[low] - new[low])))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2000x1000,20000x1000")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--nsim", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    doc = {"tool": "tools/bench_dist.py", "reps": args.reps, "warmup": args.warmup, "nsim": args.nsim, "shapes": {}}
    doc["gram_vs_matWCorr"] = bench_vs_matwcorr(max(args.reps, 9), args.warmup)
    for shp in args.shapes.split(","):
        N, C = (int(v) for v in shp.split("x"))
        doc["shapes"][shp] = bench_shape(N, C, args.reps, args.warmup, args.nsim)
    txt = json.dumps(doc, indent=1)
    print(txt)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(txt + "\n")


if __name__ == "__main__":
    main()
