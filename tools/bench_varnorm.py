#!/usr/bin/env python
"""Timing of pagoda.varnorm's stages and of pagoda.subtract.aspect (scde_amd/varnorm.py,
csrc/varnorm.hip).

    python tools/bench_varnorm.py [--out profiles/varnorm_bench.json] [--shapes 2000x200,20000x1000]
                                  [--reps 3] [--warmup 1] [--nrand 100] [--no-baseline]

Per shape (genes x cells, bench.py's synthetic generator), without a batch and with two batch
levels, host -> host wall times (each call ends in the library's stream synchronise; a warm-up,
then the median of --reps):

  * weights     the existing first stage (posteriors, modes, matw / bmatw), for scale
  * moments     scde_pagoda_varnorm_moments_host (uploads counts, modes and weights)
  * statistics  the host part between the kernels (numpy + scipy, N-vectors)
  * matrix      scde_pagoda_varnorm_matrix_host (uploads counts and weights, returns mat and matw)
  * chain       pagoda_varnorm with the prior given: the four stages with the weights left in HBM
  * subtract    pagoda_subtract_aspect on the chain's result

and the two kernels' and the subtraction's own times from the context's HIP events.  Achieved
bytes per second are the bytes a kernel must move over its time: counts (int32) once per pass
(one pass for the moments, three for the matrix), the weights once (matw, and bmatw in the
moments with a batch), mat and matw written once; for the subtraction mat and matw read and mat
written.  They stand beside the HBM peak (8.0 TB/s, MI355X_MICROARCH.md) and a device-to-device
copy of 1 GiB timed the same way.

The baseline is tests/varnorm_ref.py, the numpy restatement of the same new stages (moments,
statistics, matrix, subtraction) on one CPU thread, timed once per shape; it has no weights stage.
Prints one JSON document and writes it to --out.
"""
from __future__ import annotations

import argparse
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

HBM_PEAK = 8.0e12


def _median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def _kernel_ms(ctx, fn, reps):
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


def copy_rate(nbytes=1 << 30, reps=5):
    """Bytes per second (read + written) of a device-to-device copy of nbytes."""
    try:
        import torch
        a = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
        b = torch.ones(nbytes // 4, dtype=torch.float32, device="cuda")
        for _ in range(2):
            a.copy_(b)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            a.copy_(b)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e-3)
        del a, b
        return 2.0 * nbytes / float(np.median(ts))
    except Exception as e:  # noqa: BLE001 - reported, not hidden
        return f"not measured: {e}"


def bench_shape(N, C, batched, reps, warmup, nrand, baseline, edff_path):
    import bench
    import varnorm_ref as R
    from scde_amd import api
    from scde_amd import pagoda as PG
    from scde_amd import varnorm as V
    from scde_amd.prior import expression_prior
    models, counts, _ = bench.synthetic(7300 + N % 991, N, C, two_groups=True)
    ctx = api.default_context()
    tab = V.load_edf_table(edff_path)
    batch = np.array(["a" if i % 2 else "b" for i in range(C)]) if batched else None
    codes = np.array([0 if i % 2 else 1 for i in range(C)], np.int32) if batched else None
    prior = expression_prior(models, counts, ctx=ctx)
    api.set_rand("glibc")
    keep = {}

    def weights():
        keep["s1"] = PG.pagoda_varnorm_weights(models, counts, prior, batch=batch, n_cores=1, n_randomizations=nrand)

    r = {"weights_ms": _median_ms(weights, reps, warmup)}
    s1 = keep["s1"]
    w_used = s1["bmatw"] if batched else s1["matw"]

    def moments():
        keep["mom"] = V.varnorm_moments(models, counts, tab, s1["avmodes"], s1["matw"], s1["modes"], s1["bmatw"], codes)

    r["moments_ms"] = _median_ms(moments, reps, warmup)
    mom = keep["mom"]

    def statistics():
        keep["st"] = V.varnorm_statistics(s1["avmodes"], mom, C)

    r["statistics_ms"] = _median_ms(statistics, reps, warmup)
    st = keep["st"]

    def matrix():
        keep["mat"] = V.varnorm_matrix(models, counts, w_used, st["arv"], codes)

    r["matrix_ms"] = _median_ms(matrix, reps, warmup)

    def chain():
        keep["vi"] = V.pagoda_varnorm(models, counts, tab, batch=batch, prior=prior, n_cores=1, n_randomizations=nrand)

    r["chain_ms"] = _median_ms(chain, reps, warmup)
    vi = keep["vi"]
    vi["mat"] = np.nan_to_num(vi["mat"])
    aspect = np.random.default_rng(3).normal(size=C)
    r["subtract_ms"] = _median_ms(lambda: V.pagoda_subtract_aspect(vi, aspect), reps, warmup)
    r["valid_genes"] = int(st["vi"].sum())
    # the kernels' own times and the bytes they must move
    nc = float(N) * C
    k_mom = _kernel_ms(ctx, moments, reps)
    k_mat = _kernel_ms(ctx, matrix, reps)
    k_sub = _kernel_ms(ctx, lambda: V.pagoda_subtract_aspect(vi, aspect), reps)
    b_mom = nc * (4 + 8 + (8 if batched else 0))
    b_mat = nc * (3 * 4 + 8 + 16)
    b_sub = nc * 24
    for name, ms, nbytes in (("moments", k_mom, b_mom), ("matrix", k_mat, b_mat), ("subtract", k_sub, b_sub)):
        r[name + "_kernel_ms"] = ms
        r[name + "_bytes"] = nbytes
        r[name + "_bytes_per_s"] = nbytes / (ms * 1e-3) if ms > 0 else None
        r[name + "_share_of_hbm_peak"] = nbytes / (ms * 1e-3) / HBM_PEAK if ms > 0 else None
    if baseline:
        ref_edf = R.EdfSpline(tab.lt, tab.log_edf)
        md = {k: np.asarray(v) for k, v in models.items()}
        t0 = time.perf_counter()
        rmom = R.moments(md, counts, ref_edf, s1["avmodes"], s1["matw"], s1["modes"], s1["bmatw"], codes)
        t1 = time.perf_counter()
        rst = R.statistics(s1["avmodes"], rmom, C, st["trend"])
        t2 = time.perf_counter()
        rmat, _ = R.matrix(md, counts, w_used, rst["arv"], codes)
        t3 = time.perf_counter()
        R.subtract_aspect(vi["mat"], vi["matw"], aspect)
        t4 = time.perf_counter()
        r["numpy"] = {"moments_ms": (t1 - t0) * 1e3, "statistics_ms": (t2 - t1) * 1e3, "matrix_ms": (t3 - t2) * 1e3,
                      "subtract_ms": (t4 - t3) * 1e3}
        r["numpy"]["new_stages_ms"] = r["numpy"]["moments_ms"] + r["numpy"]["statistics_ms"] + r["numpy"]["matrix_ms"]
        r["new_stages_ms"] = r["moments_ms"] + r["statistics_ms"] + r["matrix_ms"]
        r["numpy_over_library"] = {k: r["numpy"][k + "_ms"] / r[k + "_ms"]
                                   for k in ("moments", "statistics", "matrix", "subtract", "new_stages")}
        ok = rst["vi"]
        with np.errstate(all="ignore"):
            r["max_rel_difference_arv"] = float(np.nanmax(np.abs(st["arv"][ok] / rst["arv"][ok] - 1)))
            r["max_abs_difference_mat"] = float(np.nanmax(np.abs(keep["mat"][0] - rmat)))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2000x200,20000x1000")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--nrand", type=int, default=100)
    ap.add_argument("--no-baseline", action="store_true")
    ap.add_argument("--edff", default=os.path.join(ROOT, "tests", "golden", "scde_edff.npz"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "varnorm_bench.json"))
    args = ap.parse_args()
    doc = {"tool": "tools/bench_varnorm.py", "reps": args.reps, "warmup": args.warmup, "n_randomizations": args.nrand,
           "hbm_peak_bytes_per_s": HBM_PEAK, "device_copy_bytes_per_s": copy_rate(), "shapes": {}}
    for shp in args.shapes.split(","):
        N, C = (int(v) for v in shp.split("x"))
        for batched in (False, True):
            key = shp + ("_two_batches" if batched else "_no_batch")
            doc["shapes"][key] = bench_shape(N, C, batched, args.reps, args.warmup, args.nrand,
                                             not args.no_baseline, args.edff)
            print(key, json.dumps(doc["shapes"][key]), flush=True)
    txt = json.dumps(doc, indent=1)
    print(txt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(txt + "\n")


if __name__ == "__main__":
    main()
