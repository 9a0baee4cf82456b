#!/usr/bin/env python
"""Timing of the exact t-SNE embedding (scde_amd.embedding, csrc/tsne.hip).

    python tools/bench_tsne.py [--sizes 1000,3000,10000,20000] [--perplexities 10,30] [--reps 3]
                               [--warmup 1] [--part both|device|cpu] [--cpu-size 1000]
                               [--out profiles/tsne_bench.json]

Per size n and perplexity, on the Euclidean distances of n points around 8 Gaussian cluster
centres (N(0, 4^2) in 10 dimensions, unit noise):

  device  host_to_host_ms   the median wall time of tsne_embedding (scde_tsne_host: the matrix
                            uploaded, affinities, 1,000 iterations, cost, results back on the host)
          affinities_ms     scde_tsne_affinities_dev alone on a resident matrix (check, search,
                            symmetrisation; beta read back)
          iteration_us      the time per iteration with P resident: one call of
                            scde_tsne_iterate_dev that queues enough iterations (three launches
                            each) to last about a second and ends in one synchronisation, divided
                            by their number -- a single iteration is tens of microseconds, far
                            below what a host clock around it could resolve
          for n >= 10,000   the n^2 * 8 bytes of P that an iteration reads over that time, as a
                            fraction of the 8.0 TB/s HBM peak and of the 6.29 TB/s a streaming copy
                            reaches (the gradient kernel reads the whole matrix, not a triangle)
          for n <= 3,000    the FP64 rate: n^2 pairs of 23 operations (an FMA counted as two,
                            the reciprocal estimate as one) over that time, as a fraction of the
                            78.6 TFLOP/s FP64 vector peak
          kl_start, kl      the Kullback-Leibler divergence before and after the 1,000 iterations;
                            purity_5nn: the mean share of each point's 5 nearest neighbours (of
                            2,000 sampled points when n is larger) that carry its label
  cpu     the numpy restatement of the contract that the tests use (tests/tsne_ref.py, float64,
          dense n x n temporaries), affinities and 1,000 iterations, on ONE CPU thread of the
          machine that ran this part, one run, at --cpu-size points and the first perplexity: a
          baseline for orientation, not a tuned CPU implementation

The two parts may run separately (--part) into the same --out file, which is read first and
updated.  Prints one JSON document.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FP64_VECTOR_PEAK = 256 * 4 * 16 * 2.4e9 * 2  # 78.6e12: 256 CUs x 4 SIMDs x 16 FP64 lanes x 2.4 GHz, an FMA as two
HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12
FLOPS_PER_PAIR = 23  # k_tsne_grad: 2 sub, 2 FMA, rcp, 2 FMA (Newton), 2 mul, 2 FMA, mul, 2 FMA, add
K_CENTRES = 8


def points(n):
    import numpy as np
    rng = np.random.default_rng(7300 + n)
    centres = rng.normal(0, 4, (K_CENTRES, 10))
    lab = np.arange(n) % K_CENTRES
    return centres[lab] + rng.normal(0, 1, (n, 10)), lab


def distance_matrix(n):
    import numpy as np
    x, lab = points(n)
    sq = (x * x).sum(1)
    d = x @ x.T
    d *= -2
    d += sq[:, None]
    d += sq[None, :]
    np.maximum(d, 0, out=d)
    np.sqrt(d, out=d)
    np.fill_diagonal(d, 0.0)
    return np.asfortranarray(np.tril(d)), lab  # the lower triangle is what is read


def purity(Y, lab, k=5, sample=2000):
    import numpy as np
    idx = np.arange(len(Y)) if len(Y) <= sample else np.random.default_rng(1).choice(len(Y), sample, replace=False)
    d = ((Y[idx, None, :] - Y[None, :, :]) ** 2).sum(-1)
    d[np.arange(len(idx)), idx] = np.inf
    nn = np.argpartition(d, k, axis=1)[:, :k]
    return float((lab[nn] == lab[idx, None]).mean())


def _times_ms(fn, reps, warmup):
    import numpy as np
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), float(np.min(t))


def bench_device(n, perplexity, reps, warmup, d, lab):
    import numpy as np

    from scde_amd import api, tsne_affinities, tsne_embedding, tsne_iterate
    from scde_amd._lib import check, lib
    L, ctx, P = lib(), api.default_context(), api._p
    out = {}
    res = {}

    def whole():
        res["r"] = tsne_embedding(d, perplexity=perplexity, return_details=False, ctx=ctx)
    out["host_to_host_ms"], out["host_to_host_min_ms"] = _times_ms(whole, reps, warmup)
    Y = res["r"]
    out["purity_5nn"] = purity(Y, lab)

    # the affinity stage alone, on a resident matrix
    wsb = ctypes.c_int64()
    check(L.scde_tsne_ws_bytes(n, ctypes.byref(wsb)))
    ptrs = []
    try:
        for nbytes in (d.nbytes, d.nbytes, wsb.value):
            p = ctypes.c_void_p()
            check(L.scde_dev_alloc(ctx.handle, nbytes, ctypes.byref(p)))
            ptrs.append(p)
        check(L.scde_h2d(ctx.handle, ptrs[0], P(d), d.nbytes))
        beta = np.zeros(n)
        aff = lambda: check(L.scde_tsne_affinities_dev(ctx.handle, ptrs[0], n, n, float(perplexity), 0,  # noqa: E731
                                                       ptrs[1], P(beta), ptrs[2], wsb.value))
        out["affinities_ms"], out["affinities_min_ms"] = _times_ms(aff, reps, warmup)
    finally:
        for p in ptrs:
            check(L.scde_dev_free(ctx.handle, p))

    # the time per iteration with P resident: a window of about a second per measurement
    st = tsne_affinities(d, perplexity=perplexity, ctx=ctx)
    try:
        out["kl_start"] = float(st.costs().sum())
        tsne_iterate(st, 20)  # warm-up
        t0 = time.perf_counter()
        tsne_iterate(st, 50)
        probe = (time.perf_counter() - t0) / 50
        tsne_iterate(st, 1000 - st.iter)  # the host -> host call's result, bit for bit
        out["kl"] = float(st.costs().sum())
        assert np.array_equal(np.asarray(st.Y()), Y)
        k = int(min(20000, max(200, 1.0 / max(probe, 1e-7))))
        per = []
        for _ in range(reps):
            t0 = time.perf_counter()
            tsne_iterate(st, k)
            per.append((time.perf_counter() - t0) / k)
        out["iterations_per_window"] = k
        sec = float(np.median(per))
        out["iteration_us"] = sec * 1e6
        out["iteration_min_us"] = float(np.min(per)) * 1e6
    finally:
        st.close()
    if n >= 10000:
        rate = 8.0 * n * n / sec
        out.update(p_bytes_per_iteration=8 * n * n, p_bytes_per_s=rate, fraction_of_hbm_peak=rate / HBM_PEAK,
                   fraction_of_hbm_copy_rate=rate / HBM_COPY)
    if n <= 3000:
        rate = FLOPS_PER_PAIR * float(n) * n / sec
        out.update(fp64_flop_per_iteration=FLOPS_PER_PAIR * n * n, fp64_flop_per_s=rate,
                   fraction_of_fp64_vector_peak=rate / FP64_VECTOR_PEAK)
    return out


def bench_cpu(n, perplexity):
    import numpy as np
    import tsne_ref as R

    from scde_amd.embedding import initial_Y
    d, lab = distance_matrix(n)
    t0 = time.perf_counter()
    P = R.affinities(R.lower_d2(d), perplexity)[0]
    t1 = time.perf_counter()
    Y = R.iterate(P, *R.start(initial_Y(n, 1)), 0, 1000)[0]
    t2 = time.perf_counter()
    return {"what": "tests/tsne_ref.py (numpy float64 restatement), one CPU thread, one run", "n": n,
            "perplexity": perplexity, "affinities_ms": (t1 - t0) * 1e3, "iterations_1000_ms": (t2 - t1) * 1e3,
            "total_ms": (t2 - t0) * 1e3, "kl": float(R.costs(P, Y).sum()), "purity_5nn": purity(np.asarray(Y), lab)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,3000,10000,20000")
    ap.add_argument("--perplexities", default="10,30")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--part", default="both", choices=["both", "device", "cpu"])
    ap.add_argument("--cpu-size", type=int, default=1000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.part != "device":  # the baseline is single-threaded (set before numpy loads)
        for v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
            os.environ[v] = "1"
    doc = {"tool": "tools/bench_tsne.py", "runs": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    perps = [float(v) for v in args.perplexities.split(",") if v]

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
    if args.part in ("both", "device"):
        doc.update(reps=args.reps, warmup=args.warmup, max_iter=1000, fp64_vector_peak_flop_per_s=FP64_VECTOR_PEAK,
                   hbm_peak_bytes_per_s=HBM_PEAK, hbm_copy_bytes_per_s=HBM_COPY, flops_per_pair=FLOPS_PER_PAIR)
        for n in (int(v) for v in args.sizes.split(",") if v):
            d, lab = distance_matrix(n)
            for perp in perps:
                run = bench_device(n, perp, args.reps, args.warmup, d, lab)
                doc["runs"].setdefault(str(n), {})[f"{perp:g}"] = run
                print(f"# n={n} perplexity={perp:g}: {json.dumps(run)}", file=sys.stderr, flush=True)
                write()
    if args.part == "cpu" or (args.part == "both" and args.cpu_size > 0):
        doc["cpu_baseline"] = bench_cpu(args.cpu_size, perps[0])
        run = doc["runs"].get(str(args.cpu_size), {}).get(f"{perps[0]:g}")
        if run:
            doc["cpu_baseline"]["over_host_to_host"] = doc["cpu_baseline"]["total_ms"] / run["host_to_host_ms"]
        print(f"# cpu baseline: {json.dumps(doc['cpu_baseline'])}", file=sys.stderr, flush=True)
        write()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
