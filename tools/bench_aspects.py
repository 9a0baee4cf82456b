#!/usr/bin/env python
"""Timing of PAGODA's aspect redundancy reduction (scde_amd/aspects.py, csrc/aspects.hip) against
the same chain in numpy / scipy on one CPU thread.

    python tools/bench_aspects.py [--aspects 3000] [--cells 3000] [--genes 20000] [--reps 3]
                                  [--warmup 1] [--seed 1] [--out profiles/aspects_bench.json]

The workload, generated from the seed: aspects / 3 gene sets of 10 to 1,000 genes drawn from the
gene universe, each in three near-duplicate versions (the same loadings and cell pattern with a
little noise; the third with a tenth of its genes exchanged), so that both functions have
something to collapse.  Timed host -> host (warm-up, then the median of the repetitions):
``pagoda_reduce_loading_redundancy`` and ``pagoda_reduce_redundancy`` (on the first one's
result), and per stage through the C ABI, every call ending in the library's stream synchronise:
the loading correlation (lists uploaded, r and n left in HBM), the renormalisation, the combined
distance, hclust(complete) with cutree, and the collapse.  The CPU column is the same stage in
numpy / scipy (sparse products for the loading correlation, scipy.special's incomplete beta
function and its inverse for the renormalisation, scipy's linkage, one SVD per cluster).
Prints one JSON document; --out also writes it.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
    os.environ[_v] = "1"  # the baseline is single-threaded (set before numpy loads)

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def workload(m, ncells, ngenes, seed):
    rng = np.random.default_rng(seed)
    pwpca, names, xv = {}, [], []
    for g in range((m + 2) // 3):
        size = int(rng.integers(10, 1001))
        genes = rng.choice(ngenes, size=size, replace=False)
        load = rng.normal(size=size)
        pat = rng.normal(size=ncells) * (1.0 + rng.uniform())
        for v in range(3):
            if len(names) == m:
                break
            gs = genes.copy()
            if v == 2:
                nx = max(1, size // 10)
                spare = np.setdiff1d(rng.choice(ngenes, size=2 * nx + size, replace=False), genes)[:nx]
                gs[:nx] = spare
            key = f"set{g}.{v}"
            pwpca[key] = {"xp": {"rotation": (load + 0.03 * rng.normal(size=size))[:, None],
                                 "rotation_names": [f"g{i}" for i in gs]}}
            names.append(f"#PC1# {key}")
            xv.append(pat + 0.03 * rng.normal(size=ncells))
    xv = np.array(xv)
    return {"xv": xv, "xvw": rng.uniform(0.8, 1.0, size=xv.shape), "names": names}, pwpca


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t, out = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)), out


# ------------------------------------------------------------------ the CPU chain
def cpu_loading_cor(pl, nrot):
    from scipy import sparse
    m = len(pl)
    rows = np.concatenate([np.full(len(i), k) for k, (i, _) in enumerate(pl)])
    cols = np.concatenate([i for i, _ in pl])
    vals = np.concatenate([v for _, v in pl])
    L = sparse.csr_matrix((vals, (rows, cols)), shape=(m, nrot))
    M = sparse.csr_matrix((np.ones_like(vals), (rows, cols)), shape=(m, nrot))
    L2 = L.multiply(L).tocsr()
    l12 = (L @ L.T).toarray()
    l22 = (L2 @ M.T).toarray()      # sum over the shared genes of v_i^2
    shared = (M @ M.T).toarray()
    cv = l22 * l22.T
    with np.errstate(all="ignore"):
        r = np.where(cv > 0, l12 / np.sqrt(cv), cv)
    np.fill_diagonal(r, 1.0)
    size = np.array([len(i) for i, _ in pl])
    n = size[:, None] + size[None, :] - shared
    np.fill_diagonal(n, 0)
    return r, n.astype(np.int64)


def cpu_renorm(r, n, target):
    from scipy.special import betainc, betaincinv
    iu = np.triu_indices_from(r, 1)
    x, nn = np.abs(r[iu]), n[iu]
    a, at = (nn - 2) / 2.0, (target - 2) / 2.0
    ok = (nn > 2) & (x < 1) & (x > 0)
    out = r[iu].copy()
    xa, aa = x[ok], a[ok]
    F = betainc(aa, 0.5, (1 - xa) * (1 + xa))
    centre = F > 0.5
    cr = np.empty_like(xa)
    cr[centre] = np.sqrt(betaincinv(0.5, at, betainc(0.5, aa[centre], xa[centre] ** 2)))
    cr[~centre] = np.sqrt(1 - betaincinv(at, 0.5, F[~centre]))
    out[ok] = np.copysign(cr, r[iu][ok])
    res = r.copy()
    res[iu] = out
    res.T[iu] = out
    return res


def cpu_distance(xv, cr, power):
    c = np.abs(np.corrcoef(xv))
    pclc = np.maximum(1 - np.abs(cr), 0)
    d = (1 - np.sqrt((1 - pclc) * (1 - (1 - c)))) ** power
    np.fill_diagonal(d, 0)
    return d


def cpu_cut(d, h):
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    lab = fcluster(linkage(squareform(d, checks=False), "complete"), t=h, criterion="distance")
    first = {}
    return np.array([first.setdefault(v, len(first) + 1) for v in lab])


def cpu_collapse(xv, xvw, ct):
    var = xv.var(axis=1, ddof=1)
    out, wout = [], []
    for c in np.unique(ct):
        ii = np.nonzero(ct == c)[0]
        w = (xvw[ii] * np.sqrt(var[ii])[:, None]).sum(axis=0)
        wout.append(w / w.sum())
        if len(ii) == 1:
            out.append(xv[ii[0]])
            continue
        X = (xv[ii] - xv[ii].mean(axis=1, keepdims=True)).T
        v1 = np.linalg.svd(X, full_matrices=False)[2][0]
        s = X @ v1
        a = (xv[ii] * np.abs(v1)[:, None]).mean(axis=0)
        if np.corrcoef(s, a)[0, 1] < 0:
            s = -s
        out.append(s * np.sqrt(var[ii].max()) / np.sqrt(s.var(ddof=1)))
    return np.array(out), np.array(wout)


def cpu_matwcorr_distance(xv, xvw):
    m = xv.shape[0]
    d = np.zeros((m, m))
    sq = np.sqrt(xvw)
    for i in range(m):
        jw = sq[i] * sq[i + 1:]
        jw /= jw.sum(axis=1, keepdims=True)
        a = xv[i] - (xv[i] * jw).sum(axis=1, keepdims=True)
        b = xv[i + 1:] - (xv[i + 1:] * jw).sum(axis=1, keepdims=True)
        c = (a * b * jw).sum(axis=1) / np.sqrt((a * a * jw).sum(axis=1) * (b * b * jw).sum(axis=1))
        d[i, i + 1:] = d[i + 1:, i] = 1 - c
    return d


# ------------------------------------------------------------------ the GPU stages
def gpu_stages(tam, pl, power, threshold, reps, warmup):
    from scde_amd import api, aspects
    from scde_amd._lib import check
    from scde_amd.cluster import _hclust_dev, cutree
    xv, xvw, names = aspects._tam_arrays(tam)
    m, ncells = xv.shape
    dev = aspects._Dev(api.default_context())
    h = dev.ctx.handle
    res = {}
    try:
        xd, wd = dev.put(xv), dev.put(xvw)
        off = np.zeros(m + 1, np.int64)
        off[1:] = np.cumsum([len(i) for i, _ in pl])
        idx = np.ascontiguousarray(np.concatenate([i for i, _ in pl]), np.int32)
        val = np.ascontiguousarray(np.concatenate([v for _, v in pl]))
        r, n, cr, dist = dev.alloc(8 * m * m), dev.alloc(4 * m * m), dev.alloc(8 * m * m), dev.alloc(8 * m * m)
        P = api._p
        res["loading_correlation"], _ = timed(lambda: check(dev.L.scde_plSemicompleteCor2_dev(
            h, m, P(off), P(idx), P(val), r, n)), reps, warmup)
        res["renormalisation"], _ = timed(lambda: check(dev.L.scde_t_renorm_dev(h, r, n, m, 100.0, cr)), reps, warmup)
        res["distance"], _ = timed(lambda: check(dev.L.scde_aspect_distance_dev(h, xd, ncells, m, cr, 1, float(power),
                                                                             dist)), reps, warmup)
        res["hclust"], ct = timed(lambda: cutree(_hclust_dev(dev.ctx, dist, m, "complete"), h=threshold), reps, warmup)
        res["collapse"], col = timed(lambda: aspects._collapse_dev(dev, xd, wd, ncells, m, ct, names, True, False, 1),
                                     reps, warmup)
        res["clusters"] = int(len(col[2]))
    finally:
        dev.free()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--aspects", type=int, default=3000)
    ap.add_argument("--cells", type=int, default=3000)
    ap.add_argument("--genes", type=int, default=20000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from scde_amd import aspects
    tam, pwpca = workload(args.aspects, args.cells, args.genes, args.seed)
    m = len(tam["names"])
    rotn, pl = aspects.loading_lists(pwpca, tam["names"])
    doc = {"tool": "tools/bench_aspects.py", "aspects": m, "cells": args.cells, "genes": args.genes,
           "loading_entries": int(sum(len(i) for i, _ in pl)), "reps": args.reps, "warmup": args.warmup,
           "seed": args.seed, "unit": "seconds, median of the repetitions"}

    def write():
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")

    # ---- the GPU, host -> host and per stage
    gpu = {}
    gpu["reduce_loading_redundancy"], t1 = timed(lambda: aspects.pagoda_reduce_loading_redundancy(tam, pwpca),
                                                 args.reps, args.warmup)
    gpu["reduce_redundancy"], t2 = timed(lambda: aspects.pagoda_reduce_redundancy(t1), args.reps, args.warmup)
    gpu["stages"] = gpu_stages(tam, pl, 4, 0.01, args.reps, args.warmup)
    gpu["aspects_after_first"], gpu["aspects_after_second"] = len(t1["names"]), len(t2["names"])
    doc["gpu"] = gpu
    write()
    print("# gpu: " + json.dumps(gpu), file=sys.stderr, flush=True)

    # ---- the same chain in numpy / scipy, one thread, once
    cpu, st = {}, {}
    t0 = time.perf_counter()
    st["loading_lists"] = 0.0
    r, n = cpu_loading_cor(pl, len(rotn))
    st["loading_correlation"] = time.perf_counter() - t0
    ta = time.perf_counter()
    cr = cpu_renorm(r, n, 100)
    st["renormalisation"] = time.perf_counter() - ta
    ta = time.perf_counter()
    dist = cpu_distance(tam["xv"], cr, 4)
    st["distance"] = time.perf_counter() - ta
    ta = time.perf_counter()
    ct = cpu_cut(dist, 0.01)
    st["hclust"] = time.perf_counter() - ta
    ta = time.perf_counter()
    d1, w1 = cpu_collapse(tam["xv"], tam["xvw"], ct)
    st["collapse"] = time.perf_counter() - ta
    del st["loading_lists"]
    cpu["reduce_loading_redundancy"] = time.perf_counter() - t0
    cpu["stages"] = st
    t0 = time.perf_counter()
    ct2 = cpu_cut(cpu_matwcorr_distance(d1, w1), 0.2)
    d2, _ = cpu_collapse(d1, w1, ct2)
    cpu["reduce_redundancy"] = time.perf_counter() - t0
    cpu["aspects_after_first"], cpu["aspects_after_second"] = int(len(d1)), int(len(d2))
    doc["cpu_one_thread"] = cpu
    doc["cpu_over_gpu"] = {k: cpu[k] / gpu[k] for k in ("reduce_loading_redundancy", "reduce_redundancy")}
    doc["cpu_over_gpu"]["stages"] = {k: st[k] / gpu["stages"][k] for k in st}
    doc["max_abs_difference_first_patterns"] = (float(np.max(np.abs(d1 - t1["xv"])))
                                                if d1.shape == t1["xv"].shape else None)
    write()
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
