#!/usr/bin/env python
"""Timing of the randomised half of pagoda.gene.clusters (scde_amd.cluster
.pagoda_gene_cluster_samples: csrc/rnorm.hip, pagoda.hip, hclust.hip, sigma1.hip).

    python tools/bench_gene_clusters.py [--shapes 2000x200,20000x1000] [--rounds 60] [--clusters 150]
                                        [--reps 3] [--warmup 1] [--baseline-reps 1]
                                        [--out profiles/gene_clusters_bench.json]

Per shape (genes x cells), ward.D, trim 3.1 / cells:

* batched: the host -> host wall time of pagoda_gene_cluster_samples (seeds in, {n, var, round}
  out; the batch sized from the free device memory), warm-up then the median of --reps runs, and
  the split the function keeps on the host clock around its library calls, each of which ends in
  a stream synchronise: draws + upload (waiting for the host's Mersenne-Twister words, their
  upload, the rnorm kernel), winsorize (with the keep rule and the gather), 1 - cor, clustering
  (one launch per batch, with the read-back of the steps), sigma_1^2 (one launch per batch); the
  rest is cutree and bookkeeping on the host;
* one at a time: the same rounds through the entry points that existed before the batched path,
  a round after the other: the normals from scde_r_unif_rand and scipy's ppf on the host,
  scde_winsorizeMatrix (host -> host), the keep rule in numpy, an upload, scde_cor_distance_dev,
  scde_hclust_dev, cutree, and numpy's svd per cluster on the host for the variances.

The ratio one-at-a-time / batched is recorded per shape, with the number of rounds in which the
two paths found the same clusters (scipy's ppf and AS241 differ in the last bits, and a tree of
random distances can turn on that) and a check of round 1 (its variances equal the batched run's
bit for bit and are compared with numpy's svd of the GPU's own blocks) and, untimed, both paths on
identical matrices (the host stream of seeds 1..3): rounds with equal cluster sizes row for row and
the largest difference of the variances there.  Prints one JSON document; --out also writes it,
after every shape.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


NOTE = ("Per shape genes x cells: the rounds of pagoda.gene.clusters' null model (set.seed(i), rnorm, winsorize at "
        "3.1 / cells, keep rule, 1 - cor, hclust ward.D, cutree, PC1 variance per cluster), host -> host wall "
        "seconds on one MI355X.  batched: pagoda_gene_cluster_samples, median of `reps` runs after `warmup` runs, "
        "with the time inside each group of library calls.  one_at_a_time: the same rounds through "
        "scde_r_unif_rand + scipy ppf, scde_winsorizeMatrix, scde_cor_distance_dev, scde_hclust_dev and numpy svd, "
        "one round after the other, `runs` runs.  one_at_a_time_over_batched is the ratio of the two wall times.")


def batched(ngenes, ncells, rounds, clusters, timings=None):
    from scde_amd import pagoda_gene_cluster_samples
    return pagoda_gene_cluster_samples(ngenes, ncells, 3.1 / ncells, n_clusters=clusters, n_samples=rounds,
                                       timings=timings)


def keep_rule(m):
    """which(abs(sum(diff(abs(x)))) > 0): float64 differences summed in cell order in long double."""
    d = np.diff(np.abs(m), axis=1)
    s = np.zeros(d.shape[0], np.longdouble)
    for k in range(d.shape[1]):
        s = s + d[:, k]
    return np.nonzero(s.astype(np.float64) != 0)[0]


def one_at_a_time(ngenes, ncells, rounds, clusters, tm, given=None):
    """given: a genes x cells matrix that replaces round 1's draws (the same-input check)."""
    from scipy.stats import norm

    from scde_amd import api, cutree, pagoda
    from scde_amd._lib import check, lib
    from scde_amd.cluster import _hclust_dev
    L, ctx, P = lib(), api.default_context(), api._p
    big = 134217728.0
    xd, gd = ctypes.c_void_p(), ctypes.c_void_p()
    check(L.scde_dev_alloc(ctx.handle, 8 * ngenes * ncells, ctypes.byref(xd)))
    check(L.scde_dev_alloc(ctx.handle, 8 * ngenes * ngenes, ctypes.byref(gd)))
    out, sizes = [], []

    def lap(key, t0):
        t1 = time.perf_counter()
        tm[key] = tm.get(key, 0.0) + t1 - t0
        return t1
    try:
        for i in range(1, rounds + 1):
            t0 = time.perf_counter()
            if given is None:
                st = np.zeros(625, np.uint32)
                check(L.scde_r_set_seed(i, P(st)))
                u = np.zeros(2 * ngenes * ncells)
                check(L.scde_r_unif_rand(P(st), len(u), P(u)))
                m = norm.ppf((np.floor(big * u[0::2]) + u[1::2]) / big).reshape(ncells, ngenes).T
            else:
                m = given
            t0 = lap("draw", t0)
            m = np.asarray(pagoda.winsorizeMatrix(np.asfortranarray(m), 3.1 / ncells))
            vi = keep_rule(m)
            x = np.ascontiguousarray(m[vi])
            check(L.scde_h2d(ctx.handle, xd, P(x), x.nbytes))
            t0 = lap("winsorize", t0)
            check(L.scde_cor_distance_dev(ctx.handle, xd, ncells, len(vi), gd))
            t0 = lap("distance", t0)
            hc = _hclust_dev(ctx, gd, len(vi), "ward.D")
            t0 = lap("clustering", t0)
            lab = cutree(hc, k=clusters)
            t0 = lap("cutree", t0)
            for c in range(1, clusters + 1):
                sizes.append(int((lab == c).sum()))
                out.append(np.linalg.svd(x[lab == c], compute_uv=False)[0] ** 2 / max(1, ncells - 1))
            lap("sigma1", t0)
            if i % 10 == 0:
                print(f"# one at a time: round {i} of {rounds}", file=sys.stderr, flush=True)
    finally:
        check(L.scde_dev_free(ctx.handle, xd))
        check(L.scde_dev_free(ctx.handle, gd))
    return np.array(out), np.array(sizes)


def bench_shape(ngenes, ncells, rounds, clusters, reps, warmup, base_reps):
    for _ in range(warmup):
        batched(ngenes, ncells, rounds, clusters)
    walls, splits, res = [], [], None
    for _ in range(reps):
        tm = {}
        t0 = time.perf_counter()
        res = batched(ngenes, ncells, rounds, clusters, tm)
        walls.append(time.perf_counter() - t0)
        splits.append(tm)
    doc = {"genes": ngenes, "cells": ncells, "rounds": rounds, "clusters": clusters, "method": "ward.D",
           "reps": reps, "warmup": warmup,
           "batched": {"host_to_host_s": float(np.median(walls)), "host_to_host_min_s": float(np.min(walls)),
                       "split_s": {k: float(np.median([s[k] for s in splits])) for k in splits[0]}}}
    doc["batched"]["split_s"]["host_rest"] = doc["batched"]["host_to_host_s"] - sum(doc["batched"]["split_s"].values())
    print(f"# {ngenes}x{ncells} batched: {json.dumps(doc['batched'])}", file=sys.stderr, flush=True)
    bw, bs, var = [], [], None
    for _ in range(base_reps):
        tm = {}
        t0 = time.perf_counter()
        var, _ = one_at_a_time(ngenes, ncells, rounds, clusters, tm)
        bw.append(time.perf_counter() - t0)
        bs.append(tm)
    doc["one_at_a_time"] = {"host_to_host_s": float(np.median(bw)), "runs": base_reps,
                            "split_s": {k: float(np.median([s[k] for s in bs])) for k in bs[0]}}
    doc["one_at_a_time_over_batched"] = doc["one_at_a_time"]["host_to_host_s"] / doc["batched"]["host_to_host_s"]
    doc["rounds_with_the_same_clusters"] = same_rounds(var, res, rounds, clusters)
    doc["round_1_check"] = check_round_1(ngenes, ncells, clusters, res)
    doc["same_input_check"] = check_same_inputs(ngenes, ncells, clusters)
    print(f"# {ngenes}x{ncells} one at a time: {json.dumps(doc['one_at_a_time'])} ratio "
          f"{doc['one_at_a_time_over_batched']:.2f}; same clusters in {doc['rounds_with_the_same_clusters']} of "
          f"{rounds} rounds; {json.dumps(doc['round_1_check'])}; same inputs: "
          f"{json.dumps(doc['same_input_check'])}", file=sys.stderr, flush=True)
    return doc


def same_rounds(var, res, rounds, clusters):
    """Rounds in which the two paths found the same clusters (sizes equal and variances within
    1e-9, compared as sorted lists: the labels may be numbered differently).  The one-at-a-time
    path draws its normals with scipy's ppf, which differs from R's AS241 in the last bits, and a
    tree of thousands of near-equal random distances may turn on that (supposed, not isolated);
    so this is a description of the comparison, not a check -- check_same_inputs is the check."""
    if len(var) != len(res["var"]):
        return None
    n = 0
    for r in range(rounds):
        a = np.sort(var[r * clusters:(r + 1) * clusters])
        b = np.sort(res["var"][r * clusters:(r + 1) * clusters])
        n += bool(np.allclose(a, b, rtol=1e-9, atol=0))
    return n


def check_round_1(ngenes, ncells, clusters, res):
    """Round 1 again with its details read back: the variances must be the batched run's bit
    for bit, and are compared with numpy's svd of the same blocks (the GPU's own winsorized matrix
    and labels) on the host."""
    from scde_amd import pagoda_gene_cluster_samples
    one = pagoda_gene_cluster_samples(ngenes, ncells, 3.1 / ncells, n_clusters=clusters, n_samples=1,
                                      return_details=True)
    det = one["details"][0]
    ref = np.array([np.linalg.svd(det["matrix"][det["labels"] == c], compute_uv=False)[0] ** 2 / max(1, ncells - 1)
                    for c in range(1, clusters + 1)])
    return {"equals_the_batched_run": bool(one["var"].tobytes() == res["var"][:clusters].tobytes()),
            "genes_kept": int(len(det["kept"])), "largest_cluster": int(one["n"].max()),
            "max_rel_diff_from_numpy_svd": float(np.max(np.abs(one["var"] - ref) / ref))}


def check_same_inputs(ngenes, ncells, clusters, nrounds=3):
    """Untimed: both paths on identical matrices (the host stream scde_r_norm_rand of seeds
    1..nrounds, handed to the batched path as matrices= and to the one-at-a-time path in place of
    its draws).  Rounds in which the cluster sizes are equal row for row, and over those the
    largest relative difference between the batched variances and numpy's svd."""
    from scde_amd import api, pagoda_gene_cluster_samples
    from scde_amd._lib import check, lib
    L, P = lib(), api._p
    mats = []
    for seed in range(1, nrounds + 1):
        st = np.zeros(625, np.uint32)
        z = np.zeros(ngenes * ncells)
        check(L.scde_r_set_seed(seed, P(st)))
        check(L.scde_r_norm_rand(P(st), len(z), P(z)))
        mats.append(np.ascontiguousarray(z.reshape(ncells, ngenes).T))
    got = pagoda_gene_cluster_samples(ngenes, ncells, 3.1 / ncells, n_clusters=clusters, matrices=mats)
    same, worst = 0, 0.0
    for r, m in enumerate(mats):
        var, sizes = one_at_a_time(ngenes, ncells, 1, clusters, {}, given=m)
        rows = slice(r * clusters, (r + 1) * clusters)
        if np.array_equal(got["n"][rows], sizes):
            same += 1
            worst = max(worst, float(np.max(np.abs(got["var"][rows] - var) / var)))
    return {"rounds": nrounds, "rounds_with_equal_clusters": same, "max_rel_diff_of_var": worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="2000x200,20000x1000")
    ap.add_argument("--rounds", type=int, default=60)
    ap.add_argument("--clusters", type=int, default=150)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--baseline-reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    doc = {"tool": "tools/bench_gene_clusters.py", "note": NOTE, "shapes": {}}
    if args.out and os.path.exists(args.out):  # shapes measured by an earlier call are kept
        with open(args.out) as f:
            doc["shapes"] = json.load(f).get("shapes", {})
    for shape in args.shapes.split(","):
        g, c = (int(v) for v in shape.split("x"))
        doc["shapes"][shape] = bench_shape(g, c, args.rounds, args.clusters, args.reps, args.warmup,
                                           args.baseline_reps)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc, indent=1))


if __name__ == "__main__":
    main()
