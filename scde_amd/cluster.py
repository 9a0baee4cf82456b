"""Hierarchical clustering on the GPU (csrc/hclust.hip; contract in include/scde_hip.h) and the
PAGODA steps that consume a distance matrix.

  * ``hclust`` / ``hclust_batch``          R's ``stats::hclust`` for ward.D, ward.D2, single,
                                           complete, average, mcquitty (merge, height, order in
                                           R's encoding)
  * ``cutree``                             R's ``cutree`` (numpy; O(n) per cut)
  * ``pagoda_cluster_cells``               R/functions.R:2641-2678
  * ``pagoda_gene_clusters_observed``      R/functions.R:2060-2121, the observed half of
                                           ``pagoda.gene.clusters``

Only the strict lower triangle of a distance matrix is read (what ``as.dist`` reads), and every
value there must be finite.  The pair merged at each step is the lexicographic minimum of
``(d(i, j), i, j)``, ``i < j``; that this is R's choice on tied distances is read from R's
algorithm and has not been checked against a run of R.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import api
from ._lib import check, lib

METHODS = ("ward.D", "ward.D2", "single", "complete", "average", "mcquitty")


class HClust:
    """The fields of R's ``hclust`` object: ``merge`` ((n - 1) x 2), ``height``, ``order``
    (1-based), ``method``, ``labels`` (None without any)."""

    def __init__(self, merge, height, order, method, labels=None):
        self.merge, self.height, self.order, self.method, self.labels = merge, height, order, method, labels

    def __repr__(self):
        return f"HClust(n={len(self.order)}, method={self.method!r})"


def _method_code(method):
    if method not in METHODS:
        raise ValueError(f"unknown method {method!r}: one of {', '.join(METHODS)}")
    return METHODS.index(method)


def _square(d):
    """(Fortran-ordered float64 square matrix, labels or None)."""
    labels = [str(x) for x in d.index] if hasattr(d, "index") and hasattr(d, "columns") else None
    a = np.asarray(d.values if labels is not None else d)
    if a.ndim != 2 or a.shape[0] != a.shape[1]:
        raise ValueError("d must be a square distance matrix")
    if a.shape[0] < 2:
        raise ValueError("at least 2 objects are needed")
    return np.asfortranarray(a, dtype=np.float64), labels


def hclust(d, method="ward.D", ctx: api.Context | None = None):
    """``hclust(as.dist(d), method)``.  ``d``: a square array or DataFrame (its labels are
    kept); only the lower triangle is used."""
    code = _method_code(method)
    a, labels = _square(d)
    n = a.shape[0]
    merge = np.zeros((n - 1, 2), np.int32, order="F")
    height = np.zeros(n - 1)
    order = np.zeros(n, np.int32)
    check(lib().scde_hclust_host(ctx.handle if ctx else None, api._p(a), n, n, code, api._p(merge), api._p(height),
                                 api._p(order)))
    return HClust(merge, height, order, method, labels)


def _hclust_dev(ctx, ptr, n, method, labels=None):
    """hclust of an n x n matrix resident in HBM (ld = n)."""
    merge = np.zeros((n - 1, 2), np.int32, order="F")
    height = np.zeros(n - 1)
    order = np.zeros(n, np.int32)
    check(lib().scde_hclust_dev(ctx.handle, ptr, n, n, _method_code(method), api._p(merge), api._p(height),
                                api._p(order)))
    return HClust(merge, height, order, method, labels)


def hclust_batch(ds, method="ward.D", ctx: api.Context | None = None):
    """``hclust`` of several matrices (any sizes) in one launch, one workgroup each; a list of
    results in the order of ``ds``."""
    code = _method_code(method)
    mats = [_square(d) for d in ds]
    if not mats:
        return []
    ctx = ctx or api.default_context()
    n = np.array([a.shape[0] for a, _ in mats], np.int32)
    off = np.concatenate([[0], np.cumsum(n.astype(np.int64) ** 2)[:-1]]).astype(np.int64)
    packed = np.concatenate([a.ravel(order="F") for a, _ in mats])
    steps = int((n - 1).sum())
    merge = np.zeros(2 * steps, np.int32)
    height = np.zeros(steps)
    order = np.zeros(int(n.sum()), np.int32)
    L = lib()
    ptr = ctypes.c_void_p()
    check(L.scde_dev_alloc(ctx.handle, packed.nbytes, ctypes.byref(ptr)))
    try:
        check(L.scde_h2d(ctx.handle, ptr, api._p(packed), packed.nbytes))
        check(L.scde_hclust_batch_dev(ctx.handle, len(mats), ptr, api._p(off), api._p(n), code, api._p(merge),
                                      api._p(height), api._p(order)))
    finally:
        check(L.scde_dev_free(ctx.handle, ptr))
    out, so, oo = [], 0, 0
    for (a, labels), m in zip(mats, (n - 1).tolist()):
        out.append(HClust(merge[2 * so:2 * (so + m)].reshape((m, 2), order="F").copy(order="F"),
                          height[so:so + m].copy(), order[oo:oo + m + 1].copy(), method, labels))
        so += m
        oo += m + 1
    return out


def cutree(hc, k=None, h=None):
    """R's ``cutree``: 1-based labels per observation, clusters numbered by the first
    observation they contain.  ``k`` clusters are the state after n - k steps; a height ``h``
    gives k = n - #{height <= h}."""
    if (k is None) == (h is None):
        raise ValueError("exactly one of k and h must be given")
    merge = np.asarray(hc.merge)
    height = np.asarray(hc.height, dtype=np.float64)
    n = merge.shape[0] + 1
    if h is not None:
        if np.any(np.diff(height) < 0):
            raise ValueError("the heights are not monotone: the tree cannot be cut by height")
        k = n - int(np.sum(height <= h))
    k = int(k)
    if not 1 <= k <= n:
        raise ValueError(f"k must be in [1, {n}]")
    m = n - k
    up = np.full(m, -1)   # the later step (< m) that absorbed the cluster of step s
    at = np.full(n, -1)   # the step that absorbed observation o as a singleton
    for s in range(m):
        for v in merge[s].tolist():
            if v < 0:
                at[-v - 1] = s
            else:
                up[v - 1] = s
    root = np.arange(m)
    for s in range(m - 1, -1, -1):
        if up[s] >= 0:
            root[s] = root[up[s]]
    key = np.where(at >= 0, root[np.maximum(at, 0)] if m else 0, m + np.arange(n))
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int32)
    rank[np.argsort(first)] = np.arange(1, len(first) + 1)  # numbered by first observation
    return rank[inv.ravel()]


def pagoda_cluster_cells(tam, varinfo, method="ward.D", include_aspects=False, return_details=False,
                         min_overdispersion=1, ctx: api.Context | None = None):
    """R/functions.R:2641-2678.  ``tam``: {"gw": {gene: weight} (or a Series), and with
    ``include_aspects`` "xv", "xvw": aspects x cells}; ``varinfo``: the dict
    ``pagoda_pathway_wPCA`` takes (mat, matw genes x cells; genes; optionally "cells") plus
    "arv" (per gene).  Genes of ``gw`` with rowSums(matw) * arv > min_overdispersion are kept,
    the cells' weighted correlation is ``matWCorr`` and the tree is ``hclust(1 - dm)``.  The
    optional ``cba`` leaf reordering is not restated.  With ``return_details``: {"clustering",
    "distance" (lower triangle as matWCorr fills it), "genes"}."""
    from .pagoda import matWCorr
    _method_code(method)
    mat = np.asarray(varinfo["mat"], dtype=np.float64)
    matw = np.asarray(varinfo["matw"], dtype=np.float64)
    genes = varinfo.get("genes")
    names = [str(g) for g in genes] if genes is not None else [str(i) for i in range(mat.shape[0])]
    row = {}
    for i, g in enumerate(names):
        row.setdefault(g, i)  # match(): the first row of a name
    od = matw.sum(axis=1) * np.asarray(varinfo["arv"], dtype=np.float64)
    gw = tam["gw"]
    gw_names = [str(g) for g in (gw.index if hasattr(gw, "index") else gw)]
    missing = [g for g in gw_names if g not in row]
    if missing:
        raise ValueError(f"tam['gw'] names genes that varinfo lacks: {missing[:3]}")
    keep = [g for g in gw_names if od[row[g]] > min_overdispersion]
    mi = [row[g] for g in keep]
    wgm, wgwm = mat[mi], matw[mi]  # gw / gw is 1
    if include_aspects:
        wgm = np.vstack([wgm, np.asarray(tam["xv"], dtype=np.float64)])
        wgwm = np.vstack([wgwm, np.asarray(tam["xvw"], dtype=np.float64)])
    dm = 1.0 - matWCorr(wgm, wgwm)
    hc = hclust(dm, method=method, ctx=ctx)
    cells = varinfo.get("cells")
    hc.labels = [str(c) for c in cells] if cells is not None else None
    if return_details:
        return {"clustering": hc, "distance": dm, "genes": keep}
    return hc


def pagoda_gene_clusters_observed(varinfo, trim=None, n_clusters=150, n_starts=10, n_components=1,
                                  n_internal_shuffles=0, method="ward.D", secondary_correlation=False, seed=1,
                                  return_details=False, ctx: api.Context | None = None):
    """The observed half of ``pagoda.gene.clusters`` (R/functions.R:2060-2121): winsorize
    (``trim`` defaults to 3.1 / ncells), centre by batch, drop constant rows, cluster the genes
    on 1 - cor (Pearson; optionally the correlation of that distance matrix again), cut into
    ``n_clusters`` and run one ``bwpca`` per cluster, oriented as R/functions.R:2114-2117.

    The gene x gene distance is formed in HBM and clustered there.  Returns {"clusters":
    {"geneCluster.k": [genes]}, "cl.goc": {"geneCluster.k": {"xp", "sd", "n"}}, "trim"} -- the
    shape the reference's ``old.results`` takes; with ``return_details`` also "distance" (read
    back), "clustering" and "genes" (the rows clustered).  The bwpca starts follow the
    n.cores = 1 order from ``set.seed(seed)``; internal shuffles are seeded per cluster with
    ``seed`` + its 0-based position."""
    from .pagoda import (DeviceMatrixPair, RState, WpcaBatch, _r_cor, shuffle_perms, weighted_mat_center,
                         winsorize_matrix)
    _method_code(method)
    ctx = ctx or api.default_context()
    mat = np.asarray(varinfo["mat"], dtype=np.float64)
    matw = np.asarray(varinfo["matw"], dtype=np.float64)
    ngenes, ncells = mat.shape
    genes = varinfo.get("genes")
    names = [str(g) for g in genes] if genes is not None else [str(i) for i in range(ngenes)]
    if trim is None:
        trim = 3.1 / ncells
    if trim > 0:
        mat = np.asarray(winsorize_matrix(mat, trim), dtype=np.float64)
    if varinfo.get("batch") is not None:
        mat = weighted_mat_center(mat, matw, varinfo["batch"])
    vi = np.nonzero(np.abs(np.diff(mat, axis=1)).sum(axis=1) > 0)[0]
    ng = len(vi)
    if ng < 2:
        raise ValueError("fewer than 2 non-constant genes")
    if not 1 <= int(n_clusters) <= ng:
        raise ValueError(f"n_clusters must be in [1, {ng}]")
    L = lib()
    x = np.ascontiguousarray(mat[vi])  # genes x cells row-major = cells x genes column-major
    bufs = []

    def dev(nbytes):
        p = ctypes.c_void_p()
        check(L.scde_dev_alloc(ctx.handle, nbytes, ctypes.byref(p)))
        bufs.append(p)
        return p
    try:
        xd = dev(x.nbytes)
        check(L.scde_h2d(ctx.handle, xd, api._p(x), x.nbytes))
        gd = dev(8 * ng * ng)
        check(L.scde_cor_distance_dev(ctx.handle, xd, ncells, ng, gd))
        if secondary_correlation:
            gd2 = dev(8 * ng * ng)
            check(L.scde_cor_distance_dev(ctx.handle, gd, ng, ng, gd2))
            gd = gd2
        hc = _hclust_dev(ctx, gd, ng, method, [names[i] for i in vi])
        dist = None
        if return_details:
            dist = np.zeros((ng, ng), order="F")
            check(L.scde_d2h(ctx.handle, api._p(dist), gd, dist.nbytes))
    finally:
        for p in bufs:
            check(L.scde_dev_free(ctx.handle, p))
    gcll = cutree(hc, k=int(n_clusters))
    il = [vi[gcll == c] for c in range(1, int(n_clusters) + 1)]
    keys = [f"geneCluster.{c}" for c in range(1, int(n_clusters) + 1)]
    # one bwpca per cluster (center = FALSE), all in one device call; the starts come from R's
    # in-memory stream in cluster order
    pair = DeviceMatrixPair(ctx, mat, matw)
    try:
        batch = WpcaBatch()
        mem = RState(seed)
        plan = []
        for ci, ii in enumerate(il):
            d = len(ii)
            K = min(int(n_components), d)
            per = n_starts * d * K
            starts = mem.unif_rand((1 + n_internal_shuffles) * per)
            main = batch.add(ii, n_components, n_starts, starts[:per])
            shuf = []
            if n_internal_shuffles > 0:
                perms = shuffle_perms(seed + ci, n_internal_shuffles, d, ncells)
                for s in range(n_internal_shuffles):
                    shuf.append(batch.add(ii, n_components, n_starts, starts[(1 + s) * per:(2 + s) * per], perms[s]))
            plan.append((main, shuf))
        res = batch.run(pair, smooth=0)
    finally:
        pair.free()
    goc = {}
    for key, ii, (main, shuf) in zip(keys, il, plan):
        r = res[main]
        cs = np.array([np.sign(_r_cor(r["scores"][:, i], r["colmeans"][:, i])) for i in range(r["scores"].shape[1])])
        xp = {"rotation": r["rotation"] * cs, "scores": r["scores"] * cs, "scoreweights": r["scoreweights"],
              "var": r["var"], "totvar": r["totvar"], "sd": np.sqrt(r["var"])[None, :],
              "rotation_names": [names[i] for i in ii]}
        if shuf:
            xp["randvar"] = np.array([r["totvar"] - res[q]["npres1"] for q in shuf])
        goc[key] = {"xp": xp, "sd": xp["sd"], "n": len(ii)}
    out = {"clusters": {key: [names[i] for i in ii] for key, ii in zip(keys, il)}, "cl.goc": goc, "trim": trim}
    if return_details:
        out.update(distance=dist, clustering=hc, genes=[names[i] for i in vi])
    return out
