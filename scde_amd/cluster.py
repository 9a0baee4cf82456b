"""Hierarchical clustering on the GPU (csrc/hclust.hip; contract in include/scde_hip.h) and the
PAGODA steps that consume a distance matrix.

  * ``hclust`` / ``hclust_batch``          R's ``stats::hclust`` for ward.D, ward.D2, single,
                                           complete, average, mcquitty (merge, height, order in
                                           R's encoding)
  * ``dist`` / ``hclust_dist``             R's ``stats::dist`` between the rows of a matrix
                                           (euclidean, manhattan, maximum; csrc/rdist.hip), and
                                           ``hclust(dist(x))`` with the matrix kept in HBM
  * ``cutree``                             R's ``cutree`` (numpy; O(n) per cut)
  * ``order_optimal`` / ``leaf_order_length``  ``cba::order.optimal``: the orientation of a tree
                                           whose leaf order has the smallest summed distance
                                           between neighbours (csrc/olo.hip)
  * ``pagoda_cluster_cells``               R/functions.R:2641-2678
  * ``pagoda_gene_clusters_observed``      R/functions.R:2060-2121, the observed half of
                                           ``pagoda.gene.clusters``
  * ``pagoda_gene_cluster_samples``        R/functions.R:2131-2192, its randomised half (the null
                                           model's sampled PC1 variances), rounds batched
  * ``pagoda_gene_clusters``               the whole function: both halves and the scoring of
                                           R/functions.R:2196-2211 (``scde_amd/rmt.py``)

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


DIST_METHODS = ("euclidean", "manhattan", "maximum")


def _dist_code(method):
    if method not in DIST_METHODS:
        raise ValueError(f"unknown method {method!r}: one of {', '.join(DIST_METHODS)}")
    return DIST_METHODS.index(method)


def _dist_input(x):
    """(Fortran-ordered float64 n x p matrix, row labels or None)."""
    labels = [str(v) for v in x.index] if hasattr(x, "index") and hasattr(x, "columns") else None
    a = np.asarray(x.values if labels is not None else x, dtype=np.float64)
    if a.ndim != 2 or a.shape[0] < 1:
        raise ValueError("x must be an n x p matrix with at least one row")
    return np.asfortranarray(a), labels


def dist(x, method="euclidean", ctx: api.Context | None = None):
    """R's ``as.matrix(dist(x, method))`` (csrc/rdist.hip; the contract is in
    include/scde_hip.h): the distances between the rows of the n x p ``x`` as the symmetric
    n x n float64 matrix with a zero diagonal, which ``hclust`` takes as it stands.  ``method``:
    "euclidean", "manhattan" or "maximum".  A column takes part in a pair when neither value is
    NaN and the difference is not NaN; sums over fewer than p columns are scaled up by
    p / count, and a pair without a common column is NaN, as in R.  A DataFrame's row labels come
    back on a DataFrame.  Written from R's documentation and C loop; not checked against a run
    of R."""
    code = _dist_code(method)
    a, labels = _dist_input(x)
    n, p = a.shape
    out = np.zeros((n, n), order="F")
    check(lib().scde_dist_host(ctx.handle if ctx else None, api._p(a), n, n, p, code, api._p(out)))
    if labels is not None:
        import pandas as pd
        return pd.DataFrame(out, index=labels, columns=labels)
    return out


def hclust_dist(x, dist_method="euclidean", method="complete", ctx: api.Context | None = None):
    """``hclust(dist(x, dist_method), method)`` with the distance matrix formed in HBM and
    clustered there (it never visits the host).  R's defaults for both methods."""
    _method_code(method)
    code = _dist_code(dist_method)
    ctx = ctx or api.default_context()
    a, labels = _dist_input(x)
    n, p = a.shape
    if n < 2:
        raise ValueError("at least 2 objects are needed")
    L = lib()
    bufs = []
    try:
        for nbytes in (max(a.nbytes, 8), 8 * n * n):
            ptr = ctypes.c_void_p()
            check(L.scde_dev_alloc(ctx.handle, nbytes, ctypes.byref(ptr)))
            bufs.append(ptr)
        xd, dd = bufs
        if a.nbytes:
            check(L.scde_h2d(ctx.handle, xd, api._p(a), a.nbytes))
        check(L.scde_dist_dev(ctx.handle, xd, n, n, p, code, dd))
        return _hclust_dev(ctx, dd, n, method, labels)
    finally:
        for ptr in bufs:
            L.scde_dev_free(ctx.handle, ptr)


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


def _order_optimal(ctx, d, ld, n, merge, dev):
    """The C entry on a host array (``d``: an ndarray) or a resident matrix (``d``: a pointer)."""
    merge = np.asfortranarray(merge, dtype=np.int32)
    if merge.shape != (n - 1, 2):
        raise ValueError(f"merge must be {n - 1} x 2 for {n} objects")
    merge_out = np.zeros((n - 1, 2), np.int32, order="F")
    order = np.zeros(n, np.int32)
    length = ctypes.c_double()
    f = lib().scde_order_optimal_dev if dev else lib().scde_order_optimal_host
    check(f(ctx.handle if ctx else None, d if dev else api._p(d), ld, n, api._p(merge), api._p(merge_out),
            api._p(order), ctypes.byref(length)))
    return merge_out, order, length.value


def order_optimal(hc, d, ctx: api.Context | None = None, return_length=False):
    """``cba::order.optimal(as.dist(d), hc$merge)``: ``hc`` (an ``HClust`` or anything with
    ``.merge``) re-oriented so that the summed distance between neighbouring leaves is the
    smallest of all 2^(n - 1) orientations (Bar-Joseph, Gifford and Jaakkola 2001; the contract is
    in include/scde_hip.h).  ``d`` as for ``hclust``.  Returns a new ``HClust``: ``merge`` with
    the columns of the flipped rows swapped (cba's convention), ``order`` its leaves left to
    right, ``height``, ``method`` and ``labels`` kept; with ``return_length`` also the path length
    (``leaf_order_length(d, order)``).

    The root is never flipped, and among equally short orders the (cost, position, position)
    rule of the header decides.  Which of them cba itself returns is unknown, and nothing here was
    checked against a run of R or cba."""
    a, _ = _square(d)
    merge_out, order, length = _order_optimal(ctx, a, a.shape[0], a.shape[0], hc.merge, dev=False)
    out = HClust(merge_out, getattr(hc, "height", None), order, getattr(hc, "method", None),
                 getattr(hc, "labels", None))
    return (out, length) if return_length else out


def leaf_order_length(d, order):
    """The summed distance between neighbours of ``order`` (1-based), added left to right in
    float64; ``d`` is read in its lower triangle."""
    a = np.asarray(d.values if hasattr(d, "index") and hasattr(d, "columns") else d, dtype=np.float64)
    o = np.asarray(order, dtype=np.int64) - 1
    total = 0.0
    for v in a[np.maximum(o[:-1], o[1:]), np.minimum(o[:-1], o[1:])].tolist():
        total += v
    return total


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
                         min_overdispersion=1, ctx: api.Context | None = None, optimal_order=False):
    """R/functions.R:2641-2678.  ``tam``: {"gw": {gene: weight} (or a Series), and with
    ``include_aspects`` "xv", "xvw": aspects x cells}; ``varinfo``: the dict
    ``pagoda_pathway_wPCA`` takes (mat, matw genes x cells; genes; optionally "cells") plus
    "arv" (per gene).  Genes of ``gw`` with rowSums(matw) * arv > min_overdispersion are kept,
    the cells' weighted correlation is ``matWCorr`` and the tree is ``hclust(1 - dm)``.  With
    ``optimal_order`` the tree is then re-oriented by ``order_optimal`` on the same distance, as
    the reference does when ``cba`` is installed (R/functions.R:2668-2672: ``merge`` and ``order``
    replaced); the matrix is uploaded once and stays in HBM between the two steps.  The default
    leaves hclust's own order.  With ``return_details``: {"clustering", "distance" (lower triangle
    as matWCorr fills it), "genes"}.  The walkthrough's 2-D embedding of the cells is
    ``tsne_embedding(details["distance"], perplexity=10)`` (``scde_amd/embedding.py``)."""
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
    if optimal_order:
        ctx = ctx or api.default_context()
        a, _ = _square(dm)
        n = a.shape[0]
        L = lib()
        ptr = ctypes.c_void_p()
        check(L.scde_dev_alloc(ctx.handle, a.nbytes, ctypes.byref(ptr)))
        try:
            check(L.scde_h2d(ctx.handle, ptr, api._p(a), a.nbytes))
            hc = _hclust_dev(ctx, ptr, n, method)
            hc.merge, hc.order, _ = _order_optimal(ctx, ptr, n, n, hc.merge, dev=True)
        finally:
            check(L.scde_dev_free(ctx.handle, ptr))
    else:
        hc = hclust(dm, method=method, ctx=ctx)
    cells = varinfo.get("cells")
    hc.labels = [str(c) for c in cells] if cells is not None else None
    if return_details:
        return {"clustering": hc, "distance": dm, "genes": keep}
    return hc


def pagoda_gene_clusters_observed(varinfo, trim=None, n_clusters=150, n_starts=10, n_components=1,
                                  n_internal_shuffles=0, method="ward.D", secondary_correlation=False, seed=1,
                                  return_details=False, cor_method="pearson", ctx: api.Context | None = None):
    """The observed half of ``pagoda.gene.clusters`` (R/functions.R:2060-2121): winsorize
    (``trim`` defaults to 3.1 / ncells), centre by batch, drop constant rows, cluster the genes
    on 1 - cor (``cor_method`` "pearson" / "p", or "spearman": the genes ranked over the cells on
    the device first; optionally the Pearson correlation of that distance matrix again), cut into
    ``n_clusters`` and run one ``bwpca`` per cluster, oriented as R/functions.R:2114-2117.

    The gene x gene distance is formed in HBM and clustered there.  Returns {"clusters":
    {"geneCluster.k": [genes]}, "cl.goc": {"geneCluster.k": {"xp", "sd", "n"}}, "trim"} -- the
    shape the reference's ``old.results`` takes; with ``return_details`` also "distance" (read
    back), "clustering" and "genes" (the rows clustered).  The bwpca starts follow the
    n.cores = 1 order from ``set.seed(seed)``; internal shuffles are seeded per cluster with
    ``seed`` + its 0-based position."""
    from .pagoda import (DeviceMatrixPair, RState, WpcaBatch, _r_cor, shuffle_perms, weighted_mat_center,
                         winsorize_matrix)
    from .spearman import cor_method_is_spearman
    _method_code(method)
    spearman = cor_method_is_spearman(cor_method)
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
        if spearman:  # (only the distance sees the ranks: xd is not used again)
            check(L.scde_rank_cols_dev(ctx.handle, xd, ncells, ng, xd))
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


def _ptr(base, byte_off):
    return ctypes.c_void_p(base.value + int(byte_off))


def _mt_words(seed, n):
    """The first n raw Mersenne-Twister words after ``set.seed(seed)`` (host; releases the GIL)."""
    state = np.zeros(625, np.uint32)
    words = np.empty(n, np.uint32)
    L = lib()
    check(L.scde_r_set_seed(int(seed), api._p(state)))
    check(L.scde_r_mt_words(api._p(state), n, api._p(words)))
    return words


def dev_mem_info(ctx: api.Context | None = None):
    """(free, total) bytes of the context's device."""
    ctx = ctx or api.default_context()
    free, total = ctypes.c_int64(), ctypes.c_int64()
    check(lib().scde_dev_mem_info(ctx.handle, ctypes.byref(free), ctypes.byref(total)))
    return free.value, total.value


def _hclust_ws_bytes(n):
    return 8 * n * n + 25 * n + 256  # csrc/hclust.hip's hclust_ws_bytes: the n^2 working copy and O(n) lists


def pagoda_gene_cluster_samples(ngenes, n_cells, trim, n_clusters=150, n_samples=60, method="ward.D",
                                secondary_correlation=False, rounds_per_batch=None, matrices=None,
                                return_details=False, timings=None, cor_method="pearson",
                                ctx: api.Context | None = None):
    """The randomised half of ``pagoda.gene.clusters`` (R/functions.R:2131-2192), n.cores = 1:
    for round i = 1..n_samples, ``set.seed(i)``, ``matrix(rnorm(ngenes * n_cells), nrow = ngenes)``,
    winsorize (``trim`` > 0), keep the genes with ``abs(sum(diff(abs(x)))) > 0``, cluster them on
    1 - cor (``cor_method`` "pearson" / "p", or "spearman": the kept genes ranked over the cells;
    optionally the Pearson correlation of that distance again), cut into ``n_clusters`` and take
    per cluster ``pcaMethods::sDev(pca(m[, ii], nPcs = 1, center = FALSE))^2``, read as
    sigma_1^2 / max(1, n_cells - 1) (from memory of pcaMethods; not checked against it).

    Returns {"n", "var", "round"}: one row per cluster, rounds in order 1..n_samples and within a
    round in cluster-label order (R's ``tapply`` order).

    Every step runs on matrices resident in HBM.  Rounds are processed in batches: the distance
    matrices of a batch are packed in one buffer and clustered in one launch (one workgroup per
    round), and the PC1 variances of all clusters of all its rounds come from one launch.
    ``rounds_per_batch=None`` sizes the batch so that what grows with it -- per round its distance
    matrix (twice with ``secondary_correlation``), the clustering's n^2 workspace and step lists,
    the round matrix and the PC1 kernel's workspace (at most genes x min(genes, cells) doubles) --
    and the three round-sized staging buffers take at most half of the device memory that is
    free; the batch size changes no bit of the result.  The host draws round i + 1's
    Mersenne-Twister words while the device works on round i.

    ``matrices`` (a list of genes x cells arrays) replaces the drawn matrices (``n_samples`` is
    then its length).  With ``return_details`` the result gains "details": per round {"kept" (gene
    indices), "matrix" (the winsorized kept genes x cells, read back), "distance" (read back),
    "clustering", "labels"}.  ``timings`` (a dict, for tools/bench_gene_clusters.py) receives the
    host-clock seconds spent inside each group of library calls, every one of which ends in a
    stream synchronise: "draw", "winsorize" (with the keep rule and the gather), "distance",
    "clustering", "sigma1"."""
    import time
    from concurrent.futures import ThreadPoolExecutor
    from .spearman import cor_method_is_spearman
    code = _method_code(method)
    spearman = cor_method_is_spearman(cor_method)
    ngenes, n_cells, n_clusters = int(ngenes), int(n_cells), int(n_clusters)
    if matrices is not None:
        matrices = [np.ascontiguousarray(m, dtype=np.float64) for m in matrices]
        n_samples = len(matrices)
        if any(m.shape != (ngenes, n_cells) for m in matrices):
            raise ValueError(f"every matrix must be {ngenes} x {n_cells} (genes x cells)")
    n_samples = int(n_samples)
    if ngenes < 2:
        raise ValueError("at least 2 genes are needed")
    if n_cells < 2:
        raise ValueError("at least 2 cells are needed: with one cell diff() is empty and every gene is dropped")
    if n_samples < 1:
        raise ValueError("n_samples must be at least 1")
    if not 1 <= n_clusters <= ngenes:
        raise ValueError(f"n_clusters must be in [1, {ngenes}]")
    if not 0 <= trim < 1:
        raise ValueError("trim must be in [0, 1)")
    ctx = ctx or api.default_context()
    L = lib()
    msz = 8 * ngenes * n_cells  # one round matrix
    dsz = 8 * ngenes * ngenes   # one distance matrix
    if rounds_per_batch is None:
        free, _ = dev_mem_info(ctx)
        per_round = (dsz * (2 if secondary_correlation else 1) + _hclust_ws_bytes(ngenes) + 16 * ngenes + msz
                     + 8 * (ngenes + 4) * min(ngenes, n_cells) + 256)
        # raw, wz and the library's word buffer (and the ranks, and the counting path's copy of them)
        rounds_per_batch = (free // 2 - (5 if spearman else 3) * msz) // per_round
    B = int(max(1, min(int(rounds_per_batch), n_samples)))
    tm = timings if timings is not None else {}
    for k in ("draw", "winsorize", "distance", "clustering", "sigma1"):
        tm.setdefault(k, 0.0)

    def timed(key, t0):
        t1 = time.perf_counter()
        tm[key] += t1 - t0
        return t1

    bufs = []

    def dev(nbytes):
        p = ctypes.c_void_p()
        check(L.scde_dev_alloc(ctx.handle, max(int(nbytes), 8), ctypes.byref(p)))
        bufs.append(p)
        return p

    out_n, out_var, out_round, details = [], [], [], []
    nwords = 2 * ngenes * n_cells
    pool = ThreadPoolExecutor(max_workers=1) if matrices is None else None
    try:
        nxt = pool.submit(_mt_words, 1, nwords) if pool else None
        raw = dev(msz)          # a round's matrix as drawn (or given)
        wz = dev(msz)           # the same winsorized, every gene still in place
        xw = dev(B * msz)       # the batch's winsorized, kept matrices: n_cells x (B * ngenes)
        gd = dev(B * dsz)       # the batch's distance matrices, round r at element r * ngenes^2
        gd2 = dev(B * dsz) if secondary_correlation else None
        # the ranks of a round's kept genes: only the distance sees them, sigma1 takes the values in xw
        rk = dev(msz) if spearman else None
        for b0 in range(0, n_samples, B):
            nb = min(B, n_samples - b0)
            nk = np.zeros(nb, np.int32)
            kept = []
            for r in range(nb):
                i = b0 + r + 1  # the round, R's set.seed(i)
                t0 = time.perf_counter()
                if matrices is None:
                    words = nxt.result()
                    nxt = pool.submit(_mt_words, i + 1, nwords) if i < n_samples else None
                    check(L.scde_rnorm_matrix_dev(ctx.handle, api._p(words), ngenes, n_cells, raw))
                else:
                    check(L.scde_h2d(ctx.handle, raw, api._p(matrices[i - 1]), msz))
                t0 = timed("draw", t0)
                slot = _ptr(xw, r * msz)
                check(L.scde_winsorize_dev(ctx.handle, raw, n_cells, ngenes, float(trim), wz))
                keep = np.zeros(ngenes, np.int32)
                check(L.scde_keep_absdiff_dev(ctx.handle, wz, n_cells, ngenes, api._p(keep)))
                vi = np.nonzero(keep)[0].astype(np.int32)
                # A round drops a gene when its first and last cell were clipped to the same bound and
                # the rounded differences cancel exactly (about one round in two at 120 x 24; DESIGN.md
                # section 4.8).  The kept columns go to the round's slot in one gather, which is a plain
                # copy in the rounds that keep every gene.
                if len(vi) < 2 or n_clusters > len(vi):
                    raise ValueError(f"round {i}: {len(vi)} genes pass the keep rule, fewer than "
                                     f"{max(2, n_clusters)}")
                check(L.scde_gather_cols_dev(ctx.handle, wz, n_cells, ngenes, api._p(vi), len(vi), slot))
                kept.append(vi)
                nk[r] = len(vi)
                t0 = timed("winsorize", t0)
                dr = _ptr(gd, r * dsz)
                if spearman:
                    check(L.scde_rank_cols_dev(ctx.handle, slot, n_cells, int(nk[r]), rk))
                check(L.scde_cor_distance_dev(ctx.handle, rk if spearman else slot, n_cells, int(nk[r]), dr))
                if secondary_correlation:
                    check(L.scde_cor_distance_dev(ctx.handle, dr, int(nk[r]), int(nk[r]), _ptr(gd2, r * dsz)))
                timed("distance", t0)
            t0 = time.perf_counter()
            dist_buf = gd2 if secondary_correlation else gd
            off = np.arange(nb, dtype=np.int64) * (ngenes * ngenes)
            steps = int((nk - 1).sum())
            merge = np.zeros(2 * steps, np.int32)
            height = np.zeros(steps)
            order = np.zeros(int(nk.sum()), np.int32)
            check(L.scde_hclust_batch_dev(ctx.handle, nb, dist_buf, api._p(off), api._p(nk), code, api._p(merge),
                                          api._p(height), api._p(order)))
            t0 = timed("clustering", t0)
            idx, cnt, so, oo = [], [], 0, 0
            for r in range(nb):
                m = int(nk[r]) - 1
                hc = HClust(merge[2 * so:2 * (so + m)].reshape((m, 2), order="F"), height[so:so + m],
                            order[oo:oo + m + 1], method)
                so += m
                oo += m + 1
                lab = cutree(hc, k=n_clusters)
                idx.append((np.argsort(lab, kind="stable") + r * ngenes).astype(np.int32))  # label, then gene order
                cnt.append(np.bincount(lab, minlength=n_clusters + 1)[1:])
                if return_details:
                    dist = np.zeros((m + 1, m + 1), order="F")
                    check(L.scde_d2h(ctx.handle, api._p(dist), _ptr(dist_buf, r * dsz), dist.nbytes))
                    mk = np.zeros((m + 1, n_cells))  # genes x cells, C order: the resident layout
                    check(L.scde_d2h(ctx.handle, api._p(mk), _ptr(xw, r * msz), mk.nbytes))
                    details.append({"kept": kept[r], "matrix": mk, "distance": dist, "labels": lab,
                                    "clustering": HClust(hc.merge.copy(order="F"), hc.height.copy(), hc.order.copy(),
                                                         method)})
            idx = np.ascontiguousarray(np.concatenate(idx))
            cnt = np.concatenate(cnt).astype(np.int64)
            poff = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
            s1 = np.zeros(len(cnt))
            t0 = time.perf_counter()
            check(L.scde_sigma1sq_batch_dev(ctx.handle, xw, n_cells, nb * ngenes, len(cnt), api._p(poff), api._p(idx),
                                            api._p(s1)))
            timed("sigma1", t0)
            out_n.append(cnt.astype(np.int32))
            out_var.append(s1 / max(1, n_cells - 1))
            out_round.append(np.repeat(np.arange(b0 + 1, b0 + nb + 1, dtype=np.int32), n_clusters))
    except BaseException:
        if pool:
            pool.shutdown(wait=True, cancel_futures=True)
        for p in bufs:  # (a failure to free must not replace the error on its way out)
            L.scde_dev_free(ctx.handle, p)
        raise
    if pool:
        pool.shutdown(wait=True)
    for p in bufs:
        check(L.scde_dev_free(ctx.handle, p))
    out = {"n": np.concatenate(out_n), "var": np.concatenate(out_var), "round": np.concatenate(out_round)}
    if return_details:
        out["details"] = details
    return out


def pagoda_gene_clusters(varinfo, trim=None, n_clusters=150, n_samples=60, n_internal_shuffles=0, n_starts=10,
                         n_components=1, method="ward.D", secondary_correlation=False, n_cells=None, old_results=None,
                         seed=1, cor_method="pearson", ctx: api.Context | None = None):
    """``pagoda.gene.clusters`` (R/functions.R:2058-2237; n.cores = 1, no plot, no ``show.random``):
    the observed clusters (``pagoda_gene_clusters_observed``) scored against the null model of
    ``pagoda_gene_cluster_samples`` on ``nrow(varinfo$mat)`` x ``n_cells`` random matrices
    (``n_cells`` defaults to the cells of ``varinfo``).

    Returns the reference's list: {"clusters", "cl.goc", "trim"} as the observed half gives them;
    "varm": {"n", "var", "round", "pm", "pv", "varst"}; "clvlm": the fit ``var ~ 0 + pm + n``
    ({"coefficients", "fitted.values", "residuals"}); "tci": {round: row of ``varm`` with the
    round's first maximum ``varst``}, rows 0-based (R's are 1-based); "xf": the Gumbel maximum-
    likelihood fit of ``varst`` {"location", "scale"} (``scde_amd.rmt``).

    ``old_results`` reuses its "clusters" / "cl.goc" and, when it has one, its "varm" (n, var,
    round), as R/functions.R:2074-2129 do; with a "varm" no device work is done.  ``cor_method``
    ("pearson", "p" or "spearman") is the correlation of both halves' gene distance."""
    from . import rmt
    from .spearman import cor_method_is_spearman
    _method_code(method)
    cor_method_is_spearman(cor_method)
    ngenes, ncol = np.asarray(varinfo["mat"]).shape
    if trim is None:
        trim = 3.1 / ncol
    n_cells = ncol if n_cells is None else int(n_cells)
    if old_results is not None:
        clusters, goc = old_results["clusters"], old_results["cl.goc"]
    else:
        obs = pagoda_gene_clusters_observed(varinfo, trim=trim, n_clusters=n_clusters, n_starts=n_starts,
                                            n_components=n_components, n_internal_shuffles=n_internal_shuffles,
                                            method=method, secondary_correlation=secondary_correlation, seed=seed,
                                            cor_method=cor_method, ctx=ctx)
        clusters, goc = obs["clusters"], obs["cl.goc"]
    if old_results is not None and old_results.get("varm") is not None:
        varm = {k: np.asarray(old_results["varm"][k]) for k in ("n", "var", "round")}
    else:
        varm = pagoda_gene_cluster_samples(ngenes, n_cells, trim, n_clusters=n_clusters, n_samples=n_samples,
                                           method=method, secondary_correlation=secondary_correlation,
                                           cor_method=cor_method, ctx=ctx)
    varm, clvlm, tci = rmt.score_varm(varm, n_cells)
    xf = rmt.gumbel_fit(varm["varst"])
    return {"clusters": clusters, "xf": xf, "tci": tci, "cl.goc": goc, "varm": varm, "clvlm": clvlm, "trim": trim}
