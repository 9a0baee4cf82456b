"""The walkthroughs' views of a PAGODA result, returned as data (no plots):

  * ``pagoda_view_aspects``    ``pagoda.view.aspects`` and the computing half of ``view.aspects``
                               (R/functions.R:2704-2748)
  * ``pagoda_show_pathways``   ``pagoda.show.pathways`` / ``c.view.pathways`` up to ``if(plot)``
                               (R/functions.R:5762-5969): the cell pattern of one or several
                               pathways, which ``pagoda_subtract_aspect`` takes
  * ``view_pathway_genes``     ``t.view.pathways`` (R/functions.R:5623-5736): the same steps for a
                               fixed gene list, what the PAGODA app shows per gene heat map

Everything numeric runs in kernels the package already has: the weighted PCAs (``wpca.hip``),
the correlation distances (``scde_cor_distance_dev``, ``scde_matCorr``), ``hclust``, ``dist`` and
winsorize.  What is left on the host works on the 20 or so selected genes x cells.

Written from how the reference reads; nothing here was checked against a run of R beyond the
numpy restatement in tests/views_ref.py.
"""
from __future__ import annotations

import ctypes
import math
import warnings

import numpy as np

from . import api
from ._lib import ScdeError, check, lib
from .cluster import _hclust_dev, hclust, hclust_dist
from .knn import _average_rank, _quantile7
from .pagoda import RState, _pathway_wpca, _r_cor, bwpca, matCorr, pagoda_pathway_wPCA, winsorize_matrix


def _names_of(varinfo, n):
    genes = varinfo.get("genes")
    return [str(g) for g in genes] if genes is not None else [str(i) for i in range(n)]


def _first_rows(names):
    row = {}
    for i, g in enumerate(names):
        row.setdefault(g, i)  # R's mat[name, ]: the first row of a name
    return row


def _clamp(d, zlim):
    return np.minimum(np.maximum(d, zlim[0]), zlim[1])


def _gene_tree(d):
    """hclust(as.dist(1 - abs(cor(t(d)))), "ward.D") with NA -> 1; None below 3 genes."""
    if d.shape[0] < 3:
        return None
    c = matCorr(d.T, d.T)
    dd = 1.0 - np.abs(c)
    dd[np.isnan(dd)] = 1.0
    np.fill_diagonal(dd, 0.0)
    return hclust(dd, "ward.D")


def _cell_tree(d, ctx):
    """hclust(as.dist(1 - cor(d)), "ward.D") with NA -> 1.  The cells x cells distance is formed
    and clustered in HBM; only when it holds a NaN (a cell constant over the genes) is it read
    back, mended and clustered from the host."""
    x = np.asfortranarray(d)  # genes x cells column-major: the cells are the columns
    g, n = x.shape
    L = lib()
    xd, dd = ctypes.c_void_p(), ctypes.c_void_p()
    check(L.scde_dev_alloc(ctx.handle, x.nbytes, ctypes.byref(xd)))
    try:
        check(L.scde_dev_alloc(ctx.handle, 8 * n * n, ctypes.byref(dd)))
        try:
            check(L.scde_h2d(ctx.handle, xd, api._p(x), x.nbytes))
            check(L.scde_cor_distance_dev(ctx.handle, xd, g, n, dd))
            try:
                return _hclust_dev(ctx, dd, n, "ward.D")
            except ScdeError as e:
                if "non-finite" not in str(e):
                    raise
            m = np.zeros((n, n), order="F")
            check(L.scde_d2h(ctx.handle, api._p(m), dd, m.nbytes))
        finally:
            L.scde_dev_free(ctx.handle, dd)
    finally:
        L.scde_dev_free(ctx.handle, xd)
    m[np.isnan(m)] = 1.0
    return hclust(m, "ward.D", ctx=ctx)


def _spearman(x, y):
    return _r_cor(_average_rank(np.asarray(x, np.float64)), _average_rank(np.asarray(y, np.float64)))


# ================================================================== pagoda.view.aspects
def pagoda_view_aspects(tamr, row_clustering=None, top=math.inf, ctx: api.Context | None = None):
    """``pagoda.view.aspects(tamr, row.clustering, top)`` as data.  ``tamr``: {"xv", "xvw":
    aspects x cells, "cnam" (optional)}.  A finite ``top`` keeps the ``top`` rows of largest
    variance (``order(decreasing = TRUE)``: ties by index).  The default ``row_clustering`` is
    ``hclust(dist(xv))`` (complete linkage) of the rows kept -- R evaluates the default after the
    selection -- with the distance matrix formed and clustered in HBM; for a single row, where R's
    ``hclust`` stops, it is None.  Returns {"xv", "xvw", "cnam": the rows kept; "row_clustering";
    "rcmvar": their variance; "zlim": -+ quantile(xv, 0.95), type 7; "mat": xv clamped to zlim}."""
    xv = np.asarray(tamr["xv"], dtype=np.float64)
    xvw = tamr.get("xvw")
    cnam = tamr.get("cnam")
    if xv.ndim != 2 or xv.shape[0] < 1:
        raise ValueError("tamr['xv'] must be an aspects x cells matrix")
    if math.isfinite(top):
        if top < 1:
            raise ValueError("top must be at least 1")
        rc = np.var(xv, axis=1, ddof=1)
        vi = np.argsort(-rc, kind="stable")[:min(len(rc), int(top))]
        xv = xv[vi]
        if xvw is not None:
            xvw = np.asarray(xvw)[vi]
        if cnam is not None:
            cnam = [cnam[i] for i in vi] if isinstance(cnam, (list, tuple)) else np.asarray(cnam, dtype=object)[vi]
    if row_clustering is None and xv.shape[0] >= 2:
        row_clustering = hclust_dist(xv, "euclidean", "complete", ctx=ctx)
    rcmvar = np.var(xv, axis=1, ddof=1)
    q = _quantile7(xv.ravel(), 0.95)
    zlim = (-q, q)
    return {"xv": xv, "xvw": xvw, "cnam": cnam, "row_clustering": row_clustering, "rcmvar": rcmvar, "zlim": zlim,
            "mat": _clamp(xv, zlim)}


# ================================================================== pagoda.show.pathways
def _match_names(pathways, names, goenv):
    """c.view.pathways' first step (R/functions.R:5777-5801): (pathway names, {name: genes})."""
    pathways = [str(p) for p in ([pathways] if isinstance(pathways, str) else pathways)]
    x = [goenv is not None and p in goenv for p in pathways]
    if any(x):
        if not all(x):
            warnings.warn("WARNING: partial match to pathway names. The following entries did not match: "
                          + " ".join(p for p, k in zip(pathways, x) if not k))
        kept = [p for p, k in zip(pathways, x) if k]
        return kept, {p: [str(g) for g in goenv[p]] for p in kept}
    present = set(names)
    x = [p in present for p in pathways]
    if any(x):
        if not all(x):
            warnings.warn("WARNING: partial match to gene names. The following entries did not match: "
                          + " ".join(p for p, k in zip(pathways, x) if not k))
        return ["genes"], {"genes": [p for p, k in zip(pathways, x) if k]}
    raise ValueError("ERROR: provided names do not match either gene nor pathway names (if the pathway environment "
                     "was provided)")


def _reduce(names, values, how, decreasing):
    """sort(tapply(values, as.factor(names), how), decreasing): [(name, value)], ties in the
    order of the sorted names."""
    best = {}
    for g, v in zip(names, values):
        best[g] = v if g not in best else how(best[g], v)
    lv = sorted(best)
    vals = np.array([best[g] for g in lv])
    o = np.argsort(-vals if decreasing else vals, kind="stable")
    return [(lv[i], vals[i]) for i in o]


def _select_genes(scaled_names, scaled_values, n_genes, two_sided):
    """The genes ``c.view.pathways`` keeps from the scaled loadings of several pathways
    (R/functions.R:5818-5836)."""
    if two_sided:
        k = int(round(n_genes / 2))  # R's round: half to even, as Python's
        pos = _reduce(scaled_names, scaled_values, max, True)
        neg = _reduce(scaled_names, scaled_values, min, False)
        lab = []
        for g, _ in pos[:min(len(pos), k)] + neg[:min(len(neg), k)]:
            if g not in lab:
                lab.append(g)  # the first occurrence of a name
        return lab
    red = _reduce(scaled_names, np.abs(scaled_values), max, True)
    return [g for g, _ in red[:min(len(red), int(n_genes))]]


def _finish(xp, lab, d, dw, cpc, zlim, cell_clustering, weight_by_rotation, spearman, ctx):
    """The common tail (R/functions.R:5869-5920; 5647-5700): trees, zlim, vmap, aval, the flip."""
    d = d - d.mean(axis=1)[:, None]
    hc = _gene_tree(d)
    row_order = hc.order.copy() if hc is not None else np.arange(1, len(lab) + 1, dtype=np.int32)
    vhc = cell_clustering if cell_clustering is not None else _cell_tree(d, ctx)
    if zlim is None:
        flat = d.ravel()
        zlim = (_quantile7(flat, 0.01), _quantile7(flat, 0.99))
    out = dict(xp)
    if weight_by_rotation:
        aval = (d * dw * np.abs(xp["rotation"][:, cpc])[:, None]).sum(axis=0) / dw.sum(axis=0)
    else:
        aval = (d * dw).sum(axis=0) / dw.sum(axis=0)
    if xp.get("scores") is not None:
        out["scores"], out["rotation"] = xp["scores"].copy(), xp["rotation"].copy()
        oc = out["scores"][:, cpc].copy()
        c = _spearman(oc, aval) if spearman else _r_cor(oc, aval)
        if c < 0:
            oc = -oc
            out["scores"][:, cpc] *= -1.0
            out["rotation"][:, cpc] *= -1.0
        out["oc"] = oc
    out.update(vhc=vhc, lab=list(lab), hc=hc, row_order=row_order, vmap=_clamp(d, zlim), zlim=tuple(zlim),
               aval=aval)
    return out


def pagoda_show_pathways(pathways, varinfo, goenv=None, n_genes=20, two_sided=False, n_pc=None, zlim=None,
                         cell_clustering=None, trim=0, return_details=False, device=None,
                         ctx: api.Context | None = None, seed=1):
    """``pagoda.show.pathways`` (R/functions.R:5762-5771; ``c.view.pathways`` 5776-5969 with
    everything from ``if(plot)`` on left out): the weighted PCA of each named pathway -- or of the
    named genes, when no name is a pathway of ``goenv`` -- and from it one cell pattern.

    ``varinfo``: {"mat", "matw": genes x cells, "genes", "batch"}; ``goenv``: {pathway: genes};
    ``n_pc``: the component to use per pathway (1-based, default all 1).  One pathway: its top
    ``n_genes`` genes by absolute loading of that component.  Several: every gene's loading scaled
    by sd / sqrt(n) of its pathway, the per-gene maximum of the absolute values (``two_sided``:
    ``round(n_genes / 2)`` of the largest and of the smallest signed values, the first occurrence
    of a name kept), and the consensus ``bwpca(npcs = 1, center = FALSE, nstarts = 3)`` of the
    genes kept; None when fewer than 3 remain.  Then the row-centred matrix of these genes, the
    gene tree (ward.D on 1 - |cor|, NA -> 1), the cell tree (ward.D on 1 - cor, unless
    ``cell_clustering`` is given), ``zlim`` (the 1% and 99% quantiles), the clamped ``vmap`` and
    the pattern ``oc``, flipped when its Pearson correlation with the loading-weighted mean
    expression is negative.  Partial matches of the names are a ``warnings.warn``, no match a
    ``ValueError``.

    Where R's ``sort`` meets equal loadings it keeps the order of the gene names' factor levels;
    here that is Python's ``sorted``, from which R's locale collation can differ.  The random
    starts follow R's in-memory stream from ``set.seed(seed)``: the pathways' PCAs first, the
    consensus after them.

    ``device``: a ``PagodaDevice`` made from the same ``varinfo``, so that a loop over many
    aspects uploads ``mat`` and ``matw`` once; it needs ``trim == 0`` (it holds the matrix as it
    is).  The results equal those without it bit for bit.

    Returns ``scores[:, 0]`` as R returns ``x$scores[, 1]``; with ``return_details`` a dict: the
    PCA's fields (rotation, scores, scoreweights, var, totvar, sd, rotation_names) plus "vhc",
    "lab", "hc" (an ``HClust``, None below 3 genes), "row_order" (1-based), "oc", "vmap", "zlim",
    "aval" and "consensus_pc" (1-based)."""
    ctx = ctx or (device.ctx if device is not None else api.default_context())
    mat = np.asarray(varinfo["mat"], dtype=np.float64)
    matw = np.asarray(varinfo["matw"], dtype=np.float64)
    names = _names_of(varinfo, mat.shape[0])
    pathways, p_genes = _match_names(pathways, names, goenv)
    n_pc = [1] * len(pathways) if n_pc is None else [int(k) for k in np.atleast_1d(n_pc)]
    if len(n_pc) < len(pathways) or min(n_pc) < 1:
        raise ValueError("n_pc must give a component (1-based) for every pathway")
    if device is not None and trim > 0:
        raise ValueError("device= holds the matrix as it is: trim must be 0")
    members = {g for v in p_genes.values() for g in v}
    gvi = np.array([g in members for g in names])
    if trim > 0:
        mat = np.asarray(winsorize_matrix(mat, trim), dtype=np.float64)
    kw = dict(n_components=max(n_pc), min_pathway_size=0, max_pathway_size=math.inf, n_randomizations=0,
              n_internal_shuffles=0, n_starts=2)
    if device is not None:
        ppca = _pathway_wpca(device, p_genes, verbose=0, seed=seed, rand_seed=1, em_tol=1e-6, em_maxiter=25, **kw)
    else:
        sub = {"mat": mat[gvi], "matw": matw[gvi], "genes": [g for g, k in zip(names, gvi) if k],
               "batch": varinfo.get("batch")}
        ppca = pagoda_pathway_wPCA(sub, p_genes, seed=seed, ctx=ctx, **kw)
    row = _first_rows(names)
    if len(ppca) > 1:
        sn, sv = [], []
        for p, k in zip(pathways, n_pc):
            r = ppca.get(p)
            if r is None:
                continue
            gl = r["xp"]["rotation"][:, k - 1] * r["xp"]["sd"].ravel()[k - 1] / math.sqrt(r["n"])
            sn += list(r["xp"]["rotation_names"])
            sv += gl.tolist()
        lab = _select_genes(sn, np.array(sv), n_genes, two_sided)
        if len(lab) < 3:
            return None
        if trim > 0:
            mat = np.asarray(winsorize_matrix(mat, trim), dtype=np.float64)  # (the reference trims again)
        ii = [row[g] for g in lab]
        d, dw = mat[ii], matw[ii]
        # the consensus draws its starts where the pathways' PCAs left R's in-memory stream
        mem = RState(seed)
        for r in ppca.values():
            if r is not None:
                mem.unif_rand(2 * r["n"] * min(max(n_pc), r["n"]))
        xp = bwpca(d.T, dw.T, npcs=1, center=False, nstarts=3, rstate=mem)
        xp["rotation_names"] = list(lab)
        cpc = 1
    else:
        r = next(iter(ppca.values()))
        if r is None:
            return None
        xp = dict(r["xp"])
        k = n_pc[0]
        if k > xp["rotation"].shape[1]:
            raise ValueError(f"n_pc = {k}, but the pathway has {xp['rotation'].shape[1]} component(s)")
        o = np.argsort(-np.abs(xp["rotation"][:, k - 1]), kind="stable")
        lab = [xp["rotation_names"][i] for i in o]
        if len(lab) > n_genes:
            lab = lab[:int(n_genes)]
            xp["rotation"] = xp["rotation"][o[:int(n_genes)]]
            xp["rotation_names"] = list(lab)
        # (with n_genes or fewer genes the reference leaves the rotation in matrix order while d
        # follows lab; kept as it is)
        ii = [row[g] for g in lab]
        d, dw = mat[ii], matw[ii]
        cpc = k
    out = _finish(xp, lab, d, dw, cpc - 1, zlim, cell_clustering, True, False, ctx)
    out["consensus_pc"] = cpc
    return out if return_details else out["scores"][:, 0].copy()


def view_pathway_genes(names, varinfo, goenv=None, n_pc=1, cell_clustering=None, trim=None, zlim=None,
                       ctx: api.Context | None = None, seed=1):
    """``t.view.pathways`` (R/functions.R:5623-5736) without the plot: the rows of ``varinfo``
    whose gene belongs to any of the pathways ``names`` of ``goenv`` -- or, when none does, the
    rows named by ``names`` themselves -- in matrix order; None without any.  The matrix is
    winsorized first (``trim`` defaults to 1.1 / ncells, as in R).  With more than 2 genes
    ``bwpca(npcs = n_pc, center = FALSE, nstarts = 3)`` of the rows (starts from
    ``set.seed(seed)``); then the row-centred matrix, both trees, ``zlim`` and ``vmap`` as in
    ``pagoda_show_pathways``, ``aval = colSums(d * dw) / colSums(dw)``, and component ``n_pc``
    flipped when its Spearman correlation (average ranks) with ``aval`` is negative; exactly 0
    does not flip.

    Returns the PCA's fields (absent below 3 genes) plus "vhc", "lab" (0-based rows), "lab_names",
    "hc" (None below 3 genes), "row_order" (1-based), "oc", "vmap", "zlim", "aval"."""
    ctx = ctx or api.default_context()
    mat = np.asarray(varinfo["mat"], dtype=np.float64)
    matw = np.asarray(varinfo["matw"], dtype=np.float64)
    gn = _names_of(varinfo, mat.shape[0])
    names = [str(p) for p in ([names] if isinstance(names, str) else names)]
    members = {str(g) for p in names if goenv is not None and p in goenv for g in goenv[p]}
    lab = [i for i, g in enumerate(gn) if g in members]
    if not lab:
        lab = [i for i, g in enumerate(gn) if g in set(names)]
    if not lab:
        return None
    if trim is None:
        trim = 1.1 / mat.shape[1]
    if trim > 0:
        mat = np.asarray(winsorize_matrix(mat, trim), dtype=np.float64)
    d, dw = mat[lab], matw[lab]
    xp = {}
    if len(lab) > 2:
        if not 1 <= int(n_pc) <= len(lab):
            raise ValueError(f"n_pc must be in [1, {len(lab)}]")
        xp = bwpca(d.T, dw.T, npcs=int(n_pc), center=False, nstarts=3, rstate=RState(seed))
        xp["rotation_names"] = [gn[i] for i in lab]
    out = _finish(xp, lab, d, dw, int(n_pc) - 1, zlim, cell_clustering, False, True, ctx)
    out["lab_names"] = [gn[i] for i in lab]
    return out


__all__ = ["pagoda_view_aspects", "pagoda_show_pathways", "view_pathway_genes"]
