"""A numpy restatement of scde_amd/views.py (``pagoda.view.aspects``, ``c.view.pathways`` as
``pagoda.show.pathways`` calls it, ``t.view.pathways``; R/functions.R:2704-2748, 5623-5969) with
every weighted PCA from oracle/wpca.py, winsorize from oracle/pagoda.py, the trees from
test_hclust.py's ``ref_hclust`` and ``dist`` from rdist_ref.py.  The reference of
tests/test_views.py and tests/test_gpu_views.py, and the maker of their synthetic case."""
import math
import warnings

import numpy as np

from knn_ref import average_rank, quantile7
from oracle import pagoda as OP
from oracle import wpca as W
from rdist_ref import rdist
from test_hclust import ref_hclust

G, C = 240, 96  # the size tests/test_gpu_wpca.py's pathway test uses
SET_A = [f"g{i}" for i in range(0, 30)]
SET_B = [f"g{i}" for i in range(20, 50)]   # shares g20 .. g29 with A
SET_C = [f"g{i}" for i in range(100, 125)]  # carries no pattern


def make_case(seed=5, strength=1.0):
    """{"mat", "matw" (genes x cells), "genes", "batch"}, the gene sets and the planted pattern.
    Genes g0 .. g49 carry the pattern with a loading of their own (distinct magnitudes, every
    fourth negative), the others noise."""
    rng = np.random.default_rng(seed)
    pattern = np.where(np.arange(C) % 3 == 0, 1.0, -0.5) * (1.0 + 0.3 * np.sin(np.arange(C)))
    pattern -= pattern.mean()
    load = np.zeros(G)
    load[:50] = strength * (0.8 + 0.045 * rng.permutation(50)) * np.where(np.arange(50) % 4 == 3, -1.0, 1.0)
    mat = 0.6 * rng.standard_normal((G, C)) + load[:, None] * pattern[None, :] + rng.normal(size=(G, 1))
    matw = rng.uniform(0.3, 1.0, size=(G, C))
    batch = np.array(["a", "b"] * (C // 2))
    varinfo = {"mat": mat, "matw": matw, "genes": [f"g{i}" for i in range(G)], "batch": batch}
    goenv = {"GO:A": list(SET_A), "GO:B": list(SET_B), "GO:C": list(SET_C)}
    return varinfo, goenv, pattern


def r_cor(x, y):
    x = np.asarray(x, np.float64) - np.mean(x)
    y = np.asarray(y, np.float64) - np.mean(y)
    return float((x * y).sum() / np.sqrt((x * x).sum() * (y * y).sum()))


def spearman(x, y):
    return r_cor(average_rank(x), average_rank(y))


def flips(c):
    """The flip rule of both functions: only a negative correlation flips (0 and NaN do not)."""
    return bool(c < 0)


def clamp(d, zlim):
    return np.minimum(np.maximum(d, zlim[0]), zlim[1])


def cor_cols(x):
    """cor() of the columns of x (NaN for a constant column)."""
    xc = x - x.mean(axis=0)
    ss = np.sqrt((xc * xc).sum(axis=0))
    with np.errstate(invalid="ignore", divide="ignore"):
        return (xc.T @ xc) / np.outer(ss, ss)


def tree(dd, method="ward.D"):
    dd = np.where(np.isnan(dd), 1.0, dd)
    np.fill_diagonal(dd, 0.0)
    return ref_hclust(dd, method)


# ------------------------------------------------------------------ pagoda.view.aspects
def view_aspects(xv, top=math.inf):
    xv = np.asarray(xv, np.float64)
    vi = np.arange(xv.shape[0])
    if math.isfinite(top):
        rc = np.var(xv, axis=1, ddof=1)
        vi = np.argsort(-rc, kind="stable")[:min(len(rc), int(top))]
        xv = xv[vi]
    hc = ref_hclust(rdist(xv, "euclidean"), "complete") if xv.shape[0] >= 2 else None
    q = quantile7(xv.ravel(), 0.95)
    return {"vi": vi, "xv": xv, "row_clustering": hc, "rcmvar": np.var(xv, axis=1, ddof=1), "zlim": (-q, q),
            "mat": clamp(xv, (-q, q))}


# ------------------------------------------------------------------ c.view.pathways
def match_names(pathways, names, goenv):
    pathways = list(pathways)
    x = [goenv is not None and p in goenv for p in pathways]
    if any(x):
        if not all(x):
            warnings.warn("WARNING: partial match to pathway names. The following entries did not match: "
                          + " ".join(p for p, k in zip(pathways, x) if not k))
        kept = [p for p, k in zip(pathways, x) if k]
        return kept, {p: list(goenv[p]) for p in kept}
    x = [p in set(names) for p in pathways]
    if any(x):
        if not all(x):
            warnings.warn("WARNING: partial match to gene names. The following entries did not match: "
                          + " ".join(p for p, k in zip(pathways, x) if not k))
        return ["genes"], {"genes": [p for p, k in zip(pathways, x) if k]}
    raise ValueError("ERROR: provided names do not match either gene nor pathway names (if the pathway environment "
                     "was provided)")


def reduced(names, values, how, decreasing):
    """sort(tapply(values, as.factor(names), how), decreasing = .): ties in level (sorted name) order."""
    best = {}
    for g, v in zip(names, values):
        best[g] = v if g not in best else how(best[g], v)
    lv = sorted(best)
    vals = np.array([best[g] for g in lv])
    o = np.argsort(-vals if decreasing else vals, kind="stable")
    return [(lv[i], float(vals[i])) for i in o]


def select(names, values, n_genes, two_sided):
    if two_sided:
        k = int(round(n_genes / 2))
        pos = reduced(names, values, max, True)
        neg = reduced(names, values, min, False)
        lab = []
        for g, _ in pos[:k] + neg[:k]:
            if g not in lab:
                lab.append(g)
        return lab
    return [g for g, _ in reduced(names, np.abs(values), max, True)[:int(n_genes)]]


def pathway_pcas(varinfo, p_genes, n_components, trim=0, seed=1):
    mat = np.asarray(varinfo["mat"], np.float64)
    if trim > 0:
        mat = OP.winsorize_matrix(mat, trim)
    names = list(varinfo["genes"])
    members = {g for v in p_genes.values() for g in v}
    gvi = np.array([g in members for g in names])
    sub_names = [g for g, k in zip(names, gvi) if k]
    res = W.pagoda_pathway_wPCA(mat[gvi], np.asarray(varinfo["matw"])[gvi], sub_names, p_genes,
                                n_components=n_components, min_pathway_size=0, max_pathway_size=math.inf,
                                n_randomizations=0, n_internal_shuffles=0, n_starts=2, batch=varinfo.get("batch"),
                                seed=seed)
    # the names of a pathway's rotation rows: its genes in matrix order, constant rows dropped
    cm = W.weighted_mat_center(mat[gvi], np.asarray(varinfo["matw"])[gvi], varinfo.get("batch"))
    live = np.abs(np.diff(cm, axis=1)).sum(axis=1) > 0
    for p, r in res.items():
        if r is not None:
            r["xp"]["rotation_names"] = [g for g, k in zip(sub_names, live) if k and g in set(p_genes[p])]
            assert len(r["xp"]["rotation_names"]) == r["n"]
    return res, mat


def scaled_loadings(ppca, pathways, n_pc):
    sn, sv = [], []
    for p, k in zip(pathways, n_pc):
        r = ppca.get(p)
        if r is None:
            continue
        gl = r["xp"]["rotation"][:, k - 1] * r["xp"]["sd"].ravel()[k - 1] / math.sqrt(r["n"])
        sn += r["xp"]["rotation_names"]
        sv += gl.tolist()
    return sn, np.array(sv)


def finish(xp, lab, d, dw, cpc, zlim, cell_clustering, weight_by_rotation, use_spearman):
    d = d - d.mean(axis=1)[:, None]
    hc = tree(1.0 - np.abs(cor_cols(d.T))) if len(lab) > 2 else None
    row_order = hc[2].copy() if hc is not None else np.arange(1, len(lab) + 1)
    vhc = cell_clustering if cell_clustering is not None else tree(1.0 - cor_cols(d))
    if zlim is None:
        zlim = (quantile7(d.ravel(), 0.01), quantile7(d.ravel(), 0.99))
    out = dict(xp)
    if weight_by_rotation:
        aval = (d * dw * np.abs(xp["rotation"][:, cpc])[:, None]).sum(axis=0) / dw.sum(axis=0)
    else:
        aval = (d * dw).sum(axis=0) / dw.sum(axis=0)
    if xp.get("scores") is not None:
        out["scores"], out["rotation"] = xp["scores"].copy(), xp["rotation"].copy()
        oc = out["scores"][:, cpc].copy()
        if flips(spearman(oc, aval) if use_spearman else r_cor(oc, aval)):
            oc = -oc
            out["scores"][:, cpc] *= -1.0
            out["rotation"][:, cpc] *= -1.0
        out["oc"] = oc
    out.update(vhc=vhc, lab=list(lab), hc=hc, row_order=row_order, vmap=clamp(d, zlim), zlim=tuple(zlim), aval=aval)
    return out


def show_pathways(pathways, varinfo, goenv=None, n_genes=20, two_sided=False, n_pc=None, zlim=None,
                  cell_clustering=None, trim=0, seed=1):
    """The details dict of ``pagoda_show_pathways`` (None when fewer than 3 genes remain)."""
    names = list(varinfo["genes"])
    pathways, p_genes = match_names(pathways, names, goenv)
    n_pc = [1] * len(pathways) if n_pc is None else list(n_pc)
    ppca, mat = pathway_pcas(varinfo, p_genes, max(n_pc), trim, seed)
    matw = np.asarray(varinfo["matw"], np.float64)
    row = {}
    for i, g in enumerate(names):
        row.setdefault(g, i)
    if len(ppca) > 1:
        sn, sv = scaled_loadings(ppca, pathways, n_pc)
        lab = select(sn, sv, n_genes, two_sided)
        if len(lab) < 3:
            return None
        if trim > 0:
            mat = OP.winsorize_matrix(mat, trim)
        ii = [row[g] for g in lab]
        d, dw = mat[ii], matw[ii]
        mem = W.RState(seed)
        for r in ppca.values():
            if r is not None:
                mem.unif_rand(2 * r["n"] * min(max(n_pc), r["n"]))
        xp = W.bwpca(d.T, dw.T, npcs=1, center=False, nstarts=3, rstate=mem)
        xp["rotation_names"] = list(lab)
        cpc = 1
    else:
        r = next(iter(ppca.values()))
        if r is None:
            return None
        xp = dict(r["xp"])
        k = n_pc[0]
        o = np.argsort(-np.abs(xp["rotation"][:, k - 1]), kind="stable")
        lab = [xp["rotation_names"][i] for i in o]
        if len(lab) > n_genes:
            lab = lab[:n_genes]
            xp["rotation"] = xp["rotation"][o[:n_genes]]
            xp["rotation_names"] = list(lab)
        ii = [row[g] for g in lab]
        d, dw = mat[ii], matw[ii]
        cpc = k
    out = finish(xp, lab, d, dw, cpc - 1, zlim, cell_clustering, True, False)
    out["consensus_pc"] = cpc
    return out


def pathway_genes(names, varinfo, goenv=None, n_pc=1, cell_clustering=None, trim=None, zlim=None, seed=1):
    """``t.view.pathways``."""
    mat = np.asarray(varinfo["mat"], np.float64)
    matw = np.asarray(varinfo["matw"], np.float64)
    gn = list(varinfo["genes"])
    members = {g for p in names if goenv is not None and p in goenv for g in goenv[p]}
    lab = [i for i, g in enumerate(gn) if g in members]
    if not lab:
        lab = [i for i, g in enumerate(gn) if g in set(names)]
    if not lab:
        return None
    if trim is None:
        trim = 1.1 / mat.shape[1]
    if trim > 0:
        mat = OP.winsorize_matrix(mat, trim)
    d, dw = mat[lab], matw[lab]
    xp = {}
    if len(lab) > 2:
        xp = W.bwpca(d.T, dw.T, npcs=n_pc, center=False, nstarts=3, rstate=W.RState(seed))
    out = finish(xp, lab, d, dw, n_pc - 1, zlim, cell_clustering, False, True)
    out["lab_names"] = [gn[i] for i in lab]
    return out
