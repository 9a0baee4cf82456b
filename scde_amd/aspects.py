"""PAGODA's aspect redundancy reduction on the GPU (csrc/aspects.hip; contract in
include/scde_hip.h): the two steps between ``pagoda.top.aspects`` and ``pagoda.cluster.cells``.

  * ``pathway_pc_correlation_distance``     R/functions.R:5126-5164
  * ``collapse_aspect_clusters``            R/functions.R:5166-5198
  * ``pagoda_reduce_loading_redundancy``    R/functions.R:2490-2526
  * ``pagoda_reduce_redundancy``            R/functions.R:2559-2610

A ``tam`` / ``tamr`` structure is a dict: "xv" and "xvw" (aspects x cells, float64), "names" (the
row names, ``"#PC<k># <set name>"``), optionally "cnam" ({row name: [member names]}); any other
key passes through.  ``pwpca`` is what ``pagoda_pathway_wPCA`` returns, ``clpca`` what
``pagoda_gene_clusters`` returns (its "cl.goc" is used): per set an "xp" with "rotation" and
"rotation_names".  ``plot``, ``n.cores`` and ``...`` are not restated.

Within one call the patterns, their weights, the m x m matrices and the collapsed result stay in
HBM; the loading lists go up, and only the tree, the labels and the final outputs come back.

One deviation from R: the Student-t renormalisation is the odd map in
correlation space everywhere, also on the far negative side where R's double evaluation
underflows and keeps r.
"""
from __future__ import annotations

import ctypes
import math
import re

import numpy as np

from . import api
from ._lib import check, lib
from .cluster import METHODS, _hclust_dev, _method_code, cutree

_PC = re.compile(r"^#PC(\d+)# ")


def parse_aspect_names(names):
    """[(set name, 1-based component)] of row names ``"#PC<k># <set name>"``."""
    out = []
    for nam in names:
        m = _PC.match(str(nam))
        if not m:
            raise ValueError(f"aspect name {nam!r} is not of the form '#PC<k># <set name>'")
        out.append((str(nam)[m.end():], int(m.group(1))))
    return out


def loading_lists(pcc, names):
    """(rotn, [(i, v)]): the genes of the named sets in order of first appearance, and per aspect
    its rotation column minus its own mean, ordered by increasing (0-based) index into rotn."""
    parsed = parse_aspect_names(names)
    rotn = {}
    for pnam, _ in parsed:
        if pnam not in pcc or pcc[pnam] is None:
            raise ValueError(f"no principal components for the set {pnam!r}")
        for g in pcc[pnam]["xp"]["rotation_names"]:
            rotn.setdefault(str(g), len(rotn))
    pl = []
    for (pnam, pn), nam in zip(parsed, names):
        xp = pcc[pnam]["xp"]
        rot = np.asarray(xp["rotation"], dtype=np.float64)
        if rot.ndim == 1:
            rot = rot[:, None]
        if not 1 <= pn <= rot.shape[1]:
            raise ValueError(f"{nam!r}: the set has {rot.shape[1]} component(s)")
        rt = rot[:, pn - 1]
        mi = np.array([rotn[str(g)] for g in xp["rotation_names"]], dtype=np.int32)
        if len(mi) != len(rt):
            raise ValueError(f"{pnam!r}: rotation and rotation_names differ in length")
        mo = np.argsort(mi, kind="stable")
        pl.append((mi[mo], (rt - rt.mean())[mo]))
    return list(rotn), pl


def _merge_pcc(pwpca, clpca):
    pcc = dict(clpca["cl.goc"]) if clpca is not None else {}
    pcc.update(pwpca)  # c(pwpca, clpca$cl.goc)[[name]] is the first of a name
    return pcc


class _Dev:
    """Device buffers of one call, freed together."""

    def __init__(self, ctx):
        self.ctx, self.L, self.bufs = ctx, lib(), []

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        check(self.L.scde_dev_alloc(self.ctx.handle, max(int(nbytes), 8), ctypes.byref(p)))
        self.bufs.append(p)
        return p

    def put(self, a):
        p = self.alloc(a.nbytes)
        check(self.L.scde_h2d(self.ctx.handle, p, api._p(a), a.nbytes))
        return p

    def get(self, p, shape, order="F"):
        out = np.zeros(shape, order=order)
        check(self.L.scde_d2h(self.ctx.handle, api._p(out), p, out.nbytes))
        return out

    def free(self, failing=False):
        for p in self.bufs:
            rc = self.L.scde_dev_free(self.ctx.handle, p)
            if not failing:  # (a failure to free must not replace the error on its way out)
                check(rc)
        self.bufs = []


def _run(ctx, body):
    ctx = ctx or api.default_context()
    dev = _Dev(ctx)
    try:
        out = body(dev)
    except BaseException:
        dev.free(failing=True)
        raise
    dev.free()
    return out


def _tam_arrays(tam):
    xv = np.ascontiguousarray(tam["xv"], dtype=np.float64)
    xvw = np.ascontiguousarray(tam["xvw"], dtype=np.float64)
    names = [str(n) for n in tam["names"]]
    if xv.ndim != 2 or xvw.shape != xv.shape:
        raise ValueError("tam['xv'] and tam['xvw'] must be matrices of the same shape (aspects x cells)")
    if len(names) != xv.shape[0]:
        raise ValueError(f"tam['names'] has {len(names)} entries for {xv.shape[0]} aspects")
    if xv.shape[0] < 2:
        raise ValueError("at least 2 aspects are needed")
    if xv.shape[1] < 2:
        raise ValueError("at least 2 cells are needed")
    return xv, xvw, names


def _loading_cr_dev(dev, pl, target_ndf):
    """The (renormalised) loading correlations of the lists pl, m x m, resident."""
    m = len(pl)
    off = np.zeros(m + 1, np.int64)
    off[1:] = np.cumsum([len(i) for i, _ in pl])
    idx = np.ascontiguousarray(np.concatenate([np.asarray(i, np.int32) for i, _ in pl]), np.int32)
    val = np.ascontiguousarray(np.concatenate([np.asarray(v, np.float64) for _, v in pl]))
    if idx.size == 0:
        idx, val = np.zeros(1, np.int32), np.zeros(1)
    r = dev.alloc(8 * m * m)
    n = dev.alloc(4 * m * m)
    check(dev.L.scde_plSemicompleteCor2_dev(dev.ctx.handle, m, api._p(off), api._p(idx), api._p(val), r, n))
    if target_ndf is None:
        return r
    cr = dev.alloc(8 * m * m)
    check(dev.L.scde_t_renorm_dev(dev.ctx.handle, r, n, m, float(target_ndf), cr))
    return cr


def _check_target(target_ndf):
    if target_ndf is not None and not (math.isfinite(target_ndf) and target_ndf > 2):
        raise ValueError("target_ndf must be finite and above 2")


def pathway_pc_correlation_distance(pcc, names, target_ndf=None, ctx: api.Context | None = None):
    """R/functions.R:5126-5164: 1 - |cr| (negatives set to 0) of the loading correlations cr of
    the named aspects, renormalised to ``target_ndf`` degrees of freedom when given; an m x m
    matrix with a zero diagonal.  ``pcc``: {set name: {"xp": {"rotation", "rotation_names"}}}."""
    _check_target(target_ndf)
    names = [str(n) for n in names]
    if len(names) < 2:
        raise ValueError("at least 2 aspects are needed")
    _, pl = loading_lists(pcc, names)
    m = len(names)
    cr = _run(ctx, lambda dev: dev.get(_loading_cr_dev(dev, pl, target_ndf), (m, m)))
    d = 1.0 - np.abs(cr)
    d[d < 0] = 0.0
    np.fill_diagonal(d, 0.0)
    return d


def _clusters(ct):
    """(labels in increasing order, member rows per label)."""
    ct = np.asarray(ct)
    labels = np.unique(ct)
    return labels, [np.nonzero(ct == c)[0].astype(np.int32) for c in labels]


def _collapse_dev(dev, xd, wd, ncells, m, ct, names, scale, pick_top, seed):
    """collapse.aspect.clusters on resident patterns: (d, w) resident as ncells x nclust, the
    cluster row names, the member lists and {"top", "fallback", "orientation"}."""
    from .pagoda import RState
    if len(ct) != m:
        raise ValueError(f"ct has {len(ct)} labels for {m} aspects")
    _, members = _clusters(ct)
    k = len(members)
    off = np.zeros(k + 1, np.int64)
    off[1:] = np.cumsum([len(ii) for ii in members])
    idx = np.ascontiguousarray(np.concatenate(members), np.int32)
    dd = dev.alloc(8 * ncells * k)
    dw = dev.alloc(8 * ncells * k)
    top = np.zeros(k, np.int32)
    fb = np.zeros(k, np.int32)
    orient = np.zeros(k)
    check(dev.L.scde_collapse_aspects_dev(dev.ctx.handle, xd, wd, ncells, m, k, api._p(off), api._p(idx),
                                          int(bool(scale)), int(bool(pick_top)), dd, dw, api._p(top), api._p(fb),
                                          api._p(orient)))
    multi = np.array([len(ii) > 1 for ii in members]) & (not pick_top)
    bad = np.nonzero(multi & (fb == 0) & ~np.isfinite(orient))[0]
    if len(bad):
        raise ValueError(f"cluster {int(bad[0]) + 1}: the correlation of its first component with the weighted mean "
                         "of its rows is not finite (R stops here: missing value where TRUE/FALSE needed)")
    if fb.any():
        # R draws from the session stream; here set.seed(seed) once per call, consumed by the
        # clusters that fall back, in output order, ncells normals each
        st = RState(seed)
        for p in np.nonzero(fb)[0]:
            z = np.empty(ncells)
            check(dev.L.scde_r_norm_rand(api._p(st.w), ncells, api._p(z)))
            z = np.abs(z * 1e-6)
            check(dev.L.scde_h2d(dev.ctx.handle, ctypes.c_void_p(dd.value + 8 * ncells * int(p)), api._p(z), z.nbytes))
    return dd, dw, [names[t] for t in top], members, {"top": top, "fallback": fb, "orientation": orient}


def collapse_aspect_clusters(d, dw, ct, names, scale=True, pick_top=False, seed=1, ctx: api.Context | None = None):
    """R/functions.R:5166-5198.  ``d``, ``dw``: aspects x cells; ``ct``: a label per aspect;
    clusters come out in increasing label order.  Returns {"d", "w", "names"}: per cluster its
    pattern (the row itself for one row; with ``pick_top`` the row of largest variance; else the
    scores of the first principal component of its centred rows, oriented along the mean of its
    rows weighted by |loading| and, with ``scale``, given the largest row variance), its weights
    and the name of its row of largest variance.  A cluster whose scores are constant (or all
    zero after scaling) becomes ``|rnorm(cells, sd = 1e-6)|`` from ``set.seed(seed)``, the
    clusters that fall back drawing in output order."""
    x = np.ascontiguousarray(d, dtype=np.float64)
    w = np.ascontiguousarray(dw, dtype=np.float64)
    names = [str(n) for n in names]
    if x.ndim != 2 or w.shape != x.shape:
        raise ValueError("d and dw must be matrices of the same shape (aspects x cells)")
    m, ncells = x.shape
    if len(names) != m or len(ct) != m:
        raise ValueError(f"names and ct must have one entry per aspect ({m})")
    if m < 1 or ncells < 2:
        raise ValueError("at least 1 aspect and 2 cells are needed")

    def body(dev):
        dd, dwd, rn, _, _ = _collapse_dev(dev, dev.put(x), dev.put(w), ncells, m, ct, names, scale, pick_top, seed)
        return {"d": dev.get(dd, (len(rn), ncells), "C"), "w": dev.get(dwd, (len(rn), ncells), "C"), "names": rn}
    return _run(ctx, body)


def _cnam(tam, names, members, rn):
    """The collapsed names of R/functions.R:2516-2521."""
    old = tam.get("cnam")
    out = {}
    for key, ii in zip(rn, members):
        xn = [names[i] for i in ii]
        out[key] = [g for n in xn for g in old.get(n, [])] if old is not None else xn
    return out


def pagoda_reduce_loading_redundancy(tam, pwpca, clpca=None, cluster_method="complete", distance_threshold=0.01,
                                     corr_power=4, abs=True, seed=1, return_details=False,
                                     ctx: api.Context | None = None):
    """R/functions.R:2490-2526: aspects whose gene loadings and cell patterns both agree are
    collapsed.  The distance is (1 - sqrt((1 - pclc) (1 - (1 - cda))))^corr_power with pclc the
    loading distance at ``target_ndf = 100`` and cda |cor| of the patterns (or cor with negatives
    set to 0 when ``abs`` is false); then ``hclust``, ``cutree(h = distance_threshold)`` and
    ``collapse_aspect_clusters(scale=True)``.  Returns ``tam`` with "xv", "xvw", "names" and
    "cnam" replaced; with ``return_details`` also "distance" (read back), "clustering", "ct"."""
    _method_code(cluster_method)
    xv, xvw, names = _tam_arrays(tam)
    m, ncells = xv.shape
    _, pl = loading_lists(_merge_pcc(pwpca, clpca), names)

    def body(dev):
        xd, wd = dev.put(xv), dev.put(xvw)
        cr = _loading_cr_dev(dev, pl, 100)
        dist = dev.alloc(8 * m * m)
        check(dev.L.scde_aspect_distance_dev(dev.ctx.handle, xd, ncells, m, cr, int(bool(abs)), float(corr_power),
                                             dist))
        return _finish(dev, tam, names, xd, wd, ncells, m, dist, cluster_method, distance_threshold, seed,
                       return_details)
    return _run(ctx, body)


def _finish(dev, tam, names, xd, wd, ncells, m, dist, method, threshold, seed, return_details, trim=0,
            top=math.inf):
    hc = _hclust_dev(dev.ctx, dist, m, method, list(names))
    ct = cutree(hc, h=threshold)
    dd, dw, rn, members, _ = _collapse_dev(dev, xd, wd, ncells, m, ct, names, True, False, seed)
    k = len(rn)
    cnam = _cnam(tam, names, members, rn)
    if trim > 0:  # winsorize.matrix: above 0.5 a count of cells
        wz = dev.alloc(8 * ncells * k)
        check(dev.L.scde_winsorize_dev(dev.ctx.handle, dd, ncells, k, float(trim / ncells if trim > 0.5 else trim),
                                       wz))
        dd = wz
    d = dev.get(dd, (k, ncells), "C")
    w = dev.get(dw, (k, ncells), "C")
    out = dict(tam)
    if trim > 0 or top != math.inf:
        var = d.var(axis=1, ddof=1)
        vi = np.argsort(-var, kind="stable")[:int(min(k, top))]  # order(decreasing = TRUE) keeps ties in place
        d, w, rn = d[vi], w[vi], [rn[i] for i in vi]
    out.update(xv=d, xvw=w, names=rn, cnam={key: cnam[key] for key in rn})
    if return_details:
        out.update(distance=dev.get(dist, (m, m)), clustering=hc, ct=ct)
    return out


def pagoda_reduce_redundancy(tamr, distance_threshold=0.2, cluster_method="complete", distance=None,
                             weighted_correlation=True, top=math.inf, trim=0, abs=False, seed=1,
                             return_details=False, ctx: api.Context | None = None):
    """R/functions.R:2559-2610: aspects with similar cell patterns are collapsed.  The distance
    is 1 - matWCorr(t(xv), t(xvw)) (``weighted_correlation``), 1 - cor, the |.| form of either
    (``abs``), or the caller's ``distance`` (m x m; its lower triangle is read); then ``hclust``,
    ``cutree(h = distance_threshold)``, ``collapse_aspect_clusters(scale=True)``, the optional
    ``winsorize_matrix(trim)`` of the collapsed patterns (which is what is returned), and the
    rows ordered by decreasing variance (stable on ties), the first ``min(rows, top)`` kept."""
    _method_code(cluster_method)
    xv, xvw, names = _tam_arrays(tamr)
    m, ncells = xv.shape
    if not top >= 1:
        raise ValueError("top must be at least 1")
    if not 0 <= trim < ncells:
        raise ValueError("trim must be in [0, cells)")
    if distance is not None:
        distance = np.asfortranarray(distance.values if hasattr(distance, "values") else distance, dtype=np.float64)
        if distance.shape != (m, m):
            raise ValueError(f"distance must be {m} x {m}")

    def body(dev):
        xd, wd = dev.put(xv), dev.put(xvw)
        if distance is not None:
            dist = dev.put(distance)
        else:
            dist = dev.alloc(8 * m * m)
            if weighted_correlation:
                check(dev.L.scde_matWCorr_distance_dev(dev.ctx.handle, xd, wd, ncells, m, int(bool(abs)), dist))
            else:
                check(dev.L.scde_aspect_distance_dev(dev.ctx.handle, xd, ncells, m, None, int(bool(abs)), 1.0, dist))
        # the rows are always put in variance order here (R orders them whatever top is)
        return _finish(dev, tamr, names, xd, wd, ncells, m, dist, cluster_method, distance_threshold, seed,
                       return_details, trim=trim, top=min(top, m))
    return _run(ctx, body)


__all__ = ["METHODS", "collapse_aspect_clusters", "loading_lists", "pagoda_reduce_loading_redundancy",
           "pagoda_reduce_redundancy", "parse_aspect_names", "pathway_pc_correlation_distance"]
