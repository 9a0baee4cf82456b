"""``scde.error.models`` (R/functions.R:177-200, 2953-3132, 3141-3178, 3215-3409) on the GPU: the
error models the differential-expression path starts from, fitted from a count matrix.

  * ``crossfit_pairs``      the cell pairs calculate.crossfit.models compares, group by group (host)
  * ``error_model_inputs``  everything computed before a cell's mixture fit (csrc/error_models.hip)
  * ``nb2_fit_models``      fit.nb2.mixture.model of every cell (csrc/nb2_fit.hip), ``linear_fit=False``
  * ``scde_error_models``   the whole function: R's joint model matrix

Only ``threshold_segmentation=True`` (R's default in scde.error.models) is built: a pair's
cross-fit is then a threshold rule, and with ``min_count_threshold >= 1`` R's per-pair lists reduce
to closed forms.  With ``linear_fit=True`` the fit is ``knn_fit_models``'
(fit.nb2gth.mixture.model); with ``linear_fit=False`` it is the model of the original publication,
checked against R's stored ``o.ifm`` of the ES/MEF data (tests/test_gpu_error_models.py).  Not
checked against R, which nothing here can run: the sampled pair lists of groups with more than
``max_pairs`` pairs, and ``linear_fit=True`` (no stored R result exists for it).
"""
from __future__ import annotations

import warnings

import numpy as np

from . import api, knn
from ._lib import check, lib

NB2_FIT_STATUS = dict(knn.FIT_STATUS)
NB2_FIT_STATUS.update({2: "no gene has weight in the correlated component",
                       5: "an IRLS system is singular or not finite"})


# ================================================================== stage 1: the pairs (host)
def _codes(groups, C):
    """Integer codes of the groups in R's factor-level (sorted) order; one group without groups."""
    if groups is None:
        return np.zeros(C, np.int32), ["all"]
    g = np.asarray(groups)
    if g.shape != (C,):
        raise ValueError("groups must have one entry per cell")
    if (g.dtype == object and any(v is None for v in g)) or (g.dtype.kind == "f" and np.isnan(g).any()):
        raise NotImplementedError("NA groups (cells left out of the fit) are not built")
    levels, codes = np.unique(g, return_inverse=True)
    return np.ascontiguousarray(codes.reshape(C), np.int32), [str(v) for v in levels]


def _combn2(n):
    """combn(n, 2) as two index vectors, in R's order."""
    i, j = np.triu_indices(n, 1)
    return i, j


def crossfit_pairs(groups, ncells=None, max_pairs=5000, min_pairs_per_cell=10, seed=None):
    """The 2 x P cell pairs (0-based) of calculate.crossfit.models: per group, in R's group order,
    ``combn(ids, 2)``; a group with more than ``max_pairs`` pairs keeps ``unique(c(sample(1:np,
    max.pairs), unlist(lapply(ids, function(id) sample(which(pair holds id),
    min.pairs.per.cell)))))``, drawn with R's generator (``set.seed(seed)``, R >= 3.6 rejection
    sampling) in one stream over the groups.  The sampled lists were not checked against R."""
    C = len(groups) if groups is not None else int(ncells)
    codes, _ = _codes(groups, C)
    max_pairs, mppc = int(max_pairs), int(min_pairs_per_cell)
    if max_pairs < 1 or mppc < 0:
        raise ValueError("max_pairs must be at least 1 and min_pairs_per_cell at least 0")
    rng = None
    out = []
    for g in range(int(codes.max()) + 1 if C else 0):
        ids = np.flatnonzero(codes == g)
        if len(ids) < 2:
            raise ValueError(f"group {g} has a single cell: a cross-fit needs two")
        a, b = _combn2(len(ids))
        npairs = len(a)
        if npairs > max_pairs:
            if seed is None:
                raise ValueError(f"a group of {len(ids)} cells has {npairs} pairs, more than max_pairs = {max_pairs}: "
                                 "give a seed for the random sample, or the pair list as pairs=")
            if rng is None:
                from .pagoda import RState
                rng = RState(seed)
            k = min(npairs, mppc)
            if k > len(ids) - 1:
                raise ValueError("cannot take a sample larger than the population: min_pairs_per_cell exceeds the "
                                 "pairs a cell is part of")
            pick = [rng.sample(npairs, max_pairs).astype(np.int64) - 1]
            for m in range(len(ids)):
                holds = np.flatnonzero((a == m) | (b == m))
                pick.append(holds[rng.sample(len(holds), k).astype(np.int64) - 1])
            pick = np.concatenate(pick)
            pick = pick[np.sort(np.unique(pick, return_index=True)[1])]  # R's unique(): first occurrences
            a, b = a[pick], b[pick]
        out.append(np.stack([ids[a], ids[b]]))
    return np.concatenate(out, axis=1).astype(np.int32) if out else np.zeros((2, 0), np.int32)


def _check_pairs(pairs, codes):
    p = np.asarray(pairs)
    if p.ndim != 2 or p.shape[0] != 2 or not np.issubdtype(p.dtype, np.integer):
        raise ValueError("pairs must be a 2 x P matrix of cell indices")
    C = len(codes)
    if p.size and (p.min() < 0 or p.max() >= C):
        raise ValueError("pairs must hold cell indices in [0, cells)")
    if np.any(p[0] == p[1]) or np.any(codes[p[0]] != codes[p[1]]):
        raise ValueError("a pair must hold two different cells of one group")
    key = np.minimum(p[0], p[1]).astype(np.int64) * C + np.maximum(p[0], p[1])
    if len(np.unique(key)) != len(key):
        raise ValueError("pairs lists a pair twice")
    return np.ascontiguousarray(p, np.int32)


def _partner_lists(pairs, C):
    """The pair list seen from every cell: (offsets of C + 1, partners), in the pairs' order."""
    cell = np.concatenate([pairs[0], pairs[1]])
    other = np.concatenate([pairs[1], pairs[0]])
    when = np.concatenate([np.arange(pairs.shape[1]), np.arange(pairs.shape[1])])
    order = np.lexsort((when, cell))
    off = np.zeros(C + 1, np.int32)
    off[1:] = np.cumsum(np.bincount(cell, minlength=C))
    return off, np.ascontiguousarray(other[order], np.int32)


# ================================================================== stage 2: the inputs
def _stage_args(counts, groups, min_nonfailed, min_count_threshold, min_size_entries, max_pairs, min_pairs_per_cell,
                seed, pairs, library_sizes):
    thr = knn._thr(min_count_threshold)
    if thr < 1:
        raise NotImplementedError("min_count_threshold < 1 is not built (rows of two zero counts then leave R's "
                                  "pair lists and its valid-entry matrix is no longer counts >= threshold)")
    if int(min_nonfailed) != min_nonfailed or min_nonfailed < 0:
        raise ValueError("min_nonfailed must be a non-negative integer")
    dc, mat, N, C = knn._counts_arg(counts)
    codes, levels = _codes(groups, C)
    if np.min(np.bincount(codes)) < 2:
        raise ValueError("every group needs at least two cells")
    if pairs is None:
        pairs = crossfit_pairs(codes, max_pairs=max_pairs, min_pairs_per_cell=min_pairs_per_cell, seed=seed)
    pairs = _check_pairs(pairs, codes)
    host = mat if mat is not None else None
    if library_sizes is None:
        if host is None:
            host = knn._host_counts(knn._fetch_counts(dc))
        ls = knn.estimate_library_sizes(host, min_size_entries, thr)
    else:
        ls = library_sizes
    ls = np.ascontiguousarray(ls, np.float64)
    if ls.shape != (C,) or not np.all(np.isfinite(ls)) or np.any(ls <= 0):
        raise ValueError("library sizes must hold one positive finite value per cell")
    return dc, mat, N, C, codes, levels, pairs, ls, thr, int(min_nonfailed)


def _crossfit(dc, mat, N, C, codes, pairs, ls, thr, min_nonfailed, h, fetch=True):
    off, part = _partner_lists(pairs, C)
    fpm = np.zeros((N, C), order="F") if fetch else None
    fp = np.zeros((N, C), order="F") if fetch else None
    nabove = np.zeros((N, C), np.int32, order="F") if fetch else None
    args = (N, N, C, api._p(codes), api._p(ls), api._p(off), api._p(part), thr, min_nonfailed, api._p(fpm),
            api._p(fp), api._p(nabove))
    if dc is not None:
        check(lib().scde_crossfit_inputs_dev(h, dc.ptr, *args))
    else:
        check(lib().scde_crossfit_inputs_host(h, api._p(mat), *args))
    return fpm, fp, nabove


def _inputs_dict(ls, pairs, fpm, fp, nabove, thr):
    return {"ls": ls, "pairs": pairs, "vi": ~np.isnan(fp), "fpm": fpm, "fail_prior": fp, "nabove": nabove,
            "min_count_threshold": thr}


def error_model_inputs(counts, groups=None, min_nonfailed=3, min_count_threshold=4, min_size_entries=2000,
                       max_pairs=5000, min_pairs_per_cell=10, seed=None, pairs=None, library_sizes=None,
                       ctx: api.Context | None = None):
    """Everything ``scde.error.models`` computes before it fits a cell's mixture model, in
    ``knn_model_inputs``' shape (``knn_fit_models`` and ``nb2_fit_models`` take the dict as it
    stands).  Only the counts go to the device.

    Returns a dict: ``ls`` (cells: ``estimate_library_sizes(counts, min_size_entries,
    min_count_threshold)``), ``pairs`` (2 x P, ``crossfit_pairs``' or the caller's), ``nabove``
    (genes x cells: the group's other paired cells with ``count >= threshold``), ``vi`` (genes x
    cells bool: ``nabove >= min(group size - 1, min_nonfailed)``), ``fpm`` (genes x cells: the mean
    over the group's other cells of ``count / ls``) and ``fail_prior`` (genes x cells: the
    geometric mean over the cell's pairs of the pair's failure posterior), both NaN outside
    ``vi``."""
    dc, mat, N, C, codes, _, pairs, ls, thr, mnf = _stage_args(
        counts, groups, min_nonfailed, min_count_threshold, min_size_entries, max_pairs, min_pairs_per_cell, seed,
        pairs, library_sizes)
    fpm, fp, nabove = _crossfit(dc, mat, N, C, codes, pairs, ls, thr, mnf, knn._handle(dc, ctx))
    return _inputs_dict(ls, pairs, fpm, fp, nabove, thr)


# ================================================================== stage 3b: the nb2 fit
def nb2_fit_models(inputs, counts, iter=50, background_rate=0.1, return_details=False, lds_genes=0,
                   ctx: api.Context | None = None):
    """The per-cell EM mixture fit of the original publication's model (fit.nb2.mixture.model;
    contract in include/scde_hip.h and DESIGN.md section 4.16) on what ``error_model_inputs`` or
    ``knn_model_inputs`` returned: a Poisson(``background_rate``) failure component and a negative
    binomial with ``log mu = corr.b + corr.a log fpm`` and one ``corr.theta`` per cell, mixed by a
    logistic prior in ``log fpm``.

    Returns the cells x 12 model matrix in ``models.MODEL_COLUMNS``' order, the last six columns
    NaN (a failed cell's row is NaN throughout); details as ``knn_fit_models`` (``status``:
    ``NB2_FIT_STATUS``)."""
    return knn._fit_call("nb2", inputs, counts, (float(background_rate),), iter, return_details, lds_genes, ctx)


# ================================================================== the whole function
def scde_error_models(counts, groups=None, min_nonfailed=3, threshold_segmentation=True, min_count_threshold=4,
                      zero_count_threshold=None, min_size_entries=2000, max_pairs=5000, min_pairs_per_cell=10,
                      linear_fit=True, local_theta_fit=None, theta_fit_range=(1e-2, 1e2), iter=50, seed=None,
                      pairs=None, return_details=False, ctx: api.Context | None = None, **unsupported):
    """``scde.error.models``: the input stage, then every cell's mixture fit, both on the GPU; the
    fit starts from the inputs the first stage left on the device.  Returns R's ``jmm`` as
    ``knn_error_models`` does: a DataFrame of the cells' models, columns in
    ``models.MODEL_COLUMNS``' order, rows named by the cells and ordered by group,
    ``.attrs["groups"]`` the rows' groups; ``scde_posteriors``, ``expression_prior`` and
    ``scde_expression_difference`` take it.  A cell whose fit fails is dropped with a warning.

    ``linear_fit=False``: six columns (``conc.b, conc.a, fail.r, corr.b, corr.a, corr.theta``);
    ``linear_fit=True``: get.compressed.v1.model's twelve, or seven with ``local_theta_fit=False``
    (``local_theta_fit`` defaults to ``linear_fit``, as in R).  ``zero_count_threshold`` is accepted
    and ignored: in R it only feeds a default ``prior`` that calculate.individual.models always
    overrides with the cross-fit prior.  ``seed`` is needed only when a group has more than
    ``max_pairs`` pairs; ``pairs`` (2 x P cell indices) replaces the enumeration.  Not built
    (NotImplementedError): ``threshold_segmentation=False``, ``old_cfm``, plots, NA groups,
    ``min_count_threshold < 1``.  With ``return_details``: ``(jmm, details)``, the fit's details and
    the model inputs under ``"inputs"``."""
    import pandas as pd

    from .models import MODEL_COLUMNS
    if not threshold_segmentation:
        raise NotImplementedError("threshold_segmentation = False (the three-component flexmix per pair) is not built")
    for name in ("old_cfm", "save_crossfit_plots", "save_model_plots"):
        if unsupported.pop(name, None):
            raise NotImplementedError(f"{name} is not built")
    if unsupported:
        raise TypeError(f"unexpected arguments: {sorted(unsupported)}")
    local = bool(linear_fit) if local_theta_fit is None else bool(local_theta_fit)
    cells = None if isinstance(counts, api.DeviceCounts) else api._counts_matrix(counts)[2]
    dc, mat, N, C, codes, levels, pairs, ls, thr, mnf = _stage_args(
        counts, groups, min_nonfailed, min_count_threshold, min_size_entries, max_pairs, min_pairs_per_cell, seed,
        pairs, None)
    knn._handle(dc, ctx)
    own = None
    if dc is None:
        own = dc = api.DeviceCounts(ctx or api.default_context(), mat)
    try:
        fpm, fp, nabove = _crossfit(dc, None, N, C, codes, pairs, ls, thr, mnf, dc.ctx.handle, fetch=return_details)
        if linear_fit:
            lo, hi = (float(v) for v in theta_fit_range)
            mm, det = knn._fit_call("knn", None, dc, (int(local), lo, hi, 0.5), iter, True, 0, None)
        else:
            mm, det = knn._fit_call("nb2", None, dc, (0.1,), iter, True, 0, None)
    finally:
        if own is not None:
            own.free()
    names = cells if cells is not None else [str(i) for i in range(C)]
    table = knn.FIT_STATUS if linear_fit else NB2_FIT_STATUS
    for i in np.flatnonzero(det["status"] != 0):
        warnings.warn(f"ERROR encountered in building a model for cell {names[i]} - skipping the cell. Error: "
                      f"{table.get(int(det['status'][i]), 'status %d' % det['status'][i])}")
    order = np.argsort(codes, kind="stable")
    order = order[det["status"][order] == 0]
    if not linear_fit:
        cols = MODEL_COLUMNS[:6]
    else:
        cols = [c for c in MODEL_COLUMNS if local or not c.startswith("corr.ltheta.")]
    jmm = pd.DataFrame({c: mm[order, MODEL_COLUMNS.index(c)] for c in cols}, index=[names[i] for i in order])
    jmm.attrs["groups"] = [levels[codes[i]] for i in order]
    if not return_details:
        return jmm
    det["inputs"] = _inputs_dict(ls, pairs, fpm, fp, nabove, thr)
    return jmm, det
