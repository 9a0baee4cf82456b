"""``scde.error.models`` (R/functions.R:177-200, 2953-3132, 3141-3178, 3215-3409) on the GPU: the
error models the differential-expression path starts from, fitted from a count matrix.

  * ``crossfit_pairs``      the cell pairs calculate.crossfit.models compares, group by group (host)
  * ``error_model_inputs``  everything computed before a cell's mixture fit (csrc/error_models.hip)
  * ``nb2_fit_models``      fit.nb2.mixture.model of every cell (csrc/nb2_fit.hip), ``linear_fit=False``
  * ``scde_error_models``   the whole function: R's joint model matrix
  * ``crossfit_models``     the three-component mixture of every cell pair (csrc/crossfit_fit.hip):
                            threshold.segmentation = FALSE, reached through ``crossfit="mixture"``
  * ``scde_fit_models_to_reference``  scde.fit.models.to.reference, on ``nb2_fit_models``' kernel

By default a pair's cross-fit is the threshold rule (``threshold.segmentation = TRUE``, R's default
in scde.error.models), and with ``min_count_threshold >= 1`` R's per-pair lists reduce to closed
forms; ``crossfit="mixture"`` fits the original publication's mixture per
pair instead and reduces its clusters and posteriors on the device (section 4.19; nothing of it
can be compared with a run of R).  With ``linear_fit=True`` the fit is ``knn_fit_models``'
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
def _check_ls(ls, C):
    ls = np.ascontiguousarray(ls, np.float64)
    if ls.shape != (C,) or not np.all(np.isfinite(ls)) or np.any(ls <= 0):
        raise ValueError("library sizes must hold one positive finite value per cell")
    return ls


def _stage_args(counts, groups, min_nonfailed, min_count_threshold, min_size_entries, max_pairs, min_pairs_per_cell,
                seed, pairs, library_sizes, want_ls=True):
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
    if library_sizes is None and not want_ls:  # (the mixture cross-fit's vil decides the genes: _mixture_inputs)
        return dc, mat, N, C, codes, levels, pairs, None, thr, int(min_nonfailed)
    if library_sizes is None:
        if host is None:
            host = knn._host_counts(knn._fetch_counts(dc))
        ls = knn.estimate_library_sizes(host, min_size_entries, thr)
    else:
        ls = library_sizes
    return dc, mat, N, C, codes, levels, pairs, _check_ls(ls, C), thr, int(min_nonfailed)


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


# ------------------------------------------------------------------ the mixture cross-fit of pairs
CROSSFIT_STATUS = {0: "ok", 1: "no gene has a count in either cell", 2: "no gene has weight in the correlated component",
                   3: "a parameter or the likelihood is not finite (a separable concomitant included)",
                   5: "an IRLS system is singular or not finite", 6: "a component's share fell below min_prior"}
CROSSFIT_PARAMS = ["conc.a2", "conc.b2", "conc.a3", "conc.b3", "a.c0", "a.c1", "a.theta", "b.c0", "b.c1", "b.theta"]


def _crossfit_fit(dc, mat, N, C, pairs, thr, min_prior, zero_lambda, iter, lds_rows, h, fetch=True):
    """One call of scde_crossfit_fit_*; with ``fetch`` False clusters and posteriors only stay resident."""
    P = pairs.shape[1]
    status = np.zeros(P, np.int32)
    its = np.zeros(P, np.int32)
    llh = np.zeros(P)
    params = np.zeros((P, 10), order="F")
    cl = np.zeros((P, N), np.int8) if fetch else None
    post = np.zeros((P, 2, N)) if fetch else None
    min_prior, zero_lambda = float(min_prior), float(zero_lambda)
    if not 0 <= min_prior < 1:
        raise ValueError("min_prior must lie in [0, 1)")
    if not (zero_lambda > 0 and np.isfinite(zero_lambda)):
        raise ValueError("zero_lambda must be a positive finite number")
    if int(iter) < 1:
        raise ValueError("iter must be at least 1")
    args = (N, N, C, api._p(pairs), P, thr, min_prior, zero_lambda, int(iter), int(lds_rows), api._p(status),
            api._p(its), api._p(llh), api._p(params), api._p(cl), api._p(post))
    if dc is not None:
        check(lib().scde_crossfit_fit_dev(h, dc.ptr, *args))
    else:
        check(lib().scde_crossfit_fit_host(h, api._p(mat), *args))
    out = {"pairs": pairs, "status": status, "iterations": its, "llh": llh, "params": params,
           "min_count_threshold": thr}
    if fetch:
        out["clusters"] = cl.T
        out["posterior"] = post.transpose(1, 2, 0)
    return out


def crossfit_models(counts, groups=None, pairs=None, min_count_threshold=4, min_prior=1e-5, zero_lambda=0.1, iter=200,
                    max_pairs=5000, min_pairs_per_cell=10, seed=None, lds_rows=0, ctx: api.Context | None = None):
    """``calculate.crossfit.models`` with ``threshold.segmentation = FALSE``: the three-component
    mixture of the original publication fitted to every pair of cells of a group, all pairs in one
    launch (csrc/crossfit_fit.hip; contract in include/scde_hip.h and DESIGN.md section 4.19).
    Component 1: the pair's first cell failed; 2: both amplified; 3: the second cell failed.

    Returns R's ``cfm`` as arrays: ``pairs`` (2 x P), ``status`` (P; ``CROSSFIT_STATUS``),
    ``iterations``, ``llh``, ``params`` (P x 10, ``CROSSFIT_PARAMS``), ``clusters`` (genes x P int8:
    1 / 2 / 3, 0 outside the pair's rows or in a failed pair) and ``posterior`` (2 x genes x P: of
    components 1 and 3; NaN where ``clusters`` is 0).  ``nrep > 1``, ``old_cfm`` and the plots are
    not built; no result of it can be compared with a run of R here."""
    thr = knn._thr(min_count_threshold)
    if thr < 0:
        raise ValueError("min_count_threshold must not be negative")
    dc, mat, N, C = knn._counts_arg(counts)
    codes, _ = _codes(groups, C)
    if pairs is None:
        if np.min(np.bincount(codes)) < 2:
            raise ValueError("every group needs at least two cells")
        pairs = crossfit_pairs(codes, max_pairs=max_pairs, min_pairs_per_cell=min_pairs_per_cell, seed=seed)
    pairs = _check_pairs(pairs, codes)
    return _crossfit_fit(dc, mat, N, C, pairs, thr, min_prior, zero_lambda, iter, lds_rows, knn._handle(dc, ctx))


def _check_crossfit(cf, N, codes):
    """A ``crossfit_models`` dict as the C entry takes it: pairs, status, clusters (P x N), posterior (P x 2 x N)."""
    try:
        pairs = _check_pairs(cf["pairs"], codes)
        P = pairs.shape[1]
        status = np.ascontiguousarray(cf["status"], np.int32)
        cl, post = np.asarray(cf["clusters"]), np.asarray(cf["posterior"])
    except (KeyError, TypeError):
        raise ValueError('crossfit must be None, "mixture" or a dict as crossfit_models returns it') from None
    if status.shape != (P,) or cl.shape != (N, P) or post.shape != (2, N, P):
        raise ValueError("crossfit does not belong to these counts: clusters must be genes x pairs, posterior "
                         "2 x genes x pairs and status one value per pair")
    if cl.size and (cl.min() < 0 or cl.max() > 3):
        raise ValueError("crossfit clusters must hold the codes 0 to 3")
    return (pairs, status, np.ascontiguousarray(cl.T, np.int8),
            np.ascontiguousarray(np.transpose(post, (2, 0, 1)), np.float64))


def _warn_failed_pairs(pairs, status, names, C):
    """R drops a pair whose fit failed; a cell left without a pair is an error."""
    for p in np.flatnonzero(status != 0):
        warnings.warn(f"the cross-fit of cells {names[pairs[0, p]]} and {names[pairs[1, p]]} failed "
                      f"({CROSSFIT_STATUS.get(int(status[p]), 'status %d' % status[p])}) - skipping the pair")
    ok = status == 0
    has = np.bincount(np.concatenate([pairs[0], pairs[1]]), minlength=C) > 0
    good = np.bincount(np.concatenate([pairs[0, ok], pairs[1, ok]]), minlength=C) > 0
    for c in np.flatnonzero(has & ~good):
        raise ValueError(f"every cross-fit pair of cell {names[c]} failed: no error model can be built for it")


def _reduce(dc, mat, N, C, codes, given, pairs, ls, mnf, h, fetch=True, want_vil=True):
    """One call of scde_crossfit_reduce_*; ``given`` None: the resident pair results.  ``ls`` None: vil alone."""
    full = ls is not None
    vil = np.zeros((N, C), np.uint8, order="F") if want_vil else None
    fpm = np.zeros((N, C), order="F") if fetch and full else None
    fp = np.zeros((N, C), order="F") if fetch and full else None
    nabove = np.zeros((N, C), np.int32, order="F") if fetch and full else None
    status, cl, post = given if given is not None else (None, None, None)
    args = (N, N, C, api._p(codes), api._p(ls), api._p(pairs), pairs.shape[1], api._p(status), api._p(cl),
            api._p(post), mnf, api._p(vil), api._p(fpm), api._p(fp), api._p(nabove))
    if dc is not None:
        check(lib().scde_crossfit_reduce_dev(h, dc.ptr, *args))
    else:
        check(lib().scde_crossfit_reduce_host(h, api._p(mat), *args))
    return vil, fpm, fp, nabove


def _mixture_inputs(dc, N, C, codes, pairs, ls, thr, mnf, crossfit, names, min_size_entries, min_prior, zero_lambda,
                    crossfit_iter, fetch, fetch_pairs):
    """The input stage from the mixture cross-fit, on resident counts: the pair fit (or the
    caller's), R's library sizes from its vil on the host, the reduction.  fpm and fail_prior stay
    resident for the per-cell fit.  Returns (ls, pairs, vil, fpm, fp, nabove, the pair results)."""
    h = dc.ctx.handle
    if isinstance(crossfit, str):
        cf = _crossfit_fit(dc, None, N, C, pairs, thr, min_prior, zero_lambda, crossfit_iter, 0, h, fetch=fetch_pairs)
        given = None
        _warn_failed_pairs(pairs, cf["status"], names, C)
    else:
        cf, given = crossfit  # (_crossfit_given's)
    vil = None
    if ls is None:
        vil = _reduce(dc, None, N, C, codes, given, pairs, None, mnf, h)[0]
        given = None  # (the call left them resident)
        ls = _check_ls(knn.estimate_library_sizes(knn._host_counts(knn._fetch_counts(dc)), min_size_entries, thr,
                                                  vil=vil), C)
    v2, fpm, fp, nabove = _reduce(dc, None, N, C, codes, given, pairs, ls, mnf, h, fetch=fetch,
                                  want_vil=fetch and vil is None)
    return ls, pairs, vil if vil is not None else v2, fpm, fp, nabove, cf


def _crossfit_arg(crossfit):
    if crossfit is None or isinstance(crossfit, dict):
        return crossfit
    if isinstance(crossfit, str) and crossfit == "mixture":
        return crossfit
    raise ValueError('crossfit must be None (the threshold rule), "mixture" or a dict as crossfit_models returns it')


def _crossfit_given(crossfit, pairs, N, codes, names, min_prior, zero_lambda, crossfit_iter):
    """The checks that need no device: "mixture" with its parameters, or (the dict, its arrays as
    the C entry takes them)."""
    if isinstance(crossfit, str):
        if not 0 <= float(min_prior) < 1:
            raise ValueError("min_prior must lie in [0, 1)")
        if not (float(zero_lambda) > 0 and np.isfinite(zero_lambda)):
            raise ValueError("zero_lambda must be a positive finite number")
        if int(crossfit_iter) < 1:
            raise ValueError("crossfit_iter must be at least 1")
        return crossfit
    own, status, cl, post = _check_crossfit(crossfit, N, codes)
    if not np.array_equal(own, pairs):
        raise ValueError("pairs= differs from the pairs of the crossfit dict: leave it out")
    _warn_failed_pairs(pairs, status, names, len(codes))
    return crossfit, (status, cl, post)


def error_model_inputs(counts, groups=None, min_nonfailed=3, min_count_threshold=4, min_size_entries=2000,
                       max_pairs=5000, min_pairs_per_cell=10, seed=None, pairs=None, library_sizes=None,
                       ctx: api.Context | None = None, crossfit=None, min_prior=1e-5, zero_lambda=0.1,
                       crossfit_iter=200):
    """Everything ``scde.error.models`` computes before it fits a cell's mixture model, in
    ``knn_model_inputs``' shape (``knn_fit_models`` and ``nb2_fit_models`` take the dict as it
    stands).  Only the counts go to the device.

    Returns a dict: ``ls`` (cells: ``estimate_library_sizes(counts, min_size_entries,
    min_count_threshold)``), ``pairs`` (2 x P, ``crossfit_pairs``' or the caller's), ``nabove``
    (genes x cells: the group's other paired cells with ``count >= threshold``), ``vi`` (genes x
    cells bool: ``nabove >= min(group size - 1, min_nonfailed)``), ``fpm`` (genes x cells: the mean
    over the group's other cells of ``count / ls``) and ``fail_prior`` (genes x cells: the
    geometric mean over the cell's pairs of the pair's failure posterior), both NaN outside
    ``vi``.

    ``crossfit`` chooses the cross-fit of the pairs: None is the threshold rule above
    (``threshold.segmentation = TRUE``); ``"mixture"`` fits ``crossfit_models``' three-component
    mixture to every pair on the device (``min_prior``, ``zero_lambda``, ``crossfit_iter``) and a dict
    as ``crossfit_models`` returns it is reduced as given (its ``pairs`` are the pairs).  Then
    ``nabove`` counts the cells whose ``vil`` holds (no status-0 pair of the
    cell puts the gene in the cell's failure component or outside its rows), ``fail_prior`` is the
    geometric mean of the pairs' fitted failure posteriors, ``ls`` is taken over the genes ``vil``
    selects, and the dict also holds ``vil`` (genes x cells uint8) and the pair results under
    ``"crossfit"``.  A failed pair gives a warning and is dropped; a cell whose pairs all failed is
    an error."""
    crossfit = _crossfit_arg(crossfit)
    dc, mat, N, C, codes, _, pairs, ls, thr, mnf = _stage_args(
        counts, groups, min_nonfailed, min_count_threshold, min_size_entries, max_pairs, min_pairs_per_cell, seed,
        crossfit["pairs"] if isinstance(crossfit, dict) and pairs is None and "pairs" in crossfit else pairs,
        library_sizes, want_ls=crossfit is None)
    if crossfit is None:
        fpm, fp, nabove = _crossfit(dc, mat, N, C, codes, pairs, ls, thr, mnf, knn._handle(dc, ctx))
        return _inputs_dict(ls, pairs, fpm, fp, nabove, thr)
    knn._handle(dc, ctx)
    crossfit = _crossfit_given(crossfit, pairs, N, codes, [str(i) for i in range(C)], min_prior, zero_lambda,
                               crossfit_iter)
    own = None
    if dc is None:
        own = dc = api.DeviceCounts(ctx or api.default_context(), mat)
    try:
        ls, pairs, vil, fpm, fp, nabove, cf = _mixture_inputs(
            dc, N, C, codes, pairs, ls, thr, mnf, crossfit, [str(i) for i in range(C)], min_size_entries, min_prior,
            zero_lambda, crossfit_iter, True, False)
    finally:
        if own is not None:
            own.free()
    out = _inputs_dict(ls, pairs, fpm, fp, nabove, thr)
    out["vil"], out["crossfit"] = vil, cf
    return out


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
                      pairs=None, return_details=False, ctx: api.Context | None = None, crossfit=None, min_prior=1e-5,
                      zero_lambda=0.1, crossfit_iter=200, **unsupported):
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
    (NotImplementedError): ``threshold_segmentation=False`` as an argument, ``old_cfm``, plots, NA
    groups, ``min_count_threshold < 1``.  With ``return_details``: ``(jmm, details)``, the fit's
    details and the model inputs under ``"inputs"``.

    ``crossfit="mixture"`` is R's ``threshold.segmentation = FALSE``: every pair's three-component
    mixture (``crossfit_models``; ``min_prior``, ``zero_lambda``, ``crossfit_iter``) in the place of
    the threshold rule, everything from the pair fit to the cells' fit staying on the device; a
    dict from ``crossfit_models`` is reduced as given (``error_model_inputs``).  The details then
    hold the pair results under ``"crossfit"``."""
    import pandas as pd

    from .models import MODEL_COLUMNS
    if not threshold_segmentation:
        raise NotImplementedError('threshold_segmentation = False is not an argument here: crossfit = "mixture" '
                                  "fits the three-component mixture per pair")
    crossfit = _crossfit_arg(crossfit)
    for name in ("old_cfm", "save_crossfit_plots", "save_model_plots"):
        if unsupported.pop(name, None):
            raise NotImplementedError(f"{name} is not built")
    if unsupported:
        raise TypeError(f"unexpected arguments: {sorted(unsupported)}")
    local = bool(linear_fit) if local_theta_fit is None else bool(local_theta_fit)
    cells = None if isinstance(counts, api.DeviceCounts) else api._counts_matrix(counts)[2]
    dc, mat, N, C, codes, levels, pairs, ls, thr, mnf = _stage_args(
        counts, groups, min_nonfailed, min_count_threshold, min_size_entries, max_pairs, min_pairs_per_cell, seed,
        crossfit["pairs"] if isinstance(crossfit, dict) and pairs is None and "pairs" in crossfit else pairs,
        None, want_ls=crossfit is None)
    knn._handle(dc, ctx)
    names = cells if cells is not None else [str(i) for i in range(C)]
    if crossfit is not None:
        crossfit = _crossfit_given(crossfit, pairs, N, codes, names, min_prior, zero_lambda, crossfit_iter)
    own = None
    if dc is None:
        own = dc = api.DeviceCounts(ctx or api.default_context(), mat)
    vil = cf = None
    try:
        if crossfit is None:
            fpm, fp, nabove = _crossfit(dc, None, N, C, codes, pairs, ls, thr, mnf, dc.ctx.handle,
                                        fetch=return_details)
        else:
            ls, pairs, vil, fpm, fp, nabove, cf = _mixture_inputs(
                dc, N, C, codes, pairs, ls, thr, mnf, crossfit, names, min_size_entries, min_prior, zero_lambda,
                crossfit_iter, return_details, return_details)
        if linear_fit:
            lo, hi = (float(v) for v in theta_fit_range)
            mm, det = knn._fit_call("knn", None, dc, (int(local), lo, hi, 0.5), iter, True, 0, None)
        else:
            mm, det = knn._fit_call("nb2", None, dc, (0.1,), iter, True, 0, None)
    finally:
        if own is not None:
            own.free()
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
    if crossfit is not None:
        det["inputs"]["vil"] = vil
        det["crossfit"] = cf
    return jmm, det


# ================================================================== fits against a reference
def reference_fit_inputs(counts, reference, zero_count_threshold=1, min_fpm=1):
    """The inputs ``scde.fit.models.to.reference`` gives every cell's fit (R/functions.R:990-992 and
    fit.nb2.mixture.model's default prior): ``fpm = reference / sum(reference) * 1e6`` for every
    cell, the genes with ``fpm > min_fpm``, and a starting failure posterior of 1 where the count
    is at most ``zero_count_threshold`` and 0 elsewhere; as a dict ``nb2_fit_models`` takes."""
    mat = knn._host_counts(counts)
    N, C = mat.shape
    ref = np.asarray(reference, np.float64)
    if ref.shape != (N,) or not np.all(np.isfinite(ref)) or np.any(ref < 0) or not ref.sum() > 0:
        raise ValueError("reference must hold one non-negative finite value per gene, not all zero")
    f = ref / ref.sum() * 1e6
    use = f > min_fpm
    fpm = np.asfortranarray(np.repeat(f[:, None], C, axis=1))
    fp = np.where(mat <= zero_count_threshold, 1.0, 0.0)
    fpm[~use] = np.nan
    fp[~use] = np.nan
    return {"fpm": fpm, "fail_prior": np.asfortranarray(fp), "vi": np.repeat(use[:, None], C, axis=1)}


def scde_fit_models_to_reference(counts, reference, zero_count_threshold=1, min_fpm=1, iter=50,
                                 ctx: api.Context | None = None):
    """``scde.fit.models.to.reference``: every cell's ``fit.nb2.mixture.model`` against one
    reference magnitude per gene (a bulk measurement, say) in the place of the other cells'
    (``nb2_fit_models``' kernel on ``reference_fit_inputs``).  Returns R's ``jmm``: a DataFrame of
    ``conc.b, conc.a, fail.r, corr.b, corr.a, corr.theta``, rows in the cells' order.  A cell whose
    fit fails is an error, as in R.  The plots are not built."""
    import pandas as pd

    from .models import MODEL_COLUMNS
    mat, _, cells = api._counts_matrix(counts)
    inputs = reference_fit_inputs(mat, reference, zero_count_threshold, min_fpm)
    mm, det = nb2_fit_models(inputs, knn._host_counts(mat), iter=iter, return_details=True, ctx=ctx)
    names = list(cells) if cells is not None else [str(i) for i in range(mm.shape[0])]
    for i in np.flatnonzero(det["status"] != 0):
        raise RuntimeError(f"ERROR encountered in building a model for cell {names[i]}: "
                           f"{NB2_FIT_STATUS.get(int(det['status'][i]), 'status %d' % det['status'][i])}")
    return pd.DataFrame({c: mm[:, j] for j, c in enumerate(MODEL_COLUMNS[:6])}, index=names)
