"""``knn.error.models`` (R/functions.R:1158-1299) on the GPU: the neighbourhood stage
(csrc/knn.hip), everything PAGODA's error-model fitter computes before its per-cell mixture fit,
and the fit itself (csrc/knn_fit.hip).

  * ``estimate_library_sizes``    estimate.library.sizes with ``vil = counts >= thr`` (host)
  * ``tmm_norm_factors``          edgeR's calcNormFactors(method = "TMM"), restated (host)
  * ``knn_cell_similarity``       pairwise-complete Pearson correlation of sqrt(counts)
  * ``knn_neighbours``            the k most similar cells of every cell, in R's order
  * ``knn_expected_magnitudes``   trimmed mean of the neighbours' library-scaled counts (fpm)
  * ``knn_model_inputs``          the chain, with the counts resident throughout
  * ``knn_cell_data``             one cell's ``data.frame(count, fpm)`` and ``cp``
  * ``knn_fit_models``            fit.nb2gth.mixture.model + get.compressed.v1.model of every cell
  * ``knn_error_models``          the whole function: R's joint model matrix ``jmm``

The fit is the project's statement of flexmix's EM, compared with R's
stored result on the pollen data (tests/test_gpu_knn_fit.py).  ``linear_fit=False``
(fit.nb2.mixture.model with ``prior = cp``) is ``error_models.nb2_fit_models`` on
``knn_model_inputs``' result (csrc/nb2_fit.hip); ``knn_fit_models`` and
``knn_error_models`` themselves still refuse it.  ``counts`` is an integer genes x cells matrix or
a resident ``DeviceCounts``; ``thr`` is min.count.threshold and an entry is valid when
``counts >= thr``.
The TMM factors are written from Robinson & Oshlack (2010) with edgeR's documented defaults and
were not checked against edgeR; ``norm_factors=`` / ``library_sizes=`` take a caller's values.
"""
from __future__ import annotations

import math
import warnings

import numpy as np

from . import api
from ._lib import check, lib

MAX_CELLS = 8192  # csrc/kernels.h kKnnMaxCells
THRESHOLD_PRIOR = 1 - 1e-6


# ================================================================== library sizes (host)
def _quantile7(x, p):
    x = np.sort(x)
    h = (len(x) - 1) * p
    lo = int(math.floor(h))
    hi = min(lo + 1, len(x) - 1)
    return x[lo] + (h - lo) * (x[hi] - x[lo])


def _average_rank(v):
    """R's rank(ties.method = "average")."""
    order = np.argsort(v, kind="stable")
    s = v[order]
    start = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])
    end = np.r_[start[1:], len(v)]
    r = np.empty(len(v))
    r[order] = np.repeat((start + end - 1) / 2.0 + 1.0, end - start)
    return r


def _tmm_factor(obs, ref, n_o, n_r):
    with np.errstate(divide="ignore", invalid="ignore"):
        log_r = np.log2((obs / n_o) / (ref / n_r))
        abs_e = (np.log2(obs / n_o) + np.log2(ref / n_r)) / 2
        v = (n_o - obs) / n_o / obs + (n_r - ref) / n_r / ref
    fin = np.isfinite(log_r) & np.isfinite(abs_e) & (abs_e > -1e10)
    log_r, abs_e, v = log_r[fin], abs_e[fin], v[fin]
    if len(log_r) == 0 or np.max(np.abs(log_r)) < 1e-6:
        return 1.0
    n = len(log_r)
    lo_l = math.floor(n * 0.3) + 1
    hi_l = n + 1 - lo_l
    lo_s = math.floor(n * 0.05) + 1
    hi_s = n + 1 - lo_s
    rl, rs = _average_rank(log_r), _average_rank(abs_e)
    keep = (rl >= lo_l) & (rl <= hi_l) & (rs >= lo_s) & (rs <= hi_s)
    with np.errstate(divide="ignore", invalid="ignore"):
        f = 2.0 ** (np.sum(log_r[keep] / v[keep]) / np.sum(1 / v[keep]))
    return 1.0 if np.isnan(f) else float(f)


def tmm_norm_factors(x):
    """TMM normalisation factors of the columns of ``x`` (rows x columns), scaled to a geometric
    mean of 1: weighted trimmed mean of M values against a reference column (the one whose upper
    quartile is closest to the mean upper quartile), trimming 30 % of M and 5 % of A."""
    x = np.asarray(x, np.float64)
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError("x must be a matrix with at least one column")
    if not np.all(np.isfinite(x)) or np.any(x < 0):
        raise ValueError("x must hold non-negative finite counts")
    x = x[np.any(x != 0, axis=1)]
    C = x.shape[1]
    if x.shape[0] == 0 or C == 1:
        return np.ones(C)
    f = _tmm_raw_factors(x)
    return f / np.exp(np.mean(np.log(f)))


def _tmm_reference_column(x, libsize):
    f75 = np.array([_quantile7(x[:, j], 0.75) for j in range(x.shape[1])]) / libsize
    if np.median(f75) < 1e-20:
        return int(np.argmax(np.sum(np.sqrt(x), axis=0)))
    return int(np.argmin(np.abs(f75 - np.mean(f75))))


def _tmm_raw_factors(x):
    """Every column's factor against the reference column, before the geometric-mean scaling
    (x without all-zero rows)."""
    libsize = x.sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        ref = _tmm_reference_column(x, libsize)
        return np.array([_tmm_factor(x[:, j], x[:, ref], libsize[j], libsize[ref]) for j in range(x.shape[1])])


def _host_counts(counts):
    mat = api._counts_matrix(counts)[0]
    if mat.ndim != 2:
        raise ValueError("counts must be a genes x cells matrix")
    if not np.issubdtype(mat.dtype, np.integer):
        if not np.all(np.isfinite(mat)) or np.any(mat != np.round(mat)):
            raise ValueError("counts must be integers")
    if mat.size and mat.min() < 0:
        raise ValueError("counts must not be negative")
    return np.asfortranarray(mat, dtype=np.int32)


def _thr(thr):
    if int(thr) != thr:
        raise ValueError("min_count_threshold must be an integer")
    return int(thr)


def _vil_arg(vil, shape):
    vil = np.asarray(vil)
    if vil.shape != shape:
        raise ValueError("vil must be a genes x cells matrix, as the counts")
    return vil != 0


def library_size_genes(counts, min_size_entries=2000, thr=1, vil=None):
    """The genes (0-based, in R's order) estimate.library.sizes takes.  ``vil`` (genes x cells,
    non-zero: the observation is not a likely drop-out) replaces ``counts >= thr``."""
    counts = _host_counts(counts)
    N, C = counts.shape
    mse = int(min_size_entries)
    if mse < 1:
        raise ValueError("min_size_entries must be at least 1")
    if N < mse:
        raise ValueError(f"The number of valid genes ({N}) is lower then the specified min.size.entries ({mse}). "
                         "Please either increase min.size.entries or lower min.nonfailed parameter to increase the "
                         "number of valid genes")
    nv = ((counts >= _thr(thr)) if vil is None else _vil_arg(vil, counts.shape)).sum(axis=1)
    order = np.argsort(-nv, kind="stable")
    if nv[order[mse - 1]] < C:
        return order[:mse]
    return order[nv[order] == C]


def estimate_library_sizes(counts, min_size_entries=2000, thr=1, norm_factors=None, vil=None):
    """``estimate.library.sizes(counts, vil = counts >= thr)``: library sizes in millions of reads
    over the genes detected in the most cells, times the TMM factors (or ``norm_factors``), each
    scaled to a geometric mean of 1.  ``vil``: the caller's matrix in the place of ``counts >= thr``
    (the one the cross-fit gives: ``error_model_inputs(crossfit=)``)."""
    counts = _host_counts(counts)
    sub = counts[library_size_genes(counts, min_size_entries, thr, vil)].astype(np.float64)
    if norm_factors is None:
        f = tmm_norm_factors(sub)
    else:
        f = np.asarray(norm_factors, np.float64)
        if f.shape != (counts.shape[1],) or not np.all(np.isfinite(f)) or np.any(f <= 0):
            raise ValueError("norm_factors must hold one positive finite factor per cell")
    f = f / np.exp(np.mean(np.log(f)))
    return sub.sum(axis=0) * f / 1e6


# ================================================================== device stages
def _counts_arg(counts):
    """(DeviceCounts or None, host matrix or None, N, C)."""
    if isinstance(counts, api.DeviceCounts):
        dc, mat, N, C = counts, None, counts.ngenes, counts.ncells
    else:
        mat = _host_counts(counts)
        dc, (N, C) = None, mat.shape
    if C < 1:
        raise ValueError("at least one cell is needed")
    if C > MAX_CELLS:
        raise ValueError(f"{C} cells: at most {MAX_CELLS} are supported")
    return dc, mat, N, C


def _handle(dc, ctx):
    """The context handle of a call: ``ctx``'s, which must be the resident counts' own."""
    if dc is not None and ctx is not None and ctx is not dc.ctx:
        raise ValueError("ctx is not the context the resident counts live in")
    if dc is not None:
        return dc.ctx.handle
    return ctx.handle if ctx else None


def knn_cell_similarity(counts, thr=1, cor_method="pearson", ctx: api.Context | None = None):
    """The cells x cells pairwise-complete Pearson correlation of sqrt(counts) over the entries
    with ``counts >= thr`` (``weighted_correlation`` with 0 / 1 weights, its inputs formed on the
    device).  NaN where a pair has no common valid gene or a zero variance.  Counts must not be
    negative: host matrices are checked, resident counts are the caller's word (a negative valid
    count, possible with ``thr <= 0``, is sqrt's NaN in every pair of its cell, as in R)."""
    if cor_method != "pearson":
        raise NotImplementedError("only cor_method = 'pearson' is built here: the Spearman similarity is "
                                  "spearman.spearman_cell_similarity")
    thr = _thr(thr)
    dc, mat, N, C = _counts_arg(counts)
    out = np.zeros((C, C), order="F")
    h = _handle(dc, ctx)
    if dc is not None:
        check(lib().scde_knn_similarity_dev(h, dc.ptr, N, N, C, thr, api._p(out)))
    else:
        check(lib().scde_knn_similarity_host(h, api._p(mat), N, N, C, thr, api._p(out)))
    return out


def default_k(ncells):
    """R's ``round(ncol(counts) / 2)`` (half to even)."""
    return int(np.round(ncells / 2))


def _group_codes(groups, C):
    if groups is None:
        return None
    g = np.asarray(groups)
    if g.shape != (C,):
        raise ValueError("groups must have one entry per cell")
    return np.ascontiguousarray(np.unique(g, return_inverse=True)[1].reshape(C), np.int32)


def _neighbours(sim, C, k, codes, h):
    if k is None:
        k = default_k(C)  # (0 for one cell: no neighbours, as R's round(1 / 2))
    elif int(k) < 1:
        raise ValueError("k must be at least 1")
    k = min(int(k), C - 1)  # R: "the value of k is too large, setting to ncol(counts) - 1"
    largest = C if codes is None else int(np.max(np.bincount(codes)))
    kmax = max(min(k, largest - 1), 0)
    out = np.full((C, kmax), -1, np.int32)
    check(lib().scde_knn_neighbours(h, api._p(sim), C, api._p(codes), k, kmax, api._p(out)))
    return out


def knn_neighbours(similarity, k=None, groups=None, ctx: api.Context | None = None):
    """The ``k`` most similar cells of every cell: cells x kmax int32, 0-based, padded with -1,
    kmax = min(k, largest group - 1).  Candidates are the other cells of the cell's group, in R's
    ``order(decreasing = TRUE)``: decreasing similarity, ties by index, NaN last.  ``k`` defaults
    to ``round(cells / 2)`` and is lowered to cells - 1."""
    sim = np.asfortranarray(similarity, dtype=np.float64)
    if sim.ndim != 2 or sim.shape[0] != sim.shape[1] or sim.shape[0] < 1:
        raise ValueError("similarity must be a square matrix")
    C = sim.shape[0]
    if C > MAX_CELLS:
        raise ValueError(f"{C} cells: at most {MAX_CELLS} are supported")
    return _neighbours(sim, C, k, _group_codes(groups, C), ctx.handle if ctx else None)


def _check_ls_trim(ls, C, thr, trim):
    ls = np.ascontiguousarray(ls, dtype=np.float64)
    if ls.shape != (C,):
        raise ValueError("ls must hold one library size per cell")
    if not np.all(np.isfinite(ls)) or np.any(ls < 0) or (thr <= 0 and np.any(ls == 0)):
        raise ValueError("library sizes must be finite and not negative (positive when thr <= 0)")
    trim = float(trim)
    if not trim >= 0:
        raise ValueError("trim must be at least 0")
    return ls, trim


def _magnitudes(dc, mat, N, C, nb, kmax, ls, thr, trim, h):
    fpm = np.zeros((N, C), order="F")
    nabove = np.zeros((N, C), np.int32, order="F")
    if dc is not None:
        check(lib().scde_knn_magnitudes_dev(h, dc.ptr, N, N, C, api._p(nb), kmax, api._p(ls), thr,
                                            trim, api._p(fpm), api._p(nabove)))
    else:
        check(lib().scde_knn_magnitudes_host(h, api._p(mat), N, N, C, api._p(nb), kmax, api._p(ls), thr, trim,
                                             api._p(fpm), api._p(nabove)))
    return fpm, nabove


def knn_expected_magnitudes(counts, neighbours, ls, thr=1, trim=0.25, ctx: api.Context | None = None):
    """``(fpm, nabove)``, both genes x cells.  ``fpm[g, i]`` is R's ``mean(trim =, na.rm = TRUE)``
    of ``counts[g, j] / ls[j]`` over cell i's neighbours j with ``counts[g, j] >= thr`` (NaN when
    there is none; the median for ``trim >= 0.5``); ``nabove[g, i]`` counts the neighbours with
    ``counts[g, j] > thr``."""
    thr = _thr(thr)
    dc, mat, N, C = _counts_arg(counts)
    nb = np.ascontiguousarray(neighbours, dtype=np.int32)
    if nb.ndim != 2 or nb.shape[0] != C:
        raise ValueError("neighbours must have one row per cell")
    ls, trim = _check_ls_trim(ls, C, thr, trim)
    return _magnitudes(dc, mat, N, C, nb, nb.shape[1], ls, thr, trim, _handle(dc, ctx))


# ================================================================== the chain
def _r_median(v):
    n = len(v)
    if n == 0:
        return np.nan
    h = (n + 1) // 2
    if n % 2:
        return np.partition(v, h - 1)[h - 1]
    v = np.partition(v, [h - 1, h])
    return (v[h - 1] + v[h]) / 2


def fail_priors(counts, fpm, vi, thr=1):
    """The failed-component starting posterior of every valid (gene, cell), NaN elsewhere
    (R/functions.R:1232): threshold.prior where the count is at most ``thr`` and fpm is at least
    the median fpm of the cell's such genes, 1 - threshold.prior elsewhere."""
    counts = np.asarray(counts)
    tp = THRESHOLD_PRIOR
    out = np.full(fpm.shape, np.nan, order="F")
    for i in range(fpm.shape[1]):
        g = np.flatnonzero(vi[:, i])
        f = fpm[g, i]
        low = counts[g, i] <= thr
        med = _r_median(f[low])
        with np.errstate(invalid="ignore"):
            out[g, i] = np.where(low & (f >= med), tp, 1 - tp)
    return out


def knn_model_inputs(counts, groups=None, k=None, min_nonfailed=5, min_count_threshold=1, min_size_entries=2000,
                     min_fpm=0, fpm_estimate_trim=0.25, library_sizes=None, cor_method="pearson", similarity=None,
                     ctx: api.Context | None = None):
    """Everything ``knn.error.models`` computes before it fits a cell's mixture model.  The counts
    go to the device once; the similarity and the neighbour lists stay there between the stages.

    Returns a dict: ``ls`` (cells), ``similarity`` (cells x cells; NaN between groups),
    ``neighbours`` (cells x kmax, -1 padded), ``fpm`` and ``nabove`` (genes x cells), ``vi``
    (genes x cells bool: ``nabove >= min_nonfailed and fpm > min_fpm``; R's
    ``min(ncol(oc) - 1, min.nonfailed)`` is always min.nonfailed, as ``oc`` is a vector) and
    ``fail_prior`` (genes x cells, NaN outside ``vi``).  A cell with fewer than 40 valid genes
    gives a warning, as R's message.

    ``similarity`` (cells x cells) takes the place of the Pearson similarity: the neighbours are
    found in the caller's matrix, which need not be symmetric, and everything after them is
    unchanged.  ``spearman.spearman_cell_similarity(counts, thr)`` is R's ``cor.method =
    "spearman"``; ``cor_method="spearman"`` itself still raises."""
    if similarity is not None and cor_method != "pearson":
        raise ValueError("similarity= replaces the correlation: cor_method must be left at its default with it")
    if cor_method != "pearson":
        raise NotImplementedError("only cor_method = 'pearson' is built here: pass similarity = "
                                  "spearman.spearman_cell_similarity(counts, thr) for the Spearman neighbours")
    thr = _thr(min_count_threshold)
    dc, mat, N, C = _counts_arg(counts)
    if similarity is not None:
        similarity = np.array(similarity, dtype=np.float64, order="F")
        if similarity.shape != (C, C):
            raise ValueError(f"similarity must be a {C} x {C} matrix (cells x cells)")
    codes = _group_codes(groups, C)
    _handle(dc, ctx)
    host = mat if mat is not None else _host_counts(_fetch_counts(dc))  # (int32: library sizes, priors)
    ls = estimate_library_sizes(host, min_size_entries, thr) if library_sizes is None else library_sizes
    ls, trim = _check_ls_trim(ls, C, thr, fpm_estimate_trim)
    own = None
    if dc is None:
        own = dc = api.DeviceCounts(ctx or api.default_context(), mat)
    h = dc.ctx.handle
    try:
        if similarity is None:
            sim = np.zeros((C, C), order="F")
            check(lib().scde_knn_similarity_dev(h, dc.ptr, N, N, C, thr, api._p(sim)))
        else:
            sim = similarity
        nb = _neighbours(None if similarity is None else sim, C, k, codes, h)
        fpm, nabove = _magnitudes(dc, None, N, C, None, nb.shape[1], ls, thr, trim, h)
    finally:
        if own is not None:
            own.free()
    if codes is not None:
        sim[codes[:, None] != codes[None, :]] = np.nan
    with np.errstate(invalid="ignore"):
        vi = (nabove >= min_nonfailed) & (fpm > min_fpm)
    for i in np.flatnonzero(vi.sum(axis=0) < 40):
        warnings.warn(f"only {int(vi[:, i].sum())} valid genes were found to fit the model of cell {i}")
    return {"ls": ls, "similarity": sim, "neighbours": nb, "fpm": fpm, "nabove": nabove, "vi": vi,
            "fail_prior": fail_priors(host, fpm, vi, thr), "min_count_threshold": thr}


def _fetch_counts(dc):
    out = np.zeros((dc.ngenes, dc.ncells), np.int32, order="F")
    if out.nbytes:
        check(lib().scde_d2h(dc.ctx.handle, api._p(out), dc.ptr, out.nbytes))
    return out


# ================================================================== the mixture fit
FIT_STATUS = {0: "ok", 1: "fewer than 3 valid genes", 2: "no weight on the correlated component",
              3: "a parameter or the likelihood is not finite"}


def _fit_call(kind, inputs, counts, params, iter, return_details, lds_genes, ctx):
    """One call of scde_knn_fit_* (``kind`` "knn") or scde_nb2_fit_* ("nb2") with the fit's own
    ``params``; ``inputs`` None: the inputs scde_crossfit_inputs_* left resident in the context."""
    dc, mat, N, C = _counts_arg(counts)
    fpm = fp = None
    if inputs is not None:
        fpm = np.asfortranarray(inputs["fpm"], dtype=np.float64)
        fp = np.asfortranarray(inputs["fail_prior"], dtype=np.float64)
        if fpm.shape != (N, C) or fp.shape != (N, C):
            raise ValueError("inputs do not belong to these counts")
    models = np.zeros((C, 12), order="F")
    its = np.zeros(C, np.int32)
    status = np.zeros(C, np.int32)
    llh = np.zeros(C)
    cl = np.zeros((N, C), np.int32, order="F") if return_details else None
    post = np.zeros((N, C), order="F") if return_details else None
    h = _handle(dc, ctx)
    args = (N, N, C, api._p(fpm), api._p(fp), *params, int(iter), int(lds_genes), api._p(models), api._p(its),
            api._p(llh), api._p(status), api._p(cl), api._p(post))
    fn = {("knn", True): "scde_knn_fit_dev", ("knn", False): "scde_knn_fit_host", ("nb2", True): "scde_nb2_fit_dev",
          ("nb2", False): "scde_nb2_fit_host"}[kind, dc is not None]
    check(getattr(lib(), fn)(h, dc.ptr if dc is not None else api._p(mat), *args))
    if not return_details:
        return models
    return models, {"iterations": its, "llh": llh, "status": status, "clusters": cl, "posteriors": post}


def knn_fit_models(inputs, counts, local_theta_fit=None, theta_fit_range=(1e-2, 1e2), alpha_weight_power=0.5,
                   iter=50, linear_fit=True, return_details=False, lds_genes=0, ctx: api.Context | None = None):
    """The per-cell EM mixture fit (fit.nb2gth.mixture.model + get.compressed.v1.model; contract in
    include/scde_hip.h and DESIGN.md section 4.15) on what ``knn_model_inputs`` (or
    ``error_models.error_model_inputs``) returned.

    Returns the cells x 12 model matrix in ``models.MODEL_COLUMNS``' order (a failed cell's row is
    NaN; without local theta the ``corr.ltheta.*`` columns are NaN), and with ``return_details`` a
    dict as well: ``iterations``, ``llh``, ``status`` (per cell; ``FIT_STATUS``), ``clusters``
    (genes x cells int32: 1 / 2, R's ``clusters(m1)``, 0 outside the valid genes) and
    ``posteriors`` (genes x cells: the failed component's final posterior, NaN outside).
    ``local_theta_fit`` defaults to True, as in R; ``iter = 1`` is one M-step and one E-step from the
    starting posteriors.  ``lds_genes`` is the C entry's (0: its default).  ``linear_fit=False``
    (fit.nb2.mixture.model) is a function of its own, ``error_models.nb2_fit_models``, which takes
    the same inputs."""
    if not linear_fit:
        raise NotImplementedError("linear_fit = False is error_models.nb2_fit_models (fit.nb2.mixture.model)")
    local = True if local_theta_fit is None else bool(local_theta_fit)
    lo, hi = (float(v) for v in theta_fit_range)
    return _fit_call("knn", inputs, counts, (int(local), lo, hi, float(alpha_weight_power)), iter, return_details,
                     lds_genes, ctx)


def knn_error_models(counts, groups=None, k=None, min_nonfailed=5, min_count_threshold=1, min_size_entries=2000,
                     min_fpm=0, cor_method="pearson", fpm_estimate_trim=0.25, linear_fit=True, local_theta_fit=None,
                     theta_fit_range=(1e-2, 1e2), alpha_weight_power=0.5, iter=50, return_details=False,
                     similarity=None, ctx: api.Context | None = None):
    """``knn.error.models`` (R/functions.R:1158-1299): the neighbourhood stage, then every cell's
    mixture fit, both on the GPU.  Returns R's ``jmm``: a DataFrame of the cells' models, columns in
    ``models.MODEL_COLUMNS``' order (without the ``corr.ltheta.*`` columns when
    ``local_theta_fit=False``), rows named by the cells (the counts' column names, or their
    positions) and ordered by group as R's ``rbind`` over the groups, ``.attrs["groups"]`` the rows'
    groups.  A cell whose fit fails is dropped with a warning, as R drops a ``try-error``.  With
    ``return_details``: ``(jmm, details)``, the details of ``knn_fit_models`` (all cells, in the
    counts' order) and the model inputs under ``"inputs"``.  ``similarity`` is
    ``knn_model_inputs``'."""
    import pandas as pd

    from .models import MODEL_COLUMNS
    if not linear_fit:
        raise NotImplementedError("linear_fit = False is not built here: error_models.nb2_fit_models takes "
                                  "knn_model_inputs' result")
    local = True if local_theta_fit is None else bool(local_theta_fit)
    cells = None if isinstance(counts, api.DeviceCounts) else api._counts_matrix(counts)[2]
    inputs = knn_model_inputs(counts, groups=groups, k=k, min_nonfailed=min_nonfailed,
                              min_count_threshold=min_count_threshold, min_size_entries=min_size_entries,
                              min_fpm=min_fpm, fpm_estimate_trim=fpm_estimate_trim, cor_method=cor_method,
                              similarity=similarity, ctx=ctx)
    dc = counts if isinstance(counts, api.DeviceCounts) else None
    host = counts if dc is not None else _host_counts(counts)
    mm, det = knn_fit_models(inputs, host, local_theta_fit=local, theta_fit_range=theta_fit_range,
                             alpha_weight_power=alpha_weight_power, iter=iter, return_details=True,
                             ctx=None if dc is not None else ctx)
    C = mm.shape[0]
    names = cells if cells is not None else [str(i) for i in range(C)]
    for i in np.flatnonzero(det["status"] != 0):
        warnings.warn(f"ERROR encountered in building a model for cell {names[i]} - skipping the cell. Error: "
                      f"{FIT_STATUS.get(int(det['status'][i]), 'status %d' % det['status'][i])}")
    codes = _group_codes(groups, C)
    order = np.arange(C) if codes is None else np.argsort(codes, kind="stable")
    order = order[det["status"][order] == 0]
    cols = [c for c in MODEL_COLUMNS if local or not c.startswith("corr.ltheta.")]
    jmm = pd.DataFrame({c: mm[order, MODEL_COLUMNS.index(c)] for c in cols}, index=[names[i] for i in order])
    glab = np.asarray(groups)[order] if groups is not None else np.array(["all"] * len(order))
    jmm.attrs["groups"] = [str(g) for g in glab]
    if not return_details:
        return jmm
    det["inputs"] = inputs
    return jmm, det


def knn_cell_data(inputs, counts, i):
    """Cell i's ``df$count``, ``df$fpm`` and the two-column ``cp = cbind(fp, 1 - fp)`` that
    fit.nb2gth.mixture.model takes, with ``genes`` the (0-based) rows of ``vi``."""
    mat = _fetch_counts(counts) if isinstance(counts, api.DeviceCounts) else _host_counts(counts)
    g = np.flatnonzero(inputs["vi"][:, i])
    fp = inputs["fail_prior"][g, i]
    return {"genes": g, "count": mat[g, i], "fpm": inputs["fpm"][g, i], "cp": np.column_stack([fp, 1 - fp])}
