"""Spearman rank correlation on the GPU (csrc/spearman.hip; contract in include/scde_hip.h and
DESIGN.md section 4.18).

  * ``rank_columns``              R's ``rank(ties.method = "average", na.last = "keep")`` of every
                                  column of a matrix
  * ``spearman_cell_similarity``  the pairwise-complete Spearman correlation of cells that
                                  ``knn.error.models(cor.method = "spearman")`` uses
                                  (R/functions.R:1184-1196); hand it to ``knn_model_inputs`` /
                                  ``knn_error_models`` as ``similarity=``

``cluster.pagoda_gene_clusters*(cor_method="spearman")`` rank their matrices with the same kernel.
"""
from __future__ import annotations

import numpy as np

from . import api
from ._lib import check, lib
from .knn import _counts_arg, _handle, _thr

COR_METHODS = ("pearson", "p", "spearman")


def cor_method_is_spearman(cor_method):
    """True for "spearman", False for "pearson" / "p"; anything else is a ValueError."""
    if cor_method not in COR_METHODS:
        raise ValueError(f"cor_method must be one of {', '.join(COR_METHODS)}")
    return cor_method == "spearman"


def rank_columns(x, ctx: api.Context | None = None):
    """Every column of ``x`` (rows x columns, float64) replaced by its average ranks: -0.0 ties
    with 0.0, a NaN stays NaN and the rest of its column is ranked among the non-NaN values,
    +-Inf are ordinary values.  Exact: every rank is a multiple of 0.5."""
    x = np.asfortranarray(x, dtype=np.float64)
    if x.ndim != 2:
        raise ValueError("x must be a matrix")
    out = np.zeros(x.shape, order="F")
    if x.size:
        check(lib().scde_rank_cols_host(ctx.handle if ctx else None, api._p(x), x.shape[0], x.shape[1], api._p(out)))
    return out


def spearman_cell_similarity(counts, thr=1, lds_values=0, ctx: api.Context | None = None):
    """The cells x cells Spearman correlation of the counts, every pair over the genes both cells
    have at ``counts >= thr`` (R's ``cor(sqrt(counts), method = "spearman", use = "p")`` with the
    entries below ``thr`` NA).  Ranks are average ranks within the pair's common genes; all sums
    are exact integers, so the result is the correctly rounded quotient of the contract and the
    same every run.  NaN where a pair has no common gene or one of the two cells is constant over
    them; the diagonal is 1.0 or NaN by the same rule.  ``counts`` is a host matrix or a resident
    ``DeviceCounts``; ``lds_values`` is the C entry's (0: its default)."""
    thr = _thr(thr)
    if int(lds_values) != lds_values or lds_values < 0:
        raise ValueError("lds_values must be a non-negative integer")
    dc, mat, N, C = _counts_arg(counts)
    out = np.zeros((C, C), order="F")
    h = _handle(dc, ctx)
    if dc is not None:
        check(lib().scde_spearman_similarity_dev(h, dc.ptr, N, N, C, thr, int(lds_values), api._p(out)))
    else:
        check(lib().scde_spearman_similarity_host(h, api._p(mat), N, N, C, thr, int(lds_values), api._p(out)))
    return out
