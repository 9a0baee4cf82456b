"""Drop-out-adjusted cell-to-cell distances (the reference vignette's "Adjusted distance
measures", vignettes/diffexp.md:231-301), on the GPU (csrc/dist.hip).

  * ``reciprocal_distance``      reciprocal weighting        vignette 268-278
  * ``mode_relative_distance``   mode-relative weighting     vignette 285-300
  * ``direct_dropout_distance``  simulated direct drop-out   vignette 241-258
  * ``weighted_correlation``     the weighted correlation of the columns of ``x`` with weights
                                 ``u[g, i] * u[g, j]`` (what the last two reduce to)

Each distance is the square ``1 - corr`` matrix over the models' cells (R's ``as.dist`` input),
with a zero diagonal; ``corr`` is ``boot::corr``: with ``s = sum(w)``, ``m1 = sum(x w)/s``,
``m2 = sum(y w)/s``: ``(sum(x y w)/s - m1 m2) / sqrt((sum(x^2 w)/s - m1^2) (sum(y^2 w)/s - m2^2))``.
A pair with zero weight sum or zero weighted variance is NaN.  ``counts`` may be a host matrix
(columns matched to the model rows) or a resident ``DeviceCounts``.
"""
from __future__ import annotations

import numpy as np

from . import api
from ._lib import check, lib
from .models import model_matrix


def _check_k(k):
    k = float(k)
    if not 0.0 <= k <= 1.0:
        raise ValueError("k must be in [0, 1]")
    return k


def _counts_arg(models, counts):
    """(model matrix, square_logit_conc, DeviceCounts or None, aligned host matrix or None, N, C)."""
    mm, _, sq = model_matrix(models)
    if isinstance(counts, api.DeviceCounts):
        dc, mat, N, C = counts, None, counts.ngenes, counts.ncells
    else:
        mat, _ = api._align_counts(models, counts)
        dc, (N, C) = None, mat.shape
    if C != mm.shape[0]:
        raise ValueError("counts and models disagree on the number of cells")
    if C < 1:
        raise ValueError("at least one cell is needed")
    return mm, sq, dc, mat, N, C


def _as_distance(corr):
    d = 1.0 - corr
    np.fill_diagonal(d, 0.0)
    return d


def weighted_correlation(x, u, ctx: api.Context | None = None):
    """Correlation of every pair of columns of ``x`` (rows x columns) with the separable
    weights ``u[g, i] * u[g, j]``; ``u`` of 0 / 1 gives the pairwise-complete Pearson
    correlation.  Returns the columns x columns matrix (NaN where a pair is degenerate)."""
    x = np.asfortranarray(x, dtype=np.float64)
    u = np.asfortranarray(u, dtype=np.float64)
    if x.ndim != 2 or x.shape != u.shape:
        raise ValueError("x and u must be matrices of the same shape")
    N, C = x.shape
    if C < 1:
        raise ValueError("at least one column is needed")
    out = np.zeros((C, C), order="F")
    check(lib().scde_wcorr_sep_host(ctx.handle if ctx else None, api._p(x), api._p(u), N, N, C, api._p(out)))
    return out


def reciprocal_distance(models, counts, k=0.95, ctx: api.Context | None = None):
    """Reciprocal weighting: x = log10(counts + 1) and, for cells i, j and gene g,
    w = sqrt((1 - f(model_i, fpm[g, j])) (1 - f(model_j, fpm[g, i]))) k + (1 - k) with f
    scde.failure.probability and fpm scde.expression.magnitude."""
    k = _check_k(k)
    mm, sq, dc, mat, N, C = _counts_arg(models, counts)
    out = np.zeros((C, C), order="F")
    h = ctx.handle if ctx else None
    if dc is not None:
        check(lib().scde_reciprocal_corr_dev(h or dc.ctx.handle, dc.ptr, N, N, C, api._p(mm), sq, k, api._p(out)))
    else:
        check(lib().scde_reciprocal_corr_host(h, api._p(mat), N, N, C, api._p(mm), sq, k, api._p(out)))
    return _as_distance(out)


def joint_posterior_modes(jp, prior_x):
    """log(10^prior_x - 1) at each row maximum of the joint posterior.  R's ``max.col`` breaks
    ties at random; here the first maximum wins."""
    with np.errstate(divide="ignore"):
        mag = np.log(10.0 ** np.asarray(prior_x, np.float64) - 1.0)
    return mag[np.argmax(np.asarray(jp), axis=1)]


def mode_relative_distance(models, counts, prior=None, posteriors=None, n_randomizations=100, n_cores=1,
                           ctx: api.Context | None = None):
    """Mode-relative weighting: x = log10(exp(modes) + 1), w = (matw_i matw_j)^(1/4),
    matw = 1 - sqrt(p.self.fail sqrt(p.self.fail p.mode.fail)), p.mode.fail the failure
    probability at the joint posterior's mode.  ``posteriors`` is the result of
    ``scde_posteriors(..., return_individual_posterior_modes=True)`` (``jp`` and ``modes``);
    when absent it is computed here (host counts only).  ``prior`` supplies the grid ``x``."""
    if prior is None:
        raise ValueError("prior (with the grid x) is required")
    mm, sq, dc, mat, N, C = _counts_arg(models, counts)
    if posteriors is None:
        if dc is not None:
            raise ValueError("posteriors must be given with resident counts")
        posteriors = api.scde_posteriors(models, counts, prior, n_randomizations=n_randomizations, n_cores=n_cores,
                                         return_individual_posterior_modes=True, ctx=ctx)
    jp = np.asarray(posteriors["jp"], np.float64)
    modes = np.asfortranarray(posteriors["modes"], dtype=np.float64)
    prior_x = np.asarray(prior["x"], np.float64)
    if modes.shape != (N, C) or jp.shape != (N, len(prior_x)):
        raise ValueError("posteriors do not match the counts and the prior grid")
    jpm = np.ascontiguousarray(joint_posterior_modes(jp, prior_x)) if N else np.zeros(1)
    out = np.zeros((C, C), order="F")
    h = ctx.handle if ctx else None
    if dc is not None:
        check(lib().scde_mode_fail_corr_dev(h or dc.ctx.handle, dc.ptr, N, N, C, api._p(mm), sq, api._p(modes),
                                            api._p(jpm), api._p(out)))
    else:
        check(lib().scde_mode_fail_corr_host(h, api._p(mat), N, N, C, api._p(mm), sq, api._p(modes), api._p(jpm),
                                             api._p(out)))
    return _as_distance(out)


def direct_dropout_distance(models, counts, n_simulations=10, k=0.9, seed=0, uniforms=None,
                            ctx: api.Context | None = None):
    """Direct drop-out: the mean over ``n_simulations`` rounds of the pairwise-complete
    Pearson correlation of log10(counts + 1), entry (g, c) kept in a round with probability
    1 - p.self.fail[g, c] k.  The draws come from ``uniforms`` (n_simulations x cells x genes,
    in [0, 1)) or, when None, from the library's counter-based generator keyed by ``seed``
    (include/scde_hip.h).  A pair that is NaN in any round is NaN."""
    k = _check_k(k)
    nsim = int(n_simulations)
    if nsim < 1:
        raise ValueError("n_simulations must be at least 1")
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise ValueError("seed must be in [0, 2^64)")
    mm, sq, dc, mat, N, C = _counts_arg(models, counts)
    if uniforms is not None:
        uniforms = np.ascontiguousarray(uniforms, dtype=np.float64)
        if uniforms.shape != (nsim, C, N):
            raise ValueError("uniforms must have shape (n_simulations, cells, genes)")
        if uniforms.size == 0:
            uniforms = None
    out = np.zeros((C, C), order="F")
    h = ctx.handle if ctx else None
    if dc is not None:
        check(lib().scde_direct_corr_dev(h or dc.ctx.handle, dc.ptr, N, N, C, api._p(mm), sq, k, nsim,
                                         api._p(uniforms), seed, api._p(out)))
    else:
        check(lib().scde_direct_corr_host(h, api._p(mat), N, N, C, api._p(mm), sq, k, nsim, api._p(uniforms), seed,
                                          api._p(out)))
    return _as_distance(out)
